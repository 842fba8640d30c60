"""The FID InceptionV3 feature extractor on the HIP kernels, frozen, forward only: torch-fidelity's
``pt_inception-2015-12-05`` network, the one ``torchmetrics.image.fid.FrechetInceptionDistance`` wraps, restated from its public
description up to the 2048-d pool feature --

    stem     Conv2d_1a_3x3 3->32 /2, 2a 32->32, 2b 32->64 p1, maxpool 3/2, 3b_1x1 64->80, 4a_3x3 80->192, maxpool 3/2      299 -> 35
    Mixed_5b/5c/5d  InceptionA(192 | 256 | 288; pool_features 32 | 64 | 64)                                               35 x 35
    Mixed_6a        InceptionB(288)                                                                                        35 -> 17
    Mixed_6b..6e    InceptionC(768; c7 = 128 | 160 | 160 | 192)                                                            17 x 17
    Mixed_7a        InceptionD(768)                                                                                        17 -> 8
    Mixed_7b/7c     InceptionE(1280 | 2048), 7b with an average and 7c with a MAX pool branch                              8 x 8
    global average pool -> [B, 2048] fp32

-- every ``BasicConv2d`` being a bias-free convolution, BatchNorm (eps 1e-3, running statistics) and ReLU.  The FID variant differs
from torchvision's ``inception_v3`` in four ways: the average pools of the A, C and 7b blocks take ``count_include_pad=False``, the
pool branch of ``Mixed_7c`` is a max pool, there is no ``transform_input``, and the 1008-way ``fc`` is not part of the 2048-d feature.

``state_dict()`` carries torch-fidelity's names and layouts (``<layer>.conv.weight`` [Cout, Cin, KH, KW], ``<layer>.bn.{weight, bias,
running_mean, running_var}``); what the kernels read is derived from it at load: the batch norm folded into weight and bias in fp64,
the weight tap-major ``[Cout][KH][KW][Cin]`` in the compute dtype, the two 1x1 convolutions that open a block's inner branches stacked
into one operand, the stem's weight ``[32, 27]`` padded to 32 columns.  Every operator is in ``libuwu_hip.so``: ``uwu_inception_stem``
+ ``uwu_conv2d_fwd`` (in bf16 the small 1x1 layers: ``uwu_gemm`` + ``uwu_relu_rows``) + ``uwu_pool2d_fwd`` + ``uwu_global_avgpool``; a branch writes straight into its channel slice of the block's
output, so no concatenation pass exists.  There is no backward and no CPU path.
"""
import hashlib

import torch

from . import lib as L
from . import ops
from .flat import FlatModule, _Config

BN_EPS = 1e-3
IMAGE_SIZE = 299
FEATURES = 2048
WEIGHTS_NAME = "pt_inception-2015-12-05"
# Routing, as measured: a 1x1 convolution's column matrix is the activation itself, and on the 17 x 17 and 8 x 8
# layers (small M, deep K) uwu_gemm + uwu_relu_rows beats the implicit kernel; at 35 x 35 and above the implicit kernel wins.
GEMM_1X1_MAX_PIXELS = 17 * 17


def _block_a(name, cin, pf):
    return [(f"{name}.branch1x1", cin, 64, (1, 1), 1, (0, 0)),
            (f"{name}.branch5x5_1", cin, 48, (1, 1), 1, (0, 0)), (f"{name}.branch5x5_2", 48, 64, (5, 5), 1, (2, 2)),
            (f"{name}.branch3x3dbl_1", cin, 64, (1, 1), 1, (0, 0)), (f"{name}.branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1)),
            (f"{name}.branch3x3dbl_3", 96, 96, (3, 3), 1, (1, 1)), (f"{name}.branch_pool", cin, pf, (1, 1), 1, (0, 0))]


def _block_b(name, cin):
    return [(f"{name}.branch3x3", cin, 384, (3, 3), 2, (0, 0)), (f"{name}.branch3x3dbl_1", cin, 64, (1, 1), 1, (0, 0)),
            (f"{name}.branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1)), (f"{name}.branch3x3dbl_3", 96, 96, (3, 3), 2, (0, 0))]


def _block_c(name, cin, c7):
    h, v = ((1, 7), 1, (0, 3)), ((7, 1), 1, (3, 0))
    return [(f"{name}.branch1x1", cin, 192, (1, 1), 1, (0, 0)),
            (f"{name}.branch7x7_1", cin, c7, (1, 1), 1, (0, 0)), (f"{name}.branch7x7_2", c7, c7, *h), (f"{name}.branch7x7_3", c7, 192, *v),
            (f"{name}.branch7x7dbl_1", cin, c7, (1, 1), 1, (0, 0)), (f"{name}.branch7x7dbl_2", c7, c7, *v),
            (f"{name}.branch7x7dbl_3", c7, c7, *h), (f"{name}.branch7x7dbl_4", c7, c7, *v), (f"{name}.branch7x7dbl_5", c7, 192, *h),
            (f"{name}.branch_pool", cin, 192, (1, 1), 1, (0, 0))]


def _block_d(name, cin):
    return [(f"{name}.branch3x3_1", cin, 192, (1, 1), 1, (0, 0)), (f"{name}.branch3x3_2", 192, 320, (3, 3), 2, (0, 0)),
            (f"{name}.branch7x7x3_1", cin, 192, (1, 1), 1, (0, 0)), (f"{name}.branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3)),
            (f"{name}.branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0)), (f"{name}.branch7x7x3_4", 192, 192, (3, 3), 2, (0, 0))]


def _block_e(name, cin):
    h, v = ((1, 3), 1, (0, 1)), ((3, 1), 1, (1, 0))
    return [(f"{name}.branch1x1", cin, 320, (1, 1), 1, (0, 0)),
            (f"{name}.branch3x3_1", cin, 384, (1, 1), 1, (0, 0)), (f"{name}.branch3x3_2a", 384, 384, *h), (f"{name}.branch3x3_2b", 384, 384, *v),
            (f"{name}.branch3x3dbl_1", cin, 448, (1, 1), 1, (0, 0)), (f"{name}.branch3x3dbl_2", 448, 384, (3, 3), 1, (1, 1)),
            (f"{name}.branch3x3dbl_3a", 384, 384, *h), (f"{name}.branch3x3dbl_3b", 384, 384, *v),
            (f"{name}.branch_pool", cin, 192, (1, 1), 1, (0, 0))]


STEM = [("Conv2d_1a_3x3", 3, 32, (3, 3), 2, (0, 0)), ("Conv2d_2a_3x3", 32, 32, (3, 3), 1, (0, 0)), ("Conv2d_2b_3x3", 32, 64, (3, 3), 1, (1, 1)),
        ("Conv2d_3b_1x1", 64, 80, (1, 1), 1, (0, 0)), ("Conv2d_4a_3x3", 80, 192, (3, 3), 1, (0, 0))]
# block name -> (type, input channels, its one parameter, output channels)
BLOCKS = {"Mixed_5b": ("A", 192, 32, 256), "Mixed_5c": ("A", 256, 64, 288), "Mixed_5d": ("A", 288, 64, 288), "Mixed_6a": ("B", 288, None, 768),
          "Mixed_6b": ("C", 768, 128, 768), "Mixed_6c": ("C", 768, 160, 768), "Mixed_6d": ("C", 768, 160, 768), "Mixed_6e": ("C", 768, 192, 768),
          "Mixed_7a": ("D", 768, None, 1280), "Mixed_7b": ("E", 1280, "avg_s1p1", 2048), "Mixed_7c": ("E", 2048, "max_s1p1", 2048)}
# the two 1x1 convolutions that open a block's inner branches read the same input: one operand, one launch
_STACKED = {"A": ("branch5x5_1", "branch3x3dbl_1"), "C": ("branch7x7_1", "branch7x7dbl_1"), "D": ("branch3x3_1", "branch7x7x3_1"),
            "E": ("branch3x3_1", "branch3x3dbl_1")}


def layer_table():
    """every BasicConv2d: (name, Cin, Cout, (KH, KW), stride, (ph, pw)), in ``state_dict()`` order"""
    out = list(STEM)
    for name, (kind, cin, arg, _) in BLOCKS.items():
        out += {"A": lambda: _block_a(name, cin, arg), "B": lambda: _block_b(name, cin), "C": lambda: _block_c(name, cin, arg),
                "D": lambda: _block_d(name, cin), "E": lambda: _block_e(name, cin)}[kind]()
    return out


def check_image_size(shape, what="FIDInceptionV3"):
    """the extractor takes 299 x 299 pictures only: torch-fidelity's bilinear resize of other sizes is not built"""
    if len(shape) < 3 or tuple(shape[-3:]) != (3, IMAGE_SIZE, IMAGE_SIZE):
        raise NotImplementedError(f"{what}: pictures must be [3, {IMAGE_SIZE}, {IMAGE_SIZE}], got {tuple(shape[-3:])}; the InceptionV3 resize "
                                  f"(torch-fidelity interpolates other sizes to {IMAGE_SIZE} x {IMAGE_SIZE} inside the extractor) is not "
                                  f"built: resize in the dataset transform (torchvision.transforms.Resize with size: {IMAGE_SIZE}, then "
                                  f"torchvision.transforms.CenterCrop with size: {IMAGE_SIZE})")


class FIDInceptionV3(FlatModule):
    """``forward(images) -> features fp32 [B, 2048]``; images uint8 ``[B, 3, 299, 299]``, or floats in [0, 1] under ``normalize=True``
    (``trunc(clamp(x, 0, 1) * 255)``, torchmetrics' ``(imgs * 255).byte()``), then ``(v - 128) / 128``."""

    kind = "fid_inception_v3"

    def __init__(self, compute_dtype="bf16", init_weights=True, device=None, seed=None, chunk=128):
        super().__init__()
        if compute_dtype not in ("bf16", "fp32"):
            raise ValueError(f"FIDInceptionV3: compute_dtype must be 'bf16' or 'fp32', got {compute_dtype!r}")
        self.config = _Config(compute_dtype=compute_dtype, image_size=IMAGE_SIZE, features=FEATURES, bn_eps=BN_EPS)
        self.chunk = int(chunk)  # pictures per pass: bounds the activations however large the batch of an update is
        self.spec = {name: spec for name, *spec in layer_table()}
        for name, (cin, cout, (kh, kw), _, _) in self.spec.items():
            self.P.add(name + ".conv.weight", (cout, cin, kh, kw))
            for n in ("weight", "bias", "running_mean", "running_var"):
                self.P.add(f"{name}.bn.{n}", (cout,))
        self._alloc(compute_dtype == "bf16", device, buffer=True)
        # what the kernels read: op name -> (offset into wf, offset into bf, rows, columns)
        self._ops, nw, nb = {}, 0, 0
        stacked = {f"{blk}.{a}": f"{blk}.{b}" for blk, (kind, *_) in BLOCKS.items() if kind in _STACKED for a, b in [_STACKED[kind]]}
        second = set(stacked.values())
        for name, (cin, cout, (kh, kw), _, _) in self.spec.items():
            if name in second:
                continue
            rows = cout + (self.spec[stacked[name]][1] if name in stacked else 0)
            cols = 32 if name == STEM[0][0] else kh * kw * cin
            self._ops[name] = (nw, nb, rows, cols, (name, stacked[name]) if name in stacked else (name,))
            nw, nb = nw + (rows * cols + 63) // 64 * 64, nb + (rows + 63) // 64 * 64
        self._nw, self._nb = nw, nb
        self.wf = self.bf = None
        if init_weights and self.flat.device.type != "meta":
            self.reset_parameters(seed)
        self.eval().requires_grad_(False)

    dtype = property(lambda self: self.P.dtype)

    # ------------------------------------------------------------------ parameters
    def _wants_shadow(self):
        return False  # the operands are the folded tensors below, not a cast of the stored ones

    def _load_key(self, key):
        """torch-fidelity's checkpoint also holds the 1008-way ``fc`` and BatchNorm's step counters: neither is part of the feature"""
        if key.startswith("fc.") or key.endswith(".num_batches_tracked"):
            return None
        return key

    def _after_load(self):
        self._fold()

    def _moved(self):
        self._fold()

    @torch.no_grad()
    def _fold(self):
        """BatchNorm folded into the convolution in fp64:  w' = w gamma / sqrt(var + eps),  b' = beta - mean gamma / sqrt(var + eps);
        w' stored tap-major in the compute dtype, b' in fp32"""
        dev = self.flat.device
        if dev.type == "meta":
            return
        wf = torch.zeros(self._nw, dtype=self.dtype, device=dev)
        bf = torch.zeros(self._nb, dtype=torch.float32, device=dev)
        for ow, ob, rows, cols, names in self._ops.values():
            ws, bs = [], []
            for name in names:
                scale = self.view(name + ".bn.weight").double() / (self.view(name + ".bn.running_var").double() + BN_EPS).sqrt()
                w = self.view(name + ".conv.weight").double() * scale[:, None, None, None]
                if name == STEM[0][0]:  # [32, 3, 3, 3] -> [32, 27] as it is (the operand's columns are (c, ky, kx)), padded to 32
                    w = torch.cat([w.flatten(1), w.new_zeros(w.shape[0], 5)], 1)
                else:
                    w = w.permute(0, 2, 3, 1).flatten(1)
                ws.append(w)
                bs.append(self.view(name + ".bn.bias").double() - self.view(name + ".bn.running_mean").double() * scale)
            wf[ow:ow + rows * cols].copy_(torch.cat(ws).flatten())
            bf[ob:ob + rows].copy_(torch.cat(bs))
        self.wf, self.bf = wf, bf

    @torch.no_grad()
    def reset_parameters(self, seed=None):
        """The checkpoint cannot be fetched, so the weights are drawn: convolutions N(0, 2 / fan_in) (He: a ReLU layer then keeps the
        rms of its input), BatchNorm at the identity (weight 1, bias 0, mean 0, variance 1), tensor by tensor on the CPU from `seed`
        (default: a seed made of the checkpoint's name), so every layer's output rms stays within [0.1, 10] on pictures."""
        if seed is None:
            seed = int.from_bytes(hashlib.md5(WEIGHTS_NAME.encode()).digest()[:4], "little")
        g = torch.Generator().manual_seed(seed % (2 ** 31))
        for name, v in self.named_tensors():
            if name.endswith("conv.weight"):
                v.copy_(torch.randn(v.shape, generator=g) * (2.0 / (v.shape[1] * v.shape[2] * v.shape[3])) ** 0.5)
            elif name.endswith(("bn.weight", "bn.running_var")):
                v.fill_(1.0)
            else:
                v.zero_()
        self._fold()

    # ------------------------------------------------------------------ forward
    def _conv(self, name, x, B, H, W, xoff=0, out=None, yoff=0):
        """the op `name` (a BasicConv2d, or two stacked 1x1) on channels xoff.. of x -> channels yoff.. of out"""
        ow, ob, rows, cols, names = self._ops[name]
        cin, _, k, s, p = self.spec[name]
        if name == STEM[0][0]:  # the operand kernel has already gathered the 27 taps: a 1x1 convolution over 32 columns
            cin, k, s, p = 32, (1, 1), 1, (0, 0)
        elif k == (1, 1) and H * W <= GEMM_1X1_MAX_PIXELS and self.P.bf16:
            return ops.conv1x1_gemm_fwd(x, self.wf[ow:ow + rows * cols].view(rows, cols), self.bf[ob:ob + rows], cin, rows, relu=True,
                                        xoff=xoff, out=out, yoff=yoff)
        return ops.conv2d_fwd(x, self.wf[ow:ow + rows * cols].view(rows, cols), self.bf[ob:ob + rows], B, H, W, cin, rows, k, s, p, relu=True,
                              xoff=xoff, out=out, yoff=yoff)

    def _chain(self, prefix, names, x, B, H, W, xoff, out, yoff):
        """convolutions one after another, the first reading channels xoff.. of x, the last writing channels yoff.. of out"""
        for i, n in enumerate(names):
            last = i == len(names) - 1
            x = self._conv(f"{prefix}.{n}", x, B, H, W, xoff=xoff if i == 0 else 0, out=out if last else None, yoff=yoff if last else 0)
            if self.spec[f"{prefix}.{n}"][3] == 2:
                H, W = ops.conv2d_out_hw(H, W, 3, 2, 0)
        return x

    def block(self, name, x, B, H, W):
        """one Mixed_* block on x [B*H*W, Cin] -> (y [B*Ho*Wo, Cout], Ho, Wo)"""
        kind, cin, arg, cout = BLOCKS[name]
        Ho, Wo = ops.conv2d_out_hw(H, W, 3, 2, 0) if kind in "BD" else (H, W)
        y = torch.empty(B * Ho * Wo, cout, device=x.device, dtype=x.dtype)
        c = lambda n, *a, **k: self._conv(f"{name}.{n}", *a, **k)  # noqa: E731
        if kind == "A":
            c("branch1x1", x, B, H, W, out=y)
            t = c("branch5x5_1", x, B, H, W)  # [M, 48 + 64]
            c("branch5x5_2", t, B, H, W, out=y, yoff=64)
            self._chain(name, ["branch3x3dbl_2", "branch3x3dbl_3"], t, B, H, W, 48, y, 128)
            c("branch_pool", ops.pool2d_fwd(x, B, H, W, cin, "avg_s1p1"), B, H, W, out=y, yoff=224)
        elif kind == "B":
            c("branch3x3", x, B, H, W, out=y)
            self._chain(name, ["branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"], x, B, H, W, 0, y, 384)
            ops.pool2d_fwd(x, B, H, W, cin, "max_s2", out=y, yoff=480)
        elif kind == "C":
            c("branch1x1", x, B, H, W, out=y)
            t = c("branch7x7_1", x, B, H, W)  # [M, 2 c7]
            self._chain(name, ["branch7x7_2", "branch7x7_3"], t, B, H, W, 0, y, 192)
            self._chain(name, ["branch7x7dbl_2", "branch7x7dbl_3", "branch7x7dbl_4", "branch7x7dbl_5"], t, B, H, W, arg, y, 384)
            c("branch_pool", ops.pool2d_fwd(x, B, H, W, cin, "avg_s1p1"), B, H, W, out=y, yoff=576)
        elif kind == "D":
            t = c("branch3x3_1", x, B, H, W)  # [M, 192 + 192]
            c("branch3x3_2", t, B, H, W, out=y)
            self._chain(name, ["branch7x7x3_2", "branch7x7x3_3", "branch7x7x3_4"], t, B, H, W, 192, y, 320)
            ops.pool2d_fwd(x, B, H, W, cin, "max_s2", out=y, yoff=512)
        else:
            c("branch1x1", x, B, H, W, out=y)
            t = c("branch3x3_1", x, B, H, W)  # [M, 384 + 448]
            c("branch3x3_2a", t, B, H, W, out=y, yoff=320)
            c("branch3x3_2b", t, B, H, W, out=y, yoff=704)
            u = c("branch3x3dbl_2", t, B, H, W, xoff=384)
            c("branch3x3dbl_3a", u, B, H, W, out=y, yoff=1088)
            c("branch3x3dbl_3b", u, B, H, W, out=y, yoff=1472)
            c("branch_pool", ops.pool2d_fwd(x, B, H, W, cin, arg), B, H, W, out=y, yoff=1856)
        return y, Ho, Wo

    def _require_device(self, images):
        if not torch.is_tensor(images) or not images.is_cuda or not self.flat.is_cuda:
            raise L.UwuError("FIDInceptionV3.forward runs on the HIP device only (no CPU fallback): move the model and the pictures there")

    def check_images(self, images, normalize):
        """the input rule, asked before anything runs: uint8 as it is, a float only under normalize=True, 299 x 299 only"""
        if not torch.is_tensor(images) or images.dim() != 4:
            raise TypeError("FIDInceptionV3: images must be a [B, 3, 299, 299] tensor")
        check_image_size(images.shape)
        if images.dtype != torch.uint8 and not (normalize and images.is_floating_point()):
            raise ValueError(f"FIDInceptionV3: images must be uint8 in [0, 255], or floats in [0, 1] under normalize=True; got {images.dtype} "
                             f"with normalize={bool(normalize)}")

    @torch.no_grad()
    def _features(self, images, upto=None):
        """one chunk.  `upto`: stop after that layer or block and return its output (rows, H, W) -- what the tests compare"""
        B = images.shape[0]
        x, H, W = ops.inception_stem(images, self.dtype), 149, 149
        steps = [("Conv2d_1a_3x3", None), ("Conv2d_2a_3x3", None), ("Conv2d_2b_3x3", None), ("maxpool1", 64), ("Conv2d_3b_1x1", None),
                 ("Conv2d_4a_3x3", None), ("maxpool2", 192)] + [(b, "block") for b in BLOCKS]
        for name, arg in steps:
            if arg == "block":
                x, H, W = self.block(name, x, B, H, W)
            elif arg is not None:
                x = ops.pool2d_fwd(x, B, H, W, arg, "max_s2")
                H, W = ops.conv2d_out_hw(H, W, 3, 2, 0)
            else:
                x = self._conv(name, x, B, H, W)
                if name != STEM[0][0]:
                    _, _, k, s, p = self.spec[name]
                    H, W = ops.conv2d_out_hw(H, W, k, s, p)
            if name == upto:
                return x, H, W
        return ops.global_avgpool(x, B, H * W, FEATURES)

    @torch.no_grad()
    def forward(self, images, normalize=False):
        self.check_images(images, normalize)
        self._require_device(images)
        if images.dtype != torch.uint8:
            images = images.float()
        images = images.contiguous()
        return torch.cat([self._features(images[i:i + self.chunk]) for i in range(0, images.shape[0], self.chunk)])
