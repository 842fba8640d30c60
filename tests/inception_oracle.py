"""Plain-torch restatement of the FID InceptionV3 (torch-fidelity's ``pt_inception-2015-12-05``, 2048-d pool feature) and of the FID
formula, for the tests of ``uwudiff_amd.inception`` / ``uwudiff_amd.metrics``: ``F.conv2d``, unfused ``F.batch_norm``, ``F.avg_pool2d(
count_include_pad=False)``, float64, torch-fidelity's state-dict names.  Nothing of the product is imported.

Two modes.  "fp64": the network as stated.  "bf16" (the CPU-bf16 model of the device's arithmetic): the batch norm folded into weight
and bias in fp64, the weights and the input rounded to bf16, fp32 arithmetic, every layer's and every pool's output rounded to bf16;
its distance from "fp64" is what bf16 storage costs, the yardstick the device's bf16 results are held to.
"""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-3


def _a(n, cin, pf):
    return [(n + ".branch1x1", cin, 64, (1, 1), 1, (0, 0)), (n + ".branch5x5_1", cin, 48, (1, 1), 1, (0, 0)),
            (n + ".branch5x5_2", 48, 64, (5, 5), 1, (2, 2)), (n + ".branch3x3dbl_1", cin, 64, (1, 1), 1, (0, 0)),
            (n + ".branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1)), (n + ".branch3x3dbl_3", 96, 96, (3, 3), 1, (1, 1)),
            (n + ".branch_pool", cin, pf, (1, 1), 1, (0, 0))]


def _b(n, cin):
    return [(n + ".branch3x3", cin, 384, (3, 3), 2, (0, 0)), (n + ".branch3x3dbl_1", cin, 64, (1, 1), 1, (0, 0)),
            (n + ".branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1)), (n + ".branch3x3dbl_3", 96, 96, (3, 3), 2, (0, 0))]


def _c(n, cin, c7):
    return ([(n + ".branch1x1", cin, 192, (1, 1), 1, (0, 0)), (n + ".branch7x7_1", cin, c7, (1, 1), 1, (0, 0)),
             (n + ".branch7x7_2", c7, c7, (1, 7), 1, (0, 3)), (n + ".branch7x7_3", c7, 192, (7, 1), 1, (3, 0)),
             (n + ".branch7x7dbl_1", cin, c7, (1, 1), 1, (0, 0)), (n + ".branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0)),
             (n + ".branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3)), (n + ".branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0)),
             (n + ".branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3)), (n + ".branch_pool", cin, 192, (1, 1), 1, (0, 0))])


def _d(n, cin):
    return [(n + ".branch3x3_1", cin, 192, (1, 1), 1, (0, 0)), (n + ".branch3x3_2", 192, 320, (3, 3), 2, (0, 0)),
            (n + ".branch7x7x3_1", cin, 192, (1, 1), 1, (0, 0)), (n + ".branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3)),
            (n + ".branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0)), (n + ".branch7x7x3_4", 192, 192, (3, 3), 2, (0, 0))]


def _e(n, cin):
    return [(n + ".branch1x1", cin, 320, (1, 1), 1, (0, 0)), (n + ".branch3x3_1", cin, 384, (1, 1), 1, (0, 0)),
            (n + ".branch3x3_2a", 384, 384, (1, 3), 1, (0, 1)), (n + ".branch3x3_2b", 384, 384, (3, 1), 1, (1, 0)),
            (n + ".branch3x3dbl_1", cin, 448, (1, 1), 1, (0, 0)), (n + ".branch3x3dbl_2", 448, 384, (3, 3), 1, (1, 1)),
            (n + ".branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1)), (n + ".branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0)),
            (n + ".branch_pool", cin, 192, (1, 1), 1, (0, 0))]


# block -> (type, input channels, parameter, output channels, input height = width)
BLOCKS = {"Mixed_5b": ("A", 192, 32, 256, 35), "Mixed_5c": ("A", 256, 64, 288, 35), "Mixed_5d": ("A", 288, 64, 288, 35),
          "Mixed_6a": ("B", 288, None, 768, 35), "Mixed_6b": ("C", 768, 128, 768, 17), "Mixed_6c": ("C", 768, 160, 768, 17),
          "Mixed_6d": ("C", 768, 160, 768, 17), "Mixed_6e": ("C", 768, 192, 768, 17), "Mixed_7a": ("D", 768, None, 1280, 17),
          "Mixed_7b": ("E", 1280, "avg", 2048, 8), "Mixed_7c": ("E", 2048, "max", 2048, 8)}
STEM = [("Conv2d_1a_3x3", 3, 32, (3, 3), 2, (0, 0)), ("Conv2d_2a_3x3", 32, 32, (3, 3), 1, (0, 0)), ("Conv2d_2b_3x3", 32, 64, (3, 3), 1, (1, 1)),
        ("Conv2d_3b_1x1", 64, 80, (1, 1), 1, (0, 0)), ("Conv2d_4a_3x3", 80, 192, (3, 3), 1, (0, 0))]


def layers():
    """(name, Cin, Cout, kernel, stride, padding) of the 94 BasicConv2d"""
    out = list(STEM)
    for n, (kind, cin, arg, _, _) in BLOCKS.items():
        out += {"A": _a, "B": _b, "C": _c, "D": _d, "E": _e}[kind](*((n, cin) if kind in "BDE" else (n, cin, arg)))
    return out


LAYERS = {n: spec for n, *spec in layers()}


def random_state_dict(seed, with_fc=False):
    """torch-fidelity's names; He-scaled convolutions and non-trivial BatchNorm statistics (the fold must use all four vectors)"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for n, (cin, cout, (kh, kw), _, _) in LAYERS.items():
        sd[n + ".conv.weight"] = torch.randn(cout, cin, kh, kw, generator=g) * (2.0 / (cin * kh * kw)) ** 0.5
        sd[n + ".bn.weight"] = 0.8 + 0.4 * torch.rand(cout, generator=g)
        sd[n + ".bn.bias"] = 0.1 * torch.randn(cout, generator=g)
        sd[n + ".bn.running_mean"] = 0.1 * torch.randn(cout, generator=g)
        sd[n + ".bn.running_var"] = 0.6 + 0.8 * torch.rand(cout, generator=g)
        if with_fc:
            sd[n + ".bn.num_batches_tracked"] = torch.tensor(7)
    if with_fc:
        sd["fc.weight"], sd["fc.bias"] = torch.randn(1008, 2048, generator=g) * 0.01, torch.zeros(1008)
    return sd


def pictures(n, seed, size=299):
    """structured uint8 pictures [n, 3, size, size]: smooth colour fields, a few rectangles, a little noise (low-frequency content, as
    tools/make_demo_folder.py draws; white noise would make every picture the same to a convolution)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64) / size
    out = np.empty((n, 3, size, size))
    for i in range(n):
        for c in range(3):
            fx, fy, ph = rng.uniform(0.5, 4.0), rng.uniform(0.5, 4.0), rng.uniform(0, 6.28)
            out[i, c] = 127.5 + 100.0 * np.sin(6.28 * (fx * xx + fy * yy) + ph)
        for _ in range(int(rng.integers(2, 6))):
            x0, y0 = int(rng.integers(0, size)), int(rng.integers(0, size))
            x1, y1 = x0 + int(rng.integers(4, size // 3)), y0 + int(rng.integers(4, size // 3))
            out[i, :, y0:y1, x0:x1] = rng.integers(0, 256, 3)[:, None, None]
        out[i] += rng.normal(0.0, 6.0, out[i].shape)
    return torch.from_numpy(np.clip(out, 0, 255).astype(np.uint8))


def preprocess(images, normalize=False):
    """uint8 as it is; a float in [0, 1] under normalize -> trunc(clamp(x, 0, 1) * 255) with the product in fp32; then (v - 128) / 128"""
    if images.dtype == torch.uint8:
        v = images.double()
    else:
        assert normalize, "a float needs normalize=True"
        v = (images.float().clamp(0, 1) * 255).trunc().double()
    return (v - 128) / 128


def _round(x, mode):
    return x.bfloat16().float() if mode == "bf16" else x


def basic_conv(sd, name, x, mode="fp64"):
    _, _, _, stride, pad = LAYERS[name]
    w, g, b, m, v = (sd[name + s].double() for s in (".conv.weight", ".bn.weight", ".bn.bias", ".bn.running_mean", ".bn.running_var"))
    if mode == "fp64":
        return F.relu(F.batch_norm(F.conv2d(x, w, None, stride, pad), m, v, g, b, False, 0.0, EPS))
    scale = g / (v + EPS).sqrt()
    wf, bf = (w * scale[:, None, None, None]).bfloat16().float(), (b - m * scale).float()
    return _round(F.relu(F.conv2d(x, wf, bf, stride, pad)), mode)


def block(sd, name, x, mode="fp64"):
    kind, _, arg, _, _ = BLOCKS[name]
    c = lambda n, t: basic_conv(sd, f"{name}.{n}", t, mode)  # noqa: E731
    avg = lambda t: _round(F.avg_pool2d(t, 3, 1, 1, count_include_pad=False), mode)  # noqa: E731
    if kind == "A":
        return torch.cat([c("branch1x1", x), c("branch5x5_2", c("branch5x5_1", x)),
                          c("branch3x3dbl_3", c("branch3x3dbl_2", c("branch3x3dbl_1", x))), c("branch_pool", avg(x))], 1)
    if kind == "B":
        return torch.cat([c("branch3x3", x), c("branch3x3dbl_3", c("branch3x3dbl_2", c("branch3x3dbl_1", x))), F.max_pool2d(x, 3, 2)], 1)
    if kind == "C":
        d = x
        for i in range(1, 6):
            d = c(f"branch7x7dbl_{i}", d)
        return torch.cat([c("branch1x1", x), c("branch7x7_3", c("branch7x7_2", c("branch7x7_1", x))), d, c("branch_pool", avg(x))], 1)
    if kind == "D":
        s = x
        for i in range(1, 5):
            s = c(f"branch7x7x3_{i}", s)
        return torch.cat([c("branch3x3_2", c("branch3x3_1", x)), s, F.max_pool2d(x, 3, 2)], 1)
    t = c("branch3x3_1", x)
    u = c("branch3x3dbl_2", c("branch3x3dbl_1", x))
    pooled = avg(x) if arg == "avg" else F.max_pool2d(x, 3, 1, 1)
    return torch.cat([c("branch1x1", x), c("branch3x3_2a", t), c("branch3x3_2b", t), c("branch3x3dbl_3a", u), c("branch3x3dbl_3b", u),
                      c("branch_pool", pooled)], 1)


@torch.no_grad()
def forward(sd, x, mode="fp64", rms=None):
    """x: the preprocessed pictures [B, 3, 299, 299] -> features [B, 2048] (float64).  `rms`: a dict that receives every layer's and
    block's output rms."""
    x = _round(x.float(), mode) if mode == "bf16" else x.double()

    def note(name, t):
        if rms is not None:
            rms[name] = float(t.double().square().mean().sqrt())
        return t

    for name in ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3"):
        x = note(name, basic_conv(sd, name, x, mode))
    x = F.max_pool2d(x, 3, 2)
    for name in ("Conv2d_3b_1x1", "Conv2d_4a_3x3"):
        x = note(name, basic_conv(sd, name, x, mode))
    x = F.max_pool2d(x, 3, 2)
    for name in BLOCKS:
        x = note(name, block(sd, name, x, mode))
    return x.float().mean((2, 3)).double() if mode == "bf16" else x.mean((2, 3))


def forward_batched(sd, x, mode="fp64", batch=3):
    return torch.cat([forward(sd, x[i:i + batch], mode) for i in range(0, x.shape[0], batch)])


def moments(features):
    """(mean, unbiased covariance) of features [n, D], float64"""
    f = features.double()
    mu = f.mean(0)
    d = f - mu
    return mu, d.T @ d / (f.shape[0] - 1)


def fid(mu1, s1, mu2, s2):
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 sum sqrt(eigvals(S1 S2)).real"""
    ev = np.linalg.eigvals((s1.double() @ s2.double()).numpy())
    return float((mu1 - mu2).double().square().sum() + s1.double().trace() + s2.double().trace() - 2 * np.sqrt(ev.astype(complex)).real.sum())


def fid_of_features(real, fake):
    """``fid(*moments(real), *moments(fake))`` for n << D without a D x D eigenproblem: with S1 = A^T A and S2 = B^T B (A, B the centred
    features over sqrt(n - 1)) the non-zero eigenvalues of S1 S2 are those of (A B^T)(A B^T)^T, so the sum of their square roots is
    the sum of the singular values of A B^T; the traces are the squared Frobenius norms"""
    r, f = real.double(), fake.double()
    mu1, mu2 = r.mean(0), f.mean(0)
    a, b = (r - mu1) / (r.shape[0] - 1) ** 0.5, (f - mu2) / (f.shape[0] - 1) ** 0.5
    return float((mu1 - mu2).square().sum() + a.square().sum() + b.square().sum() - 2 * torch.linalg.svdvals(a @ b.T).sum())


def rel_l2(got, ref):
    """per-picture relative L2 error: [B]"""
    got, ref = got.double().flatten(1), ref.double().flatten(1)
    return (got - ref).norm(dim=1) / ref.norm(dim=1)
