"""Fused flat-buffer optimizers + global-norm clip on the HIP kernels (csrc/optimizer*.hip).

``FusedAdamW`` mirrors ``torch.optim.AdamW`` single-tensor semantics (the reference instantiates ``torch.optim.AdamW`` from
YAML, reference src/duwu/trainer/trainer.py:52-74, configs/demo_training_latent.yaml:30-39), ``FusedLion`` is
``lion_pytorch.Lion`` (the commented alternative of the reference's training YAMLs) and ``FusedAdamWFP16`` the reference's own
``duwu.trainer.optimizers.AdamWFP16`` (src/duwu/trainer/optimizers.py); ``FusedProdigy`` is ``prodigyopt.Prodigy``, whose step
size comes from two sums over all parameters kept on the device; ``FusedAdamW8bit`` / ``FusedLion8bit`` keep the moments as 8-bit
codes with one scale per block of 256 elements (the state layout of ``bitsandbytes.optim.AdamW8bit`` / ``Lion8bit``);
``FusedAdamWScheduleFree`` is ``schedulefree.AdamWScheduleFree``, whose trained weights ``y`` are not the weights ``x`` to evaluate
(its docstring states the rule; ``eval()`` / ``train()`` put one in place of the other); ``FusedAdafactor`` is
``transformers.optimization.Adafactor``, whose rule is per tensor (row and column second moments): it walks a device table of the
tensors the flat buffer holds.
``FlatFusedOptimizer`` is what they share and what
the trainer's fused path asks for: Lightning's ``gradient_clip_val`` (global L2 norm, demo_training.yaml:12) as a device
coefficient, one launch per flat parameter buffer (or per reduced chunk of it), the consumed gradient zeroed and the bf16
shadow of the parameters (MFMA operands) refreshed by the same kernel.
"""
import bisect
import ctypes
import math

import torch
import torch.distributed as dist

from . import lib as L


def _zeros_like(t, dtype=None):
    """torch.zeros_like for the flat buffers; on the HIP device the fill is the library's (hipMemsetAsync on the current stream)."""
    if not (t.is_cuda and t.is_contiguous()):
        return torch.zeros_like(t, dtype=dtype)
    z = torch.empty_like(t, dtype=dtype)
    L.call("uwu_memset_zero", L.ptr(z), z.numel() * z.element_size(), L.stream())
    return z


def _shadow_of(p):
    """the bf16 shadow the kernels refresh along with ``p``: the one attached to it, if it covers the whole buffer"""
    shadow = getattr(p, "_uwu_bf16_shadow", None)
    return shadow if shadow is not None and shadow.numel() == p.numel() else None


class FlatFusedOptimizer(torch.optim.Optimizer):
    """Base of the optimizers that update a flat fp32 parameter buffer with one HIP kernel.  A subclass gives the state
    (``_init_state``) and the launch over one sub-range (``_launch``); ``_finish`` runs once per parameter after the
    launches of all chunks."""

    STATE_DTYPES = {}  # state key -> the dtype it is kept in, where that is not the parameter's

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._norm_ws = {}
        self.register_load_state_dict_post_hook(FlatFusedOptimizer._restore_state_dtypes)

    def _restore_state_dtypes(self):
        """torch's ``load_state_dict`` casts every floating-point or integer state tensor of a floating-point parameter to the
        parameter's dtype: fp16 moments and uint8 codes arrive as fp32 holding the same values, so the way back is lossless"""
        for st in self.state.values():
            for k, dtype in self.STATE_DTYPES.items():
                if k in st and st[k].dtype != dtype:
                    st[k] = st[k].to(dtype)

    def _ws(self, device):
        w = self._norm_ws.get(device)
        if w is None:
            w = (torch.empty(1024, device=device, dtype=torch.float32), torch.ones(2, device=device, dtype=torch.float32))
            self._norm_ws[device] = w
        return w

    @torch.no_grad()
    def grad_norm_clip(self, max_norm, pre_scale=1.0):
        """Launches the global-norm reduction; returns the device tensor [sumsq, clip_coef] (no host sync).
        Only single-buffer models (one flat parameter) are clipped in one launch."""
        ps = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
        if len(ps) != 1:
            raise NotImplementedError("grad_norm_clip expects one flat parameter buffer")
        p = ps[0]
        part, out = self._ws(p.device)
        L.call("uwu_grad_sqnorm_clip", L.ptr(p.grad), p.numel(), float(pre_scale), float(max_norm or 0.0), L.ptr(part),
               L.ptr(out), L.stream())
        return out

    def _init_state(self, p, st):
        raise NotImplementedError

    def _launch(self, group, st, p_ptr, g_ptr, shadow_ptr, off, ln, pre_scale, clip_ptr, zero_grad):
        raise NotImplementedError

    def _finish(self, group, p, st, shadow):
        pass

    @torch.no_grad()
    def step(self, closure=None, clip=None, pre_scale=1.0, chunks=None, before_chunk=None, zero_grad=False):
        """One update.  ``chunks`` = [(offset, length), ...] splits the launch over sub-ranges of the flat
        buffer (16-byte aligned offsets); ``before_chunk(i)`` is called first (waits for chunk i's all-reduce).
        ``zero_grad``: the kernel leaves the consumed gradient zeroed (the flat gradient buffer is accumulated into by the
        next backward: no separate fill launch; ``p.grad`` stays allocated -- the ``zero_grad(set_to_none=False)`` state)."""
        loss = closure() if closure is not None else None
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                p_ptr, g_ptr = L.ptr(p.data), L.ptr(p.grad)  # (a CPU parameter is refused here: there is no CPU path)
                st = self.state[p]
                if not st:
                    self._init_state(p, st)
                if "step" in st:
                    st["step"] += 1
                shadow = _shadow_of(p)
                clip_ptr = L.ptr(clip) if clip is not None else None
                for i, (off, ln) in enumerate(chunks or [(0, p.numel())]):
                    if before_chunk is not None:
                        before_chunk(i)
                    sp = shadow.data_ptr() + 2 * off if shadow is not None else None
                    self._launch(group, st, p_ptr + 4 * off, g_ptr + 4 * off, sp, off, ln, float(pre_scale), clip_ptr,
                                 int(bool(zero_grad)))
                self._finish(group, p, st, shadow)
        return loss


class FusedAdamW(FlatFusedOptimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)

    def _init_state(self, p, st):
        st["step"] = 0
        st["exp_avg"] = _zeros_like(p.data)
        st["exp_avg_sq"] = _zeros_like(p.data)

    def _launch(self, group, st, p_ptr, g_ptr, shadow_ptr, off, ln, pre_scale, clip_ptr, zero_grad):
        b1, b2 = group["betas"]
        L.call("uwu_adamw_step", p_ptr, g_ptr, st["exp_avg"].data_ptr() + 4 * off, st["exp_avg_sq"].data_ptr() + 4 * off,
               shadow_ptr, ln, float(group["lr"]), b1, b2, group["eps"], group["weight_decay"], st["step"], pre_scale,
               clip_ptr, zero_grad, L.stream())


class FusedLion(FlatFusedOptimizer):
    """``lion_pytorch.Lion`` (Chen et al. 2023) on a flat buffer: one fp32 moment, the update is ``lr * sign(...)``.
    ``use_triton`` is accepted for the package's signature and ignored (the kernel is HIP either way)."""

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.99), weight_decay=0.0, use_triton=False,
                 decoupled_weight_decay=False):
        if not lr > 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not all(0.0 <= b <= 1.0 for b in betas):
            raise ValueError(f"Invalid beta parameters: {betas}")
        if decoupled_weight_decay:
            raise NotImplementedError("FusedLion: decoupled_weight_decay is not implemented")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), weight_decay=weight_decay))

    def _init_state(self, p, st):
        st["exp_avg"] = _zeros_like(p.data)

    def _launch(self, group, st, p_ptr, g_ptr, shadow_ptr, off, ln, pre_scale, clip_ptr, zero_grad):
        b1, b2 = group["betas"]
        L.call("uwu_lion_step", p_ptr, g_ptr, st["exp_avg"].data_ptr() + 4 * off, shadow_ptr, ln, float(group["lr"]),
               b1, b2, group["weight_decay"], pre_scale, clip_ptr, zero_grad, L.stream())


def draw_decay_phases(n, threshold):
    """AdamWFP16's starting points of the accumulated weight decay (reference optimizers.py:64-66): one
    ``float(torch.rand([]) * threshold)`` per tensor, in order, from torch's global CPU generator.  The reference draws them
    per rank; here rank 0's draws are broadcast when a process group is initialised, so that data-parallel replicas decay
    on the same steps.  Host only: needs no GPU."""
    phases = [float(torch.rand([]) * threshold) for _ in range(n)]
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        box = [phases]
        dist.broadcast_object_list(box, src=0)
        phases = [float(x) for x in box[0]]
    return phases


def flat_segments(module):
    """[(offset, length), ...] of the tensors a flat-buffer module (``FlatModule``, ``LycorisNetwork``) keeps in ``flat``"""
    layout = module.offsets if hasattr(module, "offsets") else module.P.registry
    return [(off, math.prod(shape)) for off, shape in layout.values()]


class FusedAdamWFP16(FlatFusedOptimizer):
    """The reference's ``duwu.trainer.optimizers.AdamWFP16`` on a flat buffer: both moments in fp16, no first-moment bias
    correction, weight decay accumulated per tensor and applied when it crosses ``decay_threshold``.

    ``segments`` = [(offset, length), ...]: the tensors of the flat buffer, each with a decay phase of its own (the reference
    keeps one per parameter tensor); without it the whole buffer is one segment.  ``accumulated_decay`` is a list of python
    floats (a tensor in optimizer state would be cast to the parameter's dtype and device by ``load_state_dict``)."""

    decay_threshold = 1e-2
    STATE_DTYPES = {"exp_avg": torch.float16, "exp_avg_sq": torch.float16}

    def __init__(self, params, *, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, differentiable=False,
                 segments=None):
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if differentiable:
            raise NotImplementedError("FusedAdamWFP16: differentiable=True is not implemented")
        super().__init__(params, dict(betas=tuple(betas), eps=eps, weight_decay=weight_decay, lr=lr,
                                      differentiable=differentiable))
        self.segments = [(int(o), int(n)) for o, n in segments] if segments is not None else None
        if self.segments is not None and sum(len(g["params"]) for g in self.param_groups) != 1:
            raise ValueError("segments describe one flat parameter buffer")

    def _segments_of(self, p):
        segs = self.segments if self.segments is not None else [(0, p.numel())]
        if any(o < 0 or n <= 0 or o + n > p.numel() for o, n in segs):
            raise ValueError("segments reach outside the parameter buffer")
        return segs

    def _init_state(self, p, st):
        st["step"] = 0
        st["exp_avg"] = _zeros_like(p.data, dtype=torch.float16)
        st["exp_avg_sq"] = _zeros_like(p.data, dtype=torch.float16)
        st["accumulated_decay"] = draw_decay_phases(len(self._segments_of(p)), self.decay_threshold)

    def _launch(self, group, st, p_ptr, g_ptr, shadow_ptr, off, ln, pre_scale, clip_ptr, zero_grad):
        b1, b2 = group["betas"]
        L.call("uwu_adamw_fp16_step", p_ptr, g_ptr, st["exp_avg"].data_ptr() + 2 * off,
               st["exp_avg_sq"].data_ptr() + 2 * off, shadow_ptr, ln, float(group["lr"]), b1, b2, group["eps"], st["step"],
               pre_scale, clip_ptr, zero_grad, L.stream())

    def _finish(self, group, p, st, shadow):
        # optimizers.py:71-76 per tensor; the decay launches follow the step launches of all chunks on the same stream
        acc = st["accumulated_decay"]
        segs = self._segments_of(p)
        if len(acc) != len(segs):
            raise ValueError(f"accumulated_decay has {len(acc)} entries, the buffer has {len(segs)} segments")
        for i, (off, ln) in enumerate(segs):
            acc[i] += group["weight_decay"] * float(group["lr"])
            if acc[i] > self.decay_threshold:
                sp = shadow.data_ptr() + 2 * off if shadow is not None else None
                L.call("uwu_param_decay", p.data_ptr() + 4 * off, sp, ln, 1.0 - acc[i], L.stream())
                acc[i] -= acc[i]


class FusedProdigy(FlatFusedOptimizer):
    """``prodigyopt.Prodigy`` (Mishchenko & Defazio, "Prodigy: An Expeditiously Adaptive Parameter-Free Learner") on a flat
    buffer: Adam whose step size ``d`` is estimated from two sums over all parameters, ``sum g.(p0 - p)`` and ``sum |s|``.  The rule
    is written out at ``uwu_prodigy_stats`` (include/uwu_hip.h).  The package reads both sums back with an ``.item()`` per parameter
    tensor; here a step is ``uwu_prodigy_stats`` per chunk (``_launch``: the moments and one partial of each sum per workgroup, still
    behind ``before_chunk`` and so overlapped with the gradient exchange), then ``uwu_prodigy_finalize`` (one workgroup: the sums in
    slot order and the scalar recurrence) and ``uwu_prodigy_apply`` over the whole buffer (``_finish``).  Nothing is read back.

    State per parameter: ``exp_avg``, ``exp_avg_sq``, ``s``, ``p0`` (the parameters at the first step) and ``scalars``, the device
    block ``SCALARS`` names.  The block holds doubles and is kept as their fp32 words: ``load_state_dict`` casts every state tensor
    to the parameter's dtype, which leaves fp32 words bit for bit and would round a float64 tensor.  ``state_dict()`` and the
    checkpoint path carry it like any moment: 16 B of state per parameter.

    One flat parameter buffer (``d`` is one number for all parameters; several buffers would need their sums added: not built), one
    ``lr``.  ``fsdp_in_use`` is accepted for the package's signature and ignored; ``slice_p`` is not implemented.

    World > 1: every rank holds the same reduced gradient and the same parameters, so with the same chunking every rank adds the
    same partials in the same order and ``d`` is bit-identical on all of them: no extra collective."""

    SCALARS = ("d", "d_max", "d_numerator", "d_denom", "d_hat", "k", "skipped", "dlr")  # the UWU_PRODIGY_* indices

    def __init__(self, params, lr=1.0, betas=(0.9, 0.999), beta3=None, eps=1e-8, weight_decay=0, decouple=True,
                 use_bias_correction=False, safeguard_warmup=False, d0=1e-6, d_coef=1.0, growth_rate=float("inf"),
                 fsdp_in_use=False):
        if not 0.0 < d0:
            raise ValueError(f"Invalid d0 value: {d0}")
        if not 0.0 < lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 < eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), beta3=beta3, eps=eps, weight_decay=weight_decay,
                                      decouple=bool(decouple), use_bias_correction=bool(use_bias_correction),
                                      safeguard_warmup=bool(safeguard_warmup), d0=d0, d_coef=d_coef, growth_rate=growth_rate,
                                      fsdp_in_use=fsdp_in_use))
        if sum(len(g["params"]) for g in self.param_groups) != 1:
            raise NotImplementedError("FusedProdigy expects one flat parameter buffer (d is estimated over all parameters)")
        self._partials = {}  # device -> float64 workspace: a pair of partial sums per workgroup of the step's launches
        self._slots = 0  # slots the launches of the current step have written

    def _init_state(self, p, st):
        d0 = float(self.param_groups[0]["d0"])
        st["exp_avg"] = _zeros_like(p.data)
        st["exp_avg_sq"] = _zeros_like(p.data)
        st["s"] = _zeros_like(p.data)
        st["p0"] = p.data.clone()
        block = torch.tensor([d0, d0] + [0.0] * (len(self.SCALARS) - 2), dtype=torch.float64)
        st["scalars"] = block.view(torch.float32).to(p.device)

    def _workspace(self, device, slots):
        """the partials' workspace with room for ``slots`` slots; grown on the stream (what this step has written moves along)"""
        ws = self._partials.get(device)
        if ws is None or ws.numel() < 2 * slots:
            grown = torch.empty(2 * max(slots, 0 if ws is None else ws.numel()), device=device, dtype=torch.float64)
            if ws is not None and self._slots:
                grown[:2 * self._slots].copy_(ws[:2 * self._slots])
            self._partials[device] = ws = grown
        return ws

    @staticmethod
    def _beta3(group):
        return float(group["beta3"]) if group["beta3"] is not None else math.sqrt(group["betas"][1])

    def _launch(self, group, st, p_ptr, g_ptr, shadow_ptr, off, ln, pre_scale, clip_ptr, zero_grad):
        b1, b2 = group["betas"]
        blocks = L.load().uwu_prodigy_stats_blocks(ln)
        ws = self._workspace(st["s"].device, self._slots + blocks)
        L.call("uwu_prodigy_stats", p_ptr, g_ptr, L.ptr(st["p0"]) + 4 * off, L.ptr(st["exp_avg"]) + 4 * off,
               L.ptr(st["exp_avg_sq"]) + 4 * off, L.ptr(st["s"]) + 4 * off, ln, L.ptr(st["scalars"]), L.ptr(ws), ws.numel() // 2,
               self._slots, float(group["lr"]), b1, b2, self._beta3(group), float(group["weight_decay"]), int(group["decouple"]),
               float(group["d0"]), int(group["use_bias_correction"]), int(group["safeguard_warmup"]), pre_scale, clip_ptr,
               zero_grad, L.stream())
        self._slots += blocks

    def _finish(self, group, p, st, shadow):
        b1, b2 = group["betas"]
        slots, self._slots = self._slots, 0
        L.call("uwu_prodigy_finalize", L.ptr(st["scalars"]), L.ptr(self._partials[p.device]), slots, float(group["lr"]), b1, b2,
               self._beta3(group), float(group["d0"]), float(group["d_coef"]), float(group["growth_rate"]),
               int(group["use_bias_correction"]), L.stream())
        L.call("uwu_prodigy_apply", L.ptr(p.data), L.ptr(st["exp_avg"]), L.ptr(st["exp_avg_sq"]), L.ptr(shadow), p.numel(),
               L.ptr(st["scalars"]), float(group["eps"]), float(group["weight_decay"]), int(group["decouple"]), L.stream())

    @torch.no_grad()
    def step(self, *args, **kwargs):
        self._slots = 0  # (a step that raised between its launches leaves no slots behind)
        for group in self.param_groups:  # the entry points take raw pointers: the shadow's dtype is checked here, before any launch
            for p in group["params"]:
                shadow = _shadow_of(p)
                if shadow is not None and shadow.dtype != torch.bfloat16:
                    raise L.UwuError(f"uwu_prodigy_apply: the shadow must be bfloat16, got {shadow.dtype}")
        return super().step(*args, **kwargs)

    def scalars(self):
        """The scalar block as a dict of python floats, keyed by ``SCALARS``.  A host synchronisation: for logging and tests,
        never inside the step.  Before the first step: the fresh block."""
        for st in self.state.values():
            if "scalars" in st:
                return dict(zip(self.SCALARS, st["scalars"].view(torch.float64).tolist()))
        d0 = float(self.param_groups[0]["d0"])
        return dict(zip(self.SCALARS, [d0, d0] + [0.0] * (len(self.SCALARS) - 2)))

    @property
    def d(self):
        """The current step size estimate.  Reads the device scalar: a host synchronisation, meant for logging only."""
        return self.scalars()["d"]


QBLOCK = 256  # elements per quantisation block of the 8-bit state (one wave at 4 elements per lane in the kernels)


def dynamic_map(signed):
    """The 256-entry code table of the 8-bit state, a restatement of bitsandbytes' ``create_dynamic_map(signed,
    max_exponent_bits=7, total_bits=8)``: for each of 7 decades i the midpoints of ``linspace(0.1, 1, 2**i + 1)`` (unsigned:
    ``2**(i + 1) + 1``) times ``10**(i - 6)``, with both signs when signed, plus 0 and 1, sorted.  fp32, strictly increasing.
    Host only: needs no GPU."""
    data = [0.0, 1.0]
    for i in range(7):
        k = 2 ** i + 1 if signed else 2 ** (i + 1) + 1
        edges = [0.1 + 0.9 * j / (k - 1) for j in range(k)]
        for lo, hi in zip(edges[:-1], edges[1:]):
            v = 10.0 ** (i - 6) * ((lo + hi) / 2)
            data += [v, -v] if signed else [v]
    assert len(data) == 256
    return torch.tensor(sorted(data), dtype=torch.float64).to(torch.float32)


class BlockSchedule:
    """Which quantisation blocks of an ``n``-element buffer may be updated, given the chunks handed over so far.  A block is given
    out once, as part of a maximal run of whole blocks, and only when the chunks seen cover all of it: chunk offsets are multiples
    of 4 elements, not of the block, and arrive in any order, so a block can straddle two chunks.  Pure python: needs no GPU."""

    def __init__(self, n, block=QBLOCK):
        self.n, self.block = int(n), int(block)
        self.covered = []  # disjoint element ranges [a, b) the chunks cover, sorted, touching ones merged
        self.done = []  # the same of the ranges given out

    @staticmethod
    def _merged(ranges):
        out = []
        for a, b in sorted(ranges):
            if out and a <= out[-1][1]:
                out[-1] = (out[-1][0], max(out[-1][1], b))
            else:
                out.append((a, b))
        return out

    def add(self, off, ln):
        """chunk [off, off + ln) has arrived: the element ranges [(e0, e1), ...] to launch now (whole blocks; e1 may be n)"""
        a, b = int(off), int(off) + int(ln)
        if not 0 <= a < b <= self.n:
            raise ValueError(f"chunk [{a}, {b}) reaches outside the buffer of {self.n} elements")
        self.covered = self._merged(self.covered + [(a, b)])
        a, b = next((x, y) for x, y in self.covered if x <= a and b <= y)  # the covered run the chunk now belongs to
        e0 = -(-a // self.block) * self.block
        e1 = b if b == self.n else b // self.block * self.block
        out, cur = [], e0
        for x, y in self.done:
            if y <= cur or x >= e1:
                continue
            if x > cur:
                out.append((cur, x))
            cur = y
        if cur < e1:
            out.append((cur, e1))
        self.done = self._merged(self.done + out)
        return out

    def pending(self):
        """the element ranges chunks have touched that no launch has updated: the blocks only partly covered"""
        out = []
        for a, b in self.covered:
            cur = a
            for x, y in self.done:
                if y <= cur or x >= b:
                    continue
                if x > cur:
                    out.append((cur, x))
                cur = y
            if cur < b:
                out.append((cur, b))
        return out


class _Flat8bit(FlatFusedOptimizer):
    """What the 8-bit optimizers share: the state of ``MOMENTS`` moments as uint8 codes (``state1``, ``state2``), one fp32 scale
    per block of 256 elements (``absmax1``, ``absmax2``) and the code tables (``qmap1``, ``qmap2``) under the package's keys, the
    launches over whole blocks whatever the chunking, and the way back to uint8 after ``load_state_dict``."""

    MOMENTS = ()  # ((key suffix, signed table), ...)
    STATE_DTYPES = {"state1": torch.uint8, "state2": torch.uint8}

    def __init__(self, params, defaults, name, percentile_clipping=100, block_wise=True, is_paged=False):
        if percentile_clipping != 100:
            raise NotImplementedError(f"{name}: percentile_clipping is not implemented")
        if not block_wise:
            raise NotImplementedError(f"{name}: block_wise=False is not implemented")
        if is_paged:
            raise NotImplementedError(f"{name}: is_paged=True is not implemented")
        super().__init__(params, defaults)
        self._sched = {}

    def _init_state(self, p, st):
        blocks = -(-p.numel() // QBLOCK)
        for k, signed in self.MOMENTS:
            st["state" + k] = _zeros_like(p.data, dtype=torch.uint8)
            st["absmax" + k] = _zeros_like(p.data[:blocks])  # 0: every code reads as 0
            st["qmap" + k] = dynamic_map(signed).to(p.device)

    def _launch_blocks(self, group, st, p_ptr, g_ptr, shadow_ptr, e0, e1, pre_scale, clip_ptr, zero_grad):
        raise NotImplementedError

    def _launch(self, group, st, p_ptr, g_ptr, shadow_ptr, off, ln, pre_scale, clip_ptr, zero_grad):
        # the kernels take base pointers and a range of whole blocks: a block is launched once the chunks seen cover all of it
        sched = self._sched.get(id(st))
        if sched is None:
            sched = self._sched[id(st)] = BlockSchedule(st["state1"].numel())
        base_shadow = shadow_ptr - 2 * off if shadow_ptr is not None else None
        for e0, e1 in sched.add(off, ln):
            self._launch_blocks(group, st, p_ptr - 4 * off, g_ptr - 4 * off, base_shadow, e0, e1, pre_scale, clip_ptr, zero_grad)

    def _finish(self, group, p, st, shadow):
        sched = self._sched.pop(id(st), None)
        left = sched.pending() if sched is not None else []
        if left:
            raise ValueError(f"{type(self).__name__}: the chunks leave blocks of {QBLOCK} elements partly covered (elements {left}); "
                             f"their gradient was consumed by no launch")

    @torch.no_grad()
    def step(self, *args, **kwargs):
        self._sched = {}  # (a step that raised between its launches leaves no schedule behind)
        return super().step(*args, **kwargs)


class FusedAdamW8bit(_Flat8bit):
    """``bitsandbytes.optim.AdamW8bit`` on a flat buffer: AdamW whose two moments are kept as 8-bit codes of a 256-entry dynamic
    table with one fp32 scale per block of 256 elements (2.03 B of state per parameter instead of 8).  The rule is written out at
    ``uwu_adamw8_step`` (include/uwu_hip.h); the package is not installed here, so checkpoint interchange with it is not verified.

    Blocks are counted from the start of the flat buffer and ignore tensor boundaries inside it.  ``min_8bit_size`` (the package
    keeps smaller tensors in fp32) is accepted and ignored: every element of the buffer is quantised.  ``optim_bits`` and ``args``
    are accepted for the signature and ignored; ``amsgrad``, ``percentile_clipping``, ``block_wise=False`` and ``is_paged`` are not
    implemented."""

    MOMENTS = (("1", True), ("2", False))

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, optim_bits=32,
                 args=None, min_8bit_size=4096, percentile_clipping=100, block_wise=True, is_paged=False):
        if amsgrad:
            raise NotImplementedError("FusedAdamW8bit: amsgrad=True is not implemented")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay), "FusedAdamW8bit",
                         percentile_clipping, block_wise, is_paged)

    def _init_state(self, p, st):
        st["step"] = 0
        super()._init_state(p, st)

    def _launch_blocks(self, group, st, p_ptr, g_ptr, shadow_ptr, e0, e1, pre_scale, clip_ptr, zero_grad):
        b1, b2 = group["betas"]
        L.call("uwu_adamw8_step", p_ptr, g_ptr, L.ptr(st["state1"]), L.ptr(st["state2"]), L.ptr(st["absmax1"]),
               L.ptr(st["absmax2"]), L.ptr(st["qmap1"]), L.ptr(st["qmap2"]), shadow_ptr, st["state1"].numel(), e0, e1,
               float(group["lr"]), b1, b2, group["eps"], group["weight_decay"], st["step"], pre_scale, clip_ptr, zero_grad,
               L.stream())


class FusedLion8bit(_Flat8bit):
    """``bitsandbytes.optim.Lion8bit`` on a flat buffer: ``FusedLion`` whose moment is kept as 8-bit codes of the signed dynamic
    table with one fp32 scale per block of 256 elements (``uwu_lion8_step``).  Blocks, ``min_8bit_size`` and what is not
    implemented as in ``FusedAdamW8bit``."""

    MOMENTS = (("1", True),)

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.99), weight_decay=0, min_8bit_size=4096, percentile_clipping=100,
                 block_wise=True, is_paged=False):
        super().__init__(params, dict(lr=lr, betas=tuple(betas), weight_decay=weight_decay), "FusedLion8bit",
                         percentile_clipping, block_wise, is_paged)

    def _launch_blocks(self, group, st, p_ptr, g_ptr, shadow_ptr, e0, e1, pre_scale, clip_ptr, zero_grad):
        b1, b2 = group["betas"]
        L.call("uwu_lion8_step", p_ptr, g_ptr, L.ptr(st["state1"]), L.ptr(st["absmax1"]), L.ptr(st["qmap1"]), shadow_ptr,
               st["state1"].numel(), e0, e1, float(group["lr"]), b1, b2, group["weight_decay"], pre_scale, clip_ptr, zero_grad,
               L.stream())


class FusedAdamWScheduleFree(FlatFusedOptimizer):
    """``schedulefree.AdamWScheduleFree`` (Defazio et al., "The Road Less Scheduled") on a flat buffer: no learning-rate schedule,
    the gradient taken at an interpolation ``y`` and the model to validate, checkpoint and sample from the average ``x``.  The package
    is not installed here; the rule below follows ``AdamWScheduleFree.step`` (single-tensor path, package 1.4), is restated at
    ``uwu_sfadamw_step`` (include/uwu_hip.h) and pinned by an fp64 oracle (tests/test_schedulefree_cpu.py).  Checkpoint interchange
    with the package is not verified.

    Per parameter group, python floats on the host, advanced once per optimizer step (never once per chunk)::

        k (starts 0)    weight_sum (starts 0.0)    lr_max (starts -1.0)    train_mode (starts False)
        sched       = (k + 1) / warmup_steps  if k < warmup_steps  else 1.0
        bc2         = 1 - beta2 ** (k + 1)
        lr_t        = lr * sched                      -> group["scheduled_lr"]
        lr_max      = max(lr_t, lr_max)
        weight      = (k + 1) ** r * lr_max ** weight_lr_power
        weight_sum += weight
        c           = weight / weight_sum             (0.0 when weight_sum == 0)

    Per element, with ``y`` the parameter as training holds it, ``g`` the gradient after ``pre_scale`` and the clip coefficient, and
    the state ``z`` (starts as a copy of the parameter) and ``exp_avg_sq`` (``v``, starts 0)::

        v  = beta2 * v + (1 - beta2) * g * g
        gn = g / (sqrt(v / bc2) + eps) + weight_decay * y       # y BEFORE the interpolation below
        y  = lerp(y, z, c)                                      # torch.lerp's two branches: exactly z at c = 1 (the first step)
        y  = y + lr_t * (beta1 * (1 - c) - 1) * gn
        z  = z - lr_t * gn
        k += 1   (after all elements)

    ``step()`` while ``train_mode`` is False raises ``RuntimeError``, as the package does.  The two modes::

        eval():   if train_mode:      p = lerp(y, z, 1 - 1/beta1)    # x, the average; train_mode = False
        train():  if not train_mode:  p = y again;                   train_mode = True

    One departure from the package: it gets ``y`` back from ``x`` with a second ``lerp``, which does not round-trip in fp32.  Here
    ``eval()`` writes ``x`` out of place into a spare fp32 buffer as long as the parameter (``uwu_sf_average``) and exchanges the two
    with ``uwu_ema_swap``, which also refreshes the bf16 shadow and moves no pointer; ``train()`` exchanges them back: ``y`` returns
    bit for bit.  The spare buffer is allocated at the first ``eval()`` after a step, or is the buffer of a ``FlatAverage``
    (averaging.py) handed over with ``use_average``: the exchange then goes through it, and the owner of the flat buffer learns
    that its weights were written (the UNet merges its adapters again).  8 B of state per parameter and 4 B for the spare buffer.

    ``foreach`` is accepted for the package's signature and ignored.  Not built: ``SGDScheduleFree``, ``RAdamScheduleFree``, the
    closure / reference / wrapper classes, several parameter groups with different ``lr`` (the scalars are kept per group, but the
    fit loop trains one flat buffer and nothing tests more), and the recalibration of BatchNorm statistics (no batch norm trains
    here)."""

    def __init__(self, params, lr=0.0025, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, warmup_steps=0, r=0.0,
                 weight_lr_power=2.0, foreach=None):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 < betas[0] < 1.0:  # (1 / beta1 gives the averaged weights)
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]} (schedule-free AdamW needs 0 < beta1 < 1)")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, r=r, k=0, warmup_steps=warmup_steps, train_mode=False,
                                      weight_sum=0.0, lr_max=-1.0, scheduled_lr=0.0, weight_lr_power=weight_lr_power,
                                      weight_decay=weight_decay, foreach=foreach))
        self._spare = {}  # parameter -> the spare fp32 buffer (x is written there; it holds y while the parameter holds x)
        self._averages = {}  # parameter -> the FlatAverage whose buffer is the spare one (use_average)
        self._held = set()  # parameters whose spare buffer holds y right now
        self._now = {}  # id(group) -> (lr_t, c, bc2) of the step being launched
        self.register_load_state_dict_post_hook(FusedAdamWScheduleFree._nothing_held)

    @staticmethod
    def step_scalars(group):
        """The host side of one step from the group's scalars, none of them changed: (lr_t, lr_max, weight_sum, c, bc2).  Pure python:
        needs no GPU."""
        k, warmup = int(group["k"]), group["warmup_steps"]
        sched = (k + 1) / warmup if k < warmup else 1.0
        bc2 = 1 - group["betas"][1] ** (k + 1)
        lr_t = group["lr"] * sched
        lr_max = max(lr_t, group["lr_max"])
        weight = ((k + 1) ** group["r"]) * (lr_max ** group["weight_lr_power"])
        weight_sum = group["weight_sum"] + weight
        c = weight / weight_sum if weight_sum != 0 else 0.0
        return lr_t, lr_max, weight_sum, c, bc2

    def _init_state(self, p, st):
        st["z"] = torch.clone(p.data, memory_format=torch.preserve_format)
        st["exp_avg_sq"] = _zeros_like(p.data)

    def _launch(self, group, st, p_ptr, g_ptr, shadow_ptr, off, ln, pre_scale, clip_ptr, zero_grad):
        b1, b2 = group["betas"]
        lr_t, c, bc2 = self._now[id(group)]
        L.call("uwu_sfadamw_step", p_ptr, g_ptr, L.ptr(st["z"]) + 4 * off, L.ptr(st["exp_avg_sq"]) + 4 * off, shadow_ptr, ln, lr_t,
               b1, b2, float(group["eps"]), float(group["weight_decay"]), c, bc2, pre_scale, clip_ptr, zero_grad, L.stream())

    @torch.no_grad()
    def step(self, *args, **kwargs):
        if not all(g["train_mode"] for g in self.param_groups):
            raise RuntimeError("Optimizer was not in train mode when step is called. Please insert .train() and .eval() calls on the "
                               "optimizer. See the schedulefree documentation for details.")
        ahead = [self.step_scalars(g) for g in self.param_groups]  # once per step, before the first chunk's launch
        self._now = {id(g): (float(lr_t), float(c), float(bc2)) for g, (lr_t, _, _, c, bc2) in zip(self.param_groups, ahead)}
        try:
            loss = super().step(*args, **kwargs)
        finally:
            self._now = {}
        for g, (lr_t, lr_max, weight_sum, _, _) in zip(self.param_groups, ahead):  # (a step that raised advances nothing)
            g["scheduled_lr"], g["lr_max"], g["weight_sum"] = lr_t, lr_max, weight_sum
            g["k"] = int(g["k"]) + 1
        return loss

    # ------------------------------------------------------------------ the two modes
    def use_average(self, average):
        """``average`` (a ``FlatAverage`` over the module that owns the trained flat buffer) lends its buffer as the spare one and its
        ``swap`` as the exchange.  Call it while in train mode (nothing is held in a spare buffer then)."""
        p = average.owner.flat
        if p in self._held:
            raise RuntimeError("FusedAdamWScheduleFree.use_average: call train() first (the spare buffer holds the trained weights)")
        self._averages[p] = average
        self._spare.pop(p, None)

    def _spare_of(self, p):
        avg = self._averages.get(p)
        if avg is not None:
            return avg.avg
        buf = self._spare.get(p)
        if buf is None or buf.numel() != p.numel() or buf.device != p.device:
            buf = self._spare[p] = torch.empty_like(p.data, memory_format=torch.contiguous_format)
        return buf

    def _exchange(self, p):
        avg = self._averages.get(p)
        if avg is not None:
            avg.swap()
            return
        L.call("uwu_ema_swap", L.ptr(self._spare[p]), L.ptr(p.data), L.ptr(_shadow_of(p)), p.numel(), 0, L.stream())

    @torch.no_grad()
    def write_average(self, p):
        """``x = lerp(y, z, 1 - 1/beta1)`` of parameter ``p`` written into its spare buffer, which is returned; ``p`` is only read.
        Train mode only (in eval mode ``p`` holds ``x`` already).  None before the first step: ``x`` is the parameter itself."""
        group = next(g for g in self.param_groups if any(q is p for q in g["params"]))
        if not group["train_mode"]:
            raise RuntimeError("FusedAdamWScheduleFree.write_average: the parameter holds the average already (eval mode)")
        if p not in self.state or "z" not in self.state[p]:
            return None
        spare = self._spare_of(p)
        L.call("uwu_sf_average", L.ptr(p.data), L.ptr(self.state[p]["z"]), L.ptr(spare), p.numel(), 1.0 - 1.0 / group["betas"][0],
               L.stream())
        return spare

    def held_weights(self, p):
        """the buffer that holds ``y`` while ``p`` holds ``x`` (eval mode, after a step); None otherwise"""
        return self._spare_of(p) if p in self._held else None

    @torch.no_grad()
    def eval(self):
        """The parameters become the average ``x`` (and their bf16 shadow follows); ``y`` is kept aside.  Does nothing in eval mode."""
        for group in self.param_groups:
            if not group["train_mode"]:
                continue
            for p in group["params"]:
                if self.write_average(p) is not None:  # (before the first step x = y = z: nothing to exchange)
                    self._exchange(p)
                    self._held.add(p)
            group["train_mode"] = False

    @torch.no_grad()
    def train(self):
        """The parameters become ``y`` again, bit for bit.  Does nothing in train mode.  After ``load_state_dict`` nothing is kept aside:
        the parameters are taken to hold ``y`` (the fit loop resumes from ``current_model_state``)."""
        for group in self.param_groups:
            if group["train_mode"]:
                continue
            for p in group["params"]:
                if p in self._held:
                    self._exchange(p)
                    self._held.discard(p)
            group["train_mode"] = True

    def _nothing_held(self):
        """after ``load_state_dict``: whatever mode the state was saved in, no spare buffer holds a ``y`` of this optimizer"""
        self._held.clear()


def flat_tensors(module):
    """[(offset, shape), ...] of the tensors a flat-buffer module (``FlatModule``, ``LycorisNetwork``) keeps in ``flat``, with the
    shapes as stored: what ``FusedAdafactor(tensors=)`` takes.  Host only: works on a meta-device module."""
    layout = module.offsets if hasattr(module, "offsets") else module.P.registry
    return [(int(off), tuple(int(d) for d in shape)) for off, shape in layout.values()]


def adafactor_view(shape):
    """(R, C) Adafactor sees a stored tensor as: ``[shape[0], prod(shape[1:])]`` with two or more dimensions, else (0, numel)"""
    shape = tuple(int(d) for d in shape)
    if len(shape) >= 2:
        return shape[0], math.prod(shape[1:])
    return 0, math.prod(shape)


def adafactor_state_elems(tensors, beta1=False, n=None):
    """fp32 state elements ``FusedAdafactor`` keeps for ``tensors`` = [(offset, shape), ...], by state key.  ``exp_avg`` (with
    ``beta1``) is laid out as the parameters, so it has the flat buffer's ``n`` elements, padding included: give ``n``.  Pure
    python: needs no GPU."""
    views = [adafactor_view(shape) for _, shape in tensors]
    out = {"exp_avg_sq_row": sum(r for r, c in views if r), "exp_avg_sq_col": sum(c for r, c in views if r),
           "exp_avg_sq": sum(c for r, c in views if not r), "RMS": len(views)}
    if beta1:
        if n is None:
            raise ValueError("adafactor_state_elems: exp_avg is as long as the flat buffer: give n")
        out["exp_avg"] = int(n)
    return out


class TensorSchedule:
    """Which tensors of a flat buffer may be updated, given the chunks handed over so far.  ``tensors`` = [(offset, numel), ...],
    ascending and disjoint.  A tensor is given out once, by index, when the chunks seen cover all of it: chunks cut through
    tensors, arrive in any order and may touch or overlap.  Pure python: needs no GPU."""

    def __init__(self, tensors):
        self.tensors = [(int(o), int(n)) for o, n in tensors]
        if any(n <= 0 for _, n in self.tensors) or any(a[0] + a[1] > b[0] for a, b in zip(self.tensors, self.tensors[1:])):
            raise ValueError("TensorSchedule: the tensors must be non-empty, ascending and disjoint")
        self.starts = [o for o, _ in self.tensors]
        self.covered = []  # disjoint element ranges [a, b) the chunks cover, sorted, touching ones merged
        self.done = set()

    def _touched(self, a, b):
        """indices of the tensors that intersect [a, b)"""
        i = bisect.bisect_right(self.starts, a) - 1
        if i < 0 or self.tensors[i][0] + self.tensors[i][1] <= a:
            i += 1
        return range(i, bisect.bisect_left(self.starts, b))

    def add(self, off, ln):
        """chunk [off, off + ln) has arrived: the indices (ascending) of the tensors to launch now"""
        a, b = int(off), int(off) + int(ln)
        if not 0 <= a < b:
            raise ValueError(f"chunk [{a}, {b}) is empty or starts below 0")
        self.covered = BlockSchedule._merged(self.covered + [(a, b)])
        x, y = next((x, y) for x, y in self.covered if x <= a and b <= y)  # the covered run the chunk now belongs to
        out = [i for i in self._touched(x, y)
               if i not in self.done and x <= self.tensors[i][0] and self.tensors[i][0] + self.tensors[i][1] <= y]
        self.done.update(out)
        return out

    def pending(self):
        """indices of the tensors that chunks have touched and that no ``add`` has given out: the partly covered ones"""
        return sorted({i for x, y in self.covered for i in self._touched(x, y) if i not in self.done})


class FusedAdafactor(FlatFusedOptimizer):
    """``transformers.optimization.Adafactor`` (Shazeer & Stern, "Adafactor: Adaptive Learning Rates with Sublinear Memory Cost") on
    a flat buffer: the second moment of a matrix is kept as one value per row and one per column instead of one per element.  The
    rule is written out at ``uwu_adafactor_stats`` (include/uwu_hip.h); the signature and the two ``ValueError`` are the package's.
    kohya-style trainers use ``relative_step=False, scale_parameter=False, warmup_init=False`` with a manual ``lr``.

    **The unit "tensor".**  The rule is per tensor (row means, column means, a per-tensor RMS clip and parameter scale), and a tensor
    here is an entry of ``tensors`` = [(offset, shape), ...]: the flat store's registry as stored (``flat_tensors(module)``; without
    it the whole buffer is one 1-D tensor).  Anything of two or more dimensions is seen as ``[shape[0], prod(shape[1:])]``.  For the
    Linears this is the package's unit.  It is NOT the package's unit for tensors that the store packs into one entry, for the 3x3
    convolutions (stored ``(cout_store, 9 * cin_store)``: the package would factor the trailing 3 x 3 of the 4-D weight), and for
    padded channels, which hold zero weight and zero gradient, take part in the means and stay exactly zero.  What the tests hold
    the kernels to is the package's rule applied to the list of stored tensors in these 2-D views.

    State under the package's keys, each one flat fp32 tensor: ``exp_avg_sq_row`` / ``exp_avg_sq_col`` over all factored tensors,
    ``exp_avg_sq`` over the 1-D ones, ``exp_avg`` (as long as the parameters) only with ``beta1``, ``RMS`` one entry per tensor
    (written when ``scale_parameter``), and ``step``.  Checkpoint interchange with the package is not claimed.

    A step is three entry points (four kernel launches) per set of tensors that became ready, whatever their number: behind a
    chunked gradient exchange a tensor is launched once the chunks seen cover all of it (``TensorSchedule``), and its result does
    not depend on the launch it was part of, bit for bit.  Chunks that leave a touched tensor partly covered raise ``ValueError``
    at the end of the step; by then the fully covered tensors have been updated and ``step`` has advanced (a half-applied step).  ``group["lr"]`` stays a float under the schedulers; with ``relative_step``
    it is None and the step size is computed on the host from ``step`` (``lr_t``, logged by ``LearningRateMonitor``).  One flat
    parameter buffer, one parameter group.  Not built: ``AdafactorSchedule``, the package's trailing-two-dims factoring of 4-D
    tensors, 8-bit or bf16 ``exp_avg``, CAME, ``torch.optim.Adafactor`` (a different rule)."""

    def __init__(self, params, lr=None, eps=(1e-30, 1e-3), clip_threshold=1.0, decay_rate=-0.8, beta1=None, weight_decay=0.0,
                 scale_parameter=True, relative_step=True, warmup_init=False, tensors=None):
        if lr is not None and relative_step:
            raise ValueError("Cannot combine manual `lr` and `relative_step=True` options")
        if warmup_init and not relative_step:
            raise ValueError("`warmup_init=True` requires `relative_step=True`")
        if lr is None and not relative_step:
            raise ValueError("`relative_step=False` needs a manual `lr`")
        if not clip_threshold > 0.0:
            raise ValueError(f"Invalid clip_threshold value: {clip_threshold}")
        if beta1 is not None and not 0.0 <= beta1 < 1.0:
            raise ValueError(f"Invalid beta1 value: {beta1}")
        super().__init__(params, dict(lr=lr, eps=tuple(eps), clip_threshold=clip_threshold, decay_rate=decay_rate, beta1=beta1,
                                      weight_decay=weight_decay, scale_parameter=bool(scale_parameter),
                                      relative_step=bool(relative_step), warmup_init=bool(warmup_init)))
        ps = [p for g in self.param_groups for p in g["params"]]
        if len(ps) != 1:
            raise NotImplementedError("FusedAdafactor expects one flat parameter buffer")
        n = ps[0].numel()
        self.tensors = self.check_tensors(tensors if tensors is not None else [(0, (n,))], n)
        self.lr_t = None  # the step size of the last step before the parameter scale (a host float)
        self._dev = None  # the table, the workspaces and the tiling of every tensor, built at the first step
        self._lists = {}  # tuple of tensor indices -> (host launch list, device copy)
        self._sched = self._desc = None

    @staticmethod
    def check_tensors(tensors, n):
        """``tensors`` sorted by offset as [(offset, (R, C)), ...] after the checks the entry points repeat on the table: inside the
        buffer of ``n`` elements, offsets that are multiples of 4 elements, R * C < 2^31, no overlap.  Pure python."""
        out = sorted((int(off), adafactor_view(shape)) for off, shape in tensors)
        if not out:
            raise ValueError("FusedAdafactor: tensors is empty")
        end = 0
        for off, (r, c) in out:
            numel = r * c if r else c
            if numel < 1 or numel >= 2 ** 31:
                raise ValueError(f"FusedAdafactor: the tensor at {off} has {numel} elements (needs 1 <= R * C < 2^31)")
            if off % 4:
                raise ValueError(f"FusedAdafactor: the tensor at {off} is misaligned (offsets are multiples of 4 elements)")
            if off < end:
                raise ValueError(f"FusedAdafactor: the tensor at {off} overlaps its predecessor (or starts below 0)")
            if off + numel > n:
                raise ValueError(f"FusedAdafactor: the tensor [{off}, {off + numel}) is out of range of the buffer of {n} elements")
            end = off + numel
        return out

    def step_size(self, group, step):
        """``lr_t`` before the parameter scale: the package's ``_get_lr`` without ``max(eps[1], RMS)``.  A host float."""
        if not group["relative_step"]:
            return float(group["lr"])
        return min(1e-6 * step if group["warmup_init"] else 1e-2, 1.0 / math.sqrt(step))

    def _device_side(self, p):
        """the table (host and device), the workspaces and the per-tensor workgroup counts; built once per device"""
        if self._dev is not None and self._dev["device"] == p.device:
            return self._dev
        lib = L.load()
        rows, tiles, mblocks = [], [], []
        o_row = o_col = o_v = o_f = o_d = 0
        for off, (r, c) in self.tensors:
            rows.append([off, r, c, o_row, o_col, o_v, o_f, o_d])
            if r:
                o_row, o_col = o_row + r, o_col + c
            else:
                o_v += c
            o_f += lib.uwu_adafactor_ws_floats(r, c)
            o_d += lib.uwu_adafactor_ws_doubles(r, c)
            tiles.append(lib.uwu_adafactor_tiles(r, c))
            mblocks.append(lib.uwu_adafactor_moment_blocks(r, c))
        host = torch.tensor(rows, dtype=torch.int64)
        self._dev = dict(device=p.device, host=host, table=host.to(p.device), tiles=tiles, mblocks=mblocks,
                         fws=torch.empty(max(o_f, 1), device=p.device, dtype=torch.float32),
                         dws=torch.empty(max(o_d, 1), device=p.device, dtype=torch.float64))
        self._lists = {}
        return self._dev

    def _init_state(self, p, st):
        n = adafactor_state_elems([(off, (r, c) if r else (c,)) for off, (r, c) in self.tensors])
        st["step"] = 0
        for k in ("exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_sq", "RMS"):  # (an empty tensor has no pointer: one spare element)
            st[k] = _zeros_like(torch.empty(max(n[k], 1), device=p.device, dtype=torch.float32))
        if self.param_groups[0]["beta1"] is not None:
            st["exp_avg"] = _zeros_like(p.data)

    def _launch_list(self, dev, ids):
        key = tuple(ids)
        hit = self._lists.get(key)
        if hit is None:
            if len(self._lists) >= 256:  # (a chunking that changes every step: do not keep every list it ever made)
                self._lists = {}
            t_start, m_start = [0], [0]
            for i in ids:
                t_start.append(t_start[-1] + dev["tiles"][i])
                m_start.append(m_start[-1] + dev["mblocks"][i])
            host = torch.tensor(list(ids) + t_start + m_start, dtype=torch.int64)
            hit = self._lists[key] = (host, host.to(dev["device"]))
        return hit

    def descriptor(self, p, st, p_ptr, g_ptr, shadow_ptr):
        """the ``UwuAdafactorDesc`` of parameter ``p`` with state ``st``: the buffers' BASE pointers and their lengths"""
        dev = self._device_side(p)
        if len(st["RMS"]) < len(self.tensors) or ("exp_avg" in st and st["exp_avg"].numel() != p.numel()):
            raise ValueError("FusedAdafactor: the state does not fit the tensors (RMS or exp_avg has the wrong length)")
        d = L.AdafactorDesc()
        d.p, d.g, d.p_bf16 = p_ptr, g_ptr, shadow_ptr
        d.row, d.col, d.v = L.ptr(st["exp_avg_sq_row"]), L.ptr(st["exp_avg_sq_col"]), L.ptr(st["exp_avg_sq"])
        d.m, d.rms = L.ptr(st.get("exp_avg")), L.ptr(st["RMS"])
        d.fws, d.dws = L.ptr(dev["fws"]), L.ptr(dev["dws"])
        d.table_host, d.table, d.ntensors = dev["host"].data_ptr(), L.ptr(dev["table"]), len(self.tensors)
        d.n, d.n_row, d.n_col, d.n_v = p.numel(), st["exp_avg_sq_row"].numel(), st["exp_avg_sq_col"].numel(), st["exp_avg_sq"].numel()
        d.n_fws, d.n_dws = dev["fws"].numel(), dev["dws"].numel()
        return d

    def pass_calls(self, group, step, desc, ids, pre_scale, clip_ptr, zero_grad):
        """[(entry point, arguments), ...]: the three passes over the tensors ``ids`` (ascending table indices) at ``step``"""
        host, devlist = self._launch_list(self._dev, ids)
        head = (ctypes.byref(desc), host.data_ptr(), L.ptr(devlist), len(ids))
        beta2t = 1.0 - math.pow(step, group["decay_rate"])
        self.lr_t = self.step_size(group, step)
        sp, b1 = int(group["scale_parameter"]), group["beta1"]
        return [("uwu_adafactor_stats", (*head, beta2t, float(group["eps"][0]), sp, pre_scale, clip_ptr, L.stream())),
                ("uwu_adafactor_norm", (*head, pre_scale, clip_ptr, L.stream())),
                ("uwu_adafactor_apply", (*head, self.lr_t, float(group["eps"][1]), float(group["clip_threshold"]), sp,
                                         int(b1 is not None), float(b1 or 0.0), float(group["weight_decay"]), pre_scale, clip_ptr,
                                         zero_grad, L.stream()))]

    def _launch(self, group, st, p_ptr, g_ptr, shadow_ptr, off, ln, pre_scale, clip_ptr, zero_grad):
        if self._sched is None:
            self._sched = TensorSchedule([(o, r * c if r else c) for o, (r, c) in self.tensors])
        ids = self._sched.add(off, ln)
        if not ids:
            return
        if self._desc is None:  # (``_launch`` is handed the chunk's pointers)
            p = next(q for q in group["params"] if self.state[q] is st)
            self._desc = self.descriptor(p, st, p_ptr - 4 * off, g_ptr - 4 * off,
                                         shadow_ptr - 2 * off if shadow_ptr is not None else None)
        for name, args in self.pass_calls(group, int(st["step"]), self._desc, ids, pre_scale, clip_ptr, zero_grad):
            L.call(name, *args)

    def _finish(self, group, p, st, shadow):
        # (raises after the launches: the tensors the chunks did cover are updated and ``step`` has advanced -- the step is then half
        # applied, as with the 8-bit optimizers' partly covered blocks; the chunking is the caller's to repair)
        sched, self._sched, self._desc = self._sched, None, None
        left = sched.pending() if sched is not None else []
        if left:
            raise ValueError(f"FusedAdafactor: the chunks leave tensors partly covered (the tensors at offsets "
                             f"{[self.tensors[i][0] for i in left]}); their gradient was consumed by no launch")

    @torch.no_grad()
    def step(self, *args, **kwargs):
        self._sched = self._desc = None  # (a step that raised between its launches leaves no schedule behind)
        for group in self.param_groups:  # the entry points take raw pointers: the shadow's dtype is checked here, before any launch
            for p in group["params"]:
                shadow = _shadow_of(p)
                if shadow is not None and shadow.dtype != torch.bfloat16:
                    raise L.UwuError(f"uwu_adafactor_apply: the shadow must be bfloat16, got {shadow.dtype}")
        return super().step(*args, **kwargs)


def cosine_lr(base_lr, step, T_max, eta_min):
    """Closed form of torch.optim.lr_scheduler.CosineAnnealingLR (trainer.py:111-115 defaults)."""
    return eta_min + (base_lr - eta_min) * (1 + math.cos(math.pi * step / T_max)) / 2
