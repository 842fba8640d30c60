"""GPU: the fused Lion / AdamWFP16 update kernels (csrc/optimizer.hip) against the reference fixture and the fp64 restatements
of tests/test_optimizers_cpu.py, their edge shapes, and both optimizers through DMTrainer / Fitter (fused branch, checkpoint
resume, LyCORIS adapters)."""
import math
import os

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests.test_optimizers_cpu import (adamw_fp16_step, decay_bookkeeping, fixture_state_before, fp16_neighbours, fp16_special,
                                       lion_step, load_fixture)

from uwudiff_amd.flat import FlatModule

pytestmark = pytest.mark.gpu

TOML = os.path.join(ROOT, "configs", "lycoris", "sdxl-diffusers.toml")


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _bits(t):
    return t.detach().cpu().view(torch.int16).numpy().view(np.uint16)


def _half_from_bits(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).view(torch.float16).cuda()


def _check_moments(got_bits, want_bits, what, exact_special=True):
    """bit-equal or the adjacent fp16 value, adjacent on at most 1 % of the elements; inf, zero and subnormal elements exactly.
    (``exact_special=False`` where the inputs are random: a subnormal moment that is the difference of two ordinary terms
    carries their fp32 rounding, 2^-24 of THEIR size, which is a visible fraction of the fp16 subnormal spacing 2^-24.)"""
    eq, adj = fp16_neighbours(got_bits, want_bits)
    print(f"{what}: {int(adj.sum())} adjacent, {int((~(eq | adj)).sum())} further, of {eq.size}")
    assert (eq | adj).all(), what
    assert adj.sum() <= max(0.01 * eq.size, 0 if exact_special else 1), what
    if not exact_special:
        return
    special = fp16_special(want_bits)
    assert np.array_equal(got_bits[special], want_bits[special]), what
    assert np.array_equal(fp16_special(got_bits), special), what


def _flat_layout(lengths):
    """the tensors on 64-element boundaries of one flat buffer, as uwudiff_amd.flat lays them out (the last one unpadded)"""
    segs, off = [], 0
    for n in lengths:
        segs.append((off, n))
        off += (n + 63) // 64 * 64
    return segs, segs[-1][0] + segs[-1][1]


def _scatter(segs, n, packed, fill=0):
    out = np.full(n, fill, dtype=packed.dtype)
    k = 0
    for off, ln in segs:
        out[off:off + ln] = packed[k:k + ln]
        k += ln
    return out


def _gather(segs, flat):
    return np.concatenate([flat[off:off + ln] for off, ln in segs])


# ------------------------------------------------------------------------------------------------------------ AdamWFP16
def test_adamw_fp16_follows_the_reference_fixture_step_by_step():
    """Every step starts from the FIXTURE's state before it (a one-ulp fp16 difference cannot compound), runs the class with the
    fixture's segments and phases, and is compared with what the reference class recorded after it."""
    from uwudiff_amd.optim import FusedAdamWFP16

    f, lengths, hp = load_fixture()
    segs, n = _flat_layout(lengths)
    assert n % 4 and len(segs) == 3
    flat = torch.nn.Parameter(torch.zeros(n, device="cuda"))
    flat._uwu_bf16_shadow = torch.zeros(n, device="cuda", dtype=torch.bfloat16)
    opt = FusedAdamWFP16([flat], lr=hp["lr"], betas=hp["betas"], eps=hp["eps"], weight_decay=hp["weight_decay"],
                         segments=segs)
    assert opt.decay_threshold == hp["threshold"]
    for t in range(f["g"].shape[0]):
        p, m_bits, v_bits, acc = fixture_state_before(f, t)
        flat.data.copy_(_dev(_scatter(segs, n, p)))
        flat.grad = _dev(_scatter(segs, n, f["g"][t]))
        opt.state[flat] = {"step": t, "exp_avg": _half_from_bits(_scatter(segs, n, m_bits)),
                           "exp_avg_sq": _half_from_bits(_scatter(segs, n, v_bits)), "accumulated_decay": list(acc)}
        opt.step(zero_grad=True)
        torch.cuda.synchronize()
        st = opt.state[flat]
        assert st["step"] == t + 1 and st["exp_avg"].dtype == torch.float16 and st["exp_avg_sq"].dtype == torch.float16
        got_p = flat.detach().cpu().numpy()
        err = np.abs(_gather(segs, got_p) - f["p"][t])
        print(f"step {t + 1}: max |p - reference| {err.max():.3e}; accumulated_decay {st['accumulated_decay']}")
        np.testing.assert_allclose(_gather(segs, got_p), f["p"][t], rtol=1e-5, atol=1e-6)
        _check_moments(_gather(segs, _bits(st["exp_avg"])), f["m16"][t], f"step {t + 1} exp_avg")
        _check_moments(_gather(segs, _bits(st["exp_avg_sq"])), f["v16"][t], f"step {t + 1} exp_avg_sq")
        # decay on exactly the fixture's steps and tensors, with its amounts
        np.testing.assert_allclose(st["accumulated_decay"], f["acc"][t], rtol=0, atol=1e-15)
        assert [a == 0.0 for a in st["accumulated_decay"]] == [a == 0.0 for a in f["acc"][t]]
        assert torch.equal(flat._uwu_bf16_shadow, flat.detach().bfloat16())
        assert not flat.grad.any()
        pad = np.ones(n, bool)
        for off, ln in segs:
            pad[off:off + ln] = False
        assert not got_p[pad].any() and not _bits(st["exp_avg"])[pad].any()


def test_adamw_fp16_carrying_its_own_state():
    """6 steps on the kernel's own state (chunked launches at 8-byte-aligned fp16 offsets); each step against the fp64
    restatement applied to the kernel's previous state."""
    from uwudiff_amd.optim import FusedAdamWFP16

    f, lengths, hp = load_fixture()
    segs, n = _flat_layout(lengths)
    flat = torch.nn.Parameter(_dev(_scatter(segs, n, f["p0"])))
    flat._uwu_bf16_shadow = torch.zeros(n, device="cuda", dtype=torch.bfloat16)
    opt = FusedAdamWFP16([flat], lr=hp["lr"], betas=hp["betas"], eps=hp["eps"], weight_decay=hp["weight_decay"],
                         segments=segs)
    torch.manual_seed(0)
    chunks = [(0, 1236), (1236, n - 1236)]  # the second chunk's fp16 state starts 8 bytes off a 16-byte boundary
    p_prev, m_prev, v_prev, acc = flat.detach().cpu().numpy().copy(), np.zeros(n, np.uint16), np.zeros(n, np.uint16), None
    for t in range(f["g"].shape[0]):
        g = _scatter(segs, n, f["g"][t])
        flat.grad = _dev(g)
        opt.step(chunks=chunks, zero_grad=True)
        torch.cuda.synchronize()
        st = opt.state[flat]
        if acc is None:  # drawn at the first step, in segment order, from torch's global CPU generator
            torch.manual_seed(0)
            acc = [float(torch.rand([]) * opt.decay_threshold) for _ in segs]
            assert acc == [float(a) for a in f["acc0"]]
        want_p, want_m, want_v, _, _ = adamw_fp16_step(p_prev, g, m_prev.view(np.float16), v_prev.view(np.float16), t + 1,
                                                       hp["lr"], hp["betas"], hp["eps"])
        acc, applied = decay_bookkeeping(acc, hp["lr"], hp["weight_decay"], hp["threshold"])
        for (off, ln), d in zip(segs, applied):
            if d > 0:
                want_p[off:off + ln] *= 1 - d
        got_p = flat.detach().cpu().numpy()
        np.testing.assert_allclose(got_p, want_p, rtol=1e-5, atol=1e-6)
        _check_moments(_bits(st["exp_avg"]), want_m.view(np.uint16), f"step {t + 1} exp_avg")
        _check_moments(_bits(st["exp_avg_sq"]), want_v.view(np.uint16), f"step {t + 1} exp_avg_sq")
        np.testing.assert_allclose(st["accumulated_decay"], acc, rtol=0, atol=1e-15)
        assert [a == 0.0 for a in st["accumulated_decay"]] == [d > 0 for d in applied]
        assert torch.equal(flat._uwu_bf16_shadow, flat.detach().bfloat16()) and not flat.grad.any()
        p_prev, m_prev, v_prev = got_p.copy(), _bits(st["exp_avg"]).copy(), _bits(st["exp_avg_sq"]).copy()
    assert np.isinf(v_prev.view(np.float16)).any() and np.isfinite(p_prev).all()


# ------------------------------------------------------------------------------------------------------------ Lion
def _check_lion(got_p, got_m, p_prev, g_eff, m_prev, lr, betas, wd, zero):
    want_p, want_m, c, mag = lion_step(p_prev, g_eff, m_prev, lr, betas, wd)
    # fp32 rounding of c is a few 2^-24 of |beta1 m| + |(1 - beta1) g|: outside this band the sign is determined
    out = np.abs(c) < 2.0 ** -20 * mag
    print(f"lion: {int(out.sum())} of {out.size} elements left out of the p comparison")
    assert out.sum() <= 1e-3 * out.size
    np.testing.assert_allclose(got_p[~out], want_p[~out], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(got_m, want_m, rtol=1e-5, atol=1e-7)
    assert not got_m[zero].any()
    np.testing.assert_allclose(got_p[zero], p_prev[zero].astype(np.float64) * (1 - lr * wd), rtol=1e-6, atol=0)


@pytest.mark.parametrize("wd,clipped", [(0.0, False), (0.1, True)])
def test_lion_matches_fp64(wd, clipped):
    from uwudiff_amd.optim import FusedLion

    n, lr, betas, pre = 100_003, 1e-3, (0.9, 0.99), 0.5
    rng = np.random.default_rng(5)
    zero = slice(40_001, 47_002)
    flat = torch.nn.Parameter(_dev(rng.standard_normal(n).astype(np.float32)))
    flat._uwu_bf16_shadow = torch.zeros(n, device="cuda", dtype=torch.bfloat16)
    opt = FusedLion([flat], lr=lr, betas=betas, weight_decay=wd)
    p_prev, m_prev = flat.detach().cpu().numpy().copy(), np.zeros(n, np.float32)
    for t in range(5):
        g = (rng.standard_normal(n) * (10.0 if t % 2 == 0 else 1e-3)).astype(np.float32)
        g[zero] = 0
        flat.grad = _dev(g)
        if clipped:  # Lightning's gradient_clip_val on the averaged gradient: g_eff = g * pre_scale * coefficient
            clip = opt.grad_norm_clip(1.0, pre_scale=pre)
            opt.step(clip=clip, pre_scale=pre, zero_grad=True)
            norm = math.sqrt(float((g.astype(np.float64) ** 2).sum())) * pre
            sq, coef = (float(x) for x in clip.cpu())
            assert sq == pytest.approx(norm * norm, rel=1e-5) and coef == pytest.approx(min(1.0, 1.0 / (norm + 1e-6)), rel=1e-5)
            # the restated gradient uses the factor the kernel multiplies by (its own coefficient, checked above), so that the
            # band below has only the kernel's fp32 arithmetic to cover
            g_eff = g.astype(np.float64) * float(np.float32(pre) * np.float32(coef))
        else:
            opt.step(zero_grad=True)
            g_eff = g
        torch.cuda.synchronize()
        got_p, got_m = flat.detach().cpu().numpy(), opt.state[flat]["exp_avg"].cpu().numpy()
        assert opt.state[flat]["exp_avg"].dtype == torch.float32
        _check_lion(got_p, got_m, p_prev, g_eff, m_prev, lr, betas, wd, zero)
        assert torch.equal(flat._uwu_bf16_shadow, flat.detach().bfloat16()) and not flat.grad.any()
        p_prev, m_prev = got_p.copy(), got_m.copy()


# ------------------------------------------------------------------------------------------------------------ edge shapes
S_P, S_G, S_M, S_V, S_SH = 7.0, 3.0, 5.0, 2.5, 9.0  # sentinels around the launched range
SHAPES = [(0, 1), (0, 5), (0, 8), (0, 100_003), (4, 3), (4, 7), (4, 4 * 515 + 3)]


def _edge_buffers(off, ln, seed):
    rng = np.random.default_rng(seed)
    N = off + ln + 9
    r = slice(off, off + ln)
    p = np.full(N, S_P, np.float32)
    g = np.full(N, S_G, np.float32)
    p[r] = rng.standard_normal(ln)
    g[r] = rng.standard_normal(ln) * 0.5
    return N, r, p, g, rng


def _outside_untouched(r, N, **bufs):
    out = np.ones(N, bool)
    out[r] = False
    for name, (t, sentinel) in bufs.items():
        a = t.detach().float().cpu().numpy()
        assert (a[out] == sentinel).all(), name


@pytest.mark.parametrize("off,ln", SHAPES)
@pytest.mark.parametrize("zero_grad", [0, 1])
def test_adamw_fp16_entry_point_edge_shapes(off, ln, zero_grad):
    from uwudiff_amd import lib as L

    N, r, p, g, rng = _edge_buffers(off, ln, 11)
    m = np.full(N, S_M, np.float16)
    v = np.full(N, S_V, np.float16)
    m[r] = (rng.standard_normal(ln) * 0.1).astype(np.float16)
    v[r] = (rng.standard_normal(ln) ** 2 * 1e-2).astype(np.float16)
    dp, dg, dm, dv = _dev(p), _dev(g), _dev(m), _dev(v)
    sh = torch.full((N,), S_SH, device="cuda", dtype=torch.bfloat16)
    lr, betas, eps, step = 1e-3, (0.9, 0.999), 1e-8, 3
    L.call("uwu_adamw_fp16_step", dp.data_ptr() + 4 * off, dg.data_ptr() + 4 * off, dm.data_ptr() + 2 * off,
           dv.data_ptr() + 2 * off, sh.data_ptr() + 2 * off, ln, lr, betas[0], betas[1], eps, step, 1.0, None, zero_grad,
           L.stream())
    torch.cuda.synchronize()
    want_p, want_m, want_v, _, _ = adamw_fp16_step(p[r], g[r], m[r], v[r], step, lr, betas, eps)
    np.testing.assert_allclose(dp.cpu().numpy()[r], want_p, rtol=1e-5, atol=1e-6)
    _check_moments(_bits(dm)[r], want_m.view(np.uint16), "exp_avg", exact_special=False)
    _check_moments(_bits(dv)[r], want_v.view(np.uint16), "exp_avg_sq", exact_special=False)
    assert torch.equal(sh[r], dp[r].bfloat16())
    assert np.array_equal(dg.cpu().numpy()[r], np.zeros(ln, np.float32) if zero_grad else g[r])
    _outside_untouched(r, N, p=(dp, S_P), g=(dg, S_G), m=(dm, S_M), v=(dv, S_V), shadow=(sh, S_SH))


@pytest.mark.parametrize("off,ln", SHAPES)
@pytest.mark.parametrize("zero_grad", [0, 1])
def test_lion_entry_point_edge_shapes(off, ln, zero_grad):
    from uwudiff_amd import lib as L

    N, r, p, g, rng = _edge_buffers(off, ln, 12)
    m = np.full(N, S_M, np.float32)
    m[r] = rng.standard_normal(ln) * 0.1
    dp, dg, dm = _dev(p), _dev(g), _dev(m)
    sh = torch.full((N,), S_SH, device="cuda", dtype=torch.bfloat16)
    lr, betas, wd = 1e-3, (0.9, 0.99), 0.1
    L.call("uwu_lion_step", dp.data_ptr() + 4 * off, dg.data_ptr() + 4 * off, dm.data_ptr() + 4 * off,
           sh.data_ptr() + 2 * off, ln, lr, betas[0], betas[1], wd, 1.0, None, zero_grad, L.stream())
    torch.cuda.synchronize()
    want_p, want_m, c, mag = lion_step(p[r], g[r], m[r], lr, betas, wd)
    keep = np.abs(c) >= 2.0 ** -20 * mag
    assert keep.sum() >= ln - max(1, ln // 1000)
    np.testing.assert_allclose(dp.cpu().numpy()[r][keep], want_p[keep], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(dm.cpu().numpy()[r], want_m, rtol=1e-5, atol=1e-7)
    assert torch.equal(sh[r], dp[r].bfloat16())
    assert np.array_equal(dg.cpu().numpy()[r], np.zeros(ln, np.float32) if zero_grad else g[r])
    _outside_untouched(r, N, p=(dp, S_P), g=(dg, S_G), m=(dm, S_M), shadow=(sh, S_SH))


@pytest.mark.parametrize("off,ln", SHAPES + [(1, 6), (3, 4 * 515 + 3)])
def test_param_decay_entry_point_edge_shapes(off, ln):
    from uwudiff_amd import lib as L

    N, r, p, _, _ = _edge_buffers(off, ln, 13)
    dp = _dev(p)
    sh = torch.full((N,), S_SH, device="cuda", dtype=torch.bfloat16)
    L.call("uwu_param_decay", dp.data_ptr() + 4 * off, sh.data_ptr() + 2 * off, ln, 1.0 - 0.0123, L.stream())
    torch.cuda.synchronize()
    np.testing.assert_allclose(dp.cpu().numpy()[r], p[r].astype(np.float64) * (1.0 - 0.0123), rtol=1e-6, atol=0)
    assert torch.equal(sh[r], dp[r].bfloat16())
    _outside_untouched(r, N, p=(dp, S_P), shadow=(sh, S_SH))
    L.call("uwu_param_decay", dp.data_ptr() + 4 * off, None, ln, 0.5, L.stream())  # no shadow
    torch.cuda.synchronize()
    np.testing.assert_allclose(dp.cpu().numpy()[r], p[r].astype(np.float64) * (1.0 - 0.0123) * 0.5, rtol=1e-6, atol=0)
    _outside_untouched(r, N, p=(dp, S_P), shadow=(sh, S_SH))


def test_entry_points_refuse_bad_arguments():
    from uwudiff_amd import lib as L

    a = torch.zeros(64, device="cuda")
    h = torch.zeros(64, device="cuda", dtype=torch.float16)
    with pytest.raises(L.UwuError):  # p not 16-byte aligned
        L.call("uwu_lion_step", a.data_ptr() + 4, a.data_ptr(), a.data_ptr(), None, 8, 1e-3, 0.9, 0.99, 0.0, 1.0, None, 0, L.stream())
    with pytest.raises(L.UwuError):  # the two fp16 moments at different offsets within 16 bytes
        L.call("uwu_adamw_fp16_step", a.data_ptr(), a.data_ptr(), h.data_ptr(), h.data_ptr() + 8, None, 8, 1e-3, 0.9, 0.999,
               1e-8, 1, 1.0, None, 0, L.stream())
    with pytest.raises(L.UwuError):  # step counts from 1
        L.call("uwu_adamw_fp16_step", a.data_ptr(), a.data_ptr(), h.data_ptr(), h.data_ptr(), None, 8, 1e-3, 0.9, 0.999, 1e-8,
               0, 1.0, None, 0, L.stream())
    with pytest.raises(L.UwuError):
        L.call("uwu_param_decay", None, None, 8, 0.5, L.stream())


# ------------------------------------------------------------------------------------------------------------ trainer
OPTS = {"lion": ("lion_pytorch.Lion", {"weight_decay": 0.1, "betas": [0.9, 0.99]}),
        # lr * weight_decay = 4e-3 per step: every tensor's accumulated decay crosses the threshold within three steps
        "adamw_fp16": ("duwu.trainer.optimizers.AdamWFP16", {"weight_decay": 4.0, "betas": [0.9, 0.999]})}


def _fit_cfg(tmp_path, opt, steps, clip=None, lyc=None):
    from uwudiff_amd.config import load_yaml, merge

    target, opt_config = OPTS[opt]
    over = {"lightning_config": {"fast_dev_run": False, "max_steps": steps, "log_every_n_steps": 1, "gradient_clip_val": clip,
                                 "default_root_dir": str(tmp_path)},
            "data": {"dataset_config": {"sample_size": [3, 32, 32], "n_samples": 8},
                     "dataloader_config": {"batch_size": 4, "num_workers": 0}},
            "trainer": {"lr": 1e-3, "optimizer": target, "opt_config": opt_config, "lycoris_config": lyc}}
    cfg = merge(load_yaml(os.path.join(ROOT, "configs", "demo_training.yaml")), over)
    lc = dict(cfg["lightning_config"])
    lc.pop("callbacks", None)
    return cfg, lc


def _fresh(tmp_path, opt, steps, clip=None, lyc=None):
    from duwu.loader import load_all
    from uwudiff_amd.engine import Fitter, seed_everything

    cfg, lc = _fit_cfg(tmp_path, opt, steps, clip, lyc)
    seed_everything(cfg.seed)
    fit = Fitter(**lc)
    dm, tr = load_all(cfg)
    return fit, dm, tr


@pytest.mark.parametrize("clip", [None, 1.0], ids=["noclip", "clip"])
@pytest.mark.parametrize("opt", sorted(OPTS))
def test_fitter_takes_the_fused_branch(tmp_path, opt, clip):
    from uwudiff_amd.optim import FlatFusedOptimizer, FusedAdamWFP16, FusedLion

    fit, dm, tr = _fresh(tmp_path, opt, 3, clip)
    flat0 = tr.unet.flat.detach().clone()
    calls = {"refresh": 0, "at_step": []}
    inner = tr.unet.refresh_shadow

    def counted():
        calls["refresh"] += 1
        return inner()

    tr.unet.refresh_shadow = counted

    def after_step(f):
        calls["at_step"].append(calls["refresh"])
        assert not tr.unet.flat.grad.any()  # left zeroed by the update kernel

    fit.step_hooks.append(after_step)
    hist = fit.fit(tr, dm)
    optim = fit._fit_state[1]
    assert isinstance(optim, FlatFusedOptimizer) and type(optim) is {"lion": FusedLion, "adamw_fp16": FusedAdamWFP16}[opt]
    assert fit.global_step == 3 and len(hist) == 3 and all(math.isfinite(h["loss"]) for h in hist)
    assert len(set(calls["at_step"])) == 1, calls  # no refresh_shadow() once the steps have begun: the kernel wrote the shadow
    flat = tr.unet.flat.detach()
    assert torch.isfinite(flat).all() and float((flat - flat0.to(flat.device)).abs().max()) > 0
    assert torch.equal(tr.unet.shadow, flat.bfloat16())
    st = optim.state[tr.unet.flat]
    if opt == "adamw_fp16":
        assert optim.segments == [(o, math.prod(s)) for o, s in tr.unet.P.registry.values()]
        assert st["exp_avg"].dtype == torch.float16 and st["exp_avg_sq"].dtype == torch.float16 and st["step"] == 3
        acc = st["accumulated_decay"]
        assert len(acc) == len(optim.segments) and all(type(a) is float and 0 <= a <= optim.decay_threshold for a in acc)
        assert any(a < 4e-3 for a in acc)  # tensors that decayed within the last step
    else:
        assert set(st) == {"exp_avg"} and st["exp_avg"].dtype == torch.float32


class ElementwiseDenoiser(FlatModule):
    """A stand-in denoiser with a bit-reproducible gradient: per-channel and per-pixel elementwise maps of the noisy input, written
    with torch ops on views of one flat parameter (their reductions add in a fixed order).  The UNet's and the DiT's weight
    gradients are not reproducible run to run (fp32 atomics of the bias / split-K reductions): measured on the MI355X, two
    uninterrupted 5-step fits of the tiny UNet from the same seeds differ on 1.29 M (Lion) / 6.67 M (AdamWFP16) of its 6.74 M
    parameters, so a bit-for-bit statement about a resumed run can only be made on a gradient that is itself bit-for-bit."""

    def __init__(self, config=None, channels=3, size=32):
        super().__init__()
        for name, shape in (("scale", (channels, 1, 1)), ("gate", (channels, 1, 1)), ("field", (channels, size, size)),
                            ("bias", (channels, 1, 1))):
            self.P.add(name, shape)
        self._alloc(bf16=True)
        with torch.no_grad():
            gen = torch.Generator().manual_seed(3)
            for name in self.P.registry:
                self.view(name).copy_(torch.randn(self.P.registry[name][1], generator=gen) * 0.3)

    def forward(self, x, timesteps, **kwargs):
        w = lambda name: self.P._view(self.flat, name)  # noqa: E731  (views of the parameter: autograd fills flat.grad)
        x = x.float()
        return (x * w("scale") + torch.tanh(x) * w("gate") + w("field") + w("bias"),)


def _resume_pair(tmp_path, opt, unet=None):
    """run A: 5 uninterrupted steps, checkpoint written after step 3; run B: fresh objects resumed from that file, steps 4-5.
    The RNG is re-seeded at the same point of both (the pattern of test_checkpoint_resume_reproduces_the_run)."""
    from duwu.loader import load_all
    from uwudiff_amd.config import merge
    from uwudiff_amd.engine import Fitter, seed_everything

    path = str(tmp_path / "step3.ckpt")

    def fresh():
        cfg, lc = _fit_cfg(tmp_path, opt, 5)
        if unet is not None:
            cfg = merge(cfg, {"trainer": {"model_config": {"unet": {"_target_": unet}}}})
        seed_everything(cfg.seed)
        fit = Fitter(**lc)
        dm, tr = load_all(cfg)
        return fit, dm, tr

    def save_at_3(f):
        if f.global_step == 3:
            f.save_checkpoint(path)
            seed_everything(777)

    fit, dm, tr = fresh()
    fit.step_hooks.append(save_at_3)
    fit.fit(tr, dm)
    fit2, dm2, tr2 = fresh()
    orig, loaded = fit2.load_checkpoint, {}

    def load_and_seed(p):
        out = orig(p)
        st = fit2._fit_state[1].state[tr2.unet.flat]
        loaded.update({k: v.clone() if torch.is_tensor(v) else (list(v) if isinstance(v, list) else v) for k, v in st.items()})
        loaded["flat"] = tr2.unet.flat.detach().clone()
        seed_everything(777)
        return out

    fit2.load_checkpoint = load_and_seed
    hist_b = fit2.fit(tr2, dm2, ckpt_path=path)
    assert fit.global_step == 5 and fit2.global_step == 5 and len(hist_b) == 2
    assert all(math.isfinite(h["loss"]) for h in hist_b)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    return (tr, fit._fit_state[1]), (tr2, fit2._fit_state[1]), loaded, ck


def _same_bits(a, b):
    view = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.dtype == b.dtype and torch.equal(a.cpu().view(view), b.cpu().view(view))


MOMENTS = {"lion": (("exp_avg",), torch.float32), "adamw_fp16": (("exp_avg", "exp_avg_sq"), torch.float16)}


@pytest.mark.parametrize("opt", sorted(OPTS))
def test_checkpoint_resume_is_bit_identical(tmp_path, opt):
    """Checkpoint after step 3, resume in fresh objects, steps 4-5: parameters, moments (fp16 kept) and accumulated_decay equal
    the uninterrupted run's bit for bit (on the denoiser whose gradient is bit-reproducible: see ElementwiseDenoiser)."""
    (tr, opt_a), (tr2, opt_b), loaded, ck = _resume_pair(tmp_path, opt, unet=f"{ElementwiseDenoiser.__module__}.ElementwiseDenoiser")
    assert isinstance(tr.unet, ElementwiseDenoiser) and isinstance(tr2.unet, ElementwiseDenoiser)
    st_a, st_b = opt_a.state[tr.unet.flat], opt_b.state[tr2.unet.flat]
    diff = (tr2.unet.flat.detach() - tr.unet.flat.detach()).abs()
    print(f"{opt}: resumed parameters differ on {int((diff > 0).sum())} of {diff.numel()} elements, max {float(diff.max()):.3e}")
    assert float((loaded["flat"] - tr2.unet.flat.detach()).abs().max()) > 0  # steps 4-5 did move them
    assert _same_bits(tr2.unet.flat.detach(), tr.unet.flat.detach())
    names, dtype = MOMENTS[opt]
    for k in names:
        assert st_b[k].dtype == dtype and _same_bits(st_b[k], st_a[k]), k
        assert st_b[k].float().abs().max() > 0
    if opt == "adamw_fp16":
        assert st_b["accumulated_decay"] == st_a["accumulated_decay"] and st_b["step"] == st_a["step"] == 5
        assert len(st_b["accumulated_decay"]) == 4 and all(type(a) is float for a in st_b["accumulated_decay"])
        assert loaded["accumulated_decay"] != st_b["accumulated_decay"]
    assert torch.equal(tr2.unet.shadow, tr2.unet.flat.detach().bfloat16())


@pytest.mark.parametrize("opt", sorted(OPTS))
def test_resumed_state_is_the_checkpoint(tmp_path, opt):
    """On the tiny UNet: what a resumed run starts from is the file's content bit for bit -- parameters, moments in their
    dtype, step count and accumulated_decay -- and it goes on to take steps 4-5."""
    (tr, opt_a), (tr2, opt_b), loaded, ck = _resume_pair(tmp_path, opt)
    ck_st = ck["optimizer_states"][0]["state"][0]
    names, dtype = MOMENTS[opt]
    for k in names:
        assert ck_st[k].dtype == dtype and _same_bits(loaded[k], ck_st[k]), k
    if opt == "adamw_fp16":
        assert ck_st["step"] == loaded["step"] == 3
        assert isinstance(ck_st["accumulated_decay"], list) and loaded["accumulated_decay"] == ck_st["accumulated_decay"]
        assert len(ck_st["accumulated_decay"]) == len(tr2.unet.P.registry)
    sd = {k[len("unet."):]: v for k, v in ck["state_dict"].items() if k.startswith("unet.")}
    end = tr2.unet.flat.detach().clone()
    assert torch.isfinite(end).all() and float((end - loaded["flat"]).abs().max()) > 0  # steps 4-5 were taken from there
    tr2.unet.flat.data.copy_(loaded["flat"])
    for k, v in tr2.unet.state_dict().items():
        assert _same_bits(v, sd[k]), k
    assert opt_b.state[tr2.unet.flat][names[0]].dtype == dtype


def test_lycoris_adapters_train_under_lion(tmp_path):
    from uwudiff_amd.optim import FusedLion

    fit, dm, tr = _fresh(tmp_path, "lion", 2, clip=1.0, lyc=TOML)
    base0 = tr.unet.flat.detach().clone()
    ad0 = tr.lycoris_model.flat.detach().clone()

    def after_step(f):
        assert not tr.lycoris_model.flat.grad.any()

    fit.step_hooks.append(after_step)
    hist = fit.fit(tr, dm)
    optim = fit._fit_state[1]
    assert type(optim) is FusedLion and list(optim.state) == [tr.lycoris_model.flat]
    assert fit.global_step == 2 and all(math.isfinite(h["loss"]) for h in hist)
    assert float((tr.lycoris_model.flat.detach() - ad0.to(tr.lycoris_model.flat.device)).abs().max()) > 0
    assert torch.equal(tr.unet.flat.detach().cpu(), base0.cpu()) and tr.unet.flat.grad is None
    # the shadow holds W + dW for the adapted tensors (the UNet's merge); every other tensor's shadow is still the base's
    adapted = set(tr.unet.P.ad.names)
    base16 = base0.to(tr.unet.flat.device).bfloat16()
    untouched = [(o, math.prod(s)) for nm, (o, s) in tr.unet.P.registry.items() if nm not in adapted]
    assert adapted and untouched
    for o, ln in untouched:
        assert torch.equal(tr.unet.shadow[o:o + ln], base16[o:o + ln])
