"""GPU: the schedule-free AdamW kernels (csrc/optimizer.hip: uwu_sfadamw_step, uwu_sf_average) through
uwudiff_amd.optim.FusedAdamWScheduleFree, one step at a time against the fp64 restatement of tests/test_schedulefree_cpu.py under
bounds derived from the kernel's own rounding count (K_y, K_z, K_v next to sfadamw_elem), bit-identity under chunking, the two
modes (x within a derived bound, y back bit for bit) and the entry points' refusals.  DESIGN.md section 4.42."""
import numpy as np
import pytest
import torch

from tests.test_schedulefree_cpu import fresh_scalars, sf_average, sf_scalars, sf_step

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -24  # the unit roundoff of fp32
K_Y, K_Z, K_V = 16, 16, 8  # fp32 roundings on each output's path (csrc/optimizer.hip, at sfadamw_elem)
G = 8  # guard elements either side of every buffer (32 bytes: the launched range stays 16-byte aligned)
S_Y, S_G, S_Z, S_V, S_SH = 7.0, 5.0, 3.0, 11.0, 9.0  # what the guards hold
SIZES = [1, 3, 4, 5, 259, 1027, 2 ** 20 + 3]  # tail only, no tail, one vector and a tail, more than one grid-stride trip
HP = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, warmup_steps=4, r=0.5, weight_lr_power=2.0)
# shadow, zero_grad, clip coefficient (None: no clip tensor), pre_scale, weight_decay, k (0: c = 1; 2: inside warm-up; 7: past it)
COMBOS = {"k0_shadow_zero_clip_wd": (True, True, 0.37, 0.25, 0.1, 0),
          "warmup_plain": (False, False, None, 1.0, 0.0, 2),
          "past_shadow_clip_wd": (True, False, 0.37, 0.25, 0.1, 7),
          "k0_zero_wd": (False, True, None, 1.0, 0.1, 0)}


def _bits(t):
    view = {2: torch.int16, 4: torch.int32}[t.element_size()]
    return t.detach().cpu().contiguous().view(view)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _inputs(n, seed):
    """y, g, z, v as fp32: magnitudes of g from 1e-6 to 1e3 with v of the matching scale, and every fifth element (from index 2)
    an exact zero of g on v = 0, where the denominator is eps alone"""
    rng = np.random.default_rng(seed)
    g = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6, 3, n)
    v = (g * 10.0 ** rng.uniform(-1, 1, n)) ** 2
    y = rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 1, n)
    z = y + rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 0, n)
    g[2::5], v[2::5] = 0.0, 0.0
    return tuple(a.astype(np.float32) for a in (y, g, z, v))


def _scalars_at(k, **hp):
    sc = fresh_scalars()
    for _ in range(k):
        sc, _ = sf_scalars(sc, **hp)
    return sc


class Rig:
    """One parameter of n elements inside guarded buffers, with the optimizer's state set by hand and its scalars as after k steps"""

    def __init__(self, n, y, g, z, v, shadow=True, k=0, weight_decay=0.0):
        from uwudiff_amd.optim import FusedAdamWScheduleFree

        self.n = n

        def guarded(a, sentinel, dtype=torch.float32):
            buf = torch.full((n + 2 * G,), sentinel, device="cuda", dtype=dtype)
            if a is not None:
                buf[G:G + n] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
            return buf

        self.buf = {"y": guarded(y, S_Y), "g": guarded(g, S_G), "z": guarded(z, S_Z), "v": guarded(v, S_V)}
        self.sentinel = {"y": S_Y, "g": S_G, "z": S_Z, "v": S_V, "sh": S_SH}
        self.p = torch.nn.Parameter(self.buf["y"][G:G + n])
        self.p.grad = self.buf["g"][G:G + n]
        if shadow:
            self.buf["sh"] = guarded(None, S_SH, torch.bfloat16)
            self.buf["sh"][G:G + n] = self.p.data.bfloat16()
            self.p._uwu_bf16_shadow = self.buf["sh"][G:G + n]
        self.hp = dict(HP, weight_decay=weight_decay)
        self.opt = FusedAdamWScheduleFree([self.p], **self.hp)
        self.opt.state[self.p] = {"z": self.buf["z"][G:G + n], "exp_avg_sq": self.buf["v"][G:G + n]}
        self.sc = _scalars_at(k, **self.hp)
        self.opt.param_groups[0].update(self.sc)
        self.opt.train()

    def get(self, name):
        return self.buf[name][G:G + self.n].detach().clone()

    def f64(self, name):
        return self.get(name).double().cpu().numpy()

    def set_grad(self, g):
        self.buf["g"][G:G + self.n] = torch.from_numpy(np.ascontiguousarray(g)).cuda()

    def guards_intact(self):
        for name, buf in self.buf.items():
            s = self.sentinel[name]
            assert bool((buf[:G].float() == s).all()) and bool((buf[G + self.n:].float() == s).all()), f"{name}: written outside [0, n)"

    def check_step(self, before, gscale, what):
        """the kernel's step from `before` (fp64 copies of y, g, z, v and the scalars) against the oracle's, under the derived bounds"""
        y0, g0, z0, v0, sc0 = before
        wy, wz, wv, sc, info = sf_step(y0, g0 * gscale, z0, v0, sc0, **self.hp)
        lr_t, gn = info["lr_t"], np.abs(info["gn"])
        scale = np.abs(y0) + np.abs(z0) + lr_t * gn
        ratios = {}
        for name, want, bound in (("y", wy, K_Y * ULP * scale), ("z", wz, K_Z * ULP * scale), ("v", wv, K_V * ULP * np.abs(wv))):
            err = np.abs(self.f64(name) - want)
            ok = err <= bound
            ratios[name] = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
            assert ok.all(), f"{what}: {name} off at {int(np.argmax(~ok))}: err {err[~ok].max():.3e}, ratio {ratios[name]:.3f}"
        print(f"{what}: largest error / bound: y {ratios['y']:.3f}, z {ratios['z']:.3f}, v {ratios['v']:.3f}")
        g = self.opt.param_groups[0]
        assert (g["k"], g["weight_sum"], g["lr_max"], g["scheduled_lr"]) == (sc["k"], sc["weight_sum"], sc["lr_max"], sc["scheduled_lr"])
        return sc, info


@pytest.mark.parametrize("combo", sorted(COMBOS))
@pytest.mark.parametrize("n", SIZES)
def test_one_step_against_the_oracle(n, combo):
    shadow, zero_grad, coef, pre_scale, wd, k = COMBOS[combo]
    y, g, z, v = _inputs(n, seed=n % 1000 + k)
    rig = Rig(n, y, g, z, v, shadow=shadow, k=k, weight_decay=wd)
    clip = torch.tensor([123.0, coef], device="cuda", dtype=torch.float32) if coef is not None else None
    gscale = pre_scale * float(np.float32(coef)) if coef is not None else pre_scale
    before = tuple(a.astype(np.float64) for a in (y, g, z, v)) + (rig.sc,)
    rig.opt.step(clip=clip, pre_scale=pre_scale, zero_grad=zero_grad)
    torch.cuda.synchronize()
    sc, info = rig.check_step(before, gscale, f"n {n} {combo}")
    if k == 0:
        # c = 1: lerp(y, z, 1) is exactly z and a = -lr_t, so y = z + a*gn from z alone, the very expression of the new z (y != z before)
        assert info["c"] == 1.0 and (n < 3 or not np.array_equal(y, z))
        assert _same_bits(rig.get("y"), rig.get("z"))
    else:
        assert 0.0 < info["c"] < 1.0 and (n < 3 or not _same_bits(rig.get("y"), rig.get("z")))
    if shadow:
        assert _same_bits(rig.get("sh"), rig.get("y").bfloat16())
    grad = rig.get("g")
    assert (not grad.any()) if zero_grad else _same_bits(grad, torch.from_numpy(g).cuda())
    rig.guards_intact()
    if clip is not None:
        assert clip.tolist() == [123.0, float(np.float32(coef))]


def test_six_steps_on_the_kernels_own_state():
    """each step against the oracle applied to the kernel's previous state: across the warm-up (4 steps), weight decay on"""
    n = 1027
    y, g, z, v = _inputs(n, seed=11)
    z = y.copy()  # a fresh optimizer: z starts as the parameter
    rig = Rig(n, y, g, z, np.zeros(n, np.float32), shadow=True, k=0, weight_decay=0.1)
    rng = np.random.default_rng(12)
    sc = rig.sc
    for step in range(6):
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 1, n)).astype(np.float32)
        rig.set_grad(g)
        before = (rig.f64("y"), g.astype(np.float64), rig.f64("z"), rig.f64("v"), sc)
        rig.opt.step(pre_scale=0.5, zero_grad=True)
        sc, info = rig.check_step(before, 0.5, f"step {step + 1}")
        assert sc["k"] == step + 1 and not rig.get("g").any() and _same_bits(rig.get("sh"), rig.get("y").bfloat16())
    assert info["lr_t"] == HP["lr"] and 0 < info["c"] < 1
    rig.guards_intact()


def test_chunked_launches_give_the_same_bits():
    n = 1027
    y, g, z, v = _inputs(n, seed=21)
    out = []
    for chunks in (None, [(0, 4), (4, 60), (64, n - 64)]):
        rig = Rig(n, y, g, z, v, shadow=True, k=5, weight_decay=0.1)
        rig.opt.step(pre_scale=0.25, chunks=chunks, zero_grad=True)
        out.append({k: rig.get(k) for k in ("y", "z", "v", "sh", "g")})
        rig.guards_intact()
        assert rig.opt.param_groups[0]["k"] == 6  # once per step, not once per chunk
    assert not _same_bits(out[0]["y"], torch.from_numpy(y).cuda())
    for k in ("y", "z", "v", "sh", "g"):
        assert _same_bits(out[0][k], out[1][k]), k


@pytest.mark.parametrize("shadow", [True, False], ids=["shadow", "noshadow"])
@pytest.mark.parametrize("n", [5, 1027])
def test_eval_gives_x_and_train_restores_y_bit_for_bit(n, shadow):
    y, g, z, v = _inputs(n, seed=31)
    rig = Rig(n, y, g, z, v, shadow=shadow, k=3, weight_decay=0.1)
    opt, p = rig.opt, rig.p
    opt.step()
    y1, z1, v1 = rig.get("y"), rig.get("z"), rig.get("v")
    assert opt.held_weights(p) is None
    for _ in range(2):  # idempotent
        opt.eval()
        assert opt.param_groups[0]["train_mode"] is False
        x = rig.get("y")
        want = sf_average(y1.double().cpu().numpy(), z1.double().cpu().numpy(), 0.9)
        w = abs(1 - 1 / 0.9)
        # x = fma(w, z - y, y): z - y rounds once (on |y| + |z|, times |w|), w once (on |w||z - y|), the fma once (on |x|)
        bound = ULP * (2 * w * (y1.double().abs() + z1.double().abs()).cpu().numpy() + np.abs(want))
        err = np.abs(x.double().cpu().numpy() - want)
        print(f"n {n}: x, largest error / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all() and not _same_bits(x, y1)
        assert _same_bits(opt.held_weights(p), y1)  # y is kept aside
        assert _same_bits(rig.get("z"), z1) and _same_bits(rig.get("v"), v1)
        if shadow:
            assert _same_bits(rig.get("sh"), x.bfloat16())
    with pytest.raises(RuntimeError, match="train mode"):
        opt.step()
    assert opt.param_groups[0]["k"] == 4 and _same_bits(rig.get("y"), x)
    for _ in range(2):
        opt.train()
        assert opt.param_groups[0]["train_mode"] is True and opt.held_weights(p) is None
        assert _same_bits(rig.get("y"), y1) and _same_bits(rig.get("z"), z1) and _same_bits(rig.get("v"), v1)
        if shadow:
            assert _same_bits(rig.get("sh"), y1.bfloat16())
    rig.guards_intact()
    opt.step()  # and training goes on
    assert opt.param_groups[0]["k"] == 5


def test_sf_average_edge_shapes():
    """the kernel alone, out of place: every size, the second branch of lerp (w >= 0.5) too, w = 1 exactly z, nothing outside [0, n)"""
    from uwudiff_amd import lib as L

    for n in SIZES[:-1]:
        y, _, z, _ = _inputs(n, seed=41 + n)
        dy, dz = torch.from_numpy(y).cuda(), torch.from_numpy(z).cuda()
        for w in (1 - 1 / 0.9, 0.75, 1.0):
            out = torch.full((n + 2 * G,), S_Y, device="cuda")
            L.call("uwu_sf_average", L.ptr(dy), L.ptr(dz), out.data_ptr() + 4 * G, n, w, L.stream())
            got = out[G:G + n]
            if w == 1.0:
                assert _same_bits(got, dz)
            else:
                wf = float(np.float32(w))
                want = y.astype(np.float64) + wf * (z.astype(np.float64) - y) if w < 0.5 else z - (z.astype(np.float64) - y) * (1 - wf)
                bound = ULP * (3 * (np.abs(y) + np.abs(z)).astype(np.float64) + np.abs(want))
                assert (np.abs(got.double().cpu().numpy() - want) <= bound).all()
            assert bool((out[:G] == S_Y).all()) and bool((out[G + n:] == S_Y).all())
            assert _same_bits(dy, torch.from_numpy(y).cuda()) and _same_bits(dz, torch.from_numpy(z).cuda())


def test_entry_points_refuse_bad_arguments():
    from uwudiff_amd import lib as L

    a = [torch.full((64,), float(i + 1), device="cuda") for i in range(4)]
    sh = torch.full((64,), 2.0, device="cuda", dtype=torch.bfloat16)
    y, g, z, v = (t.data_ptr() for t in a)
    s = L.stream()
    tail = (1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1e-3, 1.0, None, 1, s)
    for bad in ((y + 4, g, z, v, None, 8), (y, g + 4, z, v, None, 8), (y, g, z + 4, v, None, 8), (y, g, z, v + 4, None, 8),
                (y, g, z, v, sh.data_ptr() + 2, 8), (y, g, z, v, None, 0), (None, g, z, v, None, 8), (y, g, None, v, None, 8)):
        with pytest.raises(L.UwuError):
            L.call("uwu_sfadamw_step", *bad, *tail)
    for bad in ((y + 4, z, v, 8), (y, z + 4, v, 8), (y, z, v + 4, 8), (y, z, v, 0), (y, None, v, 8)):
        with pytest.raises(L.UwuError):
            L.call("uwu_sf_average", *bad, 0.5, s)
    with pytest.raises(L.UwuError):  # a CPU tensor never reaches a launch
        L.ptr(torch.zeros(8))
    from uwudiff_amd.optim import FusedAdamWScheduleFree

    p = torch.nn.Parameter(torch.zeros(8))
    p.grad = torch.ones(8)
    opt = FusedAdamWScheduleFree([p])
    opt.train()
    with pytest.raises(L.UwuError):
        opt.step()
    assert opt.param_groups[0]["k"] == 0 and not p.detach().any()
    torch.cuda.synchronize()
    for i, t in enumerate(a):  # no launch happened
        assert bool((t == float(i + 1)).all())
    assert bool((sh.float() == 2.0).all())
