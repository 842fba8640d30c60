"""GPU: where an element sits in a launch never changes its bits (the rounding contract of csrc/optimizer_shared.h).

Every flat-buffer optimizer kernel runs the same 1024 element tuples twice through its C entry point: once as one launch with
n = 1024, where every element goes through the 16-byte vector body, and once three at a time (n = 3 at element offsets 4k), where
every element goes through the scalar tail -- for AdamWFP16 the fp16 state then starts 8 bytes past a 16-byte boundary at every odd
k, so those launches take the peeled head instead.  p, every state array, the bf16 shadow and the zeroed gradient must come out
equal as integers.  The 8-bit kernels run n = 1024 + 3: the ragged lanes of the last block against the same values in a full block
padded with zeros (the same block maximum).

The tuples: normal draws at gradient scale 1e-3, then rows of zeros, subnormals and +-large values in every column; for Lion and
Lion8 the first 256 rows put c = b1*m + (1-b1)*g at zero or within an ulp of it (g = -b1*m/(1-b1) rounded, and its two fp32
neighbours), where a product rounded in one path and fused in the other flips sign(c) and moves p by 2*lr.

Each case prints how many rows differ per column before it asserts."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 1024
GROUPS = -(-N // 3)  # scalar launches: three tuples each, the last one the remainder
SLOT = torch.tensor([4 * (t // 3) + t % 3 for t in range(N)])
SENTINEL = 7  # what the fourth slot of every group holds: no launch may touch it
LR, B1, B2, EPS, WD, STEP = 1e-3, 0.9, 0.999, 1e-8, 1e-2, 3
PRE, CLIP = 0.5, 0.37  # gscale = fp32(0.5 * 0.37), formed on the device


def _columns(seed):
    """p, g, m, v: rows 0..255 and 512.. ordinary draws, rows 256..511 cycle through zeros, subnormals and large values with
    coprime periods, so the columns meet in many combinations"""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(N, generator=gen)
    g = torch.randn(N, generator=gen) * 1e-3
    m = torch.randn(N, generator=gen) * 1e-3
    v = (torch.randn(N, generator=gen) * 1e-3) ** 2
    special = {
        "p": [0.0, -0.0, 1e-40, -1e-40, 3e15, -3e15, 1.0],
        "g": [0.0, 1e-40, -1e-40, 3e4, -3e4, 1e-3, -0.0, 1e-7, 2e-42, -5.0, 1e-30],
        "m": [0.0, 1e-40, -1e-42, 2e4, -2e4, 1e-7, -1e-3, 6e4, -1e-7, 1e-38, -0.0, 3.0, 1e-20],
        "v": [0.0, 1e-40, 1e-44, 4e8, 6e4, 1e-7, 1e-6, 1e-38, 9e-16],
    }
    for name, col in (("p", p), ("g", g), ("m", m), ("v", v)):
        vals = special[name]
        col[256:512] = torch.tensor([vals[i % len(vals)] for i in range(256)], dtype=torch.float64).float()
    return p, g, m, v


def _near_zero_c(m, b1, omb1):
    """g such that b1*m + omb1*g is zero or within an ulp of it, for fp32 b1, omb1 and m: the rounded root and its two neighbours"""
    m = m.numpy().astype(np.float32)
    g0 = (-(np.float64(b1) * m.astype(np.float64)) / np.float64(omb1)).astype(np.float32)
    up, down = np.nextafter(g0, np.float32(np.inf)), np.nextafter(g0, np.float32(-np.inf))
    pick = np.arange(m.size) % 3
    return torch.from_numpy(np.where(pick == 0, g0, np.where(pick == 1, up, down)))


def _ints(t):
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _both_ways(name, cols, launch):
    """cols: column name -> N host values; launch(ptrs, n) runs the entry point on n elements from the device pointers `ptrs`"""
    body = {k: v.cuda() for k, v in cols.items()}
    launch({k: t.data_ptr() for k, t in body.items()}, N)
    slot = SLOT.cuda()
    tail = {}
    for k, v in cols.items():
        t = torch.full((4 * GROUPS,), SENTINEL, dtype=v.dtype)
        t[SLOT] = v
        tail[k] = t.cuda()
    for q in range(GROUPS):
        launch({k: t.data_ptr() + 4 * q * t.element_size() for k, t in tail.items()}, min(3, N - 3 * q))
    torch.cuda.synchronize()
    differ = {}
    for k in cols:
        assert (tail[k][3::4] == SENTINEL).all(), f"{name}: {k} written outside the launch"
        bad = (_ints(tail[k][slot]) != _ints(body[k])).nonzero().flatten()
        differ[k] = bad.numel()
        if bad.numel():
            print(f"{name}: {k} differs in {bad.numel()} of {N} rows, first {bad[:8].tolist()}")
    print(f"{name}: rows that differ between the vector body and the scalar path: {differ}")
    assert not any(differ.values()), (name, differ)


def _clip(coef=CLIP):
    return torch.tensor([123.0, coef], device="cuda")


def _shadow():
    return torch.full((N,), float(SENTINEL), dtype=torch.bfloat16)


def test_adamw():
    from uwudiff_amd import lib as L

    p, g, m, v = _columns(1)
    clip = _clip()
    _both_ways("uwu_adamw_step", dict(p=p, g=g, m=m, v=v, sh=_shadow()), lambda P, n: L.call(
        "uwu_adamw_step", P["p"], P["g"], P["m"], P["v"], P["sh"], n, LR, B1, B2, EPS, WD, STEP, PRE, L.ptr(clip), 1, L.stream()))


def test_lion():
    from uwudiff_amd import lib as L

    p, g, m, _ = _columns(2)
    g[:256] = _near_zero_c(m[:256], np.float32(B1), np.float32(1.0 - B1))
    clip = _clip(1.0)  # gscale = 1: the kernel sees the constructed g itself
    _both_ways("uwu_lion_step", dict(p=p, g=g, m=m, sh=_shadow()), lambda P, n: L.call(
        "uwu_lion_step", P["p"], P["g"], P["m"], P["sh"], n, LR, B1, 0.99, WD, 1.0, L.ptr(clip), 1, L.stream()))


def test_adamw_fp16():
    from uwudiff_amd import lib as L

    p, g, m, v = _columns(3)
    clip = _clip()
    cols = dict(p=p, g=g, m=m.clamp(-6e4, 6e4).half(), v=v.clamp(max=6e4).half(), sh=_shadow())
    _both_ways("uwu_adamw_fp16_step", cols, lambda P, n: L.call(
        "uwu_adamw_fp16_step", P["p"], P["g"], P["m"], P["v"], P["sh"], n, LR, B1, B2, EPS, STEP, PRE, L.ptr(clip), 1, L.stream()))


def test_param_decay():
    from uwudiff_amd import lib as L

    p = _columns(4)[0]
    _both_ways("uwu_param_decay", dict(p=p, sh=_shadow()),
               lambda P, n: L.call("uwu_param_decay", P["p"], P["sh"], n, 1.0 - 0.0123, L.stream()))


@pytest.mark.parametrize("c", [0.25, 0.75])  # torch.lerp's two branches
def test_sfadamw(c):
    from uwudiff_amd import lib as L

    y, g, z, v = _columns(5)
    z = z + y  # the two sequences stay near each other
    clip = _clip()
    bc2 = 1.0 - B2 ** STEP
    _both_ways(f"uwu_sfadamw_step c={c}", dict(y=y, g=g, z=z, v=v, sh=_shadow()), lambda P, n: L.call(
        "uwu_sfadamw_step", P["y"], P["g"], P["z"], P["v"], P["sh"], n, LR, B1, B2, EPS, WD, c, bc2, PRE, L.ptr(clip), 1,
        L.stream()))


@pytest.mark.parametrize("weight", [1.0 - 1.0 / B1, 0.75])
def test_sf_average(weight):
    from uwudiff_amd import lib as L

    y, _, z, _ = _columns(6)
    _both_ways(f"uwu_sf_average w={weight:.3f}", dict(y=y, z=z + y, out=torch.zeros(N)),
               lambda P, n: L.call("uwu_sf_average", P["y"], P["z"], P["out"], n, weight, L.stream()))


def test_ema_update():
    from uwudiff_amd import lib as L

    p, _, avg, _ = _columns(7)
    _both_ways("uwu_ema_update", dict(avg=avg + p, p=p),
               lambda P, n: L.call("uwu_ema_update", P["avg"], P["p"], n, 0.999, 1.0 - 0.999, L.stream()))


def test_prodigy_stats():
    from uwudiff_amd import lib as L

    p, g, m, v = _columns(8)
    s, p0 = _columns(9)[2], p + _columns(9)[1]
    d0 = 1e-6
    scal = torch.tensor([d0, d0, 0.0, 0.0, 0.0, 2.0, 0.0, 0.0], dtype=torch.float64, device="cuda")  # d, d_max, ..., k = 2
    ws = torch.zeros(16, dtype=torch.float64, device="cuda")
    clip = _clip()
    # coupled weight decay: the gradient carries wd * p, the second product next to gscale * g
    _both_ways("uwu_prodigy_stats", dict(p=p, g=g, p0=p0, m=m, v=v, s=s), lambda P, n: L.call(
        "uwu_prodigy_stats", P["p"], P["g"], P["p0"], P["m"], P["v"], P["s"], n, L.ptr(scal), L.ptr(ws), ws.numel() // 2, 0, 1.0,
        B1, B2, math.sqrt(B2), WD, 0, d0, 1, 0, PRE, L.ptr(clip), 1, L.stream()))


def test_prodigy_apply():
    from uwudiff_amd import lib as L

    p, _, m, v = _columns(10)
    scal = torch.tensor([3e-4, 3e-4, 0.0, 1.0, 3e-4, 2.0, 0.0, 2.9e-4], dtype=torch.float64, device="cuda")  # not skipped; dlr last
    _both_ways("uwu_prodigy_apply", dict(p=p, m=m, v=v, sh=_shadow()), lambda P, n: L.call(
        "uwu_prodigy_apply", P["p"], P["m"], P["v"], P["sh"], n, L.ptr(scal), EPS, WD, 1, L.stream()))


@pytest.mark.parametrize("kind", ["adamw8", "lion8"])
def test_8bit_ragged_block(kind):
    """n = 1024 + 3: lane 0 of the last block holds three elements and takes the element-wise path; in a buffer padded with zeros
    to 1280 the same lane holds four and takes the vector path, and the block maximum is the same"""
    from uwudiff_amd import lib as L
    from uwudiff_amd.optim import dynamic_map

    n, full = N + 3, N + 256
    t1, t2 = dynamic_map(True), dynamic_map(False)
    z1, z2 = int((t1 == 0).nonzero()), int((t2 == 0).nonzero())  # the codes that read as 0
    gen = torch.Generator().manual_seed(11)
    p, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 1e-3
    c1 = torch.randint(0, 256, (n,), generator=gen, dtype=torch.uint8)
    c2 = torch.randint(0, 256, (n,), generator=gen, dtype=torch.uint8)
    a1 = torch.rand(5, generator=gen) * 1e-2 + 1e-4
    a2 = torch.rand(5, generator=gen) * 1e-5 + 1e-8
    p[256:512], g[256:512] = _columns(12)[0][256:512], _columns(12)[1][256:512]
    lion = kind == "lion8"
    if lion:  # the first 256 rows and the three ragged ones: c at zero or within an ulp of it, from the moment as the kernel decodes it
        m = t1[c1.long()] * a1[torch.arange(n) // 256]  # one fp32 product, as on the device
        near = _near_zero_c(m, np.float32(B1), np.float32(1.0 - B1))
        g[:256], g[N:] = near[:256], near[N:]
    clip = _clip(1.0 if lion else CLIP)
    pre = 1.0 if lion else PRE
    q1, q2 = t1.cuda(), t2.cuda()

    def run(length):
        pad = length - n
        dev = dict(p=torch.cat([p, torch.zeros(pad)]), g=torch.cat([g, torch.zeros(pad)]),
                   c1=torch.cat([c1, torch.full((pad,), z1, dtype=torch.uint8)]),
                   c2=torch.cat([c2, torch.full((pad,), z2, dtype=torch.uint8)]), a1=a1.clone(), a2=a2.clone(),
                   sh=torch.full((length,), float(SENTINEL), dtype=torch.bfloat16))
        dev = {k: v.cuda() for k, v in dev.items()}
        if lion:
            L.call("uwu_lion8_step", L.ptr(dev["p"]), L.ptr(dev["g"]), L.ptr(dev["c1"]), L.ptr(dev["a1"]), L.ptr(q1), L.ptr(dev["sh"]),
                   length, 0, length, LR, B1, 0.99, WD, pre, L.ptr(clip), 1, L.stream())
        else:
            L.call("uwu_adamw8_step", L.ptr(dev["p"]), L.ptr(dev["g"]), L.ptr(dev["c1"]), L.ptr(dev["c2"]), L.ptr(dev["a1"]),
                   L.ptr(dev["a2"]), L.ptr(q1), L.ptr(q2), L.ptr(dev["sh"]), length, 0, length, LR, B1, B2, EPS, WD, STEP, pre,
                   L.ptr(clip), 1, L.stream())
        torch.cuda.synchronize()
        return dev

    ragged, padded = run(n), run(full)
    differ = {}
    for k in ragged:
        keep = 5 if k in ("a1", "a2") else n
        differ[k] = int((_ints(ragged[k][:keep]) != _ints(padded[k][:keep])).sum())
    print(f"{kind}: elements that differ between the ragged and the padded last block: {differ}")
    assert not any(differ.values()), differ
    assert (padded["p"][n:] == 0).all()  # the padding stayed out of the block maximum
