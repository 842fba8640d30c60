"""Every LayerNorm kernel branch of csrc/norm.hip against a float64 reference, on rows that are hard for LayerNorm.

Reference (tests/layernorm_oracle.py, checked against torch.autograd by tests/test_layernorm_ref_cpu.py): the two-pass
formulas of include/uwu_hip.h in float64 on the rounded inputs the device gets.  Two contract points:
  * bf16: the kernel stores and normalises the bf16-rounded residual stream.  An fp32 and an fp64 evaluation of x + gate*y
    round a few elements in a million to different bf16 neighbours, so x_out must be ONE OF THE TWO bf16 neighbours of the
    fp64 value, and the reference h / mean / rstd are computed from the device's own x_out.
  * backward: the reference uses, in fp64, exactly the mean / rstd tensors handed to the kernel; every case runs once with the
    forward kernel's statistics and once with fp64 statistics rounded to fp32 (which isolates the backward).

Bars.  E32 = max over the tensor of |the same formulas in torch fp32 on the CPU - fp64|.  Per element
    |got - ref| <= 4 * max(E32, 2^-23 * A) + (bf16 output ? 2^-8 * |ref| : 0)
with A = the absolute sum of the terms for the column sums (dshift, dscale, dgate) and max |ref| for elementwise outputs.
rstd, dx and dy are ~1000x larger on the all-zero rows (rstd = eps^-1/2), so those rows ("name[0]") and the other rows are
each held to the E32 and A of their own rows.
2^-23 A is a two-ulp floor (bf16 inputs make E32 of dshift nearly zero); the margin of 4 covers summation order only (the
kernels: a lane tree, an LDS fold, atomics in arbitrary order; torch: pairwise sums).  The worst measured ratio
(|got - ref| - bf16 term) / max(E32, 2^-23 A) of every case is recorded in profiles/layernorm_accuracy_mi355x.txt; each test
prints its ratios ("[ln-acc] ...", pytest -s) before it asserts.

Inputs (layernorm_oracle.hard_inputs): unit-variance rows shifted by a per-row mean of +-off, off in {0, 16, 64}; two "massive"
channels at 100x; one all-zero row per sample (h == shift there exactly, every output finite); modulation 0.5 randn.

Semantics checked on every call: column sums are ADDED to the buffer's previous contents (a nonzero fill, subtracted
afterwards); columns of dmod outside the three slices, a slice that was not asked for, rows past M and the guard elements after
every output stay bit-identical.
"""
import pytest
import torch

from tests import layernorm_oracle as O

pytestmark = pytest.mark.gpu

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
EPS = 1e-6
MARGIN = 4.0
GUARD_ROWS = 2
SENTINEL = -777.0
NAME = {F32: "fp32", BF16: "bf16"}
BOTH = (F32, BF16)


# ---------------------------------------------------------------------------------------------------------------- device
def _out(M, D, dtype):
    return torch.full((M + GUARD_ROWS, D), SENTINEL, device="cuda", dtype=dtype)


def _stat(M):
    return torch.full((M + 8,), SENTINEL, device="cuda", dtype=F32)


def _untouched(t, M):
    return torch.equal(t[M:], torch.full_like(t[M:], SENTINEL))


def _mod_dev(mod):
    """[B, 3, D] -> device [B + 1, 3 D + 8] (gate | shift | scale | 8 spare columns; one spare row)."""
    B, _, D = mod.shape
    md = torch.full((B + 1, 3 * D + 8), SENTINEL, dtype=F32)
    md[:B, :3 * D] = mod.reshape(B, 3 * D)
    return md.cuda()


def dev_fwd(x, B, T, *, y=None, mod=None, affine=False):
    """uwu_add_ln_modulate_fwd into guarded buffers -> x_out (None without y), h, mean, rstd on the CPU."""
    from uwudiff_amd import lib as L

    M, D = x.shape
    xd, yd = x.cuda(), (y.cuda() if y is not None else None)
    x_out = _out(M, D, x.dtype) if y is not None else None
    h, mean, rstd = _out(M, D, x.dtype), _stat(M), _stat(M)
    md = _mod_dev(mod) if mod is not None else None
    sl = (lambda i: md[:, i * D:(i + 1) * D].data_ptr()) if md is not None else (lambda i: None)
    mod_ld = 0 if (affine or md is None) else md.shape[1]
    L.call("uwu_add_ln_modulate_fwd", L.ptr(xd), L.ptr(yd), sl(0) if y is not None else None, sl(1), sl(2), mod_ld,
           L.ptr(x_out if y is not None else xd), L.ptr(h), L.ptr(mean), L.ptr(rstd), B, T, D, EPS, int(affine), L.dt(xd),
           L.stream())
    torch.cuda.synchronize()
    for t in (x_out, h, mean, rstd):
        assert t is None or _untouched(t, M), "the forward wrote past row M"
    if md is not None:
        assert torch.equal(md, _mod_dev(mod)), "the forward wrote to the modulation buffer"
    return (x_out[:M].cpu() if y is not None else None), h[:M].cpu(), mean[:M].cpu(), rstd[:M].cpu()


def dev_bwd(dh, x, mean, rstd, B, T, *, mod=None, dx_in=None, y=None, affine=False, sums=True):
    """uwu_add_ln_modulate_bwd into guarded buffers; the column sums land on a nonzero fill, which is subtracted.
    -> dict(dx, dy, dshift, dscale, dgate) on the CPU (column sums in float64)."""
    from uwudiff_amd import lib as L

    M, D = x.shape
    md = _mod_dev(mod) if mod is not None else None
    ML = 3 * D + 8
    fill = torch.rand(B + 1, ML, generator=torch.Generator().manual_seed(5)) - 0.5
    dmod = fill.cuda()
    dev = lambda t: t.cuda() if t is not None else None  # noqa: E731
    dhd, xd, dind, yd, meand, rstdd = dev(dh), dev(x), dev(dx_in), dev(y), dev(mean), dev(rstd)
    dx, dy = _out(M, D, x.dtype), (_out(M, D, x.dtype) if y is not None else None)
    sl = lambda t, i: t[:, i * D:(i + 1) * D].data_ptr()  # noqa: E731
    mod_ld = 0 if affine else ML
    L.call("uwu_add_ln_modulate_bwd", L.ptr(dhd), L.ptr(xd), L.ptr(meand), L.ptr(rstdd), sl(md, 2) if md is not None else None,
           L.ptr(dind), L.ptr(yd), sl(md, 0) if y is not None else None, mod_ld, L.ptr(dx), L.ptr(dy),
           sl(dmod, 1) if sums else None, sl(dmod, 2) if sums else None, sl(dmod, 0) if (sums and y is not None) else None,
           B, T, D, int(affine), L.dt(xd), L.stream())
    torch.cuda.synchronize()
    assert _untouched(dx, M) and (dy is None or _untouched(dy, M)), "the backward wrote past row M"
    after = dmod.cpu()
    assert torch.equal(after[:, 3 * D:], fill[:, 3 * D:]) and torch.equal(after[B], fill[B]), "dmod written outside the slices"
    if not sums:
        assert torch.equal(after, fill), "column sums written although none was asked for"
    if y is None:
        assert torch.equal(after[:, :D], fill[:, :D]), "dgate written without y"
    delta = after.double() - fill.double()
    out = dict(dx=dx[:M].cpu(), dy=dy[:M].cpu() if dy is not None else None)
    out.update(dgate=delta[:B, :D], dshift=delta[:B, D:2 * D], dscale=delta[:B, 2 * D:3 * D])
    return out


# ------------------------------------------------------------------------------------------------------------------ bars
class Bars:
    def __init__(self, label):
        self.label, self.rows = label, []

    def add(self, name, got, ref, ref32, A=None, bf16_out=False):
        finite = bool(torch.isfinite(got).all())
        e32, r = O.ratio(got, ref, ref32, A=A, bf16_out=bf16_out)
        self.rows.append((name, e32, r if finite else float("inf")))

    def add_rows(self, name, got, ref, ref32, zero, bf16_out=False):
        """An elementwise output: the all-zero rows (rstd = eps^-1/2 makes their values and their fp32 error ~1000x those of
        the other rows) and the other rows each against their own E32 and A, which is no wider than one bar for the tensor."""
        rest = torch.ones(got.shape[0], dtype=torch.bool)
        rest[zero] = False
        self.add(name, got[rest], ref[rest], ref32[rest], bf16_out=bf16_out)
        self.add(name + "[0]", got[zero], ref[zero], ref32[zero], bf16_out=bf16_out)

    def done(self):
        print(f"[ln-acc] {self.label:<58s} " + "  ".join(f"{n}={r:.2f}(E32 {e:.1e})" for n, e, r in self.rows))
        bad = [(n, r) for n, _, r in self.rows if not r <= MARGIN]
        assert not bad, f"{self.label}: ratio to max(E32, 2^-23 A) above {MARGIN}: {bad}"


def check_bwd(label, B, T, D, dtype, off, stats, *, variant="full", affine=False, sums=True):
    x, y, dh, dx_in, mod = O.hard_inputs(B, T, D, off, dtype)
    if affine or variant == "no_y":
        y = None
    if variant == "no_dx_in":
        dx_in = None
    gate = mod[:, 0] if y is not None else None
    if stats == "fwd":  # the forward kernel's statistics of the same stream
        _, _, mean, rstd = dev_fwd(x, B, T)
    else:  # fp64 statistics rounded to fp32
        f = O.forward(x, T, eps=EPS)
        mean, rstd = f["mean"].float(), f["rstd"].float()
    kw = dict(scale=mod[:, 2], dx_in=dx_in, y=y, gate=gate, affine=affine)
    ref = O.backward(dh, x, mean, rstd, T, **kw)
    ref32 = O.backward(dh, x, mean, rstd, T, dtype=F32, **kw)
    got = dev_bwd(dh, x, mean, rstd, B, T, mod=mod, dx_in=dx_in, y=y, affine=affine, sums=sums)
    bars = Bars(label)
    bf = dtype == BF16
    z = O.zero_rows(B, T)
    bars.add_rows("dx", got["dx"], ref["dx"], ref32["dx"], z, bf16_out=bf)
    if y is not None:
        bars.add_rows("dy", got["dy"], ref["dy"], ref32["dy"], z, bf16_out=bf)
    if sums:
        for k in ("dshift", "dscale") + (("dgate",) if y is not None else ()):
            bars.add(k, got[k], ref[k], ref32[k], A=ref["A_" + k])
    bars.done()
    return got, ref, ref32


def _offsets(M, D):
    return (0, 16, 64) if M * D <= (1 << 20) else (64,)


def _expand(cases, variants=False):
    out = []
    for B, T, D, dtypes, why in cases:
        for dtype in dtypes:
            for off in _offsets(B * T, D):
                for stats in ("fwd", "fp64"):
                    out.append(pytest.param(B, T, D, dtype, off, stats, "full", why,
                                            id=f"{B}x{T}x{D}-{NAME[dtype]}-off{off}-{stats}"))
            if variants and B * T * D <= (1 << 20):  # (y, gate and dx_in absent, once each)
                for v in ("no_y", "no_dx_in"):
                    out.append(pytest.param(B, T, D, dtype, 16, "fp64", v, why, id=f"{B}x{T}x{D}-{NAME[dtype]}-off16-fp64-{v}"))
    return out


# (B, T, D), dtypes, the dispatcher condition that selects the branch (uwu_add_ln_modulate_bwd; M = B T; rows = the largest
# power of two <= 32 that divides T; "small" = M / rows < 1024 && T % 16 == 0 && D <= 640)
ADALN_BWD = [
    (2, 48, 640, (BF16,), "small && bf16: the 8-wave kernel, rows = 16, NIT = ceil(640 / 512) = 2"),
    (3, 64, 384, (F32,), "small but fp32: the 4-wave kernel entered with rows = 16 and 8 slabs of LDS"),
    (3, 77, 384, BOTH, "T odd: rows = 1, 77 atomics per column and sample"),
    (3, 40, 384, BOTH, "T % 16 = 8: rows = 8, not small, M / 8 < 1024: reduced to 4"),
    (2, 100, 1152, BOTH, "T % 8 = 4: rows = 4; D > 1024: NIT 3, the one-slab fold"),
    (2, 64, 768, BOTH, "D > 640: not small, rows 32 -> 4; NIT 2, a slab per wave"),
    (1, 32, 1024, BOTH, "NIT 2 with every lane busy in both passes (D = 1024), the widest slab-per-wave fold"),
    (1, 32, 2048, BOTH, "NIT 4, one slab"),
    (1, 16, 3072, BOTH, "NIT 6, the widest instantiation; T = 16: rows 16 -> 4"),
    (128, 256, 384, BOTH, "the benchmark's branch: M / 32 = 1024, not < 1024: rows = 32, grid 1024"),
    (128, 256, 64, BOTH, "the benchmark's branch at D = 64 (8 of 64 lanes busy): rows = 32, grid 1024"),
]


@pytest.mark.parametrize("B,T,D,dtype,off,stats,variant,why", _expand(ADALN_BWD, variants=True))
def test_adaln_bwd(B, T, D, dtype, off, stats, variant, why):
    check_bwd(f"adaln_bwd {B}x{T}x{D} {NAME[dtype]} off{off} {stats} {variant}", B, T, D, dtype, off, stats, variant=variant)


# (M, D): ln_affine_bwd_kernel (B = 1, mod_ld = 0, dshift and dscale given, D <= 2048): rows per block 16 / 32 / 64 for
# M < 4096 / < 16384 / above; 64 D bytes of LDS
AFFINE_BWD = [
    (1, 1000, 320, BOTH, "M < 4096: rpb 16, ragged last workgroup of 8 rows"),
    (1, 4100, 640, BOTH, "M >= 4096: rpb 32, last workgroup of 4 rows (4 of 8 waves idle), NIT 2"),
    (1, 16400, 320, BOTH, "M >= 16384: rpb 64, last workgroup of 16 rows"),
    (1, 520, 1280, BOTH, "NIT 3, 80 KB of LDS: above the 64 KB default limit (D >= 1032)"),
    (1, 40, 2048, BOTH, "NIT 4, 128 KB of LDS, the widest the kernel takes"),
]


def _expand_affine():
    out = []
    for B, T, D, dtypes, why in AFFINE_BWD:
        for dtype in dtypes:
            for off in _offsets(T, D):
                for stats in ("fwd", "fp64"):
                    out.append(pytest.param(T, D, dtype, off, stats, "no_y", why, id=f"{T}x{D}-{NAME[dtype]}-off{off}-{stats}"))
            out.append(pytest.param(T, D, dtype, 16, "fp64", "no_dx_in", why, id=f"{T}x{D}-{NAME[dtype]}-off16-fp64-no_dx_in"))
    return out


@pytest.mark.parametrize("M,D,dtype,off,stats,variant,why", _expand_affine())
def test_affine_bwd(M, D, dtype, off, stats, variant, why):
    """The UNet's LayerNorm backward: with dx_in (_AddLayerNormFn) and without it (_LayerNormFn)."""
    check_bwd(f"affine_bwd {M}x{D} {NAME[dtype]} off{off} {stats} {'dx_in' if variant == 'no_y' else 'no_dx_in'}", 1, M, D, dtype,
              off, stats, variant=variant, affine=True)


@pytest.mark.parametrize("dtype", BOTH, ids=NAME.get)
@pytest.mark.parametrize("M,D,why", [(231, 320, "T odd: the generic kernel with rows = 1"),
                                     (4096, 640, "small: rows = 16 (bf16: the 8-wave kernel, NIT 2)")])
@pytest.mark.parametrize("stats", ["fwd", "fp64"])
def test_affine_bwd_without_column_sums(M, D, why, dtype, stats):
    """Frozen weights: no dshift / dscale, so the call falls through to the generic kernel, which must write no sum."""
    check_bwd(f"affine_bwd_nosums {M}x{D} {NAME[dtype]} off64 {stats}", 1, M, D, dtype, 64, stats, variant="no_y", affine=True,
              sums=False)


# ------------------------------------------------------------------------------------------------------------- forward
# (B, T, D), UWU_LN_ROW16 values to run ("" = the dispatcher's own choice), branch (uwu_add_ln_modulate_fwd)
FWD = [
    (3, 77, 384, ("",), "M < 4096: one row per wave, NIT 1"),
    (17, 256, 384, ("", "0"), "M = 4352 >= 4096, D % 128 == 0, D <= 768: four rows per wave, NCH 3; 0: one row per wave"),
    (16, 259, 768, ("", "0"), "four rows per wave, NCH 6, row groups straddle samples; 0: one row per wave, NIT 2"),
    (1, 16, 4096, ("",), "the widest row: one row per wave, NIT 8"),
    (3, 1367, 128, ("",), "four rows per wave, NCH 1, M = 4101: a ragged last group with one row"),
]


def _expand_fwd():
    out = []
    for B, T, D, flags, why in FWD:
        for dtype in BOTH:
            for flag in flags:
                for off in _offsets(B * T, D):
                    out.append(pytest.param(B, T, D, dtype, off, flag, False, why,
                                            id=f"{B}x{T}x{D}-{NAME[dtype]}-off{off}" + ("-row16=" + flag if flag else "")))
            if D == 384:
                out.append(pytest.param(B, T, D, dtype, 16, "", True, why, id=f"{B}x{T}x{D}-{NAME[dtype]}-off16-affine"))
    return out


def check_fwd_outputs(bars, dtype, x, y, mod, T, dev, affine):
    """x_out, mean, rstd, h of one forward call against the reference; returns nothing, fills `bars`."""
    x_out, h, mean, rstd = dev
    gate, shift, scale = mod[:, 0], mod[:, 1], mod[:, 2]
    xo = O.residual(x, T, y, gate)
    if dtype == BF16:
        ok = O.is_bf16_neighbour(x_out, xo)
        assert ok.all(), f"x_out is not a bf16 neighbour of x + gate*y at {int((~ok).sum())} elements"
        base64, base32 = x_out, x_out  # the stream the kernel normalised
    else:
        xo32 = O.residual(x, T, y, gate, dtype=F32)
        bars.add("x_out", x_out, xo, xo32)  # (zero on the all-zero rows)
        base64, base32 = xo, xo32
    kw = dict(shift=shift, scale=scale, eps=EPS, affine=affine)
    ref, ref32 = O.forward(base64, T, **kw), O.forward(base32, T, dtype=F32, **kw)
    z = O.zero_rows(x.shape[0] // T, T)
    bars.add("mean", mean, ref["mean"], ref32["mean"])  # (zero on the all-zero rows)
    bars.add_rows("rstd", rstd, ref["rstd"], ref32["rstd"], z)
    if h is not None:
        bars.add("h", h, ref["h"], ref32["h"], bf16_out=dtype == BF16)  # (h == shift on the all-zero rows: test_fwd)


@pytest.mark.parametrize("B,T,D,dtype,off,row16,affine,why", _expand_fwd())
def test_fwd(B, T, D, dtype, off, row16, affine, why, monkeypatch):
    if row16:
        monkeypatch.setenv("UWU_LN_ROW16", row16)
    x, y, _, _, mod = O.hard_inputs(B, T, D, off, dtype)
    if affine:
        mod = mod[:1]
    dev = dev_fwd(x, B, T, y=y, mod=mod, affine=affine)
    bars = Bars(f"fwd {B}x{T}x{D} {NAME[dtype]} off{off}" + (f" row16={row16}" if row16 else "") + (" affine" if affine else ""))
    check_fwd_outputs(bars, dtype, x, y, mod, T, dev, affine)
    z = O.zero_rows(B, T)
    shift_rows = mod[:, 1].expand(B, D) if affine else mod[:, 1]
    assert torch.equal(dev[1][z], shift_rows.to(dtype)), "h != shift on the all-zero rows"
    assert (dev[2][z] == 0).all() and torch.allclose(dev[3][z], torch.tensor(EPS ** -0.5))
    bars.done()


def test_fwd_q8_statistics():
    """The fp8-emitting forward: its residual stream, mean and rstd on offset-64 rows (its bytes: tests/test_fp8_gpu.py)."""
    from uwudiff_amd import ops

    B, T, D, off = 2, 64, 384, 64
    x, y, _, _, mod = O.hard_inputs(B, T, D, off, BF16)
    md = _mod_dev(mod)
    qs = torch.ones(1, device="cuda")
    x_out, q8, q8t, mean, rstd = ops.add_ln_modulate_fwd_q8(x.cuda(), B, T, qs, shift=md[:, D:2 * D], scale=md[:, 2 * D:3 * D],
                                                            mod_ld=md.shape[1], y=y.cuda(), gate=md[:, 0:D])
    torch.cuda.synchronize()
    bars = Bars(f"fwd_q8 {B}x{T}x{D} bf16 off{off}")
    check_fwd_outputs(bars, BF16, x, y, mod, T, (x_out.cpu(), None, mean.cpu(), rstd.cpu()), False)
    bars.done()


# ----------------------------------------------------------------------------------------------------------- semantics
@pytest.mark.parametrize("dtype", BOTH, ids=NAME.get)
def test_bwd_twice_within_the_bar(dtype):
    """rows = 1: 77 atomics per column in arbitrary order.  Two runs need not be bit-equal; both stay within the bar."""
    for run in (1, 2):
        check_bwd(f"adaln_bwd_repeat 3x77x384 {NAME[dtype]} off64 fp64 run{run}", 3, 77, 384, dtype, 64, "fp64")


@pytest.mark.parametrize("dtype", BOTH, ids=NAME.get)
def test_bwd_refuses_d_above_3072(dtype):
    """The forward takes D <= 4096 (test_fwd runs 4096), the backward D <= 3072: D = 3584 is refused and launches nothing."""
    from uwudiff_amd import lib as L

    B, T, D = 1, 4, 3584
    x, y, dh, dx_in, mod = O.hard_inputs(B, T, D, 0, dtype)
    _, h, mean, rstd = dev_fwd(x, B, T)
    assert torch.isfinite(h).all()
    md = _mod_dev(mod)
    fill = torch.rand(B + 1, 3 * D + 8, generator=torch.Generator().manual_seed(5)) - 0.5
    dmod, dx, dy = fill.cuda(), _out(B * T, D, dtype), _out(B * T, D, dtype)
    args = [x.cuda(), dh.cuda(), mean.cuda(), rstd.cuda(), dx_in.cuda(), y.cuda()]
    with pytest.raises(L.UwuError, match="3072"):
        L.call("uwu_add_ln_modulate_bwd", L.ptr(args[1]), L.ptr(args[0]), L.ptr(args[2]), L.ptr(args[3]),
               md[:, 2 * D:3 * D].data_ptr(), L.ptr(args[4]), L.ptr(args[5]), md[:, 0:D].data_ptr(), md.shape[1], L.ptr(dx),
               L.ptr(dy), dmod[:, D:2 * D].data_ptr(), dmod[:, 2 * D:3 * D].data_ptr(), dmod[:, 0:D].data_ptr(), B, T, D, 0,
               L.dt(args[0]), L.stream())
    torch.cuda.synchronize()
    assert _untouched(dx, 0) and _untouched(dy, 0) and torch.equal(dmod.cpu(), fill)
