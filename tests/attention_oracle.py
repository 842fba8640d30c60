"""Plain softmax attention forward and backward, the reference of tests/test_attention_accuracy_gpu.py.  `evaluate` writes out the
formulas of flash attention on [B, H, T, d] tensors in the dtype it is given:

    s = scale q k^T + bias ; lse = logsumexp(s) ; p = exp(s - lse) ; o = p v
    delta = rowsum(dO * o) ; ds = p * (dO v^T - delta)
    dq = scale ds k ; dk = scale ds^T q ; dv = p^T dO

float64 is the reference.  float32 is the yardstick of the generic kernels (csrc/attention_simple.hip keeps P in fp32), and float32
with `round_p` the yardstick of the MFMA kernels: it rounds to bfloat16 exactly where csrc/attention_mfma.hip does --
  * p before P V (forward; the row sum l is taken from the unrounded p) and before P^T dO (backward),
  * ds once, before both ds k and ds^T q,
and nothing else; outputs stay unrounded (the final bf16 store is its own term of the test's bar).
The backward contract: the kernels are handed o and lse and compute p = exp(s - lse), delta = rowsum(dO * o) from exactly those.
`evaluate(..., o=, lse=)` does the same; without them the backward uses its own forward values.
The rope contract (uwu_attention_rope_fwd / _bwd): q and k are replaced by bf16(float(x) * table) while they are staged (`rope`);
everything after that is plain attention on the rotated, rounded tensors, and dq / dk are gradients with respect to those.
The key bias is finite (-10000 hides a key); -inf is not part of the contract.

tests/test_attention_ref_cpu.py checks `evaluate` against torch.autograd in float64, that faults seeded into the yardstick break the
bars, and that the routing construction (`routing_inputs`) is exact in the yardstick."""
import functools
import math

import torch

from tests.layernorm_oracle import ratio  # noqa: F401  (same meaning here: E = max |yardstick - fp64|, the bar is ratio <= 4)

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
HIDE = -10000.0
CLASSES = ("plain", "peaked", "offset", "rising", "degenerate")  # + "falling", on one case per kernel
BIAS_CLASSES = ("first_tile", "last_tile", "random40", "all_but_one", "randn2")


def _bf(t):
    return t.to(BF16).to(t.dtype)


def evaluate(q, k, v, do, *, bias=None, scale, dtype, round_p, o=None, lse=None, fault=None):
    """-> dict(o, lse, delta, dq, dk, dv) in `dtype` from [B, H, T, d] tensors (bias: [B, Tk]).  `fault` seeds one of the faults of
    tests/test_attention_ref_cpu.py into the evaluation ("drop_key", "delta_roll", "dk_noscale"); nothing else passes it."""
    q, k, v, do = (t.to(dtype) for t in (q, k, v, do))
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) * scale
    if bias is not None:
        s = s + bias.to(dtype)[:, None, None, :]
    m = s.amax(-1, keepdim=True)
    pu = torch.exp(s - m)
    l = pu.sum(-1, keepdim=True)
    own_lse = (m + torch.log(l)).squeeze(-1)
    pf = _bf(pu) if round_p else pu
    if fault == "drop_key":
        pf = pf.clone()
        pf[..., 5] = 0
    own_o = torch.einsum("bhqk,bhkd->bhqd", pf, v) / l
    lse_b = own_lse if lse is None else lse.to(dtype)
    o_b = own_o if o is None else o.to(dtype)
    p = torch.exp(s - lse_b[..., None])
    if fault == "drop_key":
        p[..., 5] = 0
    delta = (do * o_b).sum(-1)
    if fault == "delta_roll":
        delta = delta.roll(1, -1)
    ds = p * (torch.einsum("bhqd,bhkd->bhqk", do, v) - delta[..., None])
    pb, dsb = (_bf(p), _bf(ds)) if round_p else (p, ds)
    dq = torch.einsum("bhqk,bhkd->bhqd", dsb, k) * scale
    dk = torch.einsum("bhqk,bhqd->bhkd", dsb, q) * (1.0 if fault == "dk_noscale" else scale)
    dv = torch.einsum("bhqk,bhqd->bhkd", pb, do)
    return dict(o=own_o, lse=own_lse, delta=delta, dq=dq, dk=dk, dv=dv)


def forward_blockwise(q, k, v, *, bias=None, scale, dtype=F32, round_p=True, tile=64, stale_alpha_tile=None):
    """The forward as the kernels run it: key tiles of `tile`, a running maximum, o and l rescaled by alpha = exp(m_old - m_new).
    `stale_alpha_tile`: the seeded fault that leaves alpha at 1 when that tile arrives.  -> o, lse"""
    q, k, v = (t.to(dtype) for t in (q, k, v))
    B, H, Tq, d = q.shape
    m = torch.full((B, H, Tq, 1), -math.inf, dtype=dtype)
    l = torch.zeros(B, H, Tq, 1, dtype=dtype)
    o = torch.zeros(B, H, Tq, d, dtype=dtype)
    for t, k0 in enumerate(range(0, k.shape[2], tile)):
        s = torch.einsum("bhqd,bhkd->bhqk", q, k[:, :, k0:k0 + tile]) * scale
        if bias is not None:
            s = s + bias.to(dtype)[:, None, None, k0:k0 + tile]
        mn = torch.maximum(m, s.amax(-1, keepdim=True))
        alpha = torch.ones_like(m) if t == stale_alpha_tile else torch.exp(m - mn)
        p = torch.exp(s - mn)
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + torch.einsum("bhqk,bhkd->bhqd", _bf(p) if round_p else p, v[:, :, k0:k0 + tile])
        m = mn
    return o / l, (m + torch.log(l)).squeeze(-1)


def rope(x, tab):
    """rope8 / rope4 of attention_mfma.hip: bf16(float(x) * tab).  x bf16 [B, H, T, d], tab fp32 [H, T, d]"""
    return (x.float() * tab[None].float()).to(BF16)


def heads(t, B, T, H, d):
    """[B*T, H*d] -> [B, H, T, d]"""
    return t.reshape(B, T, H, d).transpose(1, 2)


def flat(t):
    """[B, H, T, d] -> [B*T, H*d]"""
    B, H, T, d = t.shape
    return t.transpose(1, 2).reshape(B * T, H * d)


# ---------------------------------------------------------------------------------------------------------------- hard inputs
def special_rows(B, Tq, Tk):
    """The rows of the `degenerate` class, per sample: zero query, zero dO, zero key, (duplicate key, its original)."""
    b = torch.arange(B)
    return dict(zq=(3 + 7 * b) % Tq, zdo=(11 + 5 * b) % Tq, zk=(5 + 3 * b) % Tk, dup=(9 + 2 * b) % Tk, src=(1 + b) % Tk)


@functools.lru_cache(maxsize=8)
def hard_inputs(cls, B, H, Tq, Tk, d, dtype, seed=0):
    """q, do [B, H, Tq, d] and k, v [B, H, Tk, d], rounded to `dtype` (returned in it), of one input class.  With scale = d^-1/2:
      plain       randn: score rows of standard deviation 1.
      peaked      q * 4: score standard deviation 4, rows near one-hot with a few competitors.
      offset      q += 40 u, k += 60 u for one unit vector u: every logit of a row moves by 2400 scale (+300 at d = 64) and lse
                  with it -- the maximum subtraction, the size of lse, the -lse / scale start of the backward's S accumulator.
      rising      every query gets +4 w (one unit vector w) and key j gets + j g w, g chosen so that the score of the mean query
                  rises by 1/8 nat per key: the running maximum rises in every key tile, alpha < 1 every time.
      falling     rising with the key order reversed: the maximum is found in the first tile and alpha stays 1.
      degenerate  plain with, per sample, an all-zero query row, an all-zero dO row, an all-zero key and two identical keys
                  (`special_rows`).
    Do not modify the results."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * d + 104729 * Tq + 31 * Tk + 13 * B + H)
    q, k, v, do = (torch.randn(B, H, T, d, generator=g) for T in (Tq, Tk, Tk, Tq))
    u = torch.randn(d, generator=g)
    u /= u.norm()
    if cls == "peaked":
        q *= 4.0
    elif cls == "offset":
        q += 40.0 * u
        k += 60.0 * u
    elif cls in ("rising", "falling"):
        q += 4.0 * u
        ramp = torch.arange(Tk, dtype=torch.float32) * (0.125 * math.sqrt(d) / 4.0)
        k += (ramp.flip(0) if cls == "falling" else ramp)[:, None] * u
    elif cls == "degenerate":
        r = special_rows(B, Tq, Tk)
        for b in range(B):
            q[b, :, r["zq"][b]] = 0
            do[b, :, r["zdo"][b]] = 0
            k[b, :, r["zk"][b]] = 0
            k[b, :, r["dup"][b]] = k[b, :, r["src"][b]]
    else:
        assert cls == "plain", cls
    return tuple(t.to(dtype) for t in (q, k, v, do))


@functools.lru_cache(maxsize=8)
def hard_bias(cls, B, Tk, seed=0):
    """fp32 [B, Tk]; at least one key stays visible in every row.
      first_tile   -10000 on the whole first 64-key tile (Tk <= 64: on all keys but the last)
      last_tile    -10000 on the whole last key tile but its first key
      random40     -10000 on a random 40 %, different per sample
      all_but_one  -10000 on every key but one (another one per sample): o is that key's v row
      randn2       2 randn, the general finite bias"""
    g = torch.Generator().manual_seed(77 * seed + 1009 * Tk + B)
    bias = torch.zeros(B, Tk)
    if cls == "first_tile":
        bias[:, :min(64, Tk - 1)] = HIDE
    elif cls == "last_tile":
        bias[:, (Tk - 1) // 64 * 64 + 1:] = HIDE
    elif cls == "random40":
        bias[torch.rand(B, Tk, generator=g) < 0.4] = HIDE
        bias[:, 0] = 0
        assert B == 1 or not torch.equal(bias[0], bias[1])
    elif cls == "all_but_one":
        bias[:] = HIDE
        bias[torch.arange(B), visible_key(B, Tk)] = 0
    else:
        assert cls == "randn2", cls
        bias = 2.0 * torch.randn(B, Tk, generator=g)
    return bias


def visible_key(B, Tk):
    return (7 + 13 * torch.arange(B)) % Tk


# ---------------------------------------------------------------------------------------------------------- exact routing
@functools.lru_cache(maxsize=4)
def routing_inputs(B, H, Tq, Tk, d, biased=False, seed=0):
    """A problem whose attention is a gather, exact in the kernels' arithmetic: every index computation is checked with no tolerance.
    Key j is a sign vector: each of the bits = ceil(log2 Tk) bits of j repeated rep = d // bits times as +-S, the remaining columns +S.
    Query i is A * the sign vector of pi(i); pi covers every (visible) key where Tq allows.  A, S: powers of two, the smallest with
    2 A S rep scale >= 120 nats between the winning key and the next, so that every losing probability is exactly 0 in fp32.
    v: integers in [-8, 8]; dO: integers in [-4, 4].  biased: -10000 hides a third of the keys and pi maps to visible keys only.
    -> dict(q, k, v, do [B, H, T, d] float32 with bf16-exact values, bias, scale, pi [B, H, Tq] and the expected
       o = v[pi], lse = scale <q_i, k_pi(i)> (float64), dv[j] = sum of dO[i] over pi(i) = j; dq = dk = 0)."""
    g = torch.Generator().manual_seed(4243 * seed + 7919 * d + 104729 * Tq + 31 * Tk + biased)
    scale = float(torch.tensor(d ** -0.5, dtype=F32))  # the fp32 value the kernels get
    bits = max(1, math.ceil(math.log2(Tk)))
    rep = d // bits
    assert rep >= 1
    n = 0
    while 2.0 * 2.0 ** n * rep * scale < 120.0:
        n += 1
    A, S = 2.0 ** ((n + 1) // 2), 2.0 ** (n // 2)
    j = torch.arange(Tk)
    sign = torch.ones(Tk, d)
    for t in range(bits):
        sign[:, t * rep:(t + 1) * rep] = (2.0 * ((j >> t) & 1) - 1.0)[:, None]
    bias = None
    visible = [j for _ in range(B)]
    if biased:
        bias = torch.zeros(B, Tk)
        for b in range(B):
            hid = torch.randperm(Tk, generator=g)[:Tk // 3]
            bias[b, hid] = HIDE
            visible[b] = j[bias[b] == 0]
    pi = torch.empty(B, H, Tq, dtype=torch.long)
    for b in range(B):
        nv = len(visible[b])
        for h in range(H):
            order = visible[b][torch.randperm(nv, generator=g)]
            pi[b, h] = order[torch.arange(Tq) % nv][torch.randperm(Tq, generator=g)]
    k = (S * sign)[None, None].expand(B, H, Tk, d).contiguous()
    q = A * sign[pi]
    v = torch.randint(-8, 9, (B, H, Tk, d), generator=g).float()
    do = torch.randint(-4, 5, (B, H, Tq, d), generator=g).float()
    idx = pi[..., None].expand(B, H, Tq, d)
    o = torch.gather(v, 2, idx)
    dv = torch.zeros(B, H, Tk, d).scatter_add_(2, idx, do)
    assert dv.abs().max() <= 256
    lse = scale * (q.double() * torch.gather(k, 2, idx).double()).sum(-1)
    assert lse.max() < 1250
    return dict(q=q, k=k, v=v, do=do, bias=bias, scale=scale, pi=pi, o=o, lse=lse, dv=dv)
