"""numpy restatement of the 8-bit block-wise AdamW / Lion rule (include/uwu_hip.h: uwu_adamw8_step, uwu_lion8_step): the code
tables, one step from a given state (p, g, codes, absmax), and the per-element acceptance bound of a quantised code.  fp64 unless a
dtype is given (``ft=np.float32`` mirrors the kernel's operation order: what the fixtures are chosen with).  No GPU, no torch."""
import numpy as np

BLOCK = 256


def dynamic_map(signed):
    """bitsandbytes' create_dynamic_map(signed, max_exponent_bits=7, total_bits=8), restated: 256 fp32 values, increasing"""
    data = [0.0, 1.0]
    for i in range(7):
        k = 2 ** i + 1 if signed else 2 ** (i + 1) + 1
        edges = 0.1 + 0.9 * np.arange(k, dtype=np.float64) / (k - 1)
        means = 10.0 ** (i - 6) * ((edges[:-1] + edges[1:]) / 2)
        data += means.tolist()
        if signed:
            data += (-means).tolist()
    return np.sort(np.asarray(data, np.float64)).astype(np.float32)


def nearest(T, x):
    """index of the entry of the increasing table T nearest to x; a tie goes to the lower index"""
    T = np.asarray(T, np.float64)
    x = np.asarray(x, np.float64)
    lo = np.clip(np.searchsorted(T, x, side="right") - 1, 0, len(T) - 1)
    hi = np.minimum(lo + 1, len(T) - 1)
    return np.where((T[hi] - x) < (x - T[lo]), hi, lo).astype(np.uint8)


def blocks_of(n):
    return -(-n // BLOCK)


def per_element(absmax, n):
    return np.repeat(np.asarray(absmax), BLOCK)[:n]


def block_max(a):
    n = a.shape[0]
    pad = np.zeros(blocks_of(n) * BLOCK, a.dtype)
    pad[:n] = a
    return pad.reshape(-1, BLOCK).max(axis=1)


def dequantise(T, codes, absmax, ft=np.float64):
    return np.asarray(T, ft)[codes] * per_element(absmax, codes.shape[0]).astype(ft)


def quantise(T, a, ft=np.float64):
    """(ratio a / absmax per element, codes, absmax per block); a block whose absmax is 0 gets the code nearest to 0"""
    a = np.asarray(a, ft)
    absmax = block_max(np.abs(a))
    d = per_element(absmax, a.shape[0])
    x = np.divide(a, d, out=np.zeros_like(a), where=d > 0)
    return x, nearest(T, x), absmax


def adamw8_step(p, g_eff, c1, a1, c2, a2, T1, T2, step, lr, betas, eps, wd, ft=np.float64):
    """one step on whole buffers; returns a dict: p, the new ratios x1 / x2, codes c1 / c2, absmax a1 / a2, and the quantities the
    acceptance bound is made of (m_old, v_old, m_new, v_new)"""
    b1, b2 = betas
    f = ft
    m_old, v_old = dequantise(T1, c1, a1, f), dequantise(T2, c2, a2, f)
    g = np.asarray(g_eff, f)
    pp = np.asarray(p, f) * f(1.0 - lr * wd)
    m = m_old + (g - m_old) * f(1.0 - b1)
    v = v_old * f(b2) + f(1.0 - b2) * g * g
    step_size, inv_bc2_sqrt = f(lr / (1.0 - b1 ** step)), f(1.0 / np.sqrt(1.0 - b2 ** step))
    pp = pp - step_size * (m / (np.sqrt(v) * inv_bc2_sqrt + f(eps)))
    x1, nc1, na1 = quantise(T1, m, f)
    x2, nc2, na2 = quantise(T2, v, f)
    return dict(p=pp, x1=x1, c1=nc1, a1=na1, x2=x2, c2=nc2, a2=na2, m_old=m_old, v_old=v_old, m_new=m, v_new=v)


def lion8_step(p, g_eff, c1, a1, T1, lr, betas, wd, ft=np.float64):
    """lion_elem with the moment dequantised before and requantised after; also c and the size of its terms (the sign of c is
    only determined outside their rounding)"""
    b1, b2 = betas
    f = ft
    m_old = dequantise(T1, c1, a1, f)
    g = np.asarray(g_eff, f)
    c = m_old * f(b1) + g * f(1.0 - b1)
    mag = np.abs(m_old * f(b1)) + np.abs(g * f(1.0 - b1))
    pp = np.asarray(p, f) * f(1.0 - lr * wd) - f(lr) * np.sign(c)
    m = m_old * f(b2) + g * f(1.0 - b2)
    x1, nc1, na1 = quantise(T1, m, f)
    return dict(p=pp, x1=x1, c1=nc1, a1=na1, m_old=m_old, m_new=m, c=c, mag=mag)


def code_slack(first, old, g_eff, absmax_new, n):
    """d of the acceptance bound: 8 * 2^-24 * (|m_old| + |g_eff|) / absmax_new for a first moment, (v_old + g_eff^2) / absmax_new
    for a second: the fp32 rounding of the element's own inputs, relative to the block's scale.  0 where absmax_new is 0."""
    size = np.abs(old) + np.abs(g_eff) if first else old + np.asarray(g_eff, np.float64) ** 2
    d = per_element(absmax_new, n).astype(np.float64)
    return 8 * 2.0 ** -24 * np.divide(size, d, out=np.zeros(n), where=d > 0)


def code_accepted(T, x, codes, d):
    """|x - T[c]| <= min_k |x - T[k]| + d per element"""
    T = np.asarray(T, np.float64)
    x = np.asarray(x, np.float64)
    best = np.abs(x - T[nearest(T, x)])
    return np.abs(x - T[codes]) <= best + d


def boundary_margin(T, x):
    """distance of x from the nearest decision boundary of the table (a midpoint of two neighbours), relative to the gap there"""
    T = np.asarray(T, np.float64)
    mid = (T[:-1] + T[1:]) / 2
    k = np.clip(np.searchsorted(mid, x), 0, len(mid) - 1)
    k0 = np.clip(k - 1, 0, len(mid) - 1)
    dist = np.minimum(np.abs(x - mid[k]) / (T[k + 1] - T[k]), np.abs(x - mid[k0]) / (T[k0 + 1] - T[k0]))
    return dist


def adamw_exact(p, g, m, v, step, lr, betas, eps, wd):
    """fp64 AdamW with fp64 moments (the rule of adamw_kernel: decay first)"""
    b1, b2 = betas
    p = p * (1.0 - lr * wd)
    m = m + (g - m) * (1.0 - b1)
    v = v * b2 + (1.0 - b2) * g * g
    p = p - lr / (1.0 - b1 ** step) * (m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** step) + eps))
    return p, m, v


# ---------------------------------------------------------------------------------------------------------------- fixtures
HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=1e-2)
LION_HP = dict(lr=1e-3, betas=(0.9, 0.99), wd=0.1)
SEED = 1


def fixture(n, later, seed=SEED):
    """(p, g, m, v) in fp32/fp64 for the one-step tests: block 0 ordinary; block 1 (n > 256) a zero gradient; block 2 one element
    1e9 times the rest (the others take the zero code); the last block of n = 3*256 + 37 partial.  ``later``: a nonzero state to
    quantise (a later step); else the zero state of step 1.  Every block's largest |m| is made negative in block 0 and positive in
    the last one, so that elements sit exactly at -absmax and +absmax."""
    rng = np.random.default_rng(seed + n + (1000 if later else 0))
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 1e-2).astype(np.float32)
    m = (rng.standard_normal(n) * 1e-2) if later else np.zeros(n)
    v = (rng.standard_normal(n) ** 2 * 1e-4) if later else np.zeros(n)
    g[5] = -2.0  # the largest |m_new| of block 0 is negative
    if later:
        m[5] = -0.05
    if n > BLOCK:
        g[BLOCK:2 * BLOCK] = 0
        g[2 * BLOCK + 17] = 1e7  # 1e9 times the others' 1e-2
        g[n - 3] = 3.0  # the largest of the last block is positive
        if later:
            m[2 * BLOCK + 17] = 1e7
            v[2 * BLOCK + 17] = 1e14
    return p, g, m, v


def quadratic_problem(n=4196, seed=11):
    """the quality guard's fixed problem: g = D (p - p*), D = exp(N(0, 0.5)), p* = N(0, 1), p0 = 0"""
    rng = np.random.default_rng(seed)
    D = np.exp(rng.standard_normal(n) * 0.5).astype(np.float32)
    pstar = rng.standard_normal(n).astype(np.float32)
    return D, pstar


def quadratic_runs(steps=200, n=4196):
    """(exact fp64 AdamW parameters, the oracle's own 8-bit run's parameters) after ``steps`` steps at lr 1e-3"""
    D, pstar = quadratic_problem(n)
    D, pstar = D.astype(np.float64), pstar.astype(np.float64)
    T1, T2 = dynamic_map(True), dynamic_map(False)
    pe, me, ve = np.zeros(n), np.zeros(n), np.zeros(n)
    pq = np.zeros(n)
    c1, c2 = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    a1, a2 = np.zeros(blocks_of(n)), np.zeros(blocks_of(n))
    for t in range(1, steps + 1):
        pe, me, ve = adamw_exact(pe, D * (pe - pstar), me, ve, t, HP["lr"], HP["betas"], HP["eps"], HP["wd"])
        o = adamw8_step(pq, D * (pq - pstar), c1, a1, c2, a2, T1, T2, t, HP["lr"], HP["betas"], HP["eps"], HP["wd"])
        pq, c1, a1, c2, a2 = o["p"], o["c1"], o["a1"], o["c2"], o["a2"]
    return pe, pq
