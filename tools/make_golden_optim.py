"""Regenerates tests/golden/adamw_fp16_3tensors.npz from the reference's own optimizer (run where /root/reference exists; the
GPU box does not have it).  Imports the reference's src/duwu/trainer/optimizers.py by path and runs ``AdamWFP16`` on the CPU over
three parameter tensors for 6 steps.  Output: data only (initial parameters, every step's gradients, and after every step the
parameters, both moments as fp16 bits and the ``accumulated_decay`` values, with the initial draws); no reference source text.

How the reference is driven.  ``AdamWFP16.step`` hands ``state["exp_avg"].float()`` to ``adamw_make_step`` and afterwards stores
``state["exp_avg"].half()``: while the state is fp16, ``.float()`` is a copy and the updated moments are dropped, so a freshly
constructed instance keeps both moments at zero for ever.  The rule the class states (optimizers.py:96-120 as called from
:78-92) -- and the one ``uwu_adamw_fp16_step`` implements -- takes effect when the state arrives as fp32, which is what
``torch.optim.Optimizer.load_state_dict`` makes of it (floating-point state is cast to the parameter's dtype).  So every step
here is taken by the reference class right after ``load_state_dict(state_dict())``, the state a resumed run is in: the moments
are widened losslessly, updated in place, and rounded to fp16 by the class's own ``.half()``.  A zero-``lr`` step with zero
gradients first lets the class create its state and make its own phase draws.

    python tools/make_golden_optim.py [--reference /root/reference]
"""
import argparse
import copy
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "adamw_fp16_3tensors.npz")

LENGTHS = (1000, 1537, 771)  # not all multiples of 8 (nor of 4)
STEPS = 6
LR, WD, BETAS, EPS = 1e-3, 4.0, (0.9, 0.999), 1e-8  # lr * wd = 4e-3 per step against decay_threshold = 1e-2
SEED = 0  # (its three phase draws put the tensors on three different decay schedules: asserted below)
# slices of every tensor (fractions of its length) and their gradient scale at steps 1..6
SLICES = (
    ("normal", 0.00, 0.40, (1, 1, 1, 1, 1, 1)),  # v in the normal fp16 range
    ("small", 0.40, 0.55, (1e-2,) * 6),  # v = 1e-3 g^2 ~ 1e-7: subnormal in fp16
    ("tiny", 0.55, 0.70, (1e-4, 1e-4, 1e-4, 1e-5, 1e-5, 1e-5)),  # v ~ 1e-11: exactly zero in fp16 (m subnormal)
    ("huge", 0.70, 0.85, (1, 1, 3e4, 1, 1, 1)),  # v overflows to inf at step 3 and stays there
    ("zero", 0.85, 1.00, (0,) * 6),  # g = 0 throughout
)


def load_reference(root):
    spec = importlib.util.spec_from_file_location("ref_optimizers", os.path.join(root, "src", "duwu", "trainer", "optimizers.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def slice_bounds(n):
    return {name: (int(round(a * n)), int(round(b * n))) for name, a, b, _ in SLICES}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    a = ap.parse_args()
    ref = load_reference(a.reference)

    gen = torch.Generator().manual_seed(SEED)
    params = [torch.nn.Parameter(torch.randn(n, generator=gen) * 0.1) for n in LENGTHS]
    grads = []  # [step][tensor]
    for t in range(STEPS):
        row = []
        for n in LENGTHS:
            g = torch.randn(n, generator=gen)
            for name, (lo, hi) in slice_bounds(n).items():
                g[lo:hi] *= dict((s[0], s[3]) for s in SLICES)[name][t]
            row.append(g)
        grads.append(row)
    p0 = np.concatenate([p.detach().numpy().copy() for p in params])

    opt = ref.AdamWFP16(params, lr=0.0, betas=BETAS, eps=EPS, weight_decay=WD)
    torch.manual_seed(SEED)
    for p in params:  # state creation + the class's own draws (optimizers.py:55-66): lr = 0 and g = 0 move nothing
        p.grad = torch.zeros_like(p)
    opt.step()
    assert np.array_equal(np.concatenate([p.detach().numpy() for p in params]), p0)
    for p in params:
        opt.state[p]["step"] = 0.0
    opt.param_groups[0]["lr"] = LR
    acc0 = np.array([opt.state[p]["accumulated_decay"] for p in params], dtype=np.float64)
    torch.manual_seed(SEED)  # the draws are what the documented rule gives from this seed, in tensor order
    assert np.array_equal(acc0, [float(torch.rand([]) * ref.AdamWFP16.decay_threshold) for _ in params])

    P, M, V, ACC = [], [], [], []
    for t in range(STEPS):
        opt.load_state_dict(copy.deepcopy(opt.state_dict()))  # the moments arrive as fp32, as in a resumed run
        for p, g in zip(params, grads[t]):
            assert opt.state[p]["exp_avg"].dtype == torch.float32
            p.grad = g.clone()
        opt.step()
        for p in params:
            assert opt.state[p]["exp_avg"].dtype == torch.float16 and opt.state[p]["exp_avg_sq"].dtype == torch.float16
        P.append(np.concatenate([p.detach().numpy().copy() for p in params]))
        M.append(np.concatenate([opt.state[p]["exp_avg"].numpy().view(np.uint16).copy() for p in params]))
        V.append(np.concatenate([opt.state[p]["exp_avg_sq"].numpy().view(np.uint16).copy() for p in params]))
        ACC.append([opt.state[p]["accumulated_decay"] for p in params])
    G = np.stack([np.concatenate([g.numpy() for g in row]) for row in grads])
    P, M, V, ACC = np.stack(P), np.stack(M), np.stack(V), np.array(ACC, dtype=np.float64)

    # ---- what the fixture must contain
    decayed = ACC == 0.0  # [step][tensor]: the accumulated amount was applied and subtracted (:71-76)
    assert decayed.any(0).all(), "every tensor decays at least once"
    assert (~decayed).any(0).all(), "every tensor has a step without decay"
    assert len({tuple(decayed[:, i]) for i in range(len(LENGTHS))}) == len(LENGTHS), "the tensors decay on different steps"
    v = V.view(np.float16)
    m = M.view(np.float16)
    expo = (V >> 10) & 31
    offs = np.concatenate([[0], np.cumsum(LENGTHS)])
    sel = {name: np.concatenate([np.arange(offs[i] + lo, offs[i] + hi) for i, n in enumerate(LENGTHS)
                                 for lo, hi in [slice_bounds(n)[name]]]) for name, *_ in SLICES}
    assert ((expo[:, sel["normal"]] > 0) & (expo[:, sel["normal"]] < 31)).mean() > 0.5  # v in the normal fp16 range
    assert ((expo[:, sel["small"]] == 0) & (V[:, sel["small"]] != 0)).mean() > 0.5  # v subnormal
    assert (V[:, sel["tiny"]] == 0).all() and (G[:, sel["tiny"]] != 0).all()  # v exactly zero though g is not
    assert (M[:, sel["tiny"]] != 0).any() and np.isfinite(m).all()
    inf3 = np.isinf(v[2, sel["huge"]])
    assert inf3.mean() > 0.5 and not np.isinf(v[1]).any()  # v overflows at step 3 ...
    assert all(np.isinf(v[t, sel["huge"]][inf3]).all() for t in range(3, STEPS))  # ... and stays inf afterwards
    assert (G[:, sel["zero"]] == 0).all() and (M[:, sel["zero"]] == 0).all() and (V[:, sel["zero"]] == 0).all()
    assert np.isfinite(P).all()

    np.savez_compressed(OUT, lengths=np.array(LENGTHS), lr=LR, weight_decay=WD, betas=np.array(BETAS), eps=EPS,
                        decay_threshold=ref.AdamWFP16.decay_threshold, p0=p0, g=G, p=P, m16=M, v16=V, acc0=acc0, acc=ACC)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes); phases {acc0.tolist()}; decay steps per tensor "
          f"{[(np.nonzero(decayed[:, i])[0] + 1).tolist() for i in range(len(LENGTHS))]}")


if __name__ == "__main__":
    main()
