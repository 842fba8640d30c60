"""CPU: the fused Lion / AdamWFP16 optimizers' host side -- target resolution, exported symbols, the fp64 restatement of the
AdamWFP16 step against the fixture recorded from the reference class (tools/make_golden_optim.py), the data-parallel phase draw
and argument validation.  The restatements here are the oracles of tests/test_optimizers_gpu.py."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.conftest import ROOT

FIXTURE = os.path.join(ROOT, "tests", "golden", "adamw_fp16_3tensors.npz")
NEW_SYMBOLS = ("uwu_lion_step", "uwu_adamw_fp16_step", "uwu_param_decay")


# ------------------------------------------------------------------------------------------------------------ restatements
def half(x):
    """fp64 -> fp16 as ``torch.Tensor.half()``: round to nearest even, subnormals kept, overflow -> inf"""
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float16)


def adamw_fp16_step(p, g, m16, v16, step, lr, betas, eps):
    """One AdamWFP16 update in fp64 (reference optimizers.py:96-120 as called from :78-92): the moments are read from fp16, the
    parameters move by the unrounded new moments, which are then rounded to fp16.  Returns (p, m16, v16, m, v)."""
    b1, b2 = betas
    g = np.asarray(g, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        m = m16.astype(np.float64) * b1 + (1 - b1) * g
        v = v16.astype(np.float64) * b2 + (1 - b2) * g * g
        p = np.asarray(p, dtype=np.float64) - lr * np.sqrt(1 - b2 ** step) * m / (np.sqrt(v) + eps)
    return p, half(m), half(v), m, v


def decay_bookkeeping(acc, lr, weight_decay, threshold):
    """optimizers.py:71-76 for a list of tensors: returns (new accumulated values, amount applied to each tensor this step)"""
    new, applied = [], []
    for a in acc:
        a = a + weight_decay * lr
        d = a if a > threshold else 0.0
        new.append(a - d)
        applied.append(d)
    return new, applied


def lion_step(p, g, m, lr, betas, weight_decay):
    """One lion_pytorch.Lion update in fp64 (Chen et al. 2023, Algorithm 2).  Returns (p, m, c, magnitude of c's two terms)."""
    b1, b2 = betas
    p, g, m = (np.asarray(a, dtype=np.float64) for a in (p, g, m))
    c = b1 * m + (1 - b1) * g
    p = p * (1 - lr * weight_decay) - lr * np.sign(c)
    return p, b2 * m + (1 - b2) * g, c, np.abs(b1 * m) + np.abs((1 - b1) * g)


def fp16_neighbours(a_bits, b_bits):
    """(equal, adjacent) masks of two uint16 arrays of fp16 bit patterns: adjacent = next representable value on either side"""
    def key(u):  # monotone integer order of the fp16 values (sign-magnitude -> two's complement, -0 == +0)
        u = u.astype(np.int32)
        return np.where(u & 0x8000, -(u & 0x7FFF), u)
    d = np.abs(key(a_bits) - key(b_bits))
    return d == 0, d == 1


def fp16_special(bits):
    """elements whose fp16 value is inf, zero or subnormal (exponent field all ones or zero)"""
    e = (bits >> 10) & 31
    return (e == 0) | (e == 31)


def load_fixture():
    f = np.load(FIXTURE)
    lengths = [int(n) for n in f["lengths"]]
    hp = dict(lr=float(f["lr"]), weight_decay=float(f["weight_decay"]), betas=tuple(float(b) for b in f["betas"]),
              eps=float(f["eps"]), threshold=float(f["decay_threshold"]))
    return f, lengths, hp


def fixture_state_before(f, t):
    """(p, m16 bits, v16 bits, accumulated_decay) the fixture holds before step t (0-based)"""
    if t == 0:
        n = f["p0"].size
        return f["p0"], np.zeros(n, np.uint16), np.zeros(n, np.uint16), [float(a) for a in f["acc0"]]
    return f["p"][t - 1], f["m16"][t - 1], f["v16"][t - 1], [float(a) for a in f["acc"][t - 1]]


def restated_fixture_step(f, lengths, hp, t, p, m_bits, v_bits, acc):
    """the restatement applied to one step of the fixture's gradients from the given state"""
    p, m16, v16, _, _ = adamw_fp16_step(p, f["g"][t], m_bits.view(np.float16), v_bits.view(np.float16), t + 1, hp["lr"],
                                        hp["betas"], hp["eps"])
    acc, applied = decay_bookkeeping(acc, hp["lr"], hp["weight_decay"], hp["threshold"])
    off = 0
    for n, d in zip(lengths, applied):
        if d > 0:
            p[off:off + n] *= 1 - d
        off += n
    return p, m16.view(np.uint16), v16.view(np.uint16), acc, applied


# ------------------------------------------------------------------------------------------------------------ tests
def test_targets_resolve_to_the_fused_classes():
    from duwu.utils import instantiate_any
    from uwudiff_amd.config import load_yaml
    from uwudiff_amd.optim import FlatFusedOptimizer, FusedAdamW, FusedAdamWFP16, FusedLion

    assert instantiate_any("duwu.trainer.optimizers.AdamWFP16") is FusedAdamWFP16
    assert instantiate_any("lion_pytorch.Lion") is FusedLion
    assert all(issubclass(c, FlatFusedOptimizer) for c in (FusedAdamW, FusedLion, FusedAdamWFP16))
    assert FusedAdamWFP16.decay_threshold == 1e-2

    def targets(node):
        if isinstance(node, dict):
            for k, v in node.items():
                if k in ("_target_", "optimizer", "lr_scheduler") and isinstance(v, str):
                    yield v
                else:
                    yield from targets(v)
        elif isinstance(node, list):
            for v in node:
                yield from targets(v)

    base = load_yaml(os.path.join(ROOT, "configs", "demo_training_latent.yaml"))
    for name, cls in (("demo_training_lion.yaml", FusedLion), ("demo_training_adamw_fp16.yaml", FusedAdamWFP16)):
        cfg = load_yaml(os.path.join(ROOT, "configs", name))
        found = list(targets(cfg))
        assert len(found) >= 6
        for t in found:
            assert instantiate_any(t) is not None, t
        assert instantiate_any(cfg["trainer"]["optimizer"]) is cls
        # demo_training_latent.yaml with only the optimizer and its options changed
        a, b = dict(cfg["trainer"]), dict(base["trainer"])
        for k in ("optimizer", "opt_config"):
            a.pop(k), b.pop(k)
        assert a == b and {k: v for k, v in cfg.items() if k != "trainer"} == {k: v for k, v in base.items() if k != "trainer"}


def test_library_exports_the_optimizer_entry_points():
    from uwudiff_amd import build, lib

    build.build(verbose=False)
    cd = ctypes.CDLL(lib.LIB_PATH)
    arity = {"uwu_lion_step": 13, "uwu_adamw_fp16_step": 15, "uwu_param_decay": 5}
    for s in NEW_SYMBOLS:
        assert hasattr(cd, s), s
        assert s in lib.exported_symbols() and len(lib._SIGS[s][1]) == arity[s]


def test_restatement_reproduces_the_reference_fixture():
    """The fp64 restatement, replayed over the fixture's gradients from the fixture's initial draws and carrying its own state,
    gives the reference's recorded moments (bit-equal or the adjacent fp16 value), decay steps, accumulated_decay and parameters."""
    f, lengths, hp = load_fixture()
    p, m_bits, v_bits, acc = fixture_state_before(f, 0)
    steps = f["g"].shape[0]
    assert steps == 6 and sum(lengths) == p.size and any(n % 8 for n in lengths)
    adjacent = total = 0
    for t in range(steps):
        p, m_bits, v_bits, acc, applied = restated_fixture_step(f, lengths, hp, t, p, m_bits, v_bits, acc)
        for mine, ref in ((m_bits, f["m16"][t]), (v_bits, f["v16"][t])):
            eq, adj = fp16_neighbours(mine, ref)
            assert (eq | adj).all(), (t, int((~(eq | adj)).sum()))
            adjacent += int(adj.sum())
            total += adj.size
        np.testing.assert_allclose(acc, f["acc"][t], rtol=0, atol=1e-15)
        assert [d > 0 for d in applied] == [a == 0.0 for a in f["acc"][t]], t  # decay on the reference's steps and tensors
        np.testing.assert_allclose(p, f["p"][t], rtol=1e-5, atol=1e-6)
    print(f"adjacent fp16 roundings: {adjacent} of {total}")
    assert adjacent <= 0.001 * total  # far below the 1 % the GPU comparison allows
    dec = np.array([[a == 0.0 for a in row] for row in f["acc"]])
    assert dec.any(0).all() and (~dec).any(0).all() and len({tuple(c) for c in dec.T}) == len(lengths)
    v_last = f["v16"][-1]
    assert np.isinf(v_last.view(np.float16)).any() and (fp16_special(v_last) & (v_last != 0) & ~np.isinf(v_last.view(np.float16))).any()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _phase_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from uwudiff_amd.optim import FusedAdamWFP16, draw_decay_phases

    torch.manual_seed(1215 + rank)  # test_train.py:68-69: seed + global_rank
    own = [float(torch.rand([]) * FusedAdamWFP16.decay_threshold) for _ in range(5)]
    torch.manual_seed(1215 + rank)
    got = draw_decay_phases(5, FusedAdamWFP16.decay_threshold)
    q.put((rank, own, got))
    dist.destroy_process_group()


def test_decay_phases_are_rank0s_on_every_rank():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_phase_worker, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(world))
    for p in ps:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, own0, got0), (_, own1, got1) = res
    assert own0 != own1  # per-rank seeds differ: the reference's replicas would decay on different steps
    assert got0 == own0 and got1 == own0
    assert all(isinstance(x, float) and 0 <= x < 1e-2 for x in got1)


def test_single_process_draw_follows_the_global_generator():
    from uwudiff_amd.optim import draw_decay_phases

    torch.manual_seed(0)
    want = [float(torch.rand([]) * 1e-2) for _ in range(3)]
    torch.manual_seed(0)
    assert draw_decay_phases(3, 1e-2) == want
    f = np.load(FIXTURE)
    assert want == [float(a) for a in f["acc0"]]  # the fixture's draws are the reference's from the same seed


def test_argument_validation():
    from uwudiff_amd import lib
    from uwudiff_amd.optim import FusedAdamWFP16, FusedLion

    def p():
        return [torch.nn.Parameter(torch.zeros(16))]

    for kw, msg in ((dict(eps=-1.0), "Invalid epsilon value"), (dict(betas=(1.0, 0.999)), "Invalid beta parameter at index 0"),
                    (dict(betas=(0.9, 1.0)), "Invalid beta parameter at index 1"), (dict(betas=(-0.1, 0.9)), "index 0"),
                    (dict(weight_decay=-1e-3), "Invalid weight_decay value")):
        with pytest.raises(ValueError, match=msg):
            FusedAdamWFP16(p(), **kw)
    with pytest.raises(TypeError):
        FusedAdamWFP16(p(), 1e-3)  # keyword-only, as the reference's
    with pytest.raises(NotImplementedError):
        FusedAdamWFP16(p(), differentiable=True)
    with pytest.raises(NotImplementedError):
        FusedLion(p(), decoupled_weight_decay=True)
    FusedLion(p(), use_triton=True)  # accepted and ignored
    with pytest.raises(ValueError):
        FusedLion(p(), lr=0.0)
    with pytest.raises(ValueError):
        FusedLion(p(), betas=(0.9, 1.5))
    for make in (lambda q: FusedLion(q), lambda q: FusedAdamWFP16(q, segments=[(0, 16)])):
        q = p()
        q[0].grad = torch.ones(16)
        opt = make(q)
        with pytest.raises(lib.UwuError):  # no CPU path
            opt.step()
        assert torch.equal(q[0].detach(), torch.zeros(16)) and not opt.state[q[0]]
    two = [torch.nn.Parameter(torch.zeros(8)), torch.nn.Parameter(torch.zeros(8))]
    with pytest.raises(ValueError):
        FusedAdamWFP16(two, segments=[(0, 8)])


def test_loaded_moments_return_to_fp16():
    """``Optimizer.load_state_dict`` casts floating-point state to the parameter's dtype; the post-hook brings the moments back to
    fp16 without loss (inf and subnormals included) and leaves ``accumulated_decay`` a list of python floats."""
    from uwudiff_amd.optim import FusedAdamWFP16

    bits = torch.from_numpy(np.array([0x0000, 0x0001, 0x03FF, 0x0400, 0x7BFF, 0x7C00, 0x8001, 0x3C01], np.uint16).view(np.int16))
    q = torch.nn.Parameter(torch.zeros(8))
    opt = FusedAdamWFP16([q], segments=[(0, 3), (3, 5)])
    sd = {"state": {0: {"step": 3, "exp_avg": bits.view(torch.float16).clone(), "exp_avg_sq": bits.view(torch.float16).clone(),
                        "accumulated_decay": [0.00125, 0.0]}},
          "param_groups": opt.state_dict()["param_groups"]}
    opt.load_state_dict(sd)
    st = opt.state[q]
    assert st["exp_avg"].dtype == torch.float16 and st["exp_avg_sq"].dtype == torch.float16
    assert torch.equal(st["exp_avg"].view(torch.int16), bits) and torch.equal(st["exp_avg_sq"].view(torch.int16), bits)
    assert st["accumulated_decay"] == [0.00125, 0.0] and all(type(a) is float for a in st["accumulated_decay"])
    assert st["step"] == 3


def test_trainer_passes_the_layout_as_segments():
    from uwudiff_amd.optim import flat_segments

    class _Store:
        registry = {"a.weight": (0, (3, 5)), "a.bias": (64, (3,)), "b": (128, (70,))}

    class _Flat:
        P = _Store()

    class _Adapters:
        offsets = {("x", "lora_down.weight"): (0, (2, 9)), ("x", "lora_up.weight"): (64, (4, 2))}

    assert flat_segments(_Flat()) == [(0, 15), (64, 3), (128, 70)]
    assert flat_segments(_Adapters()) == [(0, 18), (64, 8)]
