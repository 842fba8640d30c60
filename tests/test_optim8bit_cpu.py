"""CPU: the host side of the 8-bit block-wise optimizers (uwudiff_amd/optim.py: FusedAdamW8bit, FusedLion8bit) -- the code tables,
the aliases, the constructor refusals, the refusal of a CPU parameter and the block scheduling over chunks -- and the properties
of the fixtures tests/test_optim8bit_gpu.py relies on (tests/optim8bit_oracle.py)."""
import numpy as np
import pytest
import torch

from tests import optim8bit_oracle as O


# ------------------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("signed", [True, False])
def test_tables_have_256_increasing_entries_and_the_pinned_values(signed):
    from uwudiff_amd.optim import dynamic_map

    T = dynamic_map(signed)
    assert T.dtype == torch.float32 and T.shape == (256,)
    T = T.numpy()
    assert (np.diff(T) > 0).all() and T.min() >= -1 and T.max() <= 1
    assert np.array_equal(T, O.dynamic_map(signed))  # the oracle's restatement, entry for entry
    close = lambda a, b: a == pytest.approx(b, rel=1e-6, abs=0)  # noqa: E731
    if signed:
        assert close(T[0], -0.99296874) and T[127] == 0 and close(T[128], 5.5e-7) and T[255] == 1
        assert np.diff(T).max() == pytest.approx(0.0140625, rel=0, abs=2.0 ** -23)  # (two fp32 entries near 1)
        assert np.array_equal(T[128:255], -T[126::-1][:127])  # both signs of every midpoint
    else:
        assert T[0] == 0 and close(T[1], 3.25e-7) and T[255] == 1
        assert np.diff(T).max() == pytest.approx(0.00703125, rel=0, abs=2.0 ** -23)
    assert int(O.nearest(T, 0.0)) == (127 if signed else 0)  # the zero code


def test_nearest_breaks_a_tie_towards_the_lower_index():
    T = np.array([-1.0, 0.0, 0.5, 1.0])
    assert O.nearest(T, [-2.0, -0.5, 0.25, 0.26, 0.75, 2.0]).tolist() == [0, 0, 1, 2, 2, 3]


# ------------------------------------------------------------------------------------------------------------ classes
def test_aliases_resolve_to_the_classes():
    from uwudiff_amd.config import instantiate_any
    from uwudiff_amd.optim import FlatFusedOptimizer, FusedAdamW8bit, FusedLion8bit

    assert instantiate_any("bitsandbytes.optim.AdamW8bit") is FusedAdamW8bit
    assert instantiate_any("bitsandbytes.optim.Lion8bit") is FusedLion8bit
    assert issubclass(FusedAdamW8bit, FlatFusedOptimizer) and issubclass(FusedLion8bit, FlatFusedOptimizer)


def test_constructor_signatures_are_the_package_s():
    import inspect

    from uwudiff_amd.optim import FusedAdamW8bit, FusedLion8bit

    sig = lambda cls: [(k, v.default) for k, v in list(inspect.signature(cls.__init__).parameters.items())[2:]]  # noqa: E731
    assert sig(FusedAdamW8bit) == [("lr", 1e-3), ("betas", (0.9, 0.999)), ("eps", 1e-8), ("weight_decay", 1e-2), ("amsgrad", False),
                                   ("optim_bits", 32), ("args", None), ("min_8bit_size", 4096), ("percentile_clipping", 100),
                                   ("block_wise", True), ("is_paged", False)]
    assert sig(FusedLion8bit) == [("lr", 1e-4), ("betas", (0.9, 0.99)), ("weight_decay", 0), ("min_8bit_size", 4096),
                                  ("percentile_clipping", 100), ("block_wise", True), ("is_paged", False)]


@pytest.mark.parametrize("kw", [{"percentile_clipping": 5}, {"block_wise": False}, {"is_paged": True}])
@pytest.mark.parametrize("name", ["FusedAdamW8bit", "FusedLion8bit"])
def test_constructors_refuse_what_is_not_built(name, kw):
    from uwudiff_amd import optim

    p = torch.nn.Parameter(torch.zeros(8))
    with pytest.raises(NotImplementedError, match=name):
        getattr(optim, name)([p], **kw)
    getattr(optim, name)([p], min_8bit_size=1)  # accepted (and ignored)


def test_adamw8bit_refuses_amsgrad():
    from uwudiff_amd.optim import FusedAdamW8bit

    with pytest.raises(NotImplementedError, match="amsgrad"):
        FusedAdamW8bit([torch.nn.Parameter(torch.zeros(8))], amsgrad=True)


@pytest.mark.parametrize("name", ["FusedAdamW8bit", "FusedLion8bit"])
def test_a_cpu_parameter_is_refused(name):
    from uwudiff_amd import lib as L
    from uwudiff_amd import optim

    p = torch.nn.Parameter(torch.zeros(512))
    p.grad = torch.ones(512)
    opt = getattr(optim, name)([p])
    with pytest.raises(L.UwuError, match="no CPU path"):
        opt.step()
    assert not p.detach().any() and not opt.state[p]


def test_load_state_dict_brings_the_codes_back_to_uint8():
    """torch casts the state tensors of an fp32 parameter to fp32 on load; the post-hook casts the codes back (no GPU needed: the
    state is put there by hand)"""
    from uwudiff_amd.optim import FusedAdamW8bit, dynamic_map

    def make():
        p = torch.nn.Parameter(torch.zeros(300))
        return p, FusedAdamW8bit([p])

    p, opt = make()
    codes = torch.arange(300, dtype=torch.int64).remainder(256).to(torch.uint8)
    opt.state[p] = {"step": 4, "state1": codes.clone(), "state2": codes.flip(0).clone(), "absmax1": torch.tensor([0.5, 2.0]),
                    "absmax2": torch.tensor([1e-4, 3.0]), "qmap1": dynamic_map(True), "qmap2": dynamic_map(False)}
    sd = opt.state_dict()
    p2, opt2 = make()
    opt2.load_state_dict(sd)
    st = opt2.state[p2]
    assert st["state1"].dtype == torch.uint8 and torch.equal(st["state1"], codes)
    assert st["state2"].dtype == torch.uint8 and torch.equal(st["state2"], codes.flip(0))
    assert st["step"] == 4 and torch.equal(st["absmax1"], torch.tensor([0.5, 2.0])) and torch.equal(st["qmap2"], dynamic_map(False))


# ------------------------------------------------------------------------------------------------------------ scheduling
def _replay(n, chunks):
    from uwudiff_amd.optim import BlockSchedule

    sched = BlockSchedule(n)
    seen = np.zeros(n, bool)  # elements whose chunk has arrived
    count = np.zeros(-(-n // 256), int)  # launches per block
    for off, ln in chunks:
        seen[off:off + ln] = True
        for e0, e1 in sched.add(off, ln):
            assert e0 % 256 == 0 and (e1 % 256 == 0 or e1 == n) and 0 <= e0 < e1 <= n
            assert seen[e0:e1].all(), "a block was given out before all of its chunks"
            count[e0 // 256:-(-e1 // 256)] += 1
    return sched, seen, count


@pytest.mark.parametrize("n", [3 * 256 + 37, 4096, 10 * 256 + 4])
def test_blocks_are_given_out_once_and_never_before_their_chunks(n):
    # offsets that are multiples of 4 and not of 256, in non-ascending order (the early slices of the tail first, then the rest)
    cuts = [0, 100, 260, 516, (n - 40) // 4 * 4, n]
    chunks = [(a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    assert all(off % 4 == 0 for off, _ in chunks) and sum(off % 256 != 0 for off, _ in chunks) >= 3
    for order in ([4, 2, 3, 0, 1], [4, 3, 2, 1, 0], [1, 3, 0, 4, 2], [0, 1, 2, 3, 4]):
        sched, seen, count = _replay(n, [chunks[i] for i in order])
        assert seen.all() and (count == 1).all(), (order, count)
        assert sched.pending() == []


def test_a_maximal_run_is_one_launch_and_partial_cover_is_reported():
    from uwudiff_amd.optim import BlockSchedule

    s = BlockSchedule(2048)
    assert s.add(1000, 1048) == [(1024, 2048)]  # blocks 4-7 whole; block 3 still waits for [768, 1000)
    assert s.pending() == [(1000, 1024)]
    assert s.add(0, 4) == [] and s.add(4, 996) == [(0, 1024)]
    assert s.pending() == []
    assert s.add(0, 2048) == []  # nothing twice
    with pytest.raises(ValueError):
        s.add(2040, 16)
    whole = BlockSchedule(805)
    assert whole.add(0, 805) == [(0, 805)]


# ------------------------------------------------------------------------------------------------------------ fixtures
def test_the_fixtures_keep_an_fp32_restatement_on_the_oracle_s_codes():
    """The GPU test allows 0.1 % of the elements a code other than the oracle's own; at its shapes that is less than one element.
    The seeded fixtures are chosen so that the rule restated in fp32 (the kernel's operation order) picks the fp64 oracle's code on
    every element, with every ratio further than 1e-4 of the local table gap from a decision boundary (fp32 rounding moves a ratio
    by some 1e-7 of its size)."""
    T1, T2 = O.dynamic_map(True), O.dynamic_map(False)
    for n in (3 * 256 + 37, 256):
        for later in (False, True):
            p, g, m, v = O.fixture(n, later)
            c1, a1 = O.quantise(T1, m)[1:]
            c2, a2 = O.quantise(T2, v)[1:]
            a1, a2 = a1.astype(np.float32), a2.astype(np.float32)
            for scale in (np.float32(1.0), np.float32(0.5) * np.float32(0.37)):
                step = 7 if later else 1
                o = O.adamw8_step(p, g.astype(np.float64) * float(scale), c1, a1, c2, a2, T1, T2, step, **O.HP)
                f = O.adamw8_step(p, g * scale, c1, a1, c2, a2, T1, T2, step, **O.HP, ft=np.float32)
                assert np.array_equal(o["c1"], f["c1"]) and np.array_equal(o["c2"], f["c2"])
                assert min(O.boundary_margin(T1, o["x1"]).min(), O.boundary_margin(T2, o["x2"]).min()) > 1e-4
                lo = O.lion8_step(p, g.astype(np.float64) * float(scale), c1, a1, T1, **O.LION_HP)
                lf = O.lion8_step(p, g * scale, c1, a1, T1, **O.LION_HP, ft=np.float32)
                assert np.array_equal(lo["c1"], lf["c1"]) and O.boundary_margin(T1, lo["x1"]).min() > 1e-4
            if n > 256:  # the cases the fixture is there for
                assert not a1[1] if not later else a1[1] > 0
                assert o["a1"][1] == (0 if not later else pytest.approx(0.9 * np.abs(o["m_old"][256:512]).max()))  # zero gradient: m decays
                zero = np.delete(np.arange(512, 768), 17)
                assert (o["c1"][zero] == 127).all() and (o["c2"][zero] == 0).all() and o["c1"][512 + 17] == 255
                assert o["c1"][5] == 0 and o["x1"][5] == -1 and o["x1"][n - 3] == 1


def test_the_quality_guard_s_oracle_figure():
    """rms distance of the oracle's own 8-bit run from exact fp64 AdamW on the fixed quadratic problem after 200 steps: 0.00945
    (the parameters themselves have rms 0.176 by then).  The GPU test allows the kernel twice this."""
    pe, pq = O.quadratic_runs()
    rms = float(np.sqrt(np.mean((pq - pe) ** 2)))
    print(f"oracle 8-bit run: rms distance from exact AdamW {rms:.5f}, rms of the parameters {float(np.sqrt(np.mean(pe ** 2))):.4f}")
    assert rms == pytest.approx(0.00945, rel=0.02)


def test_the_adamw8bit_config_is_the_latent_config_with_the_optimizer_swapped():
    import os

    from tests.conftest import ROOT
    from uwudiff_amd.config import instantiate_any, load_yaml
    from uwudiff_amd.optim import FusedAdamW8bit

    base = load_yaml(os.path.join(ROOT, "configs", "demo_training_latent.yaml"))
    cfg = load_yaml(os.path.join(ROOT, "configs", "demo_training_adamw8bit.yaml"))
    assert cfg["trainer"]["optimizer"] == "bitsandbytes.optim.AdamW8bit"
    assert instantiate_any(cfg["trainer"]["optimizer"]) is FusedAdamW8bit
    base["trainer"]["optimizer"] = cfg["trainer"]["optimizer"]
    assert cfg == base
