"""GPU: the native FID InceptionV3 block by block and whole against the plain-torch oracle (tests/inception_oracle.py), and
``compute_fid`` end to end on two folders of PNGs.

Standards.  fp32: 1e-3 relative L2 per picture, the project's parity standard.  bf16: each picture's relative L2 error against the
float64 oracle is held to twice the largest per-picture error of the oracle's own CPU-bf16 mode (folded weights and every layer's
output rounded to bf16, fp32 arithmetic) -- what bf16 storage costs, measured on the same pictures and weights, not on the code under
test.  A FID is one scalar that can pass or fail by cancellation, so in bf16 it is checked on three different splits of one set of
features, each held to twice the largest of the CPU-bf16 oracle's three deviations.
"""
import os

import pytest
import torch

from tests import inception_oracle as io

gpu = pytest.mark.gpu
N_PICS = 12
SPLITS = [(list(range(0, 6)), list(range(6, 12))), (list(range(0, 12, 2)), list(range(1, 12, 2))), ([0, 1, 2, 6, 7, 8], [3, 4, 5, 9, 10, 11])]


def _rows(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def _nchw(rows, B, H, W):
    return rows.view(B, H, W, -1).permute(0, 3, 1, 2)


@pytest.fixture(scope="module")
def random_sd():
    return io.random_state_dict(1)


@pytest.fixture(scope="module")
def models(random_sd):
    from uwudiff_amd.inception import FIDInceptionV3

    out = {}
    for dt in ("fp32", "bf16"):
        m = FIDInceptionV3(compute_dtype=dt, init_weights=False)
        m.load_state_dict(random_sd)
        out[dt] = m.cuda()
    return out


# ---------------------------------------------------------------------------------------------- blocks
@gpu
@pytest.mark.parametrize("name", ["Mixed_5c", "Mixed_6a", "Mixed_6c", "Mixed_7a", "Mixed_7b", "Mixed_7c"],
                         ids=["A", "B", "C_c7_160", "D", "E_avg", "E_max"])
def test_block_against_oracle(name, random_sd, models):
    _, cin, _, cout, hw = io.BLOCKS[name]
    g = torch.Generator().manual_seed(cin + hw)
    x = (torch.randn(2, cin, hw, hw, generator=g).relu() * 0.9).bfloat16().float()  # what a ReLU layer hands on, exact in both dtypes
    ref = io.block(random_sd, name, x.double(), "fp64")
    oracle_bf16 = float(io.rel_l2(io.block(random_sd, name, x, "bf16"), ref).max())
    for dt, tol in (("fp32", 1e-3), ("bf16", 2 * oracle_bf16)):
        m = models[dt]
        y, Ho, Wo = m.block(name, _rows(x).to(m.dtype).cuda(), 2, hw, hw)
        assert y.shape == (2 * Ho * Wo, cout) and ref.shape == (2, cout, Ho, Wo)
        err = io.rel_l2(_nchw(y.float().cpu(), 2, Ho, Wo), ref)
        print(f"[{name} {dt}] relative L2 per picture {err.tolist()} (allowed {tol:.3e}; CPU-bf16 oracle {oracle_bf16:.3e})")
        assert bool((err <= tol).all()), (dt, err, tol)


# ---------------------------------------------------------------------------------------------- whole model
@pytest.fixture(scope="module")
def pics():
    return io.pictures(N_PICS, 21)


@gpu
def test_whole_model_against_oracle(random_sd, models, pics):
    u8 = pics[:2]
    ref = io.forward(random_sd, io.preprocess(u8), "fp64")
    oracle_bf16 = float(io.rel_l2(io.forward(random_sd, io.preprocess(u8), "bf16"), ref).max())
    for dt, tol in (("fp32", 1e-3), ("bf16", 2 * oracle_bf16)):
        got = models[dt](u8.cuda())
        assert got.shape == (2, 2048) and got.dtype == torch.float32
        err = io.rel_l2(got.cpu(), ref)
        print(f"[FIDInceptionV3 {dt}] relative L2 per picture {err.tolist()} (allowed {tol:.3e}; CPU-bf16 oracle {oracle_bf16:.3e})")
        assert bool((err <= tol).all()), (dt, err, tol)
    m = models["fp32"]
    fl = u8.float() / 255  # what ToTensor yields: under normalize=True the same pixel values, so the same features
    assert torch.equal(m(fl.cuda(), normalize=True), m(u8.cuda()))
    whole = m(u8.cuda())  # chunks bound the workspace and change nothing: one picture per pass against both in one
    m.chunk = 1
    try:
        chunked = m(u8.cuda())
    finally:
        m.chunk = 128
    assert chunked.shape == (2, 2048) and float(io.rel_l2(chunked, whole).max()) <= 1e-6  # the tile variant may differ: fp32 sums reorder
    # the stem's first layer alone, so a wrong operand order does not hide in the sum
    x1, H, W = m._features(u8.cuda(), upto="Conv2d_1a_3x3")
    want = io.basic_conv(random_sd, "Conv2d_1a_3x3", io.preprocess(u8))
    assert (H, W) == (149, 149) and float(io.rel_l2(_nchw(x1.cpu(), 2, H, W), want).max()) <= 1e-5


# ---------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def folders(tmp_path_factory, pics):
    from PIL import Image

    root = tmp_path_factory.mktemp("fid")
    for side, idx in (("real", range(0, 6)), ("generated", range(6, 12))):
        (root / side).mkdir()
        for i in idx:
            Image.fromarray(pics[i].permute(1, 2, 0).numpy()).save(root / side / f"{i:02d}.png")
    return root


@pytest.fixture(scope="module")
def seeded_oracle(pics):
    """the seeded extractor's features of the twelve pictures by the oracle, in float64 and in the CPU-bf16 mode"""
    from uwudiff_amd.inception import FIDInceptionV3

    sd = FIDInceptionV3(compute_dtype="fp32").state_dict()
    x = io.preprocess(pics)
    return io.forward_batched(sd, x, "fp64"), io.forward_batched(sd, x, "bf16")


def _datasets(folders):
    from duwu.data.text_image_local import LocalImageDatasetFromFolder
    from uwudiff_amd.transforms import CenterCrop, Compose, Resize, ToTensor

    t = Compose([Resize(299), CenterCrop(299), ToTensor()])
    return LocalImageDatasetFromFolder(str(folders / "generated"), t), LocalImageDatasetFromFolder(str(folders / "real"), t)


@gpu
def test_compute_fid_end_to_end_fp32(folders, seeded_oracle):
    from duwu.metrics import compute_fid

    generated, reference = _datasets(folders)
    assert len(generated) == len(reference) == 6 and generated[0].shape == (3, 299, 299)
    got = compute_fid(generated, reference, batch_size=4, device="cuda", disable_tqdm=True, normalize=True, compute_dtype="fp32")
    assert got.dtype == torch.float32 and got.dim() == 0 and got.is_cuda
    f64 = seeded_oracle[0]
    want = io.fid_of_features(f64[:6], f64[6:])
    print(f"[compute_fid fp32] {float(got):.6f} against the oracle's {want:.6f}: relative {abs(float(got) - want) / want:.3e}")
    assert abs(float(got) - want) <= 1e-3 * want


@gpu
def test_fid_bf16_on_three_splits(pics, seeded_oracle):
    from uwudiff_amd.metrics import FrechetInceptionDistance

    f64, fbf = seeded_oracle
    metric = FrechetInceptionDistance(compute_dtype="bf16").to("cuda")
    feats = metric.inception(pics.cuda())  # extracted once
    per_pic = io.rel_l2(feats.cpu(), f64)
    print(f"[FID bf16] features: relative L2 per picture up to {float(per_pic.max()):.3e} (CPU-bf16 oracle {float(io.rel_l2(fbf, f64).max()):.3e})")
    want = [io.fid_of_features(f64[r], f64[f]) for r, f in SPLITS]
    oracle_dev = [abs(io.fid_of_features(fbf[r], fbf[f]) - w) for (r, f), w in zip(SPLITS, want)]
    allowed = 2 * max(oracle_dev)
    for (r, f), w in zip(SPLITS, want):
        metric.reset()
        metric.update_features(feats[r].contiguous(), real=True)
        metric.update_features(feats[f].contiguous(), real=False)
        got = float(metric.compute())
        print(f"[FID bf16] split {r} | {f}: {got:.6f} against {w:.6f}, deviation {abs(got - w):.3e} (allowed {allowed:.3e}; the CPU-bf16 "
              f"oracle's three: {[f'{d:.3e}' for d in oracle_dev]})")
        assert abs(got - w) <= allowed


@gpu
def test_identical_sets_reset_and_launcher(pics, folders, tmp_path, capsys):
    from uwudiff_amd.metrics import FrechetInceptionDistance

    metric = FrechetInceptionDistance(reset_real_features=False, compute_dtype="bf16").to("cuda")
    metric.inception.chunk = 5  # every update below is larger than a chunk, or not a multiple of it
    u8 = pics.cuda()
    metric.update(u8[:8], real=True)
    metric.update(u8[8:], real=True)
    metric.update(u8[:5], real=False)
    metric.update(u8[5:], real=False)  # the same twelve pictures on both sides, split differently
    D = metric.num_features
    host = metric.acc[True].cpu()
    n, mean = host[0], host[1:1 + D] / host[0]
    tr = float((host[1 + D:].view(D, D).diagonal() - n * mean * mean).sum() / (n - 1))
    same = float(metric.compute())
    print(f"[FID] identical sets: {same:.3e} with tr S = {tr:.3e} ({same / tr:.3e} of it)")
    assert abs(same) < 1e-6 * tr
    real_before = metric.acc[True].clone()
    metric.reset()  # reset_real_features=False keeps the real statistics
    assert metric.acc[False] is None and torch.equal(metric.acc[True], real_before)
    with pytest.raises(RuntimeError, match="more than one sample"):
        metric.compute()
    metric.update(u8[6:], real=False)
    kept = float(metric.compute())
    fresh = FrechetInceptionDistance(compute_dtype="bf16").to("cuda")  # reset_real_features=True drops both
    fresh.update(u8, real=True)
    fresh.update(u8[6:], real=False)
    assert float(fresh.compute()) == kept and kept > 0
    fresh.reset()
    assert fresh.acc[True] is None and fresh.acc[False] is None
    # the launcher on the new config with the two folders written in
    import importlib.util

    from tests.conftest import ROOT

    spec = importlib.util.spec_from_file_location("launcher_fid_gpu", os.path.join(ROOT, "test_scripts", "test_metrics.py"))
    launcher = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(launcher)
    from uwudiff_amd.config import load_yaml

    cfg = load_yaml(os.path.join(ROOT, "configs", "demo_metrics_fid.yaml"))
    cfg.generated_image_dir = str(folders / "generated")
    cfg.metrics[0]["ref_dataset"]["image_dir"] = str(folders / "real")
    import yaml

    (tmp_path / "fid.yaml").write_text(yaml.safe_dump(_plain(cfg)))
    out = launcher.main(["--configs", str(tmp_path / "fid.yaml")])
    assert list(out) == ["FID"] and float(out["FID"]) > 0
    assert "FID: " in capsys.readouterr().out


def _plain(x):
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items()}
    if isinstance(x, list):
        return [_plain(v) for v in x]
    return x
