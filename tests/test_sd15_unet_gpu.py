"""The Stable Diffusion 1.x UNet layout (four levels, one head count for every level, 1x1-convolution proj_in / proj_out, no
pooled-text conditioning) against the fp32 CPU oracle, at the smallest widths that keep the family's three head widths:
channels (40, 80, 160, 160) with ONE head per level give d = 40, 80, 160.

Bars: tests/test_unet_gpu.py (fp32 1e-3 / 2e-3; bf16 4e-2 / 0.12) and the LyCORIS bf16 case (4e-2 on the whole gradient)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SD_TINY = dict(in_channels=4, out_channels=4, block_out_channels=(40, 80, 160, 160), layers_per_block=1,
               down_block_types=("CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"),
               up_block_types=("UpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D"),
               transformer_layers_per_block=1, attention_head_dim=1, cross_attention_dim=24, norm_num_groups=8,
               addition_embed_type=None, use_linear_projection=False)
ORACLE_CFG = dict(SD_TINY, transformer_layers_per_block=(1, 1, 1, 1), attention_head_dim=(1, 1, 1, 1))


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item(), ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def _is_proj(name):
    return name.endswith((".proj_in.weight", ".proj_out.weight"))


def oracle_model(seed=0):
    from oracle.unet import UNetOracle

    torch.manual_seed(seed)
    ora = UNetOracle(**ORACLE_CFG)
    with torch.no_grad():  # away from the near-zero init so every branch carries signal
        for n, p in ora.named_parameters():
            if p.dim() > 1:
                p.copy_(torch.randn_like(p) * (0.5 / p[0].numel() ** 0.5))
            elif n.endswith("bias"):
                p.copy_(torch.randn_like(p) * 0.05)
            else:
                p.copy_(1 + torch.randn_like(p) * 0.1)
    return ora


def checkpoint_of(ora):
    """the oracle's weights as an SD 1.x checkpoint stores them: proj_in / proj_out as 1x1 convolutions"""
    return {n: v[:, :, None, None].clone() if _is_proj(n) else v for n, v in ora.state_dict().items()}


def run_pair(dtype, B, S, Tk=7, seed=0, mask=None):
    from uwudiff_amd.unet import UNet2DConditionModel

    ora = oracle_model(seed)
    model = UNet2DConditionModel(SD_TINY, compute_dtype=dtype).cuda()
    model.load_state_dict(checkpoint_of(ora))
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, 4, S, S, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    ctx = torch.randn(B, Tk, SD_TINY["cross_attention_dim"], generator=g)
    dout = torch.randn(B, 4, S, S, generator=g) / (S * S)
    yo = ora(x, t, encoder_hidden_states=ctx, encoder_attention_mask=mask)[0]
    yo.backward(dout)
    y = model(x.cuda(), t.cuda(), encoder_hidden_states=ctx.cuda(),
              encoder_attention_mask=None if mask is None else mask.cuda())[0]
    y.backward(dout.cuda())
    torch.cuda.synchronize()
    og = dict(ora.named_parameters())
    grads = {n: (model.grad_tensor(n).reshape(og[n].shape), og[n].grad) for n in model.P.registry}
    return y, yo, grads, model, ora


def test_sd15_checkpoint_layout_round_trip():
    from uwudiff_amd.unet import UNet2DConditionModel

    ora = oracle_model()
    ckpt = checkpoint_of(ora)
    proj = [n for n in ckpt if _is_proj(n)]
    assert len(proj) == 20 and all(ckpt[n].dim() == 4 for n in proj)  # 10 Transformer2D stacks
    model = UNet2DConditionModel(SD_TINY, compute_dtype="fp32").cuda()
    model.load_state_dict(ckpt)
    sd = model.state_dict()
    assert set(sd) == set(ckpt)
    for k, v in ckpt.items():
        torch.testing.assert_close(sd[k].cpu(), v, rtol=0, atol=0)
    with pytest.raises(RuntimeError, match="size mismatch"):
        model.load_state_dict(ora.state_dict())  # the Linear layout is another model's
    linear = UNet2DConditionModel(dict(SD_TINY, use_linear_projection=True), compute_dtype="fp32").cuda()
    linear.load_state_dict(ora.state_dict())
    sd = linear.state_dict()
    for k, v in ora.state_dict().items():
        torch.testing.assert_close(sd[k].cpu(), v, rtol=0, atol=0)


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
def test_sd15_unet_fp32_matches_oracle(masked):
    """16 x 16 latents: T = 256 / 64 / 16 / 4, every attention on the generic fp32 kernels at d = 40 / 80 / 160"""
    mask = torch.tensor([[1, 1, 1, 1, 0, 0, 0], [1, 0, 1, 1, 1, 1, 0]]) if masked else None
    y, yo, grads, model, ora = run_pair("fp32", B=2, S=16, mask=mask)
    l2, mx = rel(y, yo)
    print(f"fp32 output: l2 {l2:.3e} max {mx:.3e}")
    assert l2 < 1e-3 and mx < 1e-3, (l2, mx)
    worst = max(((rel(g, go)[0], n) for n, (g, go) in grads.items()))
    print(f"fp32 worst gradient: {worst}")
    for name, (g, go) in grads.items():
        l2, mx = rel(g, go)
        assert l2 < 2e-3, (name, l2, mx)


def test_sd15_unet_bf16_close_to_oracle():
    """64 x 64 latents: T = 4096 / 1024 / 256 / 64, d = 40 and 80 on the MFMA kernels, d = 160 on the generic bf16 kernels"""
    y, yo, grads, _, _ = run_pair("bf16", B=1, S=64)
    l2, _ = rel(y, yo)
    print(f"bf16 output: l2 {l2:.3e}")
    assert l2 < 4e-2, l2
    cat = lambda i: torch.cat([grads[k][i].reshape(-1).double().cpu() for k in sorted(grads)])  # noqa: E731
    whole = rel(cat(0), cat(1))[0]
    worst = max(((rel(g, go)[0], n) for n, (g, go) in grads.items() if go.numel() >= 64))
    print(f"bf16 whole gradient: {whole:.3e}; worst tensor: {worst}")
    bad = {n: rel(g, go)[0] for n, (g, go) in grads.items() if go.numel() >= 64 and rel(g, go)[0] > 0.12}
    assert not bad, bad
    assert whole < 4e-2, whole


def test_sd15_unet_in_diffusion_loss_step():
    """No added_cond_kwargs at all: this family has no pooled-text / time-id conditioning."""
    from uwudiff_amd.objective import DiffusionLoss
    from uwudiff_amd.optim import FusedAdamW
    from uwudiff_amd.scheduler import EulerDiscreteScheduler
    from uwudiff_amd.unet import UNet2DConditionModel

    torch.manual_seed(0)
    m = UNet2DConditionModel(SD_TINY, compute_dtype="bf16").cuda()
    opt = FusedAdamW(m.parameters(), lr=1e-4)
    lf = DiffusionLoss(EulerDiscreteScheduler.from_pretrained("runwayml/stable-diffusion-v1-5"))
    x = torch.randn(4, 4, 16, 16, device="cuda")
    p0 = m.flat.data.clone()
    loss, aux = lf(x, m, encoder_hidden_states=torch.randn(4, 7, 24, device="cuda"))
    loss.backward()
    opt.step()
    assert torch.isfinite(loss) and aux.pred.shape == x.shape
    assert (m.flat.data - p0).abs().max().item() > 0


def test_sd15_unet_gradient_checkpointing_same_gradients():
    from uwudiff_amd.unet import UNet2DConditionModel

    model = UNet2DConditionModel(SD_TINY, compute_dtype="bf16").cuda()
    model.load_state_dict(checkpoint_of(oracle_model(5)))
    g = torch.Generator().manual_seed(6)
    B, S = 2, 32  # T = 1024 / 256 / 64 / 16: MFMA and generic attention
    x, t = torch.randn(B, 4, S, S, generator=g).cuda(), torch.randint(0, 1000, (B,), generator=g).cuda()
    ctx, dout = torch.randn(B, 7, 24, generator=g).cuda(), (torch.randn(B, 4, S, S, generator=g) / (S * S)).cuda()

    def run(ckpt):
        model.enable_gradient_checkpointing(ckpt)
        model.flat.grad = torch.zeros_like(model.flat.data)
        y = model(x, t, encoder_hidden_states=ctx)[0]
        y.backward(dout)
        torch.cuda.synchronize()
        return y.detach().clone(), model.flat.grad.clone()

    y0, g0 = run(False)
    ya, ga = run(False)  # run-to-run noise of the plain path (GroupNorm statistics are summed with fp32 atomics)
    y1, g1 = run(True)
    model.enable_gradient_checkpointing(False)
    noise_y, noise_g = rel(ya, y0)[0], ((ga - g0).norm() / g0.norm()).item()
    assert rel(y1, y0)[0] <= max(3 * noise_y, 5e-3), (rel(y1, y0), noise_y)
    err = ((g1 - g0).norm() / g0.norm()).item()
    assert err <= max(3 * noise_g, 5e-3), (err, noise_g)
