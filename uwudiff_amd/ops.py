"""Thin tensor-level wrappers over the C ABI (shape checks on the host, raw pointers to the kernels)."""
import ctypes

import torch

from . import lib as L


def gemm(a, b, *, trans_a=False, trans_b=False, bias=None, aux=None, epilogue=L.EPI_NONE, out=None, out2=None,
         c_dtype=None, split_k=1, M=None, N=None, K=None):
    """C = op(a) @ op(b)  with op(b) = b^T when trans_b is False (torch Linear weight layout [N,K])."""
    assert a.dim() == 2 and b.dim() == 2 and a.dtype == b.dtype
    if M is None:
        M, K_ = (a.shape[1], a.shape[0]) if trans_a else a.shape
        N, Kb = (b.shape[1], b.shape[0]) if trans_b else b.shape
        assert K_ == Kb, (a.shape, b.shape, trans_a, trans_b)
        K = K_
    c_dtype = c_dtype or a.dtype
    if out is None:
        out = (torch.zeros if epilogue == L.EPI_ACCUM else torch.empty)(M, N, device=a.device, dtype=c_dtype)
    if epilogue in (L.EPI_BIAS_GELU, L.EPI_BIAS_SILU) and out2 is None:
        out2 = torch.empty(M, N, device=a.device, dtype=c_dtype)
    L.call("uwu_gemm", L.ptr(a), L.ptr(b), L.ptr(out), L.ptr(out2), L.ptr(bias), L.ptr(aux), M, N, K, a.stride(0),
           b.stride(0), out.stride(0), aux.stride(0) if aux is not None else 0, int(trans_a), int(trans_b), L.dt(a),
           L.dt(out), epilogue, split_k, L.stream())
    return (out, out2) if out2 is not None else out


def add_ln_modulate_fwd(x_in, B, T, *, y=None, gate=None, shift=None, scale=None, mod_ld=0, eps=1e-6, affine=False):
    M, D = x_in.shape
    x_out = torch.empty_like(x_in) if y is not None else x_in
    h = torch.empty_like(x_in)
    mean = torch.empty(M, device=x_in.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    L.call("uwu_add_ln_modulate_fwd", L.ptr(x_in), L.ptr(y), _p(gate), _p(shift), _p(scale), mod_ld, L.ptr(x_out),
           L.ptr(h), L.ptr(mean), L.ptr(rstd), B, T, D, eps, int(affine), L.dt(x_in), L.stream())
    return x_out, h, mean, rstd


def add_ln_modulate_fwd_q8(x_in, B, T, q_scale, *, shift, scale, mod_ld, y=None, gate=None, eps=1e-6, amax=None):
    """fp8 mode: the LayerNorm output as e4m3 bytes, row-major [M, D] and transposed [D, M] (no bf16 h)."""
    M, D = x_in.shape
    x_out = torch.empty_like(x_in) if y is not None else x_in
    q8 = torch.empty(M, D, device=x_in.device, dtype=torch.uint8)
    q8t = torch.empty(D, M, device=x_in.device, dtype=torch.uint8)
    mean = torch.empty(M, device=x_in.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    L.call("uwu_add_ln_modulate_fwd_q8", L.ptr(x_in), L.ptr(y), _p(gate), _p(shift), _p(scale), mod_ld, L.ptr(x_out), L.ptr(q8), D,
           L.ptr(q8t), M, L.ptr(q_scale), L.ptr(amax), L.ptr(mean), L.ptr(rstd), B, T, D, eps, L.stream())
    return x_out, q8, q8t, mean, rstd


def add_ln_modulate_bwd(dh, x, mean, rstd, B, T, *, scale=None, dx_in=None, y=None, gate=None, mod_ld=0,
                        dshift=None, dscale=None, dgate=None, affine=False):
    M, D = x.shape
    dx = torch.empty_like(x)
    dy = torch.empty_like(x) if y is not None else None
    L.call("uwu_add_ln_modulate_bwd", L.ptr(dh), L.ptr(x), L.ptr(mean), L.ptr(rstd), _p(scale), L.ptr(dx_in),
           L.ptr(y), _p(gate), mod_ld, L.ptr(dx), L.ptr(dy), _p(dshift), _p(dscale), _p(dgate), B, T, D, int(affine),
           L.dt(x), L.stream())
    return dx, dy


def _p(t):
    """Pointer of a possibly non-contiguous *view* whose rows are addressed through an explicit stride."""
    if t is None:
        return None
    if not t.is_cuda:
        raise L.UwuError("device tensor required")
    return t.data_ptr()


def _key_bias(key_bias, B, Tk):
    if key_bias.dtype != torch.float32 or tuple(key_bias.shape) != (B, Tk):
        raise L.UwuError(f"key_bias must be fp32 [B, Tk] = [{B}, {Tk}], got {key_bias.dtype} {tuple(key_bias.shape)}")
    return L.ptr(key_bias)


def attention_fwd(q, k, v, B, Tq, Tk, H, d, scale=None, key_bias=None):
    """q/k/v: 2-D views [B*T, >=H*d] with unit inner stride (e.g. column slices of a packed projection).
    key_bias: optional fp32 [B, Tk] added to the scaled scores of every head and query (encoder_attention_mask)."""
    scale = scale if scale is not None else d ** -0.5
    o = torch.empty(B * Tq, H * d, device=q.device, dtype=q.dtype)
    lse = torch.empty(B, H, Tq, device=q.device, dtype=torch.float32)
    tail = (L.ptr(o), L.ptr(lse), B, Tq, Tk, H, d, q.stride(0), k.stride(0), v.stride(0), o.stride(0), scale, L.dt(q),
            L.stream())
    if key_bias is None:
        L.call("uwu_attention_fwd", _p(q), _p(k), _p(v), *tail)
    else:
        L.call("uwu_attention_bias_fwd", _p(q), _p(k), _p(v), _key_bias(key_bias, B, Tk), *tail)
    return o, lse


def attention_bwd(q, k, v, o, do, lse, dq, dk, dv, B, Tq, Tk, H, d, scale=None, key_bias=None):
    scale = scale if scale is not None else d ** -0.5
    # the C ABI has one leading dimension per (tensor, gradient) pair: a gradient laid out differently would be written out of bounds
    if (dq.stride(0), dk.stride(0), dv.stride(0), do.stride(0)) != (q.stride(0), k.stride(0), v.stride(0), o.stride(0)):
        raise ValueError("attention_bwd: dq / dk / dv / do must have the row strides of q / k / v / o")
    delta = torch.empty_like(lse)
    tail = (L.ptr(o), L.ptr(do), L.ptr(lse), L.ptr(delta), _p(dq), _p(dk), _p(dv), B, Tq, Tk, H, d, q.stride(0),
            k.stride(0), v.stride(0), o.stride(0), scale, L.dt(q), L.stream())
    if key_bias is None:
        L.call("uwu_attention_bwd", _p(q), _p(k), _p(v), *tail)
    else:
        L.call("uwu_attention_bias_bwd", _p(q), _p(k), _p(v), _key_bias(key_bias, B, Tk), *tail)
    return dq, dk, dv


def attention_route(Tq, Tk, d, ldq=None, ldk=None, ldv=None, ldo=None, dtype=torch.bfloat16, backward=False):
    """True where ``attention_fwd`` / ``attention_bwd`` run the MFMA kernels on this shape, False where the generic ones: the
    predicate of the dispatch itself (``uwu_attention_route``), asked on the host -- no GPU needed.  Strides default to one head's
    width; 16-byte-aligned tensors are assumed."""
    ld = [int(d if x is None else x) for x in (ldq, ldk, ldv, ldo)]
    dt = {torch.float32: L.F32, torch.bfloat16: L.BF16}[dtype]
    return bool(L.load().uwu_attention_route(int(bool(backward)), int(Tq), int(Tk), int(d), *ld, dt))


def colsum(x, out=None, accumulate=False):
    M, N = x.shape
    if out is None:
        out = torch.empty(N, device=x.device, dtype=torch.float32)
    L.call("uwu_colsum", L.ptr(x), L.dt(x), M, N, x.stride(0), L.ptr(out), int(accumulate), L.stream())
    return out


def colsum_batched(x, batch, M, N):
    """x: contiguous [batch*M, N] -> fp32 [batch, N] per-slab column sums."""
    out = torch.empty(batch, N, device=x.device, dtype=torch.float32)
    L.call("uwu_colsum_batched", L.ptr(x), L.dt(x), batch, M, N, N, L.ptr(out), 0, L.stream())
    return out


def im2col3x3(x, B, H, W, C, stride=1):
    Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    col = torch.empty(B * Ho * Wo, 9 * C, device=x.device, dtype=x.dtype)
    L.call("uwu_im2col3x3", L.ptr(x), L.ptr(col), B, H, W, C, stride, L.dt(x), L.stream())
    return col


def col2im3x3(dcol, B, H, W, C, stride=1):
    dx = torch.empty(B * H * W, C, device=dcol.device, dtype=dcol.dtype)
    L.call("uwu_col2im3x3", L.ptr(dcol), L.ptr(dx), B, H, W, C, stride, L.dt(dcol), L.stream())
    return dx


def conv3x3_implicit_ok(x, B, H, W, C, Cout, stride):
    return x.is_cuda and bool(L.load().uwu_conv3x3_implicit_ok(B, H, W, C, Cout, stride, L.dt(x)))


def conv3x3_fwd(x, w, bias, B, H, W, C, Cout, stride=1):
    """Implicit-GEMM 3x3 convolution: x [B*H*W, C] channels-last, w [Cout, 9*C] (tap-major), -> [B*Ho*Wo, Cout]."""
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    y = torch.empty(B * Ho * Wo, Cout, device=x.device, dtype=x.dtype)
    L.call("uwu_conv3x3_fwd", L.ptr(x), L.ptr(w), L.ptr(bias), L.ptr(y), B, H, W, C, Cout, stride, L.dt(x), L.stream())
    return y


def conv3x3_s2br_fwd(x, w, bias, B, H, W, C, Cout):
    """3x3 / stride 2 convolution padded right and bottom only (``F.pad(x, (0, 1, 0, 1))`` + stride 2, padding 0), forward:
    x [B*H*W, C] channels-last, w [Cout, 9*C] (tap-major) -> [B*Ho*Wo, Cout], Ho = (H - 2) // 2 + 1."""
    Ho, Wo = (H - 2) // 2 + 1, (W - 2) // 2 + 1
    y = torch.empty(max(B * Ho * Wo, 0), Cout, device=x.device, dtype=x.dtype)
    need = L.load().uwu_conv3x3_s2br_ws_bytes(B, H, W, C, Cout, L.dt(x))
    ws = shared_scratch(need, x.device) if need else None
    L.call("uwu_conv3x3_s2br_fwd", L.ptr(x), L.ptr(w), L.ptr(bias), L.ptr(y), B, H, W, C, Cout, L.dt(x), L.ptr(ws),
           ws.numel() if ws is not None else 0, L.stream())
    return y


def attention_d512_fwd(q, k, v, B, T, scale=None):
    """One head of width 512, forward only: q / k / v 2-D views [B*T, >= 512] with unit inner stride -> o [B*T, 512]."""
    scale = scale if scale is not None else 512 ** -0.5
    o = torch.empty(B * T, 512, device=q.device, dtype=q.dtype)
    L.call("uwu_attention_d512_fwd", _p(q), _p(k), _p(v), L.ptr(o), B, T, q.stride(0), k.stride(0), v.stride(0), o.stride(0),
           scale, L.dt(q), L.stream())
    return o


def _ids(ids, B, T, what):
    if ids.dtype != torch.int64 or tuple(ids.shape) != (B, T):
        raise L.UwuError(f"{what} must be int64 [B, T] = [{B}, {T}], got {ids.dtype} {tuple(ids.shape)}")
    return L.ptr(ids)


def attention_causal_fwd(q, k, v, B, T, H, d=64, scale=None, key_mask=None):
    """Causal self-attention of the CLIP text transformer, forward only: q / k / v 2-D views [B*T, >= H*d] with unit inner stride
    (column slices of the packed projection) -> o [B*T, H*d].  key_mask: optional int64 [B, T] (attention_mask; row 0 visible)."""
    scale = scale if scale is not None else d ** -0.5
    o = torch.empty(B * T, H * d, device=q.device, dtype=q.dtype)
    L.call("uwu_attention_causal_fwd", _p(q), _p(k), _p(v), None if key_mask is None else _ids(key_mask, B, T, "key_mask"), L.ptr(o),
           B, T, H, d, q.stride(0), k.stride(0), v.stride(0), o.stride(0), scale, L.dt(q), L.stream())
    return o


def text_embed(ids, tok_table, pos_table):
    """tok_table[ids] + pos_table[:T] -> [B*T, D] in the tables' dtype (ids outside the table are clamped)."""
    B, T = ids.shape
    vocab, D = tok_table.shape
    if pos_table.shape[0] < T or pos_table.shape[1] != D or pos_table.dtype != tok_table.dtype:
        raise L.UwuError(f"text_embed: position table {tuple(pos_table.shape)} does not cover T = {T}, D = {D}")
    out = torch.empty(B * T, D, device=tok_table.device, dtype=tok_table.dtype)
    L.call("uwu_text_embed", _ids(ids, B, T, "input_ids"), L.ptr(tok_table), L.ptr(pos_table), L.ptr(out), B, T, D, vocab, L.dt(out),
           L.stream())
    return out


def bias_act_fwd(x, kind, bias=None, out=None, N=None):
    """act(x + bias) over the first N columns of the rows of x [M, >= N]; kind "quick_gelu" | "gelu" (erf); out=x runs in place."""
    M = x.shape[0]
    N = N if N is not None else x.shape[1]
    y = out if out is not None else torch.empty_like(x)
    if y.stride(0) != x.stride(0) or y.dtype != x.dtype:
        raise L.UwuError("bias_act_fwd: out must have the dtype and row stride of x")
    L.call("uwu_bias_act_fwd", _p(x), L.ptr(bias), _p(y), M, N, x.stride(0), L.ACT[kind], L.dt(x), L.stream())
    return y


def text_pool(ids, h, eos_id):
    """h [B*T, D] -> [B, D]: the row at the eos position of each sequence (uwu_text_pool's two rules), found on the device."""
    B, T = ids.shape
    D = h.shape[1]
    pooled = torch.empty(B, D, device=h.device, dtype=h.dtype)
    L.call("uwu_text_pool", _ids(ids, B, T, "input_ids"), L.ptr(h), L.ptr(pooled), B, T, D, int(eos_id), L.dt(h), L.stream())
    return pooled


def attention_relbias_fwd(q, k, v, rel_bias, B, T, H, d=64, scale=1.0, key_mask=None):
    """Bidirectional self-attention of the T5 encoder, forward only: q / k / v 2-D views [B*T, >= H*d] with unit inner stride (column
    slices of the packed projection), rel_bias fp32 [H, 2T - 1] indexed by key - query + T - 1 -> o [B*T, H*d].  key_mask: optional
    int64 [B, T] (attention_mask; at least one visible key per sequence)."""
    if rel_bias.dtype != torch.float32 or tuple(rel_bias.shape) != (H, 2 * T - 1):
        raise L.UwuError(f"rel_bias must be fp32 [H, 2T - 1] = [{H}, {2 * T - 1}], got {rel_bias.dtype} {tuple(rel_bias.shape)}")
    o = torch.empty(B * T, H * d, device=q.device, dtype=q.dtype)
    L.call("uwu_attention_relbias_fwd", _p(q), _p(k), _p(v), L.ptr(rel_bias), None if key_mask is None else _ids(key_mask, B, T, "key_mask"),
           L.ptr(o), B, T, H, d, q.stride(0), k.stride(0), v.stride(0), o.stride(0), scale, L.dt(q), L.stream())
    return o


def attention_bidir_fwd(q, k, v, B, T, H, d=64, scale=None, key_mask=None):
    """Bidirectional self-attention without a bias (the CLIP image tower), forward only: q / k / v 2-D views [B*T, >= H*d] with unit
    inner stride (column slices of the packed projection) -> o [B*T, H*d].  d = 64, T <= 1024.  key_mask: optional int64 [B, T]."""
    scale = scale if scale is not None else d ** -0.5
    o = torch.empty(B * T, H * d, device=q.device, dtype=q.dtype)
    L.call("uwu_attention_bidir_fwd", _p(q), _p(k), _p(v), None if key_mask is None else _ids(key_mask, B, T, "key_mask"), L.ptr(o),
           B, T, H, d, q.stride(0), k.stride(0), v.stride(0), o.stride(0), scale, L.dt(q), L.stream())
    return o


def clip_patches(images, patch, dtype, ld=None, mean=None, std=None):
    """images [B, 3, S, S] (fp32, or uint8 with mean / std) -> [B * (S/patch)^2, ld] in `dtype`: the A operand of the patch-embedding
    GEMM, columns (c, i, j), zeros from 3 patch^2 up to ld (default: the next multiple of 8).  With mean / std (three numbers each)
    the images are [0, 255] and CLIP's preprocessing is fused in; without, they are copied as they are."""
    if images.dim() != 4 or images.shape[1] != 3 or images.shape[2] != images.shape[3]:
        raise L.UwuError(f"clip_patches: images must be [B, 3, S, S], got {tuple(images.shape)}")
    if images.dtype not in (torch.float32, torch.uint8) or (mean is None) != (std is None):
        raise L.UwuError(f"clip_patches: fp32 or uint8 images and mean / std together, got {images.dtype}")
    B, _, S, _ = images.shape
    if S % patch:
        raise L.UwuError(f"clip_patches: image size {S} is not a multiple of the patch size {patch}")
    K = 3 * patch * patch
    ld = ld if ld is not None else (K + 7) // 8 * 8
    out = torch.empty(B * (S // patch) ** 2, ld, device=images.device, dtype=dtype)
    F3 = ctypes.c_float * 3
    m, s = (F3(*mean), F3(*std)) if mean is not None else (None, None)
    L.call("uwu_clip_patches", L.ptr(images), int(images.dtype == torch.uint8), L.ptr(out), B, S, patch, ld, int(mean is not None), m, s,
           L.dt(out), L.stream())
    return out


def vit_embed(patch_out, class_embedding, pos_table, B):
    """patch_out [B*Np, D], class_embedding [D], pos_table [Np + 1, D] -> [B * (Np + 1), D]: the class token first, positions added."""
    M, D = patch_out.shape
    T = pos_table.shape[0]
    if M != B * (T - 1) or tuple(class_embedding.shape) != (D,) or pos_table.shape[1] != D or not (
            patch_out.dtype == class_embedding.dtype == pos_table.dtype):
        raise L.UwuError(f"vit_embed: patch_out {tuple(patch_out.shape)}, class_embedding {tuple(class_embedding.shape)} and pos_table "
                         f"{tuple(pos_table.shape)} do not fit B = {B}")
    out = torch.empty(B * T, D, device=patch_out.device, dtype=patch_out.dtype)
    L.call("uwu_vit_embed", L.ptr(patch_out), L.ptr(class_embedding), L.ptr(pos_table), L.ptr(out), B, T, D, L.dt(out), L.stream())
    return out


def clip_score_accum(image_embeds, text_embeds, acc):
    """-> scores fp32 [B] = 100 cos(image_b, text_b); acc (float64 [2] on the device) += (their sum, B), in a fixed order."""
    if image_embeds.dim() != 2 or image_embeds.shape != text_embeds.shape or image_embeds.dtype != text_embeds.dtype:
        raise L.UwuError(f"clip_score_accum: embeddings must be two [B, P] tensors of one dtype, got {tuple(image_embeds.shape)} "
                         f"{image_embeds.dtype} and {tuple(text_embeds.shape)} {text_embeds.dtype}")
    if acc.dtype != torch.float64 or acc.numel() != 2:
        raise L.UwuError("clip_score_accum: acc must be float64 [2]")
    B, P = image_embeds.shape
    scores = torch.empty(B, device=image_embeds.device, dtype=torch.float32)
    L.call("uwu_clip_score_accum", L.ptr(image_embeds), L.ptr(text_embeds), L.ptr(scores), L.ptr(acc), B, P, L.dt(image_embeds), L.stream())
    return scores


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


def conv2d_out_hw(H, W, kernel, stride=1, padding=0):
    (KH, KW), (ph, pw) = _pair(kernel), _pair(padding)
    return (H + 2 * ph - KH) // stride + 1, (W + 2 * pw - KW) // stride + 1


def conv2d_ok(B, H, W, C, Cout, kernel, stride=1, padding=0, ldx=None, xoff=0, ldy=None, yoff=0, dtype=torch.bfloat16):
    """True where ``conv2d_fwd`` runs the shape, False where it refuses it: the entry point's own predicate, asked on the host"""
    (KH, KW), (ph, pw) = _pair(kernel), _pair(padding)
    dt = {torch.float32: L.F32, torch.bfloat16: L.BF16}.get(dtype, -1)
    return bool(L.load().uwu_conv2d_ok(B, H, W, C, Cout, KH, KW, stride, ph, pw, C if ldx is None else ldx, xoff,
                                       Cout if ldy is None else ldy, yoff, dt))


def conv2d_fwd(x, w, bias, B, H, W, C, Cout, kernel, stride=1, padding=0, relu=False, xoff=0, out=None, yoff=0):
    """y = [relu](conv(x, w) + bias) on channels-last activations: x [B*H*W, ldx] of which channels xoff .. xoff + C are read, w
    [Cout, KH*KW*C] (tap-major), bias fp32 [Cout] or None -> out [B*Ho*Wo, ldy] of which channels yoff .. yoff + Cout are written (a
    new [B*Ho*Wo, Cout] without `out`)."""
    (KH, KW), (ph, pw) = _pair(kernel), _pair(padding)
    Ho, Wo = conv2d_out_hw(H, W, (KH, KW), stride, (ph, pw))
    if out is None:
        out = torch.empty(max(B * Ho * Wo, 0), Cout, device=x.device, dtype=x.dtype)
    if (x.dim() != 2 or out.dim() != 2 or x.shape[0] != B * H * W or out.shape[0] != B * Ho * Wo or out.dtype != x.dtype or w.dtype != x.dtype
            or w.numel() != Cout * KH * KW * C or (bias is not None and (bias.dtype != torch.float32 or bias.numel() != Cout))):
        raise L.UwuError(f"conv2d_fwd: x {tuple(x.shape)} {x.dtype}, w {tuple(w.shape)} {w.dtype}, out {tuple(out.shape)} {out.dtype} do not "
                         f"fit B = {B}, H = {H}, W = {W}, C = {C}, Cout = {Cout}, kernel {KH} x {KW}, stride {stride}, padding ({ph}, {pw})")
    L.call("uwu_conv2d_fwd", L.ptr(x), L.ptr(w), L.ptr(bias), L.ptr(out), B, H, W, C, Cout, KH, KW, stride, ph, pw, x.shape[1], xoff,
           out.shape[1], yoff, int(relu), L.dt(x), None, 0, L.stream())
    return out


def conv1x1_gemm_fwd(x, w, bias, C, Cout, relu=False, xoff=0, out=None, yoff=0):
    """The same result as a 1x1 / stride 1 ``conv2d_fwd`` by the explicit route, whose column matrix is the activation itself:
    ``uwu_gemm`` with the bias epilogue on channels xoff.. of x [M, ldx] into channels yoff.. of out [M, ldy], then ``uwu_relu_rows``
    in place (uwu_gemm has no ReLU epilogue)."""
    M = x.shape[0]
    if out is None:
        out = torch.empty(M, Cout, device=x.device, dtype=x.dtype)
    if (x.dim() != 2 or out.dim() != 2 or out.shape[0] != M or out.dtype != x.dtype or w.dtype != x.dtype or tuple(w.shape) != (Cout, C)
            or bias.dtype != torch.float32 or bias.numel() != Cout or xoff % 8 or yoff % 8 or xoff < 0 or yoff < 0
            or xoff + C > x.shape[1] or yoff + Cout > out.shape[1]):
        raise L.UwuError(f"conv1x1_gemm_fwd: x {tuple(x.shape)} (offset {xoff}), w {tuple(w.shape)}, out {tuple(out.shape)} (offset {yoff}) "
                         f"do not fit C = {C}, Cout = {Cout} (offsets multiples of 8, slices inside their rows)")
    es = x.element_size()
    L.call("uwu_gemm", L.ptr(x) + xoff * es, L.ptr(w), L.ptr(out) + yoff * es, None, L.ptr(bias), None, M, Cout, C, x.shape[1], C,
           out.shape[1], 0, 0, 0, L.dt(x), L.dt(out), L.EPI_BIAS, 1, L.stream())
    if relu:
        L.call("uwu_relu_rows", L.ptr(out), M, Cout, out.shape[1], yoff, L.dt(out), L.stream())
    return out


def inception_stem(images, dtype):
    """pictures [B, 3, H, W], uint8 or fp32 in [0, 1] -> the operand [B*Ho*Wo, 32] of the first convolution (3x3, stride 2) in `dtype`,
    ``(v - 128) / 128`` of the integer pixel value v fused in (a float is first turned into ``trunc(clamp(x, 0, 1) * 255)``)"""
    if images.dim() != 4 or images.shape[1] != 3 or images.dtype not in (torch.uint8, torch.float32):
        raise L.UwuError(f"inception_stem: images must be uint8 or fp32 [B, 3, H, W], got {images.dtype} {tuple(images.shape)}")
    B, _, H, W = images.shape
    out = torch.empty(B * ((H - 3) // 2 + 1) * ((W - 3) // 2 + 1), 32, device=images.device, dtype=dtype)
    L.call("uwu_inception_stem", L.ptr(images), int(images.dtype == torch.uint8), L.ptr(out), B, H, W, L.dt(out), L.stream())
    return out


POOL = {"max_s2": 0, "max_s1p1": 1, "avg_s1p1": 2}  # UWU_POOL_*


def pool2d_fwd(x, B, H, W, C, mode, xoff=0, out=None, yoff=0):
    """3x3 pooling on channels-last rows: "max_s2" (stride 2, no padding), "max_s1p1", "avg_s1p1" (count_include_pad=False);
    channels xoff .. xoff + C of x [B*H*W, ldx] -> channels yoff .. yoff + C of out [B*Ho*Wo, ldy]"""
    Ho, Wo = ((H - 3) // 2 + 1, (W - 3) // 2 + 1) if mode == "max_s2" else (H, W)
    if out is None:
        out = torch.empty(max(B * Ho * Wo, 0), C, device=x.device, dtype=x.dtype)
    if x.dim() != 2 or out.dim() != 2 or x.shape[0] != B * H * W or out.shape[0] != B * Ho * Wo or out.dtype != x.dtype:
        raise L.UwuError(f"pool2d_fwd: x {tuple(x.shape)} and out {tuple(out.shape)} do not fit B = {B}, H = {H}, W = {W} ({mode})")
    L.call("uwu_pool2d_fwd", L.ptr(x), L.ptr(out), B, H, W, C, POOL[mode], x.shape[1], xoff, out.shape[1], yoff, L.dt(x), L.stream())
    return out


def global_avgpool(x, B, HW, C):
    """x [B*HW, C] -> fp32 [B, C], the mean over each picture's pixels"""
    if x.dim() != 2 or tuple(x.shape) != (B * HW, C):
        raise L.UwuError(f"global_avgpool: x {tuple(x.shape)} is not [{B} * {HW}, {C}]")
    out = torch.empty(B, C, device=x.device, dtype=torch.float32)
    L.call("uwu_global_avgpool", L.ptr(x), L.ptr(out), B, HW, C, x.shape[1], L.dt(x), L.stream())
    return out


def fid_stats_accum(features, acc):
    """acc (float64 [1 + D + D*D] on the device: n, sum, outer) += the statistics of features fp32 [B, D], in a fixed order"""
    if features.dim() != 2 or features.dtype != torch.float32:
        raise L.UwuError(f"fid_stats_accum: features must be fp32 [B, D], got {features.dtype} {tuple(features.shape)}")
    B, D = features.shape
    if acc.dtype != torch.float64 or acc.numel() != 1 + D + D * D:
        raise L.UwuError(f"fid_stats_accum: acc must be float64 [{1 + D + D * D}]")
    L.call("uwu_fid_stats_accum", L.ptr(features), L.ptr(acc), B, D, L.stream())


def add_rmsnorm_fwd(x_in, weight, eps, y=None):
    """(x_in + y, RMSNorm(x_in + y) * weight) on [M, D]; without y the first is x_in itself.  weight fp32 [D]."""
    M, D = x_in.shape
    if weight.dtype != torch.float32 or tuple(weight.shape) != (D,) or (y is not None and (y.shape != x_in.shape or y.dtype != x_in.dtype)):
        raise L.UwuError(f"add_rmsnorm_fwd: weight must be fp32 [{D}] and y like x_in")
    x_out = torch.empty_like(x_in) if y is not None else x_in
    n = torch.empty_like(x_in)
    L.call("uwu_add_rmsnorm_fwd", L.ptr(x_in), L.ptr(y), L.ptr(weight), L.ptr(x_out) if y is not None else None, L.ptr(n), M, D, eps,
           L.dt(x_in), L.stream())
    return x_out, n


def gated_act_fwd(u, kind="gated-gelu"):
    """u [M, 2F] (the GEMM on wi_0 | wi_1) -> act(u[:, :F]) * u[:, F:] as [M, F]; kind "gated-gelu" (tanh GELU)."""
    M, F2 = u.shape
    if F2 % 2:
        raise L.UwuError(f"gated_act_fwd: u must be [M, 2F], got {tuple(u.shape)}")
    out = torch.empty(M, F2 // 2, device=u.device, dtype=u.dtype)
    L.call("uwu_gated_act_fwd", _p(u), L.ptr(out), M, F2 // 2, u.stride(0), out.stride(0), L.GATE[kind], L.dt(u), L.stream())
    return out


def t5_rel_bias(weight, bucket):
    """weight fp32 [num_buckets, H], bucket int32 [2T - 1] -> fp32 [H, 2T - 1] with out[h, o] = weight[bucket[o], h]."""
    nb, H = weight.shape
    if weight.dtype != torch.float32 or bucket.dtype != torch.int32 or bucket.dim() != 1:
        raise L.UwuError("t5_rel_bias: weight must be fp32 [num_buckets, H] and bucket int32 [2T - 1]")
    out = torch.empty(H, bucket.numel(), device=weight.device, dtype=torch.float32)
    L.call("uwu_t5_rel_bias", L.ptr(weight), L.ptr(bucket), L.ptr(out), nb, H, bucket.numel(), L.stream())
    return out


def token_embed(ids, tok_table):
    """tok_table[ids] -> [B*T, D] in the table's dtype (ids outside the table are clamped)."""
    B, T = ids.shape
    vocab, D = tok_table.shape
    out = torch.empty(B * T, D, device=tok_table.device, dtype=tok_table.dtype)
    L.call("uwu_token_embed", _ids(ids, B, T, "input_ids"), L.ptr(tok_table), L.ptr(out), B, T, D, vocab, L.dt(out), L.stream())
    return out


def posterior_draw(moments, B, latent, HW, seed=0, offset=0, *, sample=True, mean=False, logvar=False):
    """AutoencoderKL posterior from channels-last fp32 moments [B*HW, >= 2*latent]: (z, mean, logvar), each fp32 [B, latent, HW] or
    None; z = mean + exp(0.5 clamp(logvar, -30, 20)) * uwu_philox_normal(n, seed, offset)."""
    if moments.dtype != torch.float32:
        raise L.UwuError(f"posterior_draw: moments must be fp32, got {moments.dtype}")
    new = lambda on: torch.empty(B, latent, HW, device=moments.device, dtype=torch.float32) if on else None
    z, mu, lv = new(sample), new(mean), new(logvar)
    L.call("uwu_posterior_draw", L.ptr(moments), moments.stride(0), B, latent, HW, L.ptr(z), L.ptr(mu), L.ptr(lv), seed, offset,
           L.stream())
    return z, mu, lv


def conv3x3_dgrad(dy, w, B, H, W, C, Cout, stride=1):
    dx = torch.empty(B * H * W, C, device=dy.device, dtype=dy.dtype)
    L.call("uwu_conv3x3_dgrad", L.ptr(dy), L.ptr(w), L.ptr(dx), B, H, W, C, Cout, stride, L.dt(dy), L.stream())
    return dx


def conv3x3_wgrad(dy, x, dw, db, B, H, W, C, Cout, stride=1):
    """dw [Cout, 9*C] fp32 += , db [Cout] fp32 += (views of the flat gradient buffer)."""
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    need = L.load().uwu_conv3x3_wgrad_scratch_bytes(C, Cout, B * Ho * Wo)
    sc = shared_scratch(need, dy.device)
    L.call("uwu_conv3x3_wgrad", L.ptr(dy), L.ptr(x), L.ptr(dw), L.ptr(db), B, H, W, C, Cout, stride, L.dt(dy), L.ptr(sc),
           sc.numel(), L.stream())


def groupnorm_fwd(x, gamma, beta, B, HW, C, G, eps, silu):
    y = torch.empty_like(x)
    mean = torch.empty(B * G, device=x.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    L.call("uwu_groupnorm_fwd", L.ptr(x), _p(gamma), _p(beta), L.ptr(y), L.ptr(mean), L.ptr(rstd), B, HW, C, G,
           float(eps), int(silu), L.dt(x), L.stream())
    return y, mean, rstd


def groupnorm_fwd_det(x, gamma, beta, B, HW, C, G, eps, silu):
    """groupnorm_fwd with a fixed summation order (no float atomics): bit-identical between launches and batch sizes."""
    y = torch.empty_like(x)
    mean = torch.empty(B * G, device=x.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    need = L.load().uwu_groupnorm_fwd_det_ws_bytes(B, HW, C, G)
    ws = torch.empty(max(need, 4), device=x.device, dtype=torch.uint8)
    L.call("uwu_groupnorm_fwd_det", L.ptr(x), _p(gamma), _p(beta), L.ptr(y), L.ptr(mean), L.ptr(rstd), L.ptr(ws), ws.numel(), B, HW, C,
           G, float(eps), int(silu), L.dt(x), L.stream())
    return y, mean, rstd


def groupnorm_bwd(dy, x, mean, rstd, gamma, beta, dgamma, dbeta, B, HW, C, G, silu):
    dx = torch.empty_like(x)
    ws = torch.empty(2 * B * G, device=x.device, dtype=torch.float32)
    L.call("uwu_groupnorm_bwd", L.ptr(dy), L.ptr(x), L.ptr(mean), L.ptr(rstd), _p(gamma), _p(beta), L.ptr(dx),
           _p(dgamma), _p(dbeta), L.ptr(ws), B, HW, C, G, int(silu), L.dt(x), L.stream())
    return dx


def geglu_fwd(hg):
    M, F2 = hg.shape
    out = torch.empty(M, F2 // 2, device=hg.device, dtype=hg.dtype)
    L.call("uwu_geglu_fwd", L.ptr(hg), L.ptr(out), M, F2 // 2, L.dt(hg), L.stream())
    return out


def geglu_bwd(hg, dout):
    dhg = torch.empty_like(hg)
    L.call("uwu_geglu_bwd", L.ptr(hg), L.ptr(dout), L.ptr(dhg), hg.shape[0], hg.shape[1] // 2, L.dt(hg), L.stream())
    return dhg


def silu_fwd(x):
    y = torch.empty_like(x)
    L.call("uwu_silu_fwd", L.ptr(x), L.ptr(y), x.numel(), L.dt(x), L.stream())
    return y


def silu_bwd(x, dy):
    dx = torch.empty_like(x)
    L.call("uwu_silu_bwd", L.ptr(x), L.ptr(dy), L.ptr(dx), x.numel(), L.dt(x), L.stream())
    return dx


def add(a, b):
    out = torch.empty_like(a)
    L.call("uwu_add", L.ptr(a.contiguous()), L.ptr(b.contiguous()), L.ptr(out), a.numel(), L.dt(a), L.stream())
    return out


def add_rowvec(x, v, B, HW, C):
    out = x.clone()
    L.call("uwu_add_rowvec", L.ptr(out), L.ptr(v.contiguous()), B, HW, C, L.dt(x), L.stream())
    return out


def upsample2x(x, B, H, W, C, backward=False):
    n = B * H * W if backward else B * 4 * H * W
    out = torch.empty(n, C, device=x.device, dtype=x.dtype)
    L.call("uwu_upsample2x", L.ptr(x), L.ptr(out), B, H, W, C, int(backward), L.dt(x), L.stream())
    return out


def nchw_to_cl(x, dtype):
    B, C, H, W = x.shape
    out = torch.empty(B * H * W, C, device=x.device, dtype=dtype)
    L.call("uwu_nchw_to_cl", L.ptr(x), L.ptr(out), B, C, H * W, L.dt(out), L.stream())
    return out


def cl_to_nchw(x, B, C, HW):
    out = torch.empty(B, C, HW, device=x.device, dtype=torch.float32)
    L.call("uwu_cl_to_nchw", L.ptr(x), L.ptr(out), B, C, HW, L.dt(x), L.stream())
    return out


def gemm_wgrad(dy, x, dw, blocks=512, scratch=None, bias_grad=None):
    """dw[M,N] (fp32) += dy[K,M]^T @ x[K,N] -- weight gradient of a Linear; ``scratch`` (a byte tensor from
    :func:`gemm_wgrad_scratch`) switches the split-K reduction from fp32 atomics to slices + a reduce kernel;
    ``bias_grad`` (fp32[M]) += column sums of dy."""
    K, M = dy.shape
    K2, N = x.shape
    assert K == K2 and dw.shape == (M, N) and dw.dtype == torch.float32 and dy.dtype == x.dtype
    L.call("uwu_gemm_wgrad", L.ptr(dy), L.ptr(x), L.ptr(dw), L.ptr(bias_grad), M, N, K, dy.stride(0), x.stride(0), dw.stride(0), L.dt(dy),
           blocks, L.ptr(scratch), scratch.numel() if scratch is not None else 0, L.stream())
    return dw


def gemm_wgrad_pair(dy_a, x_a, dw_a, dy_b, x_b, dw_b, blocks=512, scratch=None, bias_grad_a=None, bias_grad_b=None):
    """Two weight gradients over the same tokens, dw_a += dy_a^T @ x_a and dw_b += dy_b^T @ x_b, as one launch of the wide
    streaming kernel when ``scratch`` (:func:`gemm_wgrad_pair_scratch`) allows it, else as two :func:`gemm_wgrad` calls."""
    K = dy_a.shape[0]
    args = []
    for dy, x, dw, db in ((dy_a, x_a, dw_a, bias_grad_a), (dy_b, x_b, dw_b, bias_grad_b)):
        assert dy.shape[0] == K and x.shape[0] == K and dw.shape == (dy.shape[1], x.shape[1])
        assert dw.dtype == torch.float32 and dy.dtype == x.dtype == dy_a.dtype
        args += [L.ptr(dy), L.ptr(x), L.ptr(dw), L.ptr(db), dy.shape[1], x.shape[1], dy.stride(0), x.stride(0), dw.stride(0)]
    L.call("uwu_gemm_wgrad_pair", *args, K, L.dt(dy_a), blocks, L.ptr(scratch), scratch.numel() if scratch is not None else 0,
           L.stream())
    return dw_a, dw_b


def gemm_wgrad_pair_scratch(Ma, Na, Mb, Nb, K, device="cuda"):
    """Scratch for :func:`gemm_wgrad_pair`: the grouped launch's, or the larger member's when the pair is not grouped."""
    lib = L.load()
    need = max(lib.uwu_gemm_wgrad_pair_scratch_bytes(Ma, Na, Mb, Nb, K), lib.uwu_gemm_wgrad_scratch_bytes(Ma, Na, K),
               lib.uwu_gemm_wgrad_scratch_bytes(Mb, Nb, K))
    return torch.empty(need, dtype=torch.uint8, device=device)


def gemm_wgrad_scratch(M, N, K, device="cuda"):
    return torch.empty(L.load().uwu_gemm_wgrad_scratch_bytes(M, N, K), dtype=torch.uint8, device=device)


_shared = {}


def shared_scratch(nbytes, device):
    """One growing split-K scratch per device, shared by every weight gradient of a Python-composed graph (launches on
    one stream are ordered, and a weight gradient's reduce kernel has consumed the scratch before the next one starts)."""
    sc = _shared.get(device)
    if sc is None or sc.numel() < nbytes:
        sc = _shared[device] = torch.empty(max(nbytes, 1 << 20), device=device, dtype=torch.uint8)
    return sc


def gemm_wgrad_shared(dy, x, dw, blocks=512, bias_grad=None):
    """gemm_wgrad with the per-device shared scratch: split-K slices + reduce instead of fp32 atomics (50 tiles x 8 slices
    of a 1280 x 1280 weight gradient are 52 MB of atomics at ~1.3 TB/s chip-wide -- as long as the K loop itself)."""
    K, M = dy.shape
    N = x.shape[1]
    need = L.load().uwu_gemm_wgrad_scratch_bytes(M, N, K)
    return gemm_wgrad(dy, x, dw, blocks=blocks, scratch=shared_scratch(need, dy.device) if need else None, bias_grad=bias_grad)


# ---------------------------------------------------------------------------------------------------- fp8 (config 5)
FP8_E4M3, FP8_E5M2 = 0, 1
FP8_MAX = {FP8_E4M3: 448.0, FP8_E5M2: 57344.0}


def fp8_amax(x, amax=None):
    if amax is None:
        amax = torch.zeros(1, device=x.device, dtype=torch.float32)
    L.call("uwu_fp8_amax", L.ptr(x), L.dt(x), x.numel(), L.ptr(amax), L.stream())
    return amax


def fp8_update_scales(amax, scale, fmt, margin=1.0):
    """amax / scale: fp32 [n]; fmt: int32 [n] (FP8_E4M3 / FP8_E5M2).  scale = FMT_MAX / (amax * margin); amax <- 0."""
    L.call("uwu_fp8_update_scales", L.ptr(amax), L.ptr(scale), L.ptr(fmt), amax.numel(), float(margin), L.stream())
    return scale


def fp8_quantize(x, scale, fmt=FP8_E4M3, *, rowmajor=True, transposed=False, amax=None, colsum=None):
    """x [M,K] (bf16 / fp32) -> (uint8 [M,K] | None, uint8 [K,M] | None) in one pass over x."""
    M, K = x.shape
    out = torch.empty(M, K, device=x.device, dtype=torch.uint8) if rowmajor else None
    out_t = torch.empty(K, M, device=x.device, dtype=torch.uint8) if transposed else None
    L.call("uwu_fp8_quantize", L.ptr(x), L.dt(x), M, K, x.stride(0), L.ptr(scale), fmt, L.ptr(out), K, L.ptr(out_t), M,
           L.ptr(amax), L.ptr(colsum), L.stream())
    return out, out_t


def gemm_fp8(a8, b8, scale_a, scale_b, *, fmt_a=FP8_E4M3, bias=None, aux=None, epilogue=L.EPI_NONE, out=None, out2=None):
    """C[M,N] = (a8[M,K] . b8[N,K]^T) / (scale_a * scale_b): both operands uint8 fp8 bytes, contraction-contiguous."""
    M, K = a8.shape
    N, Kb = b8.shape
    assert K == Kb and a8.dtype == torch.uint8 and b8.dtype == torch.uint8
    scratch, sbytes = None, 0
    if epilogue == L.EPI_ACCUM:
        if out is None:
            out = torch.zeros(M, N, device=a8.device, dtype=torch.float32)
        sbytes = L.load().uwu_gemm_fp8_scratch_bytes(M, N, K)
        scratch = torch.empty(sbytes, device=a8.device, dtype=torch.uint8)
    elif out is None:
        out = torch.empty(M, N, device=a8.device, dtype=torch.bfloat16)
    if epilogue == L.EPI_BIAS_GELU and out2 is None:
        out2 = torch.empty(M, N, device=a8.device, dtype=torch.bfloat16)
    L.call("uwu_gemm_fp8", L.ptr(a8), L.ptr(b8), L.ptr(out), L.ptr(out2), L.ptr(bias), L.ptr(aux), M, N, K, a8.stride(0),
           b8.stride(0), out.stride(0), aux.stride(0) if aux is not None else 0, fmt_a, epilogue, L.ptr(scale_a),
           L.ptr(scale_b), L.ptr(scratch), sbytes, L.stream())
    return (out, out2) if out2 is not None and epilogue == L.EPI_BIAS_GELU else out


def gemm_fp8_emit(a8, b8, scale_a, scale_b, q_scale, *, epilogue, fmt_a=FP8_E4M3, bias=None, aux=None, colsum=None, amax=None,
                  rowmajor=True, transposed=True):
    """The fp8 GEMM whose epilogue leaves its result as the fp8 operand of the next GEMMs (no quantising pass):
    EPI_BIAS_GELU -> (bf16 pre-activation, e4m3 gelu [M,N], its transpose [N,M]); EPI_DGELU -> (None, e5m2 [M,N], [N,M])."""
    M, K = a8.shape
    N = b8.shape[0]
    assert a8.dtype == torch.uint8 and b8.dtype == torch.uint8 and b8.shape[1] == K
    C = torch.empty(M, N, device=a8.device, dtype=torch.bfloat16) if epilogue == L.EPI_BIAS_GELU else None
    q8 = torch.empty(M, N, device=a8.device, dtype=torch.uint8) if rowmajor else None
    q8t = torch.empty(N, M, device=a8.device, dtype=torch.uint8) if transposed else None
    L.call("uwu_gemm_fp8_emit", L.ptr(a8), L.ptr(b8), L.ptr(C), L.ptr(colsum), L.ptr(bias), L.ptr(aux), M, N, K, a8.stride(0),
           b8.stride(0), N, aux.stride(0) if aux is not None else 0, fmt_a, epilogue, L.ptr(scale_a), L.ptr(scale_b), L.ptr(q8), N,
           L.ptr(q8t), M, L.ptr(q_scale), L.ptr(amax), L.stream())
    return C, q8, q8t


# ---------------------------------------------------------------------------------------------------- RoPE in attention
def axial_rope_table(pos, fh, fw, H, d):
    """Factor table m [T, H*d] (fp32) of the reference's axial RoPE for shared positions pos [T, 2]."""
    T = pos.shape[0]
    tab = torch.empty(T, H * d, device=pos.device, dtype=torch.float32)
    L.call("uwu_axial_rope_table", L.ptr(pos), L.ptr(fh), L.ptr(fw), L.ptr(tab), T, H, d, H * d, L.stream())
    return tab


class _RopeAttentionFn(torch.autograd.Function):
    """o = SDPA(rope(q), rope(k), v) with the rotation applied inside the attention kernels' q / k staging."""

    @staticmethod
    def forward(ctx, qkv, pos, fh, fw, B, T, H, d):
        D = H * d
        tab = axial_rope_table(pos, fh, fw, H, d)
        o = torch.empty(B * T, D, device=qkv.device, dtype=qkv.dtype)
        lse = torch.empty(B, H, T, device=qkv.device, dtype=torch.float32)
        q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
        L.call("uwu_attention_rope_fwd", _p(q), _p(k), _p(v), L.ptr(tab), L.ptr(o), L.ptr(lse), B, T, H, d, qkv.stride(0),
               qkv.stride(0), qkv.stride(0), D, D, d ** -0.5, L.dt(qkv), L.stream())
        ctx.save_for_backward(qkv, pos, fh, fw, tab, o, lse)
        ctx.meta = (B, T, H, d)
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, pos, fh, fw, tab, o, lse = ctx.saved_tensors
        B, T, H, d = ctx.meta
        D = H * d
        do = do.contiguous()
        dqkv = torch.empty_like(qkv)
        q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
        dq, dk, dv = dqkv[:, :D], dqkv[:, D:2 * D], dqkv[:, 2 * D:]
        L.call("uwu_attention_rope_bwd", _p(q), _p(k), _p(v), L.ptr(tab), L.ptr(o), L.ptr(do), L.ptr(lse), _p(dq), _p(dk),
               _p(dv), B, T, H, d, qkv.stride(0), qkv.stride(0), qkv.stride(0), D, D, d ** -0.5, L.dt(qkv), L.stream())
        # dq', dk' (wrt the rotated operands) -> dq, dk in place, log-frequency gradients accumulated
        dfh, dfw = torch.zeros_like(fh), torch.zeros_like(fw)
        for x, dx in ((q, dq), (k, dk)):
            L.call("uwu_axial_rope_bwd_shared", _p(x), _p(dx), L.ptr(pos), T, L.ptr(fh), L.ptr(fw), _p(dx), L.ptr(dfh),
                   L.ptr(dfw), B * T, H, d, qkv.stride(0), L.dt(qkv), L.stream())
        return dqkv, None, dfh, dfw, None, None, None, None


def rope_attention(qkv, pos, fh, fw, B, T, H, d):
    """qkv: packed projection [B*T, 3*H*d] (bf16); pos [T, 2] fp32 (shared by the batch); fh / fw [H, d/4] log-frequencies."""
    return _RopeAttentionFn.apply(qkv, pos, fh, fw, B, T, H, d)


# ------------------------------------------------------------------------- fp32 Linears with <= 64 rows (conditioning path)
def skinny_linear_ok(M, N, K):
    return bool(L.load().uwu_skinny_linear_ok(M, N, K))


def skinny_linear_fwd(x, w, bias=None, epilogue=None):
    """y = x w^T (+ bias); with epilogue L.EPI_BIAS_SILU returns (y, silu(y)).  fp32, x [M <= 64, K], w [N, K]."""
    M, K = x.shape
    N = w.shape[0]
    epi = epilogue if epilogue is not None else (L.EPI_BIAS if bias is not None else L.EPI_NONE)
    y = torch.empty(M, N, device=x.device, dtype=torch.float32)
    y2 = torch.empty_like(y) if epi == L.EPI_BIAS_SILU else None
    L.call("uwu_skinny_linear_fwd", L.ptr(x), L.ptr(w), L.ptr(bias), L.ptr(y), L.ptr(y2), M, N, K, epi, L.stream())
    return (y, y2) if y2 is not None else y


def skinny_linear_dgrad(dy, w):
    M, N = dy.shape
    K = w.shape[1]
    dx = torch.empty(M, K, device=dy.device, dtype=torch.float32)
    L.call("uwu_skinny_linear_dgrad", L.ptr(dy), L.ptr(w), L.ptr(dx), M, N, K, L.stream())
    return dx


def skinny_linear_wgrad(dy, x, dw, db=None):
    M, N = dy.shape
    K = x.shape[1]
    L.call("uwu_skinny_linear_wgrad", L.ptr(dy), L.ptr(x), L.ptr(dw), L.ptr(db), M, N, K, L.stream())
    return dw
