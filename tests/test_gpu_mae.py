"""MAE pre-training on the GPU: the three new kernels against torch / the f64 reference of
tests/mae_cases.py, attention at the encoder's 7 tokens, the model's loss and gradients (fp32 against
f64, bf16 against the fp32 HIP run), repeatability, the encoder checkpoint round trip and the
pretrain_mae.py entry point. Small shapes: each test takes seconds."""
import math

import pytest
import torch

import mae_cases as MC

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rel2(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


# ------------------------------------------------------------------------------ ivit_token_select
def _select_ref(src, idx, fill, add):
    """torch index_select of the in-range rows, fill / zeros elsewhere, plus one f32 add."""
    B, Ns, D = src.shape
    ok = (idx >= 0) & (idx < Ns)
    rows = torch.stack([src[b].index_select(0, idx[b].clamp(0, Ns - 1).long()) for b in range(B)])
    other = fill.reshape(1, 1, D).expand_as(rows) if fill is not None else torch.zeros_like(rows)
    out = torch.where(ok.unsqueeze(-1), rows, other)
    return out + add.unsqueeze(0) if add is not None else out


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("with_fill", [False, True])
@pytest.mark.parametrize("Nd", MC.SELECT_ND)
@pytest.mark.parametrize("D", MC.D_CASES)
def test_token_select_is_index_select_bitwise(D, Nd, with_fill, with_add):
    import ops
    B, Ns = MC.SELECT_B, Nd + 4
    g = torch.Generator().manual_seed(D + Nd)
    src = torch.randn((B, Ns, D), generator=g)
    idx = torch.randint(-1, Ns + 2, (B, Nd), generator=g, dtype=torch.int32)  # -1, and >= Ns: no source row
    idx[0, 0], idx[1, Nd // 2], idx[2, Nd - 1], idx[0, Nd - 1] = -1, Ns, 2 ** 31 - 1, -2 ** 31
    idx[1, 0], idx[2, 0] = 0, Ns - 1
    fill = torch.randn((D,), generator=g) if with_fill else None
    add = torch.randn((Nd, D), generator=g) if with_add else None
    got = ops.token_select(src.reshape(B * Ns, D).to(DEV), B, Ns, idx.to(DEV),
                           fill=None if fill is None else fill.to(DEV), add=None if add is None else add.to(DEV))
    ref = _select_ref(src, idx, fill, add)
    assert got.shape == (B * Nd, D)
    assert torch.equal(got.cpu().reshape(B, Nd, D), ref)


@pytest.mark.parametrize("D", MC.D_CASES)
def test_token_select_four_uses_and_their_backwards(D):
    """(a) encoder gather, (b) its backward, (c) decoder un-shuffle with mask token and position table,
    (d) the pick of the masked rows, through ops.TokenSelectFn with the model's own index arithmetic,
    against the reference's gather / un-shuffle. Integer-valued upstream gradients: every sum is exact."""
    import mae
    import ops
    B, Np = 3, 24
    K = MC.kept(Np, 0.75)
    noise = MC.perm_noise(B, Np, 9)
    ids_shuffle, ids_restore, ids_keep, mask = MC.random_masking(noise, K)
    m = mae.create_mae("vit_tiny_patch8_224", 9, (32, 48), decoder_depth=1)
    m.set_mask_noise(noise)
    K2, mask2, enc_idx, dec_idx, pidx, pick_idx, pick_inv = m._masking(B, torch.device(DEV))
    assert K2 == K and torch.equal(mask2.cpu().double(), mask)
    assert torch.equal(pidx.cpu().long(), MC.masked_ids(mask))
    g = torch.Generator().manual_seed(4)
    x = torch.randn((B, Np + 1, D), generator=g)
    # (a): CLS + the kept patches, in shuffle order
    xa = x.reshape(-1, D).to(DEV).requires_grad_(True)
    a = ops.TokenSelectFn.apply(xa, enc_idx, dec_idx, None, None, B, Np + 1)
    ref_a = torch.cat([x[:, :1], MC.gather_tokens(x[:, 1:], ids_keep)], 1)
    assert torch.equal(a.detach().cpu().reshape(B, 1 + K, D), ref_a)
    # (b): the backward scatters the rows back, zeros at the dropped patches, in one launch
    da = torch.randint(-8, 9, (B, 1 + K, D), generator=g).float()
    a.backward(da.reshape(-1, D).to(DEV))
    ref_b = torch.zeros(B, Np + 1, D)
    ref_b[:, 0] = da[:, 0]
    ref_b[:, 1:].scatter_(1, ids_keep.unsqueeze(-1).expand(-1, -1, D), da[:, 1:])
    assert torch.equal(xa.grad.cpu().reshape(B, Np + 1, D), ref_b)
    # (a) then (b) on the values themselves: identity on CLS and the kept rows, zeros elsewhere
    back = ops.token_select(a.detach(), B, 1 + K, dec_idx).cpu().reshape(B, Np + 1, D)
    keep_rows = torch.cat([torch.ones(B, 1, dtype=torch.bool), ~mask.bool()], 1)
    assert torch.equal(back, torch.where(keep_rows.unsqueeze(-1), x, torch.zeros_like(x)))
    # (c): un-shuffle with the mask token and the position table, and its backward
    y = torch.randn((B, 1 + K, D), generator=g)
    tok = torch.randn((1, 1, D), generator=g)
    pos = torch.randn((Np + 1, D), generator=g)
    yc = y.reshape(-1, D).to(DEV).requires_grad_(True)
    tc = tok.to(DEV).requires_grad_(True)
    c = ops.TokenSelectFn.apply(yc, dec_idx, enc_idx, tc, pos.to(DEV), B, 1 + K)
    ref_c = torch.cat([y[:, :1], MC.unshuffle_tokens(y[:, 1:], tok, ids_restore)], 1) + pos
    assert torch.equal(c.detach().cpu().reshape(B, Np + 1, D), ref_c)
    dc = torch.randint(-8, 9, (B, Np + 1, D), generator=g).float()
    c.backward(dc.reshape(-1, D).to(DEV))
    yr, tr = y.clone().requires_grad_(True), tok.clone().requires_grad_(True)
    (torch.cat([yr[:, :1], MC.unshuffle_tokens(yr[:, 1:], tr, ids_restore)], 1) * dc).sum().backward()
    assert torch.equal(yc.grad.cpu().reshape(B, 1 + K, D), yr.grad)
    assert tc.grad.shape == tok.shape and torch.equal(tc.grad.cpu(), tr.grad)
    # (c) then its backward's gather on the values: the un-shuffled rows of the encoder's tokens
    assert torch.equal(ops.token_select(c.detach(), B, Np + 1, enc_idx).cpu().reshape(B, 1 + K, D),
                       ref_c.gather(1, enc_idx.cpu().long().unsqueeze(-1).expand(-1, -1, D)))
    # (d): the masked rows (ascending patch order) for the prediction head, and its backward
    zd = x.reshape(-1, D).to(DEV).requires_grad_(True)
    d = ops.TokenSelectFn.apply(zd, pick_idx, pick_inv, None, None, B, Np + 1)
    mi = MC.masked_ids(mask)
    assert torch.equal(d.detach().cpu().reshape(B, Np - K, D), MC.gather_tokens(x[:, 1:], mi))
    dd = torch.randint(-8, 9, (B, Np - K, D), generator=g).float()
    d.backward(dd.reshape(-1, D).to(DEV))
    ref_d = torch.zeros(B, Np + 1, D)
    ref_d[:, 1:].scatter_(1, mi.unsqueeze(-1).expand(-1, -1, D), dd)
    assert torch.equal(zd.grad.cpu().reshape(B, Np + 1, D), ref_d)


# ------------------------------------------------------------------------------ ivit_token_fill_grad
@pytest.mark.parametrize("Nd", MC.SELECT_ND)
@pytest.mark.parametrize("D", MC.D_CASES)
def test_token_fill_grad_exact_accumulate_and_repeatable(D, Nd):
    import ops
    B, Ns = MC.SELECT_B, Nd + 4
    g = torch.Generator().manual_seed(7 * D + Nd)
    idx = torch.randint(-1, Ns + 2, (B, Nd), generator=g, dtype=torch.int32)
    idx[0, 0], idx[B - 1, Nd - 1] = -1, Ns
    out_of_range = ((idx < 0) | (idx >= Ns)).reshape(-1)
    dy = torch.randint(-8, 9, (B * Nd, D), generator=g).float()  # any summation order is exact in f32
    ref = dy.double()[out_of_range].sum(0)
    got = ops.token_fill_grad(dy.to(DEV), B, idx.to(DEV), Ns)
    assert torch.equal(got.cpu().double(), ref)
    acc = torch.randint(-8, 9, (D,), generator=g).float().to(DEV)
    base = acc.clone()
    ops.token_fill_grad(dy.to(DEV), B, idx.to(DEV), Ns, out=acc, accumulate=True)
    assert torch.equal(acc.cpu().double(), base.cpu().double() + ref)
    dyn = torch.randn((B * Nd, D), generator=g).to(DEV)
    r1 = ops.token_fill_grad(dyn, B, idx.to(DEV), Ns)
    r2 = ops.token_fill_grad(dyn, B, idx.to(DEV), Ns)
    assert torch.equal(r1, r2)
    assert _rel2(r1, dyn.double().cpu()[out_of_range].sum(0)) < 1e-5


# ------------------------------------------------------------------------------ ivit_mae_loss_*
def _loss_cases():
    out = []
    for C, P, grid in MC.LOSS_SHAPES:
        for B in MC.LOSS_B:
            for Nm in MC.loss_nm(*grid):
                out.append(pytest.param(C, P, grid, B, Nm, id=f"C{C}-P{P}-{grid[0]}x{grid[1]}-B{B}-Nm{Nm}"))
    return out


def _run_loss(pred, img, pidx, P, norm_pix, gout):
    import ops
    pd, im, pi = pred.to(DEV), img.to(DEV), pidx.to(DEV)
    loss, finite, pl, stats = ops.mae_loss_fwd(pd, im, pi, P, norm_pix)
    dpred = ops.mae_loss_bwd(pd, im, pi, P, stats, torch.tensor([gout], device=DEV), finite)
    return loss.cpu(), finite.cpu(), pl.cpu(), stats.cpu(), dpred.cpu()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,P,grid,B,Nm", _loss_cases())
def test_mae_loss_integer_inputs_within_4_ulp(C, P, grid, B, Nm, dtype):
    """Small-integer pred and raster (|v| <= 8, bf16-representable): every squared difference and
    per-patch sum is exact in f32, only the final scalings round. Per-patch loss, scalar loss and
    dpred within 4 f32 ulps of f64; a bf16 dpred within one further bf16 rounding (half a bf16 ulp)."""
    pred, img, pidx = MC.loss_case(C, P, grid, B, Nm, seed=C * 100 + B * 10 + Nm)
    gout = 0.37
    g32 = float(torch.tensor(gout, dtype=torch.float32))
    loss, finite, pl, stats, dpred = _run_loss(pred.to(dtype), img, pidx, P, False, gout)
    rl, rpl = MC.mae_loss(pred, img, pidx, P, False)
    rd = MC.mae_loss_grad(pred, img, pidx, P, False, gout=g32)
    assert float(finite) == 1.0
    assert torch.equal(stats, torch.tensor([0.0, 1.0]).expand(B * Nm, 2))
    e_pl = ((pl.double() - rpl).abs() / MC.ulp32(rpl)).max()
    e_l = (loss.double() - rl).abs() / MC.ulp32(rl)
    print(f"per-patch loss {float(e_pl):.2f} ulp, scalar loss {float(e_l):.2f} ulp")
    assert float(e_pl) <= 4.0 and float(e_l) <= 4.0
    assert dpred.dtype == dtype and dpred.shape == pred.shape
    bound = 4.0 * MC.ulp32(rd)
    if dtype == torch.bfloat16:
        bound = bound + 0.5 * MC.ulp32(rd) * 65536.0  # a bf16 ulp is 2^16 f32 ulps
    excess = ((dpred.double() - rd).abs() / bound).max()
    print(f"dpred {float(excess):.3f} of its bound")
    assert float(excess) <= 1.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,P,grid", MC.LOSS_SHAPES)
def test_mae_loss_norm_pix_with_a_zero_patch(C, P, grid, dtype):
    """Random inputs, one all-zero patch (common in LiDAR occupancy): finite, and loss and dpred within
    the fp32 bar, 1e-3 relative L2, of f64. A bf16 dpred carries one bf16 rounding of every element
    (relative 2^-9) on top, so its bar is 1e-3 + 2^-9; its pred holds bf16-representable values."""
    B, Nm = 3, grid[0] * grid[1] - 1
    pred, img, pidx = MC.loss_case(C, P, grid, B, Nm, seed=C + P, integer=False, zero_patch=True)
    pred = pred.to(dtype)
    loss, finite, pl, stats, dpred = _run_loss(pred, img, pidx, P, True, 1.5)
    rl, rpl = MC.mae_loss(pred.float(), img, pidx, P, True)
    rd = MC.mae_loss_grad(pred.float(), img, pidx, P, True, gout=1.5)
    assert float(finite) == 1.0 and torch.isfinite(pl).all() and torch.isfinite(dpred.float()).all()
    assert float(stats[0, 0]) == 0.0 and abs(float(stats[0, 1]) - 1000.0) < 1e-2  # the zero patch: rstd = 1e-6^-1/2
    errs = (abs(float(loss) - float(rl)) / float(rl), _rel2(pl, rpl), _rel2(dpred.float(), rd))
    print(f"norm_pix C{C} P{P} {dtype}: loss {errs[0]:.3e}, per-patch {errs[1]:.3e}, dpred {errs[2]:.3e}")
    assert errs[0] < 1e-3 and errs[1] < 1e-3
    assert errs[2] < (1e-3 if dtype == torch.float32 else 1e-3 + 2.0 ** -9)


def test_mae_loss_norm_pix_large_common_level():
    """A raster riding on a level 200 times its spread (the statistics are one pass of shifted sums):
    still within the fp32 bar of f64 on the f32 values the kernel reads."""
    C, P, grid, B, Nm = 5, 8, (3, 5), 2, 14
    pred, img, pidx = MC.loss_case(C, P, grid, B, Nm, seed=17, integer=False)
    img = img + 300.0
    loss, finite, pl, stats, dpred = _run_loss(pred, img, pidx, P, True, 1.0)
    rl, rpl = MC.mae_loss(pred, img, pidx, P, True)
    rd = MC.mae_loss_grad(pred, img, pidx, P, True)
    errs = (abs(float(loss) - float(rl)) / float(rl), _rel2(pl, rpl), _rel2(dpred, rd))
    print(f"norm_pix at level 300: loss {errs[0]:.3e}, per-patch {errs[1]:.3e}, dpred {errs[2]:.3e}")
    assert float(finite) == 1.0 and max(errs) < 1e-3
    t = MC.patchify(img.double(), P).gather(1, pidx.long().unsqueeze(-1).expand(-1, -1, C * P * P))
    assert _rel2(stats[:, 0], t.mean(-1).reshape(-1)) < 1e-6
    assert _rel2(stats[:, 1], 1.0 / (t.var(-1).reshape(-1) + 1e-6).sqrt()) < 1e-4


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_mae_loss_nan_gives_flag_zero_and_zero_gradient(dtype):
    C, P, grid, B, Nm = 9, 8, (4, 6), 3, 18
    pred, img, pidx = MC.loss_case(C, P, grid, B, Nm, seed=3)
    pred[Nm + 2, 77] = float("nan")
    loss, finite, pl, stats, dpred = _run_loss(pred.to(dtype), img, pidx, P, False, 1.0)
    assert float(finite) == 0.0 and math.isnan(float(loss))
    assert int(torch.isnan(pl).sum()) == 1 and math.isnan(float(pl[Nm + 2]))
    assert torch.equal(dpred.float(), torch.zeros_like(pred))
    # a patch index outside the grid reads nothing and poisons the step the same way
    pred, img, pidx = MC.loss_case(C, P, grid, B, Nm, seed=3)
    pidx[1, 4], pidx[2, 0] = grid[0] * grid[1], -1
    loss, finite, pl, stats, dpred = _run_loss(pred.to(dtype), img, pidx, P, True, 1.0)
    assert float(finite) == 0.0 and int(torch.isnan(pl).sum()) == 2
    assert torch.equal(dpred.float(), torch.zeros_like(pred))


def test_mae_loss_function_autograd_and_flag():
    import ops
    C, P, grid, B, Nm = 5, 8, (3, 5), 2, 9
    pred, img, pidx = MC.loss_case(C, P, grid, B, Nm, seed=8, integer=False)
    p = pred.to(DEV).requires_grad_(True)
    loss, finite, pl = ops.MaeLossFn.apply(p, img.to(DEV), pidx.to(DEV), P, False)
    assert loss.dim() == 0 and finite.shape == (1,) and float(finite) == 1.0 and not finite.requires_grad
    (loss * 3.0).backward()
    assert _rel2(p.grad, MC.mae_loss_grad(pred, img, pidx, P, False, gout=3.0)) < 1e-6


# ------------------------------------------------------------------------------ attention at N = 7
def _attn_ref(qkv, B, N, H):
    q, k, v = qkv.double().reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) / 8.0
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * N, H * 64), torch.logsumexp(s, -1)


@pytest.mark.parametrize("H", [3, 6])
@pytest.mark.parametrize("cd", [torch.float32, torch.bfloat16])
def test_attention_at_seven_tokens(cd, H):
    """The MAE encoder at (32, 48) runs attention at N = 1 + 6 = 7 tokens, below every N the op tests
    reach in f32 (64) and beside those of the prescaled bf16 pair (1, 33): forward and backward of the
    entries the two block paths call, at tests/test_gpu_ops.py's tolerances."""
    import ops
    from _lib import BF16, F32
    B, N, D = 2, 7, H * 64
    g = torch.Generator().manual_seed(H)
    qkv = ops.cast(torch.randn((B * N, 3 * D), generator=g).to(DEV), cd)
    do = ops.cast(torch.randn((B * N, D), generator=g).to(DEV), cd)
    qr = qkv.float().cpu().double().requires_grad_(True)
    oref, lref = _attn_ref(qr, B, N, H)
    oref.backward(do.float().cpu().double())
    gref = qr.grad.reshape(B * N, 3, D)
    if cd == torch.float32:
        o, lse = ops.attn_fwd(qkv, B, N, H, F32)
        dq = ops.attn_bwd(qkv, o, do, lse, B, N, H, F32)
        tol_o, tol_l, tol_g = 1e-5, 1e-5, 1e-4
    else:
        qs = qkv.clone()
        qs[:, :D] = (qkv[:, :D].float() * ops.Q2_SCALE).to(torch.bfloat16)
        o, lse = ops.attn_fwd_q2(qs, B, N, H)
        dq = ops.attn_bwd_q2(qs, o, do, lse, B, N, H)
        tol_o, tol_l, tol_g = 2e-2, 3e-3, 3e-2
        o2, l2 = ops.attn_fwd(qkv, B, N, H, BF16)
        assert torch.equal(o, o2) and torch.equal(lse, l2)
    assert _rel2(o.float(), oref) < tol_o and _rel2(lse, lref) < tol_l
    d = dq.float().cpu().reshape(B * N, 3, D)
    for i in range(3):
        assert _rel2(d[:, i], gref[:, i]) < tol_g, ("qkv"[i], _rel2(d[:, i], gref[:, i]))


# ------------------------------------------------------------------------------ model
def _build(arch, norm_pix, dtype, seed=0, **over):
    """A MaskedAutoencoderViT of MC.MODEL_CFG on the GPU with weights large enough to matter."""
    import mae
    cfg = dict(MC.MODEL_CFG, **over)
    torch.manual_seed(seed)
    m = mae.create_mae(arch, cfg["in_chans"], cfg["img_size"], decoder_embed_dim=cfg["decoder_embed_dim"],
                       decoder_depth=cfg["decoder_depth"], decoder_num_heads=cfg["decoder_num_heads"],
                       mask_ratio=cfg["mask_ratio"], norm_pix_loss=norm_pix)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("norm.weight") or name.endswith("norm1.weight") or name.endswith("norm2.weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            elif name in ("mask_token", "encoder.cls_token", "encoder.pos_embed"):
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
    m = m.to(DEV).train()
    m.set_compute_dtype(dtype)
    return m


def _inputs(seed=21):
    cfg = MC.MODEL_CFG
    g = torch.Generator().manual_seed(seed)
    H, W = cfg["img_size"]
    img = torch.randn((cfg["batch"], cfg["in_chans"], H, W), generator=g)
    img[0, :, 8:16, 16:24] = 0.0  # an all-zero patch
    noise = MC.perm_noise(cfg["batch"], (H // 8) * (W // 8), seed)
    return img, noise


def _step(m, img, noise):
    m.zero_grad(set_to_none=True)
    m.set_mask_noise(noise)
    loss, mask = m(img.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), mask.cpu(), {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()}


_FP32_RUNS = {}


def _fp32_run(arch, norm_pix):
    """The fp32 HIP run of (arch, norm_pix): computed once, shared by the fp32 and bf16 tests."""
    key = (arch, norm_pix)
    if key not in _FP32_RUNS:
        m = _build(arch, norm_pix, torch.float32)
        img, noise = _inputs()
        sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        _FP32_RUNS[key] = (sd, img, noise) + _step(m, img, noise)
    return _FP32_RUNS[key]


@pytest.mark.parametrize("norm_pix", [False, True])
def test_model_fp32_matches_f64_reference(norm_pix):
    cfg = MC.MODEL_CFG
    sd, img, noise, loss, mask, grads = _fp32_run(cfg["arch"], norm_pix)
    ref = {k: v.double().clone() for k, v in sd.items()}
    for k in grads:
        ref[k].requires_grad_(True)
    rloss, rmask, _, _ = MC.mae_forward(ref, img.double(), noise, patch=8, enc_heads=3, enc_depth=12,
                                        dec_heads=cfg["decoder_num_heads"], dec_depth=cfg["decoder_depth"],
                                        mask_ratio=cfg["mask_ratio"], norm_pix=norm_pix)
    rloss.backward()
    rloss = rloss.detach()
    assert torch.equal(mask.double(), rmask) and int(mask.sum()) == cfg["batch"] * 18
    e = abs(float(loss) - float(rloss)) / abs(float(rloss))
    print(f"fp32 loss {float(loss):.6f} vs f64 {float(rloss):.6f}: {e:.2e}")
    assert e < 1e-3
    assert {"mask_token", "encoder.cls_token", "encoder.pos_embed", "encoder.patch_embed.proj.weight",
            "encoder.blocks.0.attn.qkv.weight", "decoder_pred.weight", "decoder_embed.bias",
            "decoder_blocks.1.mlp.fc2.weight", "encoder.norm.weight", "decoder_norm.bias"} <= set(grads)
    assert "decoder_pos_embed" not in grads
    worst = ("", 0.0)
    for k, gk in grads.items():
        err = _rel2(gk, ref[k].grad)
        worst = max(worst, (k, err), key=lambda t: t[1])
        assert err < 5e-3, (k, err)
    print(f"worst gradient: {worst[0]} {worst[1]:.2e}")


@pytest.mark.parametrize("norm_pix", [False, True])
@pytest.mark.parametrize("arch", ["vit_tiny_patch8_224", "vit_small_patch8_224"])
def test_model_bf16_close_to_fp32(arch, norm_pix):
    """The engine path (vit_tiny, D = 192) and the row-panel path (vit_small, D = 384) in bf16 against
    the fp32 HIP run of the same weights, at test_bf16_path_close_to_fp32's bar."""
    import ops
    from _lib import BF16
    assert ops.block_on_panel(BF16, 384) and not ops.block_on_panel(BF16, 192)
    sd, img, noise, loss32, mask32, _ = _fp32_run(arch, norm_pix)
    m = _build(arch, norm_pix, torch.bfloat16)
    m.load_state_dict(sd)
    loss, mask, grads = _step(m, img, noise)
    assert torch.equal(mask, mask32)
    e = abs(float(loss) - float(loss32)) / abs(float(loss32))
    print(f"{arch} bf16 loss {float(loss):.6f} vs fp32 {float(loss32):.6f}: {e:.2e}")
    assert e < 6e-2
    assert float(m.last_finite) == 1.0
    for k, gk in grads.items():
        assert torch.isfinite(gk).all() and float(gk.abs().max()) > 0.0, k


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_model_same_noise_twice_is_bitwise_identical(dtype):
    m = _build("vit_small_patch8_224", True, dtype)
    img, noise = _inputs(5)
    l1, m1, g1 = _step(m, img, noise)
    l2, m2, g2 = _step(m, img, noise)
    assert torch.equal(l1, l2) and torch.equal(m1, m2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    # another draw gives another mask (the noise is what decides it)
    m.set_mask_noise(None)
    assert m._masking(2, torch.device(DEV))[1].shape == m1.shape


# ------------------------------------------------------------------------------ round trip
def test_encoder_checkpoint_round_trip(tmp_path):
    import model_vit
    import vit
    m = _build("vit_small_patch8_224", False, torch.float32, decoder_depth=1)
    path = tmp_path / "mae_map_encoder.pth"
    m.save_encoder(path)
    saved = torch.load(path, map_location="cpu", weights_only=True)
    assert set(saved) == set(m.encoder.state_dict())
    v = vit.create_model("vit_small_patch8_224", in_chans=9, img_size=(32, 48))
    info = v.load_pretrained(str(path))
    assert info["old_grid"] is None and info["in_chans"] is None and info["new_grid"] == (4, 6)
    for k, t in v.state_dict().items():
        assert torch.equal(t, m.encoder.state_dict()[k].cpu()), k
    v2 = vit.create_model("vit_small_patch8_224", pretrained=True, in_chans=9, img_size=(32, 48),
                          pretrained_cfg_overlay={"file": str(path)})
    assert torch.equal(v2.pos_embed.detach(), saved["pos_embed"])
    # through the detector, for one stream
    net = model_vit.IntentNetViT(backbone_cfg={"img_size": (32, 48), "pretrained_map_file": str(path)})
    for k, t in net.backbone.vit_map.state_dict().items():
        assert torch.equal(t, saved[k]), k
    assert not torch.equal(net.backbone.vit_lidar.blocks[0].attn.qkv.weight, saved["blocks.0.attn.qkv.weight"])
    # and at another grid (the existing resample path)
    v3 = vit.create_model("vit_small_patch8_224", in_chans=9, img_size=(48, 64))
    info = v3.load_pretrained(str(path), old_grid=(4, 6))
    assert info["old_grid"] == (4, 6) and info["new_grid"] == (6, 8)
    assert torch.equal(v3.blocks[3].mlp.fc1.weight.detach(), saved["blocks.3.mlp.fc1.weight"])


# ------------------------------------------------------------------------------ entry
def test_pretrain_mae_entry_lowers_the_loss_and_writes_its_files(tmp_path):
    """20 steps on one fixed synthetic batch at the learning rate test_cpu_mae_cases.py checks on the
    f64 reference with torch.optim.AdamW."""
    import pretrain_mae
    args = pretrain_mae.parse_args(["--synthetic", "--grid", "32x48", "--batch", "2", "--epochs", "1",
                                    "--batches-per-epoch", "20", "--lr", "1e-3", "--save-dir", str(tmp_path),
                                    "--dump-recon", str(tmp_path / "recon")])
    out = pretrain_mae.run(args)
    losses = out["losses"]
    print("losses:", " ".join(f"{v:.5f}" for v in losses))
    assert len(losses) == 20 and all(math.isfinite(v) for v in losses)
    assert losses[-1] < losses[0]
    full, enc, rec = tmp_path / "mae_lidar.pth", tmp_path / "mae_lidar_encoder.pth", tmp_path / "recon" / "recon_lidar.pt"
    assert full.is_file() and enc.is_file() and rec.is_file()
    ck = torch.load(full, map_location="cpu", weights_only=False)
    assert {"model_state_dict", "optimizer_state_dict", "mae_cfg", "epoch"} <= set(ck)
    assert ck["mae_cfg"]["arch"] == "vit_small_patch8_224" and tuple(ck["mae_cfg"]["img_size"]) == (32, 48)
    assert "mask_token" in ck["model_state_dict"] and "encoder.pos_embed" in ck["model_state_dict"]
    e = torch.load(enc, map_location="cpu", weights_only=True)
    assert "pos_embed" in e and not any(k.startswith(("encoder.", "decoder", "mask_token")) for k in e)
    r = torch.load(rec, map_location="cpu", weights_only=True)
    assert r["recon"].shape == r["input"].shape == (2, 290, 32, 48) and r["mask"].shape == (2, 24)
    assert torch.isfinite(r["recon"]).all()
    kept = MC.patchify(r["input"], 8)[r["mask"] < 0.5]
    assert torch.equal(MC.patchify(r["recon"], 8)[r["mask"] < 0.5], kept)  # kept patches show the input
