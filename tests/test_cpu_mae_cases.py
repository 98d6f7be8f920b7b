"""MAE pre-training without a GPU: the f64 reference of tests/mae_cases.py checked against itself and
torch, and the device-free surface of the new entries (header, ctypes prototypes, argument refusals,
workspace queries, the mask-ratio guard, the pretrain_mae.py parser)."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import _lib
import mae_cases as MC
from conftest import REPO

LIB = os.path.join(REPO, "visiontransformer-intention-prediction_amd", "libivit_hip.so")
HEADER = os.path.join(REPO, "include", "ivit.h")
F64 = torch.float64
NEW = ("ivit_token_select", "ivit_token_fill_grad_workspace", "ivit_token_fill_grad", "ivit_mae_loss_workspace",
       "ivit_mae_loss_fwd", "ivit_mae_loss_bwd")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libivit_hip.so not built (run __graft_entry__.build())")


# ------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("C,P,grid", MC.LOSS_SHAPES)
def test_patchify_is_the_patch_embedding_conv(C, P, grid):
    g = torch.Generator().manual_seed(1)
    D = 24
    img = torch.randn((2, C, grid[0] * P, grid[1] * P), generator=g, dtype=F64)
    W = torch.randn((D, C, P, P), generator=g, dtype=F64)
    b = torch.randn((D,), generator=g, dtype=F64)
    got = MC.patchify(img, P) @ W.reshape(D, -1).T + b
    ref = F.conv2d(img, W, b, stride=P).flatten(2).transpose(1, 2)
    assert torch.allclose(got, ref, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("Np,ratio", [(24, 0.75), (15, 0.75), (6, 0.5), (4500, 0.75), (7, 0.9)])
def test_masking_counts_and_inverse(Np, ratio):
    B = 3
    noise = MC.perm_noise(B, Np, seed=Np)
    assert all(len(set(noise[b].tolist())) == Np for b in range(B))  # no ties
    K = MC.kept(Np, ratio)
    ids_shuffle, ids_restore, ids_keep, mask = MC.random_masking(noise, K)
    assert torch.equal(mask.sum(1), torch.full((B,), float(Np - K), dtype=F64))
    ar = torch.arange(Np).expand(B, -1)
    assert torch.equal(torch.gather(ids_shuffle, 1, ids_restore), ar)
    assert torch.equal(torch.gather(ids_restore, 1, ids_shuffle), ar)
    # masked iff ids_restore >= K, and the kept patches are the K smallest noise values
    assert torch.equal(mask, (ids_restore >= K).to(F64))
    assert MC.masked_ids(mask).shape == (B, Np - K)
    for b in range(B):
        assert sorted(ids_keep[b].tolist()) == sorted(torch.topk(-noise[b], K).indices.tolist())


def test_unshuffle_then_gather_is_identity_on_kept_rows():
    B, Np, D = 3, 24, 8
    g = torch.Generator().manual_seed(3)
    x = torch.randn((B, Np, D), generator=g, dtype=F64)
    K = MC.kept(Np, 0.75)
    _, ids_restore, ids_keep, mask = MC.random_masking(MC.perm_noise(B, Np, 5), K)
    kept_rows = MC.gather_tokens(x, ids_keep)
    tok = torch.full((D,), 7.0, dtype=F64)
    full = MC.unshuffle_tokens(kept_rows, tok, ids_restore)
    assert torch.equal(MC.gather_tokens(full, ids_keep), kept_rows)
    m = mask.bool()
    assert torch.equal(full[~m], x[~m])  # kept rows are back in their places
    assert torch.equal(full[m], tok.expand(int(m.sum()), D))  # every masked place holds the mask token


@pytest.mark.parametrize("norm_pix", [False, True])
def test_loss_gradient_matches_autograd(norm_pix):
    C, P, grid = 5, 8, (3, 5)
    pred, img, pidx = MC.loss_case(C, P, grid, 3, 7, seed=11, integer=False, zero_patch=True)
    p = pred.to(F64).requires_grad_(True)
    loss, pl = MC.mae_loss(p, img, pidx, P, norm_pix)
    assert torch.isfinite(pl).all()
    (loss * 0.37).backward()
    ref = MC.mae_loss_grad(pred, img, pidx, P, norm_pix, gout=0.37)
    assert torch.allclose(p.grad, ref, rtol=1e-12, atol=1e-15)
    if norm_pix:  # the all-zero patch has an all-zero target
        assert torch.equal(MC.patch_targets(img, pidx, P, True)[0, 0], torch.zeros(C * P * P, dtype=F64))


def test_sincos_table_matches_the_package():
    import mae
    for dim, grid in ((192, (4, 6)), (64, (50, 90))):
        ref = MC.sincos_2d(dim, *grid)
        got = mae.sincos_pos_embed_2d(dim, grid)
        assert got.shape == (1, 1 + grid[0] * grid[1], dim) and got.dtype == torch.float32
        assert torch.equal(got[0, 0], torch.zeros(dim))
        assert torch.allclose(got[0].double(), ref, rtol=0, atol=1e-7)
    # rectangular: token gy * gw + gx holds gx in the first half, gy in the second
    t = MC.sincos_2d(8, 2, 3)[1:]
    assert torch.equal(t[0 * 3 + 2, :4], t[1 * 3 + 2, :4]) and torch.equal(t[1 * 3 + 0, 4:], t[1 * 3 + 2, 4:])


def test_reference_adamw_lowers_the_loss_of_the_entry_test():
    """tests/test_gpu_mae.py runs pretrain_mae.py for 20 steps on one fixed batch at lr 1e-3 and
    requires a lower loss at the end: the f64 reference with torch.optim.AdamW (the entry's betas and
    weight decay, a fresh mask per step) does the same."""
    import mae
    from synthetic import synthetic_batch
    torch.manual_seed(0)
    H, W = 32, 48
    model = mae.create_mae("vit_small_patch8_224", 290, (H, W))
    sd = {k: v.detach().to(F64).clone() for k, v in model.state_dict().items()}
    params = [k for k in sd if k != "decoder_pos_embed"]
    for k in params:
        sd[k].requires_grad_(True)
    img = synthetic_batch(2, (H, W))["lidar_bev"].to(F64)
    opt = torch.optim.AdamW([sd[k] for k in params], lr=1e-3, betas=(0.9, 0.95), weight_decay=0.05)
    losses = []
    for step in range(20):
        opt.zero_grad()
        loss = MC.mae_forward(sd, img, MC.perm_noise(2, 24, 100 + step), patch=8, enc_heads=6, enc_depth=12,
                              dec_heads=3, dec_depth=4, mask_ratio=0.75, norm_pix=False)[0]
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < losses[0], losses


# ------------------------------------------------------------------------------ the device-free surface
def test_header_declares_the_entries_in_c():
    txt = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    protos = _lib.parse_header()
    for name in NEW:
        assert re.search(r"\b(int|long)\s+" + name + r"\s*\(", txt), name
        assert name in protos, name
    vp, lg, it = ctypes.c_void_p, ctypes.c_long, ctypes.c_int
    assert protos["ivit_token_select"] == (it, [vp, lg, lg, lg, vp, lg, vp, vp, vp, vp])
    assert protos["ivit_token_fill_grad_workspace"] == (lg, [lg, lg, lg])
    assert protos["ivit_token_fill_grad"] == (it, [vp, lg, lg, lg, vp, lg, vp, it, vp, lg, vp])
    assert protos["ivit_mae_loss_workspace"] == (lg, [lg, lg])
    assert protos["ivit_mae_loss_fwd"] == (it, [vp, it, vp, lg, lg, lg, lg, lg, vp, lg, it, vp, vp, vp, vp, vp, lg, vp])
    assert protos["ivit_mae_loss_bwd"] == (it, [vp, it, vp, lg, lg, lg, lg, lg, vp, lg, vp, vp, vp, vp, vp])
    # the header says which column order the loss compares in
    assert "NOT the" in open(HEADER).read() and "(c, ky, kx)" in open(HEADER).read()


def _refused(rc, dll, text):
    assert rc < 0, rc
    assert text in dll.ivit_last_error().decode(), dll.ivit_last_error()


@needs_lib
def test_token_entries_refuse_bad_arguments():
    dll = _lib.lib.load()
    p = 4096  # a non-null, 16-byte aligned address: every refusal below comes before any device call
    sel = dll.ivit_token_select
    _refused(sel(p, 0, 7, 192, p, 7, None, None, p, None), dll, "non-positive size")
    _refused(sel(p, 2, 7, 192, p, -1, None, None, p, None), dll, "non-positive size")
    _refused(sel(p, 2, 7, 200, p, 7, None, None, p, None), dll, "no multiple of 64")
    _refused(sel(None, 2, 7, 192, p, 7, None, None, p, None), dll, "null src / idx / dst")
    _refused(sel(p, 2, 7, 192, None, 7, None, None, p, None), dll, "null src / idx / dst")
    _refused(sel(p, 2, 7, 192, p, 7, None, None, None, None), dll, "null src / idx / dst")
    _refused(sel(p + 4, 2, 7, 192, p, 7, None, None, p, None), dll, "16-byte aligned")
    _refused(sel(p, 2, 7, 192, p, 7, p + 8, None, p, None), dll, "16-byte aligned")
    _refused(sel(p, 2, 7, 192, p, 7, None, p + 4, p, None), dll, "16-byte aligned")
    _refused(sel(p, 2, 1 << 31, 192, p, 7, None, None, p, None), dll, "above 2^30")
    fg = dll.ivit_token_fill_grad
    need = dll.ivit_token_fill_grad_workspace(2, 25, 192)
    _refused(fg(p, 2, 25, 100, p, 7, p, 0, p, need, None), dll, "no multiple of 64")
    _refused(fg(p, 2, 0, 192, p, 7, p, 0, p, need, None), dll, "non-positive size")
    _refused(fg(None, 2, 25, 192, p, 7, p, 0, p, need, None), dll, "null dy / idx / dfill")
    _refused(fg(p, 2, 25, 192, p, 7, None, 0, p, need, None), dll, "null dy / idx / dfill")
    _refused(fg(p, 2, 25, 192, p, 7, p, 0, None, need, None), dll, "workspace")
    _refused(fg(p, 2, 25, 192, p, 7, p, 0, p + 2, need, None), dll, "misaligned")
    _refused(fg(p, 2, 25, 192, p, 7, p, 0, p, need - 1, None), dll, f"{need} needed")
    with pytest.raises(RuntimeError, match="ivit_token_select failed"):
        _lib.lib.ivit_token_select(p, 2, 7, 200, p, 7, None, None, p, None)


@needs_lib
def test_loss_entries_refuse_bad_arguments():
    dll = _lib.lib.load()
    p = 4096
    need = dll.ivit_mae_loss_workspace(2, 5)

    def fwd(pred=p, dt=_lib.F32, img=p, B=2, C=9, H=32, W=48, P=8, pidx=p, Nm=5, pl=p, st=p, loss=p, fin=p, work=p,
            wb=need):
        return dll.ivit_mae_loss_fwd(pred, dt, img, B, C, H, W, P, pidx, Nm, 0, pl, st, loss, fin, work, wb, None)

    def bwd(pred=p, dt=_lib.BF16, img=p, B=2, C=9, H=32, W=48, P=8, pidx=p, Nm=5, st=p, gout=p, fin=p, dpred=p):
        return dll.ivit_mae_loss_bwd(pred, dt, img, B, C, H, W, P, pidx, Nm, st, gout, fin, dpred, None)

    for f in (fwd, bwd):
        _refused(f(dt=7), dll, "neither f32 nor bf16")
        _refused(f(B=0), dll, "non-positive size")
        _refused(f(Nm=-3), dll, "non-positive size")
        _refused(f(P=4), dll, "patch size 4")
        _refused(f(H=36), dll, "no multiple of the patch size")
        _refused(f(W=52), dll, "no multiple of the patch size")
        _refused(f(P=16, W=40, H=32), dll, "no multiple of the patch size")
        _refused(f(Nm=25), dll, "25 masked patches in a grid of 24")
        _refused(f(pred=None), dll, "null pred / img / pidx")
        _refused(f(img=None), dll, "null pred / img / pidx")
        _refused(f(pidx=None), dll, "null pred / img / pidx")
        _refused(f(pred=p + 8), dll, "16-byte aligned")
        _refused(f(img=p + 4), dll, "16-byte aligned")
    _refused(fwd(pl=None), dll, "null patch_loss / stats / loss / finite")
    _refused(fwd(fin=None), dll, "null patch_loss / stats / loss / finite")
    _refused(fwd(work=None), dll, "workspace")
    _refused(fwd(work=p + 4), dll, "misaligned")
    _refused(fwd(wb=need - 1), dll, f"{need} needed")
    _refused(bwd(gout=None), dll, "null stats / gout / finite / dpred")
    _refused(bwd(dpred=None), dll, "null stats / gout / finite / dpred")
    _refused(bwd(dpred=p + 2), dll, "dpred not 16-byte aligned")


@needs_lib
def test_workspace_queries_are_pure_host():
    dll = _lib.lib.load()
    # fill gradient: one f32 row of partials per 64 destination rows
    assert dll.ivit_token_fill_grad_workspace(8, 4501, 192) == -(-8 * 4501 // 64) * 192 * 4
    assert dll.ivit_token_fill_grad_workspace(3, 151, 384) == 8 * 384 * 4
    assert dll.ivit_token_fill_grad_workspace(1, 1, 64) == 64 * 4
    assert dll.ivit_token_fill_grad_workspace(0, 5, 64) == 0 and dll.ivit_token_fill_grad_workspace(1, -1, 64) == 0
    # loss: (f64 sum, f64 non-finite count) per 2048 patches
    assert dll.ivit_mae_loss_workspace(8, 3375) == 14 * 16
    assert dll.ivit_mae_loss_workspace(1, 1) == 16 and dll.ivit_mae_loss_workspace(1, 2048) == 16
    assert dll.ivit_mae_loss_workspace(1, 2049) == 32
    assert dll.ivit_mae_loss_workspace(0, 4) == 0 and dll.ivit_mae_loss_workspace(4, 0) == 0


def test_mask_ratio_that_keeps_or_masks_nothing_is_refused():
    import mae
    assert mae.kept_count(24, 0.75) == 6 and mae.kept_count(4500, 0.75) == 1125
    for ratio in (1.0, 0.99, 0.97, 0.0):  # 24 patches: keeps 0, 0, 0; masks 0
        with pytest.raises(ValueError, match="at least one patch"):
            mae.kept_count(24, ratio)
        with pytest.raises(ValueError, match="at least one patch"):
            mae.create_mae("vit_tiny_patch8_224", 9, (32, 48), mask_ratio=ratio)
    with pytest.raises(ValueError, match="head dim of 64"):
        mae.create_mae("vit_tiny_patch8_224", 9, (32, 48), decoder_embed_dim=192, decoder_num_heads=4)
    m = mae.create_mae("vit_tiny_patch8_224", 9, (32, 48), decoder_depth=1)
    keys = set(m.state_dict())
    assert {"mask_token", "decoder_pos_embed", "decoder_embed.weight", "decoder_blocks.0.attn.qkv.weight",
            "decoder_norm.bias", "decoder_pred.weight", "encoder.pos_embed", "encoder.blocks.11.mlp.fc2.bias"} <= keys
    assert "decoder_pos_embed" not in dict(m.named_parameters())
    assert m.decoder_pred.weight.shape == (9 * 64, 192) and m.mask_token.shape == (1, 1, 192)
    assert all(b.drop_path_rate == 0.0 for b in m.encoder.blocks)
    assert set(m.encoder_state_dict()) == set(m.encoder.state_dict())


def test_pretrain_mae_parser():
    import pretrain_mae
    a = pretrain_mae.parse_args([])
    assert (a.stream, a.arch, a.dtype, a.mask_ratio, a.norm_pix_loss) == ("lidar", "vit_small_patch8_224", "bf16",
                                                                          0.75, False)
    assert (a.decoder_dim, a.decoder_depth, a.batch, a.clip_grad_norm, a.synthetic, a.no_save) == (192, 4, 8, None,
                                                                                                   False, False)
    assert a.grid == "400x720" and a.dump_recon is None
    a = pretrain_mae.parse_args(["--stream", "map", "--synthetic", "--arch", "vit_tiny_patch8_224", "--grid", "32x48",
                                 "--batch", "2", "--epochs", "3", "--batches-per-epoch", "5", "--dtype", "fp32",
                                 "--mask-ratio", "0.5", "--norm-pix-loss", "--decoder-dim", "128", "--decoder-depth",
                                 "2", "--lr", "1e-3", "--weight-decay", "0.1", "--clip-grad-norm", "2.5", "--augment",
                                 "--save-dir", "/tmp/x", "--no-save", "--dump-recon", "/tmp/y", "--data-dir", "/d"])
    assert (a.stream, a.synthetic, a.arch, a.grid, a.batch, a.epochs, a.batches_per_epoch) == \
        ("map", True, "vit_tiny_patch8_224", "32x48", 2, 3, 5)
    assert (a.dtype, a.mask_ratio, a.norm_pix_loss, a.decoder_dim, a.decoder_depth) == ("fp32", 0.5, True, 128, 2)
    assert (a.lr, a.weight_decay, a.clip_grad_norm, a.augment, a.save_dir, a.no_save, a.dump_recon, a.data_dir) == \
        (1e-3, 0.1, 2.5, True, "/tmp/x", True, "/tmp/y", "/d")
    for bad in (["--stream", "radar"], ["--dtype", "fp16"], ["--decoder-dim", "100"], ["--arch", "resnet50"]):
        with pytest.raises(SystemExit):
            pretrain_mae.parse_args(bad)


def test_ptr_still_refuses_host_tensors():
    import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.ptr(torch.zeros(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.token_select(torch.zeros(14, 192), 2, 7, torch.zeros((2, 7), dtype=torch.int32))
