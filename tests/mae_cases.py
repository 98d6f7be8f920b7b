"""A plain-torch f64 masked autoencoder (He et al. 2021), the reference of tests/test_gpu_mae.py, and
the case lists both MAE test files share. Nothing here touches the package's kernels.

Column order of a patch row: (c, ky, kx), the order of patch_embed.proj.weight.reshape(D, -1) (NOT the
(ky, kx, c) of the paper's patchify). Masking is the paper's random_masking from GIVEN noise; every
case's noise is a scaled permutation, so no argsort tie can decide a test."""
import math

import torch
import torch.nn.functional as F

from oracle.ivit_oracle import _vit_block

F64 = torch.float64


# ------------------------------------------------------------------------------ masking / tokens
def perm_noise(B, Np, seed):
    """[B, Np] f32 noise with distinct values per row: (a permutation + 0.5) / Np."""
    g = torch.Generator().manual_seed(seed)
    return torch.stack([(torch.randperm(Np, generator=g).float() + 0.5) / Np for _ in range(B)])


def kept(Np, mask_ratio):
    return int(Np * (1.0 - mask_ratio))


def random_masking(noise, K):
    """-> (ids_shuffle, ids_restore, ids_keep [B, K], mask [B, Np] with 1 = masked)."""
    ids_shuffle = torch.argsort(noise, dim=1)
    ids_restore = torch.argsort(ids_shuffle, dim=1)
    mask = torch.ones_like(noise, dtype=F64)
    mask[:, :K] = 0
    mask = torch.gather(mask, 1, ids_restore)
    return ids_shuffle, ids_restore, ids_shuffle[:, :K], mask


def gather_tokens(x, ids_keep):
    """x [B, Np, D] -> [B, K, D] (the paper's torch.gather)."""
    return torch.gather(x, 1, ids_keep.unsqueeze(-1).expand(-1, -1, x.shape[-1]))


def unshuffle_tokens(x_kept, mask_token, ids_restore):
    """x_kept [B, K, D] + mask tokens, back in patch order: [B, Np, D]."""
    B, K, D = x_kept.shape
    Np = ids_restore.shape[1]
    full = torch.cat([x_kept, mask_token.reshape(1, 1, D).expand(B, Np - K, D)], 1)
    return torch.gather(full, 1, ids_restore.unsqueeze(-1).expand(-1, -1, D))


def patchify(img, P):
    """[B, C, H, W] -> [B, Np, C*P*P], column (c*P + ky)*P + kx, patch gy*(W/P) + gx."""
    B, C, H, W = img.shape
    return img.reshape(B, C, H // P, P, W // P, P).permute(0, 2, 4, 1, 3, 5).reshape(B, (H // P) * (W // P), C * P * P)


def masked_ids(mask):
    """The masked patches of every sample in ascending order, [B, Nm] int64."""
    B = mask.shape[0]
    return torch.stack([torch.nonzero(mask[b] > 0.5).squeeze(1) for b in range(B)])


# ------------------------------------------------------------------------------ loss
def patch_targets(img, pidx, P, norm_pix):
    """[B, Nm, L] f64 targets of the patches pidx [B, Nm]."""
    t = patchify(img.to(F64), P)
    t = torch.gather(t, 1, pidx.long().unsqueeze(-1).expand(-1, -1, t.shape[-1]))
    if norm_pix:
        t = (t - t.mean(-1, keepdim=True)) / (t.var(-1, keepdim=True) + 1e-6).sqrt()
    return t


def mae_loss(pred, img, pidx, P, norm_pix):
    """pred [B*Nm, L] -> (scalar loss, per-patch loss [B*Nm]) in f64."""
    t = patch_targets(img, pidx, P, norm_pix).reshape(pred.shape)
    pl = ((pred.to(F64) - t) ** 2).mean(-1)
    return pl.mean(), pl


def mae_loss_grad(pred, img, pidx, P, norm_pix, gout=1.0):
    """The hand-written gradient: gout * 2 (pred - target) / (B Nm L)."""
    t = patch_targets(img, pidx, P, norm_pix).reshape(pred.shape)
    return gout * 2.0 * (pred.to(F64) - t) / pred.numel()


# ------------------------------------------------------------------------------ model
def sincos_2d(dim, gh, gw):
    """The paper's get_2d_sincos_pos_embed for a (gh, gw) grid with a zero CLS row: [1 + gh*gw, dim]."""
    omega = 1.0 / 10000 ** (torch.arange(dim // 4, dtype=F64) / (dim / 4.0))
    ys, xs = torch.meshgrid(torch.arange(gh, dtype=F64), torch.arange(gw, dtype=F64), indexing="ij")

    def enc(p):
        o = p.reshape(-1, 1) * omega.reshape(1, -1)
        return torch.cat([o.sin(), o.cos()], 1)
    return torch.cat([torch.zeros(1, dim, dtype=F64), torch.cat([enc(xs), enc(ys)], 1)], 0)


def mae_forward(sd, img, noise, *, patch, enc_heads, enc_depth, dec_heads, dec_depth, mask_ratio, norm_pix):
    """The MAE forward on a state dict with the package's names (encoder.*, mask_token, decoder_*):
    -> (loss, mask, pred [B*Nm, L], pidx [B, Nm]); only the masked rows are predicted."""
    B = img.shape[0]
    w = sd["encoder.patch_embed.proj.weight"]
    D = w.shape[0]
    t = patchify(img, patch) @ w.reshape(D, -1).T + sd["encoder.patch_embed.proj.bias"]
    Np = t.shape[1]
    pos = sd["encoder.pos_embed"]
    t = t + pos[:, 1:]
    K = kept(Np, mask_ratio)
    _, ids_restore, ids_keep, mask = random_masking(noise, K)
    t = gather_tokens(t, ids_keep)
    cls = (sd["encoder.cls_token"] + pos[:, :1]).expand(B, -1, -1)
    t = torch.cat([cls, t], 1)
    for i in range(enc_depth):
        t = _vit_block(sd, f"encoder.blocks.{i}.", t, enc_heads, None, 1e-6, "explicit")
    t = F.layer_norm(t, (D,), sd["encoder.norm.weight"], sd["encoder.norm.bias"], 1e-6)
    y = F.linear(t, sd["decoder_embed.weight"], sd["decoder_embed.bias"])
    Dd = y.shape[-1]
    y = torch.cat([y[:, :1], unshuffle_tokens(y[:, 1:], sd["mask_token"], ids_restore)], 1)
    y = y + sd["decoder_pos_embed"]
    for i in range(dec_depth):
        y = _vit_block(sd, f"decoder_blocks.{i}.", y, dec_heads, None, 1e-6, "explicit")
    y = F.layer_norm(y, (Dd,), sd["decoder_norm.weight"], sd["decoder_norm.bias"], 1e-6)
    pidx = masked_ids(mask)
    z = torch.gather(y[:, 1:], 1, pidx.unsqueeze(-1).expand(-1, -1, Dd)).reshape(-1, Dd)
    pred = F.linear(z, sd["decoder_pred.weight"], sd["decoder_pred.bias"])
    loss, _ = mae_loss(pred, img, pidx, patch, norm_pix)
    return loss, mask, pred, pidx


# ------------------------------------------------------------------------------ case lists
D_CASES = (192, 384)
SELECT_B = 3
SELECT_ND = (7, 25, 151)  # 3 * 151 = 453 rows: an odd count across workgroup boundaries

# (C, P, (gh, gw)) of the loss cases; B in LOSS_B; Nm from 1 to all-but-one patch
LOSS_SHAPES = ((9, 8, (4, 6)), (5, 8, (3, 5)), (290, 8, (2, 3)), (3, 16, (2, 3)))
LOSS_B = (1, 3)


def loss_nm(gh, gw):
    n = gh * gw
    return sorted({1, n // 2, n - 1})


def loss_case(C, P, grid, B, Nm, seed, integer=True, zero_patch=False):
    """-> (pred [B*Nm, L] f32, img [B, C, H, W] f32, pidx [B, Nm] int32 ascending). integer: values in
    [-8, 8] (every sum of the test is exact in f32 and the values are bf16-representable)."""
    g = torch.Generator().manual_seed(seed)
    gh, gw = grid
    L = C * P * P
    if integer:
        pred = torch.randint(-8, 9, (B * Nm, L), generator=g).float()
        img = torch.randint(-8, 9, (B, C, gh * P, gw * P), generator=g).float()
    else:
        pred = torch.randn((B * Nm, L), generator=g)
        img = torch.randn((B, C, gh * P, gw * P), generator=g) * 1.5 + 0.7
    pidx = torch.stack([torch.sort(torch.randperm(gh * gw, generator=g)[:Nm]).values for _ in range(B)]).to(torch.int32)
    if zero_patch:
        pi = int(pidx[0, 0])
        gy, gx = divmod(pi, gw)
        img[0, :, gy * P:(gy + 1) * P, gx * P:(gx + 1) * P] = 0.0
    return pred, img, pidx


MODEL_CFG = dict(arch="vit_tiny_patch8_224", img_size=(32, 48), in_chans=9, decoder_embed_dim=192, decoder_depth=2,
                 decoder_num_heads=3, mask_ratio=0.75, batch=2)


def ulp32(x):
    """The f32 unit in the last place at |x| (f64 tensor in, f64 out)."""
    a = x.abs().to(torch.float32)
    up = torch.nextafter(a, torch.full_like(a, math.inf))
    return (up.double() - a.double()).clamp_min(2.0 ** -149)
