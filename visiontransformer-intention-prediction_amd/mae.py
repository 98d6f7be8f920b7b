"""Masked-autoencoder pre-training of a ViT stream (He et al. 2021, "Masked Autoencoders Are Scalable
Vision Learners") on the HIP kernels: the encoder is the stream's own ``vit.VisionTransformer`` run on
the kept quarter of the tokens, the decoder a few ``vit.Block``s, the loss the masked patches' mean
squared error against the raster itself. No labels are read, so every log frame can be used, and the
result is a checkpoint that ``VisionTransformer.load_pretrained`` / ``train_vit.py --pretrained-lidar``
take as it stands.

The token gather / un-shuffle (``ops.TokenSelectFn``: ivit_token_select, ivit_token_fill_grad), the
prediction head (``ops.PredLinearFn``) and the loss (``ops.MaeLossFn``: ivit_mae_loss_*) are HIP; the
two argsorts over ``B x Np`` noise values and the index arithmetic around them are torch plumbing.
Only the masked rows reach the prediction head (the paper's code predicts every patch and masks the
loss afterwards: the same loss and gradients at 4/3 of the size).

Column order of a predicted patch: ``(c, ky, kx)``, the order of ``patch_embed.proj.weight.reshape(D, -1)``
and of ivit_patch_im2col_p — not the ``(ky, kx, c)`` of the paper's ``patchify``.

State-dict names follow the paper's code (``mask_token``, ``decoder_embed.*``, ``decoder_pos_embed``,
``decoder_blocks.i.*``, ``decoder_norm.*``, ``decoder_pred.*``); the encoder sits under ``encoder.*``
with timm's keys. Single-GPU only.
"""
from __future__ import annotations

import torch
import torch.nn as nn

import ops
import vit
from _lib import BF16, F32
from layers import LayerNorm, Linear, _LayerNormFn, _LinearFn


def sincos_pos_embed_2d(dim, grid_size, cls_token=True):
    """The paper's fixed 2-D sin-cos table for a (gh, gw) grid, f32 [1, cls + gh * gw, dim], token
    gy * gw + gx: the first half of the channels encodes gx, the second gy (get_2d_sincos_pos_embed:
    its meshgrid puts w first), each half sin then cos at the frequencies 10000^(-i / (dim / 4)); the
    CLS row is zero."""
    if dim % 4 != 0:
        raise ValueError(f"sincos_pos_embed_2d: dim {dim} is no multiple of 4")
    gh, gw = int(grid_size[0]), int(grid_size[1])
    omega = 1.0 / 10000 ** (torch.arange(dim // 4, dtype=torch.float64) / (dim / 4.0))
    gy, gx = torch.meshgrid(torch.arange(gh, dtype=torch.float64), torch.arange(gw, dtype=torch.float64),
                            indexing="ij")

    def enc(pos):
        out = pos.reshape(-1, 1) * omega.reshape(1, -1)
        return torch.cat([out.sin(), out.cos()], 1)
    tab = torch.cat([enc(gx), enc(gy)], 1)
    if cls_token:
        tab = torch.cat([torch.zeros(1, dim, dtype=torch.float64), tab], 0)
    return tab.float().unsqueeze(0)


def random_masking_indices(noise, keep):
    """The paper's random_masking from given noise [B, Np] (argsort ascending: the ``keep`` smallest
    stay): (ids_shuffle, ids_restore, mask [B, Np] f32, 1 = masked). Device tensors, no host read."""
    ids_shuffle = torch.argsort(noise, dim=1)
    ids_restore = torch.argsort(ids_shuffle, dim=1)
    mask = (ids_restore >= keep).to(torch.float32)
    return ids_shuffle, ids_restore, mask


def kept_count(num_patches, mask_ratio):
    """K = int(Np (1 - mask_ratio)); a ratio that keeps or masks nothing is refused."""
    keep = int(num_patches * (1.0 - mask_ratio))
    if keep < 1 or num_patches - keep < 1:
        raise ValueError(f"mask_ratio {mask_ratio} keeps {keep} of {num_patches} patches: at least one patch must "
                         f"be kept and at least one masked")
    return keep


def _run_blocks(blocks, t, B, N, cdt, D):
    """The blocks' forward_flat chain of VisionTransformer.forward_tokens_steps on a [B*N, D] stream:
    on the row-panel path each block's fc2 epilogue runs the next block's norm1 and the blocks hand
    their bf16 gradients back; block 0 has nobody to hand to (its input comes out of a gather)."""
    fuse = ops.block_on_panel(cdt, D)
    hands = [ops.GradHandoff() for _ in blocks] if fuse and torch.is_grad_enabled() else None
    ln = None
    for i, blk in enumerate(blocks):
        nxt = blocks[i + 1].norm1 if fuse and i + 1 < len(blocks) else None
        t, nxt_ln = blk.forward_flat(t, B, N, cdt, ln_in=ln, next_norm=nxt, hand_mine=hands[i] if hands else None,
                                     hand_prev=hands[i - 1] if hands and i > 0 else None)
        ln = nxt_ln if nxt is not None else None
    return t


class MaskedAutoencoderViT(nn.Module):
    def __init__(self, encoder, decoder_embed_dim=192, decoder_depth=4, decoder_num_heads=3, mask_ratio=0.75,
                 norm_pix_loss=False):
        super().__init__()
        if not isinstance(encoder, vit.VisionTransformer):
            raise TypeError("MaskedAutoencoderViT: encoder must be a vit.VisionTransformer")
        if decoder_embed_dim != 64 * decoder_num_heads:
            raise ValueError(f"decoder_embed_dim {decoder_embed_dim} / {decoder_num_heads} heads: the attention "
                             f"kernels take a head dim of 64")
        if any(b.drop_path_rate > 0.0 for b in encoder.blocks):
            raise ValueError("MaskedAutoencoderViT: build the encoder with drop_path_rate=0 (create_mae does)")
        if any(b.window_size is not None for b in encoder.blocks):
            # the encoder runs on a gathered subset of the tokens: a spatial window has no meaning there
            raise ValueError("MaskedAutoencoderViT: the encoder has windowed-attention blocks "
                             f"{encoder.windowed_blocks()}; pre-train with window_size=None")
        self.encoder = encoder
        pe = encoder.patch_embed
        self.patch = pe.patch_size[0]
        self.in_chans = pe.proj.weight.shape[1]
        self.mask_ratio, self.norm_pix_loss = float(mask_ratio), bool(norm_pix_loss)
        kept_count(pe.num_patches, self.mask_ratio)
        D, Dd = encoder.embed_dim, decoder_embed_dim
        self.decoder_embed = Linear(D, Dd)
        self.mask_token = nn.Parameter(torch.zeros(1, 1, Dd))
        nn.init.normal_(self.mask_token, std=0.02)
        self.register_buffer("decoder_pos_embed", sincos_pos_embed_2d(Dd, pe.grid_size))
        self.decoder_blocks = nn.ModuleList([vit.Block(Dd, decoder_num_heads, 4.0, 0.0) for _ in range(decoder_depth)])
        self.decoder_norm = LayerNorm(Dd, eps=1e-6)
        self.decoder_pred = Linear(Dd, self.in_chans * self.patch * self.patch)
        self.compute_dtype = torch.float32
        self._noise = None
        self.last_finite = None
        self.last_patch_loss = None

    def config(self):
        """The constructor arguments beside the encoder (saved with the full checkpoint)."""
        return {"decoder_embed_dim": self.decoder_embed.out_features, "decoder_depth": len(self.decoder_blocks),
                "decoder_num_heads": self.decoder_blocks[0].attn.num_heads if len(self.decoder_blocks) else
                self.decoder_embed.out_features // 64,
                "mask_ratio": self.mask_ratio, "norm_pix_loss": self.norm_pix_loss}

    def set_compute_dtype(self, dtype):
        assert dtype in (torch.float32, torch.bfloat16)
        for m in self.modules():
            m.compute_dtype = dtype
        return self

    def set_mask_noise(self, noise):
        """Inject the masking noise [B, Np] (parity tests) instead of drawing it; None draws again."""
        self._noise = noise

    def _masking(self, B, device):
        Np = self.encoder.patch_embed.num_patches
        K = kept_count(Np, self.mask_ratio)
        if self._noise is not None:
            noise = torch.as_tensor(self._noise, dtype=torch.float32).to(device)
            if tuple(noise.shape) != (B, Np):
                raise ValueError(f"mask noise {tuple(noise.shape)} != {(B, Np)}")
        else:
            noise = torch.rand((B, Np), device=device)
        ids_shuffle, ids_restore, mask = random_masking_indices(noise, K)
        i32 = torch.int32
        zero = torch.zeros((B, 1), dtype=i32, device=device)
        # token rows: 0 is CLS, 1 + p patch p
        enc_idx = torch.cat([zero, ids_shuffle[:, :K].to(i32) + 1], 1)  # encoder row j <- full row
        r = ids_restore.to(i32)
        dec_idx = torch.cat([zero, torch.where(r < K, r + 1, torch.full_like(r, -1))], 1)  # full row <- encoder row
        # the masked patches in ascending order: neighbouring workgroups of the loss share raster lines
        pidx = torch.sort(ids_shuffle[:, K:], dim=1).values
        pick_idx = (pidx + 1).to(i32)
        pick_inv = torch.full((B, Np + 1), -1, dtype=i32, device=device)
        pick_inv.scatter_(1, pidx + 1, torch.arange(Np - K, dtype=i32, device=device).expand(B, -1))
        return K, mask, enc_idx.contiguous(), dec_idx.contiguous(), pidx.to(i32).contiguous(), pick_idx.contiguous(), pick_inv

    def _cdt(self):
        return BF16 if self.compute_dtype == torch.bfloat16 else F32

    def _predict(self, x):
        """-> (pred [B*Nm, C*P*P] in the compute dtype, pidx int32 [B, Nm], mask [B, Np])."""
        enc = self.encoder
        B, C, H, W = x.shape
        if (H, W) != enc.patch_embed.img_size:
            raise ValueError(f"Input size {(H, W)} != model img_size {enc.patch_embed.img_size}")
        cdt = self._cdt()
        D, Dd = enc.embed_dim, self.decoder_embed.out_features
        Np = enc.patch_embed.num_patches
        pe = (x.float().contiguous(), enc.patch_embed.proj.weight, enc.patch_embed.proj.bias, enc.pos_embed,
              enc.cls_token, cdt)
        # no GradHandoff across the gather: the patch embedding takes its f32 token gradient
        t = ops.PatchEmbedFn.apply(*pe, None) if self.patch == 8 else ops.PatchEmbedGenericFn.apply(*pe)
        K, mask, enc_idx, dec_idx, pidx, pick_idx, pick_inv = self._masking(B, x.device)
        t = ops.TokenSelectFn.apply(t, enc_idx, dec_idx, None, None, B, Np + 1)
        t = _run_blocks(enc.blocks, t, B, 1 + K, cdt, D)
        t = _LayerNormFn.apply(t, enc.norm.weight, enc.norm.bias, 1e-6)
        y = _LinearFn.apply(t, self.decoder_embed.weight, self.decoder_embed.bias, cdt)
        y = ops.TokenSelectFn.apply(y, dec_idx, enc_idx, self.mask_token, self.decoder_pos_embed[0], B, 1 + K)
        y = _run_blocks(self.decoder_blocks, y, B, 1 + Np, cdt, Dd)
        y = _LayerNormFn.apply(y, self.decoder_norm.weight, self.decoder_norm.bias, 1e-6)
        z = ops.TokenSelectFn.apply(y, pick_idx, pick_inv, None, None, B, 1 + Np)
        pred = ops.PredLinearFn.apply(z, self.decoder_pred.weight, self.decoder_pred.bias, cdt)
        return pred, pidx, mask

    def forward(self, x):
        """-> (loss 0-d, mask [B, Np] f32 with 1 = masked). ``last_finite``: the loss's device flag
        (f32 [1], 1.0 / 0.0) for ``FusedAdamW.step(finite=...)``; a non-finite loss has zero gradients."""
        pred, pidx, mask = self._predict(x)
        loss, finite, pl = ops.MaeLossFn.apply(pred, x, pidx, self.patch, self.norm_pix_loss)
        self.last_finite, self.last_patch_loss = finite.detach(), pl.detach()
        return loss, mask

    def patchify(self, x):
        """[B, C, H, W] -> [B, Np, C*P*P], columns in (c, ky, kx) order (torch plumbing)."""
        B, C, H, W = x.shape
        P = self.patch
        return x.reshape(B, C, H // P, P, W // P, P).permute(0, 2, 4, 1, 3, 5).reshape(B, -1, C * P * P)

    def unpatchify(self, p, C, H, W):
        P = self.patch
        B = p.shape[0]
        return p.reshape(B, H // P, W // P, C, P, P).permute(0, 3, 1, 4, 2, 5).reshape(B, C, H, W)

    def reconstruct(self, x):
        """The raster with every masked patch replaced by its prediction (kept patches show the
        input), [B, C, H, W] f32, and the mask. Eval mode, no_grad; for looking at results."""
        was = self.training
        self.eval()
        try:
            with torch.no_grad():
                pred, pidx, mask = self._predict(x)
                B, C, H, W = x.shape
                Nm = pidx.shape[1]
                rows = self.patchify(x.float())
                pred = pred.float().reshape(B, Nm, -1)
                gi = pidx.long().unsqueeze(-1).expand(-1, -1, rows.shape[-1])
                if self.norm_pix_loss:  # predictions live in the normalised space of their target patch
                    tgt = rows.gather(1, gi)
                    pred = pred * (tgt.var(dim=-1, keepdim=True) + 1e-6).sqrt() + tgt.mean(dim=-1, keepdim=True)
                rows = rows.scatter(1, gi, pred)
                return self.unpatchify(rows, C, H, W).contiguous(), mask
        finally:
            self.train(was)

    def encoder_state_dict(self):
        """The encoder alone, a plain timm-keyed state dict (detached copies on the host)."""
        return {k: v.detach().cpu().clone() for k, v in self.encoder.state_dict().items()}

    def save_encoder(self, path):
        torch.save(self.encoder_state_dict(), str(path))


def create_mae(model_name, in_chans, img_size, **kw):
    """A MaskedAutoencoderViT around vit.create_model(model_name) built with drop_path_rate = 0;
    ``kw``: the MaskedAutoencoderViT arguments."""
    enc = vit.create_model(model_name, in_chans=in_chans, img_size=tuple(img_size), drop_path_rate=0.0)
    return MaskedAutoencoderViT(enc, **kw)
