"""timm-compatible VisionTransformer stream (the object ``timm.create_model`` returns at
model_vit.py:64,71): same attribute surface (``patch_embed.grid_size``, ``num_prefix_tokens``,
``embed_dim``, ``cls_token``, assignable ``head``, ``forward_features``) and the same
``state_dict`` keys as timm's ``vit_{small,tiny}_patch{8,16}_224``, so reference checkpoints load.
Compute runs in ``ops.PatchEmbedFn`` / ``PatchEmbedGenericFn`` + ``ops.ViTBlockPanelFn`` /
``ViTBlockFn`` (HIP)."""
from __future__ import annotations

import math
import os

import torch
import torch.nn as nn

import ops
from _lib import BF16, F32
from layers import Conv2d, LayerNorm, Linear, _LayerNormFn

VIT_ARCH = {
    "vit_small_patch8_224": dict(embed_dim=384, depth=12, num_heads=6, patch=8, mlp_ratio=4),
    "vit_tiny_patch8_224": dict(embed_dim=192, depth=12, num_heads=3, patch=8, mlp_ratio=4),
    # patch-16 variants (timm registry): a stream built from one of these has a coarser grid, which
    # model_vit.py:139 re-grids bilinearly onto the LiDAR grid (ops.BilinearFn)
    "vit_small_patch16_224": dict(embed_dim=384, depth=12, num_heads=6, patch=16, mlp_ratio=4),
    "vit_tiny_patch16_224": dict(embed_dim=192, depth=12, num_heads=3, patch=16, mlp_ratio=4),
}


class PatchEmbed(nn.Module):
    def __init__(self, img_size, patch_size, in_chans, embed_dim):
        super().__init__()
        self.img_size = tuple(img_size)
        self.patch_size = (patch_size, patch_size)
        self.grid_size = (self.img_size[0] // patch_size, self.img_size[1] // patch_size)
        self.num_patches = self.grid_size[0] * self.grid_size[1]
        self.proj = Conv2d(in_chans, embed_dim, patch_size, stride=patch_size)


class Attention(nn.Module):
    def __init__(self, dim, num_heads):
        super().__init__()
        self.num_heads, self.head_dim = num_heads, dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.qkv = Linear(dim, dim * 3)
        self.proj = Linear(dim, dim)


class Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = Linear(dim, hidden)
        self.fc2 = Linear(hidden, dim)


def _window_pair(window_size):
    """(wh, ww) of a window_size argument: None, one int (square) or a pair; at most 256 tokens."""
    if window_size is None:
        return None
    if isinstance(window_size, int):
        window_size = (window_size, window_size)
    try:
        wh, ww = (int(v) for v in window_size)
    except (TypeError, ValueError):
        raise ValueError(f"window_size must be None, an int or (wh, ww), got {window_size!r}") from None
    if wh < 1 or ww < 1 or wh * ww > 256:
        raise ValueError(f"window_size {wh} x {ww}: a window holds 1 to 256 tokens")
    return wh, ww


def default_global_attn_indexes(depth):
    """ViTDet's rule (Li et al. 2022): the last block of each of four equal groups stays global,
    (2, 5, 8, 11) at depth 12. Shallower streams than four blocks keep their last block global."""
    if depth < 4:
        return (depth - 1,)
    return tuple((i + 1) * depth // 4 - 1 for i in range(4))


def resolve_global_attn_indexes(depth, indexes):
    """The sorted block indices that keep global attention: ``indexes`` (negative from the end;
    outside [-depth, depth) raises), or the default rule when None."""
    if indexes is None:
        return default_global_attn_indexes(depth)
    out = set()
    for i in indexes:
        i = int(i)
        if i < -depth or i >= depth:
            raise ValueError(f"global_attn_indexes: block {i} outside a depth-{depth} stream")
        out.add(i + depth if i < 0 else i)
    return tuple(sorted(out))


class Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio, drop_path, window_size=None):
        super().__init__()
        # attention mode: None = global; (wh, ww) = inside windows of wh x ww patches tiling the
        # stream's patch grid from its top-left corner (ops.attn_win_*); assignable
        self.window_size = _window_pair(window_size)
        self.norm1 = LayerNorm(dim, eps=1e-6)
        self.attn = Attention(dim, num_heads)
        self.norm2 = LayerNorm(dim, eps=1e-6)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))
        self.drop_path_rate = drop_path
        # injection hook (parity tests): (attn_scale[B], mlp_scale[B]) used instead of the drawn
        # masks while training; the same per-sample factors oracle.vit_forward_features takes
        self.drop_path_scales = None
        self.last_scales = (None, None)

    def _scales(self, B, device, drawn=None):
        """timm DropPath: per-sample Bernoulli(1-p) / (1-p), independent per branch (identity
        in eval mode or at p = 0). ``drawn``: this block's [2, B] factors from the stream's one
        draw for all blocks (VisionTransformer._draw_drop_path)."""
        p = self.drop_path_rate
        if not self.training or p <= 0.0:
            self.last_scales = (None, None)
            return None, None
        if drawn is not None and self.drop_path_scales is None:
            self.last_scales = (drawn[0], drawn[1])
            return self.last_scales
        if self.drop_path_scales is not None:
            s = torch.stack([torch.as_tensor(v, dtype=torch.float32).reshape(B) for v in self.drop_path_scales])
            s = s.to(device)
        else:
            keep = 1.0 - p
            s = torch.empty((2, B), device=device).bernoulli_(keep).div_(keep)
        self.last_scales = (s[0].contiguous(), s[1].contiguous())
        return self.last_scales

    def forward_flat(self, x, B, N, cdt, ln_in=None, next_norm=None, hand_mine=None, hand_prev=None, drawn=None,
                     grid=None):
        """-> (x_out, (y, mean, rstd) of the next block's norm1, empty tensors without `next_norm`,
        None on the engine path). Row-panel path (ops.ViTBlockPanelFn) only: `ln_in` is this
        block's (y, mean, rstd) of norm1 computed by the previous block's fc2 epilogue; `next_norm`
        the next block's norm1, whose forward this block's fc2 epilogue runs; the hand-offs.
        ``grid``: the stream's patch grid (gh, gw), which a windowed block needs (N = 1 + gh*gw)."""
        s1, s2 = self._scales(B, x.device, drawn)
        params = (self.norm1.weight, self.norm1.bias, self.attn.qkv.weight, self.attn.qkv.bias,
                  self.attn.proj.weight, self.attn.proj.bias, self.norm2.weight, self.norm2.bias,
                  self.mlp.fc1.weight, self.mlp.fc1.bias, self.mlp.fc2.weight, self.mlp.fc2.bias)
        meta = (B, N, self.attn.num_heads, cdt, 1e-6)
        if self.window_size is not None:
            if grid is None or N != 1 + int(grid[0]) * int(grid[1]):
                raise ValueError(f"windowed block (window_size {self.window_size}): needs the patch grid of its "
                                 f"{N} tokens (got grid {grid})")
            wh, ww = _window_pair(self.window_size)
            meta = meta + ((int(grid[0]), int(grid[1]), wh, ww),)
        if not ops.block_on_panel(cdt, x.shape[1]):
            return ops.ViTBlockFn.apply(x, *params, s1, s2, meta), None
        nxw = next_norm.weight if next_norm is not None else None
        nxb = next_norm.bias if next_norm is not None else None
        li, mi, ri = ln_in if ln_in is not None else (None, None, None)
        out = ops.ViTBlockPanelFn.apply(x, li, mi, ri, *params, nxw, nxb, s1, s2, meta, hand_mine, hand_prev)
        return out[0], tuple(out[1:])

    def forward(self, x):
        B, N, D = x.shape
        cdt = BF16 if getattr(self, "compute_dtype", torch.float32) == torch.bfloat16 else F32
        return self.forward_flat(x.reshape(B * N, D).contiguous().float(), B, N, cdt)[0].reshape(B, N, D)


class VisionTransformer(nn.Module):
    def __init__(self, img_size=(224, 224), patch_size=8, in_chans=3, embed_dim=384, depth=12, num_heads=6,
                 mlp_ratio=4.0, drop_path_rate=0.0, window_size=None, global_attn_indexes=None):
        super().__init__()
        self.embed_dim = self.num_features = embed_dim
        self.num_prefix_tokens = 1
        self.patch_embed = PatchEmbed(img_size, patch_size, in_chans, embed_dim)
        n_tok = self.patch_embed.num_patches + 1
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.randn(1, n_tok, embed_dim) * 0.02)
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth)]
        # windowed attention (ViTDet): every block but the global ones attends inside windows; no
        # parameters, no state_dict keys. window_size=None: every block global
        self.window_size = _window_pair(window_size)
        self.global_attn_indexes = (resolve_global_attn_indexes(depth, global_attn_indexes)
                                    if self.window_size is not None else None)
        win = [None if self.window_size is None or i in self.global_attn_indexes else self.window_size
               for i in range(depth)]
        self.blocks = nn.ModuleList([Block(embed_dim, num_heads, mlp_ratio, dpr[i], win[i]) for i in range(depth)])
        self.norm = LayerNorm(embed_dim, eps=1e-6)
        self.head = nn.Identity()
        nn.init.normal_(self.cls_token, std=1e-6)
        self.compute_dtype = torch.float32

    def set_drop_path_scales(self, scales):
        """Inject per-block DropPath factors: a list (one per block) of (attn_scale[B],
        mlp_scale[B]), or None to draw them again (timm semantics)."""
        for i, blk in enumerate(self.blocks):
            blk.drop_path_scales = None if scales is None else scales[i]

    def _draw_drop_path(self, B, device):
        """Every block's DropPath factors of this forward in ONE draw: torch.bernoulli over a cached
        device tensor of the per-block keep probabilities ([depth, 2, B]: attention / MLP branch),
        then one divide — 2 launches per stream instead of 2 per block (timm draws per block and
        branch, the same Bernoulli(1-p)/(1-p) law, a different stream). None when no block drops."""
        if not self.training or all(b.drop_path_rate <= 0.0 for b in self.blocks):
            return None
        # the per-block rates are part of the key: a drop-path schedule that changes them rebuilds it
        key = (device, B, tuple(float(b.drop_path_rate) for b in self.blocks))
        cache = getattr(self, "_keep_cache", None)
        if cache is None or cache[0] != key:
            keep = torch.tensor([1.0 - b.drop_path_rate for b in self.blocks], dtype=torch.float32)
            keep = keep.view(-1, 1, 1).expand(len(self.blocks), 2, B).contiguous().to(device)
            self._keep_cache = cache = (key, keep)
        keep = cache[1]
        return torch.bernoulli(keep).div_(keep)

    def _cdt(self):
        return BF16 if self.compute_dtype == torch.bfloat16 else F32

    def windowed_blocks(self):
        """Indices of the blocks that run windowed attention (Block.window_size is not None)."""
        return [i for i, blk in enumerate(self.blocks) if blk.window_size is not None]

    def load_pretrained(self, path_or_state_dict, old_grid=None):
        """Load a timm checkpoint of this architecture (a ``.pth`` / ``.bin`` / ``.pt`` file through
        ``torch.load(weights_only=True)``, a ``.safetensors`` file, or a state dict) whatever grid and
        input channels it was trained at: checkpoint_filter_fn, then ``load_state_dict(strict=True)``.
        ``old_grid``: the file's patch grid when it is not square. The parameters are written in
        place, so their version counters move and the bf16 shadows and weight packs kept in ``ops``
        rebuild at the next forward. Returns what was done: {'file', 'old_grid', 'new_grid',
        'in_chans'} (old_grid / in_chans None where nothing had to change)."""
        if isinstance(path_or_state_dict, dict):
            sd, name = path_or_state_dict, None
        else:
            name = str(path_or_state_dict)
            sd = _load_file(name)
        sd, info = _filter_state_dict(sd, self, old_grid)
        self.load_state_dict(sd, strict=True)
        info["file"] = name
        return info

    def set_input_size(self, img_size):
        """timm's VisionTransformer.set_input_size: move the stream to another input size. pos_embed
        is REPLACED by a new Parameter, its patch rows resampled onto the new grid
        (resample_abs_pos_embed; the prefix rows keep their bits), and patch_embed.img_size /
        grid_size / num_patches follow. Call it before an optimizer or a ModelEMA is built on the
        model: both hold the old Parameter and would go on updating it."""
        img_size = (int(img_size[0]), int(img_size[1]))
        pe = self.patch_embed
        p = pe.patch_size[0]
        new_grid = (img_size[0] // p, img_size[1] // p)
        if new_grid[0] < 1 or new_grid[1] < 1:
            raise ValueError(f"set_input_size: {img_size} holds no patch of size {p}")
        if new_grid != tuple(pe.grid_size):
            new = resample_abs_pos_embed(self.pos_embed.detach(), new_grid, old_size=tuple(pe.grid_size),
                                         num_prefix_tokens=self.num_prefix_tokens)
            self.pos_embed = nn.Parameter(new, requires_grad=self.pos_embed.requires_grad)
        pe.img_size = img_size
        pe.grid_size = new_grid
        pe.num_patches = new_grid[0] * new_grid[1]
        self._keep_cache = None

    def forward_tokens(self, x):
        """Patch embed + all blocks, without the final norm: (B*(Np+1), D) f32 residual stream."""
        steps = self.forward_tokens_steps(x)
        while True:
            try:
                next(steps)
            except StopIteration as stop:
                return stop.value

    def forward_tokens_steps(self, x):
        """forward_tokens as a generator that yields after the patch embedding and after every
        block (the launches of one step are all enqueued on the current stream when it yields) and
        returns the token stream: model_vit.stream_tokens interleaves the LiDAR and map ViTs block
        by block, so their autograd nodes interleave in creation order and the backward engine
        (which runs the ready node created last first) feeds both HIP streams evenly instead of
        enqueueing one stream's whole backward before the other's."""
        B, C, H, W = x.shape
        if (H, W) != self.patch_embed.img_size:
            raise ValueError(f"Input size {(H, W)} != model img_size {self.patch_embed.img_size} (timm strict size)")
        cdt = self._cdt()
        # row-panel path: block i's fc2 epilogue also produces block i+1's norm1 (ops.ViTBlockPanelFn)
        fuse = ops.block_on_panel(cdt, self.embed_dim)
        # ... and in the backward, block i+1 hands block i its DropPath-scaled bf16 gradient, and
        # block 0 hands the patch embedding its bf16 token gradient
        hands = [ops.GradHandoff() for _ in self.blocks] if fuse and torch.is_grad_enabled() else None
        # (only the patch-8 embedding reads it; the generic patch path takes its f32 dtok)
        p8 = self.patch_embed.proj.weight.shape[-1] == 8
        hand_pe = ops.GradHandoff() if hands and p8 else None
        pe = (x.float().contiguous(), self.patch_embed.proj.weight, self.patch_embed.proj.bias, self.pos_embed,
              self.cls_token, cdt)
        t = ops.PatchEmbedFn.apply(*pe, hand_pe) if p8 else ops.PatchEmbedGenericFn.apply(*pe)
        N = self.patch_embed.num_patches + 1
        grid = tuple(self.patch_embed.grid_size)  # read at call time: set_input_size moves it
        ln = None
        drawn = self._draw_drop_path(B, x.device)
        yield
        for i, blk in enumerate(self.blocks):
            nxt = self.blocks[i + 1].norm1 if fuse and i + 1 < len(self.blocks) else None
            t, nxt_ln = blk.forward_flat(t, B, N, cdt, ln_in=ln, next_norm=nxt,
                                         hand_mine=hands[i] if hands else None,
                                         hand_prev=(hands[i - 1] if i > 0 else hand_pe) if hands else None,
                                         drawn=drawn[i] if drawn is not None else None, grid=grid)
            ln = nxt_ln if nxt is not None else None
            yield
        return t

    def attention_rows(self, x, sample, token, blocks=None, head_mean=True):
        """The attention probabilities of the query tokens (sample[r], token[r]) at the chosen blocks
        (what a forward hook on timm's ``Attention`` reads off softmax(q k^T / sqrt(d))): f32
        [len(blocks), R, N], or [len(blocks), R, H, N] without the head mean; N = patches + 1, key 0
        is CLS. ``blocks``: indices into ``self.blocks`` (negative from the end), default all; the
        result follows their order.

        Eval semantics (no DropPath) under ``torch.no_grad()`` whatever ``self.training`` is; the
        blocks' ``training`` / ``last_scales`` are put back. The fused block ops keep their qkv to
        themselves, so before a requested block this recomputes norm1 and the qkv projection of the
        block's input with the ops the block itself uses (one extra LayerNorm + GEMM per requested
        block; on the row-panel path the LayerNorm is the previous block's hand-over), then
        ops.attn_rows; the residual stream advances through the block's own forward_flat."""
        depth = len(self.blocks)
        blocks = list(range(depth)) if blocks is None else [int(b) for b in blocks]
        want = [b + depth if b < 0 else b for b in blocks]
        if any(b < 0 or b >= depth for b in want):
            raise ValueError(f"attention_rows: blocks {blocks} outside a depth-{depth} stream")
        windowed = [b for b in want if self.blocks[b].window_size is not None]
        if windowed:
            # the rows kernel computes global softmax rows, which a windowed block never forms
            glob = [i for i, blk in enumerate(self.blocks) if blk.window_size is None]
            raise ValueError(f"attention_rows: block(s) {windowed} run windowed attention "
                             f"(window {self.blocks[windowed[0]].window_size}); global blocks available: {glob}")
        B, C, H, W = x.shape
        if (H, W) != self.patch_embed.img_size:
            raise ValueError(f"Input size {(H, W)} != model img_size {self.patch_embed.img_size} (timm strict size)")
        cdt = self._cdt()
        cd = torch.bfloat16 if cdt == BF16 else torch.float32
        nh = self.blocks[0].attn.num_heads
        N = self.patch_embed.num_patches + 1
        fuse = ops.block_on_panel(cdt, self.embed_dim)
        req = ops.RowRequests(sample, token, B, N, x.device)  # checked and uploaded once for all blocks
        found = {}
        saved = [(blk.training, blk.last_scales) for blk in self.blocks]
        try:
            for blk in self.blocks:
                blk.training = False  # Block._scales: identity DropPath, draws nothing
            with torch.no_grad():
                pe = (x.float().contiguous(), self.patch_embed.proj.weight, self.patch_embed.proj.bias,
                      self.pos_embed, self.cls_token, cdt)
                p8 = self.patch_embed.proj.weight.shape[-1] == 8
                t = ops.PatchEmbedFn.apply(*pe, None) if p8 else ops.PatchEmbedGenericFn.apply(*pe)
                ln = None
                for i, blk in enumerate(self.blocks[:max(want) + 1]):
                    if i in want:
                        ln1 = ln[0] if ln is not None else ops.layernorm_fwd(t, blk.norm1.weight, blk.norm1.bias,
                                                                             1e-6, cd)[0]
                        qw, qb = blk.attn.qkv.weight, blk.attn.qkv.bias
                        if fuse:
                            qkv = ops.panel_fwd(ln1, qw, qb, qcols=nh * 64, qscale=ops.Q2_SCALE)[0]
                        elif cdt == BF16:
                            qkv = ops.qkv_fwd_q2(ln1, ops.cast_weight(qw, cd), qb, nh * 64)
                        else:
                            qkv = ops.linear_fwd(ln1, qw, qb, cdt)[0]
                        found[i] = ops.attn_rows(qkv, B, N, nh, cdt, req, head_mean=head_mean, prescaled=cdt == BF16)
                        del qkv
                    if i == max(want):
                        break  # nothing reads the residual stream past the last requested block
                    nxt = self.blocks[i + 1].norm1 if fuse else None
                    t, nxt_ln = blk.forward_flat(t, B, N, cdt, ln_in=ln, next_norm=nxt,
                                                 grid=tuple(self.patch_embed.grid_size))
                    ln = nxt_ln if nxt is not None else None
        finally:
            for blk, (tr, ls) in zip(self.blocks, saved):
                blk.training, blk.last_scales = tr, ls
        return torch.stack([found[b] for b in want])

    def forward_features(self, x):
        B = x.shape[0]
        t = self.forward_tokens(x)
        return _LayerNormFn.apply(t, self.norm.weight, self.norm.bias, 1e-6).reshape(B, -1, self.embed_dim)

    def forward(self, x):
        return self.head(self.forward_features(x)[:, 0])


def _op_device(device):
    """Where the two load-time ops (ops.pos_resample, ops.adapt_input_conv) run for a model on
    ``device``: the model's own GPU, or, for a model still on the host (create_model builds there,
    like timm), the current GPU; the results go back to wherever the model lives. Without a GPU
    there is nothing to run them on: no CPU fallback."""
    device = torch.device(device)
    if device.type == "cuda":
        return device
    if not torch.cuda.is_available():
        raise RuntimeError("resampling pos_embed / adapting patch_embed weights runs on the GPU kernels "
                           "(no CPU fallback): no ROCm device visible")
    return torch.device("cuda", torch.cuda.current_device())


def resample_abs_pos_embed(posemb, new_size, old_size=None, num_prefix_tokens=1, interpolation="bicubic",
                           antialias=True, verbose=False):
    """timm.layers.resample_abs_pos_embed: the patch rows of ``posemb`` (1, prefix + gh * gw, D)
    resampled from the ``old_size`` grid onto ``new_size`` (bicubic, antialiased: ops.pos_resample),
    the prefix rows copied bit for bit. ``old_size=None``: the square grid of the patch-token count.
    Equal sizes return ``posemb`` itself. Only interpolation='bicubic' with antialias=True (timm's
    defaults, what checkpoint_filter_fn uses) is built. The result is f32 on posemb's device."""
    if interpolation != "bicubic" or not antialias:
        raise ValueError(f"resample_abs_pos_embed: only interpolation='bicubic' with antialias=True is implemented "
                         f"(got {interpolation!r}, antialias={antialias})")
    new_size = (int(new_size[0]), int(new_size[1]))
    n_patch = posemb.shape[1] - num_prefix_tokens
    if old_size is None:
        hw = math.isqrt(max(n_patch, 0))
        if hw * hw != n_patch:
            raise ValueError(f"resample_abs_pos_embed: {n_patch} patch tokens are not a square grid; pass old_size")
        old_size = (hw, hw)
    old_size = (int(old_size[0]), int(old_size[1]))
    if old_size[0] * old_size[1] != n_patch:
        raise ValueError(f"resample_abs_pos_embed: old_size {old_size} does not hold {n_patch} patch tokens")
    if old_size == new_size:
        return posemb
    with torch.no_grad():
        src = posemb.detach()
        dev = _op_device(src.device)
        D = src.shape[-1]
        grid = ops.pos_resample(src[0, num_prefix_tokens:].to(dev).reshape(old_size[0], old_size[1], D), new_size)
        out = torch.empty((1, num_prefix_tokens + new_size[0] * new_size[1], D), dtype=torch.float32, device=src.device)
        out[0, :num_prefix_tokens] = src[0, :num_prefix_tokens]
        out[0, num_prefix_tokens:] = grid.reshape(-1, D).to(src.device)
    return out


def adapt_input_conv(in_chans, conv_weight):
    """timm adapt_input_conv (its argument order): 3-channel patch-embedding weights for ``in_chans``
    input channels (ops.adapt_input_conv). f32, on conv_weight's device."""
    dev = _op_device(conv_weight.device)
    return ops.adapt_input_conv(conv_weight.detach().to(dev), in_chans).to(conv_weight.device)


_DROP_PREFIXES = ("head.", "fc_norm.", "pre_logits.", "head_dist.")


def _filter_state_dict(state_dict, model, old_grid=None):
    """checkpoint_filter_fn and what it did: (state dict, {'old_grid', 'new_grid', 'in_chans'})
    with 'old_grid' / 'in_chans' None where nothing was resampled / adapted."""
    for wrap in ("model", "state_dict", "model_state_dict"):
        if wrap in state_dict and isinstance(state_dict[wrap], dict):
            state_dict = state_dict[wrap]
            break
    own = model.state_dict()
    dev = model.pos_embed.device
    new_grid = tuple(model.patch_embed.grid_size)
    info = {"old_grid": None, "new_grid": new_grid, "in_chans": None}
    out = {}
    for k, v in state_dict.items():
        if k.startswith(_DROP_PREFIXES) and k not in own:
            continue
        if k == "pos_embed" and v.dim() == 3:
            grid = tuple(old_grid) if old_grid is not None else None
            if v.shape[1] != model.pos_embed.shape[1] or (grid is not None and grid != new_grid):
                if grid is None:
                    hw = math.isqrt(max(v.shape[1] - model.num_prefix_tokens, 0))
                    grid = (hw, hw)  # resample_abs_pos_embed refuses a count that is no square
                v = resample_abs_pos_embed(v.to(_op_device(dev)), new_grid, old_size=old_grid,
                                           num_prefix_tokens=model.num_prefix_tokens)
                info["old_grid"] = grid
        elif k == "patch_embed.proj.weight" and v.dim() == 4:
            w = model.patch_embed.proj.weight
            if tuple(v.shape[2:]) != tuple(w.shape[2:]):
                raise ValueError(f"checkpoint_filter_fn: patch size {tuple(v.shape[2:])} of the file does not match "
                                 f"the stream's patch size {tuple(w.shape[2:])} (resample_patch_embed is not built)")
            if v.shape[1] != w.shape[1]:
                info["in_chans"] = (int(v.shape[1]), int(w.shape[1]))
                v = adapt_input_conv(w.shape[1], v.to(_op_device(dev)))
        out[k] = v
    return out, info


def checkpoint_filter_fn(state_dict, model, old_grid=None):
    """timm vision_transformer.checkpoint_filter_fn for a stream: unwrap a top-level 'model' /
    'state_dict' / 'model_state_dict'; drop the classifier keys the stream does not have (head.*,
    fc_norm.*, pre_logits.*); resample pos_embed onto the stream's grid when the token counts differ
    (``old_grid``: the file's (gh, gw) when it is not square; given, it also decides between two
    grids of the same count); adapt patch_embed.proj.weight to the stream's input channels. A
    patch-size mismatch is a ValueError. Every other tensor passes through as the same object."""
    return _filter_state_dict(state_dict, model, old_grid)[0]


def _load_file(path):
    path = str(path)
    if path.endswith(".safetensors"):
        try:
            from safetensors.torch import load_file
        except ImportError as e:
            raise RuntimeError(f"{path}: reading .safetensors needs the safetensors package, which does not import "
                               f"({e}); convert the file to .pth") from e
        return load_file(path, device="cpu")
    return torch.load(path, map_location="cpu", weights_only=True)


PRETRAINED_DIR_ENV = "IVIT_PRETRAINED_DIR"


def _pretrained_file(model_name, overlay):
    """The weight file of create_model(pretrained=True): pretrained_cfg_overlay['file'] (timm's
    offline route), else $IVIT_PRETRAINED_DIR/<model_name>.safetensors | .pth | .bin."""
    if overlay and overlay.get("file"):
        return str(overlay["file"])
    root = os.environ.get(PRETRAINED_DIR_ENV)
    tried = []
    if root:
        for ext in (".safetensors", ".pth", ".bin"):
            cand = os.path.join(root, model_name + ext)
            if os.path.isfile(cand):
                return cand
            tried.append(cand)
    raise RuntimeError(f"pretrained=True for {model_name}: nothing is downloaded; give the weight file as "
                       f"pretrained_cfg_overlay={{'file': PATH}}, or set {PRETRAINED_DIR_ENV} to a directory holding "
                       f"{model_name}.safetensors, .pth or .bin"
                       + (f" (looked for {', '.join(tried)})" if tried else f" ({PRETRAINED_DIR_ENV} is not set)"))


def create_model(model_name, pretrained=False, in_chans=3, img_size=(224, 224), drop_path_rate=0.0,
                 pretrained_cfg_overlay=None, window_size=None, global_attn_indexes=None, **_):
    """timm.create_model surface used by the reference (model_vit.py:64,71). ``pretrained=True``
    loads a timm checkpoint of ``model_name`` from a local file (_pretrained_file) through
    VisionTransformer.load_pretrained: pos_embed resampled onto ``img_size``'s grid, the 3-channel
    patch weights adapted to ``in_chans``. ``window_size`` / ``global_attn_indexes``: windowed
    attention in every block but the global ones (VisionTransformer); no state_dict key changes."""
    a = VIT_ARCH[model_name]
    file = _pretrained_file(model_name, pretrained_cfg_overlay) if pretrained else None
    m = VisionTransformer(img_size=img_size, patch_size=a["patch"], in_chans=in_chans, embed_dim=a["embed_dim"],
                          depth=a["depth"], num_heads=a["num_heads"], mlp_ratio=a["mlp_ratio"],
                          drop_path_rate=drop_path_rate, window_size=window_size,
                          global_attn_indexes=global_attn_indexes)
    if file is not None:
        m.load_pretrained(file)
    return m
