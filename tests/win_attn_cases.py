"""Cases and the f64 reference of the windowed attention kernels (csrc/attn_window.hip).

Token layout: token 0 is CLS, patch token 1 + r*gw + c sits at (r, c) of the gh x gw grid. A window
size (wh, ww) tiles the grid from the top-left corner; patch (r, c) belongs to window
(r // wh, c // ww); edge windows are ragged. A patch query attends to the patch keys of its own
window, CLS to itself only.

The reference is masked attention in torch on the CPU in f64, the mask built from the window ids,
gradients from autograd. Inputs are bf16-exact f32 values, so every entry (f32, bf16, q2) reads the
same numbers. The q2 reference takes the Q block as q' = q log2(e)/8 (what the qkv GEMM writes on
the bf16 path) and returns dqkv with respect to the UNSCALED q, and lse in log2 units.
"""
import math

import torch

C2 = 1.4426950408889634 / 8.0  # log2(e) / sqrt(64)
LN2 = 0.6931471805599453

# name -> (gh, gw, wh, ww, H)
CASES = {
    "exact_4x6_w2x3": (4, 6, 2, 3, 2),          # exact tiling
    "ragged_5x7_w2x3": (5, 7, 2, 3, 2),         # ragged in both directions
    "ragged_5x7_w3x7": (5, 7, 3, 7, 2),         # ragged in one direction
    "nw100_20x30_w10x10": (20, 30, 10, 10, 2),  # Nw = 100: partial MFMA tiles
    "nw256_16x32_w16x16": (16, 32, 16, 16, 2),  # Nw = 256, the limit
    "nw256_17x17_w16x16": (17, 17, 16, 16, 2),  # Nw = 256 with 1-wide ragged edges
    "nw1_3x3_w1x1": (3, 3, 1, 1, 2),            # Nw = 1
    "single_4x6_w4x6": (4, 6, 4, 6, 2),         # a single window
    "larger_4x6_w8x8": (4, 6, 8, 8, 2),         # window larger than the grid
    "heads6_20x30_w10x10": (20, 30, 10, 10, 6),  # the stream's head count
}
B = 2
DH = 64


def window_ids(gh, gw, wh, ww):
    """int64 [1 + gh*gw]: the window of every token; CLS gets the id after the last patch window."""
    r = torch.arange(gh).view(gh, 1).expand(gh, gw)
    c = torch.arange(gw).view(1, gw).expand(gh, gw)
    nwc = -(-gw // ww)
    ids = (r // wh) * nwc + (c // ww)
    ncls = (-(-gh // wh)) * nwc
    return torch.cat([torch.tensor([ncls]), ids.reshape(-1)])


def window_tokens(gh, gw, wh, ww):
    """-> list over windows (CLS excluded) of the token indices of each, in row-major order."""
    ids = window_ids(gh, gw, wh, ww)
    return [torch.nonzero(ids == w).flatten() for w in range(int(ids[0]))]


def bf16_exact(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16).float()


def make_inputs(name, seed=0):
    """-> (qkv [B*N, 3*H*64], dout [B*N, H*64]) bf16-exact f32 on the CPU; the Q block holds the
    UNSCALED q (q2_inputs gives the prescaled form)."""
    gh, gw, wh, ww, H = CASES[name]
    N = 1 + gh * gw
    base = sum(ord(ch) for ch in name) * 16 + seed
    return bf16_exact((B * N, 3 * H * DH), base), bf16_exact((B * N, H * DH), base + 1)


def q2_inputs(qkv, H):
    """The q2 form of a qkv tensor: the Q block multiplied by log2(e)/8 and rounded to bf16."""
    out = qkv.clone()
    D = H * DH
    out[:, :D] = (qkv[:, :D] * C2).to(torch.bfloat16).float()
    return out


def masked_attention(q, k, v, mask):
    """softmax(q k^T / 8 masked) v in the dtype of the inputs. q, k, v [B, H, N, 64], mask [N, N] bool.
    -> (out [B, H, N, 64], probabilities [B, H, N, N], lse [B, H, N])."""
    s = q @ k.transpose(-1, -2) / 8.0
    s = s.masked_fill(~mask, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.unsqueeze(-1))
    return p @ v, p, lse


def reference(qkv, dout, gh, gw, wh, ww, H, q2=False):
    """f64 reference: -> dict(out [B*N, D], lse [B, H, N], dqkv [B*N, 3D], p [B, H, N, N]).
    q2: the Q block of qkv is q' = q c2; lse comes in log2 units and dqkv w.r.t. the unscaled q."""
    N = 1 + gh * gw
    Bn = qkv.shape[0] // N
    D = H * DH
    x = qkv.double().reshape(Bn, N, 3, H, DH).permute(2, 0, 3, 1, 4)
    qin = x[0].clone().requires_grad_(True)
    k = x[1].clone().requires_grad_(True)
    v = x[2].clone().requires_grad_(True)
    q = qin / C2 if q2 else qin
    ids = window_ids(gh, gw, wh, ww)
    mask = ids.view(N, 1) == ids.view(1, N)
    out, p, lse = masked_attention(q, k, v, mask)
    go = dout.double().reshape(Bn, N, H, DH).permute(0, 2, 1, 3)
    out.backward(go)
    dq = qin.grad * C2 if q2 else qin.grad  # d/dq = d/dq' * c2
    flat = lambda t: t.permute(0, 2, 1, 3).reshape(Bn * N, D)
    dqkv = torch.cat([flat(dq), flat(k.grad), flat(v.grad)], dim=1)
    return dict(out=flat(out.detach()), lse=(lse.detach() / LN2 if q2 else lse.detach()), dqkv=dqkv,
                p=p.detach())


def rel_err(got, ref):
    """max |got - ref| on the scale of ref's own maximum magnitude."""
    ref = ref.double()
    scale = float(ref.abs().max())
    return float((got.double().cpu() - ref).abs().max()) / (scale if scale > 0 else 1.0)


def default_global_indexes(depth):
    """ViTDet's rule: the last block of each of four equal groups."""
    return tuple((i + 1) * depth // 4 - 1 for i in range(4)) if depth >= 4 else (depth - 1,)


assert math.isclose(C2 * 8.0 * LN2, 1.0, rel_tol=1e-15)
