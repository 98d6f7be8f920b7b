"""Peaked-score inputs for the bf16 flash attention, their f64 references and derived error bounds.

A plain helper shared by tests/test_cpu_attn_cases.py (no GPU) and tests/test_gpu_attn_peaked.py.

Inputs are built per (batch, head) directly in the layout the kernels read: q' (Q already times
log2(e)/8, the "q2" layout), k and v, [N, 64] each and bf16-exact, so the score the kernel sees is
S' = q' k^T in log2 units and the references need no allowance for input rounding. Dims 62 and 63
of q' and k carry exact additive bumps: with q'[:, 63] = 1 and k[j, 63] = beta_j, S'_ij = base_ij +
beta_j exactly (every bump used is a bf16-exact integer, at most 63 at N <= 449).

The forward (attn_fwd_bf16_v6_kernel) walks the keys in tiles of AK and moves its running maximum
only when a tile's maximum exceeds it by more than TAU log2 units; random-normal scores never do
that, so CASES is built around that branch, the ragged key mask and one-hot probabilities.
"""
import math
import os
import re

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "visiontransformer-intention-prediction_amd", "csrc")

U = 2.0 ** -8  # bf16 unit roundoff (8 significand bits, round to nearest)
LN2 = math.log(2.0)
C2 = math.log2(math.e) / 8.0  # log2(e) / sqrt(64): ops.Q2_SCALE
DH = 64

CASES = ("stair9", "stair7", "stair4", "down9", "spike_last", "spike_first", "spike_odd", "shift96", "perm", "gain6",
         "rand")


def kernel_constants():
    """(AK, TAU) as the kernel sources define them: the cases are judged against the constants the
    kernel is built with, not against a copy."""
    with open(os.path.join(CSRC, "attn_common.h")) as f:
        ak = re.search(r"constexpr\s+int\s+AK\s*=\s*(\d+)\s*;", f.read())
    with open(os.path.join(CSRC, "attention.hip")) as f:
        tau = re.search(r"constexpr\s+float\s+TAU\s*=\s*([0-9.]+)f?\s*;", f.read())
    assert ak and tau, "AK / TAU not found in the kernel sources"
    return int(ak.group(1)), float(tau.group(1))


def _bf16(x):
    return x.to(torch.bfloat16).to(torch.float32)


def make_case(name, N, seed=0):
    """(q', k, v): f32 [N, 64] tensors holding bf16-exact values."""
    g = torch.Generator().manual_seed(7919 * CASES.index(name) + 104729 * seed + N)

    def randn(*shape):
        return torch.randn(*shape, generator=g)

    k, v = _bf16(randn(N, DH)), _bf16(randn(N, DH))
    if name == "perm":
        k = torch.where(randn(N, DH) < 0, -1.0, 1.0)
        pi = torch.randperm(N, generator=g)
        return 0.5 * k[pi], k, v
    if name in ("gain6", "rand"):
        return _bf16(randn(N, DH) * (0.18 * 6 if name == "gain6" else 0.18)), k, v
    q = _bf16(randn(N, DH) * (0.18 if name == "shift96" else 0.05))
    q[:, 62:] = 0.0
    k[:, 62:] = 0.0
    j = torch.arange(N)
    if name.startswith("stair") or name == "down9":
        step = {"stair9": 9.0, "stair7": 7.0, "stair4": 4.0, "down9": -9.0}[name]
        q[:, 63] = 1.0
        k[:, 63] = step * (j // 64)
    elif name == "spike_last":
        q[:, 63] = 1.0
        k[N - 1, 63] = 40.0
    elif name == "spike_first":
        q[:, 63] = 1.0
        k[0, 63] = 40.0
    elif name == "spike_odd":
        q[1::2, 62] = 1.0
        k[N // 2, 62] = 20.0
        k[N - 1, 62] = 40.0
    elif name == "shift96":
        q[:, 63] = 1.0
        k[:, 63] = 96.0
    else:
        raise KeyError(name)
    for t in (q, k, v):
        assert torch.equal(t, _bf16(t)), name
    return q, k, v


def make_dout(N, seed=0):
    g = torch.Generator().manual_seed(15485863 + 31 * seed + N)
    return _bf16(torch.randn(N, DH, generator=g))


def pack_qkv(slots, B, N, H, dtype=torch.bfloat16):
    """[B*N, 3*H*64] as ivit_attn_* read it, slot z = b*H + h holding slots[z] = (q, k, v)."""
    assert len(slots) == B * H
    out = torch.zeros(B, N, 3, H, DH)
    for z, qkv in enumerate(slots):
        for i in range(3):
            out[z // H, :, i, z % H] = qkv[i]
    return out.reshape(B * N, 3 * H * DH).to(dtype)


def pack_rows(slots, B, N, H, dtype=torch.bfloat16):
    """[B*N, H*64] (the layout of o and dO) from one [N, 64] per slot."""
    out = torch.zeros(B, N, H, DH)
    for z, x in enumerate(slots):
        out[z // H, :, z % H] = x
    return out.reshape(B * N, H * DH).to(dtype)


def slot_rows(x, B, N, H, z):
    """Slot z of a [B*N, H*64] tensor -> f64 [N, 64]."""
    return x.reshape(B, N, H, DH)[z // H, :, z % H].double().cpu()


def slot_qkv(x, B, N, H, z):
    """Slot z of a [B*N, 3*H*64] tensor -> three f64 [N, 64]."""
    t = x.reshape(B, N, 3, H, DH)[z // H, :, :, z % H].double().cpu()
    return t[:, 0], t[:, 1], t[:, 2]


# ----------------------------------------------------------------------------- f64 references
def fwd_ref(q, k, v):
    """S' = q' k^T, lse2 = log2 sum 2^S', P = 2^(S' - lse2), o = P V, A = P |V| (all f64)."""
    q, k, v = q.double(), k.double(), v.double()
    S = q @ k.T
    mx = S.max(dim=1, keepdim=True).values
    e = torch.exp2(S - mx)
    l = e.sum(dim=1, keepdim=True)
    P = e / l
    return {"S": S, "lse2": (mx + torch.log2(l))[:, 0], "P": P, "o": P @ v, "A": P @ v.abs()}


def _ratio(err, bound):
    """max err / bound; an element with a zero bound must be exact."""
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    return float(r.max())


def fwd_ratios(o, lse, ref):
    """Forward bounds, elementwise:
      |o - o_ref| <= 2u A + u |o_ref|   (P rounded once to bf16, l summed from the same rounded P,
                                         the output rounding)
      |lse - lse_ref| <= u              (l carries at most u relative error; lse in natural-log
                                         units as the kernel returns it, lse_ref = ln2 * lse2)"""
    o, lse = o.double(), lse.double()
    return {"o": _ratio((o - ref["o"]).abs(), 2 * U * ref["A"] + U * ref["o"].abs()),
            "lse": _ratio((lse - ref["lse2"] * LN2).abs(), torch.full_like(lse, U))}


def bwd_ref(q, k, v, o, lse, dout):
    """The flash backward formula in f64 on the kernel's own inputs: q', k, v, the bf16 o and f32
    lse the forward returned, bf16 dO. Gradients are w.r.t. the unscaled q (q' = q * log2(e)/8), k, v:
      delta = rowsum(o * dO), dP = dO V^T, dS = P * (dP - delta), dV = P^T dO,
      dK = ln2 dS^T q', dQ = dS K / 8
    plus the elementwise bounds
      E  = u |dS| + 2^-16 |dS| + 2^-20 P * (|dO| |V|^T + rowsum(|o| * |dO|))
           (bf16 rounding of dS; the f32 error of the exponent S' - lse2 at |S'| <= 2^7; 16 f32 ulps
            for the 64-term f32 sums in dP - delta)
      |dV - ref| <= u P^T |dO| + u |ref|,  |dK - ref| <= ln2 E^T |q'| + u |ref|,
      |dQ - ref| <= E |k| / 8 + u |ref|"""
    q, k, v, o, lse, dout = (t.double() for t in (q, k, v, o, lse, dout))
    P = torch.exp2(q @ k.T - (lse / LN2)[:, None])
    delta = (o * dout).sum(dim=1, keepdim=True)
    dS = P * (dout @ v.T - delta)
    E = (U + 2.0 ** -16) * dS.abs() + 2.0 ** -20 * P * (dout.abs() @ v.abs().T
                                                        + (o.abs() * dout.abs()).sum(dim=1, keepdim=True))
    ref = {"dv": P.T @ dout, "dk": LN2 * dS.T @ q, "dq": dS @ k / 8.0}
    bound = {"dv": U * P.T @ dout.abs() + U * ref["dv"].abs(),
             "dk": LN2 * E.T @ q.abs() + U * ref["dk"].abs(),
             "dq": E @ k.abs() / 8.0 + U * ref["dq"].abs()}
    return ref, bound


def bwd_ratios(dq, dk, dv, ref, bound):
    got = {"dq": dq.double(), "dk": dk.double(), "dv": dv.double()}
    return {n: _ratio((got[n] - ref[n]).abs(), bound[n]) for n in ("dq", "dk", "dv")}


def assert_ratios(ratios, what):
    bad = {n: r for n, r in ratios.items() if not r <= 1.0}
    assert not bad, f"{what}: max err / bound {', '.join(f'{n} {r:.3g}' for n, r in ratios.items())}"


# ----------------------------------------------------------------------------- CPU model of the kernels
def lazy_max_trace(S, ak, tau):
    """The forward's running-maximum recurrence on scores S [rows, keys]: the maximum starts at tile
    0's row max and at step j >= 1 moves to tile j's row max where that exceeds it by more than tau.
    Returns (moved bool [steps, rows], pexp): pexp is the largest exponent any P = 2^(S' - m) is
    evaluated at (unrescaled)."""
    S = S.double()
    nt = (S.shape[1] + ak - 1) // ak
    m = S[:, :ak].max(dim=1).values
    moved, pexp = [], 0.0
    for j in range(1, nt):
        mt = S[:, j * ak:(j + 1) * ak].max(dim=1).values - m
        mv = mt > tau
        d = torch.where(mv, mt, torch.zeros_like(mt))
        m = m + d
        moved.append(mv)
        pexp = max(pexp, float((mt - d).max()))
    return (torch.stack(moved) if moved else torch.zeros(0, S.shape[0], dtype=torch.bool)), pexp


def flash_model(q, k, v, dout, ak, tau):
    """A faithful CPU model of the algorithm (not of the instruction schedule): key tiles of ak, the
    lazy maximum with tau, P rounded to bf16, f32 accumulation, bf16 outputs; the backward recomputes
    P from the f32 lse. Returns (o, lse, dq, dk, dv) with the kernel's output precisions."""
    f32 = torch.float32
    q, k, v, dout = (t.to(f32) for t in (q, k, v, dout))
    N = q.shape[0]
    nt = (N + ak - 1) // ak
    S = q @ k.T
    m = S[:, :ak].max(dim=1).values
    o = torch.zeros(N, DH, dtype=f32)
    l = torch.zeros(N, dtype=f32)
    for j in range(nt):
        sl = slice(j * ak, (j + 1) * ak)
        p = _bf16(torch.exp2(S[:, sl] - m[:, None]))
        o = o + p @ v[sl]
        l = l + p.sum(dim=1)
        if j + 1 < nt:
            mt = S[:, (j + 1) * ak:(j + 2) * ak].max(dim=1).values - m
            d = torch.where(mt > tau, mt, torch.zeros_like(mt))
            alpha = torch.exp2(-d)
            o, l, m = o * alpha[:, None], l * alpha, m + d
    o = _bf16(o * (1.0 / l)[:, None])
    lse = (m + torch.log2(l)) * f32_const(LN2)
    nlse2 = -(lse * f32_const(math.log2(math.e)))
    delta = (o * dout).sum(dim=1)
    P = torch.exp2(S + nlse2[:, None])
    dS = P * (dout @ v.T - delta[:, None])
    Pb, dSb = _bf16(P), _bf16(dS)
    dv = _bf16(Pb.T @ dout)
    dk = _bf16((dSb.T @ q) * f32_const(LN2))
    dq = _bf16((dSb @ k) * 0.125)
    return o, lse, dq, dk, dv


def f32_const(x):
    return torch.tensor(x, dtype=torch.float32)


# ----------------------------------------------------------------------------- f32 parity path
def f32_inputs(q, k, v):
    """The unscaled f32 inputs of the parity path: q = q' / c2 in f32."""
    return (q.to(torch.float32) / f32_const(C2)), k.to(torch.float32), v.to(torch.float32)


def f32_ref(q, k, v, dout):
    """f64 softmax attention (scores q k^T / 8) and its gradients on f32 inputs, with the abs-products
    the errors are measured against: A = P |V| for o; for the gradients the same sums with every
    factor replaced by its absolute value, G = P * (|dO| |V|^T + rowsum(|o| * |dO|)) bounding |dS|."""
    q, k, v, dout = (t.double() for t in (q, k, v, dout))
    P = torch.softmax(q @ k.T / 8.0, dim=1)
    o = P @ v
    dS = P * (dout @ v.T - (o * dout).sum(dim=1, keepdim=True))
    G = P * (dout.abs() @ v.abs().T + (o.abs() * dout.abs()).sum(dim=1, keepdim=True))
    ref = {"o": o, "dq": dS @ k / 8.0, "dk": dS.T @ q / 8.0, "dv": P.T @ dout}
    scale = {"o": P @ v.abs(), "dq": G @ k.abs() / 8.0, "dk": G.T @ q.abs() / 8.0, "dv": P.T @ dout.abs()}
    return ref, scale


def f32_metric(got, ref, scale):
    return {n: _ratio((got[n].double() - ref[n]).abs(), scale[n]) for n in ("o", "dq", "dk", "dv")}


def torch_sdpa_f32(q, k, v, dout):
    """torch's own f32 scaled_dot_product_attention on the CPU and its autograd gradients."""
    q, k, v = (t.detach().clone().to(torch.float32).requires_grad_(True) for t in (q, k, v))
    o = torch.nn.functional.scaled_dot_product_attention(q[None, None], k[None, None], v[None, None])[0, 0]
    o.backward(dout.to(torch.float32))
    return {"o": o.detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad}
