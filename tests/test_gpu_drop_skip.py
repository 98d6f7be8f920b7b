"""The DropPath row skip: the *_skip entry points against the plain ones.

A sample whose branch factor is exactly 0 is not computed by the kernels of that branch — attention
workgroups return early, 144-row GEMM panels that lie wholly inside dropped samples skip their main
loop — and everything another kernel still reads of it is written as zeros. Every comparison here is
exact, ``(a == b).all()`` (which takes +0 and -0 as equal and fails on a NaN); there are no tolerances.
Output buffers start as NaN, so a row that a kernel should have written and did not shows.

  test_attention        ivit_attn_fwd_q2_skip / ivit_attn_bwd_q2_skip
  test_wide_panels      ivit_linear_fwd_panel_skip (Q-prescale, GELU + GELU', plain on the transposed
                        pack), ivit_linear_dgrad_mul_panel_skip, under IVIT_KNOB_WIDE_EPI 0 and 2
  test_ln_panels        ivit_linear_resid_ln_fwd_skip, ivit_linear_dgrad_ln_bwd_skip
  test_block            ops.ViTBlockPanelFn forward + backward, IVIT_KNOB_DROP_SKIP 0 against 1, the
                        second run on recycled NaN-filled memory
  test_model_step       a 64 x 96 bf16 train step of IntentNetViT, knob 0 against 1
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
KEEP = 1.0 / (1.0 - 0.1)  # timm DropPath's factor of a kept sample at p = 0.1
D = 384
PANEL = 144  # rows per workgroup of the row-panel kernels


def _eq(a, b):
    return bool((a == b).all())


def _nan(shape, dtype):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def _rand(shape, seed, dtype=torch.float32, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(DEV)


def _knob(request, knob, value, back):
    from _lib import lib
    lib.ivit_set_knob(knob, int(value))
    request.addfinalizer(lambda: lib.ivit_set_knob(knob, back))


# ----------------------------------------------------------------------------- attention
AB, AN, AH = 3, 257, 2
ATTN_SCALES = {"middle": [KEEP, 0.0, KEEP], "kept": [KEEP, KEEP, KEEP], "dropped": [0.0, 0.0, 0.0],
               "first": [0.0, KEEP, KEEP], "last": [KEEP, KEEP, 0.0]}


def _attn_run(qkv, dout, skip):
    """-> (out, lse, dqkv) of NaN-filled buffers through the q2 entries (skip None: the plain ones)."""
    from _lib import BF16, lib, ptr, stream
    out = _nan((AB * AN, AH * 64), torch.bfloat16)
    lse = _nan((AB, AH, AN), torch.float32)
    dqkv = _nan(tuple(qkv.shape), torch.bfloat16)
    ws = torch.full((int(lib.ivit_attn_workspace(BF16, AB, AN, AH, 64, 1)) + 16,), 255, dtype=torch.uint8, device=DEV)
    if skip is None:
        lib.ivit_attn_fwd_q2(ptr(qkv), AB, AN, AH, 64, ptr(out), ptr(lse), None, 0, stream())
        lib.ivit_attn_bwd_q2(ptr(qkv), ptr(out), ptr(dout), ptr(lse), AB, AN, AH, 64, ptr(dqkv), ptr(ws), ws.numel(),
                             stream())
    else:
        lib.ivit_attn_fwd_q2_skip(ptr(qkv), AB, AN, AH, 64, ptr(out), ptr(lse), None, 0, ptr(skip), stream())
        # the backward reads this run's own out / lse: a dropped sample's lse is still NaN here
        lib.ivit_attn_bwd_q2_skip(ptr(qkv), ptr(out), ptr(dout), ptr(lse), AB, AN, AH, 64, ptr(dqkv), ptr(ws),
                                  ws.numel(), ptr(skip), stream())
    torch.cuda.synchronize()
    return out, lse, dqkv


@functools.lru_cache(maxsize=None)
def _attn_ref():
    qkv = _rand((AB * AN, 3 * AH * 64), 11, torch.bfloat16)
    dout = _rand((AB * AN, AH * 64), 12, torch.bfloat16)
    return qkv, dout, _attn_run(qkv, dout, None)


@pytest.mark.parametrize("case", sorted(ATTN_SCALES))
def test_attention(case):
    """B = 3, N = 257 (three row tiles, the last ragged), H = 2: kept samples bit-equal to the plain entry
    (out, lse, dqkv); out and dqkv of dropped samples exactly zero, written over the NaN fill."""
    qkv, dout, (out0, lse0, dq0) = _attn_ref()
    sc = ATTN_SCALES[case]
    out, lse, dq = _attn_run(qkv, dout, torch.tensor(sc, dtype=torch.float32, device=DEV))
    v = lambda t: t.reshape(AB, AN, -1)
    for b in range(AB):
        if sc[b] == 0.0:
            assert _eq(v(out)[b], torch.zeros_like(v(out)[b])), (case, b, "out")
            assert _eq(v(dq)[b], torch.zeros_like(v(dq)[b])), (case, b, "dqkv")
        else:
            assert _eq(v(out)[b], v(out0)[b]), (case, b, "out")
            assert _eq(lse[b], lse0[b]), (case, b, "lse")
            assert _eq(v(dq)[b], v(dq0)[b]), (case, b, "dqkv")


def test_attention_knob_off(request):
    """IVIT_KNOB_DROP_SKIP 0: the skip entry ignores its pointer (every sample computed)."""
    from _lib import KNOB_DROP_SKIP
    _knob(request, KNOB_DROP_SKIP, 0, 1)
    qkv, dout, ref = _attn_ref()
    got = _attn_run(qkv, dout, torch.tensor(ATTN_SCALES["middle"], dtype=torch.float32, device=DEV))
    assert all(_eq(a, b) for a, b in zip(got, ref))


# ----------------------------------------------------------------------------- row panels
# rps 257: panel [288, 432) lies wholly inside the dropped sample 1, its neighbours straddle, the last
# panel is partial. rps 50: panel 0 spans three dropped samples (skipped), panel 1 touches the kept
# sample 3 (computed), the partial last panel [288, 400) is skipped.
SHAPES = {"rps257": (257, [KEEP, 0.0, KEEP, KEEP]), "rps50": (50, [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0])}


def _rows(shape):
    """-> (M, rps, scales tensor, dropped[M], skipped[M]): rows of dropped samples, rows of skipped panels."""
    rps, sc = SHAPES[shape]
    M = rps * len(sc)
    s = torch.tensor(sc, dtype=torch.float32)
    dropped = (s == 0.0).repeat_interleave(rps)
    skipped = torch.zeros(M, dtype=torch.bool)
    for m0 in range(0, M, PANEL):
        skipped[m0:m0 + PANEL] = bool(dropped[m0:m0 + PANEL].all())
    return M, rps, s.to(DEV), dropped.to(DEV), skipped.to(DEV)


def test_panel_geometry():
    """The shapes hold what the cases are meant to: a skipped interior panel, straddling neighbours, a
    partial last panel, a panel over three dropped samples."""
    M, _, _, dropped, skipped = _rows("rps257")
    assert M == 1028 and bool(skipped[288:432].all()) and int(skipped.sum()) == 144
    assert bool(dropped[257:288].all()) and not bool(skipped[257:288].any()) and M % PANEL != 0
    M, _, _, dropped, skipped = _rows("rps50")
    assert M == 400 and bool(skipped[:144].all()) and not bool(skipped[144:288].any()) and bool(skipped[288:].all())


@functools.lru_cache(maxsize=None)
def _weights():
    w = {"qkv": _rand((3 * D, D), 21, scale=0.05), "fc1": _rand((4 * D, D), 22, scale=0.05),
         "fc2": _rand((D, 4 * D), 23, scale=0.05), "proj": _rand((D, D), 24, scale=0.05),
         "bqkv": _rand((3 * D,), 25), "bfc1": _rand((4 * D,), 26), "bproj": _rand((D,), 27),
         "gamma": _rand((D,), 28) + 1.0, "beta": _rand((D,), 29)}
    return w


def _wide_run(form, x, g, skip, rps):
    """One wide-kernel form into NaN-filled outputs -> (Y, P or None); skip None: the plain entry."""
    import ops
    from _lib import ACT_GELU_D, ACT_NONE, lib, ptr, stream
    W = _weights()
    M = x.shape[0]
    if form == "qs":
        wp, b, N, act, qc, qs, want_p = ops.packed_weight(W["qkv"]), W["bqkv"], 3 * D, ACT_NONE, D, ops.Q2_SCALE, False
    elif form == "gelu_d":
        wp, b, N, act, qc, qs, want_p = ops.packed_weight(W["fc1"]), W["bfc1"], 4 * D, ACT_GELU_D, 0, 1.0, True
    elif form == "plain":
        wp, b, N, act, qc, qs, want_p = ops.packed_weight_t(W["proj"]), None, D, ACT_NONE, 0, 1.0, False
    else:
        assert form == "dmul"
        wp, N = ops.packed_weight_t(W["fc2"]), 4 * D
    y = _nan((M, N), torch.bfloat16)
    p = None
    if form == "dmul":
        if skip is None:
            lib.ivit_linear_dgrad_mul_panel(ptr(x), x.stride(0), M, N, D, ptr(wp), ptr(g), g.stride(0), ptr(y), N,
                                            stream())
        else:
            lib.ivit_linear_dgrad_mul_panel_skip(ptr(x), x.stride(0), M, N, D, ptr(wp), ptr(g), g.stride(0), ptr(y), N,
                                                 ptr(skip), rps, stream())
    else:
        p = _nan((M, N), torch.bfloat16) if want_p else None
        if skip is None:
            lib.ivit_linear_fwd_panel(ptr(x), x.stride(0), M, N, D, ptr(wp), ptr(b), act, qc, qs, ptr(y), N, ptr(p), N,
                                      stream())
        else:
            lib.ivit_linear_fwd_panel_skip(ptr(x), x.stride(0), M, N, D, ptr(wp), ptr(b), act, qc, qs, ptr(y), N,
                                           ptr(p), N, ptr(skip), rps, stream())
    torch.cuda.synchronize()
    return y, p


@pytest.mark.parametrize("epi", [0, 2])
@pytest.mark.parametrize("form", ["qs", "gelu_d", "dmul", "plain"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_wide_panels(shape, form, epi, request):
    """rowpanel_wide_kernel, both epilogue forms: rows outside the skipped panels bit-equal to the plain
    entry (the straddling panels included), rows of skipped panels exactly zero in Y and in the P that
    the GELU + GELU' form writes; nothing left NaN."""
    from _lib import KNOB_WIDE_EPI
    _knob(request, KNOB_WIDE_EPI, epi, 0)
    M, rps, s, _, skipped = _rows(shape)
    x = _rand((M, D), 31, torch.bfloat16)
    g = _rand((M, 4 * D), 32, torch.bfloat16) if form == "dmul" else None
    y0, p0 = _wide_run(form, x, g, None, rps)
    y, p = _wide_run(form, x, g, s, rps)
    for name, got, ref in (("Y", y, y0), ("P", p, p0)):
        if got is None:
            continue
        assert not bool(torch.isnan(ref.float()).any()), (name, "plain entry left NaN")
        assert _eq(got[~skipped], ref[~skipped]), (shape, form, epi, name, "kept rows")
        assert _eq(got[skipped], torch.zeros_like(got[skipped])), (shape, form, epi, name, "skipped rows")


def _ln_fwd_run(a, resid, s, rps, skip):
    from _lib import lib, ptr, stream
    import ops
    W = _weights()
    M = a.shape[0]
    x, y = _nan((M, D), torch.float32), _nan((M, D), torch.bfloat16)
    mean, rstd = _nan((M,), torch.float32), _nan((M,), torch.float32)
    args = (ptr(a), a.stride(0), M, D, D, ptr(ops.packed_weight(W["proj"])), ptr(W["bproj"]), ptr(resid), D, ptr(s),
            rps, ptr(W["gamma"]), ptr(W["beta"]), 1e-6, ptr(x), D, ptr(y), D, ptr(mean), ptr(rstd))
    if skip:
        lib.ivit_linear_resid_ln_fwd_skip(*args, ptr(s), stream())
    else:
        lib.ivit_linear_resid_ln_fwd(*args, stream())
    torch.cuda.synchronize()
    return x, y, mean, rstd


def _ln_bwd_run(dy, xin, mean, rstd, dres, out_scale, rps, skip):
    from _lib import lib, ptr, stream
    import ops
    W = _weights()
    M, K = dy.shape
    dx, dxs = _nan((M, D), torch.float32), _nan((M, D), torch.bfloat16)
    dg, db = _nan((D,), torch.float32), _nan((D,), torch.float32)
    ws = torch.full((int(lib.ivit_linear_dgrad_ln_bwd_workspace(M, D)) + 16,), 255, dtype=torch.uint8, device=DEV)
    args = (ptr(dy), dy.stride(0), M, D, K, ptr(ops.packed_weight_t(W["qkv"])), ptr(xin), D, ptr(W["gamma"]),
            ptr(mean), ptr(rstd), ptr(dres), D, ptr(dx), D, ptr(dxs), ptr(out_scale), rps, ptr(dg), ptr(db), 0,
            ptr(ws), ws.numel())
    if skip is None:
        lib.ivit_linear_dgrad_ln_bwd(*args, stream())
    else:
        lib.ivit_linear_dgrad_ln_bwd_skip(*args, ptr(skip), stream())
    torch.cuda.synchronize()
    return dx, dxs, dg, db


@pytest.mark.parametrize("form", ["ln_fwd", "ln_bwd"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_ln_panels(shape, form):
    """rowpanel_ln_kernel<false> / <true>: every output (X, Y, mean, rstd; dX, dXs, dgamma, dbeta) of the
    skip entry bit-equal to the plain entry run on the operand with the dropped samples' rows zeroed —
    what the branch's earlier kernels hand over. The skip entry's own operand holds a finite non-zero
    value in the rows of skipped panels instead, so a main loop that still read them would show."""
    M, rps, s, dropped, skipped = _rows(shape)
    K = D if form == "ln_fwd" else 3 * D
    a0 = _rand((M, K), 41, torch.bfloat16)
    a0[dropped] = 0.0
    a1 = a0.clone()
    a1[skipped] = 3.0
    resid = _rand((M, D), 42)
    if form == "ln_fwd":
        ref = _ln_fwd_run(a0, resid, s, rps, False)
        got = _ln_fwd_run(a1, resid, s, rps, True)
    else:
        xin = _rand((M, D), 43)
        mean = xin.mean(1).contiguous()
        rstd = (xin.var(1, unbiased=False) + 1e-6).rsqrt().contiguous()
        # the output factor of dXs is another branch's: it has nothing to do with the skip
        out_scale = torch.tensor([0.0, KEEP] * (s.numel() // 2), dtype=torch.float32, device=DEV)
        ref = _ln_bwd_run(a0, xin, mean, rstd, resid, out_scale, rps, None)
        got = _ln_bwd_run(a1, xin, mean, rstd, resid, out_scale, rps, s)
    for i, (g_, r_) in enumerate(zip(got, ref)):
        assert not bool(torch.isnan(r_.float()).any()), (shape, form, i, "plain entry left NaN")
        assert _eq(g_, r_), (shape, form, i)


# ----------------------------------------------------------------------------- block
def _block_run(scales, poison):
    """One vit.Block (row-panel path) forward + backward at B = 3, N = 257 with injected DropPath factors
    -> x2, the next block's handed-over norm outputs, dx0, the twelve parameter gradients. poison: first
    fill and free large NaN tensors, so torch.empty hands the block NaN-filled memory."""
    import vit
    from _lib import BF16
    B, N = 3, 257
    torch.manual_seed(5)
    blk = vit.Block(D, 6, 4.0, 0.1).to(DEV).train()
    nxt = vit.LayerNorm(D, eps=1e-6).to(DEV)
    with torch.no_grad():
        for i, (name, p) in enumerate(list(blk.named_parameters()) + list(nxt.named_parameters())):
            p.copy_(_rand(tuple(p.shape), 50 + i, scale=0.05))
            if p.dim() == 1 and name.endswith("weight"):  # the LayerNorm gains around 1
                p.add_(1.0)
    blk.drop_path_scales = scales
    x = _rand((B * N, D), 70).requires_grad_(True)
    gy = _rand((B * N, D), 71)
    if poison:
        junk = [_nan((B * N, 4 * D), torch.float32) for _ in range(12)]
        del junk
    x2, (lnx, mx, rx) = blk.forward_flat(x, B, N, BF16, next_norm=nxt)
    x2.backward(gy)
    torch.cuda.synchronize()
    outs = [x2.detach(), lnx, mx, rx, x.grad] + [p.grad for p in blk.parameters()]
    assert len(outs) == 5 + 12
    return [o.clone() for o in outs]


@pytest.mark.parametrize("which", ["attn", "mlp", "both"])
def test_block(which, request):
    """ops.ViTBlockPanelFn, zeros in either branch's factors: x2, the handed-over norm outputs, dx0 and
    all twelve parameter gradients equal between IVIT_KNOB_DROP_SKIP 0 and 1, finite, with the knob-1
    run on recycled NaN-filled memory (an unwritten row that is still read would turn up as NaN)."""
    from _lib import KNOB_DROP_SKIP
    k, z = KEEP, 0.0
    scales = {"attn": ([k, z, k], [k, k, k]), "mlp": ([k, k, k], [z, k, z]), "both": ([z, z, k], [k, z, z])}[which]
    _knob(request, KNOB_DROP_SKIP, 0, 1)
    ref = _block_run(scales, False)
    _knob(request, KNOB_DROP_SKIP, 1, 1)
    got = _block_run(scales, True)
    for i, (g_, r_) in enumerate(zip(got, ref)):
        assert bool(torch.isfinite(g_.float()).all()), (which, i, "not finite")
        assert _eq(g_, r_), (which, i)


# ----------------------------------------------------------------------------- model
def _dp_scales(B, depth=12, rate=0.1, seed=0):
    """Per-block (attn_scale[B], mlp_scale[B]) in {0, 1/(1-p_i)}, p_i = linspace(0, rate, depth)[i]; block
    0 (p = 0) is the identity; each block from 1 on drops at least one (sample, branch) unit."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, p in enumerate(torch.linspace(0, rate, depth).tolist()):
        if p <= 0.0:
            out.append((torch.ones(B), torch.ones(B)))
            continue
        keep = (torch.rand((2, B), generator=g) > 0.3).float()
        keep[i % 2, (i // 2) % B] = 0.0
        s = keep / (1.0 - p)
        out.append((s[0], s[1]))
    return out


def _model_step():
    import loss as L
    import model_vit
    import utils
    from oracle import ivit_oracle as O
    from oracle.weights import make_state_dict, model_cfg
    H, W, B = 64, 96, 3
    cfg = model_cfg(img_size=(H, W))
    m = model_vit.IntentNetViT(backbone_cfg={"img_size": (H, W), "drop_path_rate_lidar": 0.1,
                                             "drop_path_rate_map": 0.1})
    m.load_state_dict(make_state_dict(cfg, seed=0), strict=True)
    m = m.to(DEV).set_compute_dtype(torch.bfloat16).train()
    m.backbone.vit_lidar.set_drop_path_scales(_dp_scales(B, seed=7))
    m.backbone.vit_map.set_drop_path_scales(_dp_scales(B, seed=8))
    lidar, mp, gts = O.synthetic_batch(B, (H, W), seed=3, grid_scale=H / 400.0)
    anchors = utils.generate_anchors(H, W, 8, device=DEV)
    keep = (torch.rand((B, anchors.shape[0]), generator=torch.Generator().manual_seed(3)) < 0.15).float()
    c, b, i = m(lidar.to(DEV), mp.to(DEV))
    d = L.DetectionIntentionLoss()(c, b, i, anchors, gts, intent_keep=keep)
    d["loss"].backward()
    torch.cuda.synchronize()
    return d["loss"].detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()}


def test_model_step(request):
    """A 64 x 96 bf16 train step of IntentNetViT (N = 97 tokens: panels over up to three samples) with
    injected DropPath factors: the loss and every parameter gradient equal for knob 0 and knob 1."""
    from _lib import KNOB_DROP_SKIP
    _knob(request, KNOB_DROP_SKIP, 0, 1)
    loss0, g0 = _model_step()
    _knob(request, KNOB_DROP_SKIP, 1, 1)
    loss1, g1 = _model_step()
    assert bool(torch.isfinite(loss1)) and _eq(loss0, loss1), (float(loss0), float(loss1))
    assert sorted(g0) == sorted(g1)
    bad = [k for k in g0 if not (bool(torch.isfinite(g1[k]).all()) and _eq(g0[k], g1[k]))]
    assert not bad, bad
