"""The linear-layer GEMMs op by op on inputs whose answer has no rounding (tests/gemm_cases.py): every f32
output must equal the f64 reference (torch.equal) and every bf16 output its round-to-nearest-even, bit
for bit, whatever tile, summation order or split the kernel takes. Operands are read as column slices of
wider buffers and outputs written into wider rows filled with NaN, which must be intact afterwards. The
only tolerances are the derived ones of the GELU / GELU' epilogues and of the fused LayerNorm
(gemm_cases' docstring).

Entry points and the tests that reach them (gemm_cases.coverage() lists the cases per edge):
  ivit_linear_fwd / _fwd_qs / _dgrad / _wgrad   test_engine_exact (f32 and bf16 engine, every epilogue
                         that is exact, accumulate 0 / 1, null dbias, empty and partial splits),
                         test_engine_gelu (EpiStore's GELU, EpiGeluGrad)
  ivit_linear_fwd_panel, _dgrad_gelu_panel, _dgrad_mul_panel   test_panel (every form, every value of
                         IVIT_KNOB_WIDE_EPI, both packs, rows that admit the transposed epilogue and not)
  ivit_linear_resid_ln_fwd, ivit_linear_dgrad_ln_bwd   test_resid_ln_fwd, test_dgrad_ln_bwd
  ivit_vit_block_wgrad   test_vit_block_wgrad_exact (token counts with splits that start past M)
  ivit_patch_weight_pack, ivit_weight_pack_t, ivit_weight_pack_multi   test_panel, test_pack_multi
"""
import functools

import pytest
import torch

import gemm_cases as GC
import norm_cases as NC

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32T, BF16T = torch.float32, torch.bfloat16
NAN = float("nan")


def _note(family, ratio):
    """Print a measured err / bound (pytest -s shows it; gemm_cases.RATIOS records a run)."""
    print(f"err / bound {family}: {ratio:.3g}")
    return ratio


def _out(rows, ld, dtype):
    """An output buffer [rows, ld] of NaN."""
    return torch.full((rows, ld), NAN, dtype=dtype, device=DEV)


def _ok(buf, cols, ref):
    """The first ``cols`` columns hold the reference exactly and the rest of every row is still NaN."""
    got = buf.detach().cpu()
    if got.dim() == 1:
        got = got[:, None]
    pad = got[:, cols:].float()
    return bool(torch.isnan(pad).all()) and GC.exact(got[:, :cols].contiguous(), ref.reshape(got.shape[0], cols))


def _pads_intact(buf, cols):
    return bool(torch.isnan(buf[:, cols:].float()).all()) and not bool(torch.isnan(buf[:, :cols].float()).any())


def _wide(t, dtype, pad=8, fill=77.0):
    """t as the first columns of a device buffer ``pad`` columns wider; -> (view, ld). The pad holds a
    finite value, so a kernel that read it would show."""
    rows, cols = t.shape
    buf = torch.full((rows, cols + pad), fill, dtype=dtype, device=DEV)
    buf[:, :cols] = t.to(dtype).to(DEV)
    return buf[:, :cols], cols + pad


def _nan_bytes(n, device=DEV):
    """A workspace whose every f32 is NaN: a slab the kernel did not write shows in the reduction."""
    return torch.full((max(int(n), 16),), 255, dtype=torch.uint8, device=device)


def _set_wide_epi(value, request):
    from _lib import KNOB_WIDE_EPI, lib
    lib.ivit_set_knob(KNOB_WIDE_EPI, int(value))
    request.addfinalizer(lambda: lib.ivit_set_knob(KNOB_WIDE_EPI, 0))


def _types(dtype):
    from _lib import BF16, F32
    return (BF16T, BF16, (F32T, BF16T)) if dtype == "bf16" else (F32T, F32, (F32T,))


# ----------------------------------------------------------------------------- engine
@pytest.mark.parametrize("name", sorted(GC.ENGINE))
def test_engine_exact(name):
    """ivit_linear_fwd (plain, bias, ReLU with the pre-activation copy, the residual form under every
    rows_per_scale and a null scale), ivit_linear_fwd_qs at every scale_cols, ivit_linear_dgrad (plain
    and times gelu'(0) = 1/2) and ivit_linear_wgrad (accumulate 0 and 1, null dbias, a workspace of NaN)
    of one case, on contiguous operands and on column slices of wider ones."""
    from _lib import ACT_NONE, ACT_RELU, dt, lib, ptr, stream
    c = GC.lin_case(name)
    cd, cdt, outs = _types(c.dtype)
    M, N, K = c.M, c.N, c.K
    st = stream()
    bad = []
    x, w, bias = c.x.to(cd).to(DEV), c.w.to(cd).to(DEV), c.bias.to(DEV)
    xw, ldxw = _wide(c.x, cd)
    resid, ldr = _wide(c.resid, F32T, pad=4)
    for od in outs:
        for xin, ldx, ldy, b, ref in ((x, K, N, bias, c.ref["y"]), (xw, ldxw, N + 4, bias, c.ref["y"]),
                                      (xw, ldxw, N + 5, None, c.ref["y0"])):
            y = _out(M, ldy, od)
            lib.ivit_linear_fwd(cdt, ptr(xin), ldx, ptr(w), ptr(b), M, N, K, ACT_NONE, ptr(y), ldy, dt(y), None, None, 0,
                                None, 0, st)
            if not _ok(y, N, ref):
                bad.append(f"fwd {od} ldx {ldx} ldy {ldy} bias {b is not None}")
        y, pre = _out(M, N + 4, od), _out(M, N + 4, od)
        lib.ivit_linear_fwd(cdt, ptr(xw), ldxw, ptr(w), ptr(bias), M, N, K, ACT_RELU, ptr(y), N + 4, dt(y), ptr(pre), None,
                            0, None, 0, st)
        if not (_ok(y, N, c.ref["y"].clamp_min(0.0)) and _ok(pre, N, c.ref["y"])):
            bad.append(f"fwd relu + Ypre {od}")
        for cols in GC.QS_COLS(N):
            y = _out(M, N + 4, od)
            lib.ivit_linear_fwd_qs(cdt, ptr(xw), ldxw, ptr(w), ptr(bias), M, N, K, ptr(y), N + 4, dt(y), cols, GC.QSCALE, st)
            if not _ok(y, N, GC.qs_ref(c, cols)):
                bad.append(f"qs {od} scale_cols {cols}")
    for rps in GC.RPS_OF(M) + (None,):
        scale = None if rps is None else GC.row_scale(M, rps)
        y, sd = _out(M, N + 4, F32T), None if scale is None else scale.to(DEV)
        lib.ivit_linear_fwd(cdt, ptr(xw), ldxw, ptr(w), ptr(bias), M, N, K, ACT_NONE, ptr(y), N + 4, dt(y), None,
                            ptr(resid), ldr, ptr(sd), rps or 1, st)
        if not _ok(y, N, GC.resid_ref(c, scale, rps or 1)):
            bad.append(f"resid rps {rps}")
    if N % 8 == 0:
        dy, dyw = c.dy.to(cd).to(DEV), c.dyw.to(cd).to(DEV)
        dyv, lddy = _wide(c.dy, cd)
        dywv, _ = _wide(c.dyw, cd)
        zero, ldz = _wide(torch.zeros(M, K), cd)
        for od in outs:
            for dyin, ld_in, lddx in ((dy, N, K), (dyv, lddy, K + 4)):
                dx = _out(M, lddx, od)
                lib.ivit_linear_dgrad(cdt, ptr(dyin), ld_in, ptr(w), M, N, K, ptr(dx), lddx, dt(dx), None, 0, st)
                if not _ok(dx, K, c.ref["dx"]):
                    bad.append(f"dgrad {od} lddy {ld_in} lddx {lddx}")
            dx = _out(M, K + 4, od)
            lib.ivit_linear_dgrad(cdt, ptr(dyv), lddy, ptr(w), M, N, K, ptr(dx), K + 4, dt(dx), ptr(zero), ldz, st)
            if not _ok(dx, K, c.ref["dx"] / 2):
                bad.append(f"dgrad x gelu'(0) {od}")
        nws = lib.ivit_linear_wgrad_workspace(M, N, K)
        for dyin, ld_in, xin, ldx in ((dyw, N, x, K), (dywv, lddy, xw, ldxw)):
            dW, db, ws = _out(N, K, F32T), _out(N, 1, F32T), _nan_bytes(nws)
            lib.ivit_linear_wgrad(cdt, ptr(dyin), ld_in, ptr(xin), ldx, M, N, K, ptr(dW), ptr(db), 0, ptr(ws), nws, st)
            if not (_ok(dW, K, c.ref["dw"]) and _ok(db, 1, c.ref["db"])):
                bad.append(f"wgrad lddy {ld_in} ldx {ldx}")
            dW, db, ws = c.dw0.to(DEV), c.db0.to(DEV), _nan_bytes(nws)
            lib.ivit_linear_wgrad(cdt, ptr(dyin), ld_in, ptr(xin), ldx, M, N, K, ptr(dW), ptr(db), 1, ptr(ws), nws, st)
            if not (GC.exact(dW, c.ref["dw"] + c.dw0.double()) and GC.exact(db, c.ref["db"] + c.db0.double())):
                bad.append(f"wgrad accumulate lddy {ld_in} ldx {ldx}")
        dW, ws = _out(N, K, F32T), _nan_bytes(nws)
        lib.ivit_linear_wgrad(cdt, ptr(dywv), lddy, ptr(xw), ldxw, M, N, K, ptr(dW), None, 0, ptr(ws), nws, st)
        if not _ok(dW, K, c.ref["dw"]):
            bad.append("wgrad null dbias")
        dW, ws = c.dw0.to(DEV), _nan_bytes(nws)
        lib.ivit_linear_wgrad(cdt, ptr(dywv), lddy, ptr(xw), ldxw, M, N, K, ptr(dW), None, 1, ptr(ws), nws, st)
        if not GC.exact(dW, c.ref["dw"] + c.dw0.double()):
            bad.append("wgrad accumulate, null dbias")
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", sorted(GC.ENGINE_GELU))
def test_engine_gelu(name):
    """EpiStore with ACT_GELU (the pre-activation copy exact, gelu(z) within the activation bound) and
    EpiGeluGrad (acc * gelu'(pre) within the bound scaled by the exact accumulator), f32 and bf16
    outputs, into wider rows."""
    from _lib import ACT_GELU, dt, lib, ptr, stream
    c = GC.gelu_case(name)
    cd, cdt, outs = _types(c.dtype)
    M, N, K = c.M, c.N, c.K
    st = stream()
    x, ldx = _wide(c.x, cd)
    w, bias = c.w.to(cd).to(DEV), c.bias.to(DEV)
    dy, lddy = _wide(c.dy, cd)
    w2 = c.w2.to(cd).to(DEV)
    pre_in, ldp = _wide(c.pre, cd)
    ratios = {}
    for od in outs:
        y, pre = _out(M, N + 4, od), _out(M, N + 4, od)
        lib.ivit_linear_fwd(cdt, ptr(x), ldx, ptr(w), ptr(bias), M, N, K, ACT_GELU, ptr(y), N + 4, dt(y), ptr(pre), None, 0,
                            None, 0, st)
        assert _ok(pre, N, c.z), (name, od, "Ypre")
        assert _pads_intact(y.cpu(), N), (name, od)
        ratios[f"gelu {od}"] = _note(f"engine {c.dtype} gelu -> {od}", GC.act_ratio(y.cpu()[:, :N], GC.gelu(c.z)))
        dx = _out(M, N + 4, od)   # dX[M, N] = dy[M, K] w2[K, N]: the ABI's reduction length is this case's K
        lib.ivit_linear_dgrad(cdt, ptr(dy), lddy, ptr(w2), M, K, N, ptr(dx), N + 4, dt(dx), ptr(pre_in), ldp, st)
        assert _pads_intact(dx.cpu(), N), (name, od)
        ref = c.acc * GC.gelu_grad(c.pre.double())
        ratios[f"gelu' {od}"] = _note(f"engine {c.dtype} acc gelu' -> {od}", GC.act_ratio(dx.cpu()[:, :N], ref, acc=c.acc))
    NC.assert_ratios(ratios, name)


# ----------------------------------------------------------------------------- row panel
def _pack(w):
    from _lib import lib, ptr, stream
    N, K = w.shape
    wp = torch.zeros(N * K, dtype=BF16T, device=DEV)
    assert lib.ivit_patch_weight_pack_bytes(N, K // 64) == 2 * N * K
    wd = w.float().contiguous().to(DEV)
    lib.ivit_patch_weight_pack(ptr(wd), N, K // 64, ptr(wp), stream())
    return wp


def _pack_t(wt):
    from _lib import lib, ptr, stream
    K, N = wt.shape
    wp = torch.zeros(N * K, dtype=BF16T, device=DEV)
    wd = wt.float().contiguous().to(DEV)
    lib.ivit_weight_pack_t(ptr(wd), K, N, ptr(wp), stream())
    return wp


@pytest.mark.parametrize("knob", GC.PANEL_KNOBS)
@pytest.mark.parametrize("name", sorted(GC.PANEL))
def test_panel(name, knob, request):
    """Every form of the wide row-panel kernels under one value of IVIT_KNOB_WIDE_EPI, with output rows
    of N + 4 (never 16-B aligned rows: the LDS-tile epilogue whatever the knob) and N + 8 (the transposed
    epilogue where the knob selects it): act NONE on both packs (bias, qcols in {0, 384, N}) bit exact,
    GELU with the exact pre-activation, GELU with GELU', the data gradient times gelu'(pre) and times a
    given G (exact)."""
    from _lib import ACT_GELU, ACT_GELU_D, ACT_NONE, lib, ptr, stream
    _set_wide_epi(knob, request)
    c = GC.panel_case(name)
    M, N, K = c.M, c.N, c.K
    st = stream()
    a, lda = _wide(c.a, BF16T)
    wp, wpt, wpg = _pack(c.w), _pack_t(c.wt), _pack(c.w / c.div)
    assert GC.same_bits(wp, GC.pack_ref(c.w)) and GC.same_bits(wpt, GC.pack_ref(c.w)), "packs"
    assert GC.same_bits(wpg, GC.pack_ref(c.w / c.div))
    bias, bias_g = c.bias.to(DEV), c.bias_g.to(DEV)
    bad, ratios = [], {}
    for pad in GC.PANEL_LDS:
        ld = N + pad
        for q in GC.QCOLS(N):
            y = _out(M, ld, BF16T)
            lib.ivit_linear_fwd_panel(ptr(a), lda, M, N, K, ptr(wp), ptr(bias), ACT_NONE, q, GC.QSCALE, ptr(y), ld, None, 0, st)
            if not _ok(y, N, GC.panel_none_ref(c, q)):
                bad.append(f"none qcols {q} ld {ld}")
        y = _out(M, ld, BF16T)   # ops.panel_dgrad: the transposed pack, no bias
        lib.ivit_linear_fwd_panel(ptr(a), lda, M, N, K, ptr(wpt), None, ACT_NONE, 0, 1.0, ptr(y), ld, None, 0, st)
        if not _ok(y, N, c.y0):
            bad.append(f"none_t ld {ld}")
        y, pre = _out(M, ld, BF16T), _out(M, ld, BF16T)
        lib.ivit_linear_fwd_panel(ptr(a), lda, M, N, K, ptr(wpg), ptr(bias_g), ACT_GELU, 0, 1.0, ptr(y), ld, ptr(pre), ld, st)
        if not (_ok(pre, N, c.z) and _pads_intact(y.cpu(), N)):
            bad.append(f"gelu Ypre / pads ld {ld}")
        ratios[f"gelu ld {ld}"] = GC.act_ratio(y.cpu()[:, :N], GC.gelu(c.z))
        y = _out(M, ld, BF16T)   # GELU without the copy
        lib.ivit_linear_fwd_panel(ptr(a), lda, M, N, K, ptr(wpg), ptr(bias_g), ACT_GELU, 0, 1.0, ptr(y), ld, None, 0, st)
        ratios[f"gelu, no Ypre, ld {ld}"] = GC.act_ratio(y.cpu()[:, :N], GC.gelu(c.z)) if _pads_intact(y.cpu(), N) else NAN
        y, g = _out(M, ld, BF16T), _out(M, ld, BF16T)
        lib.ivit_linear_fwd_panel(ptr(a), lda, M, N, K, ptr(wpg), ptr(bias_g), ACT_GELU_D, 0, 1.0, ptr(y), ld, ptr(g), ld, st)
        if not (_pads_intact(y.cpu(), N) and _pads_intact(g.cpu(), N)):
            bad.append(f"gelu_d pads ld {ld}")
        ratios[f"gelu_d y ld {ld}"] = GC.act_ratio(y.cpu()[:, :N], GC.gelu(c.z))
        ratios[f"gelu_d g ld {ld}"] = GC.act_ratio(g.cpu()[:, :N], GC.gelu_grad(c.z))
        pre_in, ldp = _wide(c.pre, BF16T, pad=pad)
        dx = _out(M, ld, BF16T)
        lib.ivit_linear_dgrad_gelu_panel(ptr(a), lda, M, N, K, ptr(wpt), ptr(pre_in), ldp, ptr(dx), ld, st)
        if not _pads_intact(dx.cpu(), N):
            bad.append(f"dgelu pads ld {ld}")
        ratios[f"dgelu ld {ld}"] = GC.act_ratio(dx.cpu()[:, :N], c.y0 * GC.gelu_grad(c.pre.double()), acc=c.y0)
        G, ldg = _wide(c.G, BF16T, pad=pad)
        dx = _out(M, ld, BF16T)
        lib.ivit_linear_dgrad_mul_panel(ptr(a), lda, M, N, K, ptr(wpt), ptr(G), ldg, ptr(dx), ld, st)
        if not _ok(dx, N, c.y0 * c.G.double()):
            bad.append(f"dmul ld {ld}")
    for n, r in ratios.items():
        _note(f"panel {n.split(' ld')[0].replace(',', '')}", r)
    assert not bad, (name, knob, bad)
    NC.assert_ratios(ratios, f"{name} knob {knob}")


# ----------------------------------------------------------------------------- fused GEMM + LayerNorm
@pytest.mark.parametrize("name", sorted(GC.FUSED_LN))
def test_resid_ln_fwd(name):
    """ivit_linear_resid_ln_fwd: X bit exact; Y, mean and rstd within norm_cases' LayerNorm bounds on that
    X; every buffer read or written with a wider leading dimension."""
    from _lib import lib, ptr, stream
    c = GC.resid_ln_case(name)
    M, N, K = c.M, c.N, c.K
    a, lda = _wide(c.a, BF16T)
    R, ldr = _wide(c.R, F32T, pad=4)
    X, Y = _out(M, N + 4, F32T), _out(M, N + 8, BF16T)
    mean, rstd = _out(M, 1, F32T), _out(M, 1, F32T)
    wp, bias, gamma, beta = _pack(c.w), c.bias.to(DEV), c.ln.gamma.to(DEV), c.ln.beta.to(DEV)
    scale = None if c.scale is None else c.scale.to(DEV)
    lib.ivit_linear_resid_ln_fwd(ptr(a), lda, M, N, K, ptr(wp), ptr(bias), ptr(R), ldr, ptr(scale), c.rps, ptr(gamma),
                                 ptr(beta), GC.LN_EPS, ptr(X), N + 4, ptr(Y), N + 8, ptr(mean), ptr(rstd), stream())
    assert _ok(X, N, c.X), name
    assert _pads_intact(Y.cpu(), N)
    ratios = NC.ln_ratios(c.ln, {"y": Y.cpu()[:, :N], "mean": mean.cpu()[:, 0], "rstd": rstd.cpu()[:, 0]})
    for n, r in ratios.items():
        _note(f"resid_ln_fwd {n}", r)
    NC.assert_ratios(ratios, name)


@pytest.mark.parametrize("name", sorted(GC.FUSED_LN))
def test_dgrad_ln_bwd(name):
    """ivit_linear_dgrad_ln_bwd: dX, dXs, dgamma and dbeta within norm_cases' backward bounds with
    dy := the exact product G; dX in place of dres or apart from it; dgamma / dbeta also accumulated."""
    from _lib import lib, ptr, stream
    d = GC.dgrad_ln_case(name)
    ln = d.ln
    M, N, K = d.M, d.N, d.K
    st = stream()
    dy, lddy = _wide(d.dy, BF16T)
    wpt = _pack_t(d.w)
    X, ldx = _wide(ln.X, F32T, pad=4)
    gamma = ln.gamma.to(DEV)
    mean, rstd = ln.ref["mean"].float().to(DEV), ln.ref["rstd"].float().to(DEV)
    scale = None if ln.row_scale is None else ln.row_scale.to(DEV)
    nws = lib.ivit_linear_dgrad_ln_bwd_workspace(M, N)

    def run(acc):
        dres = _out(M, N + 4, F32T)
        dres[:, :N] = ln.dres.to(DEV)
        dX, lddx = (dres, N + 4) if d.alias else (_out(M, N + 8, F32T), N + 8)
        dXs = _out(M, N, BF16T)
        if acc is None:
            dg, db = _out(N, 1, F32T), _out(N, 1, F32T)
        else:
            dg, db = acc["dgamma"].to(DEV)[:, None].contiguous(), acc["dbeta"].to(DEV)[:, None].contiguous()
        ws = _nan_bytes(nws)
        lib.ivit_linear_dgrad_ln_bwd(ptr(dy), lddy, M, N, K, ptr(wpt), ptr(X), ldx, ptr(gamma), ptr(mean), ptr(rstd),
                                     ptr(dres), N + 4, ptr(dX), lddx, ptr(dXs), ptr(scale), d.rps, ptr(dg), ptr(db),
                                     0 if acc is None else 1, ptr(ws), nws, st)
        assert _pads_intact(dX.cpu(), N), name
        if not d.alias:
            assert _ok(dres, N, ln.dres.double()), "dres changed"
        return NC.ln_ratios(ln, {"dx": dX.cpu()[:, :N], "dxs": dXs.cpu(), "dgamma": dg.cpu()[:, 0], "dbeta": db.cpu()[:, 0]},
                            acc=acc)

    ratios = run(None)
    g = torch.Generator().manual_seed(5)
    acc = {"dgamma": torch.randn(N, generator=g) * 100, "dbeta": torch.randn(N, generator=g) * 100}
    ratios.update({f"{n} (accumulated)": r for n, r in run(acc).items() if n in ("dgamma", "dbeta")})
    for n, r in ratios.items():
        _note(f"dgrad_ln_bwd {n}", r)
    NC.assert_ratios(ratios, name)


# ----------------------------------------------------------------------------- ivit_vit_block_wgrad
def _wb_call(M, Hd, ops):
    from _lib import lib, ptr, stream
    D = GC.WB_D
    outs = []
    for n, k in GC.wb_shapes(Hd):
        outs += [_out(n, k, F32T), _out(n, 1, F32T)]
    nws = lib.ivit_vit_block_wgrad_workspace(M, D, Hd)
    ws = _nan_bytes(nws)
    lib.ivit_vit_block_wgrad(M, D, Hd, *[ptr(t) for t in ops], *[ptr(t) for t in outs], ptr(ws), nws, stream())
    return outs


@functools.lru_cache(maxsize=None)
def _eights(Hd):
    M = GC.WB_RESIDUE_M
    return [torch.full((M, n), 8.0, dtype=BF16T, device=DEV) for s in GC.wb_shapes(Hd) for n in s]


@pytest.mark.parametrize("M", GC.WB_MS)
@pytest.mark.parametrize("Hd", GC.WB_HDS)
def test_vit_block_wgrad_exact(M, Hd):
    """All eight outputs of ivit_vit_block_wgrad bit-equal to f64 and two runs bitwise equal, on a
    workspace of NaN. A token count with splits that start past M (gemm_cases.wb_empty) runs after a
    call on all-8 operands, so that the workgroups' LDS holds non-zero residue: the bias sums of such
    a split must not pick it up."""
    c = GC.wb_case(M, Hd)
    if GC.wb_empty(M):
        R = GC.WB_RESIDUE_M
        outs = _wb_call(R, Hd, _eights(Hd))
        for q in range(4):
            assert bool((outs[2 * q] == 64.0 * R).all()) and bool((outs[2 * q + 1] == 8.0 * R).all()), (q, "residue call")
    ops = [t.to(BF16T).to(DEV) for t in c.ops]
    got, again = _wb_call(M, Hd, ops), _wb_call(M, Hd, ops)
    bad = []
    for q, (rw, rb) in enumerate(c.ref):
        if not _ok(got[2 * q], rw.shape[1], rw):
            bad.append(f"dW {q}")
        if not _ok(got[2 * q + 1], 1, rb):
            bad.append(f"db {q}")
        if not (GC.same_bits(got[2 * q], again[2 * q]) and GC.same_bits(got[2 * q + 1], again[2 * q + 1])):
            bad.append(f"run to run {q}")
    assert not bad, (M, Hd, GC.wb_empty(M), bad)


# ----------------------------------------------------------------------------- packs
def test_pack_multi():
    """One ivit_weight_pack_multi launch over plain and transposed jobs of different sizes returns the
    bytes of the single ivit_patch_weight_pack / ivit_weight_pack_t calls, which are the documented
    fragment order of the bf16-rounded weight."""
    from _lib import lib, ptr, stream
    ws = [w.to(DEV) for w in GC.pack_weights()]
    single = [(_pack_t if t else _pack)(w) for w, (_, _, t) in zip(ws, GC.PACK_JOBS)]
    multi = [torch.full((w.numel(),), NAN, dtype=BF16T, device=DEV) for w in ws]
    jobs = torch.tensor([[w.data_ptr(), o.data_ptr(), r, c, t] for w, o, (r, c, t) in zip(ws, multi, GC.PACK_JOBS)],
                        dtype=torch.int64).to(DEV)
    lib.ivit_weight_pack_multi(len(ws), ptr(jobs), max(r * c for r, c, _ in GC.PACK_JOBS), stream())
    torch.cuda.synchronize()
    for w, s, m, (r, c, t) in zip(ws, single, multi, GC.PACK_JOBS):
        assert GC.same_bits(s, m), (r, c, t)
        assert GC.same_bits(s, GC.pack_ref(w.cpu().T.contiguous() if t else w.cpu())), (r, c, t)
