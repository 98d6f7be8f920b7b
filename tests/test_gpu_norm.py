"""The LayerNorm and BatchNorm kernels of csrc/norm.hip, op by op, against the f64 references and the
derived bounds of tests/norm_cases.py (max err / bound <= 1 everywhere; no tolerance is set here).

Dispatch branches and the tests that reach them:
  ivit_layernorm_fwd / _bwd  ln_fwd_vec_kernel / ln_bwd_vec_kernel NC = 1, 2, 3, 4 (D = 128, 256, 384, 512) and the
                             one-wave-per-row ln_fwd_kernel / ln_bwd_kernel (D = 64, 192, 448: widths 1, 3, 7):
                             test_layernorm_grid; the fallback forced at D = 384 by a misaligned X, a row
                             stride of 385 and a misaligned dY: test_layernorm_forced_fallback; TY / TS
                             instantiations: test_layernorm_bwd_operand_combinations
  launch_bn_partial          bn_partial8_kernel (C % 8 == 0, two column blocks at C = 520) and bn_partial_kernel
                             (C = 35): test_batchnorm_train; the unaligned branch of load8f:
                             test_batchnorm_8wide_and_scalar_kernels_agree_bitwise
  ivit_bn_apply / ivit_bn_bwd  bn_apply8_kernel / bn_bwd_apply8_kernel and the scalar bn_apply_kernel /
                             bn_bwd_apply_kernel (C = 35, or a misaligned operand): the same two tests
"""
import functools
import itertools

import pytest
import torch

import norm_cases as NC

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = NC.kernel_constants()
MS = NC.ln_ms()
SENTINEL = -777.25
F32, BF16T = torch.float32, torch.bfloat16


@functools.lru_cache(maxsize=None)
def _ln(family, M, D, eps, dy_bf16=False, with_dres=True):
    """Built once per case, shared and left unchanged."""
    return NC.ln_case(family, M, D, eps, dy_bf16=dy_bf16, with_dres=with_dres)


@functools.lru_cache(maxsize=None)
def _neck(family, D):
    return NC.ln_case(family, NC.NECK_B * NC.NECK_NP, D, 1e-5, rowmap=NC.NECK_MAP, row_scale=NC.NECK_SCALE,
                      rps=NC.NECK_NP)


@functools.lru_cache(maxsize=None)
def _bn(M, C, kind, relu, resid, momentum=0.1):
    return NC.bn_case(M, C, kind, relu, resid, momentum)


def _d(t, dtype=F32):
    return None if t is None else t.to(dtype).to(DEV)


def _off(t, dtype=F32):
    """t on the device at a 4-byte offset into a larger buffer (allocations are 256-B aligned)."""
    if t is None:
        return None
    k = 4 // torch.empty((), dtype=dtype).element_size()
    buf = torch.empty(t.numel() + 8, dtype=dtype, device=DEV)
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t.to(dtype))
    assert v.data_ptr() % 16 == 4
    return v


def _wide_rows(t, ld):
    """t [M, D] as a view with row stride ld of a wider buffer."""
    buf = torch.full((t.shape[0], ld), SENTINEL, dtype=F32, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf[:, :t.shape[1]]


def _ln_run(case, out_dtype=F32, xs_dtype=F32, dres="separate", x=None, dy=None, dx=None, dy_dtype=F32):
    """Forward and backward through ops.layernorm_fwd / _bwd; returns the outputs by name."""
    import ops
    x = _d(case.X) if x is None else x
    g, b = _d(case.gamma), _d(case.beta)
    y, mean, rstd = ops.layernorm_fwd(x, g, b, case.eps, out_dtype, rowmap=case.rowmap, M=case.M)
    dy = _d(case.dy, dy_dtype) if dy is None else dy
    dr = None
    if dres == "separate":
        dr = _d(case.dres) if dx is None or dx.is_contiguous() else _wide_rows(case.dres, dx.stride(0))
        dx = torch.full(case.X.shape, SENTINEL, dtype=F32, device=DEV) if dx is None else dx
    elif dres == "inplace":  # the wrapper's default: dx is dres
        assert dx is None
        dr = _d(case.dres).clone()
    elif dx is None:
        dx = torch.full(case.X.shape, SENTINEL, dtype=F32, device=DEV)
    dx, dxs, dg, db = ops.layernorm_bwd(x, g, mean, rstd, dy, dres=dr, dx=dx, xs_dtype=xs_dtype,
                                        row_scale=_d(case.row_scale), rps=case.rps, rowmap=case.rowmap)
    torch.cuda.synchronize()
    return {"y": y, "mean": mean, "rstd": rstd, "dx": dx, "dxs": dxs, "dgamma": dg, "dbeta": db}


def _judge_ln(case, got, what):
    r = NC.ln_ratios(case, got)
    print(f"ln {what}: " + " ".join(f"{n} {v:.3f}" for n, v in r.items())
          + " | tol " + " ".join(f"{n} {v:.1e}" for n, v in case.tol.items()))
    NC.assert_ratios(r, what)


# ----------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("family", NC.LN_FAMILIES)
@pytest.mark.parametrize("D", NC.LN_DS)
def test_layernorm_grid(D, family):
    """ivit_layernorm_fwd / _bwd at M in {1, R-1, R+1, 2R+6} (R rows per block), eps 1e-6 and 1e-5, f32
    and bf16 outputs: ln_fwd_vec_kernel / ln_bwd_vec_kernel<NC = D / 128> for D % 128 == 0, the
    one-wave-per-row ln_fwd_kernel / ln_bwd_kernel for D = 64, 192, 448 (1, 3, 7 values per lane).

    Measured on an MI355X, worst max err / bound over all LayerNorm tests of this file: f32 y 0.33,
    mean 0.07, rstd 0.07, dx and dxs 0.17, dgamma 0.18, dbeta 0.01 (tolerances 2.0e-6 .. 6.1e-6 for y,
    .. 3.5e-6 for dx); bf16 y and dxs 0.995 (the half ulp of the rounding is the bound's first term)."""
    for M in MS:
        for eps in (1e-6, 1e-5):
            case = _ln(family, M, D, eps)
            for od in (F32, BF16T):
                _judge_ln(case, _ln_run(case, out_dtype=od, xs_dtype=od), f"{family} M={M} D={D} eps={eps} {od}")


@pytest.mark.parametrize("D", [576, 96])
def test_layernorm_bad_width_is_an_argument_error_and_launches_nothing(D):
    from _lib import F32 as CF32, lib, ptr, stream
    M = 4
    x = torch.randn(M, D, device=DEV)
    g = torch.ones(D, device=DEV)
    outs = [torch.full((M, D), SENTINEL, device=DEV) for _ in range(3)]
    vecs = [torch.full((max(M, D),), SENTINEL, device=DEV) for _ in range(4)]
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        lib.ivit_layernorm_fwd(ptr(x), D, 0, 0, 0, M, D, ptr(g), ptr(g), 1e-6, ptr(outs[0]), D, CF32, ptr(vecs[0]),
                               ptr(vecs[1]), stream())
    with pytest.raises(RuntimeError, match="multiple of 64"):
        lib.ivit_layernorm_bwd(ptr(x), D, 0, 0, 0, M, D, ptr(g), ptr(g), ptr(g), ptr(x), D, CF32, None, ptr(outs[1]), D,
                               ptr(outs[2]), CF32, None, 1, ptr(vecs[2]), ptr(vecs[3]), 0, ptr(ws), ws.numel(), stream())
    torch.cuda.synchronize()
    for t in outs + vecs:
        assert bool((t == SENTINEL).all())


@pytest.mark.parametrize("way", ["x_offset", "x_stride_385", "dy_offset"])
def test_layernorm_forced_fallback(way):
    """D = 384 takes the vector kernels when aligned (test_layernorm_grid); a 4-byte-offset X, a row
    stride of 385 and a 4-byte-offset dY each send it to ln_fwd_kernel / ln_bwd_kernel (dY: the
    backward only). Same reference and bounds as the aligned run."""
    case = _ln("plain", MS[3], 384, 1e-6)
    kw = {}
    dx_buf = torch.full((case.M, 385), SENTINEL, device=DEV)
    if way == "x_offset":
        kw["x"] = _off(case.X)
    elif way == "x_stride_385":
        kw["x"] = _wide_rows(case.X, 385)
        kw["dx"] = dx_buf[:, :384]
    else:
        kw["dy"] = _off(case.dy)
    for od in (F32, BF16T):
        got = _ln_run(case, out_dtype=od, xs_dtype=od, **kw)
        _judge_ln(case, got, f"fallback {way} {od}")
    if way == "x_stride_385":  # dx went into the 385-wide buffer, and its pad column is not written
        assert got["dx"].data_ptr() == dx_buf.data_ptr()
        assert bool((dx_buf[:, 384] == SENTINEL).all())


@pytest.mark.parametrize("D", [128, 384, 192])
@pytest.mark.parametrize("family", ["plain", "wide"])
def test_layernorm_neck_row_map(D, family):
    """The row map (Np, Np + 1, 1) with B = 3, Np = 23 (X has 72 rows, M = 69) on the vector (D = 128,
    384) and the fallback (D = 192) kernels, with row_scale = (0, 0.5, 2) per sample: y, mean, rstd and
    dXs are indexed by the logical row, X, dres and dX by the mapped one; the three CLS rows of a
    sentinel-filled dX come back bit-identical; dXs of the zero-scaled sample is exactly 0 and dX is
    not scaled."""
    case = _neck(family, D)
    for od in (F32, BF16T):
        got = _ln_run(case, out_dtype=od, xs_dtype=od)
        _judge_ln(case, got, f"neck {family} D={D} {od}")
        cls_rows = torch.arange(NC.NECK_B) * (NC.NECK_NP + 1)
        assert bool((got["dx"].cpu()[cls_rows] == SENTINEL).all())
        assert got["y"].shape[0] == got["mean"].shape[0] == got["dxs"].shape[0] == case.M
        assert bool((got["dxs"][:NC.NECK_NP] == 0).all())
        assert bool((got["dx"].cpu()[case.idx[:NC.NECK_NP]] != 0).any())


@pytest.mark.parametrize("D", [256, 192])
@pytest.mark.parametrize("dy_dtype", [F32, BF16T])
def test_layernorm_bwd_operand_combinations(D, dy_dtype):
    """dres in {None, dx itself (in place), a separate tensor} x dXs in {None, f32, bf16} x dY in {f32,
    bf16}: every <TY, TS> instantiation of ln_bwd_vec_kernel (D = 256) and the runtime dtype codes of
    ln_bwd_kernel (D = 192)."""
    for dres in (None, "inplace", "separate"):
        case = _ln("plain", MS[3], D, 1e-6, dy_bf16=dy_dtype == BF16T, with_dres=dres is not None)
        for xs in (None, F32, BF16T):
            got = _ln_run(case, xs_dtype=xs, dres=dres, dy_dtype=dy_dtype)
            assert (got["dxs"] is None) == (xs is None)
            _judge_ln(case, got, f"bwd D={D} dy={dy_dtype} dres={dres} dxs={xs}")


@pytest.mark.parametrize("D", [128, 448])
def test_layernorm_bwd_accumulate(D):
    """accumulate = 1 adds to pre-filled dgamma / dbeta; accumulate = 0 overwrites a NaN pre-fill."""
    import ops
    from _lib import F32 as CF32, lib, ptr, stream, workspace
    case = _ln("plain", MS[3], D, 1e-6)
    M = case.M
    x, g, b, dy = _d(case.X), _d(case.gamma), _d(case.beta), _d(case.dy)
    _, mean, rstd = ops.layernorm_fwd(x, g, b, case.eps, F32)
    gen = torch.Generator().manual_seed(5)
    pre = {"dgamma": torch.randn(D, generator=gen), "dbeta": torch.randn(D, generator=gen)}
    for acc in (1, 0):
        dg = _d(pre["dgamma"]) if acc else torch.full((D,), float("nan"), device=DEV)
        db = _d(pre["dbeta"]) if acc else torch.full((D,), float("nan"), device=DEV)
        dx = torch.empty(M, D, device=DEV)
        ws = workspace(lib.ivit_layernorm_bwd_workspace(M, D), DEV)
        lib.ivit_layernorm_bwd(ptr(x), D, 0, 0, 0, M, D, ptr(g), ptr(mean), ptr(rstd), ptr(dy), D, CF32, None, ptr(dx), D,
                               None, CF32, None, 1, ptr(dg), ptr(db), acc, ptr(ws), ws.numel(), stream())
        torch.cuda.synchronize()
        assert bool(torch.isfinite(dg).all()) and bool(torch.isfinite(db).all())
        r = NC.ln_ratios(case, {"dgamma": dg, "dbeta": db}, acc=pre if acc else None)
        print(f"ln accumulate={acc} D={D}: {r}")
        NC.assert_ratios(r, f"accumulate={acc}")


def test_layernorm_long_partial_list():
    """M = R (16 CR_COLS + 1) + 5 row blocks' partials: colreduce_kernel's phases go round their batch
    of 16 loads a second time."""
    M = NC.ln_long_m()
    case = _ln("plain", M, 128, 1e-6)
    assert -(-M // K["LN_ROWS"]) > 16 * K["CR_COLS"]
    _judge_ln(case, _ln_run(case), f"long M={M}")


@pytest.mark.parametrize("D", [384, 448])
def test_layernorm_is_deterministic(D):
    """The file header's promise: two runs on the same input give the same bits, every output."""
    case = _ln("plain", MS[3], D, 1e-6)
    a, b = _ln_run(case, xs_dtype=BF16T), _ln_run(case, xs_dtype=BF16T)
    for n in a:
        assert torch.equal(a[n], b[n]), n


# ----------------------------------------------------------------------------- BatchNorm
def _bn_dtypes(kind):
    """x, y (= residual, dy), dx (= dr)."""
    return {"f32": (F32, F32, F32), "bf16": (BF16T, BF16T, BF16T), "mixed": (F32, BF16T, F32)}[kind]


def _bn_run(case, want_dr=True, put=_d):
    import ops
    xd, yd, dxd = _bn_dtypes(case.kind)
    x, g, b = put(case.x, xd), put(case.gamma), put(case.beta)
    rm, rv = _d(case.rm).clone(), _d(case.rv).clone()
    st = ops.bn_forward(x, g, b, rm, rv, True, momentum=case.momentum, eps=case.eps)
    y = ops.bn_apply(x, st, g, b, yd, resid=put(case.res, yd), relu=case.relu)
    ym = y if put is _d else put(y, yd)
    dx, dr, dg, db = ops.bn_backward(x, ym, put(case.dy, yd), st, g, case.relu, dxd, want_dr=want_dr)
    torch.cuda.synchronize()
    return {"mean": st.mean, "invstd": st.invstd, "y": y, "rm": rm, "rv": rv, "dx": dx, "dr": dr, "dg": dg, "db": db}


@pytest.mark.parametrize("kind", NC.BN_KINDS)
@pytest.mark.parametrize("M,C", NC.bn_shapes())
def test_batchnorm_train(M, C, kind):
    """ivit_bn_stats / ivit_bn_apply / ivit_bn_bwd with relu and the residual on and off, dr wanted or
    not, momentum 0.1 and 0.3. C = 35 takes bn_partial_kernel, bn_apply_kernel and bn_bwd_apply_kernel;
    the others bn_partial8_kernel (two column blocks at C = 520), bn_apply8_kernel and
    bn_bwd_apply8_kernel, with the BN8_R row tail at odd M; M = 32 * 8 * BN_PH + 19 takes bn_colsum past
    its first batch of partials. The running stats are the reference's (unbiased variance).

    Measured on an MI355X, worst max err / bound: f32 y 0.09, mean 0.11, invstd 0.03, running mean 0.05,
    running var 0.08, dx 0.09, dg 0.02, db 0.01, dr exact (every tolerance at the 2e-6 floor); bf16 y
    and dx 0.994."""
    for relu, resid, want_dr, momentum in itertools.product((False, True), (False, True), (False, True), (0.1, 0.3)):
        case = _bn(M, C, kind, relu, resid, momentum)
        assert case.left_out <= NC.MASK_CAP
        got = _bn_run(case, want_dr)
        assert (got["dr"] is None) == (not want_dr)
        r = NC.bn_ratios(case, got)
        what = f"bn ({M},{C}) {kind} relu={relu} resid={resid} dr={want_dr} momentum={momentum}"
        print(what + ": " + " ".join(f"{n} {v:.3f}" for n, v in r.items())
              + " | tol " + " ".join(f"{n} {v:.1e}" for n, v in case.tol.items()))
        NC.assert_ratios(r, what)


@pytest.mark.parametrize("kind", NC.BN_KINDS)
@pytest.mark.parametrize("M,C", NC.bn_shapes()[:4])
def test_batchnorm_eval(M, C, kind):
    """ivit_bn_eval_stats then ivit_bn_apply against F.batch_norm(training=False)'s formula in f64, at
    running variances 1e-8 (eps dominates), 1 and 1e4."""
    import ops
    xd, yd, _ = _bn_dtypes(kind)
    for rvar in (1e-8, 1.0, 1e4):
        for relu, resid in ((True, True), (False, False)):
            case = NC.bn_eval_case(M, C, kind, relu, resid, rvar)
            x, g, b, rm, rv = _d(case.x, xd), _d(case.gamma), _d(case.beta), _d(case.rm), _d(case.rv)
            st = ops.bn_forward(x, g, b, rm, rv, False, eps=case.eps)
            y = ops.bn_apply(x, st, g, b, yd, resid=_d(case.res, yd), relu=relu)
            assert torch.equal(rm.cpu(), case.rm) and torch.equal(rv.cpu(), case.rv)  # eval leaves them alone
            r = {n: NC.value_ratio(t, case.ref[n], case.tol[n], case.scale[n])
                 for n, t in (("mean", st.mean), ("invstd", st.invstd), ("y", y))}
            print(f"bn eval ({M},{C}) {kind} rvar={rvar} relu={relu}: {r}")
            NC.assert_ratios(r, f"eval rvar={rvar}")


@pytest.mark.parametrize("kind", NC.BN_KINDS)
def test_batchnorm_8wide_and_scalar_kernels_agree_bitwise(kind):
    """The source comments' promise at C = 96: bn_apply8_kernel / bn_bwd_apply8_kernel (aligned run) give
    the bits of bn_apply_kernel / bn_bwd_apply_kernel (every operand at a 4-byte offset), and the
    aligned and the unaligned branch of load8f inside bn_partial8_kernel sum alike: mean, invstd, y, dx,
    dr, dg, db are torch.equal, with relu and the residual each on and off."""
    for relu, resid in itertools.product((True, False), repeat=2):
        case = _bn(33, 96, kind, relu, resid)
        a, b = _bn_run(case), _bn_run(case, put=_off)
        for n in ("mean", "invstd", "y", "dx", "dr", "dg", "db"):
            assert torch.equal(a[n], b[n]), (n, relu, resid)
        NC.assert_ratios(NC.bn_ratios(case, b), f"offset run {kind} relu={relu} resid={resid}")


@pytest.mark.parametrize("C", [35, 96])
def test_batchnorm_bwd_accumulate(C):
    """accumulate = 1 adds to pre-filled dg / db (scalar and 8-wide kernels); 0 overwrites NaN."""
    import ops
    from _lib import F32 as CF32, lib, ptr, stream, workspace
    case = _bn(33, C, "f32", True, True)
    M = case.M
    x, g, b, dy = _d(case.x), _d(case.gamma), _d(case.beta), _d(case.dy)
    st = ops.bn_forward(x, g, b, None, None, True)
    y = ops.bn_apply(x, st, g, b, F32, resid=_d(case.res), relu=True)
    gen = torch.Generator().manual_seed(6)
    pre = {"dg": torch.randn(C, generator=gen), "db": torch.randn(C, generator=gen)}
    for acc in (1, 0):
        dg = _d(pre["dg"]) if acc else torch.full((C,), float("nan"), device=DEV)
        db = _d(pre["db"]) if acc else torch.full((C,), float("nan"), device=DEV)
        dx = torch.empty(M, C, device=DEV)
        ws = workspace(lib.ivit_bn_workspace(M, C), DEV)
        lib.ivit_bn_bwd(ptr(x), CF32, ptr(y), CF32, ptr(dy), CF32, M, C, ptr(st.mean), ptr(st.invstd), ptr(g), 1, ptr(dx),
                        CF32, None, ptr(dg), ptr(db), acc, ptr(ws), ws.numel(), stream())
        torch.cuda.synchronize()
        r = NC.bn_ratios(case, {"dx": dx, "dg": dg, "db": db}, acc=pre if acc else None)
        print(f"bn accumulate={acc} C={C}: {r}")
        NC.assert_ratios(r, f"accumulate={acc}")
