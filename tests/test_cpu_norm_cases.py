"""tests/norm_cases.py held to account without a GPU: the explicit f64 LayerNorm / BatchNorm references
agree with torch.autograd in f64, torch's own f32 CPU ops meet every bound the helper hands out (so a
correct f32 implementation passes), the ReLU-mask cap holds, the kernel constants parse, and planted
bugs are rejected (so the bounds can fail)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import norm_cases as NC

K = NC.kernel_constants()
MS = NC.ln_ms()
EPS = (1e-6, 1e-5)


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))


@functools.lru_cache(maxsize=None)
def _ln(family, M, D, eps):
    return NC.ln_case(family, M, D, eps)


@functools.lru_cache(maxsize=None)
def _neck(family, D):
    return NC.ln_case(family, NC.NECK_B * NC.NECK_NP, D, 1e-5, rowmap=NC.NECK_MAP, row_scale=NC.NECK_SCALE,
                      rps=NC.NECK_NP)


@functools.lru_cache(maxsize=None)
def _bn(M, C, kind, relu, resid, momentum=0.1):
    return NC.bn_case(M, C, kind, relu, resid, momentum)


def _phys(case, dx_rows):
    p = torch.zeros(case.X.shape, dtype=dx_rows.dtype)
    p[case.idx] = dx_rows
    return p


def test_kernel_constants_parse_and_agree():
    for n in ("LNV_ROWS", "LNB_ROWS", "LN_MAXV", "BN8_R", "BN_PH", "CR_COLS", "CS_ROWS", "BN_ROWS0", "LN_ROWS"):
        assert isinstance(K[n], int) and K[n] > 0, n
    assert 8 * K["LNV_ROWS"] == 4 * K["LNB_ROWS"] == K["LN_ROWS"]
    assert max(NC.LN_DS) == 64 * K["LN_MAXV"]
    # the derived shapes straddle what they are meant to, whatever the constants are
    R = K["LN_ROWS"]
    assert MS == (1, R - 1, R + 1, 2 * R + 6)
    assert -(-NC.ln_long_m() // R) > 16 * K["CR_COLS"]          # past colreduce_kernel's first batch
    Mb, Cb = NC.bn_shapes()[-1]
    assert -(-Mb // K["BN_ROWS0"]) > 8 * K["BN_PH"] and Mb % 2 == 1 and Cb % 8 == 0


@pytest.mark.parametrize("family", NC.LN_FAMILIES)
@pytest.mark.parametrize("D", [64, 384])
def test_ln_reference_is_autograd_f64(family, D):
    """Outputs and all gradients, with the neck's row map, dres and row_scale, and plain."""
    for case in (_neck(family, D), _ln(family, MS[2], D, 1e-6)):
        M, idx, ref = case.M, case.idx, case.ref
        x = case.X.double()[idx].clone().requires_grad_(True)
        g, b = case.gamma.double().requires_grad_(True), case.beta.double().requires_grad_(True)
        y = F.layer_norm(x, (D,), g, b, case.eps)
        y.backward(case.dy.double())
        dx = x.grad + case.dres.double()[idx]
        sc = torch.ones(M, dtype=torch.float64)
        if case.row_scale is not None:
            sc = torch.repeat_interleave(case.row_scale.double(), case.rps)
        xd = x.detach()
        pairs = {"y": y.detach(), "mean": xd.mean(1), "rstd": 1.0 / torch.sqrt(xd.var(1, unbiased=False) + case.eps),
                 "dx": dx, "dxs": dx * sc[:, None], "dgamma": g.grad, "dbeta": b.grad}
        for n, t in pairs.items():
            assert _rel(ref[n], t) <= 1e-12, (n, _rel(ref[n], t))
        # per row too: the small rows of "wide" must not hide under the large ones
        for n in ("y", "dx"):
            rr = (ref[n] - pairs[n]).abs().amax(1) / pairs[n].abs().amax(1)
            assert float(rr.max()) <= 1e-11, (n, float(rr.max()))


@pytest.mark.parametrize("M,C", NC.bn_shapes())
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("resid", [False, True])
@pytest.mark.parametrize("momentum", [0.1, 0.3])
def test_bn_reference_is_autograd_f64(M, C, relu, resid, momentum):
    """Outputs, all gradients and the running stats (unbiased variance), training and eval."""
    case = _bn(M, C, "f32", relu, resid, momentum)
    ref = case.ref
    x = case.x.double().requires_grad_(True)
    g, b = case.gamma.double().requires_grad_(True), case.beta.double().requires_grad_(True)
    r = case.res.double().requires_grad_(True) if resid else None
    rm, rv = case.rm.double().clone(), case.rv.double().clone()
    pre = F.batch_norm(x, rm, rv, g, b, training=True, momentum=momentum, eps=case.eps)
    pre = pre + r if resid else pre
    y = F.relu(pre) if relu else pre
    y.backward(case.dy.double())
    pairs = {"y": y.detach(), "rm": rm, "rv": rv, "dx": x.grad, "dg": g.grad, "db": b.grad}
    if resid:
        pairs["dr"] = r.grad
    for n, t in pairs.items():
        # dx is a difference of terms of size max(invstd gamma) max|dz|: judged against that
        den = float(case.scale["dx"]) if n == "dx" else float(t.abs().max()) + 1e-300
        assert float((ref[n] - t).abs().max()) / den <= 1e-12, n
    ev = NC.bn_ref(case.x, case.gamma, case.beta, case.rm, case.rv, momentum, case.eps, relu, case.res, None, False)
    pe = F.batch_norm(case.x.double(), case.rm.double(), case.rv.double(), case.gamma.double(), case.beta.double(),
                      training=False, eps=case.eps)
    pe = pe + case.res.double() if resid else pe
    assert _rel(ev["y"], F.relu(pe) if relu else pe) <= 1e-12


@pytest.mark.parametrize("family", NC.LN_FAMILIES)
@pytest.mark.parametrize("D", NC.LN_DS)
def test_torch_f32_layernorm_meets_every_bound(family, D):
    """f32 outputs by construction (4 x their own error); the column sums and the bf16 outputs
    (torch's f32 values rounded by torch) are the real checks. The f32 tolerances stay where the
    derivation puts them: at the 2e-6 floor or a small multiple of it."""
    cases = [_ln(family, M, D, eps) for M in MS for eps in EPS] + [_neck(family, D)]
    for case in cases:
        t = case.t32
        got = {"y": t["y"], "mean": t["mean"], "rstd": t["rstd"], "dx": _phys(case, t["dx"]), "dxs": t["dxs"],
               "dgamma": t["dgamma"], "dbeta": t["dbeta"]}
        NC.assert_ratios(NC.ln_ratios(case, got), f"f32 {family} M={case.M} D={D}")
        got16 = {"y": t["y"].to(torch.bfloat16), "dxs": t["dxs"].to(torch.bfloat16)}
        NC.assert_ratios(NC.ln_ratios(case, got16), f"bf16 {family} M={case.M} D={D}")
        assert all(v <= 1e-5 for v in case.tol.values()), case.tol


@pytest.mark.parametrize("M,C", NC.bn_shapes())
@pytest.mark.parametrize("kind", NC.BN_KINDS)
def test_torch_f32_batchnorm_meets_every_bound_and_mask_cap(M, C, kind):
    for relu in (False, True):
        for resid in (False, True):
            case = _bn(M, C, kind, relu, resid)
            assert case.left_out <= NC.MASK_CAP, case.left_out
            t = case.t32
            got = {n: t[n] for n in ("y", "rm", "rv", "dx", "dr", "dg", "db")}
            what = f"bn ({M},{C}) {kind} relu={relu} resid={resid}"
            NC.assert_ratios(NC.bn_ratios(case, got), what)
            NC.assert_ratios(NC.bn_ratios(case, {"y": t["y"].to(torch.bfloat16), "dx": t["dx"].to(torch.bfloat16)}),
                             what + " bf16")
            assert all(v <= 1e-5 for n, v in case.tol.items() if n != "dx"), case.tol
    for rvar in (1e-8, 1.0, 1e4):
        ev = NC.bn_eval_case(M, C, kind, True, True, rvar)
        r = NC.value_ratio(ev.t32["y"], ev.ref["y"], ev.tol["y"], ev.scale["y"])
        assert r <= 1.0, (rvar, r)


# ----------------------------------------------------------------------------- planted bugs
def _truncate_bf16(x):
    """f32 -> bf16 by dropping the low 16 bits (what a cast without rounding does)."""
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def test_planted_one_pass_variance_is_rejected():
    case = _ln("offset", MS[3], 384, 1e-6)
    x = case.X
    mean = x.mean(1, keepdim=True)
    var = (x * x).mean(1, keepdim=True) - mean * mean  # f32, one pass
    y = (x - mean) / torch.sqrt(var + case.eps) * case.gamma + case.beta
    assert NC.ln_ratios(case, {"y": y})["y"] > 1.0
    assert NC.ln_ratios(case, {"rstd": (1.0 / torch.sqrt(var + case.eps))[:, 0]})["rstd"] > 1.0
    # the same arithmetic with the two-pass variance passes
    var2 = ((x - mean) ** 2).mean(1, keepdim=True)
    y2 = (x - mean) / torch.sqrt(var2 + case.eps) * case.gamma + case.beta
    assert NC.ln_ratios(case, {"y": y2})["y"] <= 1.0


def test_planted_row_scale_by_mapped_row_is_rejected():
    case = _neck("plain", 128)
    rs = case.row_scale.double()
    bad = case.ref["dx"] * rs[(case.idx // case.rps).clamp_max(len(rs) - 1)][:, None]
    assert not torch.equal(bad, case.ref["dxs"])
    assert NC.ln_ratios(case, {"dxs": bad.float()})["dxs"] > 1.0
    assert NC.ln_ratios(case, {"dxs": case.ref["dxs"].float()})["dxs"] <= 1.0
    # and dx written at the logical instead of the physical row
    assert NC.ln_ratios(case, {"dx": torch.cat([case.ref["dx"], case.ref["dx"][:3]]).float()})["dx"] > 1.0


def test_planted_biased_running_variance_is_rejected():
    for M, C in NC.bn_shapes()[:4]:
        case = _bn(M, C, "f32", True, True)
        x = case.x.double()
        biased = (1 - case.momentum) * case.rv.double() + case.momentum * x.var(0, unbiased=False)
        assert NC.bn_ratios(case, {"rv": biased.float()})["rv"] > 1.0, (M, C)
        assert NC.bn_ratios(case, {"rv": case.ref["rv"].float()})["rv"] <= 1.0


def test_planted_truncating_bf16_cast_is_rejected():
    case = _ln("plain", MS[2], 128, 1e-6)
    assert NC.ln_ratios(case, {"y": _truncate_bf16(case.ref["y"])})["y"] > 1.0
    assert NC.ln_ratios(case, {"y": case.ref["y"].to(torch.bfloat16)})["y"] <= 1.0
    bn = _bn(33, 96, "bf16", True, True)
    assert NC.bn_ratios(bn, {"y": _truncate_bf16(bn.ref["y"])})["y"] > 1.0
    assert NC.bn_ratios(bn, {"y": bn.ref["y"].to(torch.bfloat16)})["y"] <= 1.0


def test_planted_wrong_relu_mask_and_column_sum_are_rejected():
    """dr with the mask dropped, and a column sum that lost one row."""
    bn = _bn(33, 96, "f32", True, True)
    assert NC.bn_ratios(bn, {"dr": bn.dy})["dr"] > 1.0
    assert NC.bn_ratios(bn, {"dr": bn.ref["dr"].float()})["dr"] <= 1.0
    lost = bn.ref["db"] - bn.ref["dz"][-1]
    assert NC.bn_ratios(bn, {"db": lost.float()})["db"] > 1.0
