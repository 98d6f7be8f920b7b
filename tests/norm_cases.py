"""Inputs, explicit f64 references and derived error bounds for the LayerNorm and BatchNorm kernels
of csrc/norm.hip (and the column-sum bound the element-wise tests share).

A plain helper (torch only) shared by tests/test_cpu_norm_cases.py (no GPU), tests/test_gpu_norm.py
and tests/test_gpu_elementwise.py.

Inputs are f32 tensors from a seeded generator; where a kernel operand is bf16 its values are made
bf16-exact here with torch's own CPU rounding, so a reference needs no allowance for input rounding.
The references are written out from the formulas in f64 (test_cpu_norm_cases.py holds them to
torch.autograd); every bound is handed out together with its reference:

  f32 outputs     |err| <= tol * scale, scale = the row's max |ref| (LayerNorm y, dx, dxs), the
                  tensor's max |ref| (BatchNorm y, running stats, mean), the value itself (rstd,
                  invstd), and tol = max(2e-6, 4 * e_torch): e_torch is the same figure for torch's own
                  f32 CPU op on the same case, computed at run time. 2e-6 is test_layernorm's bound; the
                  factor 4 allows for a different summation tree (a half-wave of 32 lanes x 4..16
                  elements against torch's vector lanes; both O(log D) roundings).
  bf16 outputs    |err| <= 2^-8 |ref| + tol * scale: one bf16 ulp, half of it the rounding and half the
                  f32 value falling on the other side of a tie.
  column sums     per column |err_c| <= 1e-5 * sum_r |term_rc|: no lane adds more than about 100 values in
                  sequence (8 rows per phase, the partial batches, the phase tree), 100 * 2^-24 = 6e-6.
                  Relative to max |ref| a near-cancelling column could hide. BatchNorm dg and db, dbeta
                  and ivit_colsum are held to exactly this.
  LayerNorm       the same, + tol_y * sum_r |dy_rc| max_c |xhat_rc|. dgamma sums dy * xhat, and the f32
  dgamma          xhat carries the error the forward is allowed (xhat is y at gamma = 1, beta = 0: at
                  most tol_y times the row's largest |xhat|), whatever size xhat_rc itself has; a term's
                  error is |dy_rc| times that, not 2^-24 |dy_rc xhat_rc|. Without the term torch's own f32
                  stands at 15 times the plain bound at M = 1 on "offset" and at 1.9 times on "plain"
                  (one row: a column whose xhat is 1e-2 has a bound of 1e-7 |dy| and an error of 1e-6
                  |dy|). The error is there at every M, so the term is too: at ordinary M (|xhat| ~ 1 on
                  average, its row maximum ~ 3, tol_y >= 2e-6) it about doubles the bound, which torch's
                  f32 meets at 0.13 or better without it. BatchNorm dg needs no such term: torch's f32
                  sits at 0.012 of the plain bound on every case here.
  BatchNorm dx    against max_c(invstd_c |gamma_c|) * max |dz| (dz = dy after the ReLU mask), not against
                  max |dx|: at M = 2 dx is analytically almost zero and torch's own f32 is 4e-3 "relative".
  ReLU mask       the reference masks on its own f64 pre-activation; elements with |pre| < 1e-4 are left
                  out of the dx / dr comparison, at most 0.1 % of a case.
"""
import functools
import math
import os
import re
from types import SimpleNamespace

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "visiontransformer-intention-prediction_amd", "csrc")

U = 2.0 ** -8        # bf16 unit roundoff: one ulp is at most 2^-7 |x|, half of it is the rounding
F32_FLOOR = 2e-6     # test_layernorm's bound on the f32 forward
F32_FACTOR = 4.0     # summation-tree allowance over torch's own f32 error
COL_REL = 1e-5       # column sums: ~100 sequential adds * 2^-24, rounded up
MASK_EPS = 1e-4      # |pre-activation| below which the ReLU mask is not judged
MASK_CAP = 1e-3      # at most this fraction of a case may be left out

LN_FAMILIES = ("plain", "offset", "wide")
BN_KINDS = ("f32", "bf16", "mixed")  # x / y / dy / dx: all f32, all bf16, f32 x and dx with bf16 y and dy


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def kernel_constants():
    """The constants the dispatch and the block shapes hang on, as the kernel sources define them, so
    every "straddles a block edge" shape follows the kernel if one changes. LN_ROWS is the number of
    rows one LayerNorm workgroup covers, in the vector (8 half-waves x LNV_ROWS) and the fallback
    (4 waves x LNB_ROWS) kernels alike: the backward workspace relies on the two being equal."""
    def cint(txt, name):
        m = re.search(r"constexpr\s+int\s+[^;]*?\b%s\s*=\s*(\d+)\s*[,;]" % name, txt)
        assert m, f"{name} not found in the kernel sources"
        return int(m.group(1))

    norm, common, gemm = _read("norm.hip"), _read("ivit_common.h"), _read("gemm_ops.hip")
    k = {n: cint(norm, n) for n in ("LNV_ROWS", "LNB_ROWS", "LN_MAXV", "BN8_R", "BN_PH")}
    k["CR_COLS"] = cint(common, "CR_COLS")
    k["CS_ROWS"] = cint(gemm, "CS_ROWS")
    m = re.search(r"static\s+int\s+bn_rows\s*\(\s*long\s+M\s*\)\s*\{\s*long\s+r\s*=\s*(\d+)\s*;", norm)
    assert m, "the start value of bn_rows not found in norm.hip"
    k["BN_ROWS0"] = int(m.group(1))
    assert 8 * k["LNV_ROWS"] == 4 * k["LNB_ROWS"], "the two LayerNorm kernels cover different rows per block"
    k["LN_ROWS"] = 8 * k["LNV_ROWS"]
    return k


LN_DS = (64, 128, 192, 256, 384, 448, 512)  # every NC of the vector kernel; fallback widths 1, 3 and 7
NECK_B, NECK_NP = 3, 23                      # the neck's row map (Np, Np + 1, 1): 72-row X, M = 69
NECK_MAP = (NECK_NP, NECK_NP + 1, 1)
NECK_SCALE = (0.0, 0.5, 2.0)                 # per-sample row_scale, rps = Np


def ln_ms():
    """Row counts around the rows-per-block edge: one row, a block less one, a block plus one, two
    blocks and a ragged third."""
    R = kernel_constants()["LN_ROWS"]
    return (1, R - 1, R + 1, 2 * R + 6)


def ln_long_m():
    """Enough row blocks that the partial list runs past colreduce_kernel's first batch (16 phases x
    16 loads in flight = 16 * CR_COLS partials)."""
    k = kernel_constants()
    return k["LN_ROWS"] * (16 * k["CR_COLS"] + 1) + 5


def bn_shapes():
    """(M, C): 35 is the detection head's width (C % 8 != 0: the scalar kernels); 520 spans two column
    blocks of bn_partial8_kernel; the last runs bn_colsum past its first 8 * BN_PH partials; odd M
    exercises the BN8_R row tail."""
    k = kernel_constants()
    return ((2, 8), (31, 35), (33, 96), (257, 520), (k["BN_ROWS0"] * 8 * k["BN_PH"] + 19, 8))


def bf16_exact(x):
    """x rounded to bf16 by torch's CPU cast (round to nearest even), back in f32."""
    return x.to(torch.bfloat16).to(torch.float32)


def rowmap_index(M, rowmap):
    """Physical row of each logical row r under (rpb, rstride, roff): (r / rpb) * rstride + roff +
    r % rpb, the identity when rpb == 0. The neck's (Np, Np + 1, 1) skips each sample's CLS row."""
    rpb, rstride, roff = rowmap
    r = torch.arange(M)
    return r if rpb == 0 else (r // rpb) * rstride + roff + r % rpb


def phys_rows(M, rowmap):
    rpb, rstride, _ = rowmap
    if rpb == 0:
        return M
    assert M % rpb == 0
    return (M // rpb) * rstride


# ----------------------------------------------------------------------------- ratios
def _ratio(err, bound):
    """max err / bound; an element with a zero bound must be exact."""
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    return float(r.max()) if r.numel() else 0.0


def _base(got32, ref, scale, keep=None):
    """The f32 figure of torch's own op: max |err| / scale."""
    err = (got32.double() - ref).abs()
    scale = scale.expand_as(ref)
    ok = scale > 0 if keep is None else (scale > 0) & keep
    return float((err[ok] / scale[ok]).max()) if bool(ok.any()) else 0.0


def f32_tol(base):
    return max(F32_FLOOR, F32_FACTOR * base)


def value_ratio(got, ref, tol, scale, keep=None):
    """err / bound of an f32 or bf16 output (the output's dtype picks the bound)."""
    err = (got.detach().cpu().double() - ref).abs()
    bound = tol * scale.expand_as(ref)
    if got.dtype == torch.bfloat16:
        bound = bound + U * ref.abs()
    if keep is not None:
        err = torch.where(keep, err, torch.zeros_like(err))
    return _ratio(err, bound)


def col_ratio(got, ref, absum, extra=None):
    """Column sums: max_c |err_c| / (1e-5 * sum_r |term_rc| (+ extra_c))."""
    bound = COL_REL * absum
    return _ratio((got.detach().cpu().double() - ref).abs(), bound if extra is None else bound + extra)


def assert_ratios(ratios, what):
    bad = {n: r for n, r in ratios.items() if not r <= 1.0}
    assert not bad, f"{what}: max err / bound {', '.join(f'{n} {r:.3g}' for n, r in ratios.items())}"


# ----------------------------------------------------------------------------- LayerNorm
def ln_inputs(family, M, D, rowmap=(0, 0, 0), seed=0):
    """X [physical rows, D], gamma, beta, dy [M, D], dres [physical rows, D], all f32."""
    g = torch.Generator().manual_seed(1009 * LN_FAMILIES.index(family) + 7919 * seed + 31 * M + D)
    rows = phys_rows(M, rowmap)
    x = torch.randn(rows, D, generator=g)
    if family == "plain":
        x = 2.0 * x + 0.5
    elif family == "offset":  # a one-pass E[x^2] - mean^2 variance loses it here
        x = 0.5 * x + 8.0
    elif family == "wide":  # the smallest rows have variance ~ eps
        x = x * torch.logspace(-3, 3, rows)[:, None]
    else:
        raise KeyError(family)
    gamma = 1.0 + 0.1 * torch.randn(D, generator=g)
    beta = 0.1 * torch.randn(D, generator=g)
    dy = torch.randn(M, D, generator=g)
    dres = torch.randn(rows, D, generator=g)
    return x, gamma, beta, dy, dres


def ln_ref(X, gamma, beta, eps, M, rowmap=(0, 0, 0), dy=None, dres=None, row_scale=None, rps=1):
    """LayerNorm forward and backward in f64 from the formulas. Logical row r reads X[idx[r]]; y, mean,
    rstd, dy and dxs are indexed by the logical row, dx and dres by the physical one (dx is returned
    for the logical rows, "dx" [M, D] = the kernel's dX[idx]); dxs = dx * row_scale[r // rps].
      xhat = (x - mean) rstd, y = xhat gamma + beta
      dx = dres + rstd (gamma dy - mean_D(gamma dy) - xhat mean_D(gamma dy xhat))
      dgamma = sum_r dy xhat, dbeta = sum_r dy"""
    idx = rowmap_index(M, rowmap)
    x, g, b = X.double()[idx], gamma.double(), beta.double()
    mu = x.mean(dim=1, keepdim=True)
    xc = x - mu
    var = (xc * xc).mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = xc * rstd
    out = {"y": xh * g + b, "mean": mu[:, 0], "rstd": rstd[:, 0], "var": var[:, 0]}
    if dy is None:
        return out
    dy = dy.double()
    gy = dy * g
    s1 = gy.mean(dim=1, keepdim=True)
    s2 = (gy * xh).mean(dim=1, keepdim=True)
    dx = rstd * (gy - s1 - xh * s2)
    if dres is not None:
        dx = dx + dres.double()[idx]
    sc = torch.ones(M, dtype=torch.float64)
    if row_scale is not None:
        sc = row_scale.double()[torch.arange(M) // rps]
    out.update({"dx": dx, "dxs": dx * sc[:, None], "dgamma": (dy * xh).sum(dim=0), "dbeta": dy.sum(dim=0),
                "dgamma_abs": (dy * xh).abs().sum(dim=0), "dbeta_abs": dy.abs().sum(dim=0),
                "dgamma_xh": (dy.abs() * xh.abs().amax(dim=1, keepdim=True)).sum(dim=0)})
    return out


def ln_torch_f32(X, gamma, beta, eps, M, rowmap=(0, 0, 0), dy=None, dres=None, row_scale=None, rps=1):
    """torch's own f32 CPU LayerNorm (native_layer_norm and its autograd) on the same case."""
    idx = rowmap_index(M, rowmap)
    D = X.shape[1]
    x = X.float()[idx].clone().requires_grad_(True)
    g, b = gamma.float().clone().requires_grad_(True), beta.float().clone().requires_grad_(True)
    y, mean, rstd = torch.native_layer_norm(x, (D,), g, b, eps)
    out = {"y": y.detach(), "mean": mean.detach().reshape(-1), "rstd": rstd.detach().reshape(-1)}
    if dy is None:
        return out
    y.backward(dy.float())
    dx = x.grad if dres is None else x.grad + dres.float()[idx]
    sc = torch.ones(M) if row_scale is None else row_scale.float()[torch.arange(M) // rps]
    out.update({"dx": dx, "dxs": dx * sc[:, None], "dgamma": g.grad, "dbeta": b.grad})
    return out


def _ln_scales(ref):
    s = {"y": ref["y"].abs().amax(dim=1, keepdim=True),
         "mean": ref["mean"].abs() + torch.sqrt(ref["var"]),  # the row's own spread: a mean near 0 is not "relative"
         "rstd": ref["rstd"]}
    if "dx" in ref:
        s["dx"] = ref["dx"].abs().amax(dim=1, keepdim=True)
        s["dxs"] = ref["dxs"].abs().amax(dim=1, keepdim=True)
    return s


def ln_case(family, M, D, eps, rowmap=(0, 0, 0), dy_bf16=False, with_dres=True, row_scale=None, rps=1, seed=0,
            X=None, dy=None):
    """One LayerNorm case: inputs, the f64 reference, torch's f32 figures and the tolerances.
    row_scale: a tuple of per-sample scales (or None). X, dy: given tensors in place of the family's
    (a fused GEMM's exact product as the LayerNorm input or as the incoming gradient)."""
    given_x, given_dy = X, dy
    X, gamma, beta, dy, dres = ln_inputs(family, M, D, rowmap, seed)
    if given_x is not None:
        assert given_x.shape == X.shape
        X = given_x.float()
    if given_dy is not None:
        assert given_dy.shape == dy.shape
        dy = given_dy.float()
    if dy_bf16:
        dy = bf16_exact(dy)
    if not with_dres:
        dres = None
    rs = None if row_scale is None else torch.tensor(row_scale, dtype=torch.float32)
    args = (X, gamma, beta, eps, M, rowmap, dy, dres, rs, rps)
    ref, t32 = ln_ref(*args), ln_torch_f32(*args)
    scale = _ln_scales(ref)
    base = {n: _base(t32[n], ref[n], scale[n]) for n in scale}
    return SimpleNamespace(family=family, M=M, D=D, eps=eps, rowmap=rowmap, idx=rowmap_index(M, rowmap), X=X,
                           gamma=gamma, beta=beta, dy=dy, dres=dres, row_scale=rs, rps=rps, ref=ref, t32=t32,
                           scale=scale, base=base, tol={n: f32_tol(v) for n, v in base.items()})


def ln_ratios(case, got, acc=None):
    """err / bound for every output in ``got`` (name -> tensor; "dx" is the kernel's physical-row dX,
    gathered here at the logical rows). acc: {"dgamma": pre, "dbeta": pre}, the values an accumulating
    call added to (they join the reference and its sum of |terms|)."""
    out = {}
    for n, t in got.items():
        if t is None:
            continue
        if n in ("dgamma", "dbeta"):
            ref, ab = case.ref[n], case.ref[n + "_abs"]
            if acc is not None:
                ref, ab = ref + acc[n].double(), ab + acc[n].double().abs()
            out[n] = col_ratio(t, ref, ab, case.tol["y"] * case.ref["dgamma_xh"] if n == "dgamma" else None)
            continue
        t = t.detach().cpu()
        if n == "dx":
            t = t[case.idx]
        out[n] = value_ratio(t, case.ref[n], case.tol[n], case.scale[n])
    return out


# ----------------------------------------------------------------------------- BatchNorm
def bn_inputs(M, C, kind, resid, seed=0):
    """x, gamma, beta, running mean / var, residual (or None), dy: f32, bf16-exact where the kernel
    operand is bf16 (kind "bf16": x, residual, dy; "mixed": residual and dy, which have y's dtype)."""
    g = torch.Generator().manual_seed(15485863 + 104729 * seed + 131 * M + C)
    x = 3.0 * torch.randn(M, C, generator=g) + 1.0
    gamma = 1.0 + 0.1 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    rm = 0.5 * torch.randn(C, generator=g)
    rv = 0.5 + torch.rand(C, generator=g)
    res = torch.randn(M, C, generator=g)
    dy = torch.randn(M, C, generator=g)
    if kind == "bf16":
        x = bf16_exact(x)
    if kind in ("bf16", "mixed"):
        res, dy = bf16_exact(res), bf16_exact(dy)
    return x, gamma, beta, rm, rv, (res if resid else None), dy


def bn_ref(x, gamma, beta, rm, rv, momentum, eps, relu, res, dy=None, training=True):
    """BatchNorm over the rows of [M, C] in f64 from the formulas. Training: batch mean and biased
    variance normalise, the running stats move by momentum with the unbiased variance (M / (M - 1));
    eval: the running stats normalise. pre = xhat gamma + beta (+ res), y = relu(pre) or pre.
      dz = dy where pre > 0 (relu) or dy, dr = dz, db = sum_r dz, dg = sum_r dz xhat
      dx = invstd gamma (dz - mean_r(dz) - xhat mean_r(dz xhat))        (training)"""
    x, g, b = x.double(), gamma.double(), beta.double()
    M = x.shape[0]
    if training:
        mean = x.mean(dim=0)
        var = ((x - mean) ** 2).mean(dim=0)
        out = {"rm": (1.0 - momentum) * rm.double() + momentum * mean,
               "rv": (1.0 - momentum) * rv.double() + momentum * (var * M / (M - 1) if M > 1 else var)}
    else:
        mean, var = rm.double(), rv.double()
        out = {}
    invstd = 1.0 / torch.sqrt(var + eps)
    xh = (x - mean) * invstd
    pre = xh * g + b
    if res is not None:
        pre = pre + res.double()
    out.update({"mean": mean, "invstd": invstd, "pre": pre, "y": pre.clamp_min(0.0) if relu else pre})
    out["keep"] = (pre.abs() >= MASK_EPS) if relu else torch.ones_like(pre, dtype=torch.bool)
    if dy is None:
        return out
    dz = dy.double()
    if relu:
        dz = torch.where(pre > 0, dz, torch.zeros_like(dz))
    m1, m2 = dz.mean(dim=0), (dz * xh).mean(dim=0)
    out.update({"dz": dz, "dr": dz, "dx": invstd * g * (dz - m1 - xh * m2), "db": dz.sum(dim=0),
                "dg": (dz * xh).sum(dim=0), "db_abs": dz.abs().sum(dim=0), "dg_abs": (dz * xh).abs().sum(dim=0)})
    return out


def bn_torch_f32(x, gamma, beta, rm, rv, momentum, eps, relu, res, dy=None, training=True):
    """torch's own f32 CPU batch_norm (+ residual, relu) and its autograd on the same case."""
    F = torch.nn.functional
    xr = x.float().clone().requires_grad_(True)
    g, b = gamma.float().clone().requires_grad_(True), beta.float().clone().requires_grad_(True)
    r = None if res is None else res.float().clone().requires_grad_(True)
    rm2, rv2 = rm.float().clone(), rv.float().clone()
    pre = F.batch_norm(xr, rm2, rv2, g, b, training=training, momentum=momentum, eps=eps)
    if r is not None:
        pre = pre + r
    y = F.relu(pre) if relu else pre
    out = {"y": y.detach(), "rm": rm2, "rv": rv2}
    if dy is not None:
        y.backward(dy.float())
        out.update({"dx": xr.grad, "dr": None if r is None else r.grad, "dg": g.grad, "db": b.grad})
    return out


def bn_case(M, C, kind, relu, resid, momentum=0.1, eps=1e-5, seed=0):
    """One training-mode BatchNorm case: inputs, the f64 reference, torch's f32 figures, tolerances."""
    x, gamma, beta, rm, rv, res, dy = bn_inputs(M, C, kind, resid, seed)
    args = (x, gamma, beta, rm, rv, momentum, eps, relu, res, dy)
    ref, t32 = bn_ref(*args), bn_torch_f32(*args)
    scale = {"y": ref["y"].abs().max(), "rm": ref["rm"].abs().max(), "rv": ref["rv"].abs().max(),
             "dx": (ref["invstd"] * gamma.double().abs()).max() * ref["dz"].abs().max()}
    base = {n: _base(t32[n], ref[n], scale[n], ref["keep"] if n == "dx" else None) for n in scale}
    tol = {n: f32_tol(v) for n, v in base.items()}
    # mean and invstd are not outputs of torch's op: they are held to the running stats' tolerances,
    # the same sums. mean against the batch's largest |mean|. invstd = (var + eps)^-1/2 relatively,
    # times the conditioning of the two-pass variance: x - mean carries an absolute error of about
    # u max|x_c| (the rounded mean), so var a relative one of 2 u max|x_c| invstd and invstd half of
    # that (at M = 2 a column's two values can lie 1 % of their size apart)
    scale["mean"], tol["mean"] = ref["mean"].abs().max(), tol["rm"]
    scale["invstd"] = ref["invstd"] * (1.0 + x.double().abs().amax(dim=0) * ref["invstd"])
    tol["invstd"] = tol["rv"]
    return SimpleNamespace(M=M, C=C, kind=kind, relu=relu, momentum=momentum, eps=eps, x=x, gamma=gamma, beta=beta,
                           rm=rm, rv=rv, res=res, dy=dy, ref=ref, t32=t32, scale=scale, base=base, tol=tol,
                           left_out=1.0 - float(ref["keep"].double().mean()))


def bn_ratios(case, got, acc=None):
    """err / bound for every output in ``got``; dr is exact (dy under the mask, in dy's own dtype or a
    wider one) and both dx and dr skip the elements whose mask is not judged."""
    out = {}
    keep = case.ref["keep"]
    for n, t in got.items():
        if t is None:
            continue
        if n in ("dg", "db"):
            ref, ab = case.ref[n], case.ref[n + "_abs"]
            if acc is not None:
                ref, ab = ref + acc[n].double(), ab + acc[n].double().abs()
            out[n] = col_ratio(t, ref, ab)
        elif n == "dr":
            err = (t.detach().cpu().double() - case.ref["dr"]).abs()
            out[n] = _ratio(torch.where(keep, err, torch.zeros_like(err)), torch.zeros_like(err))
        else:
            out[n] = value_ratio(t, case.ref[n], case.tol[n], case.scale[n], keep if n == "dx" else None)
    return out


def bn_eval_case(M, C, kind, relu, resid, rvar, eps=1e-5, seed=0):
    """Eval mode: running mean random, every running var = rvar; y against the f64 formula."""
    x, gamma, beta, rm, _, res, _ = bn_inputs(M, C, kind, resid, seed)
    rv = torch.full((C,), rvar, dtype=torch.float32)
    args = (x, gamma, beta, rm, rv, 0.0, eps, relu, res, None, False)
    ref, t32 = bn_ref(*args), bn_torch_f32(*args)
    scale = {"y": ref["y"].abs().max()}
    base = {"y": _base(t32["y"], ref["y"], scale["y"])}
    tol = {"y": f32_tol(base["y"])}
    scale["mean"], tol["mean"] = ref["mean"].abs().max(), 0.0  # a copy of the running mean
    scale["invstd"], tol["invstd"] = ref["invstd"], tol["y"]
    return SimpleNamespace(M=M, C=C, kind=kind, relu=relu, eps=eps, x=x, gamma=gamma, beta=beta, rm=rm, rv=rv, res=res,
                           ref=ref, t32=t32, scale=scale, base=base, tol=tol)
