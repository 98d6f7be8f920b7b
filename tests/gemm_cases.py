"""Inputs on which a linear layer has no rounding, their f64 references, a mirror of the dispatch and
the derived bounds of the epilogues that cannot be exact, for the GEMMs of csrc/gemm_engine.h (behind
ivit_linear_fwd / _fwd_qs / _dgrad / _wgrad), csrc/rowpanel.hip (the row-panel and fused GEMM + LayerNorm
kernels), csrc/wgrad_block.hip (ivit_vit_block_wgrad) and the weight packs that feed them.

A plain helper (torch only) shared by tests/test_cpu_gemm_cases.py (no GPU) and tests/test_gpu_gemm.py.

Every defect these kernels can have is an indexing defect (a wrong K tail, clamp, swizzle, split boundary
or epilogue column). One dropped or doubled K element at K = 1536 moves an output of Gaussian operands by
0.025 standard deviations, under any relative bar; so, as in tests/conv_cases.py, the operands are chosen
such that every product and every partial sum is exactly representable in f32. Any correct kernel then
returns the bits of the f64 reference whatever its tile, summation order or split:

  bf16 cases   x, w, dy integers in [-8, 8]; bias and residual multiples of 1/4 with |.| <= 16; row
               scales from {0, 0.5, 1, 2}; col_scale / qscale 0.125 (ops.Q2_SCALE is no power of two, so
               the scale goes through the ABI); the G of ivit_linear_dgrad_mul_panel multiples of 1/8 in
               [-1, 1].
  f32 cases    one operand of each product integers in [-4, 4], the other n / 512 with odd |n| < 512 (not
               bf16-exact: an f32 path that rounds its operands to bf16 fails). The forward and the data
               gradient read w = n / 512; the weight gradient reads its own ``dyw`` = n / 512 against the
               integer x (two operands of nine significant bits each would leave six bits for the sum).

  budget       per output, max over its elements of sum |terms| (the same product on |operands|, plus
               |bias|, the scale and the residual) times 2^(fraction bits of the result). It must stay
               below 2^24: then every partial sum in any order is an integer multiple of the unit below
               2^24 and f32 holds it. test_cpu_gemm_cases.py asserts it per case and shows torch's own f32
               CPU matmul bit-equal to the f64 one.
  bf16 outputs are compared with torch's CPU round-to-nearest-even of the exact value, bit for bit
               (tests/test_gpu_elementwise.py pins ivit_cast to that rounding).
  magnitude    on bf16 cases whose sums have at least conv_cases.MAG_TERMS = 144 terms, a third of the
               outputs exceed 256 in magnitude (a sum of n products of uniform integers in [-8, 8] has
               standard deviation 24 sqrt(n)): an accumulation in bf16 could not return them.
  sentinels    every output buffer, and the columns of a wider-than-N row that the kernel must leave
               alone, hold a sentinel before the call; the comparison is on the whole buffer, so the
               sentinel must be intact afterwards (NaN, in tests/test_gpu_gemm.py).

Epilogues that cannot be exact (no bound below is fitted to the kernel):

  GELU / GELU' the pre-activation z is exact; the weight is scaled by a power of two so that z has
               standard deviation 3 to 4 (w = n / 64 at K = 64, n / 128 at K = 320 and 384, n / 256 at
               K = 1536: 72-82 % of z in |z| < 4; K = 128 has no such power of two and takes n / 64, a
               deviation of 4.2 with 65 % inside). Bound: |err| <= ACT_TOL max(1, |ref|), ACT_TOL = 1e-6,
               plus 2^-8 |ref| for a bf16 output: the bound of _act_ratio in tests/test_gpu_elementwise.py,
               against f64 with the exact erf. For a product acc * gelu'(pre) the error scales with the
               exact accumulator: ACT_TOL max(1, |acc|) (+ 2^-8 |ref|). The bf16-output form evaluates erf
               by Abramowitz-Stegun 7.1.26, documented error 1.5e-7, at most 0.75e-7 |z| on gelu: inside
               the bound for |z| <= 12.
  ivit_linear_resid_ln_fwd   X (f32) is exact; mean, rstd and Y are held to the LayerNorm bounds of
               tests/norm_cases.py (ln_case / ln_ratios) with the exact X as the LayerNorm input.
  ivit_linear_dgrad_ln_bwd   the product G = dY W is exact but not observable; dX, dXs, dgamma and dbeta
               are held to norm_cases' backward bounds with dy := G.

Split-K: the engine cuts the reduction of ivit_linear_wgrad into ``engine_splits`` ranges of
``engine_chunk`` rows by splitk_choice's cost model (mirrored by conv_cases.wgrad_engine_splits at 512
resident workgroups, which is what an MI355X gives), and ivit_vit_block_wgrad cuts its tokens into
``wb_splits`` ranges of ``wb_chunk``. Both round the range up to whole K steps, so the last ranges can
start past the end: M = 8250, N = 136, K = 72 takes 16 bf16 splits of 576 rows, the last empty and the one
before it 186 rows, and 64 f32 splits with six empty; ivit_vit_block_wgrad has an empty split at every M
with 6 * ceil(steps / 7) >= steps. There its loader waves used to add 16 bf16 values per lane of LDS they
never wrote into the bias gradient; the kernel now guards the sum, and the host launches and reduces only
the ``wb_launched`` non-empty splits.

Row-panel epilogue forms: ivit_set_knob(IVIT_KNOB_WIDE_EPI) 1 / 2 selects the transposed-accumulator
epilogue only where every output row is 16-B aligned (ld % 8 == 0: ``wide_transposed``), so each form runs
at ld = N + 4 (the LDS-tile epilogue whatever the knob) and at ld = N + 8.

Measured on an MI355X, worst err / bound of each family that is not exact (test_gpu_gemm.py prints them
with -s; RATIOS below): the f32 outputs of the engine's GELU stand at 0.09 - 0.11 and of acc * gelu' at
0.14 - 0.15 of the bound, for erff / __expf (f32 operands) and for Abramowitz-Stegun (bf16 operands) alike;
every bf16 output's 0.99 is its half ulp, as in tests/test_gpu_elementwise.py. The fused LayerNorm's f32
outputs stand at 0.004 (mean), 0.07 (rstd), 0.10 (dx), 0.01 (dgamma) of norm_cases' bounds, dbeta is exact
(a sum of the integer G).
"""
import functools
import math
import re
from types import SimpleNamespace

import torch

import conv_cases as CC
import norm_cases as NC

CSRC = CC.CSRC
LIMIT = CC.LIMIT
MAG_TERMS = CC.MAG_TERMS
ACT_TOL = 1e-6          # _act_ratio's bound (tests/test_gpu_elementwise.py)
U = NC.U                # bf16 unit roundoff
QSCALE = 0.125
ROW_SCALES = (1.0, 0.5, 2.0, 0.0)
rne_bf16, same_bits = CC.rne_bf16, CC.same_bits

# worst err / bound per family as measured on an MI355X (see the docstring); a record, not a bound
RATIOS = {"engine f32 gelu -> f32": 0.111, "engine f32 acc gelu' -> f32": 0.145, "engine bf16 gelu -> f32": 0.0884,
          "engine bf16 acc gelu' -> f32": 0.144, "engine bf16 gelu -> bf16": 0.996, "engine bf16 acc gelu' -> bf16": 0.996,
          "panel gelu": 0.996, "panel gelu_d y": 0.996, "panel gelu_d g": 0.987, "panel dgelu": 0.996,
          "resid_ln_fwd y": 0.995, "resid_ln_fwd mean": 0.00414, "resid_ln_fwd rstd": 0.0662,
          "dgrad_ln_bwd dx": 0.1, "dgrad_ln_bwd dxs": 0.994, "dgrad_ln_bwd dgamma": 0.0098, "dgrad_ln_bwd dbeta": 0.0,
          "dgrad_ln_bwd dgamma (accumulated)": 0.00811, "dgrad_ln_bwd dbeta (accumulated)": 0.00584}


@functools.lru_cache(maxsize=None)
def kernel_constants():
    """The tile sizes the edge shapes hang on, as the kernel sources define them."""
    def cint(txt, name):
        m = re.search(r"constexpr\s+int\s+[^;]*?\b%s\s*=\s*(\d+)\s*[,;]" % name, txt)
        assert m, f"{name} not found in the kernel sources"
        return int(m.group(1))

    eng, pan, wb = CC._read("gemm_engine.h"), CC._read("rowpanel.hip"), CC._read("wgrad_block.hip")
    k = {n: cint(eng, n) for n in ("GBM", "GBN", "GBK16", "GBK32")}
    k.update({n: cint(pan, n) for n in ("RP_MT", "RP_N")})
    k.update({n: cint(wb, n) for n in ("WB_BK", "WB_SMAX")})
    return k


# ----------------------------------------------------------------------------- dispatch mirror
def engine_splits(M, N, K, bf):
    """ivit_linear_wgrad's wgrad_splits(N, K, M, bf) -> splitk_choice: the split of the token reduction."""
    return CC.wgrad_engine_splits(M, N, K, bf)


def engine_chunk(M, splits, bf):
    """launch_gemm's kchunk: rows of the reduction per split, a multiple of the K tile."""
    c = kernel_constants()
    bk = c["GBK16"] if bf else c["GBK32"]
    return max(-(-(-(-M // splits)) // bk) * bk, bk)


def engine_split_rows(M, N, K, bf):
    """Rows of the reduction each split covers (0: an empty split)."""
    s = engine_splits(M, N, K, bf)
    ch = engine_chunk(M, s, bf)
    return [max(0, min(M, (i + 1) * ch) - i * ch) for i in range(s)]


def wb_steps(M):
    return -(-M // kernel_constants()["WB_BK"])


def wb_splits(M):
    """wb_splits (wgrad_block.hip): the nominal split count, which sizes the workspace."""
    steps, smax = wb_steps(M), kernel_constants()["WB_SMAX"]
    return (steps if steps > 0 else 1) if steps < smax else smax


def wb_chunk(M):
    """Tokens per split: ceil(steps / wb_splits) K steps."""
    return -(-wb_steps(M) // wb_splits(M)) * kernel_constants()["WB_BK"]


def wb_empty(M):
    """How many of the nominal splits start at or past M."""
    return sum(1 for i in range(wb_splits(M)) if i * wb_chunk(M) >= M)


def wb_launched(M):
    """The splits ivit_vit_block_wgrad launches and reduces: the non-empty ones."""
    bk = kernel_constants()["WB_BK"]
    return -(-wb_steps(M) // (wb_chunk(M) // bk))


def wide_transposed(knob, form, ld_ok):
    """launch_wide (rowpanel.hip): the transposed-accumulator epilogue runs iff the knob asks for it for
    this form and every output row is 16-B aligned."""
    return bool(ld_ok and knob != 0 and (form in ("none", "none_t", "gelu_d") or knob == 2))


# ----------------------------------------------------------------------------- generators
def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


_odd512 = CC._odd512


def _quarters(g, shape):
    return _ints(g, shape, -64, 64) / 4.0


def row_scale(M, rps):
    """A row scale per group of rps rows, cycling through ROW_SCALES."""
    n = -(-M // rps)
    return torch.tensor(ROW_SCALES)[torch.arange(n) % len(ROW_SCALES)]


def _expand(scale, M, rps):
    return torch.ones(M, dtype=torch.float64) if scale is None else scale.double()[torch.arange(M) // rps]


def gelu(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def gelu_grad(z):
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def act_ratio(got, ref, acc=None):
    """max |err| / (ACT_TOL max(1, |acc or ref|) (+ 2^-8 |ref| for a bf16 output))."""
    base = ref if acc is None else acc
    bound = ACT_TOL * base.abs().clamp_min(1.0)
    if got.dtype == torch.bfloat16:
        bound = bound + U * ref.abs()
    return NC._ratio((got.detach().cpu().double().reshape(ref.shape) - ref).abs(), bound)


def exact(got, ref):
    """f32: equal to the f64 reference; bf16: the bits of its round-to-nearest-even."""
    if got.dtype == torch.bfloat16:
        return same_bits(got, rne_bf16(ref).reshape(got.shape))
    return torch.equal(got.detach().cpu().double().reshape(ref.shape), ref)


# ----------------------------------------------------------------------------- engine cases
# name: (dtype, M, N, K). M at the 128-row tile edge, N with a ragged 8-column chunk (the forward only:
# the gradients' ABI demands N % 8 == 0), a ragged tile and two tiles, K below, at and past the K tile.
def _engine_table():
    t = {}
    for d in ("bf16", "f32"):
        s = d[0]
        t[f"{s}_m1_n1_k8"] = (d, 1, 1, 8)          # the smallest fast_ok C; one row, one column
        t[f"{s}_m127_n7_k56"] = (d, 127, 7, 56)    # only a partial K tile (bf16), N < 8
        t[f"{s}_m128_n8_k64"] = (d, 128, 8, 64)    # only full tiles
        t[f"{s}_m128_n128_k64"] = (d, 128, 128, 64)
        t[f"{s}_m129_n129_k72"] = (d, 129, 129, 72)  # 2 x 2 tiles, a full K tile plus a tail, N % 8 == 1
        t[f"{s}_m129_n136_k520"] = (d, 129, 136, 520)
        t[f"{s}_m300_n200_k136"] = (d, 300, 200, 136)  # 3 x 2 tiles: no multiple of 8 for the XCD remap
        t[f"{s}_m300_n136_k8"] = (d, 300, 136, 8)
        # the weight gradient's splits
        t[f"{s}_m8250_n136_k72"] = (d, 8250, 136, 72)  # an empty last split (bf16), six (f32)
        t[f"{s}_m2100_n136_k72"] = (d, 2100, 136, 72)  # four bf16 splits, none empty
        t[f"{s}_m5_n136_k72"] = (d, 5, 136, 72)        # fewer rows than one K tile
        t[f"{s}_m1700_n304_k72"] = (d, 1700, 304, 72)  # 3 tiles x 3 (bf16) or 13 (f32) splits: the XCD remap's tail
    return t


ENGINE = _engine_table()
ENGINE_MS, ENGINE_NS, ENGINE_KS = (1, 127, 128, 129, 300), (1, 7, 8, 128, 129, 136, 200), (8, 56, 64, 72, 136, 520)
RPS_OF = lambda M: (1, 7, (M + 1) // 2, M)  # noqa: E731
QS_COLS = lambda N: sorted({c for c in (0, 8, 136, N) if c <= N and c % 8 == 0})  # noqa: E731


def _seed(table, name):
    return 15485867 + 32452867 * sorted(table).index(name)


@functools.lru_cache(maxsize=None)
def lin_case(name):
    """One engine case: operands (f32 tensors, exact in the case's compute dtype), the f64 references
    y0 = x w^T, y = y0 + bias, dx = dy w, dw = dyw^T x, db = colsum(dyw), and the budgets."""
    dtype, M, N, K = ENGINE[name]
    g = torch.Generator().manual_seed(_seed(ENGINE, name))
    if dtype == "bf16":
        x, w, dy = _ints(g, (M, K), -8, 8), _ints(g, (N, K), -8, 8), _ints(g, (M, N), -8, 8)
        dyw, frac = dy, 1
    else:
        x, w, dy = _ints(g, (M, K), -4, 4), _odd512(g, (N, K)), _ints(g, (M, N), -4, 4)
        dyw, frac = _odd512(g, (M, N)), 512
    bias, resid = _quarters(g, (N,)), _quarters(g, (M, N))
    dw0, db0 = _ints(g, (N, K), -16, 16), _ints(g, (N,), -16, 16)   # what an accumulating wgrad adds to
    X, W, DY, DYW = x.double(), w.double(), dy.double(), dyw.double()
    ref = {"y0": X @ W.T, "dx": DY @ W, "dw": DYW.T @ X, "db": DYW.sum(0)}
    ref["y"] = ref["y0"] + bias.double()
    ay = X.abs() @ W.abs().T + bias.double().abs()
    budget = {"y": float(ay.max()) * max(frac, 4), "dx": float((DY.abs() @ W.abs()).max()) * frac,
              "dw": (float((DYW.abs().T @ X.abs()).max()) + 16) * frac, "db": (float(DYW.abs().sum(0).max()) + 16) * frac,
              # columns times 1/8 on a quarter bias; residual + scale (1/2) * (y0 + quarter bias)
              "qs": float(ay.max()) * max(frac, 32), "resid": (2 * float(ay.max()) + 16) * max(2 * frac, 8)}
    return SimpleNamespace(name=name, dtype=dtype, M=M, N=N, K=K, x=x, w=w, dy=dy, dyw=dyw, bias=bias, resid=resid,
                           dw0=dw0, db0=db0, ref=ref, budget=budget)


def qs_ref(c, cols, bias=True):
    y = (c.ref["y"] if bias else c.ref["y0"]).clone()
    y[:, :cols] *= QSCALE
    return y


def resid_ref(c, scale, rps, bias=True):
    return c.resid.double() + _expand(scale, c.M, rps)[:, None] * (c.ref["y"] if bias else c.ref["y0"])


# GELU through the engine's epilogues: (dtype, M, N, K, the power of two the weight is divided by)
ENGINE_GELU = {"b_gelu_k64": ("bf16", 129, 136, 64, 64), "b_gelu_k384": ("bf16", 300, 200, 384, 128),
               "f_gelu_k64": ("f32", 129, 136, 64, 4)}


@functools.lru_cache(maxsize=None)
def gelu_case(name):
    """z = x w^T + bias exact with a standard deviation of 3 to 4; the data gradient acc = dy w2 exact,
    times gelu'(pre) at pre = multiples of 1/8 in [-6, 6]."""
    dtype, M, N, K, div = ENGINE_GELU[name]
    g = torch.Generator().manual_seed(_seed(ENGINE_GELU, name) + 1)
    if dtype == "bf16":
        x, w, dy, w2 = _ints(g, (M, K), -8, 8), _ints(g, (N, K), -8, 8) / div, _ints(g, (M, K), -8, 8), _ints(g, (K, N), -8, 8)
        frac = 4 * div
    else:
        x, w, dy, w2 = _ints(g, (M, K), -4, 4), _odd512(g, (N, K)) / div, _ints(g, (M, K), -4, 4), _odd512(g, (K, N))
        frac = 512 * div
    bias = _quarters(g, (N,)) / 16.0     # |bias| <= 1: z keeps its spread
    pre = _ints(g, (M, N), -48, 48) / 8.0
    z = x.double() @ w.double().T + bias.double()
    acc = dy.double() @ w2.double()
    budget = {"z": float((x.double().abs() @ w.double().abs().T + 1).max()) * max(frac, 64),
              "acc": float((dy.double().abs() @ w2.double().abs()).max()) * (512 if dtype == "f32" else 1)}
    return SimpleNamespace(name=name, dtype=dtype, M=M, N=N, K=K, x=x, w=w, bias=bias, dy=dy, w2=w2, pre=pre, z=z,
                           acc=acc, budget=budget)


# ----------------------------------------------------------------------------- row-panel cases
# name: (M, N, K, the power of two the GELU forms' weight is divided by). M around the 144-row panel.
PANEL = {"p_m1_n384_k64": (1, 384, 64, 64), "p_m143_n768_k128": (143, 768, 128, 64),
         "p_m144_n384_k320": (144, 384, 320, 128), "p_m145_n1152_k128": (145, 1152, 128, 64),
         "p_m289_n768_k64": (289, 768, 64, 64), "p_m289_n1152_k320": (289, 1152, 320, 128)}
PANEL_MS, PANEL_NS, PANEL_KS = (1, 143, 144, 145, 289), (384, 768, 1152), (64, 128, 320)
PANEL_FORMS = ("none", "none_t", "gelu", "gelu_d", "dgelu", "dmul")
PANEL_KNOBS = (0, 1, 2)
PANEL_LDS = (4, 8)   # output rows N + 4 (never 16-B aligned rows: the LDS-tile epilogue) and N + 8
QCOLS = lambda N: sorted({0, 384, N})  # noqa: E731


@functools.lru_cache(maxsize=None)
def panel_case(name):
    """a [M, K], w [N, K] integers; the transposed pack reads wt = w^T [K, N], so both packs hold the
    same matrix and y0 = a w^T serves the forward and ops.panel_dgrad alike. The GELU forms read w / div."""
    M, N, K, div = PANEL[name]
    g = torch.Generator().manual_seed(_seed(PANEL, name) + 2)
    a, w = _ints(g, (M, K), -8, 8), _ints(g, (N, K), -8, 8)
    bias = _quarters(g, (N,))
    bias_g = bias / 16.0
    pre = _ints(g, (M, N), -48, 48) / 8.0
    G = _ints(g, (M, N), -8, 8) / 8.0
    y0 = a.double() @ w.double().T
    ay = float((a.double().abs() @ w.double().abs().T).max())
    z = y0 / div + bias_g.double()
    budget = {"y": (ay + 16) * 32, "z": (ay / div + 1) * 64 * div, "dmul": ay * 8}
    return SimpleNamespace(name=name, M=M, N=N, K=K, div=div, a=a, w=w, wt=w.T.contiguous(), bias=bias, bias_g=bias_g,
                           pre=pre, G=G, y0=y0, z=z, budget=budget)


def panel_none_ref(c, qcols, bias=True):
    y = c.y0 + c.bias.double() if bias else c.y0.clone()
    y[:, :qcols] *= QSCALE
    return y


# ----------------------------------------------------------------------------- fused GEMM + LayerNorm
# name: (M, K, scale?, rps, dX aliases dres)
LN_EPS = 1e-6
FUSED_LN = {"ln_m1_k64": (1, 64, True, 1, True), "ln_m143_k128": (143, 128, False, 1, False),
            "ln_m145_k320": (145, 320, True, 5, True), "ln_m289_k64": (289, 64, True, 289, False),
            "ln_m289_k128": (289, 128, True, 1, True)}
FUSED_MS, FUSED_KS = (1, 143, 145, 289), (64, 128, 320)


@functools.lru_cache(maxsize=None)
def resid_ln_case(name):
    """ivit_linear_resid_ln_fwd: X = R + scale[m / rps] (a w^T + bias) exact, then norm_cases' LayerNorm
    case on that X."""
    M, K, sc, rps, _ = FUSED_LN[name]
    N = kernel_constants()["RP_N"]
    g = torch.Generator().manual_seed(_seed(FUSED_LN, name) + 3)
    a, w, bias, R = _ints(g, (M, K), -8, 8), _ints(g, (N, K), -8, 8), _quarters(g, (N,)), _quarters(g, (M, N))
    scale = row_scale(M, rps) if sc else None
    if scale is not None and M == 1:
        scale = torch.tensor([2.0])   # one row: a scale that is not 1
    prod = a.double() @ w.double().T + bias.double()
    X = R.double() + _expand(scale, M, rps)[:, None] * prod
    budget = (2 * float((a.double().abs() @ w.double().abs().T).max() + 16) + 16) * 8
    ln = NC.ln_case("plain", M, N, LN_EPS, X=X.float())
    return SimpleNamespace(name=name, M=M, N=N, K=K, a=a, w=w, bias=bias, R=R, scale=scale, rps=rps, X=X, budget=budget,
                           ln=ln)


@functools.lru_cache(maxsize=None)
def dgrad_ln_case(name):
    """ivit_linear_dgrad_ln_bwd: G = dy w [K, N] exact (integers), norm_cases' backward case with
    dy := G; mean and rstd are the f64 statistics of X rounded to f32, as the forward hands them on."""
    M, K, sc, rps, alias = FUSED_LN[name]
    N = kernel_constants()["RP_N"]
    g = torch.Generator().manual_seed(_seed(FUSED_LN, name) + 4)
    dy, w = _ints(g, (M, K), -8, 8), _ints(g, (K, N), -8, 8)
    G = dy.double() @ w.double()
    budget = float((dy.double().abs() @ w.double().abs()).max())
    scale = tuple(row_scale(M, rps).tolist()) if sc else None
    ln = NC.ln_case("plain", M, N, LN_EPS, dy_bf16=False, with_dres=True, row_scale=scale, rps=rps, seed=1, dy=G.float())
    return SimpleNamespace(name=name, M=M, N=N, K=K, dy=dy, w=w, G=G, budget=budget, alias=alias, ln=ln, rps=rps)


# ----------------------------------------------------------------------------- ivit_vit_block_wgrad
WB_D = 384
WB_HDS = (384, 768)
WB_MS = (1, 31, 32, 33, 194, 224, 225, 256, 257, 384, 449, 1126)
WB_RESIDUE_M = 4501   # a call on all-8 operands before each empty-split M leaves non-zero LDS behind


def wb_shapes(Hd):
    """(dY columns, X columns) of fc2, fc1, proj, qkv."""
    D = WB_D
    return ((D, Hd), (Hd, D), (D, D), (3 * D, D))


@functools.lru_cache(maxsize=None)
def wb_case(M, Hd):
    """The eight bf16 operands (dy2, a, dh, x2, dyp, o, dyq, x1) as integer f32 tensors and the f64
    dW = dY^T X, db = colsum(dY) of the four linears."""
    g = torch.Generator().manual_seed(49979693 + 1009 * M + Hd)
    ops, ref, budget = [], [], 0.0
    for n, k in wb_shapes(Hd):
        dy, x = _ints(g, (M, n), -8, 8), _ints(g, (M, k), -8, 8)
        ops += [dy, x]
        ref.append((dy.double().T @ x.double(), dy.double().sum(0)))
        budget = max(budget, float((dy.double().abs().T @ x.double().abs()).max()))
    return SimpleNamespace(M=M, Hd=Hd, ops=ops, ref=ref, budget=budget)


# ----------------------------------------------------------------------------- packs
# (rows, cols, transposed) of one ivit_weight_pack_multi launch: plain [N][K] and transposed [K][N] jobs
PACK_JOBS = ((384, 64, 0), (64, 384, 1), (768, 320, 0), (320, 1152, 1), (1152, 128, 0), (128, 384, 1))


def pack_weights():
    g = torch.Generator().manual_seed(86028121)
    return [torch.randn(r, c, generator=g) for r, c, _ in PACK_JOBS]


def pack_ref(w):
    """The row-panel fragment order of W [N][K] (ivit_patch_weight_pack; ivit_weight_pack_t gives the
    same of its operand's transpose): 16-B chunk ((s * N / 16 + nb) * 64 + lane) holds the bf16 of
    W[16 nb + lane % 16][32 s + 8 (lane / 16) .. + 7], rounded to nearest even."""
    N, K = w.shape
    t = w.reshape(N // 16, 16, K // 32, 4, 8).permute(2, 0, 3, 1, 4)
    return t.contiguous().bfloat16().reshape(-1)


# ----------------------------------------------------------------------------- coverage
def coverage():
    """{edge: [case names]} for every edge the case tables must reach."""
    c = kernel_constants()
    E = {n: SimpleNamespace(name=n, dtype=v[0], M=v[1], N=v[2], K=v[3]) for n, v in ENGINE.items()}
    cov = {}

    def put(edge, pred, table=E):
        cov[edge] = [n for n, g in table.items() if pred(g)]

    for d in ("bf16", "f32"):
        bk = c["GBK16"] if d == "bf16" else c["GBK32"]
        bf = d == "bf16"
        for m in ENGINE_MS:
            put(f"{d} M = {m}", lambda g: g.dtype == d and g.M == m)
        for n in ENGINE_NS:
            put(f"{d} N = {n}", lambda g: g.dtype == d and g.N == n)
        for k in ENGINE_KS:
            put(f"{d} K = {k}", lambda g: g.dtype == d and g.K == k)
        put(f"{d} only a partial K tile", lambda g: g.dtype == d and g.K < bk)
        put(f"{d} only full K tiles", lambda g: g.dtype == d and g.K % bk == 0)
        put(f"{d} full K tiles and a tail", lambda g: g.dtype == d and g.K > bk and g.K % bk)
        put(f"{d} N % 8 != 0", lambda g: g.dtype == d and g.N % 8)
        put(f"{d} tiles no multiple of 8", lambda g: g.dtype == d and g.M <= 300 and
            (-(-g.M // c["GBM"]) * -(-g.N // c["GBN"])) % 8 and -(-g.M // c["GBM"]) * -(-g.N // c["GBN"]) > 1)
        grads = lambda g: g.dtype == d and g.N % 8 == 0  # noqa: E731
        put(f"{d} wgrad: an empty split", lambda g: grads(g) and 0 in engine_split_rows(g.M, g.N, g.K, bf))
        put(f"{d} wgrad: a partial split", lambda g: grads(g) and any(
            0 < r < engine_chunk(g.M, engine_splits(g.M, g.N, g.K, bf), bf) for r in engine_split_rows(g.M, g.N, g.K, bf)[1:]))
        put(f"{d} wgrad: splits, none empty", lambda g: grads(g) and engine_splits(g.M, g.N, g.K, bf) > 1 and
            0 not in engine_split_rows(g.M, g.N, g.K, bf))
        put(f"{d} wgrad: tiles x splits no multiple of 8", lambda g: grads(g) and engine_splits(g.M, g.N, g.K, bf) > 1 and
            (-(-g.N // c["GBM"]) * -(-g.K // c["GBN"]) * engine_splits(g.M, g.N, g.K, bf)) % 8)
        put(f"{d} wgrad: one split", lambda g: grads(g) and engine_splits(g.M, g.N, g.K, bf) == 1)
        put(f"{d} wgrad: M below one K tile", lambda g: grads(g) and g.M < bk)
        put(f"{d} gelu epilogues", lambda g: g[0] == d, ENGINE_GELU)
    P = {n: SimpleNamespace(M=v[0], N=v[1], K=v[2]) for n, v in PANEL.items()}
    for m in PANEL_MS:
        put(f"panel M = {m}", lambda g: g.M == m, P)
    for n in PANEL_NS:
        put(f"panel N = {n}", lambda g: g.N == n, P)
    for k in PANEL_KS:
        put(f"panel K = {k}", lambda g: g.K == k, P)
    L = {n: SimpleNamespace(M=v[0], K=v[1], sc=v[2], rps=v[3], alias=v[4]) for n, v in FUSED_LN.items()}
    for m in FUSED_MS:
        put(f"fused LN M = {m}", lambda g: g.M == m, L)
    for k in FUSED_KS:
        put(f"fused LN K = {k}", lambda g: g.K == k, L)
    put("fused LN no scale", lambda g: not g.sc, L)
    put("fused LN rps = 1", lambda g: g.sc and g.rps == 1 and g.M > 1, L)
    put("fused LN rps = 5", lambda g: g.sc and g.rps == 5, L)
    put("fused LN rps = M", lambda g: g.sc and g.rps == g.M and g.M > 1, L)
    put("fused LN dX aliases dres", lambda g: g.alias, L)
    put("fused LN dX apart from dres", lambda g: not g.alias, L)
    for form in PANEL_FORMS:
        for knob in PANEL_KNOBS:
            cov[f"panel {form} knob {knob}: LDS-tile epilogue"] = [
                ld for ld in PANEL_LDS if not wide_transposed(knob, form, ld % 8 == 0)]
            if wide_transposed(knob, form, True):
                cov[f"panel {form} knob {knob}: transposed epilogue"] = [ld for ld in PANEL_LDS if ld % 8 == 0]
    return cov
