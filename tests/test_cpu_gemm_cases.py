"""tests/gemm_cases.py held to account without a GPU: the exactness budgets, torch's own f32 CPU matmul
against the f64 references, the magnitude check, the dispatch mirrors against the kernel sources and the
library, and a case at every edge the GPU tests are to reach."""
import os
import re

import pytest
import torch

import conv_cases as CC
import gemm_cases as GC

ENGINE_NAMES = sorted(GC.ENGINE)


def _mm32(a, b):
    return (a.float() @ b.float()).double()


@pytest.mark.parametrize("name", ENGINE_NAMES)
def test_engine_case_budget_and_f32_equals_f64(name):
    c = GC.lin_case(name)
    assert max(c.budget.values()) < GC.LIMIT, c.budget
    assert torch.equal(_mm32(c.x, c.w.T), c.ref["y0"])
    assert torch.equal((c.x @ c.w.T + c.bias).double(), c.ref["y"])
    assert torch.equal(_mm32(c.dy, c.w), c.ref["dx"])
    assert torch.equal(_mm32(c.dyw.T, c.x), c.ref["dw"])
    assert torch.equal(c.dyw.sum(0).double(), c.ref["db"])
    assert torch.equal((c.dyw.T @ c.x + c.dw0).double(), c.ref["dw"] + c.dw0.double())
    for cols in GC.QS_COLS(c.N):
        y = c.x @ c.w.T + c.bias
        y[:, :cols] *= GC.QSCALE
        assert torch.equal(y.double(), GC.qs_ref(c, cols))
    for rps in GC.RPS_OF(c.M):
        s = GC.row_scale(c.M, rps)
        y = c.resid + s[torch.arange(c.M) // rps][:, None] * (c.x @ c.w.T + c.bias)
        assert torch.equal(y.double(), GC.resid_ref(c, s, rps))
    # every reference is a value f32 holds, and a bf16 output's reference rounds from it
    for r in c.ref.values():
        assert torch.equal(r.float().double(), r)


@pytest.mark.parametrize("name", [n for n in ENGINE_NAMES if GC.ENGINE[n][0] == "f32"])
def test_f32_operands_are_not_bf16_exact(name):
    c = GC.lin_case(name)
    assert not torch.equal(c.w.bfloat16().float(), c.w)      # forward and data gradient
    assert not torch.equal(c.dyw.bfloat16().float(), c.dyw)  # weight gradient
    assert torch.equal(c.x.bfloat16().float(), c.x) and torch.equal(c.dy.bfloat16().float(), c.dy)


@pytest.mark.parametrize("name", [n for n in ENGINE_NAMES if GC.ENGINE[n][0] == "bf16"])
def test_bf16_operands_are_bf16_exact(name):
    c = GC.lin_case(name)
    for t in (c.x, c.w, c.dy):
        assert torch.equal(t.bfloat16().float(), t)


def _third_above_256(t):
    return float((t.abs() > 256).double().mean()) >= 1.0 / 3.0


def test_outputs_exceed_bf16_integers():
    """A third of the outputs above 256 wherever the sums have at least MAG_TERMS terms: a kernel that
    accumulated in bf16 could not return them. Every family has such a case."""
    seen = set()
    for n in ENGINE_NAMES:
        c = GC.lin_case(n)
        if c.dtype != "bf16":
            continue
        for out, terms in (("y0", c.K), ("dx", c.N), ("dw", c.M)):
            if terms >= GC.MAG_TERMS:
                assert _third_above_256(c.ref[out]), (n, out)
                seen.add(out)
    assert seen == {"y0", "dx", "dw"}
    for n in GC.PANEL:
        c = GC.panel_case(n)
        if c.K >= GC.MAG_TERMS:
            assert _third_above_256(c.y0), n
            seen.add("panel")
    for n in GC.FUSED_LN:
        c, d = GC.resid_ln_case(n), GC.dgrad_ln_case(n)
        if c.K >= GC.MAG_TERMS:
            assert _third_above_256(d.G), n
            seen.add("ln")
    for Hd in GC.WB_HDS:
        for M in GC.WB_MS:
            if M >= GC.MAG_TERMS:
                assert all(_third_above_256(dw) for dw, _ in GC.wb_case(M, Hd).ref), (M, Hd)
                seen.add("wb")
    assert {"panel", "ln", "wb"} <= seen


@pytest.mark.parametrize("name", sorted(GC.ENGINE_GELU))
def test_gelu_cases(name):
    c = GC.gelu_case(name)
    assert max(c.budget.values()) < GC.LIMIT, c.budget
    assert torch.equal((c.x @ c.w.T + c.bias).double(), c.z)
    assert torch.equal(_mm32(c.dy, c.w2), c.acc)
    inside = float((c.z.abs() < 4).double().mean())
    assert 0.68 <= inside <= 0.86, inside   # a standard deviation of 3 to 4
    assert float(c.z.abs().max()) <= 24     # erf_as's documented error stays inside ACT_TOL
    if c.dtype == "bf16":
        for t in (c.x, c.w, c.dy, c.w2, c.pre):
            assert torch.equal(t.bfloat16().float(), t)
    else:
        assert not torch.equal(c.w.bfloat16().float(), c.w) and not torch.equal(c.w2.bfloat16().float(), c.w2)


@pytest.mark.parametrize("name", sorted(GC.PANEL))
def test_panel_cases(name):
    c = GC.panel_case(name)
    assert max(c.budget.values()) < GC.LIMIT, c.budget
    assert torch.equal(_mm32(c.a, c.w.T), c.y0)
    for q in GC.QCOLS(c.N):
        y = c.a @ c.w.T + c.bias
        y[:, :q] *= GC.QSCALE
        assert torch.equal(y.double(), GC.panel_none_ref(c, q))
    assert torch.equal((c.a @ (c.w / c.div).T + c.bias_g).double(), c.z)
    assert torch.equal(((c.a @ c.w.T) * c.G).double(), c.y0 * c.G.double())
    inside = float((c.z.abs() < 4).double().mean())
    assert (0.68 if c.K != 128 else 0.62) <= inside <= 0.86 or c.M == 1, inside   # K = 128: 4.2, see gemm_cases
    for t in (c.a, c.w / c.div, c.pre, c.G):
        assert torch.equal(t.bfloat16().float(), t)
    assert float(c.G.abs().max()) <= 1.0


@pytest.mark.parametrize("name", sorted(GC.FUSED_LN))
def test_fused_ln_cases(name):
    c, d = GC.resid_ln_case(name), GC.dgrad_ln_case(name)
    assert c.budget < GC.LIMIT and d.budget < GC.LIMIT
    s = torch.ones(c.M) if c.scale is None else c.scale[torch.arange(c.M) // c.rps]
    assert torch.equal((c.R + s[:, None] * (c.a @ c.w.T + c.bias)).double(), c.X)
    assert torch.equal(c.ln.X.double(), c.X)                 # norm_cases' LayerNorm input is the exact X
    assert torch.equal(_mm32(d.dy, d.w), d.G) and torch.equal(d.ln.dy.double(), d.G)
    assert (c.scale is not None) == GC.FUSED_LN[name][2]
    # norm_cases' own bounds, unchanged: tolerances from torch's f32 on the same case, never below the floor
    for ln in (c.ln, d.ln):
        assert all(t >= 2e-6 for t in ln.tol.values())


@pytest.mark.parametrize("Hd", GC.WB_HDS)
def test_wb_cases(Hd):
    for M in GC.WB_MS:
        c = GC.wb_case(M, Hd)
        assert c.budget < GC.LIMIT
        for q, (n, k) in enumerate(GC.wb_shapes(Hd)):
            dy, x = c.ops[2 * q], c.ops[2 * q + 1]
            assert dy.shape == (M, n) and x.shape == (M, k)
            assert torch.equal(_mm32(dy.T, x), c.ref[q][0]) and torch.equal(dy.sum(0).double(), c.ref[q][1])
    assert 64.0 * GC.WB_RESIDUE_M < GC.LIMIT


def test_wb_split_mirror():
    """Which token counts have a split that starts past M, by the mirror of wb_splits: the ranges the
    case list is built on, the set of the list's own M, and what the host launches now."""
    bk, smax = GC.kernel_constants()["WB_BK"], GC.kernel_constants()["WB_SMAX"]
    assert (bk, smax) == (32, 7)
    steps_with = {s for s in range(1, 60) if GC.wb_empty(s * bk)}
    assert steps_with == set(range(8, 13)) | set(range(15, 19)) | {22, 23, 24, 29, 30, 36}
    assert [M for M in GC.WB_MS if GC.wb_empty(M)] == [225, 256, 257, 384, 449, 1126]
    assert GC.wb_empty(225) == 3 and GC.wb_empty(1126) == 1      # 8 steps: 4 splits of 2; 36: 6 of 6
    assert not GC.wb_empty(GC.WB_RESIDUE_M)
    for M in list(range(1, 1300)) + [4501, 36008]:
        S, ch = GC.wb_launched(M), GC.wb_chunk(M)
        assert 1 <= S <= GC.wb_splits(M) and (S - 1) * ch < M <= S * ch, M   # every launched split has tokens
        assert S == GC.wb_splits(M) - GC.wb_empty(M)
    assert GC.wb_launched(36008) == 7 and GC.wb_chunk(36008) == 161 * bk     # the bench shape: as before
    src = open(os.path.join(GC.CSRC, "wgrad_block.hip")).read()
    for txt in ("return (int)(steps < WB_SMAX ? (steps > 0 ? steps : 1) : WB_SMAX);",
                "const long csteps = (steps + wb_splits(M) - 1) / wb_splits(M);",
                "const int S = (int)((steps + csteps - 1) / csteps);", "const int kchunk = (int)csteps * WB_BK;",
                "if (dob && nk > 0) bias(0);"):
        assert txt in src, txt


def test_wb_workspace_mirror_agrees_with_the_library():
    from _lib import lib
    dll = lib.load()
    for Hd in GC.WB_HDS:
        for M in GC.WB_MS:
            D = GC.WB_D
            nw, nb = 2 * D * Hd + 4 * D * D, 5 * D + Hd
            assert dll.ivit_vit_block_wgrad_workspace(M, D, Hd) == GC.wb_splits(M) * (nw + 2 * nb) * 4 + 256


def test_engine_split_mirror():
    """The weight-gradient shapes take the splits the case list says: computed with the kernel's own cost
    model at 512 resident workgroups (what the library assumes without a device too)."""
    rows = GC.engine_split_rows(8250, 136, 72, True)
    assert len(rows) == 16 and rows[-1] == 0 and rows[-2] == 186 and set(rows[:-2]) == {576}
    rows = GC.engine_split_rows(8250, 136, 72, False)
    assert len(rows) == 64 and rows.count(0) == 6 and min(r for r in rows if r) < max(rows)
    rows = GC.engine_split_rows(2100, 136, 72, True)
    assert len(rows) == 4 and 0 not in rows and sum(rows) == 2100
    assert GC.engine_split_rows(5, 136, 72, True) == [5] and GC.engine_split_rows(5, 136, 72, False) == [5]
    eng = open(os.path.join(GC.CSRC, "gemm_engine.h")).read()
    ops = open(os.path.join(GC.CSRC, "gemm_ops.hip")).read()
    for txt in ("int kchunk = ivit_cdiv(ivit_cdiv(K, splits), bk) * bk;", "if (kchunk <= 0) kchunk = bk;",
                "const int kbeg = split * kchunk, kend = min(K, kbeg + kchunk);"):
        assert txt in eng, txt
    for txt in ("const int splits = (int)wgrad_splits(N, K, M, bf);", "return 2L * cus;", "cus = 256;",
                "if (s > 1 && kt / s < 8.0) break;", "const double cost = rounds * (kt / s + 4.0);"):
        assert txt in ops, txt
    assert CC.ENGINE_SLOTS == 512


@pytest.mark.parametrize("name", [n for n in ENGINE_NAMES if GC.ENGINE[n][2] % 8 == 0])
def test_engine_workspace_mirror_agrees_with_the_library(name):
    from _lib import lib
    _, M, N, K = GC.ENGINE[name]
    s = max(GC.engine_splits(M, N, K, True), GC.engine_splits(M, N, K, False))
    cw = -(-M // 256) * N * 4
    assert lib.load().ivit_linear_wgrad_workspace(M, N, K) == s * N * K * 4 + max(s * N * 4, cw)


def test_constants_come_from_the_sources():
    k = GC.kernel_constants()
    assert k == {"GBM": 128, "GBN": 128, "GBK16": 64, "GBK32": 16, "RP_MT": 144, "RP_N": 384, "WB_BK": 32, "WB_SMAX": 7}
    assert {n: k[n] for n in ("GBM", "GBN", "GBK16", "GBK32")} == {n: CC.kernel_constants()[n] for n in
                                                                  ("GBM", "GBN", "GBK16", "GBK32")}
    pan = open(os.path.join(GC.CSRC, "rowpanel.hip")).read()
    for txt in ("ev1 = ev1 && mode != 0 && (EPI == EPI_QS || EPI == EPI_GELUD || mode == 2);",
                "return p == nullptr || (((uintptr_t)p & 15) == 0 && ld % 8 == 0);"):
        assert txt in pan, txt
    # the shapes follow the tiles
    assert set(GC.ENGINE_MS) >= {k["GBM"] - 1, k["GBM"], k["GBM"] + 1}
    assert set(GC.PANEL_MS) >= {k["RP_MT"] - 1, k["RP_MT"], k["RP_MT"] + 1, 2 * k["RP_MT"] + 1}
    assert all(n % k["RP_N"] == 0 for n in GC.PANEL_NS)
    assert set(GC.WB_MS) >= {k["WB_BK"] - 1, k["WB_BK"], k["WB_BK"] + 1, 7 * k["WB_BK"], 7 * k["WB_BK"] + 1}
    el = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_elementwise.py")).read()
    m = re.search(r"^ACT_TOL = (\S+)", el, flags=re.M)
    assert m and float(m.group(1)) == GC.ACT_TOL


def test_every_edge_has_a_case():
    cov = GC.coverage()
    empty = [k for k, v in cov.items() if not v]
    assert not empty, empty
    # the forms and knob values: every form runs under each knob value at an unaligned and an aligned ld
    assert GC.wide_transposed(1, "none", True) and GC.wide_transposed(1, "gelu_d", True)
    assert not GC.wide_transposed(1, "gelu", True) and not GC.wide_transposed(1, "dmul", True)
    assert all(GC.wide_transposed(2, f, True) and not GC.wide_transposed(2, f, False) for f in GC.PANEL_FORMS)
    assert not any(GC.wide_transposed(0, f, True) for f in GC.PANEL_FORMS)
    assert all(q % GC.kernel_constants()["RP_N"] == 0 for n in GC.PANEL_NS for q in GC.QCOLS(n))
    assert GC.QS_COLS(136) == [0, 8, 136] and GC.QS_COLS(200) == [0, 8, 136, 200] and GC.QS_COLS(7) == [0]


def test_pack_jobs_mix_plain_and_transposed():
    kinds = {t for _, _, t in GC.PACK_JOBS}
    assert kinds == {0, 1} and len({r * c for r, c, _ in GC.PACK_JOBS}) > 2
    for r, c, t in GC.PACK_JOBS:
        n, k = (c, r) if t else (r, c)
        assert n % 384 == 0 or n % 192 == 0
        assert k % 64 == 0
