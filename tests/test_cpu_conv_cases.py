"""tests/conv_cases.py held to account without a GPU: torch's own f32 CPU convolution, unfold and
fold return the bits of the f64 references on every case (which proves the exactness budget and
the references), the budgets hold, the outputs are large enough that a bf16 accumulation would
show, the f32 operands are not bf16-exact, the dispatch mirror follows the kernel sources and
the library, and every path has a case at each of its edges."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import conv_cases as CC

NAMES = sorted(CC.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_f32_cpu_conv_equals_f64_and_budget(name):
    c = CC.conv_case(name)
    assert max(c.budget.values()) < CC.LIMIT, c.budget
    t32 = CC.conv_refs(c.x, c.w, c.bias, c.dy, c.dyw, c.B, c.H, c.W, dt=torch.float32)
    for n in ("y", "dx", "dw", "db"):
        assert t32[n].dtype == torch.float32 and c.ref[n].dtype == torch.float64
        assert torch.equal(t32[n].double(), c.ref[n]), (name, n)
    assert torch.equal(c.ref["y0"] + c.bias.double(), c.ref["y"])
    # the operands are exact in the case's compute dtype
    if c.dtype == "bf16":
        for t in (c.x, c.w, c.dy):
            assert torch.equal(t.bfloat16().float(), t)
            assert float(t.abs().max()) <= 8 and torch.equal(t, t.round())
    assert float(c.bias.abs().max()) <= 16 and torch.equal(c.bias * 4, (c.bias * 4).round())


def test_head_case_exact():
    h = CC.head_case()
    assert h.budget["dx"] < CC.LIMIT
    dyr = h.dy[:, :h.Cw].reshape(h.B, h.H, h.W, h.Cw).permute(0, 3, 1, 2)
    t32 = F.conv_transpose2d(dyr, h.w, padding=h.k // 2).permute(0, 2, 3, 1).reshape(h.M, h.Cin)
    assert torch.equal(t32.double(), h.ref["dx"])
    assert not h.dy[:, h.Cw:].any()
    # the shape reaches ivit_conv_dgrad_t only through the zero padding to 128 channels
    assert not CC.dgrad_t_ok("bf16", h.M, h.Cin, h.Cp, h.Cq, h.k)
    assert CC.dgrad_t_ok("bf16", h.M, h.Cin, h.Cq, h.Cq, h.k)


@pytest.mark.parametrize("name", [n for n in NAMES if CC.CASES[n][0] == "bf16"
                                  and CC.CASES[n][6] ** 2 * CC.CASES[n][4] >= 576])
def test_outputs_exceed_bf16_integers(name):
    """A third of y and of dw above 256 wherever the sums are long enough (conv_cases' docstring): a
    kernel that accumulated in bf16 could not return them."""
    c = CC.conv_case(name)
    ny, nw = CC.term_counts(name)
    if ny >= CC.MAG_TERMS:
        assert float((c.ref["y"].abs() > 256).double().mean()) >= 1 / 3
    if nw >= CC.MAG_TERMS:
        assert float((c.ref["dw"].abs() > 256).double().mean()) >= 1 / 3


def test_magnitude_check_reaches_every_large_map():
    """The term-count condition leaves out only maps with fewer than 256 pixels or smaller than the kernel."""
    for n in NAMES:
        dtype, B, H, W, Cin, Cout, k = CC.CASES[n]
        if dtype == "bf16" and k * k * Cin >= 576 and H >= k and W >= k and B * H * W >= 255:
            ny, nw = CC.term_counts(n)
            assert ny >= CC.MAG_TERMS and nw >= CC.MAG_TERMS, (n, ny, nw)


@pytest.mark.parametrize("name", [n for n in NAMES if CC.CASES[n][0] == "f32"])
def test_f32_operands_are_not_bf16_exact(name):
    c = CC.conv_case(name)
    assert not torch.equal(c.w.bfloat16().float(), c.w)      # forward and data gradient
    assert not torch.equal(c.dyw.bfloat16().float(), c.dyw)  # weight gradient
    # and rounding them would change every output
    w16, d16 = c.w.bfloat16().float(), c.dyw.bfloat16().float()
    r16 = CC.conv_refs(c.x, w16, c.bias, c.dy, d16, c.B, c.H, c.W)
    for n in ("y", "dx", "dw", "db"):
        assert not torch.equal(r16[n], c.ref[n]), (name, n)


def test_constants_come_from_the_sources():
    k = CC.kernel_constants()
    eng = open(os.path.join(CC.CSRC, "gemm_engine.h")).read()
    pan = open(os.path.join(CC.CSRC, "conv_panel.hip")).read()
    for n in ("GBM", "GBN", "GBK16", "GBK32"):
        assert re.search(r"\b%s = %d\b" % (n, k[n]), eng), n
    for n in ("CP_BM", "CP_BN", "CW_BK"):
        assert re.search(r"\b%s = %d\b" % (n, k[n]), pan), n
    # the mirror's predicates are the ones in the source text
    assert "M >= CP_BM && N >= 128 && N % 8 == 0 && Cin % 64 == 0 && lda % 8 == 0" in pan
    assert "M >= 256 && Cout >= 128 && Cout % 8 == 0 && Cin % 8 == 0 && lddy % 8 == 0" in pan
    assert "ks * ks * Cin >= 128" in pan and "long s = 256 / tiles;" in pan and "s = steps / 4" in pan
    assert "Cin % 64 == 0 && R > 0" in eng and "Cout % 64 == 0 && C >= 8" in eng
    assert k["CP_BM"] == 288 and k["GBM"] == 128  # the case table's M edges (287..289, 128, 129) are literal


def test_dgrad_t_rejects_what_the_mirror_rejects():
    """ivit_conv_dgrad_t returns IVIT_ERR_ARG before any launch (so without a device) for a shape
    conv_panel_ok rejects; the header documents the conditions."""
    from _lib import BF16, F32, lib
    dll = lib.load()
    BM = CC.kernel_constants()["CP_BM"]
    # (B, H, W, Cout, Cin, ks, lddy)
    bad = [(1, 1, BM - 1, 128, 128, 3, 128), (1, 1, BM, 128, 120, 3, 128), (1, 1, BM, 72, 128, 3, 72),
           (1, 1, BM, 128, 128, 2, 128), (1, 1, BM, 128, 128, 3, 132), (1, 1, BM, 128, 132, 3, 128)]
    for B, H, W, Cout, Cin, ks, lddy in bad:
        assert not CC.panel_ok(B * H * W, Cin, Cout, lddy, ks)
        rc = dll.ivit_conv_dgrad_t(BF16, None, lddy, B, H, W, Cout, None, Cin, ks, None, F32, None)
        assert rc == -1, (B, H, W, Cout, Cin, ks, lddy, rc)
    assert dll.ivit_conv_dgrad_t(F32, None, 128, 1, 1, BM, 128, None, 128, 3, None, F32, None) == -1
    hdr = open(os.path.join(CC.REPO, "include", "ivit.h")).read()
    doc = hdr[hdr.index("Data gradient on the transposed"):hdr.index("int ivit_conv_dgrad_t")]
    for cond in ("Cout % 64 == 0", "Cin >= 128", "Cin % 8 == 0", "lddy % 8 == 0", "B*H*W >= 288"):
        assert cond in doc, cond


def test_im2col_rejects_a_map_smaller_than_the_kernel():
    """H + 2 pad < k has no output (nn.Conv2d raises); C's truncating division would make Ho = 1 of it."""
    from _lib import F32, lib
    dll = lib.load()
    assert CC.out_size(1, 1, 2, 2, 0) is None
    assert dll.ivit_im2col(F32, None, 1, 1, 1, 8, 2, 2, 0, 1, 1, None, 32, F32, None) == -1
    assert dll.ivit_col2im(None, 32, 1, 1, 1, 8, 2, 2, 0, 1, 1, None, None) == -1
    assert dll.ivit_col2im(None, 8 * 513, 1, 4, 4, 513, 1, 1, 0, 4, 4, None, None) == -1


def test_every_path_has_a_case_at_each_edge():
    cov = CC.coverage()
    empty = [k for k, v in cov.items() if not v]
    assert not empty, empty
    paths = {p for p, _ in cov}
    assert paths == {"fwd:engine_f32", "fwd:engine_gather", "fwd:engine_dma", "fwd:panel", "dgrad:engine_f32",
                     "dgrad:engine_gather", "dgrad:engine_dma", "dgrad:panel_t", "wgrad:engine_f32",
                     "wgrad:engine_bf16", "wgrad:panel"}
    edges = {e for _, e in cov}
    for e in ["map (2,1,2) k=1", "map (2,1,2) k=3", "map (2,1,2) k=5", "map (3,2,1) k=1", "map (3,2,1) k=3",
              "map (3,2,1) k=5", "map (3,2,49) k=5", "map (1,1,289) k=5", "border (37,3,3) k=5", "border (5,8,8) k=5",
              "M = 287 (panel declines)", "M = 287 (panel_t declines)", "M = 288", "M = 289",
              "M = 255 (panel declines)", "M = 256", "M = 257", "M = 128", "M = 129", "W = 65 (qW = 0)",
              "W = 64 (rW = 0)", "W = 1", "(20,5,3): H * W < 64", "empty last split", "Cout = 8", "Cout = 40",
              "Cout = 120", "Cout = 128", "Cout = 136", "Cout = 264", "Cout = 384", "Cin = 8", "Cin = 24", "Cin = 48",
              "Cin = 64", "Cin = 128", "Cin = 192", "Cin = 128 (minimum)", "K = 72 (no multiple of GBK32)", "K = 8",
              "K = 216", "two N tiles"]:
        assert e in edges, e
    # the pairs of the issue's table, spelled out
    must = [("fwd:panel", "M = 288"), ("fwd:panel", "M = 289"), ("dgrad:panel_t", "M = 288"),
            ("dgrad:panel_t", "M = 289"), ("wgrad:panel", "M = 256"), ("wgrad:panel", "M = 257"),
            ("fwd:engine_f32", "M = 128"), ("fwd:engine_f32", "M = 129"), ("fwd:engine_dma", "M = 128"),
            ("fwd:engine_dma", "M = 129"), ("fwd:engine_gather", "M = 128"), ("fwd:engine_gather", "M = 129"),
            ("wgrad:panel", "empty last split"), ("wgrad:panel", "W = 1"), ("fwd:panel", "Cout = 136"),
            ("fwd:panel", "Cout = 264"), ("fwd:panel", "Cout = 384"), ("wgrad:panel", "Cin = 8"),
            ("wgrad:panel", "Cin = 24"), ("wgrad:panel", "Cin = 48"), ("fwd:panel", "Cin = 192"),
            ("fwd:panel", "border (37,3,3) k=5"), ("dgrad:panel_t", "map (1,1,289) k=5"),
            ("dgrad:panel_t", "border (37,3,3) k=5"), ("dgrad:panel_t", "border (5,8,8) k=5"),
            ("fwd:panel", "border (5,8,8) k=5"), ("wgrad:panel", "border (5,8,8) k=5"),
            ("wgrad:engine_f32", "more than one split"), ("wgrad:engine_bf16", "more than one split"),
            ("wgrad:engine_f32", "one split"), ("wgrad:engine_bf16", "one split")]
    for pe in must:
        assert cov.get(pe), pe


@pytest.mark.parametrize("name", NAMES)
def test_wgrad_split_mirror_agrees_with_the_library(name):
    """ivit_conv_wgrad_workspace sizes its slab for the largest of the three split counts (the engine's
    f32 and bf16 choice, the panel's): splits * Cout * K * 4 bytes + max(splits * Cout * 4, the column
    sum's workspace). Without a device the engine's cost model assumes 256 CUs, as the mirror does."""
    from _lib import lib
    dll = lib.load()
    g = CC._geom(name)
    s = CC.wgrad_workspace_splits(g.M, g.Cout, g.K)
    cw = dll.ivit_colsum_workspace(g.M, g.Cout)
    assert dll.ivit_conv_wgrad_workspace(g.B, g.H, g.W, g.Cin, g.Cout, g.k) == \
        s * g.Cout * g.K * 4 + max(s * g.Cout * 4, cw)


def test_wgrad_engine_split_mirror_is_the_source():
    ops = open(os.path.join(CC.CSRC, "gemm_ops.hip")).read()
    for txt in ("return 2L * cus;", "cus = 256;", "for (int s = 1; s <= 128; ++s) {", "if (s > 1 && kt / s < 8.0) break;",
                "const double cost = rounds * (kt / s + 4.0);", "if (cost < best_cost - 1e-9)",
                "const long tiles = (long)ivit_cdiv(Mo, GBM) * ivit_cdiv(No, GBN);",
                "return splitk_choice(tiles, Kr, bf ? GBK16 : GBK32);"):
        assert txt in ops, txt
    # the engine's bf16 weight gradient of the empty-split shape (the knob off) takes three splits
    g = CC._geom("empty_split")
    assert CC.wgrad_engine_splits(g.M, g.Cout, g.K, True) == 3


def test_empty_split_case_has_one():
    g = CC._geom("empty_split")
    s, chunk = CC.wgrad_panel_splits(g.M, g.Cout, g.K), CC.wgrad_panel_chunk(g.M, g.Cout, g.K)
    assert CC.wgrad_path("bf16", g.M, g.Cin, g.Cout, g.k) == "panel"
    assert s > 1 and (s - 1) * chunk >= g.M and (s - 2) * chunk < g.M


def _cols_combos():
    for k, s, p in CC.COLS_GEOMS:
        for H, W in CC.COLS_MAPS:
            if CC.out_size(H, W, k, s, p) is not None:
                yield k, s, p, H, W


def test_unfold_fold_f32_equal_f64():
    """torch's f32 unfold / fold return the references' bits: im2col is a copy, and col2im on integer
    dcols has no rounding. A pixel no window covers is 0 (k = 1, s = 2)."""
    assert sum(1 for _ in _cols_combos()) == len(CC.COLS_GEOMS) * len(CC.COLS_MAPS) - 1  # (2, 2, 0) on (1, 1)
    g = torch.Generator().manual_seed(5)
    for k, s, p, H, W in _cols_combos():
        for C in (1, 3, 65):
            x = CC.cols_x(CC.COLS_B, H, W, C)
            ref = CC.im2col_ref(x, k, s, p)
            Ho, Wo = CC.out_size(H, W, k, s, p)
            assert ref.shape == (CC.COLS_B * Ho * Wo, k * k * C)
            u32 = F.unfold(x.permute(0, 3, 1, 2), k, padding=p, stride=s)
            u32 = u32.reshape(CC.COLS_B, C, k * k, -1).permute(0, 3, 2, 1).reshape(ref.shape)
            assert torch.equal(u32.double(), ref)
            # the definition, at one entry per tap: cols[(b, oy, ox)][(ky * k + kx) * C + c]
            b, oy, ox, c = CC.COLS_B - 1, Ho - 1, Wo - 1, C - 1
            for ky in range(k):
                for kx in range(k):
                    y, xx = oy * s - p + ky, ox * s - p + kx
                    want = float(x[b, y, xx, c]) if 0 <= y < H and 0 <= xx < W else 0.0
                    assert float(ref[(b * Ho + oy) * Wo + ox, (ky * k + kx) * C + c]) == want
            d = torch.randint(-8, 9, ref.shape, generator=g).float()
            dref = CC.col2im_ref(d, CC.COLS_B, H, W, C, k, s, p)
            assert torch.equal(CC.col2im_ordered_f32(d, CC.COLS_B, H, W, C, k, s, p).double(), dref)
            # fold is the adjoint of unfold
            assert float((dref * x.double()).sum()) == pytest.approx(float((d.double() * ref).sum()), rel=1e-12)
            if (k, s) == (1, 2) and H > 1:
                assert not dref[:, 1].any()


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("i", range(len(CC.STRIDED)))
def test_strided_cases_exact(i, dtype):
    c = CC.strided_case(i, dtype)
    assert max(c.budget.values()) < CC.LIMIT, c.budget
    x, w, b = (t.clone().requires_grad_(True) for t in (c.x, c.w, c.bias))
    y = F.conv2d(x, w, b, stride=c.s, padding=c.p)
    (dx,) = torch.autograd.grad(y, x, c.dy, retain_graph=True)
    dw, db = torch.autograd.grad(y, (w, b), c.dyw)
    for n, t in (("y", y.detach()), ("dx", dx), ("dw", dw), ("db", db)):
        assert torch.equal(t.double(), c.ref[n]), n
    if dtype == "f32":
        assert not torch.equal(c.w.bfloat16().float(), c.w)
        assert not torch.equal(c.dyw.bfloat16().float(), c.dyw)
        # rounding the weight gradient's operand to bf16 would change dw and db
        r16 = F.conv2d(x, w, b, stride=c.s, padding=c.p)
        dw16, db16 = torch.autograd.grad(r16, (w, b), c.dyw.bfloat16().float())
        assert not torch.equal(dw16.double(), c.ref["dw"]) and not torch.equal(db16.double(), c.ref["db"])
    else:
        assert c.dyw is c.dy


def test_pack_refs():
    w = torch.arange(2 * 3 * 3 * 3, dtype=torch.float32).reshape(2, 3, 3, 3)
    p, t = CC.pack_ref(w, 4), CC.pack_t_ref(w, 5)
    assert p.shape == (4, 3, 3, 3) and t.shape == (3, 3, 3, 5)
    assert float(p[1, 2, 0, 1]) == float(w[1, 1, 2, 0]) and not p[2:].any()
    assert float(t[1, 0, 2, 1]) == float(w[1, 1, 2, 0]) and not t[..., 2:].any()


def test_bn_offset_inputs_are_offset():
    B, H, W, Cin, Cout, k, _ = CC.BN_OFFSET_SHAPE
    x, w, _, _ = CC.bn_offset_inputs(B, H, W, Cin, Cout, k)
    y = x.double() @ w.double().reshape(Cout, Cin).T
    ratio = y.mean(0).abs() / y.std(0)
    assert float(ratio.min()) > 50 and float(ratio.median()) > 80
