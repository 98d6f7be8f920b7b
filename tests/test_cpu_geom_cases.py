"""Box geometry primitives, CPU side: the references of tests/geom_cases.py against each other, the
distances of the cases from the guards, planted defects in Python restatements of the four
kernels (every one must be rejected by the committed cases under the committed bounds), and the
host build of csrc/geom.h under AddressSanitizer + UBSan (tools/geom_host.cpp, a stand-alone
program run as a child process) under the same bounds as the device.

Planted defects that no case can reject:
  * the union guard (u <= 1e-6 -> 0) dropped. With both areas >= 1e-6 and the intersection at most
    the smaller area, u = A1 + A2 - inter >= max(A1, A2) >= 1e-6: only A1 = A2 = inter = 1e-6 to the
    last bit reaches it, and a NaN is caught by the intersection guard before it. The guard is
    unreachable, so its removal changes no output; test_union_guard_is_unreachable records that.
Cases added because a defect needed them: "negative_size" (one negative size makes rect_poly's
corners clockwise; nothing else reaches make_ccw), the (16, 16, 5) anchor grid with an odd stride
(integer stride // 2), decode rows beyond +-pi (a missing wrap passes a comparison modulo 2 pi and
fails the range check).
"""
import math
import os
import subprocess

import numpy as np
import pytest

import geom_cases as G
from conftest import PKG, REPO

F32 = np.float32
RATIOS = {}


def _note(family, ratio):
    """Print a measured err / bound (pytest -s shows it; profiles/geom_parity.txt records a run)."""
    RATIOS[family] = ratio
    print(f"err / bound {family}: {ratio:.3g}")
    return ratio


# ============================================================================ the references themselves
def test_exact_rational_clip_agrees_with_the_oracle():
    worst = 0.0
    sets = {**G.rot_families(), **{f"shape_{a}x{b}": v for (a, b), v in G.rot_shapes().items()}}
    for name, (b1, b2, ref) in sets.items():
        orc = G.RotRef(b1, b2, exact=False)
        d = float(np.abs(ref.val - orc.val).max())
        worst = max(worst, d)
        assert d <= 1e-12, (name, d)
        # and against the oracle's own entry point, which rounds to f32
        with np.errstate(all="ignore"):
            m = G.O.rotated_iou_numpy(b1, b2)
        assert np.array_equal(m, orc.val.astype(F32)), name
    print(f"exact rational clip vs oracle f64: {worst:.3g}")


def test_bounded_cases_keep_their_distance_from_the_guards():
    n = 0
    for name in G.CLEAN_FAMILIES:
        ref = G.rot_families()[name][2]
        assert ref.clean().all(), (name, np.argwhere(~ref.clean())[:3])
        n += ref.val.size
    for shape, (_, _, ref) in G.rot_shapes().items():
        assert ref.clean().all(), (shape, np.argwhere(~ref.clean())[:3])
        n += ref.val.size
    assert n > 1500
    # the families are not comparisons of zeros
    fam = G.rot_families()
    assert (fam["random"][2].val > 0.05).sum() >= 40
    for name in ("identical", "wl_swapped", "yaw_plus_pi", "yaw_out_of_range"):
        d = np.diag(fam[name][2].val)
        assert (d > (0.999999 if name != "yaw_out_of_range" else 0.3)).all(), (name, d)
    assert np.abs(fam["identical"][0][:, :2]).max() == 72.0
    assert np.abs(fam["yaw_out_of_range"][0][:, 4]).max() == 7.0 and (np.abs(fam["yaw_out_of_range"][0][:, 4]) > 3.2).all()
    sh = G.rot_shapes()
    assert all((r.val > 0).sum() >= 10 for (a, b), (_, _, r) in sh.items() if a * b > 100)


def test_guard_cases_sit_a_factor_two_from_their_guard():
    fam = G.rot_families()
    a = fam["area_guard"][2]
    for A in (a.A1, a.A2[1:]):
        r = A / G.AREA_GUARD
        assert (np.minimum(np.abs(r - 0.5), np.abs(r - 2.0)) < 0.01).all(), r
    assert (a.A1 < 1e-6).sum() == 2 and (a.A1 > 1e-6).sum() == 2
    assert a.val[0, 0] == 0.0 and abs(a.val[1, 0] - 2e-6 / 8.0) < 1e-9 and abs(a.val[1, 1] - 1.0) < 1e-12
    # an area below the guard with an intersection above the intersection guard: only the area guard zeroes it
    assert a.inter[0, 0] > 2 * G.INTER_GUARD and a.A1[0] < G.AREA_GUARD
    i = fam["inter_guard"][2]
    r = i.inter / G.INTER_GUARD
    assert (np.minimum(np.abs(r - 0.5), np.abs(r - 2.0)) < 0.01).all(), r
    assert ((i.val == 0) == (i.inter < 1e-7)).all() and (i.val > 0).sum() == 2
    t = fam["touching_rotated"][2]
    assert (t.inter < 2 * G.INTER_GUARD).all() and (t.val == 0).all()
    assert (t.inter > G.INTER_GUARD / 2).sum() == 1  # f32(pi/2) is not pi/2: a sliver of 8.7e-8 m^2
    d = fam["degenerate"][2]
    assert d.A1[1] == 0.0 and d.A2[2] == 0.0 and d.A2[3] == 0.0


def test_union_guard_is_unreachable():
    for _, (_, _, ref) in {**G.rot_families(), **G.rot_shapes(), **G.trusted_families()}.items():
        live = (ref.A1 >= 1e-6)[:, None] & (ref.A2 >= 1e-6)[None, :] & (ref.inter > 1e-7)
        u = ref.A1[:, None] + ref.A2[None, :] - ref.inter
        assert (u[live] > 1e-6).all()


def test_trusted_families_cover_their_sources():
    tr = G.trusted_families()
    assert sum(k.startswith("nms_") for k in tr) == 3 and sum(k.startswith("fuse_") for k in tr) >= 10
    assert sum(k.startswith("det_errors_") for k in tr) >= 8
    clipped = 0
    for name, (b1, b2, ref) in tr.items():
        assert max(len(b1), len(b2)) <= G.TRUST_CAP
        assert not (ref.pruned & (ref.val != 0)).any()
        clipped += int((~ref.pruned).sum())
        if len(b1) >= 50:
            assert (ref.val > 0.2).sum() >= 20, name  # the relation these files read has members
    print(f"trusted families: {clipped} pairs clipped")


# ============================================================================ decode and anchors
def test_decode_references_agree_within_half_the_bound():
    c = G.decode_case()
    anc = c["table"][c["idx"]]
    worst, fails = G.judge_decode(G.decode_ref32(c["rel"], anc), c["rel"], anc, share=0.5)
    assert not fails, fails
    for k, v in worst.items():
        _note(f"decode torch f32 {k} (of half the bound)", v)


def test_decode_cases_hold_what_they_claim():
    c = G.decode_case()
    rel, kind = c["rel"], c["kind"]
    anc = c["table"][c["idx"]]
    ref, raw = G.decode_ref64(rel, anc)
    assert rel.shape == (G.DEC_N, 6) and c["table"].shape == (G.DEC_TABLE, 5)
    assert len(np.unique(c["idx"])) < G.DEC_N and (np.diff(c["idx"]) < 0).any()  # repeated, out of order
    rnd = kind == "random"
    share = float((np.abs(raw[rnd]) > math.pi).mean())
    print(f"random decode rows that wrap: {share:.1%}")
    assert share >= 0.10
    small = kind == "small_angle_terms"
    assert abs(small.mean() - 0.25) < 0.02 and np.abs(rel[small, 4:6]).max() < 6e-3
    z = kind == "zero_angle_terms"
    assert z.sum() >= 32 and (rel[z, 4:6] == 0).all() and np.abs(ref[z, 4] - anc[z, 4]).max() < 1e-15  # atan2(0, 0) = 0
    at = kind == "yaw_at_pi"
    assert at.sum() >= 32 and (np.abs(np.abs(raw[at]) - math.pi) < 1.001e-3).all()
    assert (raw[at] > 0).any() and (raw[at] < 0).any()
    assert (np.abs(raw[at]) > math.pi).any() and (np.abs(raw[at]) < math.pi).any()
    bey = kind == "yaw_beyond_pi"
    assert bey.sum() >= 32 and (np.abs(raw[bey]) > math.pi + 0.009).all() and (np.abs(ref[:, 4]) <= math.pi).all()
    ex = kind == "exp_range"
    r32 = G.decode_ref32(rel, anc)
    # e^80 = 5.5e34 and e^-80 = 1.8e-35 are ordinary f32 numbers: those rows fall under the size
    # bound; +-110 is what overflows (inf) and underflows (0) in f32
    for v, test in ((80.0, np.isfinite), (-80.0, lambda x: np.isfinite(x) & (x > 0)), (110.0, np.isinf), (-110.0, lambda x: x == 0)):
        for col in (2, 3):
            rows = ex & (rel[:, col] == v)
            assert rows.sum() >= 8 and test(r32[rows, col]).all(), (v, col)
    assert set(map(tuple, np.round(anc[:, 2:4], 4))) >= {(2.0, 4.5), (2.5, 2.5), (1.5, 9.0), (4.0, 2.0)}


def anchors_restate(case, defect=None):
    """anchors_kernel in numpy f32, one row per thread index."""
    H, W, s, voxel, _, _, cfg = case
    ox, oy = (F32(v) for v in G.anchor_offsets(case))
    voxel = F32(voxel)
    fh, fw, A = H // s, W // s, len(cfg)
    i = np.arange(fh * fw * A)
    a, loc = (i // (fh * fw), i % (fh * fw)) if defect == "anchor_major" else (i % A, i // A)
    gy, gx = loc // fw, loc % fw
    half = F32(s // 2) if defect == "integer_half_stride" else F32(s) / F32(2)
    px, py = (gx * s).astype(F32) + half, (gy * s).astype(F32) + half
    if defect == "offset_after_scale":
        x, y = oy - py * voxel, px * voxel - ox
    else:
        x, y = (oy - py) * voxel, (px - ox) * voxel
    if defect == "xy_swapped":
        x, y = y, x
    c = np.asarray(cfg, F32)
    return np.stack([x, y, c[a, 0], c[a, 1], c[a, 2]], 1).astype(F32)


ANCHOR_DEFECTS = ("xy_swapped", "anchor_major", "integer_half_stride", "offset_after_scale")


def test_anchor_cases_and_planted_defects():
    refs = [G.anchors_ref(c) for c in G.ANCHOR_CASES]
    for c, r in zip(G.ANCHOR_CASES, refs):
        assert r.shape == ((c[0] // c[2]) * (c[1] // c[2]) * len(c[6]), 5) and r.shape[0] > 0
        assert G.same_bits(anchors_restate(c), r), c[:6]
    assert G.anchors_ref(G.ANCHOR_EMPTY).shape[0] == 0
    assert refs[0].shape[0] == 22500 and {len(c[6]) for c in G.ANCHOR_CASES} == {1, 5}
    for d in ANCHOR_DEFECTS:
        caught = [c[:3] for c, r in zip(G.ANCHOR_CASES, refs) if not G.same_bits(anchors_restate(c, d), r)]
        print(f"anchors defect {d}: rejected by {len(caught)} of {len(refs)} cases")
        assert caught, d
    # the odd stride is the only case that rejects the integer half stride
    assert all(G.same_bits(anchors_restate(c, "integer_half_stride"), r) == (c[2] % 2 == 0)
               for c, r in zip(G.ANCHOR_CASES, refs))


def decode_restate(rel, anc, defect=None):
    """decode_one in numpy f32."""
    d, a = G.f32(rel), G.f32(anc)
    with np.errstate(over="ignore"):
        e2 = np.exp(d[:, 3] if defect == "exp_wrong_column" else d[:, 2])
        e3 = np.exp(d[:, 3])
    t = np.arctan2(d[:, 5], d[:, 4]) if defect == "atan2_swapped" else np.arctan2(d[:, 4], d[:, 5])
    yaw = a[:, 4] + t
    if defect != "no_wrap":
        yaw = np.arctan2(np.sin(yaw), np.cos(yaw))
    return np.stack([d[:, 0] * a[:, 2] + a[:, 0], d[:, 1] * a[:, 3] + a[:, 1], e2 * a[:, 2], e3 * a[:, 3], yaw], 1).astype(F32)


def test_decode_planted_defects():
    c = G.decode_case()
    anc = c["table"][c["idx"]]
    worst, fails = G.judge_decode(decode_restate(c["rel"], anc), c["rel"], anc)
    assert not fails, fails
    for d in ("exp_wrong_column", "atan2_swapped", "no_wrap"):
        _, fails = G.judge_decode(decode_restate(c["rel"], anc, d), c["rel"], anc)
        print(f"decode defect {d}: {fails}")
        assert fails, d
    # the wrap is seen by the range check alone: the comparison is modulo 2 pi
    _, fails = G.judge_decode(decode_restate(c["rel"], anc, "no_wrap"), c["rel"], anc)
    assert fails == ["yaw outside [-pi, pi]"]
    # a gather that ignores idx
    _, fails = G.judge_decode(decode_restate(c["rel"], c["table"][np.arange(G.DEC_N) % G.DEC_TABLE]), c["rel"], anc)
    assert fails


# ============================================================================ IoU restatements and defects
def rot_restate(a, b, defect=None):
    """geom.h's rotated_iou(const float*, const float*) in Python f64, 12-slot polygons included."""
    def poly(r):
        cx, cy, w, l, yaw = (float(v) for v in r)
        if defect == "wl_swapped":
            w, l = l, w
        if defect == "yaw_sign":
            yaw = -yaw
        hw, hl = w / 2.0, l / 2.0
        c, s = math.cos(yaw), math.sin(yaw)
        P = [(lx * c - ly * s + cx, lx * s + ly * c + cy) for lx, ly in ((-hw, -hl), (hw, -hl), (hw, hl), (-hw, hl))]
        sa = 0.5 * sum(P[i][0] * P[(i + 1) % 4][1] - P[i][1] * P[(i + 1) % 4][0] for i in range(4))
        if sa < 0.0 and defect != "no_ccw":
            P = P[::-1]
        return P, abs(sa)
    (P, A1), (Q, A2) = poly(a), poly(b)
    if defect != "no_area_guard" and (A1 < 1e-6 or A2 < 1e-6):
        return F32(0)
    for e in range(3 if defect == "three_edges" else 4):
        if not P:
            break
        (ax, ay), (bx, by) = Q[e], Q[(e + 1) % 4]
        ex, ey = bx - ax, by - ay
        out = []
        for j in range(len(P)):
            (cxp, cyp), (pxp, pyp) = P[j], P[j - 1]
            sc = ex * (cyp - ay) - ey * (cxp - ax)
            sp = ex * (pyp - ay) - ey * (pxp - ax)
            if sc >= 0.0:
                if sp < 0.0 and len(out) < 12:
                    t = sp / (sp - sc)
                    out.append((pxp + t * (cxp - pxp), pyp + t * (cyp - pyp)))
                if len(out) < 12:
                    out.append((cxp, cyp))
            elif sp >= 0.0 and len(out) < 12:
                t = sp / (sp - sc)
                out.append((pxp + t * (cxp - pxp), pyp + t * (cyp - pyp)))
        P = out
    n = len(P)
    inter = abs(0.5 * sum(P[i][0] * P[(i + 1) % n][1] - P[i][1] * P[(i + 1) % n][0] for i in range(n))) if n >= 3 else 0.0
    if defect != "no_inter_guard" and not inter > 1e-7:
        return F32(0)
    u = A1 + A2 if defect == "union_is_sum" else A1 + A2 - inter
    if defect != "no_union_guard" and not u > 1e-6:
        return F32(0)
    return F32(inter / u) if u != 0 else F32(0)


def axis_restate(a, b):
    a, b = G.f32(a), G.f32(b)
    two, zero = F32(2), F32(0)
    with np.errstate(all="ignore"):
        ax1, ay1, ax2, ay2 = a[0] - a[2] / two, a[1] - a[3] / two, a[0] + a[2] / two, a[1] + a[3] / two
        bx1, by1, bx2, by2 = b[0] - b[2] / two, b[1] - b[3] / two, b[0] + b[2] / two, b[1] + b[3] / two
        iw = max(min(ax2, bx2) - max(ax1, bx1), zero)
        ih = max(min(ay2, by2) - max(ay1, by1), zero)
        inter = iw * ih
        return inter / (((a[2] * a[3] + b[2] * b[3]) - inter) + F32(1e-7))


def matrix_restate(pair, n1, n2, defect=None):
    """iou_matrix_kernel over a pair function of (row, column); indices past an array wrap, as a
    model of reading whatever lies there."""
    out = np.full(n1 * n2, np.nan, F32)
    for i in range(n1 * n2):
        r, c = (i // n1, i % n1) if defect == "row_stride_n1" else (i // n2, i % n2)
        v = pair(r % n1, c % n2)
        out[(c % n2) * n1 + (r % n1) if defect == "transposed" else i] = v
    return out.reshape(n1, n2)


PAIR_DEFECTS = ("wl_swapped", "yaw_sign", "no_ccw", "three_edges", "union_is_sum", "no_area_guard", "no_inter_guard")


def test_rotated_restatement_and_planted_defects():
    fam = G.rot_families()
    worst = 0.0
    for name, (b1, b2, ref) in fam.items():
        got = np.array([[rot_restate(a, b) for b in b2] for a in b1], F32)
        w, fails = G.judge_rotated(got, ref)
        assert not fails, (name, fails[:3])
        worst = max(worst, w)
    _note("rotated IoU, Python restatement", worst)
    for d in PAIR_DEFECTS:
        caught = [name for name, (b1, b2, ref) in fam.items()
                  if G.judge_rotated(np.array([[rot_restate(a, b, d) for b in b2] for a in b1], F32), ref)[1]]
        print(f"rotated defect {d}: rejected by {caught}")
        assert caught, d
    # which case carries which defect
    def rejects(name, d):
        b1, b2, ref = fam[name]
        return bool(G.judge_rotated(np.array([[rot_restate(a, b, d) for b in b2] for a in b1], F32), ref)[1])
    assert rejects("negative_size", "no_ccw") and not any(rejects(k, "no_ccw") for k in fam if k != "negative_size")
    assert rejects("area_guard", "no_area_guard") and rejects("inter_guard", "no_inter_guard")
    # the union guard cannot be reached (module docstring): dropping it changes nothing
    for name, (b1, b2, ref) in fam.items():
        assert not rejects(name, "no_union_guard")


def test_matrix_layout_defects_are_rejected_by_the_shapes():
    sh = G.rot_shapes()
    for d in ("transposed", "row_stride_n1"):
        caught_rot, caught_axis = [], []
        for (n1, n2), (b1, b2, ref) in sh.items():
            val = ref.val.astype(F32)
            assert not G.judge_rotated(matrix_restate(lambda r, c: val[r, c], n1, n2), ref)[1]
            if G.judge_rotated(matrix_restate(lambda r, c: val[r, c], n1, n2, d), ref)[1]:
                caught_rot.append((n1, n2))
            ax = G.axis_ref(b1, b2)
            assert G.same_bits(matrix_restate(lambda r, c: ax[r, c], n1, n2), ax)
            if not G.same_bits(matrix_restate(lambda r, c: ax[r, c], n1, n2, d), ax):
                caught_axis.append((n1, n2))
        print(f"layout defect {d}: rotated {caught_rot}, axis {caught_axis}")
        assert (3, 130) in caught_rot and (129, 2) in caught_rot and (2, 128) in caught_rot
        assert (3, 130) in caught_axis and (129, 2) in caught_axis and (2, 128) in caught_axis
    # a square or golden-shaped matrix of one box list against itself would not see a transposition
    b = G.rot_families()["identical"][0]
    sym = G.axis_ref(b, b)
    assert G.same_bits(matrix_restate(lambda r, c: sym[r, c], 8, 8, "transposed"), sym)


def test_axis_restatement_is_bit_equal_to_the_oracle():
    n = 0
    for name, (b1, b2) in G.axis_cases().items():
        ref = G.axis_ref(b1, b2)
        got = np.array([[axis_restate(a, b) for b in b2] for a in b1], F32).reshape(ref.shape)
        assert G.same_bits(got, ref), name
        n += ref.size
    assert n > 2000
    sp = G.axis_ref(*G.axis_special_pool())
    assert np.isnan(sp).any() and np.isinf(G.axis_special_pool()[0]).any() and (sp == 1.0).any() and (sp == 0.0).any()


# ============================================================================ host build of geom.h
def _host_compiler():
    import importlib.util
    spec = importlib.util.spec_from_file_location("asan_abi", os.path.join(REPO, "tools", "asan_abi.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    cxx = os.path.join(os.path.dirname(os.path.realpath(m.HIPCC)), "..", "lib", "llvm", "bin", "clang++")
    if not os.path.exists(cxx):
        cxx = "/opt/rocm/lib/llvm/bin/clang++"
    return cxx if os.path.exists(cxx) else None


@pytest.fixture(scope="module")
def geom_host(tmp_path_factory):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host compiler (the ROCm clang++ that tools/asan_abi.py links with)")
    tmp = tmp_path_factory.mktemp("geom_host")
    exe = str(tmp / "geom_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-ffp-contract=off", "-I", os.path.join(PKG, "csrc"), os.path.join(REPO, "tools", "geom_host.cpp"),
                    "-o", exe], check=True)
    count = [0]

    def run(b1, b2):
        """-> (rotated [n1, n2], axis [n1, n2]) f32 of every pair, row-major as the kernel stores them."""
        b1, b2 = G.boxes(b1), G.boxes(b2)
        count[0] += 1
        path = str(tmp / f"cases{count[0]}.txt")
        with open(path, "w") as fh:
            for a in b1:
                for b in b2:
                    fh.write(" ".join(repr(float(x)) for x in np.concatenate([a, b])) + "\n")
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
        p = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        assert "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-2000:]
        out = np.array([[float(x) for x in ln.split()] for ln in p.stdout.splitlines()], np.float64).reshape(-1, 2)
        assert out.shape[0] == len(b1) * len(b2)
        return out[:, 0].astype(F32).reshape(len(b1), len(b2)), out[:, 1].astype(F32).reshape(len(b1), len(b2))
    return run


def test_host_build_rotated_under_the_bounds(geom_host):
    sets = {**G.rot_families(), **{f"shape_{a}x{b}": v for (a, b), v in G.rot_shapes().items()}}
    for name, (b1, b2, ref) in sets.items():
        rot, _ = geom_host(b1, b2)
        w, fails = G.judge_rotated(rot, ref)
        assert not fails, (name, fails[:3])
        _note(f"host rotated {name}", w)
        # symmetry: each order within the bound of the reference, not bit-equal to the other
        rot_t, _ = geom_host(b2, b1)
        ref_t = G.RotRef(b2, b1, exact=True)
        assert np.abs(ref_t.val - ref.val.T).max() <= 1e-12
        w, fails = G.judge_rotated(rot_t, ref_t)
        assert not fails, (name, "swapped", fails[:3])
    fam = G.rot_families()
    deg, _ = geom_host(*fam["degenerate"][:2])
    assert (deg[1] == 0).all() and (deg[:, 2] == 0).all() and (deg[:, 3] == 0).all() and (deg > 0.2).sum() == 4


def test_host_build_on_the_families_other_tests_trust(geom_host):
    for name, (b1, b2, ref) in G.trusted_families().items():
        rot, _ = geom_host(b1, b2)
        w, fails = G.judge_rotated(rot, ref)
        assert not fails, (name, len(fails), fails[:3])
        _note(f"host rotated trusted {name}", w)


def test_host_build_axis_bit_equal(geom_host):
    for name, (b1, b2) in G.axis_cases().items():
        _, ax = geom_host(b1, b2)
        assert G.same_bits(ax, G.axis_ref(b1, b2)), name
    b1, b2, rows, cols = G.axis_nan_pool()
    _, ax = geom_host(b1, b2)
    ref = G.axis_ref(b1, b2)
    assert G.same_bits(ax[np.ix_(rows, cols)], ref[np.ix_(rows, cols)])
    assert np.isfinite(ref[np.ix_(rows, cols)]).all() and (ref[np.ix_(rows, cols)] > 0).any()
