"""Cases, references and judges for the box geometry primitives (support module, no tests):
ivit_generate_anchors, ivit_axis_iou, ivit_rotated_iou, ivit_decode_boxes.

References, none of which calls the library:
  rotated IoU  ``exact_pair``: the f64 corners of rect_poly's formulas (csrc/geom.h), then the
               Sutherland-Hodgman clip and the shoelace areas in exact rational arithmetic on
               those corners, so nothing depends on an order of floating-point operations.
               ``oracle_pair``: the oracle's own f64 helpers (what rotated_iou_numpy computes before
               it rounds its result to f32), for boxes with a non-finite field, which have no
               rational corners. (The exact clip takes ~0.1 ms a pair, so it serves every matrix.)
  axis IoU     oracle.axis_aligned_iou (torch CPU f32, the reference's operation order).
  decode       ``decode_ref64``: riou_cases.decode_f64 plus the final wrap, in f64; oracle.decode_boxes
               is the f32 restatement.
  anchors      oracle.generate_anchors.

Every box is an f32 array; seeds are fixed; nothing is larger than 130 x 130 pairs or 4 096 rows
(the anchor grids are the ones the models use).

The judges return (worst err / bound, [failure strings]) and are shared by the host build of
csrc/geom.h (tests/test_cpu_geom_cases.py) and the device (tests/test_gpu_geom.py).
"""
import functools
import math
from fractions import Fraction

import numpy as np
import torch

import riou_cases as R
from oracle import ivit_oracle as O

PI = math.pi
F32 = np.float32
TAIL = 16  # extra elements behind every output buffer, prefilled and checked


def f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64), dtype=np.float32)


def boxes(rows):
    return f32(rows).reshape(-1, 5)


# ============================================================================ rotated IoU: references
AREA_GUARD, INTER_GUARD, UNION_GUARD = 1e-6, 1e-7, 1e-6
ZONE = 1.5  # a quantity within this factor of its guard may fall on either side; f64 rounding moves it by ~1e-10
ROT_REL, ROT_ABS = 2.0 ** -24, 1e-9  # one f32 rounding of the result + the f64 clip (areas >= 0.1, |xy| <= 200)


def rot_bound(ref):
    return ROT_REL * np.abs(ref) + ROT_ABS


def corners64(b):
    """rect_poly: the f64 corners of one f32 box row, in the header's order."""
    cx, cy, w, l, a = (float(v) for v in b)
    hw, hl = w / 2.0, l / 2.0
    c, s = math.cos(a), math.sin(a)
    return [((lx * c - ly * s) + cx, (lx * s + ly * c) + cy) for lx, ly in ((-hw, -hl), (hw, -hl), (hw, hl), (-hw, hl))]


def _area2(P):
    n = len(P)
    return sum(P[i][0] * P[(i + 1) % n][1] - P[i][1] * P[(i + 1) % n][0] for i in range(n))


def _clip(P, Q):
    """Sutherland-Hodgman on any exact number type: P clipped by the ccw convex Q."""
    out = list(P)
    for i in range(len(Q)):
        if not out:
            break
        (ax, ay), (bx, by) = Q[i], Q[(i + 1) % len(Q)]
        ex, ey = bx - ax, by - ay
        inp, out = out, []
        sides = [ex * (p[1] - ay) - ey * (p[0] - ax) for p in inp]
        for j in range(len(inp)):
            cur, prv, sc, sp = inp[j], inp[j - 1], sides[j], sides[j - 1]
            if sc >= 0:
                if sp < 0:
                    t = sp / (sp - sc)
                    out.append((prv[0] + t * (cur[0] - prv[0]), prv[1] + t * (cur[1] - prv[1])))
                out.append(cur)
            elif sp >= 0:
                t = sp / (sp - sc)
                out.append((prv[0] + t * (cur[0] - prv[0]), prv[1] + t * (cur[1] - prv[1])))
    return out


def _exact_poly(b):
    P = [(Fraction(x), Fraction(y)) for x, y in corners64(b)]
    a2 = _area2(P)
    return (P if a2 >= 0 else P[::-1]), abs(a2) / 2


def exact_pair(pa, pb):
    """(A1, A2, intersection) of two _exact_poly records as exact rationals."""
    (P, A1), (Q, A2) = pa, pb
    if A1 == 0 or A2 == 0:
        return A1, A2, Fraction(0)
    C = _clip(P, Q)
    return A1, A2, (abs(_area2(C)) / 2 if len(C) >= 3 else Fraction(0))


def _oracle_poly(b):
    with np.errstate(all="ignore"):
        P = O._rect_corners(b)
        return P, O._poly_area(P)


def oracle_pair(pa, pb):
    """The same three numbers from the oracle's f64 helpers (convex_clip, _poly_area)."""
    (P, A1), (Q, A2) = pa, pb
    if A1 < AREA_GUARD / ZONE or A2 < AREA_GUARD / ZONE:  # far below the area guard: never clipped (a NaN area is)
        return A1, A2, 0.0
    with np.errstate(all="ignore"):
        return A1, A2, O._poly_area(O.convex_clip(P, Q))


def guarded(A1, A2, inter):
    """The three guards of rotated_iou_numpy on f64 numbers -> the IoU (f64, not rounded to f32)."""
    if A1 < AREA_GUARD or A2 < AREA_GUARD:
        return 0.0
    if not inter > INTER_GUARD:
        return 0.0
    u = A1 + A2 - inter
    return inter / u if u > UNION_GUARD else 0.0


class RotRef:
    """The reference of one n1 x n2 matrix: A1 [n1], A2 [n2], inter / val / raw [n1, n2] (f64).
    val carries the guards; raw is inter / union wherever the union is positive."""

    def __init__(self, b1, b2, exact, pairs=None):
        b1, b2 = boxes(b1), boxes(b2)
        self.b1, self.b2, self.exact = b1, b2, exact
        # a box with a non-finite field has no rational corners: its pairs go through the oracle
        ex1 = [exact and bool(np.isfinite(b).all()) for b in b1]
        ex2 = [exact and bool(np.isfinite(b).all()) for b in b2]
        p1 = [_exact_poly(b) if e else _oracle_poly(b) for b, e in zip(b1, ex1)]
        p2 = [_exact_poly(b) if e else _oracle_poly(b) for b, e in zip(b2, ex2)]
        o1 = {i: _oracle_poly(b1[i]) for i, e in enumerate(ex1) if exact and not all(ex2)}
        o2 = {j: _oracle_poly(b2[j]) for j, e in enumerate(ex2) if exact and not all(ex1)}
        n1, n2 = len(b1), len(b2)
        self.A1 = np.array([float(p[1]) for p in p1], np.float64).reshape(n1)
        self.A2 = np.array([float(p[1]) for p in p2], np.float64).reshape(n2)
        self.inter = np.zeros((n1, n2))
        self.val = np.zeros((n1, n2))
        self.raw = np.zeros((n1, n2))
        self.pruned = np.zeros((n1, n2), bool)  # pairs decided by the centre distance, never clipped
        for i in range(n1):
            for j in range(n2):
                if pairs is not None and not pairs[i, j]:
                    self.pruned[i, j] = True
                    continue
                if ex1[i] and ex2[j]:
                    A1, A2, inter = exact_pair(p1[i], p2[j])
                else:
                    A1, A2, inter = oracle_pair(o1[i] if ex1[i] else p1[i], o2[j] if ex2[j] else p2[j])
                u = A1 + A2 - inter
                self.inter[i, j] = float(inter)
                self.val[i, j] = guarded(float(A1), float(A2), float(inter))
                self.raw[i, j] = float(inter / u) if u > 0 else 0.0

    def clean(self):
        """[n1, n2] bool: the pair meets what the bound was derived for (areas >= 0.1 or exactly 0,
        |coordinates| <= 200, the intersection 0 or >= 1e-4: two orders of magnitude from the guard)."""
        def ok_area(A):
            return (A == 0) | (A >= 0.1)

        def ok_xy(b):
            return np.array([max(abs(v) for p in corners64(r) for v in p) <= 200.0 for r in b], bool).reshape(len(b))
        box_ok = (ok_area(self.A1) & ok_xy(self.b1))[:, None] & (ok_area(self.A2) & ok_xy(self.b2))[None, :]
        return box_ok & ((self.inter == 0) | (self.inter >= 1e-4))


def judge_rotated(got, ref):
    """got: [n1, n2] f32 from the code under test. Per pair:
      * a box whose area is below the guard by the factor ZONE or more (zero areas included), a pair
        pruned by its centre distance, or an intersection that far below its guard: exactly 0.0f;
      * an area or an intersection within the factor ZONE of its guard: exactly 0.0f, or within the bound
        of the unguarded value (f64 rounding may fall either way);
      * every other pair: |got - ref| <= 2^-24 |ref| + 1e-9.
    -> (worst err / bound over the bounded pairs, failures)."""
    got = np.asarray(got, np.float32).reshape(ref.val.shape).astype(np.float64)
    fails, worst = [], 0.0
    dead = (ref.A1 < AREA_GUARD / ZONE)[:, None] | (ref.A2 < AREA_GUARD / ZONE)[None, :]
    edge = ((ref.A1 >= AREA_GUARD / ZONE) & (ref.A1 < AREA_GUARD * ZONE))[:, None] | \
           ((ref.A2 >= AREA_GUARD / ZONE) & (ref.A2 < AREA_GUARD * ZONE))[None, :]
    for i in range(got.shape[0]):
        for j in range(got.shape[1]):
            g, raw, inter = got[i, j], ref.raw[i, j], ref.inter[i, j]
            if dead[i, j] or ref.pruned[i, j] or inter <= INTER_GUARD / ZONE:
                if not (g == 0.0):  # also rejects NaN
                    fails.append(f"[{i},{j}] {g!r}: exactly 0 required (areas {ref.A1[i]:.3g} {ref.A2[j]:.3g}, "
                                 f"intersection {inter:.3g})")
                continue
            err, bnd = abs(g - raw), float(rot_bound(raw))
            if edge[i, j] or inter < INTER_GUARD * ZONE:
                if not (g == 0.0 or err <= bnd):
                    fails.append(f"[{i},{j}] {g!r}: 0 or {raw!r} +- {bnd:.3g} required (next to a guard)")
                continue
            if not err <= bnd:
                fails.append(f"[{i},{j}] {g!r} vs {raw!r}: err / bound {err / bnd:.3g}")
            worst = max(worst, err / bnd) if err == err else math.inf
    return worst, fails


# ============================================================================ rotated IoU: case families
def _rand_boxes(rng, n, half=5.0):
    """Vehicle-sized boxes with centres in +-half m and any yaw."""
    return boxes(np.stack([rng.uniform(-half, half, n), rng.uniform(-half, half, n), rng.uniform(1.5, 2.5, n),
                           rng.uniform(3.5, 6.0, n), rng.uniform(-PI, PI, n)], 1))


def _families():
    q, h = PI / 4, PI / 2
    fam = {}
    rng = np.random.RandomState(11)
    draws = [R.draw_case(rng) for _ in range(12)]
    fam["random"] = (boxes([d[0] for d in draws]), boxes([d[1] for d in draws]))
    # identical boxes at arbitrary yaw, the last four at the corners of the BEV (+-72 m)
    ident = np.concatenate([_rand_boxes(rng, 4, 60.0), boxes([[72, 72, 2, 4.5, 0.7], [-72, 72, 2.5, 2.5, -2.1],
                                                               [72, -72, 1.5, 9, 3.0], [-72, -72, 4, 2, -0.4]])])
    fam["identical"] = (ident, ident.copy())
    base = np.concatenate([_rand_boxes(rng, 5, 30.0), boxes([[10, -20, 2, 4.5, 0.0], [-30, 40, 1.5, 9, -3.0]])])
    swap = base.astype(np.float64)[:, [0, 1, 3, 2, 4]]
    swap[:, 4] += h
    fam["wl_swapped"] = (base, boxes(swap))
    turn = base.astype(np.float64).copy()
    turn[:, 4] += np.where(turn[:, 4] > 0, -PI, PI)
    fam["yaw_plus_pi"] = (base, boxes(turn))
    far = base.astype(np.float64).copy()
    far[:, 4] = [-7.0, 7.0, 3.5, -3.5, 5.0, -6.25, 6.9]
    near = far.copy()
    near[:, :2] += rng.uniform(-0.6, 0.6, (len(far), 2))
    near[:, 4] += rng.uniform(-0.3, 0.3, len(far))
    fam["yaw_out_of_range"] = (boxes(far), boxes(near))
    small, big = [0.4, -0.1, 1.0, 2.0, 1.0], [0.3, -0.2, 3.0, 6.0, 0.4]
    fam["containment"] = (boxes([small, big, [50, 50, 0.5, 0.75, -2.0]]), boxes([big, small, [50.25, 49.75, 4, 8, 2.5]]))
    # yaw 0: cos = 1 and sin = 0 exactly, the corners are exact and a shared edge or corner has intersection 0
    fam["shared_edge_axis"] = (boxes([[0, 0, 2, 4, 0], [10, 10, 3, 1, 0]]),
                               boxes([[2, 0, 2, 4, 0], [0, 4, 2, 4, 0], [10, 11, 3, 1, 0], [13, 10, 3, 1, 0]]))
    fam["corner_touch_axis"] = (boxes([[0, 0, 2, 4, 0], [-20, 5, 1, 1, 0]]),
                                boxes([[2, 4, 2, 4, 0], [-2, -4, 2, 4, 0], [-19, 6, 1, 1, 0], [-21, 4, 1, 1, 0]]))
    fam["half_overlap"] = (boxes([[0, 0, 2, 4, 0], [5, 5, 2, 4, 0.5], [-8, 3, 3, 3, q]]),
                           boxes([[1, 0, 2, 4, 0], [0, 2, 2, 4, 0], [5 - math.sin(0.5) * 2, 5 + math.cos(0.5) * 2, 2, 4, 0.5],
                                  [-8 + 1.5 * math.cos(q), 3 + 1.5 * math.sin(q), 3, 3, q]]))
    fam["same_centre_45"] = (boxes([[0, 0, 2, 2, 0], [7, -3, 2, 10, 0.3], [-40, 60, 4.5, 2, -1.0]]),
                             boxes([[0, 0, 2, 2, q], [7, -3, 2, 10, 0.3 + q], [-40, 60, 4.5, 2, -1.0 - q],
                                    [-40, 60, 2, 4.5, -1.0 + q]]))
    fam["thin"] = (boxes([[0, 0, 0.3, 12, 0.2], [20, 0, 0.3, 12, -1.0], [0, 30, 12, 0.3, 2.0]]),
                   boxes([[0, 0, 0.3, 12, 0.201], [0.05, 0, 0.3, 12, 0.199], [0, 0, 0.3, 12, 0.2 + h], [0, 1, 0.3, 12, 1.0],
                          [20, 0, 0.3, 12, -1.001], [20, 0.5, 0.3, 12, 0.6], [0, 30, 12, 0.3, 2.001], [0, 30, 0.3, 12, 2.0]]))
    # one negative size gives rect_poly's corners clockwise: the only inputs on which make_ccw acts
    fam["negative_size"] = (boxes([[3, 4, 2, 4.5, 0.6], [3, 4, -2, 4.5, 0.6], [-6, 1, 2.5, -2.5, -1.2]]),
                            boxes([[3, 4, -2, 4.5, 0.6], [3.5, 4.25, 2, -4.5, 0.5], [3, 4, -2, -4.5, 0.6], [-6, 1, 2.5, 2.5, -1.2],
                                   [-5.5, 1, -2.5, 2.5, 0.3]]))
    deg = [1.0, 0.5, 0.0, 4.0, 0.3]
    fam["degenerate"] = (boxes([[1, 0.5, 2, 4, 0.3], deg, [0, 0, 2.5, 2.5, 0]]),
                         boxes([[1.2, 0.4, 2, 4, 0.1], [0.5, 0, 2, 4.5, 1.0], deg, [1, 0.5, 0, 0, 0]]))
    return fam


CLEAN_FAMILIES = ("random", "identical", "wl_swapped", "yaw_plus_pi", "yaw_out_of_range", "containment",
                  "shared_edge_axis", "corner_touch_axis", "half_overlap", "same_centre_45", "thin", "negative_size",
                  "degenerate")


def _near_guard_families():
    """Judged by the guard rules of judge_rotated, not by the bound alone."""
    q, h = PI / 4, PI / 2
    fam = {}
    # areas a factor 2 below and above 1e-6 at the origin (small coordinates keep their f64 areas exact to
    # 1e-16 relative), inside a vehicle-sized box and on top of each other
    lo, hi = math.sqrt(0.5e-6), math.sqrt(2e-6)
    fam["area_guard"] = (boxes([[0, 0, lo, lo, 0.3], [0, 0, hi, hi, 0.3], [0, 0, lo * 2, lo / 2, 0], [0, 0, hi / 2, hi * 2, 1.0]]),
                         boxes([[0, 0, 2, 4, 0.1], [0, 0, hi, hi, 0.3], [0, 0, lo, lo, 0.3]]))
    # corner overlaps of d x d with d^2 a factor 2 below and above 1e-7
    dl, dh = math.sqrt(0.5e-7), math.sqrt(2e-7)
    fam["inter_guard"] = (boxes([[0, 0, 2, 4, 0]]), boxes([[2 - dl, 4 - dl, 2, 4, 0], [2 - dh, 4 - dh, 2, 4, 0],
                                                           [-(2 - dl), 4 - dl, 2, 4, 0], [-(2 - dh), -(4 - dh), 2, 4, 0]]))
    # f32(pi/2) and f32(pi/4) are not the angles: the touching edge or corner leaves a sliver or a gap
    fam["touching_rotated"] = (boxes([[0, 0, 2, 4, 0], [70, 0, 2, 2, q], [0, 20, 2, 4, h]]),
                               boxes([[2, 0, 4, 2, h], [70 + 2 * math.sqrt(2.0), 0, 2, 2, q], [0, 22, 2, 2, h],
                                      [70 + math.sqrt(2.0), math.sqrt(2.0), 2, 2, q]]))
    return fam


@functools.lru_cache(maxsize=None)
def rot_families():
    """{name: (b1, b2, RotRef by the exact rational clip)}, computed once."""
    out = {}
    for k, (b1, b2) in {**_families(), **_near_guard_families()}.items():
        out[k] = (b1, b2, RotRef(b1, b2, exact=True))
    return out


SHAPES = ((1, 1), (3, 130), (129, 2), (1, 127), (1, 128), (1, 129), (2, 128))
EMPTY_SHAPES = ((0, 5), (5, 0))


SHAPE_SEED = 23


@functools.lru_cache(maxsize=None)
def _shape_pool(seed=SHAPE_SEED):
    """130 row boxes and 130 column boxes: every family's boxes moved into one 7 m neighbourhood
    (so rows meet columns of other families), then random vehicles."""
    rng = np.random.RandomState(seed)
    rows, cols = [], []
    for k, (b1, b2) in _families().items():
        if k == "identical":
            continue
        for src, dst in ((b1, rows), (b2, cols)):
            m = src.astype(np.float64).copy()
            m[:, :2] = m[:, :2] - m[0, :2] + rng.uniform(-3.5, 3.5, 2)
            dst.extend(m)
    rows = np.concatenate([boxes(rows), _rand_boxes(rng, 130, 3.5)])[:130]
    cols = np.concatenate([boxes(cols), _rand_boxes(rng, 130, 3.5)])[:130]
    perm1, perm2 = rng.permutation(130), rng.permutation(130)
    return rows[perm1], cols[perm2]


@functools.lru_cache(maxsize=None)
def rot_shapes(seed=SHAPE_SEED):
    """{(n1, n2): (b1, b2, RotRef by the exact rational clip)}: the first n1 row boxes, the last n2
    column boxes of the pool."""
    rows, cols = _shape_pool(seed)
    out = {}
    for n1, n2 in SHAPES:
        b1, b2 = rows[:n1].copy(), cols[130 - n2:].copy()
        out[(n1, n2)] = (b1, b2, RotRef(b1, b2, exact=True))
    return out


def half_diag_pairs(b1, b2):
    """[n1, n2] bool: False where the centres are further apart than the sum of the half diagonals
    (such boxes are disjoint); a non-finite field leaves the pair in."""
    b1, b2 = boxes(b1).astype(np.float64), boxes(b2).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        h1, h2 = 0.5 * np.hypot(b1[:, 2], b1[:, 3]), 0.5 * np.hypot(b2[:, 2], b2[:, 3])
        d = np.hypot(b1[:, None, 0] - b2[None, :, 0], b1[:, None, 1] - b2[None, :, 1])
        return ~(d > h1[:, None] + h2[None, :])


TRUST_CAP = 130


@functools.lru_cache(maxsize=None)
def trusted_families():
    """{name: (b1, b2, RotRef)}: the box families from which test_gpu_nms_rotated.py, test_gpu_box_fuse.py
    and test_gpu_det_errors.py read their reference relation off the device, capped at 130 boxes a
    side. Pairs further apart than their half diagonals are pruned (exactly 0 required); the rest
    goes through the exact clip (a box with a NaN or infinite field: through the oracle's). The
    oracle's own shoelace sum loses 1e-8 at the coordinates near 1e4 of the NMS adversaries, twenty
    times the bound, so it cannot be the reference there."""
    import fuse_cases as FC
    import test_gpu_det_errors as DE
    import test_gpu_nms_rotated as NR
    sets = {}
    b, s = NR._family(129, 100 + 129)
    b = b[NR._order(s)]
    sets["nms_family_129"] = (b, b)
    b, s = NR._adversaries()
    b = b[NR._order(s)][:TRUST_CAP]
    sets["nms_adversaries_sorted"] = (b, b)
    b = NR._adversaries()[0]
    sets["nms_adversaries_tail"] = (b[-TRUST_CAP:], b[-TRUST_CAP:])
    for name, c in FC.all_cases():
        if c["scores"].shape[0] == 0:
            continue
        b = c["boxes"][FC.order_of(c["scores"])][:TRUST_CAP]
        sets[f"fuse_{name}"] = (b, b)
    for i, r in enumerate(DE._inputs()):
        p, g = r["pred_boxes_xywha"], r["gt_boxes_xywha"]
        if len(p) == 0 or len(g) == 0:
            continue
        p = p[np.argsort(-r["pred_scores"], kind="stable")][:TRUST_CAP]
        sets[f"det_errors_{i}"] = (p, g[:TRUST_CAP])
    return {k: (boxes(b1), boxes(b2), RotRef(b1, b2, exact=True, pairs=half_diag_pairs(b1, b2)))
            for k, (b1, b2) in sets.items()}


# ============================================================================ axis IoU
def axis_special_pool():
    """Rows and columns with zero, negative, 1e-20, 1e19 and infinite sizes, and identical boxes."""
    inf = float("inf")
    rows = boxes([[0, 0, 2, 4, 0], [0, 0, 0, 4, 0], [0, 0, 2, 0, 0], [0, 0, 0, 0, 0], [1, 1, -2, 4, 0], [1, 1, -2, -4, 0],
                  [0, 0, 1e-20, 1e-20, 0], [0, 0, 1e-20, 4, 0], [0, 0, 1e19, 1e19, 0], [5, 5, 1e19, 2, 0],
                  [0, 0, inf, 4, 0], [0, 0, inf, inf, 0], [0, 0, -inf, 4, 0], [72, -72, 2, 4.5, 0], [0.5, 0.25, 3, 1, 0]])
    cols = np.concatenate([rows[::-1], boxes([[0.5, 0.5, 2, 4, 0], [3e38, 0, 2, 4, 0]])])
    return rows, cols


def axis_nan_pool():
    """(b1, b2, finite rows of b1, finite columns of b2): one NaN field per poisoned box."""
    nan = float("nan")
    b1 = boxes([[0, 0, 2, 4, 0], [nan, 0, 2, 4, 0], [0.5, 0.5, 2, 4, 0], [0, nan, 2, 4, 0], [1, 0, 3, 3, 0]])
    b2 = boxes([[0, 0, nan, 4, 0], [0, 1, 2, 4, 0], [0, 0, 2, nan, 0], [1, 1, 2, 2, 0], [0, 0, 2, 4, nan], [-1, 0, 4, 2, 0],
                [0.25, 0, 1, 1, 0]])
    return b1, b2, np.array([0, 2, 4]), np.array([1, 3, 4, 5, 6])  # column 4: the yaw is not read


def axis_cases():
    """{name: (b1, b2)}: every rotated family and shape (columns 0..3 are read), and the special sizes."""
    out = {f"family_{k}": (b1, b2) for k, (b1, b2) in {**_families(), **_near_guard_families()}.items()}
    rows, cols = _shape_pool()
    for n1, n2 in SHAPES:
        out[f"shape_{n1}x{n2}"] = (rows[:n1].copy(), cols[130 - n2:].copy())
    out["special_sizes"] = axis_special_pool()
    return out


def axis_ref(b1, b2):
    with np.errstate(all="ignore"):
        return O.axis_aligned_iou(torch.from_numpy(boxes(b1)), torch.from_numpy(boxes(b2))).numpy()


def same_bits(got, ref):
    """Bit-equal f32 arrays; a NaN must meet a NaN (its sign and payload are not compared)."""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    if got.shape != ref.shape:
        return False
    gn, rn = np.isnan(got), np.isnan(ref)
    return bool(np.array_equal(gn, rn) and np.array_equal(got[~gn].view(np.int32), ref[~rn].view(np.int32)))


# ============================================================================ decode
DEC_C = 4.0
DEC_ULP = 2.0 ** -23
DEC_N, DEC_TABLE = 4096, 1024
DEC_SIZES = (1, 255, 256, 257, DEC_N)  # the launch uses 256-thread blocks


@functools.lru_cache(maxsize=None)
def decode_case():
    """-> dict: rel [4096, 6], table [1024, 5] (the paper configs and arbitrary sizes and yaws), idx
    [4096] int64 (out of order, repeated), kind [4096] (names below), all fixed."""
    rng = np.random.RandomState(5)
    T, n = DEC_TABLE, DEC_N
    cfg = np.array(O.ANCHOR_CONFIGS)
    table = np.empty((T, 5))
    table[:, 0] = rng.uniform(-20, 60, T)
    table[:, 1] = rng.uniform(-72, 72, T)
    table[:, 2:5] = cfg[rng.randint(0, len(cfg), T)]
    arb = rng.rand(T) < 0.5
    table[arb, 4] = rng.uniform(-PI, PI, int(arb.sum()))
    odd = rng.rand(T) < 0.2
    table[odd, 2] = rng.uniform(0.5, 4.0, int(odd.sum()))
    table[odd, 3] = rng.uniform(1.0, 10.0, int(odd.sum()))
    table = f32(table)
    idx = rng.randint(0, T, n).astype(np.int64)
    rel = rng.normal(size=(n, 6))
    rel[:, 2:4] *= 2.0
    kind = np.array(["random"] * n, dtype=object)
    quarter = np.arange(n) % 4 == 1
    rel[quarter, 4:6] *= 1e-3
    kind[quarter] = "small_angle_terms"
    spec = np.arange(8, n, 16)  # 256 rows, spread over every block
    zero, near, beyond, big = spec[0::4], spec[1::4], spec[2::4], spec[3::4]
    rel[zero, 4:6] = 0.0
    rel[zero[1::2], 4] = -0.0
    kind[zero] = "zero_angle_terms"
    # rows aimed at +-pi: atan2 stays inside (-pi, pi), so the sum a4 + atan2(d4, d5) reaches and passes
    # +-pi only on the side of the anchor's own yaw, and only for an anchor that is turned itself
    turned = np.nonzero(np.abs(table[:, 4]) > 0.1)[0]
    for rows in (near, beyond):
        idx[rows] = turned[rng.randint(0, len(turned), len(rows))]
    a4 = table[idx, 4].astype(np.float64)

    def aim(rows, past):
        """d4, d5 of `rows` so that the unwrapped yaw a4 + atan2(d4, d5) is sign(a4) * (pi + past)."""
        sg = np.sign(a4[rows])
        th = sg * (PI + past - np.abs(a4[rows]))
        assert (np.abs(th) < PI).all()
        r = rng.uniform(0.5, 1.5, len(rows))
        rel[rows, 4], rel[rows, 5] = r * np.sin(th), r * np.cos(th)
    aim(near, rng.uniform(-1e-3, 1e-3, len(near)))
    kind[near] = "yaw_at_pi"
    aim(beyond, np.minimum(rng.uniform(0.01, 3.0, len(beyond)), np.abs(a4[beyond]) - 0.05))
    kind[beyond] = "yaw_beyond_pi"
    vals = np.array([80.0, -80.0, 110.0, -110.0])
    rel[big, 2] = vals[np.arange(len(big)) % 4]
    rel[big, 3] = vals[(np.arange(len(big)) // 4) % 4]
    kind[big] = "exp_range"
    return {"rel": f32(rel), "table": table, "idx": idx, "kind": kind}


def decode_ref64(rel, anchors):
    """riou_cases.decode_f64 and the final wrap, in f64 -> ([n, 5] f64, unwrapped yaw [n])."""
    d, a = torch.from_numpy(f32(rel)).double(), torch.from_numpy(f32(anchors)).double()
    out = R.decode_f64(d.T, a.T).T.clone()
    raw = out[:, 4].clone()
    out[:, 4] = torch.atan2(torch.sin(raw), torch.cos(raw))
    return out.numpy(), raw.numpy()


def decode_ref32(rel, anchors):
    """oracle.decode_boxes: the f32 restatement (torch CPU)."""
    return O.decode_boxes(torch.from_numpy(f32(rel)), torch.from_numpy(f32(anchors))).numpy()


def judge_decode(got, rel, anchors, share=1.0):
    """Centres bit-equal to torch's CPU f32; sizes within share * C * 2^-23 |ref|, inf or 0 where the
    f32 reference overflows or underflows; the yaw within share * C * 2^-23 * 2 pi modulo 2 pi and in
    [-pi, pi] up to that. -> ({centre, size, yaw: worst err / bound}, failures)."""
    got = np.asarray(got, np.float32)
    ref64, _ = decode_ref64(rel, anchors)
    ref32 = decode_ref32(rel, anchors)
    fails = []
    if not same_bits(got[:, :2], ref32[:, :2]):
        bad = np.nonzero((got[:, :2].view(np.int32) != ref32[:, :2].view(np.int32)).any(axis=1))[0]
        fails.append(f"centres differ from torch f32 in {len(bad)} rows, first {bad[:5].tolist()}")
    worst = {}
    g, r, r32 = got[:, 2:4].astype(np.float64), ref64[:, 2:4], ref32[:, 2:4]
    ends = np.isinf(r32) | (r32 == 0)
    if not np.array_equal(g[ends], r32[ends].astype(np.float64)):
        fails.append(f"sizes: inf / 0 of the f32 reference not met in {int((g[ends] != r32[ends]).sum())} elements")
    with np.errstate(invalid="ignore"):
        ratio = np.abs(g - r)[~ends] / (share * DEC_C * DEC_ULP * np.abs(r[~ends]))
    worst["size"] = float(np.nanmax(ratio)) if ratio.size else 0.0
    if not (ratio <= 1.0).all():
        fails.append(f"sizes: err / bound {worst['size']:.3g} in {int((~(ratio <= 1.0)).sum())} elements")
    ybound = share * DEC_C * DEC_ULP * 2 * PI
    dy = (got[:, 4].astype(np.float64) - ref64[:, 4] + PI) % (2 * PI) - PI
    worst["yaw"] = float(np.abs(dy).max() / ybound) if not np.isnan(dy).any() else math.inf
    if not (np.abs(dy) <= ybound).all():
        fails.append(f"yaw: err / bound {worst['yaw']:.3g}")
    if not (np.abs(got[:, 4].astype(np.float64)) <= PI + ybound).all():
        fails.append("yaw outside [-pi, pi]")
    return worst, fails


# ============================================================================ anchors
CFG_ONE = ((3.25, 7.5, 0.4),)
# (H, W, stride, voxel, off_x, off_y, configs); off None: the defaults (360, 300)
ANCHOR_CASES = (
    (400, 720, 8, 0.2, None, None, tuple(O.ANCHOR_CONFIGS)),
    (400, 720, 16, 0.2, None, None, tuple(O.ANCHOR_CONFIGS)),
    (32, 48, 8, 0.2, None, None, tuple(O.ANCHOR_CONFIGS)),
    (37, 50, 8, 0.1, 48.0, 48.0, tuple(O.ANCHOR_CONFIGS)),      # floor division of both sides
    (8, 720, 8, 0.3, 359.5, 299.25, tuple(O.ANCHOR_CONFIGS)),   # one row, fractional offsets
    (16, 16, 5, 0.2, 48.0, 48.0, CFG_ONE),                      # odd stride: the half-pixel centre is 2.5; A = 1
    (64, 96, 8, 0.1, 359.5, 299.25, CFG_ONE),
    (24, 40, 8, 0.3, 48.0, 48.0, tuple(O.ANCHOR_CONFIGS)),
)
ANCHOR_EMPTY = (7, 720, 8, 0.2, None, None, tuple(O.ANCHOR_CONFIGS))  # H < stride: no rows


def anchors_ref(case):
    H, W, s, voxel, ox, oy, cfg = case
    return O.generate_anchors(H, W, s, list(cfg), voxel, ox, oy).numpy()


def anchor_offsets(case):
    return (360.0 if case[4] is None else case[4]), (300.0 if case[5] is None else case[5])
