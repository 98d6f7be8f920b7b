"""Cases and the reference for the rotated-IoU regression tests (support module, no tests).

``riou_ref`` is the Sutherland-Hodgman clip of oracle/ivit_oracle.py (``_rect_corners``,
``convex_clip``, ``_poly_area``, the guards of ``rotated_iou_numpy``) restated on torch f64
scalars, so autograd differentiates it. It never calls the library.

All generated boxes are f32-representable numbers held in f64 arrays: the same case feeds the f64
host build of csrc/geom_ad.h and, cast to f32 without change, the device op.
"""
import functools
import math

import numpy as np
import torch

F64 = torch.float64


# ----------------------------------------------------------------------------- reference
def _corners(b):
    cx, cy, w, l, a = b.unbind()
    hw, hl = w / 2.0, l / 2.0
    c, s = torch.cos(a), torch.sin(a)
    return [(lx * c - ly * s + cx, lx * s + ly * c + cy) for lx, ly in ((-hw, -hl), (hw, -hl), (hw, hl), (-hw, hl))]


def _fl(x):
    return float(x.detach()) if torch.is_tensor(x) else float(x)


def _area_signed(P):
    s = 0.0
    for i in range(len(P)):
        j = (i + 1) % len(P)
        s = s + (P[i][0] * P[j][1] - P[i][1] * P[j][0])
    return 0.5 * s


def _ccw(P):
    return P if _fl(_area_signed(P)) >= 0 else P[::-1]


def _clip(P, Q):
    P, Q = _ccw(P), _ccw(Q)
    out = list(P)
    for i in range(len(Q)):
        if not out:
            break
        a, b = Q[i], Q[(i + 1) % len(Q)]
        inp, out = out, []
        ex, ey = b[0] - a[0], b[1] - a[1]

        def side(p):
            return ex * (p[1] - a[1]) - ey * (p[0] - a[0])
        for j in range(len(inp)):
            cur, prv = inp[j], inp[j - 1]
            sc, sp = side(cur), side(prv)
            if _fl(sc) >= 0:
                if _fl(sp) < 0:
                    t = sp / (sp - sc)
                    out.append((prv[0] + t * (cur[0] - prv[0]), prv[1] + t * (cur[1] - prv[1])))
                out.append(cur)
            elif _fl(sp) >= 0:
                t = sp / (sp - sc)
                out.append((prv[0] + t * (cur[0] - prv[0]), prv[1] + t * (cur[1] - prv[1])))
    return out


def riou_ref(box, target):
    """IoU of two rotated boxes as a 0-d f64 tensor connected to ``box`` (a constant 0 where a guard
    of rotated_iou_numpy applies: either area < 1e-6, intersection <= 1e-7, union <= 1e-6)."""
    box = box.to(F64)
    target = target.detach().to(F64)
    P, Q = _corners(box), _corners(target)
    A1, A2 = _area_signed(P).abs(), _area_signed(Q).abs()
    zero = torch.zeros((), dtype=F64)
    if _fl(A1) < 1e-6 or _fl(A2) < 1e-6:
        return zero
    C = _clip(P, Q)
    if len(C) < 3:
        return zero
    inter = _area_signed(C).abs()
    if not _fl(inter) > 1e-7:
        return zero
    u = A1 + A2 - inter
    if not _fl(u) > 1e-6:
        return zero
    return inter / u


def riou_ref_grad(box, target):
    """-> (IoU, dIoU/dbox (5,)) as f64 numpy, from autograd on riou_ref."""
    b = torch.as_tensor(np.asarray(box, np.float64)).clone().requires_grad_(True)
    v = riou_ref(b, torch.as_tensor(np.asarray(target, np.float64)))
    if not v.requires_grad:
        return float(v), np.zeros(5)
    (g,) = torch.autograd.grad(v, b)
    return _fl(v), g.numpy()


def decode_f64(raw, anchor):
    """decode_boxes' formulas in f64 from f32 raw outputs (6,) and an f32 anchor (5,), without the
    final angle wrap (torch, differentiable in ``raw``)."""
    raw, anchor = raw.to(F64), anchor.to(F64)
    return torch.stack([raw[0] * anchor[2] + anchor[0], raw[1] * anchor[3] + anchor[1],
                        torch.exp(raw[2]) * anchor[2], torch.exp(raw[3]) * anchor[3],
                        anchor[4] + torch.atan2(raw[4], raw[5])])


def riou_ref_decoded(raw, anchor, target):
    """-> (IoU, dIoU/draw (6,)) f64 numpy for f32 raw outputs / anchor and an f32 target box."""
    r = torch.as_tensor(np.asarray(raw, np.float32)).to(F64).clone().requires_grad_(True)
    a = torch.as_tensor(np.asarray(anchor, np.float32)).to(F64)
    v = riou_ref(decode_f64(r, a), torch.as_tensor(np.asarray(target, np.float32)).to(F64))
    if not v.requires_grad:
        return float(v), np.zeros(6)
    (g,) = torch.autograd.grad(v, r)
    return _fl(v), g.numpy()


def oracle_iou(box, target):
    """The same IoU from the oracle's own f64 helpers (numpy, value only)."""
    from oracle import ivit_oracle as O
    P, Q = O._rect_corners(box), O._rect_corners(target)
    A1, A2 = O._poly_area(P), O._poly_area(Q)
    if A1 < 1e-6 or A2 < 1e-6:
        return 0.0
    inter = O._poly_area(O.convex_clip(P, Q))
    if not inter > 1e-7:
        return 0.0
    u = A1 + A2 - inter
    return inter / u if u > 1e-6 else 0.0


# ----------------------------------------------------------------------------- cases
def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _np_corners(b):
    cx, cy, w, l, a = b
    c, s = math.cos(a), math.sin(a)
    return [((lx * c - ly * s) + cx, (lx * s + ly * c) + cy)
            for lx, ly in ((-w / 2, -l / 2), (w / 2, -l / 2), (w / 2, l / 2), (-w / 2, l / 2))]


def near_kink(box, target, dist=1e-3, ang=1e-2):
    """A corner of one box within ``dist`` of an edge line of the other, or two edges within ``ang``
    rad of parallel: next to such configurations the IoU's derivative is one-sided."""
    d = (box[4] - target[4]) % (math.pi / 2)
    if min(d, math.pi / 2 - d) < ang:
        return True
    for A, B in ((box, target), (target, box)):
        ca, cb = _np_corners(A), _np_corners(B)
        for i in range(4):
            (x0, y0), (x1, y1) = cb[i], cb[(i + 1) % 4]
            ex, ey = x1 - x0, y1 - y0
            n = math.hypot(ex, ey)
            for (px, py) in ca:
                if abs(ex * (py - y0) - ey * (px - x0)) / n < dist:
                    return True
    return False


def draw_case(rng):
    """One draw of the law: target centre in +-5 m, 1.5-2.5 m x 3.5-6 m, any yaw; prediction = target
    plus N(0, (0.4, 0.4, 0.2, 0.4, 0.25)). f32-representable."""
    t = np.array([rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(1.5, 2.5), rng.uniform(3.5, 6.0),
                  rng.uniform(-math.pi, math.pi)])
    p = t + rng.normal(size=5) * np.array([0.4, 0.4, 0.2, 0.4, 0.25])
    return _f32(p), _f32(t)


@functools.lru_cache(maxsize=None)
def _smooth(seed, n):
    rng = np.random.RandomState(seed)
    boxes, targets, draws = [], [], 0
    while len(boxes) < n:
        p, t = draw_case(rng)
        draws += 1
        if near_kink(p, t):
            continue
        boxes.append(p)
        targets.append(t)
    share = (draws - n) / max(1, draws)
    assert share < 0.2, f"smooth_cases({seed}, {n}) redrew {share:.1%} of its draws"
    return np.array(boxes).reshape(n, 5), np.array(targets).reshape(n, 5), share


def smooth_cases(seed, n):
    """-> (boxes (n, 5), targets (n, 5)) f64 arrays of f32-representable numbers, away from the
    gradient kinks (near_kink cases are redrawn; fewer than 20 % of the draws, asserted)."""
    b, t, _ = _smooth(seed, n)
    return b.copy(), t.copy()


def redraw_share(seed, n):
    return _smooth(seed, n)[2]


def closed_form_cases():
    """[(box, target, iou, grad (5,))]: one box strictly inside the other at a different yaw."""
    small, big = _f32([0.4, -0.1, 1.0, 2.0, 1.0]), _f32([0.3, -0.2, 3.0, 6.0, 0.4])
    out = []
    iou = (small[2] * small[3]) / (big[2] * big[3])
    out.append((small, big, iou, np.array([0.0, 0.0, iou / small[2], iou / small[3], 0.0])))
    out.append((big, small, iou, np.array([0.0, 0.0, -iou / big[2], -iou / big[3], 0.0])))
    return out


def edge_cases():
    """{name: (box, target)} (f64 arrays; inf / nan where named)."""
    inf, nan = float("inf"), float("nan")
    base = [0.0, 0.0, 2.0, 4.0, 0.0]
    c = {"identical": ([1.0, 2.0, 2.0, 4.0, 0.25], [1.0, 2.0, 2.0, 4.0, 0.25]),
         "shared_edge": (base, [2.0, 0.0, 2.0, 4.0, 0.0]),
         "corner_touch": (base, [2.0, 4.0, 2.0, 4.0, 0.0]),
         "disjoint": ([0.0, 0.0, 2.0, 4.0, 0.25], [10.0, 10.0, 2.0, 4.0, 1.0]),
         "zero_w": ([0.0, 0.0, 0.0, 4.0, 0.125], base),
         "w_inf": ([0.0, 0.0, inf, 4.0, 0.0], base),
         "w_nan": ([0.0, 0.0, nan, 4.0, 0.0], base),
         "x_inf": ([inf, 0.0, 2.0, 4.0, 0.0], base),
         "x_nan": ([nan, 0.0, 2.0, 4.0, 0.0], base)}
    return {k: (np.array(b, np.float64), np.array(t, np.float64)) for k, (b, t) in c.items()}


ZERO_CASES = ("disjoint", "zero_w", "corner_touch")
FINITE_CASES = ("identical", "shared_edge")
NAN_CASES = ("w_inf", "w_nan", "x_inf", "x_nan")

# d4 = d5 = 0: atan2(0, 0) = 0, and the two angle derivatives are defined as 0
ZERO_ANGLE_CASE = (np.array([0.1, -0.05, 0.1, -0.1, 0.0, 0.0]), np.array([0.0, 0.0, 2.0, 4.5, 0.5]),
                   np.array([0.2, 0.1, 2.2, 4.4, 0.75]))


@functools.lru_cache(maxsize=None)
def pool(n=257):
    """The op-level pool shared by the tests: the closed-form cases, then smooth_cases(0, n - 2), with
    the reference IoU and gradient of each, computed once. -> (boxes, targets, iou, grad) f64."""
    cf = closed_form_cases()
    sb, st = smooth_cases(0, n - len(cf))
    boxes = np.concatenate([np.array([c[0] for c in cf]), sb])
    targets = np.concatenate([np.array([c[1] for c in cf]), st])
    ref = [riou_ref_grad(b, t) for b, t in zip(boxes, targets)]
    return boxes, targets, np.array([r[0] for r in ref]), np.array([r[1] for r in ref])
