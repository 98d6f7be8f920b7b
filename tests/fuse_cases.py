"""Case generators and the reference for weighted box fusion (ivit_nms_fuse_batched,
ivit_eval_post_tta; the contract is in include/ivit.h).

The reference is a plain sequential f64 implementation that takes the suppression relation of the
SORTED rows as an input matrix: the axis cases compute it from boxes on a lattice (centres and
sizes are multiples of 0.5, so every IoU is an exact rational and test_cpu_fuse_cases.py can hold
all of them 1e-3 away from the threshold), the rotated cases read it from the device IoU matrix.

A case is a dict: boxes [n, 5] f32, scores [n] f32, intents [n] int32, views [n] int32."""
import math

import numpy as np

THR = 0.2
K = 8
SIZES = (0, 1, 2, 63, 64, 65, 129, 700)
PITCH = 40.0  # distance between two objects: far more than any box, so objects never overlap
HALF_PI = math.pi / 2


def order_of(scores):
    s = np.asarray(scores, np.float32) + np.float32(0.0)  # -0 ties with +0
    return np.argsort(-s, kind="stable")


def axis_iou_matrix(b):
    """Exact (f64 on lattice values) IoU of the axis-aligned corners of rows b[:, :4]."""
    b = np.asarray(b, np.float64)
    x1, x2 = b[:, 0] - b[:, 2] / 2, b[:, 0] + b[:, 2] / 2
    y1, y2 = b[:, 1] - b[:, 3] / 2, b[:, 1] + b[:, 3] / 2
    w = np.clip(np.minimum(x2[:, None], x2[None]) - np.maximum(x1[:, None], x1[None]), 0, None)
    h = np.clip(np.minimum(y2[:, None], y2[None]) - np.maximum(y1[:, None], y1[None]), 0, None)
    inter = w * h
    area = (x2 - x1) * (y2 - y1)
    return inter / (area[:, None] + area[None] - inter)


def axis_relation(case, thr=THR):
    """sup[p, q] over the sorted rows."""
    o = order_of(case["scores"])
    return axis_iou_matrix(case["boxes"][o]) > thr


def wrap(a):
    while a > math.pi:
        a -= 2 * math.pi
    while a <= -math.pi:
        a += 2 * math.pi
    return a


def reference(case, sup, n_views=1, fuse=True, k_classes=K):
    """The contract, sequentially. sup: [n, n] bool over the SORTED rows (the upper triangle is
    used). Returns leaders (local rows), boxes (f64, unrounded; the leader's f32 row with
    fuse=False), scores (f32), intents, members, in output order, and the margins the GPU tests rely on:
    'turn_margin' = the least distance of any d / (pi/2) from a half-integer, 'vote_margin' = the
    least relative gap between the best and the second-best vote of a cluster with two voted classes."""
    b = np.asarray(case["boxes"], np.float32)
    s = np.asarray(case["scores"], np.float32)
    it = np.asarray(case["intents"])
    vw = np.asarray(case["views"]) if n_views == 2 else np.zeros(len(s), np.int64)
    n = len(s)
    o = order_of(s)
    owner = [-1] * n
    clusters = []
    for p in range(n):  # the greedy walk: the first leader whose row has q removes q
        if owner[p] != -1:
            continue
        owner[p] = p
        mem = [p]
        for q in range(p + 1, n):
            if owner[q] == -1 and sup[p][q]:
                owner[q] = p
                mem.append(q)
        clusters.append(mem)
    rows, turn_margin, vote_margin = [], math.inf, math.inf
    for mem in clusters:
        lp = int(o[mem[0]])
        if not fuse:
            rows.append((lp, [float(v) for v in b[lp]], s[lp], int(it[lp]), len(mem)))
            continue
        ap = float(b[lp, 4])
        S = sx = sy = sw = sl = sd = 0.0
        votes = [0.0] * k_classes
        m = [None, None]
        for q in mem:
            r = int(o[q])
            sq = float(s[r])
            d = float(b[r, 4]) - ap
            t = d / HALF_PI
            k = round(t)
            turn_margin = min(turn_margin, abs(abs(t - math.floor(t)) - 0.5))
            delta = d - k * HALF_PI
            w, l = (float(b[r, 3]), float(b[r, 2])) if k % 2 else (float(b[r, 2]), float(b[r, 3]))
            S += sq
            sx += sq * float(b[r, 0])
            sy += sq * float(b[r, 1])
            sw += sq * w
            sl += sq * l
            sd += sq * delta
            votes[int(it[r])] += sq
            v = int(vw[r])
            m[v] = s[r] if m[v] is None else max(m[v], s[r])
        top = sorted(votes, reverse=True)
        if top[1] > 0.0:
            vote_margin = min(vote_margin, (top[0] - top[1]) / top[0])
        m0 = np.float32(0.0) if m[0] is None else m[0]
        m1 = np.float32(0.0) if m[1] is None else m[1]
        score = np.float32((m0 + m1) * np.float32(0.5)) if n_views == 2 else m0
        box = [sx / S, sy / S, sw / S, sl / S, wrap(ap + sd / S)]
        rows.append((lp, box, score, int(np.argmax(votes)), len(mem)))
    sc = np.asarray([r[2] for r in rows], np.float32)
    perm = order_of(sc) if rows else np.zeros((0,), np.int64)
    rows = [rows[i] for i in perm]
    return {"leaders": np.asarray([r[0] for r in rows], np.int64),
            "boxes": np.asarray([r[1] for r in rows], np.float64).reshape(-1, 5),
            "scores": np.asarray([r[2] for r in rows], np.float32),
            "intents": np.asarray([r[3] for r in rows], np.int64),
            "members": np.asarray([r[4] for r in rows], np.int32),
            "turn_margin": turn_margin, "vote_margin": vote_margin}


# ---------------------------------------------------------------- generators
def _case(rows):
    a = np.asarray(rows, np.float64).reshape(-1, 8)
    return {"boxes": a[:, :5].astype(np.float32), "scores": a[:, 5].astype(np.float32),
            "intents": a[:, 6].astype(np.int32), "views": a[:, 7].astype(np.int32)}


def _object(rng, cx, cy, size, base_angle=None, view_mode=2, equal_scores=False):
    """`size` candidates of one object: centres within +-0.5 of (cx, cy) on the 0.5 lattice, w in
    {4, 5}, l in {6, 7}, the yaw within +-0.2 of the object's, each row in one of the three forms of
    the same rectangle ((w, l, a), (l, w, a + pi/2), (w, l, a + pi)); most rows vote for the object's
    intention. view_mode 0 / 1: every row of that view; 2: both views occur."""
    base = rng.uniform(-2.5, 2.5) if base_angle is None else base_angle
    intent = int(rng.integers(0, K))
    rows = []
    for i in range(size):
        x = cx + 0.5 * int(rng.integers(-1, 2))
        y = cy + 0.5 * int(rng.integers(-1, 2))
        w, l = 4.0 + int(rng.integers(0, 2)), 6.0 + int(rng.integers(0, 2))
        a = base + rng.uniform(-0.2, 0.2)
        form = int(rng.integers(0, 3))
        if form == 1:
            w, l, a = l, w, a + HALF_PI
        elif form == 2:
            a = a + math.pi
        s = 0.5 if equal_scores else float(rng.uniform(0.15, 0.95))
        c = intent if (i == 0 or rng.uniform() < 0.7) else int(rng.integers(0, K))
        v = view_mode if view_mode < 2 else (i % 2 if i < 2 else int(rng.integers(0, 2)))
        rows.append([x, y, w, l, wrap(a), s, c, v])
    return rows


def random_case(n, seed, max_cluster=6):
    """n rows in clusters of 1..max_cluster rows on a grid of objects; clusters with only view 0,
    only view 1 and both; every fourth object's yaw lies just inside +-pi."""
    rng = np.random.default_rng(seed)
    rows, k = [], 0
    while len(rows) < n:
        size = min(int(rng.integers(1, max_cluster + 1)), n - len(rows))
        ang = None if k % 4 else (math.pi - 1e-3) * (1 if k % 8 else -1)
        rows += _object(rng, PITCH * (k % 16), PITCH * (k // 16), size, ang, view_mode=k % 3)
        k += 1
    perm = rng.permutation(len(rows))  # the members of a cluster are spread over the rows
    return _case([rows[i] for i in perm])


def one_cluster_case(n, seed):
    rng = np.random.default_rng(seed)
    return _case(_object(rng, 0.0, 0.0, n, view_mode=2))


def singletons_case(n, seed):
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(n):
        rows += _object(rng, PITCH * (k % 16), PITCH * (k // 16), 1, view_mode=k % 2)
    return _case(rows)


def chain_case(shared_first=True):
    """A, B, C in a row, 2 apart, 4 x 6 each: IoU(A, B) = IoU(B, C) = 1/3, IoU(A, C) = 0.
    shared_first: scores A > B > C, clusters {A, B}, {C}. Otherwise A > C > B: B is overlapped by
    two leaders and belongs to the earlier one, A."""
    sc = (0.9, 0.8, 0.7) if shared_first else (0.9, 0.7, 0.8)
    return _case([[0, 0, 4, 6, 0.1, sc[0], 1, 0], [2, 0, 4, 6, 0.2, sc[1], 2, 1], [4, 0, 4, 6, 0.3, sc[2], 3, 0]])


def far_member_case(seed, gap=200):
    """A leader, `gap` singletons with scores between, then the leader's member: more than three
    mask words after it in the sorted order."""
    rng = np.random.default_rng(seed)
    rows = [[0, 0, 4, 6, 0.3, 0.99, 2, 0]]
    for k in range(gap):
        rows.append([PITCH * (1 + k % 16), PITCH * (k // 16), 4, 6, 0.0, float(rng.uniform(0.3, 0.9)), 0, k % 2])
    rows.append([0.5, 0.5, 5, 7, 0.35, 0.11, 2, 1])
    return _case(rows)


def equal_scores_case():
    """Two clusters of equal scores: row order decides the leaders; votes 3 : 2 and 2 : 1."""
    rng = np.random.default_rng(5)
    a = _object(rng, 0.0, 0.0, 5, view_mode=2, equal_scores=True)
    b = _object(rng, PITCH, 0.0, 3, view_mode=0, equal_scores=True)
    for r, c in zip(a, (2, 2, 2, 1, 1)):
        r[6] = c
    for r, c in zip(b, (4, 4, 6)):
        r[6] = c
    return _case(a + b)


def sized_cases():
    """One case per size of SIZES."""
    return [random_case(n, 1000 + n) for n in SIZES]


def shape_cases():
    """(name, case) for the listed cluster shapes."""
    return [("one_cluster", one_cluster_case(65, 11)), ("singletons", singletons_case(64, 12)),
            ("chain", chain_case(True)), ("two_leaders", chain_case(False)), ("far_member", far_member_case(13)),
            ("equal_scores", equal_scores_case())]


def all_cases():
    return [(f"n{c['scores'].shape[0]}", c) for c in sized_cases()] + shape_cases()


def ulp32(x):
    x = np.abs(np.asarray(x, np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)
