"""The conditions test_gpu_box_fuse.py relies on (CPU): the axis cases' IoUs keep their distance
from the threshold, the alignment never sits at a half turn, no intention vote is close, the case
sets hold the listed shapes; the workspace queries are pure host functions, the chunking rule keeps
the workspace within its bound, and bad arguments are refused before the device is touched."""
import math
import os

import numpy as np
import pytest

import fuse_cases as F
from conftest import REPO

LIB = os.path.join(REPO, "visiontransformer-intention-prediction_amd", "libivit_hip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libivit_hip.so not built (run __graft_entry__.build())")


@pytest.fixture(scope="module")
def cases():
    return F.all_cases()


@pytest.fixture(scope="module")
def refs(cases):
    return {name: {v: F.reference(c, F.axis_relation(c), n_views=v) for v in (1, 2)} for name, c in cases}


def test_axis_ious_keep_their_distance_from_the_threshold(cases):
    for name, c in cases:
        b = c["boxes"].astype(np.float64)
        assert np.array_equal(b[:, :4] * 2, np.round(b[:, :4] * 2)), name  # the 0.5 lattice: exact corners
        if b.shape[0]:
            assert np.abs(F.axis_iou_matrix(b) - F.THR).min() >= 1e-3, name


def test_alignment_and_vote_margins(refs):
    for name, r in refs.items():
        for v in (1, 2):
            assert r[v]["turn_margin"] >= 1e-3, (name, v)
            assert r[v]["vote_margin"] >= 1e-6, (name, v)


def test_case_sets_hold_the_listed_shapes(cases, refs):
    by = dict(cases)
    assert tuple(c["scores"].shape[0] for c in F.sized_cases()) == F.SIZES == (0, 1, 2, 63, 64, 65, 129, 700)
    assert refs["one_cluster"][1]["members"].tolist() == [65]
    assert refs["singletons"][1]["members"].tolist() == [1] * 64
    # the chain: {A, B}, {C}; with C ahead of B, B still goes to A, the earlier of its two leaders
    for name in ("chain", "two_leaders"):
        r = refs[name][1]
        assert sorted(zip(r["leaders"].tolist(), r["members"].tolist())) == [(0, 2), (2, 1)], name
        sup = F.axis_relation(by[name])
        o = F.order_of(by[name]["scores"]).tolist()
        assert sup[o.index(0)][o.index(1)] and sup[o.index(2)][o.index(1)] and not sup[o.index(0)][o.index(2)]
    far = by["far_member"]
    o = F.order_of(far["scores"]).tolist()
    assert o.index(far["scores"].shape[0] - 1) - o.index(0) > 192
    assert refs["far_member"][2]["members"][0] == 2 and refs["far_member"][2]["leaders"][0] == 0
    eq = by["equal_scores"]
    assert np.unique(eq["scores"]).size == 1 and refs["equal_scores"][1]["leaders"].tolist() == [0, 5]
    # view mixes, both rectangle forms and leaders just inside +-pi, in the large random case
    big, rb = by["n700"], refs["n700"][2]
    o = F.order_of(big["scores"])
    kinds = set()
    sup = F.axis_relation(big)
    pos = {int(r): p for p, r in enumerate(o)}
    for lead, m in zip(rb["leaders"], rb["members"]):
        p = pos[int(lead)]
        rows = [int(lead)] + [int(o[q]) for q in np.nonzero(sup[p])[0] if q > p]
        assert len(rows) == m  # objects do not overlap: a leader's row names exactly its cluster
        kinds.add(frozenset(int(big["views"][r]) for r in rows))
    assert {frozenset({0}), frozenset({1}), frozenset({0, 1})} <= kinds
    lead_a = np.abs(big["boxes"][rb["leaders"], 4])
    assert (lead_a > math.pi - 0.25).any() and (big["boxes"][rb["leaders"], 4] < -math.pi + 0.25).any()
    turns = set()
    for lead in rb["leaders"]:
        near = np.nonzero(np.hypot(*(big["boxes"][:, :2] - big["boxes"][lead, :2]).T) < 2.0)[0]
        for r in near:
            turns.add(int(round((float(big["boxes"][r, 4]) - float(big["boxes"][lead, 4])) / F.HALF_PI)) % 4)
    assert turns == {0, 1, 2, 3}
    assert rb["members"].max() >= 3 and (rb["members"] == 1).any()


def test_reference_hand_values():
    """Two rows of one object, the second a quarter turn on: (4, 6, 0.1) and (6.5, 4, 0.1 + pi/2 + 0.06)."""
    c = F._case([[0, 0, 4, 6, 0.1, 0.75, 1, 0], [1, 0, 6.5, 4, 0.1 + F.HALF_PI + 0.06, 0.25, 2, 1]])
    r = F.reference(c, np.array([[False, True], [False, False]]), n_views=2)
    assert r["leaders"].tolist() == [0] and r["members"].tolist() == [2] and r["intents"].tolist() == [1]
    assert r["scores"][0] == np.float32(0.5)  # (0.75 + 0.25) / 2
    np.testing.assert_allclose(r["boxes"][0], [0.25, 0.0, 4.0, 6.125, 0.1 + 0.25 * 0.06], atol=1e-7)
    one = F.reference(c, np.array([[False, True], [False, False]]), n_views=1)
    assert one["scores"][0] == np.float32(0.75)
    keep = F.reference(c, np.array([[False, True], [False, False]]), n_views=2, fuse=False)
    assert keep["scores"][0] == np.float32(0.75) and keep["boxes"][0].tolist() == c["boxes"][0].astype(float).tolist()
    # near +pi the fused yaw wraps into (-pi, pi]
    w = F._case([[0, 0, 4, 6, math.pi - 0.01, 0.5, 0, 0], [0, 0, 4, 6, -math.pi + 0.03, 0.5, 0, 0]])
    rw = F.reference(w, np.array([[False, True], [False, False]]))
    assert -math.pi < rw["boxes"][0][4] <= math.pi and abs(rw["boxes"][0][4] - (-math.pi + 0.01)) < 1e-6


@needs_lib
def test_workspace_queries_are_pure_host_and_monotone():
    import _lib
    dll = _lib.lib.load()
    assert dll.ivit_nms_fuse_batched_workspace(0, 0, 0, 0) == 64
    assert dll.ivit_eval_post_tta_workspace(0, 2, 22500, 0) == 64
    for rot in (0, 1):
        base = (dll.ivit_nms_rotated_batched_workspace if rot else dll.ivit_nms_batched_workspace)(3, 1000, 16000)
        assert dll.ivit_nms_fuse_batched_workspace(3, 1000, 16000, rot) == base + 28 * 1000
        prev = 0
        for total in (1, 64, 65, 1000, 5000):
            cur = dll.ivit_nms_fuse_batched_workspace(2, total, total * 4, rot)
            assert cur > prev
            prev = cur
        post = dll.ivit_eval_post_rotated_workspace if rot else dll.ivit_eval_post_workspace
        for V in (1, 2):
            prev = 0
            for B in (1, 2, 3, 8, 32):
                cur = dll.ivit_eval_post_tta_workspace(B, V, 22500, rot)
                assert cur > prev and cur >= post(B, V * 22500)
                prev = cur
        assert dll.ivit_eval_post_tta_workspace(4, 2, 1000, rot) > dll.ivit_eval_post_tta_workspace(4, 1, 1000, rot)
        assert dll.ivit_eval_post_tta_workspace(4, 2, 1001, rot) >= dll.ivit_eval_post_tta_workspace(4, 2, 1000, rot)


@needs_lib
@pytest.mark.parametrize("rotated", [False, True])
def test_chunking_rule_keeps_the_workspace_within_its_bound(rotated):
    import _lib
    import utils
    dll = _lib.lib.load()
    post = dll.ivit_eval_post_rotated_workspace if rotated else dll.ivit_eval_post_workspace
    for B, NA in ((32, 22500), (8, 22500), (5, 130), (16, 4500), (64, 1000)):
        for V in (1, 2):
            Bc = utils.tta_chunk(B, V, NA, rotated)
            assert 1 <= Bc <= B
            fits = dll.ivit_eval_post_tta_workspace(Bc, V, NA, int(rotated)) <= post(B, NA)
            assert fits, (B, NA, V, Bc)
            if Bc < B:  # and the largest such chunk
                assert dll.ivit_eval_post_tta_workspace(Bc + 1, V, NA, int(rotated)) > post(B, NA)
    assert 6 <= utils.tta_chunk(32, 2, 22500, rotated) <= 8  # about B / 4 for two views
    assert utils.tta_chunk(1, 2, 22500, rotated) == 1  # one sample cannot be split: the floor of the rule


@needs_lib
def test_bad_arguments_are_refused_without_a_device():
    import _lib
    dll = _lib.lib.load()
    big = 1 << 40

    def fuse(n_views=1, K=8, max_n=10, work_bytes=big):
        return dll.ivit_nms_fuse_batched(None, None, None, None, None, None, 1, 10, max_n, 10, K, n_views, 1, 0, 0.2,
                                         None, None, None, None, None, None, None, work_bytes, None)

    def tta(V=2, K=8, NA=100, work_bytes=big):
        return dll.ivit_eval_post_tta(None, None, None, None, V, 2, NA, K, None, 0.1, 0.2, 0, 1, None, None, None,
                                      None, None, None, work_bytes, None)

    for call, word in ((lambda: fuse(n_views=3), b"n_views"), (lambda: fuse(n_views=0), b"n_views"),
                       (lambda: fuse(K=33), b"K must"), (lambda: fuse(K=0), b"K must"),
                       (lambda: fuse(max_n=131073), b"exceeds"), (lambda: fuse(work_bytes=64), b"workspace too small"),
                       (lambda: tta(V=3), b"V must"), (lambda: tta(K=33), b"K must"),
                       (lambda: tta(NA=65537), b"exceeds"), (lambda: tta(work_bytes=64), b"workspace too small")):
        assert call() < 0
        assert word in dll.ivit_last_error(), (word, dll.ivit_last_error())
    assert tta(V=1, NA=131072, work_bytes=64) < 0 and b"workspace too small" in dll.ivit_last_error()
    flip = (__import__("ctypes").c_int * 8)(0, 2, 1, 4, 3, 5, 6, 9)
    rc = dll.ivit_eval_post_tta(None, None, None, None, 2, 2, 100, 8, flip, 0.1, 0.2, 0, 1, None, None, None, None,
                                None, None, big, None)
    assert rc < 0 and b"flip_intent" in dll.ivit_last_error()
    with pytest.raises(RuntimeError, match="ivit_nms_fuse_batched failed"):
        _lib.lib.ivit_nms_fuse_batched(None, None, None, None, None, None, 1, 10, 10, 10, 8, 3, 1, 0, 0.2, None, None,
                                       None, None, None, None, None, big, None)


def test_eval_flags_parse_and_default_off():
    import constants
    import eval_vit
    assert constants.EVAL_TTA_FLIP is False and constants.EVAL_FUSE_BOXES is False
    a = eval_vit.parse_args(["--synthetic"])
    assert a.tta_flip is False and a.fuse_boxes is False
    b = eval_vit.parse_args(["--synthetic", "--tta-flip", "--fuse-boxes", "--rotated-nms"])
    assert b.tta_flip and b.fuse_boxes and b.rotated_nms
    assert eval_vit.parse_args(["--fuse-boxes"]).tta_flip is False


def test_default_post_call_is_unchanged(monkeypatch):
    """Without the options postprocess_batch and PostPipeline make the call they always made; with
    them they go through the TTA launch with the views in order."""
    import torch
    import utils
    calls = []
    monkeypatch.setattr(utils, "_post_launch", lambda *a, **k: calls.append(("plain", len(a), k)) or "L")
    monkeypatch.setattr(utils, "_post_launch_tta", lambda views, *a, **k: calls.append(("tta", len(views), a[3:])) or "T")
    monkeypatch.setattr(utils, "_post_collect", lambda p: [p])
    anchors = torch.zeros(4, 5)
    x = (torch.zeros(2, 4), torch.zeros(2, 4, 6), torch.zeros(2, 4, 8))
    assert utils.postprocess_batch(*x, anchors) == ["L"]
    assert utils.postprocess_batch(*x, anchors, fuse_boxes=True) == ["T"]
    assert utils.postprocess_batch(*x, anchors, rotated_nms=True, tta_logits=x) == ["T"]
    pipe = utils.PostPipeline(anchors)
    pipe.push(*x)
    assert pipe.flush() == ["L"]
    pipe = utils.PostPipeline(anchors, tta_flip=True, fuse_boxes=True)
    pipe.push(*x, tta_logits=x)
    assert pipe.flush() == ["T"]
    with pytest.raises(ValueError):
        pipe.push(*x)
    assert calls == [("plain", 7, {}), ("tta", 1, (False, True, None)), ("tta", 2, (True, False, None)),
                     ("plain", 6, {}), ("tta", 2, (False, True))]
