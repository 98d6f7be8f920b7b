"""Weighted box fusion and flip test-time augmentation on the device (ivit_nms_fuse_batched,
ivit_eval_post_tta through utils.py; the contract is in include/ivit.h).

Reference: fuse_cases.reference, sequential f64, over the suppression relation of the sorted rows.
Axis cases sit on a lattice whose IoUs keep 1e-3 from the threshold (test_cpu_fuse_cases.py), so
the relation is computed on the host; rotated cases read it from the device compute_rotated_iou
matrix, the function the mask kernel itself decides with. Leaders, counts, member counts and
intentions are exact and the fused score is bitwise exact. The f64 sums differ from the sequential
reference only by reordering (at most n * 2^-53 relative), so after the one rounding to f32 each
fused x, y, w, l is within max(1 f32 ulp of the reference, 1e-9); yaws are compared modulo 2 pi
within 2^-21."""
import math

import numpy as np
import pytest
import torch

import fuse_cases as F
from oracle import ivit_oracle as O

pytestmark = pytest.mark.gpu

THR = F.THR
EMPTY = F.random_case(0, 1)


def _lists(cases, views=True):
    bl = [torch.from_numpy(c["boxes"]).cuda() for c in cases]
    sl = [torch.from_numpy(c["scores"]).cuda() for c in cases]
    il = [torch.from_numpy(c["intents"]).cuda() for c in cases]
    vl = [torch.from_numpy(c["views"]).cuda() for c in cases] if views else None
    return bl, sl, il, vl


def _run(cases, n_views=1, fuse=True, rotated=False):
    import utils
    bl, sl, il, vl = _lists(cases, views=n_views == 2)
    out = utils.nms_fuse_batched(bl, sl, il, vl, THR, rotated=rotated, fuse=fuse, num_classes=F.K)
    assert len(out) == len(cases)
    for r in out:
        assert r["leaders"].dtype == torch.int64 and r["intentions"].dtype == torch.int64
        assert r["members"].dtype == torch.int32 and r["boxes"].dtype == torch.float32
    return [{k: v.cpu().numpy() for k, v in r.items()} for r in out]


def _rotated_relation(case):
    import utils
    n = case["scores"].shape[0]
    if n == 0:
        return np.zeros((0, 0), bool)
    sb = torch.from_numpy(case["boxes"][F.order_of(case["scores"])]).cuda()
    return utils.compute_rotated_iou(sb, sb).cpu().numpy().astype(np.float64) > THR


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def _check_boxes(got, ref64, tag):
    ref = ref64.astype(np.float32)
    err = np.abs(got[:, :4].astype(np.float64) - ref[:, :4].astype(np.float64))
    tol = np.maximum(F.ulp32(ref[:, :4]), 1e-9)
    assert (err <= tol).all(), (tag, float((err / tol).max()))
    da = (got[:, 4].astype(np.float64) - ref64[:, 4] + math.pi) % (2 * math.pi) - math.pi
    assert (np.abs(da) <= 2.0 ** -21).all(), (tag, float(np.abs(da).max()))


def _check(got, ref, tag, fuse=True):
    assert np.array_equal(got["leaders"], ref["leaders"]), tag
    assert np.array_equal(got["members"], ref["members"]), tag
    assert np.array_equal(got["intentions"], ref["intents"]), tag
    assert np.array_equal(_bits(got["scores"]), _bits(ref["scores"])), tag
    if fuse:
        _check_boxes(got["boxes"], ref["boxes"], tag)
    else:
        assert np.array_equal(_bits(got["boxes"]), _bits(ref["boxes"])), tag


@pytest.fixture(scope="module")
def batch():
    """Every case in one batch; the first sample (size 0) and an inner one are empty. Never modified."""
    named = F.all_cases()
    named.insert(4, ("inner_empty", EMPTY))
    assert named[0][1]["scores"].shape[0] == 0
    return named


@pytest.fixture(scope="module")
def relations(batch):
    return {False: [F.axis_relation(c) for _, c in batch], True: [_rotated_relation(c) for _, c in batch]}


@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("n_views", [1, 2])
def test_fusion_against_the_reference(batch, relations, n_views, rotated):
    got = _run([c for _, c in batch], n_views, True, rotated)
    fused_any = False
    for (name, c), sup, g in zip(batch, relations[rotated], got):
        ref = F.reference(c, sup, n_views=n_views)
        _check(g, ref, (name, n_views, rotated))
        fused_any |= bool((ref["members"] > 1).any())
        if name == "far_member":
            assert g["members"][g["leaders"].tolist().index(0)] == 2
        if name in ("chain", "two_leaders") and not rotated:
            assert sorted(zip(g["leaders"].tolist(), g["members"].tolist())) == [(0, 2), (2, 1)]
    assert fused_any
    for i in (0, 4):
        assert got[i]["leaders"].shape == (0,) and got[i]["boxes"].shape == (0, 5)


@pytest.mark.parametrize("rotated", [False, True])
def test_no_fusion_is_nms_over_the_union(batch, relations, rotated):
    """fuse = 0: the leaders' own rows in keep order; with one view the leaders are nms_batched's keep lists."""
    import utils
    cases = [c for _, c in batch]
    bl, sl, _, _ = _lists(cases)
    keep = utils.nms_batched(bl, sl, THR, rotated=rotated)
    for n_views in (1, 2):
        got = _run(cases, n_views, False, rotated)
        for (name, c), sup, g, k in zip(batch, relations[rotated], got, keep):
            assert np.array_equal(g["leaders"], k.cpu().numpy()), name
            _check(g, F.reference(c, sup, n_views=n_views, fuse=False), (name, n_views), fuse=False)
            assert np.array_equal(_bits(g["scores"]), _bits(c["scores"][g["leaders"]])), name
            assert int(g["members"].sum()) == c["scores"].shape[0], name  # every row belongs to one cluster


@pytest.mark.parametrize("rotated", [False, True])
def test_bitwise_repeatable_and_independent_of_the_batch(batch, rotated):
    cases = [c for _, c in batch]
    a = _run(cases, 2, True, rotated)
    b = _run(cases, 2, True, rotated)
    for (name, _), x, y in zip(batch, a, b):
        for key in x:
            assert np.array_equal(x[key].view(np.uint8), y[key].view(np.uint8)), (name, key)
    for i in (len(cases) - 1, [n for n, _ in batch].index("n700"), [n for n, _ in batch].index("one_cluster")):
        alone = _run([cases[i]], 2, True, rotated)[0]
        for key in alone:
            assert np.array_equal(alone[key].view(np.uint8), a[i][key].view(np.uint8)), (batch[i][0], key)


@pytest.mark.parametrize("rotated", [False, True])
def test_mirror_property(batch, relations, rotated):
    """View 1 an exact copy of view 0: the same leaders, the leader's score bit for bit (the two
    maxima are equal), and the one-view fusion's boxes (every weight doubled)."""
    names = ("n65", "n129", "n700", "one_cluster", "far_member", "equal_scores")
    picked = [(n, c, sup) for (n, c), sup in zip(batch, relations[rotated]) if n in names]
    doubled = []
    for _, c, _ in picked:
        n = c["scores"].shape[0]
        doubled.append({"boxes": np.concatenate([c["boxes"]] * 2), "scores": np.concatenate([c["scores"]] * 2),
                        "intents": np.concatenate([c["intents"]] * 2),
                        "views": np.concatenate([np.zeros(n, np.int32), np.ones(n, np.int32)])})
    got = _run(doubled, 2, True, rotated)
    for (name, c, sup), g in zip(picked, got):
        ref = F.reference(c, sup, n_views=1)
        assert np.array_equal(g["leaders"], ref["leaders"]), name
        assert np.array_equal(_bits(g["scores"]), _bits(c["scores"][g["leaders"]])), name
        assert np.array_equal(g["members"], 2 * ref["members"]), name
        assert np.array_equal(g["intentions"], ref["intents"]), name
        _check_boxes(g["boxes"], ref["boxes"], name)


# ---------------------------------------------------------------- ivit_eval_post_tta
B_POST, NA_POST, K_POST = 3, 130, 8


@pytest.fixture(scope="module")
def post_inputs():
    """Two views' logits at B = 3, NA = 130 (three mask words per view, the last partial); nothing
    passes in the first sample. The anchors are the first rows of a grid that is symmetric about
    y = 0, so the un-mirrored second view lands on the first one's boxes."""
    import utils
    g = torch.Generator().manual_seed(17)
    anchors = utils.generate_anchors(64, 96, 8, offset_x_px=48.0, offset_y_px=48.0, device="cuda")[:NA_POST]
    views = []
    for _ in range(2):
        cls = torch.randn(B_POST, NA_POST, 1, generator=g) * 2.0
        cls[0] = -20.0
        views.append((cls.cuda(), (torch.randn(B_POST, NA_POST, 6, generator=g) * 0.3).cuda(),
                      torch.randn(B_POST, NA_POST, K_POST, generator=g).cuda()))
    return anchors.contiguous(), views


def _same(p, q, keys=("pred_scores", "pred_boxes_xywha", "pred_intentions")):
    for key in keys:
        assert p[key].dtype == q[key].dtype and torch.equal(p[key], q[key]), key


@pytest.mark.parametrize("rotated", [False, True])
def test_eval_post_tta_one_view_without_fusion_is_eval_post(post_inputs, rotated):
    import _lib
    import utils
    anchors, views = post_inputs
    want = utils.postprocess_batch(*views[0], anchors, 0.1, THR, rotated_nms=rotated)
    assert want[0]["pred_scores"].numel() == 0 and 0 < want[1]["pred_scores"].numel() < NA_POST
    # through the new entry: the launch helper with one view and fuse = 0
    got = utils._post_collect(utils._post_launch_tta([views[0]], anchors, 0.1, THR, rotated, False))
    for p, q in zip(got, want):
        _same(p, q)
        assert p["pred_members"].dtype == torch.int32
        assert p["pred_members"].numel() == q["pred_scores"].numel()
    passing = (torch.sigmoid(views[0][0].reshape(B_POST, NA_POST)) >= 0.1).sum(1).cpu().tolist()
    assert [int(p["pred_members"].sum()) for p in got] == passing
    # and with the member counts not asked for (the leaders' rows are copied straight out)
    dev = anchors.device
    sc = torch.empty((B_POST, NA_POST), device=dev)
    bx = torch.empty((B_POST, NA_POST, 5), device=dev)
    ii = torch.empty((B_POST, NA_POST), dtype=torch.int64, device=dev)
    cnt = torch.empty((B_POST,), dtype=torch.int64, device=dev)
    ws = _lib.workspace(_lib.lib.ivit_eval_post_tta_workspace(B_POST, 1, NA_POST, int(rotated)), dev)
    c, r, t = (x.reshape(B_POST, NA_POST, -1).contiguous() for x in views[0])
    _lib.lib.ivit_eval_post_tta(_lib.ptr(c), _lib.ptr(r), _lib.ptr(t), _lib.ptr(anchors), 1, B_POST, NA_POST, K_POST,
                                None, 0.1, THR, int(rotated), 0, _lib.ptr(sc), _lib.ptr(bx), _lib.ptr(ii), None,
                                _lib.ptr(cnt), _lib.ptr(ws), ws.numel(), _lib.stream())
    for b, q in enumerate(want):
        n = int(cnt[b])
        _same({"pred_scores": sc[b, :n], "pred_boxes_xywha": bx[b, :n], "pred_intentions": ii[b, :n]}, q)


def _union_candidates(anchors, views, n_views):
    """Per sample what ivit_eval_post_tta selects: each view's passing rows from postprocess_batch
    with nms_threshold = 1.0 (nothing is suppressed there), view 1 un-mirrored in torch."""
    import utils
    flip = torch.from_numpy(utils._FLIP_INTENTION).cuda()
    per_view = [utils.postprocess_batch(*views[v], anchors, 0.1, 1.0) for v in range(n_views)]
    bl, sl, il, vl = [], [], [], []
    for b in range(B_POST):
        bs, ss, is_, vs = [], [], [], []
        for v in range(n_views):
            p = per_view[v][b]
            box = p["pred_boxes_xywha"].clone()
            it = p["pred_intentions"]
            if v == 1:
                box[:, 1] = -box[:, 1]
                box[:, 4] = -box[:, 4]
                it = flip[it]
            bs.append(box)
            ss.append(p["pred_scores"])
            is_.append(it)
            vs.append(torch.full_like(it, v))
        bl.append(torch.cat(bs))
        sl.append(torch.cat(ss))
        il.append(torch.cat(is_))
        vl.append(torch.cat(vs))
    return bl, sl, il, vl


@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("n_views", [1, 2])
def test_eval_post_tta_equals_nms_fuse_batched(post_inputs, n_views, fuse, rotated):
    import utils
    anchors, views = post_inputs
    bl, sl, il, vl = _union_candidates(anchors, views, n_views)
    want = utils.nms_fuse_batched(bl, sl, il, vl if n_views == 2 else None, THR, rotated=rotated, fuse=fuse,
                                  num_classes=K_POST)
    if fuse or n_views == 2:
        got = utils.postprocess_batch(*views[0], anchors, 0.1, THR, rotated_nms=rotated,
                                      tta_logits=views[1] if n_views == 2 else None, fuse_boxes=fuse)
    else:  # neither option is postprocess_batch's plain path: the new entry through its launch helper
        got = utils._post_collect(utils._post_launch_tta([views[0]], anchors, 0.1, THR, rotated, False))
    assert got[0]["pred_scores"].numel() == 0 and got[0]["pred_members"].numel() == 0
    for b, (p, w) in enumerate(zip(got, want)):
        assert torch.equal(p["pred_scores"], w["scores"]), b
        assert torch.equal(p["pred_boxes_xywha"], w["boxes"]), b
        assert torch.equal(p["pred_intentions"], w["intentions"]), b
        assert torch.equal(p["pred_members"], w["members"]), b
    for b in (1, 2):
        assert int(got[b]["pred_members"].max()) > 1 and int(got[b]["pred_members"].sum()) == bl[b].shape[0]
        if n_views == 2:  # clusters that hold both views: the two-view score rule is in play
            lead = want[b]["leaders"]
            if fuse:
                assert not torch.equal(got[b]["pred_scores"], sl[b][lead])
                assert bool((got[b]["pred_scores"][:-1] >= got[b]["pred_scores"][1:]).all())
            else:
                assert torch.equal(got[b]["pred_scores"], sl[b][lead])
                assert bool((vl[b][lead] == 1).any()) and bool((vl[b][lead] == 0).any())


# ---------------------------------------------------------------- the Python layer
def test_flip_bev_batch_is_the_last_axis_mirror():
    import utils
    g = torch.Generator().manual_seed(3)
    lidar = torch.rand(2, 7, 24, 40, generator=g).cuda()
    mp = (torch.rand(2, 3, 24, 40, generator=g) < 0.3).float().cuda()
    fl, fm = utils.flip_bev_batch(lidar, mp)
    assert fl.data_ptr() != lidar.data_ptr() and fl.shape == lidar.shape and fm.shape == mp.shape
    assert torch.equal(fl, torch.flip(lidar, dims=[-1])) and torch.equal(fm, torch.flip(mp, dims=[-1]))
    bl, bm = utils.flip_bev_batch(fl, fm)
    assert torch.equal(bl, lidar) and torch.equal(bm, mp)


def _batches(n, B, NA, seed):
    g = torch.Generator().manual_seed(seed)
    return [[(torch.randn(B, NA, generator=g) * 2.0, torch.randn(B, NA, 6, generator=g) * 0.3,
              torch.round(torch.randn(B, NA, 8, generator=g))) for _ in range(2)] for _ in range(n)]


@pytest.mark.parametrize("rotated", [False, True])
def test_post_pipeline_tta_equals_per_batch_postprocess(rotated):
    import utils
    anchors = utils.generate_anchors(64, 96, 8, offset_x_px=48.0, offset_y_px=48.0, device="cuda")
    batches = [[tuple(t.cuda() for t in v) for v in vs] for vs in _batches(3, 2, anchors.shape[0], 6)]
    want = [utils.postprocess_batch(*v0, anchors, rotated_nms=rotated, tta_logits=v1, fuse_boxes=True)
            for v0, v1 in batches]
    want = [[{k: v.cpu() for k, v in p.items()} for p in w] for w in want]
    pipe = utils.PostPipeline(anchors, rotated_nms=rotated, tta_flip=True, fuse_boxes=True)
    got = []
    for v0, v1 in batches:
        prev = pipe.push(*v0, tta_logits=v1)
        if prev is not None:
            got.append([{k: v.cpu() for k, v in p.items()} for p in prev])
    got.append([{k: v.cpu() for k, v in p.items()} for p in pipe.flush()])
    assert pipe.flush() is None and len(got) == len(want) == 3
    for k, (gb, wb) in enumerate(zip(got, want)):
        assert len(gb) == len(wb) == 2, k
        for p, q in zip(gb, wb):
            assert q["pred_scores"].numel() > 0 and int(q["pred_members"].max()) > 1
            assert set(p) == set(q) == {"pred_scores", "pred_boxes_xywha", "pred_intentions", "pred_members"}
            for key in q:
                assert torch.equal(p[key], q[key]), (k, key)


@pytest.mark.parametrize("n_views", [1, 2])
def test_chunked_and_unchunked_agree_bitwise(n_views):
    import utils
    anchors = utils.generate_anchors(64, 96, 8, offset_x_px=48.0, offset_y_px=48.0, device="cuda")
    B = 5
    v0, v1 = [tuple(t.cuda() for t in v) for v in _batches(1, B, anchors.shape[0], 9)[0]]
    tta = v1 if n_views == 2 else None
    assert utils.tta_chunk(B, n_views, anchors.shape[0]) < B  # the default rule splits this batch
    runs = [utils.postprocess_batch(*v0, anchors, tta_logits=tta, fuse_boxes=True, tta_chunk_size=c)
            for c in (None, 1, 2, B)]
    for other in runs[1:]:
        for p, q in zip(runs[0], other):
            assert p["pred_scores"].numel() > 0
            for key in p:
                assert torch.equal(p[key], q[key]), key


@pytest.mark.parametrize("rotated_nms", [False, True])
def test_eval_vit_tta_fuse_entry_point(rotated_nms, capsys):
    import eval_vit
    rc = eval_vit.main_eval_vit(["--synthetic", "--checkpoint", "/nonexistent.pth", "--batch", "2", "--batches", "1",
                                 "--grid", "32x48", "--tta-flip", "--fuse-boxes"]
                                + (["--rotated-nms"] if rotated_nms else []))
    out = capsys.readouterr().out
    print(out)
    assert rc == 0
    assert "flip TTA: True, weighted box fusion: True" in out and "mAP @ IoU=0.5" in out
    assert "Collected results for 2 samples" in out
