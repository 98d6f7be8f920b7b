"""Rotated NMS on the device (ivit_nms_rotated_batched / ivit_eval_post_rotated through utils.py).

The definition is greedy NMS in torchvision's form with the IoU swapped: stable descending sort of
the scores, and sorted box p suppresses a later sorted box q iff
(double)compute_rotated_iou(sorted, sorted)[p, q] > thr. The device takes that decision with the
same function, so the reference below (the greedy walk over the IoU matrix read back from the
device) must be met with array_equal, without a margin around the threshold."""
import math

import numpy as np
import pytest
import torch

from oracle import ivit_oracle as O

pytestmark = pytest.mark.gpu

THR = 0.2
SIZES = (1, 63, 64, 65, 129, 700, 1300)
# side of the square the centres are drawn from, per sqrt(n): about 0.3 boxes per square metre,
# at which 60-75 % of the boxes survive the walk at THR (the CPU oracle's walk, every size below)
SIDE_PER_SQRT_N = 1.8
ORACLE_N, ORACLE_SEED = 150, 3


def _family(n, seed, side=None):
    """n boxes: centres uniform in a square of side SIDE_PER_SQRT_N * sqrt(n), w in [0.5, 2.5],
    l in [1, 6], yaw in (-pi, pi], scores quantised to 1/8 (mass ties)."""
    rng = np.random.default_rng(seed)
    side = SIDE_PER_SQRT_N * math.sqrt(n) if side is None else side
    b = np.empty((n, 5), np.float32)
    b[:, 0:2] = rng.uniform(0.0, side, (n, 2))
    b[:, 2] = rng.uniform(0.5, 2.5, n)
    b[:, 3] = rng.uniform(1.0, 6.0, n)
    b[:, 4] = -rng.uniform(-math.pi, math.pi, n)  # (-pi, pi]
    s = (np.round(rng.uniform(0.0, 1.0, n) * 8.0) / 8.0).astype(np.float32)
    return b, s


def _walk(iou, thr):
    """Greedy walk over the upper triangle of the IoU matrix of the SORTED boxes -> kept positions."""
    n = iou.shape[0]
    sup = np.zeros(n, bool)
    keep = []
    for p in range(n):
        if sup[p]:
            continue
        keep.append(p)
        sup[p + 1:] |= iou[p, p + 1:].astype(np.float64) > thr
    return np.asarray(keep, np.int64)


def _order(scores):
    s = np.asarray(scores, np.float32) + np.float32(0.0)  # -0 ties with +0
    return np.argsort(-s, kind="stable")


def _ref_keep(boxes, scores, thr):
    """The reference: stable descending sort, device IoU matrix of the sorted boxes, greedy walk."""
    import utils
    boxes = np.asarray(boxes, np.float32).reshape(-1, 5)
    if boxes.shape[0] == 0:
        return np.zeros((0,), np.int64)
    order = _order(scores)
    sb = torch.from_numpy(boxes[order]).cuda()
    iou = utils.compute_rotated_iou(sb, sb).cpu().numpy()
    return order[_walk(iou, thr)]


def _dev(boxes, scores):
    return (torch.from_numpy(np.asarray(boxes, np.float32).reshape(-1, 5)).cuda(),
            torch.from_numpy(np.asarray(scores, np.float32)).cuda())


def _apply(boxes, scores, thr, rotated=True):
    import utils
    b, s = _dev(boxes, scores)
    return utils.apply_nms(b, s, thr, rotated=rotated).cpu().numpy()


def test_hand_cases_rotated_and_axis_disagree_both_ways():
    """Two vehicles crossing at one centre: identical axis-aligned corners (axis NMS drops one),
    rotated IoU 4/36 (both stay). Two boxes nose to tail along x: disjoint axis-aligned corners
    (axis keeps both), rotated IoU 3.5/8.5 (one goes). Both modes asserted: the default did not move."""
    hp = math.pi / 2
    cross = np.array([[0, 0, 2, 10, 0], [0, 0, 2, 10, hp]], np.float32)
    tail = np.array([[0, 0, 1, 6, hp], [2.5, 0, 1, 6, hp]], np.float32)
    s = np.array([0.9, 0.8], np.float32)
    assert _apply(cross, s, THR, rotated=True).tolist() == [0, 1]
    assert _apply(cross, s, THR, rotated=False).tolist() == [0]
    assert _apply(tail, s, THR, rotated=True).tolist() == [0]
    assert _apply(tail, s, THR, rotated=False).tolist() == [0, 1]
    import utils
    bt, st = _dev(tail, s)
    assert utils.apply_nms(bt, st, THR).cpu().tolist() == [0, 1]  # no keyword: the axis-aligned rule


@pytest.fixture(scope="module")
def sized_cases():
    """(boxes, scores, reference keep) per size of SIZES; computed once, never modified."""
    out = []
    for n in SIZES:
        b, s = _family(n, 100 + n)
        ref = _ref_keep(b, s, THR)
        if n >= 63:  # n = 1 has one outcome; every other case is held away from the trivial ends
            assert 0.2 * n < ref.shape[0] < 0.9 * n, (n, ref.shape[0])
        out.append((b, s, ref))
    return out


def test_bitexact_against_iou_matrix_per_size(sized_cases):
    """Row / column block edges (63, 64, 65), the diagonal block, more than one (700) and more than
    two (1300) chunks of NMS_CB column blocks."""
    for b, s, ref in sized_cases:
        got = _apply(b, s, THR)
        assert np.array_equal(got, ref), b.shape[0]


def test_bitexact_against_iou_matrix_batched(sized_cases):
    import utils
    bl, sl = zip(*[_dev(b, s) for b, s, _ in sized_cases])
    got = utils.nms_batched(list(bl), list(sl), THR, rotated=True)
    assert len(got) == len(sized_cases)
    for g, (b, _, ref) in zip(got, sized_cases):
        assert g.dtype == torch.int64
        assert np.array_equal(g.cpu().numpy(), ref), b.shape[0]


def _oracle_keep(boxes, scores, thr):
    """Greedy walk over the CPU oracle's rotated IoU, computed only for the pairs whose centres
    are closer than the sum of the half diagonals (all others are disjoint). Also returns the
    smallest distance of any computed IoU from thr."""
    order = _order(scores)
    sb = boxes[order].astype(np.float32)
    n = sb.shape[0]
    hd = 0.5 * np.hypot(sb[:, 2].astype(np.float64), sb[:, 3].astype(np.float64))
    iou = np.zeros((n, n), np.float32)
    gap = np.inf
    for p in range(n):
        d = np.hypot(sb[p + 1:, 0].astype(np.float64) - sb[p, 0], sb[p + 1:, 1].astype(np.float64) - sb[p, 1])
        for q in (np.nonzero(d < hd[p] + hd[p + 1:])[0] + p + 1):
            v = O.rotated_iou_numpy(sb[p:p + 1], sb[q:q + 1])[0, 0]
            iou[p, q] = v
            gap = min(gap, abs(float(v) - thr))
    return order[_walk(iou, thr)], gap


def test_against_cpu_oracle():
    """An independent implementation (numpy convex clip). The seed was picked on the CPU so that no
    oracle IoU lies within 1e-6 of the threshold; with that, the keep lists must be equal."""
    b, s = _family(ORACLE_N, ORACLE_SEED)
    ref, gap = _oracle_keep(b, s, THR)
    assert gap > 1e-6, gap
    assert 0.2 * ORACLE_N < ref.shape[0] < 0.9 * ORACLE_N
    assert np.array_equal(_apply(b, s, THR), ref)


def _adversaries():
    q = math.pi / 4
    rows = []
    # thin long boxes at +-45 degrees on a 1 m lattice: bounding circles and AABBs overlap hugely,
    # the exact IoU is 0 (parallel neighbours) or tiny (crossing ones)
    for i in range(6):
        for j in range(6):
            rows.append([i * 1.0, j * 1.0, 0.1, 30.0, q if (i + j) % 2 else -q])
    # touching along an edge, at a corner (axis-aligned and rotated)
    rows += [[50, 0, 2, 4, 0], [52, 0, 2, 4, 0], [60, 0, 2, 2, 0], [62, 2, 2, 2, 0],
             [70, 0, 2, 2, q], [70 + 2 * math.sqrt(2.0), 0, 2, 2, q]]
    # exact duplicates
    rows += [[80, 5, 1.7, 4.3, 0.6]] * 5
    # concentric, differing only in yaw
    rows += [[90, 5, 2, 5, k * math.pi / 8] for k in range(8)]
    # zero area
    rows += [[91, 5, 0, 3, 0.3], [90, 5, 0, 0, 0], [90, 5, 2, 5, 0.1]]
    # one NaN / one inf field each, next to finite boxes at the same place
    nan, inf = float("nan"), float("inf")
    rows += [[nan, 5, 2, 5, 0], [90, nan, 2, 5, 0], [90, 5, nan, 5, 0], [90, 5, 2, nan, 0], [90, 5, 2, 5, nan],
             [inf, 5, 2, 5, 0], [90, -inf, 2, 5, 0], [90, 5, inf, 5, 0], [90, 5, 2, inf, 0], [90, 5, 2, 5, inf],
             [3e38, 3e38, 1e38, 1e38, 0.3], [2e6, 0, 3, 3, 0.2], [2e6 + 1, 0, 3, 3, 0.9]]
    # coordinates near 1e4 (f32 spacing ~1e-3) with sizes near 1: a random cloud ...
    rng = np.random.default_rng(7)
    for _ in range(60):
        rows.append([1e4 + rng.uniform(0, 6), 1e4 + rng.uniform(0, 6), rng.uniform(0.5, 1.5), rng.uniform(0.5, 1.5),
                     rng.uniform(-math.pi, math.pi)])
    # ... and diamonds whose centre distance steps across the sum of their half diagonals (sqrt 2)
    for k, dx in enumerate((1.40, 1.413, 1.414, 1.4142, 1.4143, 1.415, 1.42)):
        rows += [[1e4 + 20, 1e4 + 3 * k, 1, 1, q], [1e4 + 20 + dx, 1e4 + 3 * k, 1, 1, q]]
    b = np.asarray(rows, np.float32)
    s = (np.round(rng.uniform(0.0, 1.0, b.shape[0]) * 16.0) / 16.0).astype(np.float32)
    return b, s


@pytest.mark.parametrize("thr", [THR, 0.0])
def test_prefilter_adversaries_bitexact(thr):
    """Boxes chosen against the f32 prefilter (it may only reject pairs whose exact IoU is 0, and
    never one with a non-finite operand); thr = 0 makes any wrongly rejected overlap visible."""
    b, s = _adversaries()
    ref = _ref_keep(b, s, thr)
    assert 1 < ref.shape[0] < b.shape[0]
    assert np.array_equal(_apply(b, s, thr), ref)


def test_thresholds_zero_and_negative():
    b, s = _family(65, 9)
    got0 = _apply(b, s, 0.0)
    assert np.array_equal(got0, _ref_keep(b, s, 0.0))
    assert 1 < got0.shape[0] < 65
    # IoU 0 > -0.5: the first box suppresses every other one, disjoint ones included
    gotn = _apply(b, s, -0.5)
    assert gotn.tolist() == [int(_order(s)[0])]
    assert np.array_equal(gotn, _ref_keep(b, s, -0.5))


def test_empty_segments_in_a_batch():
    """A leading and an inner empty segment: the rotated scan settles n = 0 before it reads anything."""
    import utils
    b10, s10 = _family(10, 21, side=8.0)
    b65, s65 = _family(65, 22)
    e = np.zeros((0, 5), np.float32)
    es = np.zeros((0,), np.float32)
    parts = [(e, es), (b10, s10), (e, es), (b65, s65)]
    bl, sl = zip(*[_dev(b, s) for b, s in parts])
    got = utils.nms_batched(list(bl), list(sl), THR, rotated=True)
    assert [g.numel() for g in got][0::2] == [0, 0]
    for g, (b, s) in zip(got, parts):
        assert g.dtype == torch.int64 and g.is_cuda
        assert np.array_equal(g.cpu().numpy(), _ref_keep(b, s, THR))
    assert 0 < got[1].numel() and 0 < got[3].numel() < 65
    assert utils.apply_nms(bl[0], sl[0], THR, rotated=True).numel() == 0


def _post_reference_rotated(cls, box, it, anchors, conf=0.1, thr=THR):
    """Per sample: torch's GPU sigmoid -> where -> device decode -> matrix-walk NMS -> argmax."""
    import utils
    out = []
    for b in range(cls.shape[0]):
        s = torch.sigmoid(cls[b].reshape(-1).float())
        idx = torch.where(s >= conf)[0]
        if idx.numel() == 0:
            out.append((torch.empty(0), torch.empty((0, 5)), torch.empty(0, dtype=torch.long)))
            continue
        dec = utils.decode_box_predictions(box[b].reshape(-1, 6)[idx], anchors[idx]).cpu()
        keep = torch.from_numpy(_ref_keep(dec.numpy(), s[idx].cpu().numpy(), thr))
        out.append((s[idx].cpu()[keep], dec[keep], torch.argmax(it[b].reshape(cls.shape[1], -1)[idx].cpu()[keep], -1)))
    return out


def test_postprocess_batch_rotated_nms():
    import utils
    g = torch.Generator().manual_seed(5)
    B, NA = 3, 4500
    anchors = O.generate_anchors(240, 600, 8)[:NA]
    cls = torch.randn(B, NA, 1, generator=g) * 2 - 1.0
    cls[0] = -30.0  # nothing passes in the FIRST sample
    box = torch.randn(B, NA, 6, generator=g) * 0.3  # columns 4, 5: non-zero yaw deltas
    it = torch.randn(B, NA, 8, generator=g)
    dev_args = (cls.cuda(), box.cuda(), it.cuda(), anchors.cuda())
    got = utils.postprocess_batch(*dev_args, 0.1, THR, rotated_nms=True)
    want = _post_reference_rotated(*dev_args)
    axis = utils.postprocess_batch(*dev_args, 0.1, THR)
    assert got[0]["pred_scores"].numel() == 0 and got[0]["pred_boxes_xywha"].shape == (0, 5)
    for b, (p, (ws, wb, wi)) in enumerate(zip(got, want)):
        assert torch.equal(p["pred_scores"].cpu(), ws), b
        assert torch.equal(p["pred_boxes_xywha"].cpu(), wb), b
        assert torch.equal(p["pred_intentions"].cpu(), wi), b
        assert p["pred_intentions"].dtype == torch.int64
    for b in (1, 2):
        assert got[b]["pred_scores"].numel() > 0
        assert float(got[b]["pred_boxes_xywha"][:, 4].abs().max()) > 0.1  # the yaw is in play
        ga, aa = got[b]["pred_scores"], axis[b]["pred_scores"]
        assert ga.shape != aa.shape or not torch.equal(ga, aa)  # and changes the outcome


@pytest.mark.parametrize("rotated", [False, True])
def test_postprocess_batch_leading_sample_with_nothing_passing(rotated):
    """NA = 130 (three mask words, the last one partial); samples 0 and 2 have no row above the
    confidence threshold, so the walk of the FIRST sample starts at the front of its buffers."""
    import utils
    from test_gpu_entry import _post_reference
    g = torch.Generator().manual_seed(8)
    B, NA, K = 3, 130, 8
    anchors = O.generate_anchors(64, 96, 8)[:NA]
    cls = torch.randn(B, NA, 1, generator=g) * 2.0
    cls[0] = -20.0
    cls[2] = -20.0
    box = torch.randn(B, NA, 6, generator=g) * 0.3
    it = torch.randn(B, NA, K, generator=g)
    dev_args = (cls.cuda(), box.cuda(), it.cuda(), anchors.cuda())
    want = (_post_reference_rotated if rotated else _post_reference)(*dev_args)
    passing = int((torch.sigmoid(dev_args[0][1].reshape(-1)) >= 0.1).sum())
    assert 1 <= want[1][0].numel() < passing  # the reference keeps a box and suppresses one
    got = utils.postprocess_batch(*dev_args, 0.1, THR, rotated_nms=rotated)
    assert len(got) == B
    for b, (p, (ws, wb, wi)) in enumerate(zip(got, want)):
        assert p["pred_scores"].dtype == torch.float32 and p["pred_boxes_xywha"].dtype == torch.float32
        assert p["pred_intentions"].dtype == torch.int64
        assert torch.equal(p["pred_scores"].cpu(), ws), b
        assert torch.equal(p["pred_boxes_xywha"].cpu(), wb), b
        assert torch.equal(p["pred_intentions"].cpu(), wi), b
    for b in (0, 2):
        assert got[b]["pred_scores"].shape == (0,) and got[b]["pred_boxes_xywha"].shape == (0, 5)
        assert got[b]["pred_intentions"].shape == (0,)


def test_post_pipeline_rotated_equals_per_batch_postprocess():
    import utils
    g = torch.Generator().manual_seed(6)
    anchors = O.generate_anchors(64, 96, 8).cuda()
    NA = anchors.shape[0]
    batches = [(torch.randn(2, NA, generator=g) * 2.0, torch.randn(2, NA, 6, generator=g) * 0.3,
                torch.round(torch.randn(2, NA, 8, generator=g))) for _ in range(3)]
    want = [utils.postprocess_batch(c.cuda(), b.cuda(), i.cuda(), anchors, rotated_nms=True) for c, b, i in batches]
    want = [[{k: v.cpu() for k, v in p.items()} for p in w] for w in want]
    pipe = utils.PostPipeline(anchors, rotated_nms=True)
    got = []
    for c, b, i in batches:
        prev = pipe.push(c.cuda(), b.cuda(), i.cuda())
        if prev is not None:
            got.append([{k: v.cpu() for k, v in p.items()} for p in prev])
    got.append([{k: v.cpu() for k, v in p.items()} for p in pipe.flush()])
    assert pipe.flush() is None and len(got) == len(want) == 3
    for k, (gb, wb) in enumerate(zip(got, want)):
        assert len(gb) == len(wb) == 2, k
        for p, q in zip(gb, wb):
            assert q["pred_scores"].numel() > 0
            for key in q:
                assert torch.equal(p[key], q[key]), (k, key)


def test_eval_vit_rotated_nms_entry_point():
    import eval_vit
    rc = eval_vit.main_eval_vit(["--synthetic", "--checkpoint", "/nonexistent.pth", "--batch", "2", "--batches", "1",
                                 "--grid", "32x48", "--rotated", "--rotated-nms"])
    assert rc == 0
