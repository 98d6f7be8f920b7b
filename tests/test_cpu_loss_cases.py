"""tests/loss_cases.py held to account without a GPU: the explicit f64 reference agrees with f64
autograd of oracle.ivit_oracle.detection_loss wherever autograd is finite, the scenes hold what their
families claim, an f32 restatement of the kernel's formulas meets every bound with a factor 2 to spare,
every planted bug is rejected by at least one case, the rotated cases keep their margins, and the
kernel constants parse."""
import functools

import numpy as np
import pytest
import torch

import loss_cases as LC
from oracle import ivit_oracle as O

F32, F64 = np.float32, np.float64


def _find(case, box):
    """Index of the planted anchor equal to ``box`` (f32)."""
    hit = np.nonzero((case.anchors == np.asarray(box, F32)[None]).all(axis=1))[0]
    assert hit.size >= 1, box
    return int(hit[0])


@functools.lru_cache(maxsize=None)
def _f32(name, bug=None):
    c = LC.case(name)
    return LC.check(c, c.ref, LC.evaluate(c, F32, bugs=(bug,) if bug else (), kernel_form=True))


def test_kernel_constants_and_shapes():
    k = LC.kernel_constants()
    assert k["LB"] > 1 and k["NPART"] == 5
    lb = k["LB"]
    sh = LC.shapes()
    if lb == 256:
        assert sh == ((1, 1), (1, 255), (2, 257), (3, 513), (2, 1025))
    assert sh[0] == (1, 1)
    assert all((B * NA) % lb != 0 for B, NA in sh)             # the last block is never full
    assert any(NA % lb != 0 and B * NA > lb for B, NA in sh)   # a sample boundary inside a block
    assert max(NA for _, NA in sh) > 4 * 256                   # several strides of the best-anchor scan
    used = {LC.SPECS[n][0] for n in LC.CASE_NAMES}
    assert used == set(range(len(sh)))
    assert {LC.SPECS[n][1] for n in LC.CASE_NAMES} == {3, 8}
    assert {LC.SPECS[n][2] for n in LC.CASE_NAMES} == {0, 1, 7}
    assert {LC.SPECS[n][5] for n in LC.CASE_NAMES} == set(range(len(LC.FOCAL)))
    assert {LC.SPECS[n][6] for n in LC.CASE_NAMES} == set(range(len(LC.WEIGHTS)))
    assert {LC.SPECS[n][7] for n in LC.CASE_NAMES} == {"cw", "none", "ds_keep", "ds_null", "ds_dropall", "ds_bitK"}
    assert {LC.SPECS[n][8] for n in LC.CASE_NAMES} == {None, 1.0, 0.37, 0.0, -2.0}


# ----------------------------------------------------------------------------- the scenes
@pytest.mark.parametrize("name", ["ties", "strides"])
def test_anchor_ties_lowest_index_wins(name):
    c = LC.case(name)
    i = c.tie_at
    assert i + 256 < c.NA
    assert np.array_equal(c.anchors[i], c.anchors[i + 1]) and np.array_equal(c.anchors[i], c.anchors[i + 256])
    iou = LC.iou_matrix(c, 0)
    assert iou[i, 0] == iou[:, 0].max() and c.neg_thr <= iou[i, 0] < c.pos_thr    # force-match decides
    assert [int(c.ref.t[0, j]) for j in (i, i + 1, i + 256)] == [1, -1, -1]


def test_gt_ties_first_gt_wins():
    c = LC.case("ties")
    assert np.array_equal(c.gt[0, 1], c.gt[0, 2]) and c.gint[0, 1] != c.gint[0, 2]
    pos = c.ref.t[0] == 1
    hit = pos & (LC.iou_matrix(c, 0)[:, 1] >= c.pos_thr)
    assert hit.sum() >= 5
    assert (c.ref.arg[0][hit] == 1).all() and (c.ref.it[0][hit] == c.gint[0, 1]).all()


@pytest.mark.parametrize("which,want", [("pos", (1, -1)), ("neg", (-1, 0))])
def test_threshold_equalities(which, want):
    eq, nx = LC.case(which + "_eq"), LC.case(which + "_next")
    assert eq.thr_anchor == nx.thr_anchor and eq.thr_iou == nx.thr_iou
    assert np.array_equal(eq.anchors, nx.anchors) and np.array_equal(eq.gt, nx.gt)
    key = which + "_thr"
    assert getattr(eq, key) == eq.thr_iou and getattr(nx, key) == float(np.nextafter(F32(eq.thr_iou), F32(2)))
    a = eq.thr_anchor
    assert (int(eq.ref.t[0, a]), int(nx.ref.t[0, a])) == want


def test_force_match_families():
    c = LC.case("ties")
    b = c.B - 1  # the sample holding A, B, C, D as GT rows 0..3
    iou = LC.iou_matrix(c, b)
    best = iou.argmax(axis=0)
    # best IoU below neg_thr: stays negative
    a4 = _find(c, LC._shift(LC._T4, 0.55))
    i0 = LC.iou_matrix(c, 0)
    assert i0[:, 4].argmax() == a4 and i0[a4, 4] < c.neg_thr and c.ref.t[0, a4] == 0
    # B's best anchor X has argmax A: positive through B, encoded against A
    x = _find(c, LC._shift(LC._A, 0.28))
    assert best[1] == x and best[0] != x and iou[x].argmax() == 0
    assert c.neg_thr <= iou[x, 1] < iou[x, 0] < c.pos_thr
    assert c.ref.t[b, x] == 1 and c.ref.arg[b, x] == 0 and c.ref.it[b, x] == c.gint[b, 0]
    # C and D share the best anchor Y, both in the ignore band
    y = _find(c, LC._shift(LC._C, 0.29))
    assert best[2] == y and best[3] == y and c.neg_thr <= iou[y, 3] < iou[y, 2] < c.pos_thr
    assert c.ref.t[b, y] == 1 and c.ref.arg[b, y] == 2


def test_empty_and_padded():
    c = LC.case("empty_middle")
    assert [int(v) for v in c.ngt] == [6, 0, 7] and (c.ref.t[1] == 0).all()
    assert np.isnan(c.gt[0, 6]).all() or c.gt[0, 6, 0] == F32(1e30) or c.gint[0, 6] == 99
    junk = [(c.gt[b, g], int(c.gint[b, g])) for b in range(c.B) for g in range(int(c.ngt[b]), c.gt.shape[1])]
    assert any(np.isnan(g).all() for g, _ in junk) and any((g == F32(1e30)).all() for g, _ in junk)
    assert any(lab >= c.K for _, lab in junk) and any(lab < 0 for _, lab in junk)
    for n in ("all_empty_g1", "gmax0", "no_pos_far_gt", "one_anchor_empty"):
        c = LC.case(n)
        assert c.ref.stats[LC.ST_NPOS] == 0 and c.ref.stats[LC.ST_CDEN] == 1 and c.ref.stats[LC.ST_IDEN] == 1, n
        assert not c.ref.dbox.any() and not c.ref.dint.any() and c.ref.stats[LC.ST_BOXL] == 0
    assert LC.case("gmax0").G == 0 and int(LC.case("all_empty_g1").ngt.max()) == 0
    assert int(LC.case("no_pos_far_gt").ngt[0]) == 1


def test_term_families_are_planted():
    for n in ("short_block", "ties", "strides", "empty_middle", "neg_eq"):
        c = LC.case(n)
        for sel in (c.ref.t == 0, c.ref.t == 1):
            assert set(F32(LC.CLS_VALUES)) <= set(c.cls[sel].tolist()), n
        d = (c.box.astype(F64) - c.ref.box_t.astype(F32).astype(F64))[c.ref.t == 1]
        beta = F64(F32(c.beta))
        assert (d == 0).any() and (d == beta).any() and (d == -beta).any() and (np.abs(d) > 4).any(), n
        near = np.abs(np.abs(d) / beta - 1.0)
        assert ((near > 0) & (near < 2e-6)).any(), n
    c = LC.case("pos_next")
    assert c.keep is not None and not c.keep.any() and c.ref.stats[LC.ST_KEEP] == 0 and c.ref.stats[LC.ST_IDEN] == 1
    c = LC.case("strides")
    assert c.dominant_mask >> (c.K - 1) & 1 and 1 < c.ref.stats[LC.ST_KEEP] < c.ref.stats[LC.ST_NPOS]
    assert LC.case("pos_eq").keep is None and LC.case("pos_eq").downsampling == 1


# ----------------------------------------------------------------------------- reference vs autograd
def _gt_list(c):
    return [{"boxes_xywha": torch.tensor(c.gt[b, :int(c.ngt[b])]), "intentions": torch.tensor(c.gint[b, :int(c.ngt[b])])}
            for b in range(c.B)]


def _rot_iou(a, b):
    return torch.from_numpy(O.rotated_iou_numpy(a.numpy(), b.numpy()))


@pytest.mark.parametrize("name", LC.CASE_NAMES)
def test_reference_is_autograd_f64(name):
    c, ref = LC.case(name), LC.case(name).ref
    anchors = torch.tensor(c.anchors)
    iou_fn = _rot_iou if c.rotated else O.axis_aligned_iou
    cls_t, box_t, int_t = O.assign_targets(anchors, _gt_list(c), pos_thr=c.pos_thr, neg_thr=c.neg_thr, iou_fn=iou_fn)
    assert np.array_equal(cls_t.numpy(), ref.t) and np.array_equal(int_t.numpy(), ref.it)
    pos = ref.t == 1
    np.testing.assert_allclose(box_t.numpy()[pos], ref.box_t[pos], rtol=1e-6, atol=1e-6)
    ts = [torch.tensor(v).double().requires_grad_(True) for v in (c.cls[..., None], c.box, c.intent)]
    keep = None
    if c.downsampling:
        keep = torch.ones((c.B, c.NA)) if c.keep is None else torch.tensor(c.keep)
    dom = [k for k in range(c.K) if c.dominant_mask >> k & 1]
    cw = None if c.class_w is None else torch.tensor(c.class_w).double()
    d = O.detection_loss(*ts, anchors, _gt_list(c), downsampling=bool(c.downsampling), keep=keep, dominant=dom,
                         class_weights=cw, alpha=c.alpha, gamma=c.gamma, beta=c.beta, w_cls=c.w_cls, w_box=c.w_box,
                         w_int=c.w_int, iou_fn=iou_fn, pos_thr=c.pos_thr, neg_thr=c.neg_thr)
    assert d["num_pos_anchors"] == int(ref.stats[LC.ST_NPOS])
    got = [float(d[k].detach()) for k in ("loss", "cls_loss", "box_loss", "intent_loss")]
    want = [ref.stats[k] for k in (LC.ST_LOSS, LC.ST_CLS, LC.ST_BOXL, LC.ST_INT)]
    np.testing.assert_allclose(got, want, rtol=1e-6)  # the oracle's box targets are rounded to f32
    np.testing.assert_allclose([got[1], got[3]], [want[1], want[3]], rtol=1e-12)
    if not d["loss"].requires_grad:
        assert not ref.dcls.any() and not ref.dbox.any() and not ref.dint.any()
        return
    go = 1.0 if c.go is None else LC.f32r(c.go)
    (d["loss"] * go).backward()
    grads = [np.zeros(t.shape) if t.grad is None else t.grad.numpy() for t in ts]
    s = abs(go)
    refs = (ref.dcls[..., None], LC.dbox_at(c, ref, box_t.numpy()), ref.dint)
    for g, r, nm in zip(grads, refs, ("dcls", "dbox", "dint")):
        fin = np.isfinite(g)
        if c.gamma >= 1 or nm != "dcls":
            assert fin.all(), nm
        else:
            assert fin.mean() > 0.9, nm     # autograd's pow is singular only at the saturated logits
        err = np.abs(g - r)[fin]
        assert (err <= 1e-10 * np.abs(r)[fin] + 1e-13 * s).all(), (nm, float(err.max()))


# ----------------------------------------------------------------------------- bounds have room, and teeth
@pytest.mark.parametrize("name", LC.CASE_NAMES)
def test_f32_restatement_has_room(name):
    r = _f32(name)
    assert set(r) == set(LC.FAMILIES)
    assert max(r.values()) <= 0.5, r


def test_saturated_gradients_are_finite_and_small():
    """gamma in {0, 0.5} at +-17 ... +-110, on negatives and positives: the reference and the f32 fixed form
    are finite, and where the logit is confidently right the gradient is below 1e-6 of its scale."""
    for n in ("strides", "empty_middle", "neg_eq", "short_block_g1"):
        c = LC.case(n)
        assert c.gamma < 1
        got = LC.evaluate(c, F32, kernel_form=True)
        sat = np.abs(c.cls) >= 17
        assert sat.sum() >= 16 and np.isfinite(got.dcls).all() and np.isfinite(c.ref.dcls).all()
        right = sat & (c.ref.t >= 0) & ((c.cls > 0) == (c.ref.t == 1))
        s = abs(float(c.ref.go)) * c.w_cls / c.ref.stats[LC.ST_CDEN]
        assert right.sum() >= 8 and (np.abs(c.ref.dcls[right]) <= 1e-6 * s).all()


@pytest.mark.parametrize("bug", LC.BUGS)
def test_planted_bug_is_rejected(bug):
    caught = [n for n in LC.CASE_NAMES if max(_f32(n, bug).values()) > 1.0]
    print(bug, "rejected by", caught)
    assert caught, bug


def test_rotated_margins():
    assert len(LC.ROTATED_CASES) >= 2
    for n in LC.ROTATED_CASES:
        c = LC.case(n)
        m = LC.rot_margins(c)
        assert min(m) >= 1e-5, (n, m)
        assert int(c.ref.stats[LC.ST_NPOS]) >= 5
    c = LC.case("rotated")
    # yaw 0, pi / 2, an identical rectangle and a contained one are among the pairs
    i6 = _find(c, [LC._T6[0], LC._T6[1], LC._T6[3], LC._T6[2], 0.0])
    assert abs(LC.iou_matrix(c, 0)[i6, 3] - 1.0) < 1e-6 and c.ref.t[0, i6] == 1
    i7 = _find(c, [LC._T7[0] + 0.2, LC._T7[1] - 0.3, 1.0, 2.0, 1.0])
    assert abs(LC.iou_matrix(c, 0)[i7, 4] - 2.0 / 18.0) < 1e-6
    assert (c.anchors[:, 4] == 0).any() and (c.gt[0, :, 4] == F32(np.pi / 2)).any()
