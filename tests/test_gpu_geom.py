"""The box geometry primitives on the device, called through the C ABI: ivit_generate_anchors,
ivit_axis_iou, ivit_rotated_iou and ivit_decode_boxes against the references of
tests/geom_cases.py (an exact rational clip, the oracle, f64 decode formulas), under the bounds
stated there. tests/test_cpu_geom_cases.py proves the cases, the references and the judges
without a GPU and runs the same cases through a host build of csrc/geom.h.

Every output buffer is 16 elements longer than needed and prefilled with NaN: the tail must stay
NaN and no required element may be NaN where the reference is finite."""
import numpy as np
import pytest
import torch

import geom_cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
I32 = np.int32


def _note(family, ratio):
    """Print a measured err / bound (pytest -s shows it; profiles/geom_parity.txt records a run)."""
    print(f"err / bound {family}: {ratio:.3g}")
    return ratio


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _buf(n, fill=NAN):
    return torch.full((n + G.TAIL,), fill, dtype=torch.float32, device=DEV)


def _untouched(buf, n=0):
    return bool(torch.isnan(buf[n:]).all())


def _matrix(entry, b1, b2, fill=NAN):
    """One ivit_*_iou call -> ([n1, n2] f32 numpy, the whole buffer)."""
    import _lib
    b1, b2 = G.boxes(b1), G.boxes(b2)
    n1, n2 = len(b1), len(b2)
    d1, d2 = _dev(b1), _dev(b2)
    out = _buf(n1 * n2, fill)
    rc = getattr(_lib.lib, entry)(_lib.ptr(d1), n1, _lib.ptr(d2), n2, _lib.ptr(out), _lib.stream())
    torch.cuda.synchronize()
    assert rc == 0
    return out[: n1 * n2].cpu().numpy().reshape(n1, n2), out


# ----------------------------------------------------------------------------- anchors
def test_anchors_bitexact():
    import _lib
    import utils
    for case in G.ANCHOR_CASES + (G.ANCHOR_EMPTY,):
        H, W, s, voxel, _, _, cfg = case
        ox, oy = G.anchor_offsets(case)
        ref = G.anchors_ref(case)
        n = ref.shape[0]
        assert (n == 0) == (case is G.ANCHOR_EMPTY)
        d_cfg = _dev(np.asarray(cfg, np.float32).reshape(-1))
        out = _buf(n * 5)
        rc = _lib.lib.ivit_generate_anchors(H, W, s, _lib.ptr(d_cfg), len(cfg), voxel, ox, oy, _lib.ptr(out), _lib.stream())
        torch.cuda.synchronize()
        assert rc == 0 and _untouched(out, n * 5), case[:6]
        got = out[: n * 5].cpu().numpy().reshape(n, 5)
        assert not np.isnan(got).any() and G.same_bits(got, ref), case[:6]
        via = utils.generate_anchors(H, W, s, list(cfg), voxel, ox, oy, device=DEV)
        assert via.shape == (n, 5) and G.same_bits(via.cpu().numpy(), ref), case[:6]
    # the defaults of utils.generate_anchors are the first case
    assert G.same_bits(utils.generate_anchors(device=DEV).cpu().numpy(), G.anchors_ref(G.ANCHOR_CASES[0]))


# ----------------------------------------------------------------------------- axis IoU
def test_axis_iou_matrix_bitexact():
    for name, (b1, b2) in G.axis_cases().items():
        got, buf = _matrix("ivit_axis_iou", b1, b2)
        ref = G.axis_ref(b1, b2)
        assert _untouched(buf, got.size), name
        assert G.same_bits(got, ref), (name, int((got.view(I32) != ref.view(I32)).sum()))
    for n1, n2 in G.EMPTY_SHAPES:  # an empty side returns before the launch
        rows, cols = G.axis_special_pool()
        got, buf = _matrix("ivit_axis_iou", rows[:n1], cols[:n2])
        assert got.size == 0 and _untouched(buf)


def test_axis_iou_nan_fields_write_every_element():
    """include/ivit.h promises for a NaN field only that the element is written (fmaxf / fminf drop
    a NaN that torch.maximum propagates, so the value is unspecified); the pairs of finite boxes in
    the same matrix still follow the reference bit for bit."""
    b1, b2, rows, cols = G.axis_nan_pool()
    mark = 12345.0  # not an IoU
    got, buf = _matrix("ivit_axis_iou", b1, b2, fill=mark)
    assert (got != mark).all() and bool((buf[got.size:] == mark).all())
    ref = G.axis_ref(b1, b2)
    assert G.same_bits(got[np.ix_(rows, cols)], ref[np.ix_(rows, cols)])


# ----------------------------------------------------------------------------- rotated IoU
def _judge(name, b1, b2, ref):
    got, buf = _matrix("ivit_rotated_iou", b1, b2)
    assert _untouched(buf, got.size), name
    assert not np.isnan(got).any(), name
    worst, fails = G.judge_rotated(got, ref)
    assert not fails, (name, len(fails), fails[:3])
    _note(f"rotated {name}", worst)
    return got


def test_rotated_iou_matrix_bounds():
    fam = G.rot_families()
    sets = {**fam, **{f"shape_{a}x{b}": v for (a, b), v in G.rot_shapes().items()}}
    for name, (b1, b2, ref) in sets.items():
        got = _judge(name, b1, b2, ref)
        # symmetry: iou(b, a) is within the bound of the reference as well; it is not required to
        # be bit-equal to iou(a, b) (geom.h: the clip order shows in the last bits)
        swapped = _judge(f"{name} swapped", b2, b1, G.RotRef(b2, b1, exact=True))
        assert swapped.shape == got.T.shape
    deg = _matrix("ivit_rotated_iou", *fam["degenerate"][:2])[0]
    zero = np.zeros((), np.float32).view(I32)
    assert (deg[1].view(I32) == zero).all() and (deg[:, 2:].view(I32) == zero).all() and (deg > 0.2).sum() == 4
    # the guard cases: a factor 2 below a guard is exactly 0.0f, a factor 2 above it a value
    area = _matrix("ivit_rotated_iou", *fam["area_guard"][:2])[0]
    assert (area[[0, 2]] == 0).all() and (area[:, 2] == 0).all() and (area[[1, 3], :2] > 0).all()
    inter = _matrix("ivit_rotated_iou", *fam["inter_guard"][:2])[0]
    assert (inter[0, [0, 2]] == 0).all() and (inter[0, [1, 3]] > 1e-8).all()
    for n1, n2 in G.EMPTY_SHAPES:
        b1, b2 = fam["random"][:2]
        got, buf = _matrix("ivit_rotated_iou", b1[:n1], b2[:n2])
        assert got.size == 0 and _untouched(buf)


def test_rotated_iou_on_the_families_other_tests_trust():
    """test_gpu_nms_rotated.py, test_gpu_box_fuse.py and test_gpu_det_errors.py read their reference
    relation from this matrix; here the matrix of their own boxes is held to a reference that
    is not the device. No pair is left out: one pruned by its centre distance must be exactly 0.0f."""
    total = 0
    for name, (b1, b2, ref) in G.trusted_families().items():
        _judge(f"trusted {name}", b1, b2, ref)
        total += ref.val.size
    assert total > 150000


# ----------------------------------------------------------------------------- decode
def _decode(rel, anchors, idx):
    import _lib
    n = len(rel)
    d_rel, d_anc = _dev(G.f32(rel)), _dev(G.f32(anchors))
    d_idx = None if idx is None else _dev(np.asarray(idx, np.int64))
    out = _buf(n * 5)
    rc = _lib.lib.ivit_decode_boxes(_lib.ptr(d_rel), _lib.ptr(d_anc), _lib.ptr(d_idx), n, _lib.ptr(out), _lib.stream())
    torch.cuda.synchronize()
    assert rc == 0 and _untouched(out, n * 5)
    return out[: n * 5].cpu().numpy().reshape(n, 5)


def test_decode_bounds():
    c = G.decode_case()
    assert int(c["idx"].max()) < len(c["table"]) and int(c["idx"].min()) >= 0
    for n in G.DEC_SIZES:
        rel, idx = c["rel"][:n], c["idx"][:n]
        anc = c["table"][idx]
        gathered = _decode(rel, c["table"], idx)   # the idx path: rows of the longer table
        plain = _decode(rel, anc, None)            # the same rows gathered beforehand
        assert np.array_equal(gathered.view(I32), plain.view(I32)), n
        assert not np.isnan(plain).any(), n
        worst, fails = G.judge_decode(plain, rel, anc)
        assert not fails, (n, fails)
        if n == G.DEC_N:
            for k, v in worst.items():
                _note(f"decode {k}", v)
            for kind in sorted(set(c["kind"])):
                rows = c["kind"] == kind
                w, _ = G.judge_decode(plain[rows], rel[rows], anc[rows])
                print(f"err / bound decode rows {kind}: size {w['size']:.3g} yaw {w['yaw']:.3g}")
    import _lib
    out = _buf(0)
    assert _lib.lib.ivit_decode_boxes(None, None, None, 0, _lib.ptr(out), _lib.stream()) == 0 and _untouched(out)


def test_eval_post_decode_is_the_same_function():
    """utils.postprocess_batch (ivit_eval_post) decodes with the function ivit_decode_boxes runs:
    with every anchor above the confidence threshold and nothing suppressed, its boxes are
    ivit_decode_boxes' rows in score order, bit for bit. The comparisons of the post-processing
    with utils.decode_box_predictions elsewhere end at this pinned function."""
    import utils
    c = G.decode_case()
    pick = np.nonzero(c["kind"] != "exp_range")[0][:400].reshape(2, 200)
    NA = 200
    anchors = c["table"][c["idx"][pick[0]]]
    rel = np.stack([c["rel"][pick[0]], c["rel"][pick[1]]])
    rng = np.random.RandomState(3)
    logits = np.stack([rng.permutation(NA), rng.permutation(NA)]).astype(np.float32) * 0.02 - 1.0  # distinct scores
    intent = rng.normal(size=(2, NA, 8)).astype(np.float32)
    # an IoU never exceeds 1: nothing is suppressed
    out = utils.postprocess_batch(_dev(logits), _dev(rel), _dev(intent), _dev(anchors), conf_threshold=0.1,
                                  nms_threshold=1.0)
    for b in range(2):
        order = np.argsort(-logits[b], kind="stable")
        want = _decode(rel[b][order], anchors[order], None)
        got = out[b]["pred_boxes_xywha"].cpu().numpy()
        sc = out[b]["pred_scores"].cpu().numpy()
        assert got.shape == (NA, 5) and (np.diff(sc) < 0).all()
        assert np.array_equal(got.view(I32), want.view(I32)), b
        worst, fails = G.judge_decode(got, rel[b][order], anchors[order])
        assert not fails, fails
