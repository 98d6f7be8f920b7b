"""Detection error breakdown, host side (no GPU): argument validation of ivit_det_errors before
any device call, the derived numbers / table / JSON of metrics.report_from_tallies on a
hand-written tally, and the eval_vit flags."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

import _lib
import metrics
from conftest import REPO

LIB = os.path.join(REPO, "visiontransformer-intention-prediction_amd", "libivit_hip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libivit_hip.so not built (run __graft_entry__.build())")


def _call(max_gt=10, edges=(20.0, 40.0, 60.0), thr_fg=0.5, thr_bg=0.1, work_bytes=1 << 20):
    dll = _lib.lib.load()
    e = (ctypes.c_float * max(len(edges), 1))(*edges)
    # one sample, ten predictions; every pointer but the host-side edges is null: a check must
    # refuse the call before anything is dereferenced or launched
    rc = dll.ivit_det_errors(None, None, None, None, None, None, 1, 10, None, None, None, None, thr_fg, thr_bg, e,
                             len(edges), None, None, None, None, None, None, None, None, work_bytes, max_gt, None)
    return rc, dll.ivit_last_error().decode()


@needs_lib
@pytest.mark.parametrize("kw,word", [
    (dict(max_gt=4097), "4096 GT"),
    (dict(edges=tuple(float(i) for i in range(1, 9))), "range bins"),   # 8 edges = 9 bins
    (dict(edges=(20.0, 60.0, 40.0)), "ascending"),
    (dict(edges=(20.0, 20.0)), "ascending"),
    (dict(thr_fg=0.5, thr_bg=0.5), "thr_bg < thr_fg"),
    (dict(thr_fg=0.3, thr_bg=0.4), "thr_bg < thr_fg"),
    (dict(thr_fg=0.5, thr_bg=-0.1), "thr_bg < thr_fg"),
    (dict(work_bytes=16), "workspace"),
])
def test_argument_validation_without_device(kw, word):
    rc, msg = _call(**kw)
    assert rc < 0
    assert "ivit_det_errors" in msg and word in msg, msg


@needs_lib
def test_workspace_query_is_pure_host():
    dll = _lib.lib.load()
    # prec f32 + cum i32 per (variant, prediction), one matched count per sample, one byte per prediction
    assert dll.ivit_det_errors_workspace(3, 1000) == 5 * 8 * 1000 + 4 * 3 + 1000
    assert dll.ivit_det_errors_workspace(0, 0) > 0
    with pytest.raises(RuntimeError, match="ivit_det_errors failed"):
        _lib.lib.ivit_det_errors(None, None, None, None, None, None, 1, 10, None, None, None, None, 0.5, 0.1, None,
                                 0, None, None, None, None, None, None, None, None, 0, 5000, None)


# ------------------------------------------------------------------ a hand-written tally, 2 bins
def _hand():
    # columns: tp dup loc bkg missed_near missed_none gt ate ase aoe aoe_pi intent_skipped
    tallies = np.array([[6, 2, 1, 3, 1, 1, 8, 1.5, 0.6, 0.9, 0.3, 0],
                        [0, 0, 2, 5, 0, 3, 3, 0.0, 0.0, 0.0, 0.0, 0]], np.float64)
    conf = np.zeros((2, 8, 8), np.int64)
    conf[0, 0, 0] = 2
    conf[0, 0, 1] = 1
    conf[0, 1, 1] = 1
    conf[0, 3, 1] = 1
    conf[0, 5, 5] = 1
    ap = np.array([[0.5, 0.6, 0.7, 0.55, 0.9], [0.25, 0.25, 0.5, 0.2, 1.0]])
    settings = {"iou_thr": 0.5, "bg_thr": 0.1, "rotated": False, "range_edges": [30.0], "n_samples": 2}
    return tallies, conf, ap, settings


def test_report_derived_numbers():
    tallies, conf, ap, settings = _hand()
    r = metrics.report_from_tallies(tallies, conf, ap, settings)
    b0, b1, tot = r["bins"][0], r["bins"][1], r["total"]
    assert b0["range"] == [0.0, 30.0] and b1["range"] == [30.0, math.inf]
    assert (b0["tp"], b0["dup"], b0["loc"], b0["bkg"], b0["missed_near"], b0["missed_none"], b0["gt"]) == \
        (6, 2, 1, 3, 1, 1, 8)
    assert b0["predictions"] == 12 and b1["predictions"] == 7 and tot["predictions"] == 19
    assert b0["recall"] == 6 / 8 and b0["precision"] == 6 / 12
    assert b0["ate"] == 1.5 / 6 and b0["ase"] == 0.6 / 6 and b0["aoe"] == 0.9 / 6 and b0["aoe_pi"] == 0.3 / 6
    # a bin without TPs: recall and precision are 0, the mean errors do not exist
    assert b1["recall"] == 0.0 and b1["precision"] == 0.0
    assert all(math.isnan(b1[k]) for k in ("ate", "ase", "aoe", "aoe_pi"))
    assert tot["gt"] == 11 and tot["tp"] == 6 and tot["recall"] == 6 / 11 and tot["ate"] == 1.5 / 6
    assert tot["gt"] == tot["tp"] + tot["missed_near"] + tot["missed_none"]
    assert r["map"]["base"] == pytest.approx(0.375, abs=1e-15)
    assert r["map"]["no_miss"] == pytest.approx(0.95, abs=1e-15)
    for v in ("no_dup", "no_bkg", "fix_loc", "no_miss"):
        assert r["dAP"][v] == r["map"][v] - r["map"]["base"]
    assert r["dAP"]["fix_loc"] == pytest.approx(0.0, abs=1e-15)
    assert np.array_equal(np.asarray(tot["confusion"]), conf.sum(axis=0))


def test_intention_scores_agree_with_sklearn():
    from sklearn.metrics import accuracy_score, f1_score
    rng = np.random.default_rng(3)
    conf = rng.integers(0, 6, size=(2, 8, 8))
    conf[:, 6, :] = 0   # a class that never occurs as GT
    conf[:, :, 2] = 0   # a class that is never predicted
    conf[:, 7, :] = 0
    conf[:, :, 7] = 0   # and one that never occurs at all (zero_division)
    tallies, _, ap, settings = _hand()
    r = metrics.report_from_tallies(tallies, conf, ap, settings)
    total = conf.sum(axis=0)
    yt = [g for g in range(8) for p in range(8) for _ in range(total[g, p])]
    yp = [p for g in range(8) for p in range(8) for _ in range(total[g, p])]
    labels = list(range(8))
    it = r["intention"]
    assert it["accuracy"] == pytest.approx(accuracy_score(yt, yp), abs=1e-12)
    assert it["f1_macro"] == pytest.approx(f1_score(yt, yp, labels=labels, average="macro", zero_division=0), abs=1e-12)
    assert it["f1_weighted"] == pytest.approx(f1_score(yt, yp, labels=labels, average="weighted", zero_division=0),
                                              abs=1e-12)
    np.testing.assert_allclose(it["f1_per_class"], f1_score(yt, yp, labels=labels, average=None, zero_division=0),
                               atol=1e-12, rtol=0)
    # no TP at all: nothing to score
    empty = metrics.report_from_tallies(tallies * 0, conf * 0, ap, settings)["intention"]
    assert math.isnan(empty["accuracy"]) and math.isnan(empty["f1_macro"]) and math.isnan(empty["f1_weighted"])
    assert empty["f1_per_class"] == [0.0] * 8


def test_format_error_report_table():
    tallies, conf, ap, settings = _hand()
    r = metrics.report_from_tallies(tallies, conf, ap, settings)
    txt = metrics.format_error_report(r)
    lines = txt.splitlines()
    assert "IoU>=0.5" in lines[0] and "axis-aligned" in lines[0] and "2 samples" in lines[0]
    head = lines[1].split()
    assert head[:2] == ["range", "[m]"] and head[2:] == ["GT", "TP", "DUP", "LOC", "BKG", "near", "none", "recall",
                                                          "prec", "ATE", "ASE", "AOE", "AOE_pi"]
    assert lines[2].split() == ["0-30", "8", "6", "2", "1", "3", "1", "1", "0.750", "0.500", "0.250", "0.100",
                                "0.150", "0.050"]
    assert lines[3].split() == ["30+", "3", "0", "0", "2", "5", "0", "3", "0.000", "0.000", "-", "-", "-", "-"]
    assert lines[4].split()[:3] == ["all", "11", "6"]
    assert len({len(ln) for ln in lines[1:5]}) == 1  # aligned columns
    assert "nan" not in txt
    assert "mAP 0.3750" in txt and "no_miss 0.9500 (+0.5750)" in txt and "fix_loc 0.3750 (+0.0000)" in txt
    assert "accuracy 0.6667" in txt


def test_error_report_json_round_trip():
    tallies, conf, ap, settings = _hand()
    r = metrics.report_from_tallies(tallies, conf, ap, settings)
    r["per_sample"] = [object()]  # whatever the device path adds stays out of the file
    r["ap_per_sample"] = ap
    back = json.loads(metrics.error_report_json(r))
    assert set(back) == {"settings", "bins", "total", "intention", "map", "dAP"}
    assert "NaN" not in metrics.error_report_json(r) and "Infinity" not in metrics.error_report_json(r)
    assert back["bins"][1]["ate"] is None and back["bins"][1]["range"] == [30.0, None]
    assert back["bins"][0]["ate"] == 0.25 and back["bins"][0]["tp"] == 6
    assert back["total"]["confusion"] == conf.sum(axis=0).tolist()
    assert back["settings"] == {"iou_thr": 0.5, "bg_thr": 0.1, "rotated": False, "range_edges": [30.0],
                                "n_samples": 2}
    assert back["map"]["base"] == r["map"]["base"] and back["dAP"]["no_bkg"] == r["dAP"]["no_bkg"]


def test_eval_flags():
    import eval_vit
    a = eval_vit.parse_args([])
    assert a.error_report is None and a.error_iou == 0.5 and a.error_bg_iou == 0.1
    assert a.error_range_edges == "20,40,60"
    # the old flags keep their defaults
    assert (a.synthetic, a.batch, a.batches, a.dtype, a.rotated, a.rotated_nms, a.attn_maps, a.attn_top,
            a.attn_blocks, a.checkpoint) == (False, 8, 4, "fp32", False, False, None, 8, "-1", None)
    b = eval_vit.parse_args(["--error-report", "out.json", "--error-iou", "0.7", "--error-bg-iou", "0.2",
                             "--error-range-edges", "10,30", "--rotated"])
    assert (b.error_report, b.error_iou, b.error_bg_iou, b.error_range_edges, b.rotated) == \
        ("out.json", 0.7, 0.2, "10,30", True)
    assert b.rotated_nms is False and b.batch == 8
