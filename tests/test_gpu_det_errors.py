"""Detection error breakdown on the device (ivit_det_errors, metrics.error_analysis) against a
literal restatement in this file: Python loops and numpy f64 over the reference's sequential
matching (eval_vit.py:224-257, as _walk in test_gpu_metrics.py) plus the category, GT status,
error, range-bin and AP-variant definitions, on the same device IoU matrices (the IoU kernels are
pinned separately by tests/golden/geometry.npz)."""
import json
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

THR_FG, THR_BG, EDGES = 0.5, 0.1, (20.0, 40.0, 60.0)
TP, DUP, LOC, BKG = 0, 1, 2, 3
MATCHED, MISSED_NEAR, MISSED_NONE = 0, 1, 2
SIZES = [(50, 10), (255, 25), (256, 1), (257, 40), (700, 40), (2000, 60), (30, 80), (120, 300), (0, 5), (7, 0),
         (0, 0), (1, 1)]


# --------------------------------------------------------------------------------------- inputs
def _scene(seed, P, G):
    """Boxes in metres over the BEV extent; predictions are copies of random GTs cycling through
    tight jitter / loose jitter / clutter / tight jitter with the heading flipped."""
    rng = np.random.default_rng(seed)

    def boxes(n):
        return np.stack([rng.uniform(-20, 60, n), rng.uniform(-72, 72, n), rng.uniform(1.5, 3, n),
                         rng.uniform(3, 9, n), rng.uniform(-math.pi, math.pi, n)], 1)

    gt = boxes(G)
    pred = gt[rng.integers(0, G, P)].copy() if G else boxes(P)
    kind = np.arange(P) % 4
    pred[:, :2] += rng.normal(0, 1, (P, 2)) * np.where(kind == 1, 1.2, 0.15)[:, None]
    clutter = kind == 2
    pred[clutter, 0] = rng.uniform(-20, 60, int(clutter.sum()))
    pred[clutter, 1] = rng.uniform(-72, 72, int(clutter.sum()))
    pred[kind == 3, 4] += math.pi
    pred[:, 2:4] *= rng.uniform(0.9, 1.1, (P, 2))
    pred[:, 4] += rng.normal(0, 0.05, P)
    return {"pred_scores": rng.uniform(0, 1, P).astype(np.float32), "pred_boxes_xywha": pred.astype(np.float32),
            "gt_boxes_xywha": gt.astype(np.float32), "pred_intentions": rng.integers(0, 8, P),
            "gt_intentions": rng.integers(0, 8, G)}


def _inputs():
    res = [_scene(100 + i, P, G) for i, (P, G) in enumerate(SIZES)]
    res[1]["pred_scores"][1::3] = res[1]["pred_scores"][0]      # score ties: the stable order decides
    res[4]["pred_scores"][5::7] = res[4]["pred_scores"][2]
    for i in (0, 3, 5):                                          # a duplicated GT row: IoU ties, first index wins
        res[i]["gt_boxes_xywha"][2] = res[i]["gt_boxes_xywha"][1]
    res[5]["pred_intentions"][::5] = 9                        # intentions outside 0..7 are counted apart
    res[5]["gt_intentions"][3] = -1
    # hand-placed sample: a GT at range exactly 20.0 (upper bin) met by a prediction with the yaw
    # pair (3.1, -3.1); a second GT at 70 m nobody predicts; clutter at 50 m
    res.append({"pred_scores": np.array([0.9, 0.8], np.float32),
                "pred_boxes_xywha": np.array([[12, 16, 2, 4, -3.1], [30, 40, 2, 4, 0]], np.float32),
                "gt_boxes_xywha": np.array([[12, 16, 2, 4, 3.1], [0, 70, 2, 4, 0]], np.float32),
                "pred_intentions": np.array([3, 1]), "gt_intentions": np.array([2, 0])})
    return res


def _cuda(res):
    return [{k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in r.items()} for r in res]


def _ordered(r, rotated):
    """Score order and the device IoU matrix of the ordered predictions, as error_analysis builds them."""
    from utils import compute_axis_aligned_iou, compute_rotated_iou
    order = np.argsort(-r["pred_scores"], kind="stable")
    pb, gb = r["pred_boxes_xywha"][order], r["gt_boxes_xywha"]
    iou = None
    if len(pb) and len(gb):
        p, g = torch.from_numpy(pb).cuda(), torch.from_numpy(gb).cuda()
        iou = (compute_rotated_iou(p, g) if rotated else compute_axis_aligned_iou(p[:, :4], g[:, :4])).cpu().numpy()
    return order, iou, pb, gb, r["pred_intentions"][order], r["gt_intentions"]


# ------------------------------------------------------------------------------------ yardstick
def _ap(tp_kept, gv):
    """The project's AP over the kept predictions (eval_vit.py:209-214, 249-257)."""
    from utils import calculate_ap
    n = len(tp_kept)
    if n == 0:
        return 1.0 if gv == 0 else 0.0
    if gv == 0:
        return 0.0
    cum = np.cumsum(np.asarray(tp_kept, bool).astype(np.float32))
    rec = cum / (gv + 1e-9)
    prec = cum / (np.arange(1, n + 1, dtype=np.float32) + 1e-9)
    return calculate_ap(rec, prec)


def _bin(box, edges):
    x, y = float(box[0]), float(box[1])
    r = math.sqrt(x * x + y * y)
    return sum(r >= float(np.float32(e)) for e in edges)


def _yardstick(iou, pb, gb, pi, gi, thr_fg, thr_bg, edges):
    P, G, nb = len(pb), len(gb), len(edges) + 1
    fg, bg = np.float32(thr_fg), np.float32(thr_bg)
    cat = np.full(P, BKG, np.uint8)
    best = np.full(P, -1, np.int64)
    matched = np.zeros(G, bool)
    for k in range(P):                      # the reference's walk, in score order
        if G == 0:
            continue
        j = int(np.argmax(iou[k]))
        best[k] = j
        if iou[k, j] >= fg:
            if not matched[j]:
                cat[k] = TP
                matched[j] = True
            else:
                cat[k] = DUP
        elif iou[k, j] >= bg:
            cat[k] = LOC
    status = np.zeros(G, np.uint8)
    for g in range(G):
        if not matched[g]:
            near = P > 0 and max(iou[k, g] for k in range(P)) >= bg
            status[g] = MISSED_NEAR if near else MISSED_NONE
    err = np.zeros((P, 4), np.float64)
    tally = np.zeros((nb, 12), np.float64)
    conf = np.zeros((nb, 8, 8), np.int64)
    for k in range(P):
        if cat[k] == TP:
            p, g = pb[k].astype(np.float64), gb[best[k]].astype(np.float64)
            b = _bin(gb[best[k]], edges)
            inter = min(p[2], g[2]) * min(p[3], g[3])
            err[k] = [math.sqrt((p[0] - g[0]) ** 2 + (p[1] - g[1]) ** 2),
                      1.0 - inter / (p[2] * p[3] + g[2] * g[3] - inter),
                      abs(math.remainder(p[4] - g[4], 2 * math.pi)), abs(math.remainder(p[4] - g[4], math.pi))]
            tally[b, 7:11] += err[k]
            if 0 <= gi[best[k]] < 8 and 0 <= pi[k] < 8:
                conf[b, gi[best[k]], pi[k]] += 1
            else:
                tally[b, 11] += 1
        else:
            b = _bin(pb[k], edges)
        tally[b, cat[k]] += 1
    for g in range(G):
        b = _bin(gb[g], edges)
        tally[b, 6] += 1
        if status[g] != MATCHED:
            tally[b, 3 + status[g]] += 1
    # fix_loc: the first LOC prediction of a GT that base leaves unmatched becomes a TP, other LOCs go
    promoted, taken = np.zeros(P, bool), set()
    for k in range(P):
        if cat[k] == LOC and not matched[best[k]] and best[k] not in taken:
            promoted[k] = True
            taken.add(best[k])
    tp = cat == TP
    ap = [_ap(tp, G),
          _ap(tp[cat != DUP], G),
          _ap(tp[cat != BKG], G),
          _ap((tp | promoted)[(cat != LOC) | promoted], G),
          _ap(tp, int(matched.sum()))]
    return {"cat": cat, "best": best, "status": status, "err": err, "tally": tally, "conf": conf,
            "ap": np.asarray(ap), "promoted": promoted}


def _check(report, res, rotated, thr_fg=THR_FG, thr_bg=THR_BG, edges=EDGES):
    """Every output of the device run against the yardstick; -> the yardstick's summed tallies."""
    total = np.zeros((len(edges) + 1, 12))
    for i, r in enumerate(res):
        order, iou, pb, gb, pi, gi = _ordered(r, rotated)
        y = _yardstick(iou, pb, gb, pi, gi, thr_fg, thr_bg, edges)
        d = report["per_sample"][i]
        assert np.array_equal(d["order"].cpu().numpy(), order), i
        assert np.array_equal(d["category"].cpu().numpy(), y["cat"]), i
        assert np.array_equal(d["gt_status"].cpu().numpy(), y["status"]), i
        assert np.array_equal(d["best_gt"].cpu().numpy(), y["best"]), i
        got = report["tallies_per_sample"][i]
        assert np.array_equal(got[:, :7], y["tally"][:, :7]) and np.array_equal(got[:, 11], y["tally"][:, 11]), i
        assert np.array_equal(report["confusion_per_sample"][i], y["conf"]), i
        e = d["errors"].cpu().numpy()
        assert e.shape == y["err"].shape and (np.abs(e - y["err"]).max() if e.size else 0.0) <= 1e-9, i
        assert np.abs(got[:, 7:11] - y["tally"][:, 7:11]).max() <= 1e-9, i
        print(f"sample {i}: P={len(pb)} G={len(gb)} ap dev {report['ap_per_sample'][i]} yardstick {y['ap']}")
        assert np.abs(report["ap_per_sample"][i] - y["ap"]).max() <= 1e-12, (i, report["ap_per_sample"][i], y["ap"])
        total += y["tally"]
    return total


@pytest.fixture(scope="module")
def run():
    import metrics
    res = _inputs()
    return res, metrics.error_analysis(_cuda(res), THR_FG, THR_BG, False, EDGES)


# ---------------------------------------------------------------------------------------- tests
def test_det_errors_equal_yardstick(run):
    res, report = run
    total = _check(report, res, rotated=False)
    # the inputs reach every category in at least two range bins (else they, not the kernel, are at fault)
    for c, name in enumerate(("tp", "dup", "loc", "bkg", "missed_near", "missed_none")):
        assert (total[:, c] > 0).sum() >= 2, (name, total[:, c])
    assert total[:, 11].sum() > 0  # and the out-of-range intentions
    # the aggregate report is the sum over samples
    for b, blk in enumerate(report["bins"]):
        assert [blk[k] for k in ("tp", "dup", "loc", "bkg", "missed_near", "missed_none", "gt")] == \
            total[b, :7].astype(int).tolist()
    t = report["total"]
    assert t["predictions"] == sum(P for P, _ in SIZES) + 2 == t["tp"] + t["dup"] + t["loc"] + t["bkg"]
    assert t["gt"] == sum(G for _, G in SIZES) + 2 == t["tp"] + t["missed_near"] + t["missed_none"]
    assert t["ate"] == pytest.approx(total[:, 7].sum() / total[:, 0].sum(), abs=1e-9)
    assert report["map"]["base"] == pytest.approx(float(np.mean(report["ap_per_sample"][:, 0])), abs=1e-15)
    assert report["dAP"]["no_bkg"] == report["map"]["no_bkg"] - report["map"]["base"]


def test_hand_placed_sample(run):
    res, report = run
    i = len(res) - 1
    d = report["per_sample"][i]
    assert d["category"].cpu().tolist() == [TP, BKG] and d["gt_status"].cpu().tolist() == [MATCHED, MISSED_NONE]
    t = report["tallies_per_sample"][i]
    # the GT at (12, 16) is at range 20.0 exactly: bin 1 (20 <= r < 40), with its TP; clutter at 50 m, GT at 70 m
    assert t[:, 6].tolist() == [0, 1, 0, 1] and t[:, 0].tolist() == [0, 1, 0, 0]
    assert t[:, 3].tolist() == [0, 0, 1, 0] and t[:, 5].tolist() == [0, 0, 0, 1]
    e = d["errors"].cpu().numpy()
    assert e[0, 2] == pytest.approx(2 * math.pi - 6.2, abs=1e-6) and 0.08 < e[0, 2] < 0.09  # not 6.2
    assert e[0, 3] == pytest.approx(2 * math.pi - 6.2, abs=1e-6)
    assert e[0, 0] == 0.0 and e[0, 1] == 0.0 and not e[1].any()
    assert report["confusion_per_sample"][i][1, 2, 3] == 1 and report["confusion_per_sample"][i].sum() == 1


def test_thresholds_met_exactly():
    """A best IoU equal to thr_fg (f32) qualifies, equal to thr_bg is a localisation error; one
    f32 step below each is the category underneath. IoU matrices written by hand."""
    import metrics
    fg, bg = np.float32(THR_FG), np.float32(THR_BG)
    below = lambda v: np.nextafter(v, np.float32(0))  # noqa: E731
    iou = np.zeros((6, 3), np.float32)
    iou[0, 0] = fg          # TP of GT 0
    iou[1, 0] = fg          # DUP
    iou[2, 1] = below(fg)   # LOC, promoted by fix_loc (GT 1 unmatched)
    iou[3, 1] = bg          # LOC, dropped by fix_loc
    iou[4, 2] = below(bg)   # BKG; GT 2 has no prediction at thr_bg
    iou[5, 1] = 0.3         # LOC
    rng = np.random.default_rng(0)
    pb = np.concatenate([rng.uniform(5, 70, (6, 2)), np.full((6, 2), 2.0), np.zeros((6, 1))], 1).astype(np.float32)
    gb = np.concatenate([rng.uniform(5, 70, (3, 2)), np.full((3, 2), 2.0), np.zeros((3, 1))], 1).astype(np.float32)
    pi, gi = np.arange(6) % 8, np.arange(3) % 8
    c = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    report = metrics.det_errors_device([c(iou)], [c(pb)], [c(gb)], [c(pi)], [c(gi)], THR_FG, THR_BG, EDGES)
    d = report["per_sample"][0]
    assert d["category"].cpu().tolist() == [TP, DUP, LOC, LOC, BKG, LOC]
    assert d["gt_status"].cpu().tolist() == [MATCHED, MISSED_NEAR, MISSED_NONE]
    y = _yardstick(iou, pb, gb, pi, gi, THR_FG, THR_BG, EDGES)
    assert y["cat"].tolist() == [TP, DUP, LOC, LOC, BKG, LOC] and y["promoted"].tolist() == [0, 0, 1, 0, 0, 0]
    assert np.array_equal(report["tallies_per_sample"][0][:, :7], y["tally"][:, :7])
    assert np.abs(report["ap_per_sample"][0] - y["ap"]).max() <= 1e-12
    # base: TP FP FP FP FP FP over 3 GTs = 1/3; fix_loc keeps TP, DUP, promoted LOC, BKG: 1/3 + 1/3 * 2/3
    assert report["ap_per_sample"][0][0] == pytest.approx(1 / 3, abs=1e-7)
    assert report["ap_per_sample"][0][3] == pytest.approx(1 / 3 + 2 / 9, abs=1e-7)
    assert report["ap_per_sample"][0][4] == pytest.approx(1.0, abs=1e-7)


def test_base_agrees_with_match_device(run):
    import metrics
    res, report = run
    ap, per = metrics.match_device(_cuda(res), [THR_FG])
    for i in range(len(res)):
        assert report["ap_per_sample"][i, 0] == pytest.approx(ap[i, 0], abs=1e-12), i
        assert torch.equal(per[i][0], report["per_sample"][i]["order"])
        if per[i][1].shape[1] and len(res[i]["gt_boxes_xywha"]):
            assert torch.equal(per[i][1][0], report["per_sample"][i]["category"] == TP), i
            assert torch.equal(per[i][2], report["per_sample"][i]["best_gt"]), i


def test_removing_an_error_type_never_lowers_ap(run):
    _, report = run
    ap = report["ap_per_sample"]
    for v in (1, 2, 4):  # no_dup, no_bkg, no_miss; fix_loc carries no such bound
        assert (ap[:, v] >= ap[:, 0] - 1e-12).all(), (v, ap[:, v] - ap[:, 0])


def test_two_runs_give_identical_bytes(run):
    import metrics
    res, a = run
    b = metrics.error_analysis(_cuda(res), THR_FG, THR_BG, False, EDGES)
    for k in ("tallies_per_sample", "confusion_per_sample", "ap_per_sample"):
        assert a[k].tobytes() == b[k].tobytes(), k
    for da, db in zip(a["per_sample"], b["per_sample"]):
        for k in ("category", "errors", "gt_status", "best_gt", "order"):
            assert da[k].cpu().numpy().tobytes() == db[k].cpu().numpy().tobytes(), k


def test_rotated_iou_run_equals_yardstick():
    import metrics
    res = _inputs()
    report = metrics.error_analysis(_cuda(res), THR_FG, THR_BG, True, EDGES)
    assert report["settings"]["rotated"] is True
    total = _check(report, res, rotated=True)
    assert total[:, 0].sum() > 0 and total[:, 2].sum() > 0
    # the heading-flipped copies are TPs under rotated IoU too, and cost pi of orientation error each
    e = torch.cat([d["errors"] for d in report["per_sample"]]).cpu().numpy()
    assert (e[:, 2] > 3.0).sum() > 10
    assert e[:, 2].max() <= math.pi and e[:, 3].max() <= math.pi / 2 and e.min() >= 0.0


def test_too_many_gt_boxes_raise():
    import metrics
    r = _scene(1, 3, 4097)
    with pytest.raises(ValueError, match="4096 GT boxes"):
        metrics.error_analysis(_cuda([r]))


ARGV = ["--synthetic", "--grid", "64x64", "--batch", "2", "--batches", "2"]


def test_eval_vit_error_report(tmp_path, monkeypatch, capsys):
    import eval_vit
    monkeypatch.chdir(tmp_path)
    out = tmp_path / "errors.json"
    torch.manual_seed(0)  # the random-init weights of the run
    assert eval_vit.main_eval_vit(ARGV + ["--error-report", str(out)]) == 0
    printed = capsys.readouterr().out
    assert "Detection Error Breakdown" in printed and "range [m]" in printed
    assert printed.index("Detection Error Breakdown") > printed.index("Detection Results (mAP)")
    rep = json.loads(out.read_text())
    t = rep["total"]
    assert t["predictions"] == t["tp"] + t["dup"] + t["loc"] + t["bkg"] and t["predictions"] > 0
    assert t["gt"] == t["tp"] + t["missed_near"] + t["missed_none"] and t["gt"] > 0
    assert sum(b["gt"] for b in rep["bins"]) == t["gt"] and len(rep["bins"]) == 4
    assert rep["settings"] == {"iou_thr": 0.5, "bg_thr": 0.1, "rotated": False, "range_edges": [20.0, 40.0, 60.0],
                               "n_samples": 4}
    assert set(rep["map"]) == {"base", "no_dup", "no_bkg", "fix_loc", "no_miss"}
    assert "per_sample" not in rep


def test_eval_vit_without_the_flag_prints_no_table(tmp_path, monkeypatch, capsys):
    import eval_vit
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    assert eval_vit.main_eval_vit(ARGV) == 0
    printed = capsys.readouterr().out
    assert "Error Breakdown" not in printed and "range [m]" not in printed and "Error report" not in printed
    assert "Detection Results (mAP)" in printed and not list(tmp_path.glob("*.json"))
