"""Detection mAP and intention-matching metrics of eval_vit.py:191-311 (host side).

The reference walks the score-sorted predictions one by one: a prediction is a true positive
when the IoU with its best GT (``torch.max`` over the row, first index on ties) reaches the
threshold and that GT is not matched yet. The best GT of a prediction does not depend on the
matching state, so the walk is exactly "the first qualifying prediction of each GT, in sorted
order" — computed here with one ``np.unique(return_index=True)`` per threshold instead of a
Python loop over up to 22 500 predictions.
"""
from __future__ import annotations

import numpy as np
import torch

from constants import DETECTION_IOU_THRESHOLDS, IOU_THRESHOLD_FOR_INTENTION_MATCH
from utils import calculate_ap, compute_axis_aligned_iou, compute_rotated_iou


def _iou(pred, gt, rotated):
    """(P,5) x (G,5) → (P,G) numpy f32; device kernels (utils.py:276-392 semantics)."""
    dev = torch.device("cuda")
    p = pred.to(dev).float()
    g = gt.to(dev).float()
    if rotated:
        return compute_rotated_iou(p, g).cpu().numpy()
    return compute_axis_aligned_iou(p[:, :4], g[:, :4]).cpu().numpy()


def _first_match(iou_sorted: np.ndarray, thr: float) -> np.ndarray:
    """TP flags of the sequential greedy matching (eval_vit.py:236-247) in sorted order."""
    best = iou_sorted.max(axis=1)
    arg = iou_sorted.argmax(axis=1)
    q = np.nonzero(best >= thr)[0]
    tp = np.zeros(iou_sorted.shape[0], dtype=bool)
    if q.size:
        _, first = np.unique(arg[q], return_index=True)
        tp[q[first]] = True
    return tp


def _stable_desc(scores: np.ndarray) -> np.ndarray:
    # torch.argsort(descending=True) on CPU is not guaranteed stable; a stable order is used
    # here (ties are measure-zero for sigmoid scores of distinct anchors).
    return np.argsort(-scores, kind="stable")


def detection_map(results, thresholds=DETECTION_IOU_THRESHOLDS, rotated=False):
    """results: list of dicts with pred_scores, pred_boxes_xywha, gt_boxes_xywha → {thr: mAP}."""
    aps = {t: [] for t in thresholds}
    for r in results:
        ps = np.asarray(r["pred_scores"].cpu(), dtype=np.float32)
        npred, ngt = ps.shape[0], r["gt_boxes_xywha"].shape[0]
        iou = None
        for t in thresholds:
            if npred == 0:
                aps[t].append(1.0 if ngt == 0 else 0.0)
                continue
            if ngt == 0:
                aps[t].append(0.0)
                continue
            if iou is None:
                order = _stable_desc(ps)
                iou = _iou(r["pred_boxes_xywha"][torch.from_numpy(order)], r["gt_boxes_xywha"], rotated)
            tp = _first_match(iou, t)
            cum = np.cumsum(tp.astype(np.float32))
            recall = cum / (ngt + 1e-9)
            precision = cum / (np.arange(1, npred + 1, dtype=np.float32) + 1e-9)
            aps[t].append(calculate_ap(recall, precision))
    return {t: (float(np.mean(v)) if v else 0.0) for t, v in aps.items()}


def intention_matches(results, thr=IOU_THRESHOLD_FOR_INTENTION_MATCH, rotated=False):
    """Matched (pred_intent, gt_intent) pairs of eval_vit.py:268-292."""
    mp, mg = [], []
    for r in results:
        npred, ngt = r["pred_boxes_xywha"].shape[0], r["gt_boxes_xywha"].shape[0]
        if npred == 0 or ngt == 0:
            continue
        ps = np.asarray(r["pred_scores"].cpu(), dtype=np.float32)
        order = _stable_desc(ps)
        iou = _iou(r["pred_boxes_xywha"], r["gt_boxes_xywha"], rotated)[order]
        tp = _first_match(iou, thr)
        gt_idx = iou.argmax(axis=1)
        pi = np.asarray(r["pred_intentions"].cpu())[order]
        gi = np.asarray(r["gt_intentions"].cpu())
        for k in np.nonzero(tp)[0]:
            mp.append(int(pi[k]))
            mg.append(int(gi[gt_idx[k]]))
    return mp, mg


# ---------------------------------------------------------------------------- device path (§8f-2)
def match_device(results, thresholds, rotated=False):
    """All samples' greedy matching + VOC AP in one launch (ivit_det_match).

    results: dicts with pred_scores / pred_boxes_xywha / gt_boxes_xywha (device tensors; the
    predictions are re-ordered by a stable descending score sort — postprocess_batch already
    emits them in that order). Returns (ap [S, T] float64 numpy, per-sample (order, tp [T, P]
    bool, best_gt [P]) on the device)."""
    from _lib import lib, ptr, stream, workspace
    dev = torch.device("cuda")
    S, T = len(results), len(thresholds)
    ious, npred, ngt, orders = [], [], [], []
    for r in results:
        ps = r["pred_scores"].to(dev)
        P, G = int(ps.shape[0]), int(r["gt_boxes_xywha"].shape[0])
        order = torch.sort(ps, descending=True, stable=True).indices if P else torch.zeros(0, dtype=torch.long,
                                                                                           device=dev)
        if P and G:
            pb = r["pred_boxes_xywha"].to(dev).float()[order]
            gb = r["gt_boxes_xywha"].to(dev).float()
            m = compute_rotated_iou(pb, gb) if rotated else compute_axis_aligned_iou(pb[:, :4], gb[:, :4])
            ious.append(m.reshape(-1))
        npred.append(P)
        ngt.append(G)
        orders.append(order)
    if max(ngt, default=0) > 4096:
        raise ValueError("device matching supports at most 4096 GT boxes per sample")
    iou = torch.cat(ious) if ious else torch.zeros(1, device=dev)
    sizes = [p * g if p and g else 0 for p, g in zip(npred, ngt)]
    iou_off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64) if S else np.zeros(0, np.int64)
    pred_off = np.concatenate([[0], np.cumsum(npred)[:-1]]).astype(np.int64) if S else np.zeros(0, np.int64)
    tot = int(sum(npred))
    h2d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_iou_off, d_pred_off = h2d(iou_off), h2d(pred_off)
    d_np, d_ng = h2d(np.asarray(npred, np.int32)), h2d(np.asarray(ngt, np.int32))
    d_thr = h2d(np.asarray(thresholds, np.float32))
    ap = torch.empty((S, T), dtype=torch.float64, device=dev)
    best = torch.empty(max(tot, 1), dtype=torch.int32, device=dev)
    tp = torch.empty((T, max(tot, 1)), dtype=torch.uint8, device=dev)
    ws = workspace(8 * T * max(tot, 1), dev)
    lib.ivit_det_match(ptr(iou), ptr(d_iou_off), ptr(d_np), ptr(d_ng), ptr(d_pred_off), S, tot, ptr(d_thr), T,
                       ptr(ap), ptr(best), ptr(tp), ptr(ws), ws.numel(), max(ngt, default=0), stream())
    per = [(orders[i], tp[:, pred_off[i]:pred_off[i] + npred[i]].bool(), best[pred_off[i]:pred_off[i] + npred[i]])
           for i in range(S)]
    return ap.cpu().numpy(), per


def detection_map_device(results, thresholds=DETECTION_IOU_THRESHOLDS, rotated=False):
    """detection_map (eval_vit.py:191-262) with the matching and AP on the device."""
    if not results:
        return {t: 0.0 for t in thresholds}
    ap, _ = match_device(results, thresholds, rotated)
    return {t: float(np.mean(ap[:, i])) for i, t in enumerate(thresholds)}


def intention_matches_device(results, thr=IOU_THRESHOLD_FOR_INTENTION_MATCH, rotated=False):
    """intention_matches (eval_vit.py:268-292): the TPs at `thr` with their best GT, on the device."""
    if not results:
        return [], []
    _, per = match_device(results, [thr], rotated)
    mp, mg = [], []
    for r, (order, tp, best) in zip(results, per):
        if order.numel() == 0 or r["gt_boxes_xywha"].shape[0] == 0:
            continue
        k = torch.nonzero(tp[0]).flatten()
        pi = r["pred_intentions"].to(order.device)[order][k]
        gi = r["gt_intentions"].to(order.device)[best[k].long()]
        mp.extend(pi.cpu().tolist())
        mg.extend(gi.cpu().tolist())
    return mp, mg


# ------------------------------------------------------------- error breakdown (ivit_det_errors)
ERROR_CATEGORIES = ("tp", "dup", "loc", "bkg")                  # category byte 0..3
GT_STATUSES = ("matched", "missed_near", "missed_none")         # GT status byte 0..2
AP_VARIANTS = ("base", "no_dup", "no_bkg", "fix_loc", "no_miss")
TALLY_COLUMNS = ("tp", "dup", "loc", "bkg", "missed_near", "missed_none", "gt",
                 "ate_sum", "ase_sum", "aoe_sum", "aoe_pi_sum", "intent_skipped")
_N_INTENT = 8  # the confusion matrix of ivit_det_errors is 8 x 8


def _ratio(a, b):
    return float(a) / float(b) if b else float("nan")


def _f1_from_confusion(conf):
    """accuracy and per-class / macro / weighted F1 of a [GT, predicted] confusion matrix, as
    sklearn's accuracy_score / f1_score(labels=all classes, zero_division=0) give them."""
    conf = np.asarray(conf, dtype=np.float64)
    n = conf.sum()
    tp = np.diag(conf)
    den = conf.sum(axis=0) + conf.sum(axis=1)  # 2 TP + FP + FN
    f1 = np.divide(2.0 * tp, den, out=np.zeros_like(tp), where=den > 0)
    support = conf.sum(axis=1)
    return {"accuracy": _ratio(tp.sum(), n), "f1_per_class": [float(v) for v in f1],
            "f1_macro": float(f1.mean()) if n else float("nan"),
            "f1_weighted": float((f1 * support).sum() / n) if n else float("nan")}


def _tally_block(row, conf):
    c = {k: int(round(row[i])) for i, k in enumerate(TALLY_COLUMNS[:7])}
    npred = c["tp"] + c["dup"] + c["loc"] + c["bkg"]
    out = dict(c)
    out["predictions"] = npred
    out["recall"] = _ratio(c["tp"], c["gt"])
    out["precision"] = _ratio(c["tp"], npred)
    for i, k in enumerate(("ate", "ase", "aoe", "aoe_pi")):
        out[k] = _ratio(row[7 + i], c["tp"])
    out["intent_skipped"] = int(round(row[11]))
    out["confusion"] = np.asarray(conf, dtype=np.int64).tolist()
    return out


def report_from_tallies(tallies, confusion, ap, settings):
    """The aggregate report of error_analysis from the tallies summed over samples: tallies
    [bins, 12] f64 (TALLY_COLUMNS), confusion [bins, 8, 8], ap [S, 5] (AP_VARIANTS)."""
    tallies = np.asarray(tallies, dtype=np.float64)
    confusion = np.asarray(confusion, dtype=np.int64)
    ap = np.asarray(ap, dtype=np.float64).reshape(-1, len(AP_VARIANTS))
    edges = [float(e) for e in settings["range_edges"]]
    lo, hi = [0.0] + edges, edges + [float("inf")]
    bins = []
    for b in range(tallies.shape[0]):
        blk = _tally_block(tallies[b], confusion[b])
        blk["range"] = [lo[b], hi[b]]
        bins.append(blk)
    total_conf = confusion.sum(axis=0)
    maps = {v: (float(np.mean(ap[:, i])) if ap.shape[0] else 0.0) for i, v in enumerate(AP_VARIANTS)}
    return {"settings": dict(settings, range_edges=edges),
            "bins": bins,
            "total": _tally_block(tallies.sum(axis=0), total_conf),
            "intention": _f1_from_confusion(total_conf),
            "map": maps,
            "dAP": {v: maps[v] - maps["base"] for v in AP_VARIANTS[1:]}}


def error_analysis(results, iou_thr=IOU_THRESHOLD_FOR_INTENTION_MATCH, bg_thr=0.1, rotated=False,
                   range_edges=(20.0, 40.0, 60.0)):
    """Why detections and GTs did not count at ``iou_thr`` (ivit_det_errors; one launch and one
    host read of the tallies for all samples). results: the dicts match_device takes, with
    pred_intentions / gt_intentions. Every prediction is a TP, a duplicate (DUP), mislocalised
    (LOC: bg_thr <= best IoU < iou_thr) or background (BKG); every GT is matched, missed with a
    prediction nearby or missed with none; all of it per range bin (metres from the ego vehicle),
    with the TP translation / scale / orientation errors, the intention confusion matrix and the
    mAP each error type costs (report_from_tallies). ``"per_sample"``: device tensors per sample —
    order, category [P] u8, errors [P, 4] f64, best_gt [P], gt_status [G] u8."""
    dev = torch.device("cuda")
    ious, orders, pbs, gbs, pis, gis = [], [], [], [], [], []
    for r in results:
        ps = r["pred_scores"].to(dev)
        P, G = int(ps.shape[0]), int(r["gt_boxes_xywha"].shape[0])
        order = torch.sort(ps, descending=True, stable=True).indices if P else torch.zeros(0, dtype=torch.long,
                                                                                           device=dev)
        pb = r["pred_boxes_xywha"].to(dev).float().reshape(-1, 5)[order]
        gb = r["gt_boxes_xywha"].to(dev).float().reshape(-1, 5)
        if G > 4096:
            raise ValueError("device matching supports at most 4096 GT boxes per sample")
        m = None
        if P and G:
            m = compute_rotated_iou(pb, gb) if rotated else compute_axis_aligned_iou(pb[:, :4], gb[:, :4])
        ious.append(m)
        orders.append(order)
        pbs.append(pb)
        gbs.append(gb)
        pis.append(r["pred_intentions"].to(dev).reshape(-1)[order])
        gis.append(r["gt_intentions"].to(dev).reshape(-1))
    report = det_errors_device(ious, pbs, gbs, pis, gis, iou_thr, bg_thr, range_edges, rotated)
    for d, order in zip(report["per_sample"], orders):
        d["order"] = order
    return report


def det_errors_device(ious, pred_boxes, gt_boxes, pred_int, gt_int, iou_thr, bg_thr, range_edges, rotated=False):
    """The launch behind error_analysis on prepared per-sample device inputs, predictions in score
    order: ious[i] [P_i, G_i] f32 (ignored when either is 0), boxes [., 5], integer intentions."""
    from _lib import lib, ptr, stream, workspace
    dev = torch.device("cuda")
    S = len(pred_boxes)
    edges = [float(e) for e in range_edges]
    nb = len(edges) + 1
    settings = {"iou_thr": float(iou_thr), "bg_thr": float(bg_thr), "rotated": bool(rotated),
                "range_edges": edges, "n_samples": S}
    pbs = [b.to(dev).float().reshape(-1, 5) for b in pred_boxes]
    gbs = [b.to(dev).float().reshape(-1, 5) for b in gt_boxes]
    pis = [t.to(dev).reshape(-1).to(torch.int32) for t in pred_int]
    gis = [t.to(dev).reshape(-1).to(torch.int32) for t in gt_int]
    npred, ngt = [int(b.shape[0]) for b in pbs], [int(b.shape[0]) for b in gbs]
    if max(ngt, default=0) > 4096:
        raise ValueError("device matching supports at most 4096 GT boxes per sample")
    for m, p, g in zip(ious, npred, ngt):
        if p and g and tuple(m.shape) != (p, g):
            raise ValueError(f"IoU matrix {tuple(m.shape)} for {p} predictions and {g} GT boxes")
    ious = [m.to(dev).float().reshape(-1) for m, p, g in zip(ious, npred, ngt) if p and g]
    pad = lambda ts, shape, dtype: (torch.cat(ts) if ts and sum(t.shape[0] for t in ts)  # noqa: E731
                                    else torch.zeros(shape, dtype=dtype, device=dev))
    iou = torch.cat(ious) if ious else torch.zeros(1, device=dev)
    pbox, gbox = pad(pbs, (1, 5), torch.float32).contiguous(), pad(gbs, (1, 5), torch.float32).contiguous()
    pint, gint = pad(pis, (1,), torch.int32), pad(gis, (1,), torch.int32)
    sizes = [p * g if p and g else 0 for p, g in zip(npred, ngt)]
    offs = lambda v: (np.concatenate([[0], np.cumsum(v)[:-1]]).astype(np.int64) if S  # noqa: E731
                      else np.zeros(0, np.int64))
    iou_off, pred_off, gt_off = offs(sizes), offs(npred), offs(ngt)
    tot, totg = int(sum(npred)), int(sum(ngt))
    h2d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_iou_off, d_pred_off, d_gt_off = h2d(iou_off), h2d(pred_off), h2d(gt_off)
    d_np, d_ng = h2d(np.asarray(npred, np.int32)), h2d(np.asarray(ngt, np.int32))
    cat = torch.empty(max(tot, 1), dtype=torch.uint8, device=dev)
    gts = torch.empty(max(totg, 1), dtype=torch.uint8, device=dev)
    best = torch.empty(max(tot, 1), dtype=torch.int32, device=dev)
    err = torch.empty((max(tot, 1), 4), dtype=torch.float64, device=dev)
    # one buffer for everything the host reads: tallies [S, nb, 12] | ap [S, 5] | confusion [S, nb, 8, 8]
    nt, na = S * nb * len(TALLY_COLUMNS), S * len(AP_VARIANTS)
    host = torch.empty(max(nt + na, 1), dtype=torch.float64, device=dev)
    conf = torch.empty(max(S * nb * _N_INTENT * _N_INTENT, 1), dtype=torch.int32, device=dev)
    h_edges = np.ascontiguousarray(edges, dtype=np.float32)
    ws = workspace(lib.ivit_det_errors_workspace(S, tot), dev)
    lib.ivit_det_errors(ptr(iou), ptr(d_iou_off), ptr(d_np), ptr(d_ng), ptr(d_pred_off), ptr(d_gt_off), S, tot,
                        ptr(pbox), ptr(gbox), ptr(pint), ptr(gint), float(iou_thr), float(bg_thr),
                        h_edges.ctypes.data if len(edges) else None, len(edges), ptr(cat), ptr(gts), ptr(best),
                        ptr(err), ptr(host), ptr(conf), ptr(host[nt:]) if S else ptr(host), ptr(ws), ws.numel(),
                        max(ngt, default=0), stream())
    # the one host read: the f64 buffer and the confusion counts (exact in f64) in one transfer
    flat = torch.cat([host[:nt + na], conf[:S * nb * _N_INTENT * _N_INTENT].double()]).cpu().numpy() if S \
        else np.zeros(0)
    tallies = flat[:nt].reshape(S, nb, len(TALLY_COLUMNS))
    ap = flat[nt:nt + na].reshape(S, len(AP_VARIANTS))
    confusion = np.rint(flat[nt + na:]).astype(np.int64).reshape(S, nb, _N_INTENT, _N_INTENT)
    report = report_from_tallies(tallies.sum(axis=0), confusion.sum(axis=0), ap, settings)
    report["ap_per_sample"] = ap
    report["per_sample"] = [
        {"category": cat[pred_off[i]:pred_off[i] + npred[i]],
         "errors": err[pred_off[i]:pred_off[i] + npred[i]], "best_gt": best[pred_off[i]:pred_off[i] + npred[i]],
         "gt_status": gts[gt_off[i]:gt_off[i] + ngt[i]]} for i in range(S)]
    report["tallies_per_sample"] = tallies
    report["confusion_per_sample"] = confusion
    return report


def _fmt(v, spec):
    return format(v, spec) if v == v else "-".rjust(len(format(0.0, spec)))


def format_error_report(report) -> str:
    """The report of error_analysis / report_from_tallies as a terminal table."""
    s = report["settings"]
    out = [f"Detection error breakdown @ IoU>={s['iou_thr']:g} (background < {s['bg_thr']:g}, "
           f"{'rotated' if s['rotated'] else 'axis-aligned'} IoU, {s['n_samples']} samples)",
           f"{'range [m]':<12}{'GT':>7}{'TP':>7}{'DUP':>7}{'LOC':>7}{'BKG':>7}{'near':>7}{'none':>7}"
           f"{'recall':>8}{'prec':>8}{'ATE':>8}{'ASE':>8}{'AOE':>8}{'AOE_pi':>8}"]

    def row(name, b):
        return (f"{name:<12}{b['gt']:>7}{b['tp']:>7}{b['dup']:>7}{b['loc']:>7}{b['bkg']:>7}"
                f"{b['missed_near']:>7}{b['missed_none']:>7}{_fmt(b['recall'], '8.3f')}{_fmt(b['precision'], '8.3f')}"
                f"{_fmt(b['ate'], '8.3f')}{_fmt(b['ase'], '8.3f')}{_fmt(b['aoe'], '8.3f')}{_fmt(b['aoe_pi'], '8.3f')}")

    for b in report["bins"]:
        lo, hi = b["range"]
        out.append(row(f"{lo:g}-{hi:g}" if hi != float("inf") else f"{lo:g}+", b))
    out.append(row("all", report["total"]))
    out.append("missed GTs: 'near' have a prediction at IoU >= background threshold, 'none' have not; "
               "ATE m, ASE 1-IoU, AOE rad (AOE_pi: heading-agnostic)")
    m, d = report["map"], report["dAP"]
    out.append(f"mAP {m['base']:.4f}; without an error type: " + ", ".join(
        f"{v} {m[v]:.4f} ({d[v]:+.4f})" for v in AP_VARIANTS[1:]))
    it = report["intention"]
    out.append(f"intention on TPs: accuracy {_fmt(it['accuracy'], '.4f').strip()}, F1 macro "
               f"{_fmt(it['f1_macro'], '.4f').strip()}, weighted {_fmt(it['f1_weighted'], '.4f').strip()}"
               + (f", {report['total']['intent_skipped']} outside 0..7" if report["total"]["intent_skipped"] else ""))
    return "\n".join(out)


def error_report_json(report) -> str:
    """The aggregate report as JSON: no tensors or per-sample arrays, nan / inf written as null."""
    def clean(v):
        if isinstance(v, dict):
            return {k: clean(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [clean(x) for x in v]
        if isinstance(v, (float, np.floating)):
            return float(v) if np.isfinite(v) else None
        if isinstance(v, np.integer):
            return int(v)
        return v
    import json
    keep = ("settings", "bins", "total", "intention", "map", "dAP")
    return json.dumps(clean({k: report[k] for k in keep}), indent=2, allow_nan=False)
