"""What ``--iou-loss-weight`` adds to the detection loss: DetectionIntentionLoss forward + backward
at B = 8, NA = 22 500 (the 400 x 720 grid's anchors), 60 GT boxes per sample drawn as
tools/det_errors_bench.py draws its own, with iou_loss_weight 0 and 1. Device events around CALLS
back-to-back forward + backward calls after a warm-up, the two weights alternating inside one run,
REPS repeats; the spread over the repeats is reported next to the median.

    python tools/iou_loss_bench.py [--out profiles/iou_loss_bench.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visiontransformer-intention-prediction_amd"))


def gt_boxes(rng, n):
    """GT boxes over the BEV extent (tools/det_errors_bench.py scene())."""
    return np.stack([rng.uniform(-20, 60, n), rng.uniform(-72, 72, n), rng.uniform(1.5, 3, n), rng.uniform(3, 9, n),
                     rng.uniform(-math.pi, math.pi, n)], 1)


def timed_us(fn, calls):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iou_loss_bench.json"))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--gt", type=int, default=60)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rotated-assign", action="store_true", help="use_rotated_iou=True for the assignment")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("iou_loss_bench.py measures on the GPU: no ROCm device visible")
    import loss as L
    import utils
    rng = np.random.default_rng(0)
    anchors = utils.generate_anchors(400, 720, 8, device="cuda")
    NA, B = anchors.shape[0], args.batch
    gts = [{"boxes_xywha": torch.from_numpy(gt_boxes(rng, args.gt).astype(np.float32)),
            "intentions": torch.from_numpy(rng.integers(0, 8, args.gt))} for _ in range(B)]
    g = torch.Generator().manual_seed(0)
    ts = [torch.randn((B, NA, 1), generator=g), 0.1 * torch.randn((B, NA, 6), generator=g),
          torch.randn((B, NA, 8), generator=g)]
    ts[1][..., 5] += 1.0  # cos-like: decoded yaw near the anchor's
    ts = [t.cuda().requires_grad_(True) for t in ts]
    losses = {lam: L.DetectionIntentionLoss(use_rotated_iou=args.rotated_assign, sync_guard=False,
                                            iou_loss_weight=lam) for lam in (0.0, 1.0)}

    def step(lam):
        for t in ts:
            t.grad = None
        d = losses[lam](*ts, anchors, gts)
        d["loss"].backward()
        return d

    for lam in losses:
        for _ in range(5):
            d = step(lam)
    torch.cuda.synchronize()
    npos, pos_iou = int(d["num_pos_anchors"]), float(d["pos_iou"])
    runs = {lam: [] for lam in losses}
    for lam in losses:
        timed_us(lambda: step(lam), 10)  # the timed loop's own warm-up (event creation, allocator)
    for _ in range(args.reps):
        for lam in losses:
            runs[lam].append(timed_us(lambda: step(lam), args.calls))
    # the term's own launches, called directly on the workspaces of one det-loss forward (no autograd,
    # no GT packing): an upper bound of their device time, the ctypes launch overhead included
    from _lib import lib, ptr, stream, workspace
    from loss import pack_gt
    gt, ng, gi = pack_gt(gts, "cuda")
    cls, box, it = (t.detach().reshape(B, NA, -1).contiguous() for t in ts)
    cfg = losses[1.0]._cfg("cuda")
    stats = torch.zeros((16,), dtype=torch.float32, device="cuda")
    ws = workspace(lib.ivit_det_loss_workspace(B, NA, gt.shape[1]), "cuda")
    iws = workspace(lib.ivit_det_iou_loss_workspace(B, NA), "cuda")
    lib.ivit_det_loss_fwd(ptr(cls), ptr(box), ptr(it), ptr(anchors), B, NA, 8, ptr(gt), ptr(ng), ptr(gi), gt.shape[1],
                          None, cfg["dominant_mask"], 0, None, cfg["pos_thr"], cfg["neg_thr"], cfg["alpha"],
                          cfg["gamma"], cfg["beta"], cfg["w_cls"], cfg["w_box"], cfg["w_int"], int(cfg["rotated"]),
                          ptr(stats), ptr(ws), ws.numel(), stream())
    stats0, dbox, one = stats.clone(), torch.zeros_like(box), torch.ones(1, device="cuda")

    def term_fwd():
        stats.copy_(stats0)
        lib.ivit_det_iou_loss_fwd(ptr(box), ptr(anchors), B, NA, ptr(gt), ptr(ng), gt.shape[1], int(cfg["rotated"]),
                                  cfg["w_box"], 1.0, ptr(ws), ws.numel(), ptr(stats), ptr(iws), iws.numel(), stream())

    def term_bwd():
        lib.ivit_det_iou_loss_bwd(B, NA, cfg["w_box"], 1.0, ptr(stats), ptr(one), ptr(ws), ws.numel(), ptr(iws),
                                  iws.numel(), ptr(dbox), stream())

    direct = {}
    for name, fn in (("fwd_with_stats_copy", term_fwd), ("bwd", term_bwd)):
        timed_us(fn, 10)
        v = [timed_us(fn, args.calls) for _ in range(args.reps)]
        direct[name] = {"us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}
    props = torch.cuda.get_device_properties(0)
    blk ={f"weight_{lam:g}": {"us": round(statistics.median(v), 1), "min_us": round(min(v), 1),
                               "max_us": round(max(v), 1)} for lam, v in runs.items()}
    added = [b - a for a, b in zip(runs[0.0], runs[1.0])]
    res = {"box": {"gpu": torch.cuda.get_device_name(0), "arch": getattr(props, "gcnArchName", None),
                   "torch": torch.__version__, "hip": torch.version.hip},
           "config": {"B": B, "NA": NA, "gt_per_sample": args.gt, "positives": npos, "pos_iou": round(pos_iou, 4),
                      "rotated_assignment": bool(args.rotated_assign), "calls_per_rep": args.calls, "reps": args.reps,
                      "timing": "device events around back-to-back loss forward + backward calls (host launches "
                                "included), warm, weights alternating within the run"},
           "loss_fwd_bwd": blk,
           "term_launches_direct": direct,
           "iou_term_adds_us": {"median": round(statistics.median(added), 1), "min": round(min(added), 1),
                                "max": round(max(added), 1)}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
