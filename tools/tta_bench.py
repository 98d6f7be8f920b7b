"""Micro-benchmark of flip TTA and weighted box fusion in the eval post-processing
(ivit_eval_post_tta against ivit_eval_post).

utils.postprocess_batch at the config-4 shape (B = 32, NA = 22 500: the 400 x 720 grid, stride 8)
on trained-like logits: about 13 % of the anchors pass the confidence threshold (a few thousand
candidates per sample), the second view's scores are the first view's at the mirrored location
plus noise, so most objects are seen in both views. Per suppression test (axis, rotated):
  * eval_post          today's path (ivit_eval_post / ivit_eval_post_rotated);
  * tta_v1_fuse0       the new entry, one view, no fusion (the same rows, plus the cluster sizes);
  * tta_v1_fuse1       one view, fused;
  * tta_v2_fuse0       two views, NMS over the union;
  * tta_v2_fuse1       two views, fused.
Every figure includes the one host read of the counts and, for the new entry, the chunking of the
batch (utils.tta_chunk). Each configuration is timed --repeats times (warm; a window ends in a
device synchronise); the median, the extremes and the spread (max - min) / median are recorded.
Writes one JSON file (default profiles/tta_bench.json) and prints it."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "visiontransformer-intention-prediction_amd")]
import torch

import utils

CONF, THR = 0.1, 0.2


def timed(fn, min_s=0.3, max_it=30):
    """-> ms per call: one warm call, then calls until min_s has passed (at most max_it)."""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    one = time.perf_counter() - t0
    it = int(max(2, min(max_it, math.ceil(min_s / max(one, 1e-6)))))
    t0 = time.perf_counter()
    for _ in range(it):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / it


def views(B, Hf, Wf, A, seed):
    """Two views' logits: P(sigmoid(x) >= 0.1) = P(x >= ln(1/9)) = 13 % for x ~ N(-3.32, 1)."""
    g = torch.Generator().manual_seed(seed)
    NA = Hf * Wf * A
    cls0 = torch.randn(B, NA, generator=g) - 3.32
    cls1 = torch.flip(cls0.reshape(B, Hf, Wf, A), dims=[2]).reshape(B, NA) + 0.3 * torch.randn(B, NA, generator=g)
    out = []
    for cls in (cls0, cls1):
        box = torch.randn(B, NA, 6, generator=g) * 0.1
        box[..., 4] *= 0.2  # yaw delta atan2(d4, d5) near 0: the views agree on the heading
        box[..., 5] = 1.0
        out.append((cls.cuda(), box.cuda(), torch.randn(B, NA, 8, generator=g).cuda()))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tta_bench.json"))
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD)")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--grid", type=str, default="400x720")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tta_bench.py needs a ROCm GPU")
    commit = args.commit
    if commit is None:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else "unknown"
    H, W = (int(v) for v in args.grid.lower().split("x"))
    anchors = utils.generate_anchors(H, W, 8)
    NA, B = anchors.shape[0], args.batch
    v0, v1 = views(B, H // 8, W // 8, NA // ((H // 8) * (W // 8)), 17)
    out = {"commit": commit, "device": torch.cuda.get_device_name(0), "B": B, "NA": NA, "conf_thr": CONF,
           "iou_thr": THR, "repeats": args.repeats,
           "passing_per_sample": [round(float((torch.sigmoid(v[0]) >= CONF).sum()) / B, 1) for v in (v0, v1)],
           "rows": []}
    for rot in (False, True):
        configs = [("eval_post", {}), ("tta_v1_fuse0", None), ("tta_v1_fuse1", {"fuse_boxes": True}),
                   ("tta_v2_fuse0", {"tta_logits": v1}), ("tta_v2_fuse1", {"tta_logits": v1, "fuse_boxes": True})]
        row = {"rotated": rot, "chunk_v1": utils.tta_chunk(B, 1, NA, rot), "chunk_v2": utils.tta_chunk(B, 2, NA, rot)}
        for name, kw in configs:
            if kw is None:  # one view, no fusion, through the new entry
                fn = lambda: utils._post_collect(utils._post_launch_tta([v0], anchors, CONF, THR, rot, False))  # noqa: E731
            else:
                fn = lambda kw=kw: utils.postprocess_batch(*v0, anchors, CONF, THR, rotated_nms=rot, **kw)  # noqa: E731
            ms = [timed(fn) for _ in range(args.repeats)]
            res = fn()
            med = statistics.median(ms)
            row[name] = {"ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
                         "spread": round((max(ms) - min(ms)) / med, 4),
                         "kept_per_sample": round(sum(p["pred_scores"].numel() for p in res) / B, 1)}
            if "pred_members" in res[0]:
                row[name]["members_per_kept"] = round(
                    sum(int(p["pred_members"].sum()) for p in res) / max(1, sum(p["pred_scores"].numel() for p in res)), 2)
        out["rows"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
