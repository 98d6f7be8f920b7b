"""What gradient-norm clipping costs on the IntentNetViT parameter set (B = 8, 400x720, bf16), each
figure next to its floor (bytes moved / 8 TB/s HBM3E peak, as DESIGN.md states floors):

* the two ivit_grad_norm launches, warm, isolated;
* the AdamW launch plain (ivit_adamw_chunked) and with the device gradient scale
  (ivit_adamw_chunked_scaled), and the unfused ivit_grad_scale pass;
* the full train step with and without Trainer(max_grad_norm=...), same process, alternating;
* with --parent-tree DIR (a checkout of the parent commit with its library built, e.g. from
  ``git archive`` + tools/ab_build.sh): bench.py's default line of this tree against the parent's,
  alternating, REPS runs each — the unclipped step must lie within the parent's own spread.

    python tools/grad_clip_bench.py [--parent-tree ab/parent] [--out profiles/grad_clip_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visiontransformer-intention-prediction_amd"))
HBM_PEAK = 8.0e12  # B/s, HBM3E


def timed_us(fn, iters=20, reps=5):
    """Median over reps of the mean device time of `iters` back-to-back calls (events), warm."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) / iters * 1e3)
    return {"us": round(statistics.median(out), 2), "min_us": round(min(out), 2), "max_us": round(max(out), 2)}


def with_floor(t, nbytes):
    t = dict(t, bytes=int(nbytes), floor_us=round(nbytes / HBM_PEAK * 1e6, 2))
    t["achieved_TBps"] = round(nbytes / (t["us"] * 1e-6) / 1e12, 2)
    t["frac_of_peak"] = round(t["floor_us"] / t["us"], 3)
    return t


def bench_line(tree, steps, warmup):
    r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup)], capture_output=True, text=True, timeout=600, cwd=tree)
    if r.returncode != 0:
        raise SystemExit(f"bench.py in {tree} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_clip_bench.json"))
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--reps", type=int, default=3, help="bench.py runs per tree (alternating)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4, help="alternations of the clipped / unclipped full step")
    args = ap.parse_args()

    res = {"box": {"gpu": None, "torch": torch.__version__, "hip": torch.version.hip},
           "config": "IntentNetViT bf16, B = 8, 400x720, FusedAdamW, check_nan=False", "hbm_peak_TBps": HBM_PEAK / 1e12}
    # bench.py children first: this process has not opened the GPU yet
    if args.parent_tree:
        runs = {"parent": [], "this": []}
        for _ in range(args.reps):
            for name, tree in (("parent", os.path.abspath(args.parent_tree)), ("this", ROOT)):
                runs[name].append(bench_line(tree, args.steps, args.warmup)["ms_per_step"])
        pm, tm = statistics.median(runs["parent"]), statistics.median(runs["this"])
        spread = max(runs["parent"]) - min(runs["parent"])
        res["bench_default_line"] = {
            "command": f"bench.py --gpus 1 --steps {args.steps} --warmup {args.warmup}", "ms_per_step": runs,
            "median_parent": pm, "median_this": tm, "diff_ms": round(tm - pm, 3), "parent_spread_ms": round(spread, 3),
            "within_parent_spread": bool(abs(tm - pm) <= spread)}

    import loss as L
    import model_vit
    import ops
    import utils
    from _lib import lib, ptr, stream
    from optim import FusedAdamW
    from synthetic import synthetic_batch
    from trainer import Trainer
    dev = torch.device("cuda", 0)
    props = torch.cuda.get_device_properties(0)
    res["box"].update(gpu=torch.cuda.get_device_name(0), arch=getattr(props, "gcnArchName", None),
                      compute_units=props.multi_processor_count, hbm_GB=round(props.total_memory / 2 ** 30, 1))
    H, W, B = 400, 720, 8
    torch.manual_seed(0)
    model = model_vit.IntentNetViT(backbone_cfg={"img_size": (H, W)}).to(dev).set_compute_dtype(torch.bfloat16).train()
    anchors = utils.generate_anchors(H, W, 8, device=dev)
    batch = synthetic_batch(B, (H, W), torch.Generator().manual_seed(1234), device=dev)
    opt = FusedAdamW(model.parameters(), lr=1e-4, weight_decay=1e-4)
    lf = L.DetectionIntentionLoss(use_rotated_iou=False, apply_intention_downsampling=True)
    plain = Trainer(model, lf, opt, anchors, check_nan=False)
    clip = Trainer(model, lf, opt, anchors, check_nan=False, max_grad_norm=1.0)

    # full step, alternating in one process
    full = {"plain": [], "clipped": []}
    for tr in (plain, clip):
        for _ in range(3):
            tr.step(batch)
    for _ in range(args.rounds):
        for name, tr in (("plain", plain), ("clipped", clip)):
            full[name].append(timed_us(lambda: tr.step(batch), iters=10, reps=1)["us"] / 1e3)
    res["full_step_ms"] = {k: [round(v, 3) for v in vs] for k, vs in full.items()}
    res["full_step_ms"]["median_plain"] = round(statistics.median(full["plain"]), 3)
    res["full_step_ms"]["median_clipped"] = round(statistics.median(full["clipped"]), 3)
    res["full_step_ms"]["clip_cost_ms"] = round(res["full_step_ms"]["median_clipped"] - res["full_step_ms"]["median_plain"], 3)
    st = clip.grad_stats()
    res["grad_stats_of_the_clipped_steps"] = st

    # isolated launches on the step's own gradients
    ps = [p for p in model.parameters() if p.grad is not None]
    n = sum(p.numel() for p in ps)
    nshadow = sum(p.numel() for p in ps if ops.shadow_of(p) is not None)
    res["parameters"] = {"tensors": len(ps), "elements": n, "grad_MB": round(n * 4 / 1e6, 1)}
    one = torch.ones((), device=dev)
    grads = [p.grad for p in ps]
    tg, sizes, (chunks, nch) = opt._table(grads, dev), opt._table_sizes(ps, dev), opt._table_chunks(ps, dev)
    ws = torch.empty(lib.ivit_grad_norm_workspace(nch), dtype=torch.uint8, device=dev)
    rec = torch.empty(4, device=dev)
    na = (len(ps), ptr(tg), ptr(sizes), ptr(chunks), nch, 1.0, ptr(one), ptr(ws), ws.numel(), ptr(rec), None)
    res["grad_norm_two_launches"] = with_floor(timed_us(lambda: lib.ivit_grad_norm(*na, stream())), n * 4 + nch * 16)
    # the same through FusedAdamW.grad_norm: back to back the host side (327-entry table keys) is the limit
    res["grad_norm_python_call"] = timed_us(lambda: opt.grad_norm(1.0, finite=one))
    half = torch.full((), 0.999, device=dev)
    res["grad_scale_pass"] = with_floor(timed_us(lambda: opt._scale_launch(grads, half)), n * 8)
    # the update alone (the pack rebuild that FusedAdamW.step adds is the same in both forms)
    st_ = [opt.state[p] for p in ps]
    tabs = [opt._table(ps, dev), opt._table(grads, dev), opt._table([s["exp_avg"] for s in st_], dev),
            opt._table([s["exp_avg_sq"] for s in st_], dev)]
    tsh = opt._table_ptrs([ops.shadow_of(p).data_ptr() if ops.shadow_of(p) is not None else 0 for p in ps], dev)
    sin, sout = opt._device_steps(ps)
    a = (len(ps), *[ptr(t) for t in tabs], ptr(tsh), ptr(sizes), ptr(chunks), nch, 1e-4, 0.9, 0.999, 1e-8, 1e-4, 1.0,
         1.0, ptr(one), ptr(sin), ptr(sout))
    upd_bytes = n * 28 + nshadow * 2
    res["adamw_plain"] = with_floor(timed_us(lambda: lib.ivit_adamw_chunked(*a, stream())), upd_bytes)
    res["adamw_scaled"] = with_floor(timed_us(lambda: lib.ivit_adamw_chunked_scaled(*a, ptr(one), stream())), upd_bytes)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
