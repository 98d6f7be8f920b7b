"""What the weight EMA costs on IntentNetViT's real parameter list (bf16, 400x720; gradients, live
bf16 shadows and row-panel packs as two training steps leave them), all in one process, the four
cases alternating inside every repetition:

  (a) the update launch without the average (ivit_adamw_chunked);
  (b) the update launch with it (ivit_adamw_chunked_ema: +8 B per element on the 28 B + shadows);
  (c) (a) followed by torch._foreach_lerp_ on a plain copy of the parameters: the usual way to keep
      an EMA, a second pass of 12 B per element and one launch per tensor (or per foreach group);
  (d) ModelEMA.swapped() enter + exit: two ivit_swap_chunked launches (16 B per element + shadows
      each) and two ivit_weight_pack_multi rebuilds.

Recorded: (b) - (a) against (c) - (a), and against the byte estimate +8 / (bytes per element of (a)).
With --parent-tree DIR (a checkout of the parent commit with its library built): bench.py's default
line of this tree against the parent's, alternating, --reps runs each, before this process opens
the GPU — the default-off step must lie within the parent's own spread.

    python tools/ema_bench.py [--parent-tree ab/parent] [--out profiles/ema_bench.json]
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


def window_us(fn, iters):
    """Mean device time (events) of `iters` back-to-back calls."""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def summary(vals, nbytes=None):
    t = {"us": round(statistics.median(vals), 2), "min_us": round(min(vals), 2), "max_us": round(max(vals), 2)}
    if nbytes is not None:
        t.update(bytes=int(nbytes), floor_us=round(nbytes / HBM_PEAK * 1e6, 2),
                 achieved_TBps=round(nbytes / (t["us"] * 1e-6) / 1e12, 2))
    return t


def bench_line(tree, steps, warmup):
    r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup)], capture_output=True, text=True, timeout=600, cwd=tree)
    if r.returncode != 0:
        raise SystemExit(f"bench.py in {tree} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_bench.json"))
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--reps", type=int, default=3, help="bench.py runs per tree (alternating)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=100, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=7, help="timed windows per case (alternating a, b, c, d)")
    args = ap.parse_args()

    res = {"box": {"gpu": None, "torch": torch.__version__, "hip": torch.version.hip},
           "config": "IntentNetViT bf16, 400x720, FusedAdamW's parameter list after two training steps at B = 2",
           "hbm_peak_TBps": HBM_PEAK / 1e12}
    # bench.py children first: this process has not opened the GPU yet
    if args.parent_tree:
        runs, lines = {"parent": [], "this": []}, {}
        trees = (("parent", os.path.abspath(args.parent_tree)), ("this", ROOT))
        for rep in range(args.reps):
            for name, tree in (trees if rep % 2 == 0 else trees[::-1]):  # neither tree always runs second
                lines[name] = bench_line(tree, args.steps, args.warmup)
                runs[name].append(lines[name]["ms_per_step"])
        pm, tm = statistics.median(runs["parent"]), statistics.median(runs["this"])
        spread = max(runs["parent"]) - min(runs["parent"])
        res["bench_default_line"] = {
            "command": f"bench.py --gpus 1 --steps {args.steps} --warmup {args.warmup}", "ms_per_step": runs,
            "median_parent": pm, "median_this": tm, "diff_ms": round(tm - pm, 3), "parent_spread_ms": round(spread, 3),
            "this_spread_ms": round(max(runs["this"]) - min(runs["this"]), 3),
            "within_parent_spread": bool(abs(tm - pm) <= spread), "last_line_parent": lines["parent"],
            "last_line_this": lines["this"]}

    import loss as L
    import model_vit
    import ops
    import utils
    from _lib import lib, ptr, stream
    from optim import FusedAdamW, ModelEMA
    from synthetic import synthetic_batch
    from trainer import Trainer
    dev = torch.device("cuda", 0)
    props = torch.cuda.get_device_properties(0)
    res["box"].update(gpu=torch.cuda.get_device_name(0), arch=getattr(props, "gcnArchName", None),
                      compute_units=props.multi_processor_count, hbm_GB=round(props.total_memory / 2 ** 30, 1))
    H, W, B = 400, 720, 2
    torch.manual_seed(0)
    model = model_vit.IntentNetViT(backbone_cfg={"img_size": (H, W)}).to(dev).set_compute_dtype(torch.bfloat16).train()
    anchors = utils.generate_anchors(H, W, 8, device=dev)
    batch = synthetic_batch(B, (H, W), torch.Generator().manual_seed(1234), device=dev)
    opt = FusedAdamW(model.parameters(), lr=1e-4, weight_decay=1e-4)
    ema = ModelEMA(model)
    lf = L.DetectionIntentionLoss(use_rotated_iou=False, apply_intention_downsampling=True)
    tr = Trainer(model, lf, opt, anchors, check_nan=False, ema=ema)
    for _ in range(2):
        tr.step(batch)

    ps = [p for p in model.parameters() if p.grad is not None]
    n = sum(p.numel() for p in ps)
    nshadow = sum(p.numel() for p in ps if ops.shadow_of(p) is not None)
    npacked = sum(p.numel() * sum(x is not None for x in ops.packs_of(p)) for p in ps)
    res["parameters"] = {"tensors": len(ps), "elements": n, "shadowed_elements": nshadow, "pack_elements": npacked,
                         "tracked_by_ema": sum(v != 0 for v in ema._ptrs(ps))}
    one = torch.ones((), device=dev)
    st = [opt.state[p] for p in ps]
    tabs = [opt._table(ps, dev), opt._table([p.grad for p in ps], dev), opt._table([s["exp_avg"] for s in st], dev),
            opt._table([s["exp_avg_sq"] for s in st], dev)]
    tsh = opt._table_ptrs([ops.shadow_of(p).data_ptr() if ops.shadow_of(p) is not None else 0 for p in ps], dev)
    te = opt._table_ptrs(ema._ptrs(ps), dev)
    sizes, (chunks, nch) = opt._table_sizes(ps, dev), opt._table_chunks(ps, dev)
    sin, sout = opt._device_steps(ps)
    a = (len(ps), *[ptr(t) for t in tabs], ptr(tsh), ptr(sizes), ptr(chunks), nch, 1e-4, 0.9, 0.999, 1e-8, 1e-4, 1.0,
         1.0, ptr(one), ptr(sin), ptr(sout))
    copy = [p.detach().clone() for p in ps]  # (c): the average as a plain per-tensor copy
    live = [p.detach() for p in ps]
    w = 1.0 - ema.decay

    def case_a():
        lib.ivit_adamw_chunked(*a, stream())

    def case_b():
        lib.ivit_adamw_chunked_ema(*a, None, ptr(te), ema.decay, int(ema.warmup), stream())

    def case_c():
        lib.ivit_adamw_chunked(*a, stream())
        torch._foreach_lerp_(copy, live, w)

    def case_d():
        with ema.swapped(model):
            pass

    cases = {"a_update": case_a, "b_update_with_ema": case_b, "c_update_then_foreach_lerp": case_c,
             "d_swapped_enter_exit": case_d}
    for fn in cases.values():  # warm every case: code objects, table uploads, the foreach grouping
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in cases}
    for _ in range(args.windows):
        for k, fn in cases.items():
            t[k].append(window_us(fn, args.iters if k != "d_swapped_enter_exit" else max(args.iters // 5, 1)))
    upd = n * 28 + nshadow * 2
    nbytes = {"a_update": upd, "b_update_with_ema": upd + n * 8, "c_update_then_foreach_lerp": upd + n * 12,
              "d_swapped_enter_exit": 2 * (n * 16 + nshadow * 2)}  # (d): the swaps; the pack rebuilds come on top
    res["timing"] = {"iters_per_window": args.iters, "windows": args.windows, "order": "a, b, c, d alternating"}
    for k in cases:
        res[k] = summary(t[k], nbytes[k])
    fused = [b - x for x, b in zip(t["a_update"], t["b_update_with_ema"])]
    sep = [c - x for x, c in zip(t["a_update"], t["c_update_then_foreach_lerp"])]
    est = 8.0 * n / upd
    res["ema_cost"] = {
        "fused_b_minus_a_us": summary(fused), "separate_c_minus_a_us": summary(sep),
        "fused_over_a": round(statistics.median(fused) / res["a_update"]["us"], 3),
        "byte_estimate_over_a": round(est, 3),
        "fused_below_separate": bool(statistics.median(fused) < statistics.median(sep))}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
