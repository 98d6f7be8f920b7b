"""Windowed attention against global attention: the isolated _q2 kernels and the training step.

    python tools/win_attn_bench.py kernels [--out profiles/win_attn_bench.json]
    python tools/win_attn_bench.py step    [--out ...]     (merges into the same file)
    python tools/win_attn_bench.py once                    (a few launches of each kernel, for
                                                            rocprofv3 --kernel-trace --stats)

kernels: ivit_attn_win_fwd_q2 / _bwd_q2 with 10 x 10 windows against ivit_attn_fwd_q2 / _bwd_q2 at
B = 8, H = 6 on the 50 x 90 and 100 x 180 grids; warm, REPEATS windows of ITERS launches between two
device events, per-launch ms of every window reported (min / median / max). For the windowed kernels
also the bytes they must move over the time, in TB/s and as a fraction of the 8.0 TB/s HBM3E peak and
of the 6.29 TB/s a float4 copy reaches (MI355X_MICROARCH.md): forward qkv read + o written, backward
qkv and dout read + dqkv written (it reads neither o nor lse). Back-to-back launches on the same
buffers: at 50 x 90 the 110 / 193 MB fit the 256 MB Infinity Cache, so a figure above the HBM rate there
is the cache, not HBM.

step: `train_vit.py --synthetic --dtype bf16 --batch 8` itself at 400 x 720 and 800 x 1440 (B = 8 is also
the batch of the README's large-grid figure), without and with `--window 10x10`, one process per run,
alternating (global, windowed, global, windowed); the samples/s of the epoch summaries it logs, the first
epoch (warm-up) kept apart.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visiontransformer-intention-prediction_amd"))

B, H, WIN = 8, 6, (10, 10)
GRIDS = ((50, 90), (100, 180))
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12


def _summ(ms):
    return {"min_ms": min(ms), "median_ms": statistics.median(ms), "max_ms": max(ms), "windows": ms}


def _time(fn, repeats, iters, warm=3):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return out


def _operands(gh, gw):
    import torch
    N, D = 1 + gh * gw, H * 64
    g = torch.Generator().manual_seed(gh * 1000 + gw)
    qkv = (torch.randn((B * N, 3 * D), generator=g) * 0.5).to(torch.bfloat16).cuda()
    dout = torch.randn((B * N, D), generator=g).to(torch.bfloat16).cuda()
    return N, D, qkv, dout


def kernels(args):
    import ops
    res = {}
    for gh, gw in GRIDS:
        N, D, qkv, dout = _operands(gh, gw)
        win = (gh, gw) + WIN
        o_w, lse_w = ops.attn_win_fwd_q2(qkv, B, N, H, win)
        o_g, lse_g = ops.attn_fwd_q2(qkv, B, N, H)
        iters = args.iters if N < 10000 else max(2, args.iters // 8)
        t = {"win_fwd": _time(lambda: ops.attn_win_fwd_q2(qkv, B, N, H, win), args.repeats, iters),
             "global_fwd": _time(lambda: ops.attn_fwd_q2(qkv, B, N, H), args.repeats, iters),
             "win_bwd": _time(lambda: ops.attn_win_bwd_q2(qkv, o_w, dout, lse_w, B, N, H, win), args.repeats, iters),
             "global_bwd": _time(lambda: ops.attn_bwd_q2(qkv, o_g, dout, lse_g, B, N, H), args.repeats, iters)}
        elems = B * N * D
        floor = {"win_fwd": 2 * 4 * elems, "win_bwd": 2 * 7 * elems}  # bytes: qkv + o; qkv + dout + dqkv
        entry = {"tokens": N, "iters_per_window": iters}
        for k, ms in t.items():
            entry[k] = _summ(ms)
            if k in floor:
                rate = floor[k] / (entry[k]["median_ms"] * 1e-3)
                entry[k].update(floor_bytes=floor[k], tb_per_s=rate / 1e12, frac_hbm_peak=rate / HBM_PEAK,
                                frac_hbm_copy=rate / HBM_COPY, floor_us_at_copy_rate=floor[k] / HBM_COPY * 1e6)
        entry["fwd_speedup"] = entry["global_fwd"]["median_ms"] / entry["win_fwd"]["median_ms"]
        entry["bwd_speedup"] = entry["global_bwd"]["median_ms"] / entry["win_bwd"]["median_ms"]
        res[f"{gh}x{gw}"] = entry
        print(f"kernels {gh}x{gw}: " + " ".join(f"{k}={entry[k]['median_ms']:.4f}ms" for k in t), flush=True)
    return {"kernels": {"B": B, "H": H, "window": list(WIN), "repeats": args.repeats, "grids": res}}


def once(args):
    import torch

    import ops
    for gh, gw in GRIDS:
        N, D, qkv, dout = _operands(gh, gw)
        win = (gh, gw) + WIN
        for _ in range(5):
            o_w, lse_w = ops.attn_win_fwd_q2(qkv, B, N, H, win)
            ops.attn_win_bwd_q2(qkv, o_w, dout, lse_w, B, N, H, win)
            o_g, lse_g = ops.attn_fwd_q2(qkv, B, N, H)
            ops.attn_bwd_q2(qkv, o_g, dout, lse_g, B, N, H)
        torch.cuda.synchronize()
    return None


def _entry_run(grid, window, batches, epochs):
    """One `train_vit.py --synthetic --dtype bf16 --grid HxW --batch 8 [--window 10x10]` process ->
    the samples/s of its epoch summaries (the first epoch holds the warm-up and is reported apart)."""
    import re
    import subprocess
    cmd = [sys.executable, os.path.join(ROOT, "visiontransformer-intention-prediction_amd", "train_vit.py"),
           "--synthetic", "--dtype", "bf16", "--grid", f"{grid[0]}x{grid[1]}", "--batch", str(B), "--epochs",
           str(epochs), "--batches-per-epoch", str(batches), "--no-save"]
    if window is not None:
        cmd += ["--window", f"{window[0]}x{window[1]}"]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stdout
    rates = [float(v) for v in re.findall(r"\[([0-9.]+) samples/s\]", out)]
    if len(rates) != epochs:
        raise RuntimeError(f"{' '.join(cmd)}: {len(rates)} epoch summaries for {epochs} epochs\n{out[-2000:]}")
    line = [ln for ln in out.splitlines() if ln.startswith("Windowed attention")]
    return rates, (line[0] if line else None)


def step(args):
    """The entry point itself, one process per run, global and windowed alternating; B = 8 at both grids
    (the batch behind the README's 800 x 1440 figure, profiles/r04_g_bench_large_config5.json)."""
    res = {}
    for grid, batches in (((400, 720), args.steps), ((800, 1440), max(4, args.steps // 4))):
        runs = {"global": [], "windowed": []}
        first = {"global": [], "windowed": []}
        line = None
        for _ in range(args.rounds):
            for name, window in (("global", None), ("windowed", WIN)):
                rates, ln = _entry_run(grid, window, batches, args.epochs)
                first[name].append(rates[0])
                runs[name].append(rates[1:])
                line = ln or line
                print(f"step {grid[0]}x{grid[1]} {name}: epochs {rates} samples/s", flush=True)
        flat = {k: [r for run in v for r in run] for k, v in runs.items()}
        g, w = statistics.median(flat["global"]), statistics.median(flat["windowed"])
        res[f"{grid[0]}x{grid[1]}"] = {
            "batch": B, "batches_per_epoch": batches, "epochs": args.epochs,
            "samples_per_s_global": runs["global"], "samples_per_s_windowed": runs["windowed"],
            "first_epoch_samples_per_s": first, "median_ms_per_step_global": B / g * 1e3,
            "median_ms_per_step_windowed": B / w * 1e3, "speedup": w / g, "log_line": line}
    return {"train_step": {"command": "train_vit.py --synthetic --dtype bf16 --grid HxW --batch 8 --no-save "
                                      "[--window 10x10]", "window": list(WIN), "grids": res}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernels", "step", "once"])
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "win_attn_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("win_attn_bench.py measures on the GPU: no ROCm device visible")
    part = {"kernels": kernels, "step": step, "once": once}[args.mode](args)
    if part is None:
        return
    doc = {"tool": "win_attn_bench", "device": torch.cuda.get_device_name(0)}
    if os.path.isfile(args.out):
        with open(args.out) as f:
            doc.update(json.load(f))
    doc.update(part)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(part), flush=True)


if __name__ == "__main__":
    main()
