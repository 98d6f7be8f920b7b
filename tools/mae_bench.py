"""What MAE pre-training costs at the workload's shape (B = 8, 400x720, bf16, mask ratio 0.75), all
in one process:

  * the pre-training step (forward, backward, FusedAdamW update with the loss's finite flag) of
    mae.MaskedAutoencoderViT for the LiDAR stream (290 channels) and the map stream (9 channels),
    vit_small_patch8_224 encoder, decoder 192 x 4;
  * each new kernel on its own at the LiDAR stream's shape (Np = 4500, K = 1125, Nm = 3375,
    L = 18 560), with the bytes it has to move (computed from the shapes below) and the bandwidth
    that implies against the HBM peak: ivit_token_select as the encoder gather (D = 384) and as the
    decoder un-shuffle with mask token and position table (D = 192), ivit_token_fill_grad,
    ivit_mae_loss_fwd (with and without norm_pix) and ivit_mae_loss_bwd; the loss also at the map
    stream's L = 576.

Nothing existed to compare with: the values are recorded, no threshold is set.

    python tools/mae_bench.py [--out profiles/mae_bench.json]
"""
import argparse
import json
import os
import statistics
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
                 achieved_TBps=round(nbytes / (t["us"] * 1e-6) / 1e12, 3))
    return t


def timed(fn, iters, windows, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    return [window_us(fn, iters) for _ in range(windows)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mae_bench.json"))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--grid", default="400x720")
    ap.add_argument("--step-iters", type=int, default=5, help="steps per timed window")
    ap.add_argument("--iters", type=int, default=20, help="kernel calls per timed window")
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mae_bench.py measures on the GPU: no ROCm device visible")

    import mae
    import ops
    from optim import FusedAdamW
    from synthetic import synthetic_batch
    dev = torch.device("cuda", 0)
    props = torch.cuda.get_device_properties(0)
    H, W = (int(v) for v in args.grid.lower().split("x"))
    B, P = args.batch, 8
    Np = (H // P) * (W // P)
    K = mae.kept_count(Np, 0.75)
    Nm = Np - K
    res = {"box": {"gpu": torch.cuda.get_device_name(0), "arch": getattr(props, "gcnArchName", None),
                   "compute_units": props.multi_processor_count, "torch": torch.__version__, "hip": torch.version.hip},
           "config": f"B = {B}, {H}x{W}, bf16, mask ratio 0.75, vit_small_patch8_224 encoder, decoder 192 x 4",
           "shape": {"Np": Np, "kept": K, "masked": Nm}, "hbm_peak_TBps": HBM_PEAK / 1e12,
           "timing": {"step_iters_per_window": args.step_iters, "kernel_iters_per_window": args.iters,
                      "windows": args.windows, "clock": "device events around back-to-back calls, after warm-up"}}
    batch = synthetic_batch(B, (H, W), torch.Generator().manual_seed(1234), device=dev)

    # ---- the pre-training step, both streams
    for stream, key, C in (("map", "map_bev", 9), ("lidar", "lidar_bev", 290)):
        torch.manual_seed(0)
        model = mae.create_mae("vit_small_patch8_224", C, (H, W)).to(dev).set_compute_dtype(torch.bfloat16).train()
        opt = FusedAdamW(model.parameters(), lr=1.5e-4, betas=(0.9, 0.95), weight_decay=0.05)
        x = batch[key]

        def step():
            opt.zero_grad(set_to_none=True)
            loss, _ = model(x)
            loss.backward()
            opt.step(finite=model.last_finite)

        t = timed(step, args.step_iters, args.windows)
        torch.cuda.synchronize()
        res[f"step_{stream}"] = dict(summary(t), ms=round(statistics.median(t) / 1e3, 3), channels=C,
                                     samples_per_s=round(B / (statistics.median(t) * 1e-6), 2),
                                     peak_memory_GB=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))
        del model, opt
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()

    # ---- the kernels on their own (LiDAR stream's shape)
    g = torch.Generator().manual_seed(5)
    noise = torch.rand((B, Np), generator=g).to(dev)
    ids_shuffle, ids_restore, _ = mae.random_masking_indices(noise, K)
    i32 = torch.int32
    zero = torch.zeros((B, 1), dtype=i32, device=dev)
    enc_idx = torch.cat([zero, ids_shuffle[:, :K].to(i32) + 1], 1).contiguous()
    r = ids_restore.to(i32)
    dec_idx = torch.cat([zero, torch.where(r < K, r + 1, torch.full_like(r, -1))], 1).contiguous()
    pidx = torch.sort(ids_shuffle[:, K:], dim=1).values.to(i32).contiguous()
    kern = {}
    D, Dd = 384, 192
    tok = torch.randn((B * (Np + 1), D), device=dev)
    kern["token_select_encoder_gather_D384"] = (
        lambda: ops.token_select(tok, B, Np + 1, enc_idx),
        2 * B * (1 + K) * D * 4 + B * (1 + K) * 4)  # the gathered rows read and written, the index
    y = torch.randn((B * (1 + K), Dd), device=dev)
    mtok, pos = torch.randn((Dd,), device=dev), torch.randn((Np + 1, Dd), device=dev)
    kern["token_select_decoder_unshuffle_D192"] = (
        lambda: ops.token_select(y, B, 1 + K, dec_idx, fill=mtok, add=pos),
        B * (1 + K) * Dd * 4 + B * (Np + 1) * Dd * 4 + (Np + 1) * Dd * 4 + B * (Np + 1) * 4)
    dy = torch.randn((B * (Np + 1), Dd), device=dev)
    gout = torch.empty((Dd,), device=dev)
    kern["token_fill_grad_D192"] = (
        lambda: ops.token_fill_grad(dy, B, dec_idx, 1 + K, out=gout),
        B * Nm * Dd * 4 + B * (Np + 1) * 4)  # the masked rows of dy, the index
    one = torch.ones((1,), device=dev)
    for stream, key, C in (("lidar", "lidar_bev", 290), ("map", "map_bev", 9)):
        L = C * P * P
        img = batch[key]
        pred = torch.randn((B * Nm, L), device=dev).to(torch.bfloat16)
        fwd_bytes = B * Nm * L * (2 + 4) + B * Nm * 4 * 4  # pred (bf16) + the masked patches of the raster
        for npx in (False, True):
            kern[f"mae_loss_fwd_{stream}" + ("_norm_pix" if npx else "")] = (
                lambda pred=pred, img=img, npx=npx: ops.mae_loss_fwd(pred, img, pidx, P, npx), fwd_bytes)
        _, fin, _, stats = ops.mae_loss_fwd(pred, img, pidx, P, False)
        kern[f"mae_loss_bwd_{stream}"] = (
            lambda pred=pred, img=img, stats=stats, fin=fin: ops.mae_loss_bwd(pred, img, pidx, P, stats, one, fin),
            B * Nm * L * (2 + 4 + 2))
    for name, (fn, nbytes) in kern.items():
        res[name] = summary(timed(fn, args.iters, args.windows), nbytes)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
