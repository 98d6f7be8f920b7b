"""What the attention maps cost next to the forward they explain (ivit_attn_rows).

At B = 8, 400 x 720, bf16, R = 64 requests (8 per sample, cells spread over the grid), in one process:
* the eval forward of the batch (IntentNetViT under inference_mode);
* IntentNetViT.attention_maps of the same batch for the last block only and for all 12 blocks
  (each walks both ViT streams up to the last requested block: patch embedding, the blocks'
  forward, and per requested block one qkv GEMM + the attn_rows kernel);
* ops.attn_rows alone on a qkv tensor of the stream's shape (N = 4501, H = 6), head mean and per
  head, launched back to back with the requests already on the device, and the K bytes it reads
  (the K panel of every (request, head), once) over that time.
The three model timings alternate and repeat (``--rounds``), forward first and last, so the spread
of the forward's figures is the noise of the run. Warm timings: every shape runs before its timed
window; a window ends in a device synchronise. Writes one JSON file (default
profiles/attn_rows_bench.json) and prints it."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "visiontransformer-intention-prediction_amd")]
import torch

import _lib
import model_vit
import ops
from synthetic import synthetic_batch

LDS_KEYS = 15360  # csrc/attn_rows.hip AR_LDS_KEYS: scores kept in LDS between the kernel's two sweeps


def timed(fn, min_s=0.5, max_it=200):
    """-> (ms per call, calls): one warm call, then calls until min_s has passed (at most max_it)."""
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
    return 1e3 * (time.perf_counter() - t0) / it, it


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--grid", type=str, default="400x720")
    ap.add_argument("--per-sample", type=int, default=8, help="requests per sample (R = batch x this)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_rows_bench.json"))
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_rows_bench.py needs a ROCm GPU")
    commit = args.commit
    if commit is None:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else "unknown"
    H, W = (int(v) for v in args.grid.lower().split("x"))
    B, R = args.batch, args.batch * args.per_sample
    cd = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    torch.manual_seed(0)
    model = model_vit.IntentNetViT(backbone_cfg={"img_size": (H, W)}).cuda().set_compute_dtype(cd)
    model.train(False)
    batch = synthetic_batch(B, (H, W), torch.Generator().manual_seed(1234), device=torch.device("cuda"))
    lidar, mp = batch["lidar_bev"], batch["map_bev"]
    g = torch.Generator().manual_seed(5)
    sample = torch.arange(B).repeat_interleave(args.per_sample)
    # metric centres over the raster: x in (offset_y - H, offset_y) px, y in (-offset_x, W - offset_x) px, 0.2 m / px
    centres = torch.stack([(300.0 - H * torch.rand(R, generator=g)) * 0.2,
                           (W * torch.rand(R, generator=g) - 360.0) * 0.2], dim=1)

    def forward():
        with torch.inference_mode():
            model(lidar, mp)

    def maps(blocks):
        with torch.inference_mode():
            return model.attention_maps(lidar, mp, sample, centres, blocks=blocks)

    out = {"commit": commit, "device": torch.cuda.get_device_name(0), "dtype": args.dtype, "B": B, "grid": [H, W],
           "R": R, "rounds": []}
    legs = (("forward", forward), ("maps_last_block", lambda: maps((-1,))),
            ("maps_all_blocks", lambda: maps(tuple(range(12)))), ("forward_again", forward))
    for _ in range(args.rounds):
        row = {}
        for tag, fn in legs:
            ms, calls = timed(fn)
            row[tag + "_ms"], row[tag + "_calls"] = round(ms, 3), calls
        out["rounds"].append(row)
        print(json.dumps(row), flush=True)
    med = lambda k: sorted(r[k] for r in out["rounds"])[len(out["rounds"]) // 2]  # noqa: E731
    fwd = sorted(r[k] for r in out["rounds"] for k in ("forward_ms", "forward_again_ms"))
    out["forward_ms_min_median_max"] = [fwd[0], fwd[len(fwd) // 2], fwd[-1]]
    out["maps_last_block_ms_median"] = med("maps_last_block_ms")
    out["maps_all_blocks_ms_median"] = med("maps_all_blocks_ms")
    out["maps_last_block_over_forward"] = round(out["maps_last_block_ms_median"] / fwd[len(fwd) // 2], 3)
    out["maps_all_blocks_over_forward"] = round(out["maps_all_blocks_ms_median"] / fwd[len(fwd) // 2], 3)

    # the kernel alone, on a qkv tensor of the stream's shape
    vit = model.backbone.vit_lidar
    N, nh = vit.patch_embed.num_patches + 1, vit.blocks[0].attn.num_heads
    cdt = _lib.BF16 if cd == torch.bfloat16 else _lib.F32
    qkv = torch.randn((B * N, 3 * nh * 64), generator=torch.Generator().manual_seed(9)).to(cd).cuda()
    token = torch.randint(0, N, (R,), generator=g)
    # each (request, head) reads its K panel once, and again the keys whose scores do not fit in LDS
    k_bytes = R * nh * (N + max(0, N - LDS_KEYS)) * 64 * qkv.element_size()
    out["kernel"] = {"N": N, "H": nh, "R": R, "k_bytes_read": k_bytes, "out_bytes_head_mean": R * N * 4,
                     "out_bytes_per_head": R * nh * N * 4}
    req = ops.RowRequests(sample, token, B, N, qkv.device)  # uploaded once: the timed calls only launch
    for tag, hm in (("head_mean", True), ("per_head", False)):
        ms, calls = timed(lambda: ops.attn_rows(qkv, B, N, nh, cdt, req, head_mean=hm, prescaled=cd == torch.bfloat16))
        out["kernel"][tag + "_ms"], out["kernel"][tag + "_calls"] = round(ms, 4), calls
        out["kernel"][tag + "_k_read_TBps"] = round(k_bytes / (ms * 1e-3) / 1e12, 3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "rounds"}))


if __name__ == "__main__":
    main()
