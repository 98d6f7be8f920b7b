"""Dropped share of the bench's DropPath draws, and the DropPath row skip's predicted against its measured
saving (DESIGN.md §3 "DropPath row skip").

Builds bench.py's train model with bench.py's seeds (torch.manual_seed(0) before the constructor, the
synthetic batch from generator 1234), runs the same warm-up + timed steps once with IVIT_KNOB_DROP_SKIP 0
and once with 1 — both from the same seed, so they see the same draws — and counts, per timed step, the
zero factors in every block's ``last_scales``: a (sample, branch) unit with factor 0 is what the skip
leaves out. Prints the dropped share, the saving predicted from it and the isolated attention times
(one attention-branch unit costs (fwd + bwd pair) / B of kernel time), and the measured difference.

    python tools/drop_skip_bench.py [--steps 20 --warmup 3 --attn-fwd-ms 0.276 --attn-bwd-ms 0.70]

One JSON line on stdout. The two variants run one after the other in one process: the measured
difference is a same-call figure, but the step A/B of record is the alternating bench.py one.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visiontransformer-intention-prediction_amd"))


def run(knob, args):
    import torch

    import loss as L
    import model_vit
    import utils
    from _lib import KNOB_DROP_SKIP, lib
    from optim import FusedAdamW
    from synthetic import synthetic_batch
    from trainer import Trainer
    H, W = (int(v) for v in args.grid.split("x"))
    dev = torch.device("cuda:0")
    lib.ivit_set_knob(KNOB_DROP_SKIP, knob)
    torch.manual_seed(0)
    model = model_vit.IntentNetViT(backbone_cfg={"img_size": (H, W)}).to(dev).set_compute_dtype(torch.bfloat16)
    model.train()
    anchors = utils.generate_anchors(H, W, 8, device=dev)
    batch = synthetic_batch(args.batch, (H, W), torch.Generator().manual_seed(1234), device=dev)
    opt = FusedAdamW(model.parameters(), lr=1e-4, weight_decay=1e-4)
    lf = L.DetectionIntentionLoss(use_rotated_iou=False, apply_intention_downsampling=True)
    trainer = Trainer(model, lf, opt, anchors, world=1, check_nan=False)
    blocks = list(model.backbone.vit_lidar.blocks) + list(model.backbone.vit_map.blocks)
    for _ in range(args.warmup):
        trainer.step(batch)
    torch.cuda.synchronize()
    kept = []  # per step: the blocks' factor tensors (read after the timed region: no sync inside it)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        d = trainer.step(batch)
        kept.append([blk.last_scales for blk in blocks])
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    units = drop_attn = drop_mlp = 0
    for step in kept:
        for s1, s2 in step:
            units += 2 * args.batch
            if s1 is not None:
                drop_attn += int((s1 == 0).sum())
                drop_mlp += int((s2 == 0).sum())
    loss = float(d["loss"].detach())
    lib.ivit_set_knob(KNOB_DROP_SKIP, 1)
    del trainer, opt, model
    torch.cuda.empty_cache()
    return {"knob": knob, "ms_per_step": ms, "units_per_step": units / args.steps,
            "dropped_attn_per_step": drop_attn / args.steps, "dropped_mlp_per_step": drop_mlp / args.steps,
            "loss": loss}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--grid", type=str, default="400x720")
    ap.add_argument("--attn-fwd-ms", type=float, default=0.276, help="isolated attention forward, all samples")
    ap.add_argument("--attn-bwd-ms", type=float, default=0.70, help="isolated attention backward pair")
    args = ap.parse_args()
    off, on = run(0, args), run(1, args)
    assert (off["dropped_attn_per_step"], off["dropped_mlp_per_step"]) == \
        (on["dropped_attn_per_step"], on["dropped_mlp_per_step"]), "the two variants saw different draws"
    dropped = on["dropped_attn_per_step"] + on["dropped_mlp_per_step"]
    unit_ms = (args.attn_fwd_ms + args.attn_bwd_ms) / args.batch
    out = {"tool": "drop_skip_bench", "steps": args.steps, "warmup": args.warmup, "batch": args.batch,
           "grid": args.grid, "units_per_step": on["units_per_step"],
           "dropped_attn_per_step": on["dropped_attn_per_step"], "dropped_mlp_per_step": on["dropped_mlp_per_step"],
           "dropped_share": dropped / on["units_per_step"],
           "expected_share": 2 * 0.6 / 24,  # sum of linspace(0, 0.1, 12) over 12 blocks x 2 branches, per stream
           "attn_unit_ms": unit_ms, "predicted_attn_saving_ms": on["dropped_attn_per_step"] * unit_ms,
           "ms_per_step_skip_off": off["ms_per_step"], "ms_per_step_skip_on": on["ms_per_step"],
           "measured_saving_ms": off["ms_per_step"] - on["ms_per_step"],
           "loss_skip_off": off["loss"], "loss_skip_on": on["loss"]}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
