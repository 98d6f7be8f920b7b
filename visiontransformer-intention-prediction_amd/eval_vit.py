"""IntentNetViT evaluation entry point — the flow of the reference's eval_vit.py:27-316 on the
MI355X kernels (BASELINE config 4: batched forward + rotated/axis IoU + NMS on one GPU).

Checkpoint → model (same cfg defaults as eval_vit.py:72-84) → anchors → batched inference with
confidence threshold 0.1, decode, NMS(0.2), argmax intention → detection mAP at
DETECTION_IOU_THRESHOLDS and intention accuracy / F1 on matched detections.

Differences, none in the numerics: without ``--synthetic`` the Argoverse-2 logs under
``--data-dir`` (VAL_DATA_DIR by default) are evaluated through dataset.FrameBatchLoader, rasters
built on the GPU, on the constants.py grid only; ``--synthetic`` evaluates seeded synthetic BEV batches
(random-init weights when no checkpoint exists, which makes every anchor pass the threshold
— the worst case for NMS); checkpoints load with ``torch.load(weights_only=True)`` (the
pickled ``BasicBlock`` class in ``backbone_cfg`` is allow-listed by name); post-processing runs
on the device for the whole batch (utils.postprocess_batch, pipelined by utils.PostPipeline); the mAP / intention matching
walk runs on the device for all samples in one launch (metrics.match_device, ivit_det_match). The reference's undefined names (eval_vit.py:12-13,39,196,219)
come from constants.py / utils.py. ``--rotated-nms`` (off by default; the reference's future work)
makes the NMS suppress on the rotated IoU of the decoded boxes instead of their axis-aligned corners.
``--tta-flip`` (off by default) runs every batch a second time on the mirrored rasters (the training
flip) and merges both views' candidates, the second un-mirrored, before the NMS; ``--fuse-boxes``
(off by default) replaces every kept box by the score-weighted fusion of the candidates it
suppressed and its intention by their weighted vote (utils.postprocess_batch, ivit_eval_post_tta).
The two are independent of each other and of ``--rotated-nms``.
``--attn-maps DIR`` (the reference's other future-work item, qualitative analysis of the attention)
writes, per batch, the attention maps of both ViT streams for each sample's ``--attn-top`` best
detections at ``--attn-blocks`` (AttnDump; IntentNetViT.attention_maps).
``--error-report PATH`` (the reference's "detailed error analysis" future-work item) says where the
mAP is lost: after the intention block it prints, per range bin from the ego vehicle
(``--error-range-edges``), how many detections at ``--error-iou`` are true positives, duplicates,
mislocalised (best IoU between ``--error-bg-iou`` and ``--error-iou``) or background, how many GTs
were missed with and without a detection nearby, the translation / scale / orientation error of the
true positives and the mAP each error type costs, and writes the same numbers to PATH as JSON
(metrics.error_analysis, ivit_det_errors: all samples in one launch; ``--rotated`` picks the IoU).
Without the flag the output is unchanged.
``--ema`` evaluates the averaged weights a ``train_vit.py --ema-decay`` run saved ('ema_state_dict')
instead of the last step's; a checkpoint without them is an error, not a fallback.
``--regrid`` evaluates a checkpoint at ``--grid`` instead of the grid it was trained at: the model is
built at ``--grid`` and the two streams' pos_embed are resampled onto it (bicubic, antialiased:
model_vit.load_state_dict_regrid); everything else loads bit for bit. Without the flag the model has
the checkpoint's ``img_size``, as before.
"""
from __future__ import annotations

import argparse
import os
import time
from pathlib import Path

import numpy as np
import torch

import model_vit
from constants import (ANCHOR_CONFIGS_PAPER, DETECTION_IOU_THRESHOLDS, EVAL_FUSE_BOXES, EVAL_TTA_FLIP,
                       EVAL_USE_ROTATED_IOU, EVAL_USE_ROTATED_NMS, GRID_HEIGHT_PX, GRID_WIDTH_PX, INTENTIONS_MAP_REV, IOU_THRESHOLD_FOR_INTENTION_MATCH,
                       LIDAR_SWEEPS, LIDAR_TOTAL_CHANNELS, MAP_CHANNELS, NUM_INTENTION_CLASSES)
from metrics import detection_map_device as detection_map, intention_matches_device as intention_matches
from model_vit import IntentNetViT
from synthetic import SyntheticBEVLoader
from utils import PostPipeline, flip_bev_batch, generate_anchors

VAL_DATA_DIR = "./data/argoverse2/sensor/val"
MODEL_SAVE_PATH_VIT = "./trained_models_vit/vit_model.pth"

CONFIDENCE_THRESHOLD = 0.1
NMS_IOU_THRESHOLD = 0.2
INFERENCE_BATCH_SIZE = 8
NUM_WORKERS_EVAL = 0


MODEL_SAVE_PATH_CNN = "./trained_models_cnn/cnn_model.pth"  # eval_cnn.py:19


def load_checkpoint(path, device):
    import model_cnn
    torch.serialization.add_safe_globals([model_vit.BasicBlock, model_cnn.BasicBlock])
    return torch.load(path, map_location=device, weights_only=True)


def default_cfg(cfg: dict, grid):
    cfg.setdefault('img_size', tuple(grid))
    cfg.setdefault('lidar_input_channels', LIDAR_TOTAL_CHANNELS)
    cfg.setdefault('map_input_channels', MAP_CHANNELS)
    cfg.setdefault('vit_model_name_lidar', 'vit_small_patch8_224')
    cfg.setdefault('vit_model_name_map', 'vit_tiny_patch8_224')
    cfg.setdefault('pretrained_lidar', False)
    cfg.setdefault('pretrained_map', False)
    cfg.setdefault('drop_path_rate_lidar', 0.1)
    cfg.setdefault('drop_path_rate_map', 0.1)
    cfg.setdefault('lidar_adapter_out_channels', 192)
    cfg.setdefault('map_adapter_out_channels', 128)
    return cfg


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--data-dir", type=str, default=VAL_DATA_DIR, help="Argoverse-2 sensor split to evaluate")
    ap.add_argument("--num-sweeps", type=int, default=LIDAR_SWEEPS, help="LiDAR sweeps per sample (dataset.py:158)")
    ap.add_argument("--checkpoint", type=str, default=None)
    ap.add_argument("--batch", type=int, default=INFERENCE_BATCH_SIZE)
    ap.add_argument("--batches", type=int, default=4, help="synthetic batches")
    ap.add_argument("--grid", type=str, default=f"{GRID_HEIGHT_PX}x{GRID_WIDTH_PX}")
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="fp32")
    ap.add_argument("--rotated", action="store_true", default=EVAL_USE_ROTATED_IOU,
                    help="rotated IoU for mAP / matching (device kernel; no shapely needed)")
    ap.add_argument("--rotated-nms", action="store_true", default=EVAL_USE_ROTATED_NMS,
                    help="suppress on the rotated IoU of the decoded boxes (independent of --rotated)")
    ap.add_argument("--tta-flip", action="store_true", default=EVAL_TTA_FLIP,
                    help="flip test-time augmentation: a second forward on the mirrored rasters, its candidates "
                         "un-mirrored and merged with the first view's before the NMS")
    ap.add_argument("--fuse-boxes", action="store_true", default=EVAL_FUSE_BOXES,
                    help="weighted box fusion: every kept box becomes the score-weighted consensus of the candidates "
                         "it suppressed, its intention their weighted vote (independent of --tta-flip)")
    ap.add_argument("--attn-maps", type=str, default=None, metavar="DIR",
                    help="write the attention maps of each sample's best detections, one .npz per batch (ViT only)")
    ap.add_argument("--attn-top", type=int, default=8, help="detections per sample (highest score after NMS)")
    ap.add_argument("--attn-blocks", type=str, default="-1",
                    help="comma list of ViT block indices, negative from the end")
    ap.add_argument("--error-report", type=str, default=None, metavar="PATH",
                    help="write the detection error breakdown (metrics.error_analysis) as JSON and print its table")
    ap.add_argument("--error-iou", type=float, default=IOU_THRESHOLD_FOR_INTENTION_MATCH,
                    help="IoU a detection needs to count in the error breakdown")
    ap.add_argument("--error-bg-iou", type=float, default=0.1,
                    help="best IoU below which a detection is background, not a localisation error")
    ap.add_argument("--error-range-edges", type=str, default="20,40,60",
                    help="comma list of range-bin edges in metres from the ego vehicle (ascending, at most 7)")
    ap.add_argument("--ema", action="store_true",
                    help="load the checkpoint's 'ema_state_dict' (train_vit.py --ema-decay) instead of 'model_state_dict'")
    ap.add_argument("--regrid", action="store_true",
                    help="build the model at --grid instead of the checkpoint's img_size and resample the streams' "
                         "pos_embed onto it (ViT only)")
    from train_vit import add_window_args, window_args
    add_window_args(ap)
    args = ap.parse_args(argv)
    args.window_size, args.global_attn_indexes = window_args(ap, args, blocks_alone=True)
    return args


class AttnDump:
    """``--attn-maps``: for every sample of a batch, the ``top`` highest-scoring detections after NMS
    -> the head-mean attention maps of both ViT streams at ``blocks`` for the token under each box
    centre (IntentNetViT.attention_maps), written to ``out_dir/attn_batch_<k>.npz``:
      lidar, map [L, R, Hf, Wf]; lidar_cls, map_cls [L, R]; lidar_cells, map_cells [R, 2] (gy, gx);
      boxes_xywha [R, 5]; scores [R]; sample [R] (index inside the batch); blocks [L].
    R = the batch's chosen detections, sample-major, best first."""

    def __init__(self, out_dir, top=8, blocks=(-1,)):
        self.out_dir, self.top, self.blocks = str(out_dir), int(top), tuple(int(b) for b in blocks)
        if self.top < 1:
            raise ValueError("--attn-top must be at least 1")
        os.makedirs(self.out_dir, exist_ok=True)
        self.written = 0

    def __call__(self, model, lidar_bev, map_bev, preds):
        sample, boxes, scores = [], [], []
        for b, p in enumerate(preds):
            sc = p["pred_scores"].float().cpu()
            top = torch.topk(sc, min(self.top, sc.numel())).indices
            sample.append(torch.full((top.numel(),), b, dtype=torch.long))
            boxes.append(p["pred_boxes_xywha"].float().cpu()[top].reshape(-1, 5))
            scores.append(sc[top])
        sample, boxes, scores = torch.cat(sample), torch.cat(boxes), torch.cat(scores)
        maps = model.attention_maps(lidar_bev, map_bev, sample, boxes[:, :2], blocks=self.blocks, head_mean=True)
        path = os.path.join(self.out_dir, f"attn_batch_{self.written:05d}.npz")
        np.savez(path, **{k: v.cpu().numpy() for k, v in maps.items()}, boxes_xywha=boxes.numpy(),
                 scores=scores.numpy(), sample=sample.numpy(), blocks=np.asarray(self.blocks, dtype=np.int64))
        self.written += 1
        return path


def run_inference(model, loader, anchors, conf=CONFIDENCE_THRESHOLD, nms=NMS_IOU_THRESHOLD, rotated_nms=False,
                  attn_dump=None, tta_flip=False, fuse_boxes=False):
    """eval_vit.py:136-180: forward + post-processing per batch, in loader order. The
    post-processing of a batch (utils.PostPipeline) runs beside the next batch's forward; results
    are the per-batch postprocess_batch ones, appended in the same order. ``rotated_nms``: the
    NMS suppresses on the rotated IoU (utils.apply_nms(rotated=True)). ``attn_dump`` (AttnDump):
    a batch's inputs are kept until its detections arrive (one batch late), then its attention
    maps are computed and written; the results are the same with and without it.
    ``tta_flip``: every batch is also run mirrored (utils.flip_bev_batch) and both views' candidates
    go through one NMS; ``fuse_boxes``: the kept boxes are fused with what they suppressed
    (utils.postprocess_batch). With either, the results gain 'pred_members'."""
    results = []
    tta_kw = {k: True for k, v in (("tta_flip", tta_flip), ("fuse_boxes", fuse_boxes)) if v}
    pipe = PostPipeline(anchors, conf, nms, rotated_nms=rotated_nms, **tta_kw)
    gts = []
    held = []  # attn_dump: the (lidar, map) rasters of the batches whose detections are still pending

    def emit(preds):
        if attn_dump is not None:
            attn_dump(model, *held.pop(0), preds)
        for p, gt in zip(preds, gts.pop(0)):
            results.append({**{k: v.cpu() for k, v in p.items()},
                            "gt_boxes_xywha": gt.get("boxes_xywha", torch.empty((0, 5))),
                            "gt_intentions": gt.get("intentions", torch.empty(0, dtype=torch.long))})

    with torch.inference_mode():
        for batch in loader:
            dev = anchors.device
            lidar, mp = batch["lidar_bev"].to(dev, non_blocking=True), batch["map_bev"].to(dev, non_blocking=True)
            cls, box, it = model(lidar, mp)
            gts.append(batch["gt_list"])
            if attn_dump is not None:
                held.append((lidar, mp))
            if tta_flip:
                prev = pipe.push(cls, box, it, tta_logits=model(*flip_bev_batch(lidar, mp)))
            else:
                prev = pipe.push(cls, box, it)
            if prev is not None:
                emit(prev)
        last = pipe.flush()
        if last is not None:
            emit(last)
    return results


def main_eval_vit(argv=None, variant="vit"):
    """variant "vit" (eval_vit.py) or "cnn" (eval_cnn.py: IntentNetCNN, stride 8)."""
    args = parse_args(argv)
    tag = "ViT" if variant == "vit" else "CNN"
    if args.attn_maps is not None and variant != "vit":
        raise SystemExit("--attn-maps: IntentNetCNN has no attention to map (use eval_vit.py)")
    if args.regrid and variant != "vit":
        raise SystemExit("--regrid: IntentNetCNN has no position embedding tied to a grid (use eval_vit.py)")
    if args.window_size is not None and variant != "vit":
        raise SystemExit("--window: IntentNetCNN has no attention to window (use eval_vit.py)")
    if args.checkpoint is None:
        args.checkpoint = MODEL_SAVE_PATH_VIT if variant == "vit" else MODEL_SAVE_PATH_CNN
    if not torch.cuda.is_available():
        raise RuntimeError("eval_vit.py runs on the MI355X kernels: no ROCm GPU visible")
    device = torch.device("cuda")
    H, W = (int(v) for v in args.grid.lower().split("x"))
    print(f"--- {tag} Model Evaluation ---")
    print(f"Torch version: {torch.__version__}, device: {torch.cuda.get_device_name(0)}")
    print(f"Evaluation using Rotated IoU for mAP/matching: {args.rotated}")
    print(f"Evaluation using Rotated NMS: {args.rotated_nms}")
    if args.tta_flip or args.fuse_boxes:
        print(f"Evaluation using flip TTA: {args.tta_flip}, weighted box fusion: {args.fuse_boxes}")

    ckpt = None
    if Path(args.checkpoint).is_file():
        print(f"\nLoading TRAINED {tag} Model from: {args.checkpoint}")
        ckpt = load_checkpoint(args.checkpoint, device)
        cfg = ckpt.get('backbone_cfg')
        if not cfg:
            print(f"ERROR: 'backbone_cfg' not found in {tag} checkpoint.")
            return 1
    elif args.synthetic:
        print(f"No checkpoint at {args.checkpoint}: random-init weights (synthetic run)")
        from train_vit import backbone_cfg, cnn_backbone_cfg
        cfg = backbone_cfg((H, W)) if variant == "vit" else cnn_backbone_cfg()
    else:
        print(f"ERROR: {tag} Model checkpoint not found at {args.checkpoint}")
        return 1
    if variant == "vit":
        cfg = default_cfg(dict(cfg), (H, W))
        # the flags override what the checkpoint says: --window its window (the global blocks then follow
        # --global-blocks, or the default rule), --global-blocks alone the global blocks of its window
        if args.window_size is not None:
            cfg['vit_window_size'] = args.window_size
            cfg['vit_global_attn_indexes'] = args.global_attn_indexes
        elif args.global_attn_indexes is not None:
            if cfg.get('vit_window_size') is None:
                raise SystemExit("--global-blocks: the checkpoint has no window to keep blocks out of (add --window)")
            cfg['vit_global_attn_indexes'] = args.global_attn_indexes
        src_img_size = tuple(cfg['img_size'])
        if args.regrid:
            cfg['img_size'] = (H, W)
        model = IntentNetViT(backbone_cfg=cfg).to(device)
        if cfg.get('vit_window_size') is not None:
            from train_vit import window_line
            print(window_line(model))
        img_size = tuple(cfg['img_size'])
    else:
        from model_cnn import IntentNetCNN
        model = IntentNetCNN(backbone_cfg=dict(cfg)).to(device)
        img_size = (H, W)
    if args.ema:
        if ckpt is None or 'ema_state_dict' not in ckpt:
            print(f"ERROR: --ema: no 'ema_state_dict' in {args.checkpoint} (train with --ema-decay to save one).")
            return 1
        print(f"Evaluating the EMA weights ('ema_state_dict', decay {ckpt.get('ema_decay')}, "
              f"warmup {ckpt.get('ema_warmup')})")
        weights = ckpt['ema_state_dict']
    else:
        weights = ckpt['model_state_dict'] if ckpt is not None else None
    if weights is not None and args.regrid:
        done = model_vit.load_state_dict_regrid(model, weights, src_img_size)
        for key, (old, new) in done.items():
            print(f"--regrid: {key} {old[0]}x{old[1]} -> {new[0]}x{new[1]}")
    elif weights is not None:
        model.load_state_dict(weights)
    model.set_compute_dtype(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    model.eval()

    if args.synthetic:
        loader = SyntheticBEVLoader(args.batch, args.batches, img_size, rank=0, device=device,
                                    resident=False)
    else:
        if not Path(args.data_dir).is_dir():
            print(f"ERROR: Evaluation data directory not found: {args.data_dir} (use --synthetic)")
            return 1
        if (H, W) != (GRID_HEIGHT_PX, GRID_WIDTH_PX) or tuple(img_size) != (GRID_HEIGHT_PX, GRID_WIDTH_PX):
            raise SystemExit(f"--grid {args.grid} / checkpoint img_size {tuple(img_size)}: Argoverse-2 rasters have "
                             f"the constants.py grid {GRID_HEIGHT_PX}x{GRID_WIDTH_PX}; other grids need --synthetic")
        from dataset import ArgoverseIntentNetDataset, FrameBatchLoader  # pandas / pyarrow only in this mode
        val_set = ArgoverseIntentNetDataset(args.data_dir, num_sweeps=args.num_sweeps, is_train=False, device=device)
        loader = FrameBatchLoader(val_set, args.batch, shuffle=False, device=device)

    if variant == "vit":
        stride = int(cfg.get('vit_model_name_lidar', 'vit_small_patch8_224').split('_patch')[-1].split('_')[0]) \
            * cfg.get('fusion_block_stride', 1)
    else:
        stride = 8  # eval_cnn.py: FEATURE_MAP_STRIDE_CNN
    Hc, Wc = img_size
    anchors = generate_anchors(Hc, Wc, stride, ANCHOR_CONFIGS_PAPER, device=device)
    print(f"Anchors for {tag} evaluation generated (stride {stride}), shape: {tuple(anchors.shape)}")

    t0 = time.perf_counter()
    dump = None
    if args.attn_maps is not None:
        dump = AttnDump(args.attn_maps, args.attn_top, [int(b) for b in args.attn_blocks.split(",") if b.strip()])
    results = run_inference(model, loader, anchors, rotated_nms=args.rotated_nms, attn_dump=dump,
                            tta_flip=args.tta_flip, fuse_boxes=args.fuse_boxes)
    torch.cuda.synchronize()
    if dump is not None:
        print(f"Attention maps of {dump.written} batches written to {dump.out_dir}")
    dt = time.perf_counter() - t0
    print(f"Collected results for {len(results)} samples ({len(results) / dt:.2f} samples/s incl. host transfer)")

    print(f"\n--- {tag} Detection Results (mAP) ---")
    maps = detection_map(results, DETECTION_IOU_THRESHOLDS, args.rotated)
    for t, v in maps.items():
        print(f"{tag} mAP @ IoU={t:.1f}: {v:.4f}")

    mp, mg = intention_matches(results, IOU_THRESHOLD_FOR_INTENTION_MATCH, args.rotated)
    if mp:
        from sklearn.metrics import accuracy_score, f1_score
        labels = list(range(NUM_INTENTION_CLASSES))
        print(f"\n--- {tag} Intention Prediction Results (on TP detections @ IoU>={IOU_THRESHOLD_FOR_INTENTION_MATCH}) ---")
        print(f"{tag} Overall Accuracy: {accuracy_score(mg, mp):.4f}")
        print(f"{tag} F1 (Macro):   {f1_score(mg, mp, labels=labels, average='macro', zero_division=0):.4f}")
        print(f"{tag} F1 (Weighted): {f1_score(mg, mp, labels=labels, average='weighted', zero_division=0):.4f}")
        per = f1_score(mg, mp, labels=labels, average=None, zero_division=0)
        print(f"{tag} F1 (Per Class):")
        for i in labels:
            print(f"  {INTENTIONS_MAP_REV.get(i, f'Class_{i}'):<20}: {per[i]:.4f}")
    else:
        print(f"\nNo True Positive detections found for {tag} model at IoU >= {IOU_THRESHOLD_FOR_INTENTION_MATCH} "
              "to evaluate intention.")
    if args.error_report is not None:
        from metrics import error_analysis, error_report_json, format_error_report
        edges = [float(e) for e in args.error_range_edges.split(",") if e.strip()]
        report = error_analysis(results, args.error_iou, args.error_bg_iou, args.rotated, edges)
        print(f"\n--- {tag} Detection Error Breakdown ---")
        print(format_error_report(report))
        with open(args.error_report, "w") as f:
            f.write(error_report_json(report) + "\n")
        print(f"Error report written to {args.error_report}")
    print(f"\n--- Evaluation Script for {tag} Finished ---")
    return 0


if __name__ == '__main__':
    raise SystemExit(main_eval_vit())
