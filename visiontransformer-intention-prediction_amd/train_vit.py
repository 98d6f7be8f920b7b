"""IntentNetViT training entry point — the flow of the reference's train_vit.py:15-211 on the
MI355X kernels.

Same module-level configuration, same model/loss/optimizer/scheduler/anchor construction, the
same per-batch NaN skips and the same checkpoint dict ({'epoch', 'model_state_dict',
'optimizer_state_dict', 'backbone_cfg'}). Differences, all outside the numerics:

* ``--synthetic`` feeds seeded synthetic BEV batches of the constants.py grid (synthetic.py);
  without it the script trains on the Argoverse-2 logs under ``--data-dir`` (TRAIN_DATA_DIR by
  default, and the reference's stop when it is missing): dataset.ArgoverseIntentNetDataset and
  a FrameBatchLoader build every batch's rasters on the GPU (``--augment`` included), rank r
  takes every world-th sequence; real rasters have the constants.py grid, so another ``--grid``
  is refused; the logs need annotations_with_intent.feather (preprocess_intent_labels.py);
* data parallel: run under ``torchrun --nproc-per-node N`` — one process per GPU, gradients
  all-reduced over RCCL in buckets overlapped with backward (ddp.py); rank r draws synthetic
  shard 1234 + r; only rank 0 prints and saves;
* the optimizer is FusedAdamW (same AdamW update, one launch per step); ``--dtype bf16`` runs
  the kernels in bf16 with f32 master weights, ``fp32`` is the parity setting;
* ``--clip-grad-norm X`` bounds the global gradient norm (trainer.Trainer ``max_grad_norm``); the
  epoch line then reports the mean and max norm and the clipped / skipped steps (one host read);
* ``--ema-decay D`` keeps an exponential moving average of the weights in the optimiser's launch
  (optim.ModelEMA, trainer.Trainer ``ema``; ``--ema-no-warmup`` drops the (1 + n) / (10 + n) ramp); the
  checkpoint then also holds 'ema_state_dict' (the model's state dict with the averaged parameters),
  'ema_decay' and 'ema_warmup', which ``eval_vit.py --ema`` evaluates. Off by default;
* ``--pretrained-lidar PATH`` / ``--pretrained-map PATH`` initialise a stream's ViT from a timm checkpoint
  (vit.VisionTransformer.load_pretrained: pos_embed resampled onto ``--grid``, the 3-channel patch weights
  adapted to the stream's channels); the saved 'backbone_cfg' keeps ``pretrained_*: False``, so the
  checkpoint stays self-contained. ``--init-from CKPT`` starts from the weights of one of this script's
  checkpoints, trained at the same or another grid (model_vit.load_state_dict_regrid);
* ``--layer-decay D`` / ``--no-decay-1d`` build the fine-tuning parameter groups of
  optim.layer_decay_param_groups (lr scaled by D per ViT layer below the top; no weight decay on 1-D
  parameters, biases, ``pos_embed`` and ``cls_token``) and update them all in ONE launch
  (``FusedAdamW(fuse_groups=True)``); ``--sched cosine`` replaces ReduceLROnPlateau by optim.WarmupCosineLR,
  stepped per update (``--warmup-epochs``, ``--min-lr``), and the checkpoint gains 'lr_schedule_state_dict';
  ``--lr`` / ``--weight-decay`` set the base values. All off by default: one group, plateau schedule;
* the reference's import-time defects (train_vit.py:34-35 undefined LIDAR_TOTAL_CHANNELS /
  MAP_CHANNELS, :131 ``verbose``) are fixed without changing any value.
"""
from __future__ import annotations

import argparse
import time
from pathlib import Path

import torch

from constants import (ANCHOR_CONFIGS_PAPER, BOX_IOU_LOSS_WEIGHT, DOMINANT_CLASSES_FOR_DOWNSAMPLING, GRAD_CLIP_NORM,
                       GRID_HEIGHT_PX, GRID_WIDTH_PX, INTENTION_DOWNSAMPLE_RATIO, LIDAR_SWEEPS, LIDAR_TOTAL_CHANNELS,
                       MAP_CHANNELS)
from ddp import all_reduce_sum, any_rank, init_distributed
from loss import DetectionIntentionLoss
from model_vit import BasicBlock, IntentNetViT
from optim import FusedAdamW, ModelEMA, WarmupCosineLR, group_summary, layer_decay_param_groups
from synthetic import SyntheticBEVLoader
from trainer import Trainer
from utils import generate_anchors

TRAIN_DATA_DIR = "./data/argoverse2/sensor/train"
MODEL_SAVE_DIR_VIT = "./trained_models_vit"

TRAIN_BATCH_SIZE = 8
NUM_WORKERS = 0
LEARNING_RATE = 1e-4
WEIGHT_DECAY = 1e-4
NUM_EPOCHS = 10

USE_ROTATED_IOU = False
APPLY_INTENTION_DOWNSAMPLING = True
USE_INTENTION_WEIGHTS = False


def parse_window(text):
    """'HxW' (or one number for a square window) -> (wh, ww); ValueError for anything else or a
    window outside 1 .. 256 tokens."""
    parts = str(text).lower().split("x")
    try:
        vals = [int(v) for v in parts]
    except ValueError:
        raise ValueError(f"--window {text!r}: expected HxW, e.g. 10x10") from None
    if len(vals) == 1:
        vals = vals * 2
    if len(vals) != 2 or min(vals) < 1 or vals[0] * vals[1] > 256:
        raise ValueError(f"--window {text!r}: expected HxW with 1 <= H*W <= 256")
    return vals[0], vals[1]


def parse_global_blocks(text):
    """'i,j,...' -> a tuple of block indices (negative from the end); ValueError otherwise."""
    try:
        vals = tuple(int(v) for v in str(text).split(",") if v.strip() != "")
    except ValueError:
        raise ValueError(f"--global-blocks {text!r}: expected a comma list of block indices") from None
    if not vals:
        raise ValueError(f"--global-blocks {text!r}: names no block")
    return vals


def add_window_args(ap):
    ap.add_argument("--window", type=str, default=None, metavar="HxW",
                    help="windowed attention in the ViT streams: attention inside windows of H x W patches in every "
                         "block but the global ones (ViT only; no parameter changes)")
    ap.add_argument("--global-blocks", type=str, default=None, metavar="I,J,...",
                    help="with --window: the blocks that keep global attention (default: the last block of each of "
                         "four equal groups, 2,5,8,11 at depth 12)")


def window_args(ap, args, blocks_alone=False):
    """-> (window or None, global blocks or None) of the parsed flags; ap.error on bad values.
    blocks_alone: --global-blocks without --window is allowed (eval_vit.py: the window then comes from
    the checkpoint)."""
    try:
        win = parse_window(args.window) if args.window is not None else None
        glob = parse_global_blocks(args.global_blocks) if args.global_blocks is not None else None
    except ValueError as e:
        ap.error(str(e))
    if glob is not None and win is None and not blocks_alone:
        ap.error("--global-blocks needs --window")
    return win, glob


def window_line(model):
    """One log line: the window, the global blocks and the windows per stream."""
    vl = model.backbone.vit_lidar
    wh, ww = vl.window_size
    gh, gw = vl.patch_embed.grid_size
    nwin = -(-gh // wh) * -(-gw // ww)
    return (f"Windowed attention: {wh}x{ww} patches, global blocks {list(vl.global_attn_indexes)}, "
            f"{nwin} windows per stream on the {gh}x{gw} grid (+ CLS alone)")


def backbone_cfg(img_size=(GRID_HEIGHT_PX, GRID_WIDTH_PX), window=None, global_blocks=None):
    """``window`` / ``global_blocks``: vit_window_size / vit_global_attn_indexes, present in the
    dict only when a window is set."""
    win = {}
    if window is not None:
        win['vit_window_size'] = tuple(window)
        win['vit_global_attn_indexes'] = None if global_blocks is None else tuple(global_blocks)
    return {
        'lidar_input_channels': LIDAR_TOTAL_CHANNELS,
        'map_input_channels': MAP_CHANNELS,
        'vit_model_name_lidar': 'vit_small_patch8_224',
        'vit_model_name_map': 'vit_small_patch8_224',
        'pretrained_lidar': False,
        'pretrained_map': False,
        'img_size': tuple(img_size),
        'drop_path_rate_lidar': 0.1,
        'drop_path_rate_map': 0.1,
        'lidar_adapter_out_channels': 192,
        'map_adapter_out_channels': 192,
        'fusion_block_planes': 512,
        'fusion_block_layers': 2,
        'fusion_block_kernel_size': 3,
        'fusion_block_stride': 1,
        'res_block_type': BasicBlock,
        **win,
    }


MODEL_SAVE_DIR_CNN = "./trained_models_cnn"
FEATURE_MAP_STRIDE_CNN = 8  # train_cnn.py:42


def cnn_backbone_cfg():
    """train_cnn.py:32-40 (CNN_BACKBONE_CFG)."""
    from model_cnn import BasicBlock as CNNBlock
    return {'block': CNNBlock, 'lidar_input_channels': LIDAR_TOTAL_CHANNELS, 'map_input_channels': MAP_CHANNELS,
            'lidar_s1_planes': 160, 'lidar_s2_planes': 192, 'lidar_s3_planes': 224,
            'map_s1_planes': 32, 'map_s2_planes': 64, 'map_s3_planes': 96,
            'fusion_block_planes': 512, 'fusion_block_layers': 2, 'num_blocks_per_stage': 2,
            'res_block2_kernel_size': 5, 'fusion_block_kernel_size': 3}


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--synthetic", action="store_true", help="seeded synthetic BEV batches instead of TRAIN_DATA_DIR")
    ap.add_argument("--data-dir", type=str, default=TRAIN_DATA_DIR, help="Argoverse-2 sensor split to train on")
    ap.add_argument("--num-sweeps", type=int, default=LIDAR_SWEEPS, help="LiDAR sweeps per sample (dataset.py:158)")
    ap.add_argument("--epochs", type=int, default=NUM_EPOCHS)
    ap.add_argument("--batches-per-epoch", type=int, default=16, help="synthetic batches per epoch")
    ap.add_argument("--batch", type=int, default=TRAIN_BATCH_SIZE, help="per-GPU batch")
    ap.add_argument("--grid", type=str, default=f"{GRID_HEIGHT_PX}x{GRID_WIDTH_PX}")
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--bucket-mb", type=float, default=64.0)
    ap.add_argument("--save-dir", type=str, default=None)
    ap.add_argument("--no-save", action="store_true")
    ap.add_argument("--fresh-batches", action="store_true", help="draw a new synthetic batch every step")
    ap.add_argument("--augment", action="store_true",
                    help="training-time augment_bev on every batch (dataset.py:352-353), on the GPU")
    ap.add_argument("--clip-grad-norm", type=float, default=GRAD_CLIP_NORM, metavar="X",
                    help="clip the global gradient L2 norm to X on the device (no host sync); a non-finite "
                         "gradient norm skips the update")
    ap.add_argument("--iou-loss-weight", type=float, default=BOX_IOU_LOSS_WEIGHT, metavar="X",
                    help="add X * (1 - rotated IoU of the decoded box and its matched GT) per positive anchor to the "
                         "Smooth-L1 sum of the box loss (0: off)")
    ap.add_argument("--ema-decay", type=float, default=None, metavar="D",
                    help="keep an exponential moving average of the weights with decay D in [0, 1) (updated in the "
                         "optimiser's launch) and save it as 'ema_state_dict'")
    ap.add_argument("--ema-no-warmup", action="store_true",
                    help="with --ema-decay: use D from the first step, without the min(D, (1 + n) / (10 + n)) ramp")
    ap.add_argument("--pretrained-lidar", type=str, default=None, metavar="PATH",
                    help="timm weights (.pth / .bin / .safetensors) of the LiDAR stream's ViT: pos_embed resampled "
                         "to --grid, the 3-channel patch weights adapted to the LiDAR channels (ViT only)")
    ap.add_argument("--pretrained-map", type=str, default=None, metavar="PATH",
                    help="the same for the map stream's ViT")
    ap.add_argument("--init-from", type=str, default=None, metavar="CKPT",
                    help="start from the 'model_state_dict' of one of this script's checkpoints, trained at the "
                         "same or another --grid (pos_embed resampled); its optimizer state is not taken")
    ap.add_argument("--lr", type=float, default=LEARNING_RATE, metavar="X", help="base learning rate")
    ap.add_argument("--weight-decay", type=float, default=WEIGHT_DECAY, metavar="X")
    ap.add_argument("--layer-decay", type=float, default=None, metavar="D",
                    help="layer-wise lr decay in (0, 1]: a ViT stream's block i trains at lr * D ** (depth - i), its "
                         "patch/pos/cls embeddings at lr * D ** (depth + 1); neck, heads (and all of the CNN) at lr")
    ap.add_argument("--no-decay-1d", action="store_true",
                    help="no weight decay on 1-D parameters (norm scales), biases, pos_embed and cls_token")
    ap.add_argument("--sched", choices=["plateau", "cosine"], default="plateau",
                    help="plateau: ReduceLROnPlateau on the epoch loss; cosine: linear warmup then cosine decay to "
                         "--min-lr over --epochs, stepped every update")
    ap.add_argument("--warmup-epochs", type=float, default=0.0, metavar="E", help="with --sched cosine")
    ap.add_argument("--min-lr", type=float, default=0.0, metavar="X", help="with --sched cosine")
    add_window_args(ap)
    args = ap.parse_args(argv)
    args.window_size, args.global_attn_indexes = window_args(ap, args)
    if not 0.0 <= args.iou_loss_weight < float("inf"):
        ap.error(f"--iou-loss-weight {args.iou_loss_weight}: must be a finite number >= 0")
    if args.layer_decay is not None and not 0.0 < args.layer_decay <= 1.0:
        ap.error(f"--layer-decay {args.layer_decay}: must be in (0, 1]")
    if args.sched == "cosine":
        if args.epochs <= 0:
            ap.error("--sched cosine: the schedule spans --epochs x batches per epoch updates; --epochs must be > 0")
        if not 0.0 <= args.warmup_epochs <= args.epochs:
            ap.error(f"--warmup-epochs {args.warmup_epochs:g}: must lie in [0, --epochs]")
    return args


def param_groups_requested(args):
    """Whether the flags ask for the fine-tuning groups (else: one group, as the reference builds it)."""
    return args.layer_decay is not None or args.no_decay_1d


def build_optimizer(model, args, log=print):
    """FusedAdamW as the flags ask: by default the reference's single group; with --layer-decay /
    --no-decay-1d the groups of optim.layer_decay_param_groups, fused into one launch."""
    if not param_groups_requested(args):
        return FusedAdamW(model.parameters(), lr=args.lr, weight_decay=args.weight_decay)
    groups = layer_decay_param_groups(model, 1.0 if args.layer_decay is None else args.layer_decay, args.weight_decay,
                                      no_decay_1d=args.no_decay_1d)
    log(f"Parameter groups: {len(groups)} (layer decay {args.layer_decay}, no decay on 1-D: {args.no_decay_1d}), "
        f"one fused AdamW launch")
    for lid, scale, tensors, elems in group_summary(groups):
        log(f"  layer {lid:2d}: lr scale {scale:.6f}, {tensors} tensors, {elems} elements")
    return FusedAdamW(groups, lr=args.lr, weight_decay=args.weight_decay, fuse_groups=True)


def build_schedule(optimizer, args, steps_per_epoch):
    """WarmupCosineLR over --epochs x steps_per_epoch updates for --sched cosine, else None."""
    if args.sched != "cosine":
        return None
    total = args.epochs * int(steps_per_epoch or 0)
    if total <= 0:
        raise SystemExit(f"--sched cosine: no updates to schedule ({args.epochs} epoch(s) x {steps_per_epoch} batch(es) "
                         f"per epoch); the schedule needs the total from --epochs and the loader's length")
    return WarmupCosineLR(optimizer, int(round(args.warmup_epochs * steps_per_epoch)), total, min_lr=args.min_lr)


def _grid_str(g):
    return f"{g[0]}x{g[1]}"


def load_initial_weights(model, args, variant, device, log):
    """--init-from, then --pretrained-lidar / --pretrained-map, on the freshly built model (before the
    optimizer, the EMA and the Trainer exist: a resampled pos_embed replaces nothing they hold). Every
    rank reads the same files, so the replicas start identical. One log line per load."""
    if args.init_from is not None:
        from eval_vit import load_checkpoint
        from model_vit import load_state_dict_regrid
        ckpt = load_checkpoint(args.init_from, device)
        src = tuple((ckpt.get('backbone_cfg') or {}).get('img_size', (0, 0)))
        if variant == "vit" and src == (0, 0):
            raise SystemExit(f"--init-from {args.init_from}: no backbone_cfg['img_size'] in the checkpoint")
        done = load_state_dict_regrid(model, ckpt['model_state_dict'], src)
        what = ", ".join(f"{k.split('.')[1]} pos_embed {_grid_str(o)} -> {_grid_str(n)}" for k, (o, n) in done.items())
        log(f"Initialised from {args.init_from} (model_state_dict; {what or 'same grid, loaded as saved'})")
    for name, path in (("vit_lidar", args.pretrained_lidar), ("vit_map", args.pretrained_map)):
        if path is None:
            continue
        info = getattr(model.backbone, name).load_pretrained(path)
        og, ch = info["old_grid"], info["in_chans"]
        log(f"Pretrained {name} from {path}: pos_embed "
            + (f"{_grid_str(og)} -> {_grid_str(info['new_grid'])}" if og else f"{_grid_str(info['new_grid'])} as saved")
            + (f", patch weights {ch[0]} -> {ch[1]} channels" if ch else ", patch weights as saved"))


def grad_clip_line(st, max_norm):
    """The epoch's gradient-norm report from Trainer.grad_stats() (the norms are the same on every rank)."""
    ok = st["steps"] - st["nonfinite"]
    mean = st["norm_sum"] / ok if ok > 0 else float("nan")
    return (f"  Grad norm (clip {max_norm:g}): mean {mean:.4g}, max {st['norm_max']:.4g}, "
            f"clipped {int(st['clipped'])}/{int(st['steps'])} steps, skipped {int(st['nonfinite'])} (non-finite)")


def _in_lockstep(loader, device):
    """The loader's batches until ANY rank has run out: a rank's shard may hold one sequence fewer,
    or more samples the dataset gives up on, and every rank must take the same number of steps
    (the gradient all-reduce pairs them). A plain pass-through on one rank."""
    it = iter(loader)
    while True:
        batch = next(it, None)
        if any_rank(batch is None, device):
            return
        yield batch


def main(argv=None, variant="vit"):
    """variant "vit" (train_vit.py) or "cnn" (train_cnn.py: IntentNetCNN, stride 8)."""
    args = parse_args(argv)
    tag = "ViT" if variant == "vit" else "CNN"
    if args.save_dir is None:
        args.save_dir = MODEL_SAVE_DIR_VIT if variant == "vit" else MODEL_SAVE_DIR_CNN
    if variant != "vit" and (args.pretrained_lidar is not None or args.pretrained_map is not None):
        raise SystemExit("--pretrained-lidar / --pretrained-map: IntentNetCNN has no ViT stream to load timm weights "
                         "into (use train_vit.py; --init-from works for both)")
    if variant != "vit" and args.window_size is not None:
        raise SystemExit("--window: IntentNetCNN has no attention to window (use train_vit.py)")
    rank, local, world, device = init_distributed()
    if device.type != "cuda":
        raise RuntimeError("train_vit.py runs on the MI355X kernels: no ROCm GPU visible")
    H, W = (int(v) for v in args.grid.lower().split("x"))
    if variant == "vit":
        cfg = backbone_cfg((H, W), args.window_size, args.global_attn_indexes)
        stride = int(cfg['vit_model_name_lidar'].split('_patch')[-1].split('_')[0]) * cfg.get('fusion_block_stride', 1)
    else:
        cfg, stride = cnn_backbone_cfg(), FEATURE_MAP_STRIDE_CNN
    log = print if rank == 0 else (lambda *a, **k: None)

    log(f"--- {tag} Training Configuration ---")
    log(f"Device: {device} x {world} rank(s)")
    log(f"Training data: {'synthetic' if args.synthetic else args.data_dir}")
    log(f"BEV Image Size for {tag}: {(H, W)}")
    log(f"Using Rotated IoU: {USE_ROTATED_IOU}")
    log(f"Batch Size: {args.batch}/GPU (global {args.batch * world}), Num Epochs: {args.epochs}, LR: {args.lr}")
    log(f"Feature Map Stride ({tag}): {stride}")
    log(f"Apply Intention Downsampling: {APPLY_INTENTION_DOWNSAMPLING}")
    log(f"Compute dtype: {args.dtype}")
    log("---------------------------------")

    if args.synthetic:
        loader = SyntheticBEVLoader(args.batch, args.batches_per_epoch, (H, W), rank=rank, device=device,
                                    resident=not args.fresh_batches, augment=args.augment)
    else:
        if not Path(args.data_dir).is_dir():
            log(f"ERROR: Training data directory not found: {args.data_dir} (use --synthetic)")
            return 1
        if (H, W) != (GRID_HEIGHT_PX, GRID_WIDTH_PX):
            raise SystemExit(f"--grid {args.grid}: Argoverse-2 rasters have the constants.py grid "
                             f"{GRID_HEIGHT_PX}x{GRID_WIDTH_PX}; other grids need --synthetic")
        from dataset import ArgoverseIntentNetDataset, FrameBatchLoader  # pandas / pyarrow only in this mode
        train_set = ArgoverseIntentNetDataset(args.data_dir, num_sweeps=args.num_sweeps, is_train=True, device=device)
        loader = FrameBatchLoader(train_set, args.batch, shuffle=True, rank=rank, world=world, augment=args.augment,
                                  device=device)

    if USE_INTENTION_WEIGHTS and APPLY_INTENTION_DOWNSAMPLING:
        log("Warning: Both USE_INTENTION_WEIGHTS and APPLY_INTENTION_DOWNSAMPLING are True. "
            "Downsampling will be applied; explicit weights will be ignored by the loss function.")

    if variant == "vit":
        model = IntentNetViT(backbone_cfg=cfg).to(device)
        if args.window_size is not None:
            log(window_line(model))
    else:
        from model_cnn import IntentNetCNN
        model = IntentNetCNN(backbone_cfg=cfg).to(device)
    load_initial_weights(model, args, variant, device, log)
    model.set_compute_dtype(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    loss_fn = DetectionIntentionLoss(use_rotated_iou=USE_ROTATED_IOU, intention_class_weights=None,
                                     apply_intention_downsampling=APPLY_INTENTION_DOWNSAMPLING,
                                     dominant_intentions=DOMINANT_CLASSES_FOR_DOWNSAMPLING,
                                     intention_downsample_ratio=INTENTION_DOWNSAMPLE_RATIO,
                                     iou_loss_weight=args.iou_loss_weight).to(device)
    if args.iou_loss_weight > 0:
        log(f"Box loss: Smooth-L1 + {args.iou_loss_weight:g} x (1 - rotated IoU) per positive anchor")
    optimizer = build_optimizer(model, args, log)
    # every rank's loader has the same length in lockstep mode or a shorter one ends the epoch for all:
    # the schedule then simply reaches fewer updates than it spans
    lr_sched = build_schedule(optimizer, args, len(loader))
    scheduler = None
    if lr_sched is None:
        scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, mode='min', factor=0.1, patience=3)
    else:
        log(f"LR schedule: {lr_sched.warmup_steps} warmup + cosine over {lr_sched.total_steps} updates, "
            f"min lr {args.min_lr:g}")
    anchors = generate_anchors(H, W, stride, ANCHOR_CONFIGS_PAPER, device=device)
    log(f"Anchors generated (stride {stride}), shape: {tuple(anchors.shape)}")
    ema = None
    if args.ema_decay is not None:
        ema = ModelEMA(model, decay=args.ema_decay, warmup=not args.ema_no_warmup)
        log(f"Weight EMA: decay {ema.decay:g}, warmup {ema.warmup}")
    trainer = Trainer(model, loss_fn, optimizer, anchors, world=world, bucket_mb=args.bucket_mb, check_nan=True,
                      max_grad_norm=args.clip_grad_norm, ema=ema)

    log(f"\n--- Starting {tag} Training ---")
    for epoch in range(args.epochs):
        model.train()
        iou_on = args.iou_loss_weight > 0
        acc = torch.zeros(6 if iou_on else 4, dtype=torch.float64, device=device)
        n_ok = 0
        t0 = time.perf_counter()
        for batch_idx, batch in enumerate(_in_lockstep(loader, device) if not args.synthetic else loader):
            d = trainer.step(batch)
            if lr_sched is not None:
                lr_sched.step()  # per batch, skipped ones included: the same index on every rank
            if d is None:
                log(f"Warning: NaN detected at batch {batch_idx + 1}. Skipping batch.")
                continue
            terms = [d["loss"].detach(), d["cls_loss"], d["box_loss"], d["intent_loss"]]
            if iou_on:
                terms += [d["iou_loss"], d["pos_iou"]]
            acc += torch.stack(terms).double()
            n_ok += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        # global epoch mean over ranks: every rank steps ReduceLROnPlateau on the same value, so
        # the LR (and with it the all-reduced update) stays identical across replicas
        tot = all_reduce_sum(acc.tolist() + [n_ok], device)
        acc, n_ok = torch.tensor(tot[:-1], dtype=torch.float64), int(round(tot[-1]))
        if n_ok > 0:
            avg = (acc / n_ok).tolist()
            iou_terms = f", iou_loss: {avg[4]:.4f}, pos_iou: {avg[5]:.4f}" if iou_on else ""
            log(f"Epoch {epoch + 1} Summary: Avg Loss: {avg[0]:.4f} (Cls: {avg[1]:.4f}, Box: {avg[2]:.4f}, "
                f"Intent: {avg[3]:.4f}{iou_terms}) LR: {optimizer.param_groups[0]['lr']:{'.1e' if lr_sched is None else '.3e'}}  "
                f"[{n_ok * args.batch / dt:.1f} samples/s]")
            if args.clip_grad_norm is not None:
                log(grad_clip_line(trainer.grad_stats(), args.clip_grad_norm))
                trainer.reset_grad_stats()
            if scheduler is not None:
                scheduler.step(avg[0])
        else:
            log(f"Epoch {epoch + 1} Warning: No batches processed successfully.")
    log(f"\n--- {tag} Training Finished ---")

    if rank == 0 and not args.no_save:
        save_dir = Path(args.save_dir)
        save_dir.mkdir(parents=True, exist_ok=True)
        path = save_dir / f"{variant}_model.pth"
        ckpt = {'epoch': args.epochs, 'model_state_dict': model.state_dict(),
                'optimizer_state_dict': optimizer.state_dict(), 'backbone_cfg': cfg}
        if lr_sched is not None:
            ckpt['lr_schedule_state_dict'] = lr_sched.state_dict()
        if ema is not None:
            ckpt.update(ema_state_dict=ema.state_dict(model), ema_decay=ema.decay, ema_warmup=ema.warmup)
        torch.save(ckpt, path)
        log(f"Saved final TRAINED {tag} model to {path}")
    if world > 1:
        torch.distributed.destroy_process_group()
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
