"""Self-supervised MAE pre-training of one ViT stream (mae.MaskedAutoencoderViT) on the MI355X kernels.

Reads the same batches as train_vit.py (``--synthetic``, or the Argoverse-2 logs under ``--data-dir``
through dataset.FrameBatchLoader) and discards the labels: ``--stream lidar`` trains on the LiDAR
raster, ``--stream map`` on the map raster. The optimiser is FusedAdamW; its update launch reads the
loss's device finite flag (and, with ``--clip-grad-norm``, the clip coefficient of
``FusedAdamW.grad_norm``), so a step makes no host sync: the per-step losses stay on the device and are
read once per epoch for the log line. ``--sched cosine --warmup-epochs E --min-lr X`` is the MAE recipe's
schedule (optim.WarmupCosineLR, stepped per update; default: constant lr) and ``--no-decay-1d`` its weight
decay rule (none on norm scales, biases, ``pos_embed``, ``cls_token`` and ``mask_token``; the two groups
update in one fused launch). Layer-wise lr decay is a fine-tuning device and is not offered here.

Writes ``mae_<stream>.pth`` (the whole model, its config and the optimizer state, for resuming) and
``mae_<stream>_encoder.pth`` (the encoder alone, timm keys: what ``train_vit.py --pretrained-lidar`` /
``--pretrained-map`` and ``VisionTransformer.load_pretrained`` take). ``--dump-recon DIR`` also writes
``recon_<stream>.pt``: the last batch's input, reconstruction and mask.

Single GPU: pre-training under DDP is not built.
"""
from __future__ import annotations

import argparse
import time
from pathlib import Path

import torch

from constants import GRID_HEIGHT_PX, GRID_WIDTH_PX, LIDAR_SWEEPS, LIDAR_TOTAL_CHANNELS, MAP_CHANNELS
from mae import create_mae
from optim import FusedAdamW, WarmupCosineLR, layer_decay_param_groups
from synthetic import SyntheticBEVLoader
from train_vit import TRAIN_DATA_DIR
from vit import VIT_ARCH

MODEL_SAVE_DIR_MAE = "./trained_models_mae"
STREAMS = {"lidar": ("lidar_bev", LIDAR_TOTAL_CHANNELS), "map": ("map_bev", MAP_CHANNELS)}


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--stream", choices=sorted(STREAMS), default="lidar", help="which raster (and stream) to pre-train")
    ap.add_argument("--synthetic", action="store_true", help="seeded synthetic BEV batches instead of --data-dir")
    ap.add_argument("--data-dir", type=str, default=TRAIN_DATA_DIR, help="Argoverse-2 sensor split to read")
    ap.add_argument("--num-sweeps", type=int, default=LIDAR_SWEEPS)
    ap.add_argument("--arch", choices=sorted(VIT_ARCH), default="vit_small_patch8_224")
    ap.add_argument("--grid", type=str, default=f"{GRID_HEIGHT_PX}x{GRID_WIDTH_PX}")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--batches-per-epoch", type=int, default=16, help="synthetic batches per epoch")
    ap.add_argument("--fresh-batches", action="store_true", help="draw a new synthetic batch every step")
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--mask-ratio", type=float, default=0.75)
    ap.add_argument("--norm-pix-loss", action="store_true",
                    help="normalise every target patch by its own mean and (n - 1) variance")
    ap.add_argument("--decoder-dim", type=int, default=192, help="decoder width (64 per head)")
    ap.add_argument("--decoder-depth", type=int, default=4)
    ap.add_argument("--lr", type=float, default=1.5e-4)
    ap.add_argument("--weight-decay", type=float, default=0.05)
    ap.add_argument("--no-decay-1d", action="store_true",
                    help="no weight decay on 1-D parameters, biases, pos_embed, cls_token and mask_token")
    ap.add_argument("--sched", choices=["constant", "cosine"], default="constant",
                    help="cosine: linear warmup then cosine decay to --min-lr over --epochs, stepped every update")
    ap.add_argument("--warmup-epochs", type=float, default=0.0, metavar="E", help="with --sched cosine")
    ap.add_argument("--min-lr", type=float, default=0.0, metavar="X", help="with --sched cosine")
    ap.add_argument("--clip-grad-norm", type=float, default=None, metavar="X",
                    help="clip the global gradient L2 norm to X on the device (FusedAdamW.grad_norm, no host sync)")
    ap.add_argument("--augment", action="store_true", help="training-time augment_bev on every batch, on the GPU")
    ap.add_argument("--seed", type=int, default=0, help="seed of the weights' initialisation and the masks")
    ap.add_argument("--save-dir", type=str, default=MODEL_SAVE_DIR_MAE)
    ap.add_argument("--no-save", action="store_true")
    ap.add_argument("--dump-recon", type=str, default=None, metavar="DIR",
                    help="write recon_<stream>.pt (input, reconstruction, mask of the last batch) into DIR")
    args = ap.parse_args(argv)
    if args.decoder_dim <= 0 or args.decoder_dim % 64 != 0:
        ap.error(f"--decoder-dim {args.decoder_dim}: a positive multiple of 64 (the attention head dim)")
    if args.sched == "cosine":
        if args.epochs <= 0:
            ap.error("--sched cosine: the schedule spans --epochs x batches per epoch updates; --epochs must be > 0")
        if not 0.0 <= args.warmup_epochs <= args.epochs:
            ap.error(f"--warmup-epochs {args.warmup_epochs:g}: must lie in [0, --epochs]")
    return args


def build_model(args, grid, device):
    key, chans = STREAMS[args.stream]
    model = create_mae(args.arch, chans, grid, decoder_embed_dim=args.decoder_dim, decoder_depth=args.decoder_depth,
                       decoder_num_heads=args.decoder_dim // 64, mask_ratio=args.mask_ratio,
                       norm_pix_loss=args.norm_pix_loss).to(device)
    model.set_compute_dtype(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    return model, key


def run(args):
    """The pre-training loop. -> {'losses': per-step losses (list of float), 'files': paths written}."""
    if not torch.cuda.is_available():
        raise RuntimeError("pretrain_mae.py runs on the MI355X kernels: no ROCm GPU visible")
    device = torch.device("cuda", torch.cuda.current_device())
    H, W = (int(v) for v in args.grid.lower().split("x"))
    torch.manual_seed(args.seed)
    model, key = build_model(args, (H, W), device)
    print("--- MAE Pre-training Configuration ---")
    print(f"Stream: {args.stream} ({STREAMS[args.stream][1]} channels), encoder {args.arch}, grid {(H, W)}")
    print(f"Data: {'synthetic' if args.synthetic else args.data_dir}")
    print(f"Mask ratio {args.mask_ratio:g}, norm_pix_loss {args.norm_pix_loss}, decoder {args.decoder_dim} x "
          f"{args.decoder_depth}, batch {args.batch}, epochs {args.epochs}, LR {args.lr:g}, dtype {args.dtype}")
    if args.synthetic:
        loader = SyntheticBEVLoader(args.batch, args.batches_per_epoch, (H, W), device=device,
                                    resident=not args.fresh_batches, augment=args.augment)
    else:
        if not Path(args.data_dir).is_dir():
            raise SystemExit(f"ERROR: data directory not found: {args.data_dir} (use --synthetic)")
        if (H, W) != (GRID_HEIGHT_PX, GRID_WIDTH_PX):
            raise SystemExit(f"--grid {args.grid}: Argoverse-2 rasters have the constants.py grid "
                             f"{GRID_HEIGHT_PX}x{GRID_WIDTH_PX}; other grids need --synthetic")
        from dataset import ArgoverseIntentNetDataset, FrameBatchLoader
        data = ArgoverseIntentNetDataset(args.data_dir, num_sweeps=args.num_sweeps, is_train=True, device=device)
        loader = FrameBatchLoader(data, args.batch, shuffle=True, rank=0, world=1, augment=args.augment, device=device)
    if args.no_decay_1d:
        groups = layer_decay_param_groups(model, 1.0, args.weight_decay, no_decay_1d=True)
        print("Weight decay: " + ", ".join(f"{g['weight_decay']:g} on {len(g['params'])} tensors" for g in groups))
        opt = FusedAdamW(groups, lr=args.lr, betas=(0.9, 0.95), weight_decay=args.weight_decay, fuse_groups=True)
    else:
        opt = FusedAdamW(model.parameters(), lr=args.lr, betas=(0.9, 0.95), weight_decay=args.weight_decay)
    sched = None
    if args.sched == "cosine":
        total = args.epochs * len(loader)
        if total <= 0:
            raise SystemExit(f"--sched cosine: no updates to schedule ({args.epochs} epoch(s) x {len(loader)} batch(es))")
        sched = WarmupCosineLR(opt, int(round(args.warmup_epochs * len(loader))), total, min_lr=args.min_lr)
        print(f"LR schedule: {sched.warmup_steps} warmup + cosine over {sched.total_steps} updates, min lr {args.min_lr:g}")
    model.train()
    losses, last = [], None
    for epoch in range(args.epochs):
        t0 = time.perf_counter()
        step_loss = []
        for batch in loader:
            x = batch[key]
            last = x
            opt.zero_grad(set_to_none=True)
            loss, _ = model(x)
            loss.backward()
            fin = model.last_finite
            if args.clip_grad_norm is not None:
                gn = opt.grad_norm(args.clip_grad_norm, finite=fin)
                opt.step(finite=gn.finite, grad_scale=gn.coef)
            else:
                opt.step(finite=fin)
            if sched is not None:
                sched.step()
            step_loss.append(loss.detach())
        if not step_loss:
            print(f"Epoch {epoch + 1}: no batches")
            continue
        vals = torch.stack(step_loss).tolist()  # the epoch's one host read
        dt = time.perf_counter() - t0
        losses += vals
        ok = [v for v in vals if v == v and abs(v) != float("inf")]
        mean = sum(ok) / len(ok) if ok else float("nan")
        print(f"Epoch {epoch + 1}: loss mean {mean:.6f} (first {vals[0]:.6f}, last {vals[-1]:.6f}), "
              f"{len(vals) - len(ok)} non-finite step(s) skipped"
              + (f", LR {opt.param_groups[0]['lr']:.3e}" if sched is not None else "")
              + f"  [{len(vals) * args.batch / dt:.1f} samples/s]")
    files = []
    if not args.no_save:
        save_dir = Path(args.save_dir)
        save_dir.mkdir(parents=True, exist_ok=True)
        full, enc = save_dir / f"mae_{args.stream}.pth", save_dir / f"mae_{args.stream}_encoder.pth"
        torch.save({"epoch": args.epochs, "model_state_dict": model.state_dict(), "optimizer_state_dict": opt.state_dict(),
                    **({"lr_schedule_state_dict": sched.state_dict()} if sched is not None else {}),
                    "mae_cfg": dict(model.config(), arch=args.arch, stream=args.stream, img_size=(H, W),
                                    in_chans=STREAMS[args.stream][1])}, full)
        model.save_encoder(enc)
        files += [str(full), str(enc)]
        print(f"Saved {full} and {enc} (the encoder: --pretrained-{args.stream} of train_vit.py)")
    if args.dump_recon is not None and last is not None:
        out = Path(args.dump_recon)
        out.mkdir(parents=True, exist_ok=True)
        rec, mask = model.reconstruct(last)
        path = out / f"recon_{args.stream}.pt"
        torch.save({"input": last.cpu(), "recon": rec.cpu(), "mask": mask.cpu()}, path)
        files.append(str(path))
        print(f"Saved {path}")
    return {"losses": losses, "files": files}


def main(argv=None):
    run(parse_args(argv))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
