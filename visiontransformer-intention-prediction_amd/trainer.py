"""One IntentNetViT training step — the loop body of train_vit.py:151-187 — shared by
train_vit.py and bench.py.

zero_grad → forward → (NaN skip) → DetectionIntentionLoss → (non-finite-loss no-op) → backward
(gradient buckets all-reduce while it runs when world > 1) → FusedAdamW.

* NaN in the model outputs skips the batch (train_vit.py:160-162): ``step`` returns None.
* A non-finite total loss comes back from the loss as a zero (loss.py:190-198 returns a
  disconnected zero leaf): the reference's ``loss.backward()`` then produces no gradient and
  ``optimizer.step()`` updates nothing (AdamW skips parameters whose ``.grad`` is None, step
  counters included). Here backward and the optimizer step are skipped outright, so the
  weights, the Adam moments and the step counters stay bit-identical; the zero loss dict is
  returned, and the caller accumulates it as the reference's loop does.

Both checks are taken collectively across ranks (ddp.any_rank) so every rank stays on the same
step; under DDP one rank's non-finite loss therefore skips the update on every rank (the
replicas stay identical). They cost one host sync each, as the reference's ``torch.isnan``
checks do; the benchmark turns them off (``check_nan=False``) — nothing else is skipped. Without
the host checks a non-finite loss still zeroes the update: backward runs (exact-zero gradients
from the loss kernel) and FusedAdamW's launch reads the loss's device finite flag (min over ranks
under DDP) and leaves weights and moments untouched; only its host step counters advance.

``max_grad_norm`` (None = off, exactly the step above): global L2-norm clipping without a host
read. After ``buckets.finish()`` the gradients are final (and bit-identical on every rank, so the
norm needs no collective); FusedAdamW.grad_norm takes their norm (f64 sums, a fixed order), and the
update launch multiplies each gradient by the clip coefficient as it loads it and reads
``finite = loss flag AND norm finite``: a gradient that overflowed skips the update like a
non-finite loss does (weights, moments and device step counts unchanged). The loss dict gains
``grad_norm`` (the norm before clipping, a 0-d device tensor); ``clipped`` / ``nonfinite_grad`` /
``grad_stats()`` read the device accumulator on demand.

``ema`` (optim.ModelEMA; None = off, exactly the step above): every optimiser call becomes
``FusedAdamW.step_ema``, whose launch moves the average towards the weight it has just written. A
batch the host checks skip never reaches the optimiser and a launch that reads finite = 0 writes
nothing, so neither moves the average. Under DDP nothing is communicated for it: the parameters are
bit-identical on every rank after the update, and so is the average.
"""
from __future__ import annotations

import torch

from ddp import GradBuckets, any_rank, broadcast_state, grad_order, min_on_device
from loss import device_guard
from optim import STATS_FIELDS, FusedAdamW, ModelEMA


class Trainer:
    def __init__(self, model, loss_fn, optimizer, anchors, world: int = 1, bucket_mb: float = 64.0,
                 check_nan: bool = True, force_buckets: bool = False, max_grad_norm: float | None = None,
                 ema: ModelEMA | None = None):
        if ema is not None:
            if not isinstance(ema, ModelEMA):
                raise TypeError("Trainer: ema is an optim.ModelEMA or None")
            if not isinstance(optimizer, FusedAdamW):
                raise TypeError("Trainer: ema needs FusedAdamW (the average is part of its launch)")
        self.ema = ema
        if max_grad_norm is not None:
            if not float(max_grad_norm) > 0.0:
                raise ValueError(f"Trainer: max_grad_norm must be > 0 or None (got {max_grad_norm})")
            if not isinstance(optimizer, FusedAdamW):
                raise TypeError("Trainer: max_grad_norm needs FusedAdamW (the clip is part of its launch)")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self._grad_stats = None  # device f64 [5], optim.STATS_FIELDS
        self.model, self.loss_fn, self.optimizer, self.anchors = model, loss_fn, optimizer, anchors
        self.world = world
        self.check_nan = check_nan
        if world > 1:
            # identical replicas from the first step, whatever each rank's RNG did
            broadcast_state(model)
        # force_buckets: the bucketed all-reduce path even at world 1 (tests on one GPU over RCCL)
        # buckets in the order the interleaved backward produces gradients, the last ones in a
        # 32-MB bucket of their own (the collective left after the backward)
        self.buckets = GradBuckets(grad_order(model), bucket_mb, force_collectives=force_buckets,
                                   last_bucket_mb=min(32.0, bucket_mb)) if world > 1 or force_buckets else None
        self.skipped = 0
        self.nonfinite = 0

    def zero_grad(self):
        if self.buckets is not None:
            self.buckets.zero_grad()
        else:
            self.optimizer.zero_grad(set_to_none=True)

    def grad_stats(self):
        """{steps, clipped, nonfinite, norm_sum, norm_max} of the clipped steps so far: ONE host read."""
        vals = self._grad_stats.tolist() if self._grad_stats is not None else [0.0] * len(STATS_FIELDS)
        return dict(zip(STATS_FIELDS, vals))

    def reset_grad_stats(self):
        if self._grad_stats is not None:
            self._grad_stats.zero_()

    @property
    def clipped(self):
        """Steps whose gradient norm exceeded max_grad_norm (a host read)."""
        return int(self.grad_stats()["clipped"])

    @property
    def nonfinite_grad(self):
        """Steps skipped because the gradient norm was not finite (a host read)."""
        return int(self.grad_stats()["nonfinite"])

    def _loss_finite(self, d):
        fin = getattr(self.loss_fn, "last_finite", None)
        if fin is None:
            return bool(torch.isfinite(d["loss"]).all())
        return bool(fin) and not bool(torch.isnan(d["loss"]))

    def _opt_step(self, **kw):
        if self.ema is None:
            return self.optimizer.step(**kw)
        return self.optimizer.step_ema(self.ema, **kw)

    def step(self, batch: dict):
        """Returns the loss dict, or None when the batch was skipped (NaN in the outputs)."""
        lidar, mp, gts = batch["lidar_bev"], batch["map_bev"], batch["gt_list"]
        self.zero_grad()
        cls, box, intent = self.model(lidar, mp)
        dev = cls.device
        if self.check_nan:
            bad = torch.isnan(cls).any() | torch.isnan(box).any() | torch.isnan(intent).any()
            if any_rank(bool(bad), dev):
                self.skipped += 1
                return None
        with device_guard():  # the sync-free guard: last_finite decides below (loss.py docstring)
            d = self.loss_fn(cls, box, intent, self.anchors, gts)
        if self.check_nan and any_rank(not self._loss_finite(d), dev):
            self.nonfinite += 1
            return d
        d["loss"].backward()
        if self.buckets is not None:
            self.buckets.finish()
        fin = getattr(self.loss_fn, "last_finite", None)
        if self.max_grad_norm is not None:
            # with the host checks on, every rank has already agreed that the loss is finite
            if not self.check_nan and fin is not None and self.buckets is not None and self.world > 1:
                fin = min_on_device(fin)
            if self._grad_stats is None:
                self._grad_stats = torch.zeros(len(STATS_FIELDS), dtype=torch.float64, device=dev)
            gn = self.optimizer.grad_norm(self.max_grad_norm, finite=fin, stats=self._grad_stats)
            self._opt_step(finite=gn.finite, grad_scale=gn.coef)
            d["grad_norm"] = gn.norm
        elif not self.check_nan and fin is not None and isinstance(self.optimizer, FusedAdamW):
            # no host sync: the update launch itself reads the loss's finite flag and does nothing
            # on 0 (weights and moments unchanged, as with the reference's disconnected zero loss)
            if self.buckets is not None and self.world > 1:
                fin = min_on_device(fin)  # every rank skips together (replicas stay identical)
            self._opt_step(finite=fin)
        else:
            self._opt_step()
        return d
