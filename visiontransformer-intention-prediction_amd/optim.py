"""Fused AdamW (torch.optim.AdamW semantics as used at train_vit.py:130: lr 1e-4, wd 1e-4,
betas (0.9, 0.999), eps 1e-8, decoupled weight decay) over device pointer tables instead of torch's
per-tensor foreach kernels: one HIP launch per parameter group, or with ``fuse_groups=True`` ONE
launch for all groups that share lr, betas and eps (their per-group ``lr_scale`` and ``weight_decay``
go to the kernel as a per-tensor table). Beside it the fine-tuning recipe those groups are for:
``layer_decay_param_groups`` (layer-wise lr decay, no decay on 1-D tensors and tokens) and
``WarmupCosineLR`` (linear warmup, cosine decay, stepped per update)."""
from __future__ import annotations

import contextlib
import ctypes
import math

import torch

import ops
from _lib import lib, ptr, stream, workspace


class _Tables:
    """Cached device tables of a tensor list (pointers, sizes, (tensor, chunk) records): what the
    chunked launches (ivit_adamw_chunked, ivit_grad_norm, ivit_grad_scale) take."""

    def __init__(self):
        self._tables = {}

    def _table(self, tensors, device):
        key = tuple(t.data_ptr() for t in tensors)
        tab = self._tables.get(key)
        if tab is None:
            # pinned staging + non_blocking: a pageable H2D copy would stall the host until the
            # GPU drains (a bubble every step when gradient buffers move)
            tab = torch.tensor(key, dtype=torch.int64).pin_memory().to(device, non_blocking=True)
            if len(self._tables) > 64:
                self._tables.clear()
            self._tables[key] = tab
        return tab

    def _table_chunks(self, ps, device):
        """Device int32 [n][2] table of (tensor, chunk) for ivit_adamw_chunked: every
        ivit_adamw_chunk_elems()-element chunk of every tensor of the launch."""
        key = ("chunks",) + tuple(p.numel() for p in ps)
        tab = self._tables.get(key)
        if tab is None:
            ce = lib.ivit_adamw_chunk_elems()
            rec = [(t, c) for t, p in enumerate(ps) for c in range(-(-p.numel() // ce))]
            tab = (torch.tensor(rec, dtype=torch.int32).reshape(len(rec), 2).pin_memory().to(device, non_blocking=True),
                   len(rec))
            if len(self._tables) > 64:
                self._tables.clear()
            self._tables[key] = tab
        return tab

    def _table_sizes(self, ps, device):
        key = ("sizes",) + tuple(p.numel() for p in ps)
        tab = self._tables.get(key)
        if tab is None:
            tab = torch.tensor([p.numel() for p in ps], dtype=torch.int64).pin_memory().to(device, non_blocking=True)
            self._tables[key] = tab
        return tab

    def _norm_launch(self, grads, max_norm, finite, stats):
        """ivit_grad_norm over ``grads`` (device f32, contiguous) -> GradNorm; no host read."""
        max_norm = float(max_norm)
        if not max_norm > 0.0:
            raise ValueError(f"max_norm must be > 0 (got {max_norm})")
        for g in grads:
            if not g.is_cuda:
                raise RuntimeError("ivit ops take device tensors (no CPU fallback)")
            if g.dtype != torch.float32 or not g.is_contiguous():
                raise TypeError("grad norm: contiguous f32 gradients required")
        if stats is not None and (stats.dtype != torch.float64 or stats.numel() < 5):
            raise TypeError("grad norm: stats is a device f64 tensor of 5 elements")
        dev = grads[0].device if grads else (finite.device if finite is not None else torch.device("cuda"))
        chunks, nch = self._table_chunks(grads, dev)
        key = ("normws", nch, str(dev))
        ws = self._tables.get(key)
        if ws is None:
            ws = self._tables[key] = workspace(lib.ivit_grad_norm_workspace(nch), dev)
        rec = torch.empty(4, dtype=torch.float32, device=dev)  # a fresh record: it outlives later steps
        tg, sizes = (self._table(grads, dev), self._table_sizes(grads, dev)) if grads else (None, None)
        lib.ivit_grad_norm(len(grads), ptr(tg), ptr(sizes), ptr(chunks) if nch else None, nch, max_norm, ptr(finite),
                           ptr(ws), ws.numel(), ptr(rec), ptr(stats), stream())
        return GradNorm(rec)

    def _scale_launch(self, grads, coef):
        """ivit_grad_scale: g *= coef (device scalar) in place over ``grads``."""
        if not grads:
            return
        dev = grads[0].device
        chunks, nch = self._table_chunks(grads, dev)
        lib.ivit_grad_scale(len(grads), ptr(self._table(grads, dev)), ptr(self._table_sizes(grads, dev)),
                            ptr(chunks) if nch else None, nch, ptr(coef), stream())

    def _followers(self, ps):
        """What follows the f32 weights ``ps`` and is rewritten when a launch changes them behind the
        version counter: (bf16 shadow pointer per tensor, 0 = none; ivit_weight_pack_multi jobs of the
        live row-panel packs; the largest pack in elements)."""
        shadows, jobs, big = [], [], 0
        for p in ps:
            sh = ops.shadow_of(p)
            shadows.append(sh.data_ptr() if sh is not None else 0)
            pk, pkt = ops.packs_of(p)
            rows, cols = p.shape[0], p.numel() // p.shape[0]
            for pack, tr in ((pk, 0), (pkt, 1)):
                if pack is not None:
                    jobs.append((p.data_ptr(), pack.data_ptr(), rows, cols, tr))
                    big = max(big, rows * cols)
        return shadows, jobs, big

    def _table_ptrs(self, ptrs, device):
        key = ("ptrs",) + tuple(ptrs)
        tab = self._tables.get(key)
        if tab is None:
            tab = torch.tensor(ptrs, dtype=torch.int64).pin_memory().to(device, non_blocking=True)
            if len(self._tables) > 64:
                self._tables.clear()
            self._tables[key] = tab
        return tab

    def _table_hyper(self, runs, device):
        """Device f32 [n][2] table of (lr_scale, weight_decay) per tensor of an ivit_adamw_chunked_pt
        launch, from ``runs`` = [(lr_scale, weight_decay, count)]: consecutive tensors with the same pair
        (a parameter group's). The table holds values only, so the runs are its key: the same groups
        over other gradient buffers reuse it, and the lr itself is a kernel scalar (a schedule that
        moves it every step uploads nothing)."""
        key = ("hyper",) + tuple(runs)
        tab = self._tables.get(key)
        if tab is None:
            rows = [(s, w) for s, w, n in runs for _ in range(n)]
            tab = torch.tensor(rows, dtype=torch.float32).reshape(len(rows), 2).pin_memory().to(device, non_blocking=True)
            if len(self._tables) > 64:
                self._tables.clear()
            self._tables[key] = tab
        return tab

    def _pack_jobs(self, jobs, device):
        """Device table of ivit_weight_pack_multi records (w, wpack, rows, cols, transposed), 40 B each."""
        key = ("packs",) + tuple(jobs)
        tab = self._tables.get(key)
        if tab is None:
            rec = []
            for w, wp, rows, cols, tr in jobs:
                rec += [w, wp, rows, cols, tr]
            tab = torch.tensor(rec, dtype=torch.int64).pin_memory().to(device, non_blocking=True)
            if len(self._tables) > 64:
                self._tables.clear()
            self._tables[key] = tab
        return tab


class GradNorm:
    """The device record of one ivit_grad_norm call: ``norm`` (the global L2 norm before clipping),
    ``coef`` (min(1, max_norm / (norm + 1e-6)), 1 when the norm is not finite) and ``finite`` (1.0 /
    0.0: the incoming flag and a finite norm), each a 0-d f32 view of ``record``."""
    __slots__ = ("record", "norm", "coef", "finite")

    def __init__(self, record):
        self.record = record
        self.norm, self.coef, self.finite = record[0], record[1], record[2]


STATS_FIELDS = ("steps", "clipped", "nonfinite", "norm_sum", "norm_max")  # ivit_grad_norm's stats (f64 [5])


def _f32(x):
    return ctypes.c_float(x).value


def effective_lr(lr, lr_scale):
    """f32(lr) * f32(lr_scale) rounded to f32: the learning rate of a group with ``lr_scale``, as the
    per-group launch receives it and as ivit_adamw_chunked_pt forms it from its table."""
    return _f32(_f32(lr) * _f32(lr_scale))  # the f64 product of two f32 values is exact: one rounding


class FusedAdamW(torch.optim.Optimizer, _Tables):
    """``lr_scale`` (optional per group, the timm key; absent = 1): the group's learning rate is
    ``effective_lr(group['lr'], group['lr_scale'])``; it is part of ``state_dict()`` like every other
    group entry. ``fuse_groups=False``: one launch per group (a group without ``lr_scale`` makes exactly
    the call it always made). ``fuse_groups=True``: the groups that share lr, betas and eps go out in
    ONE ivit_adamw_chunked_pt launch (per distinct step count when the host counts, as within a group)
    with their (lr_scale, weight_decay) in a per-tensor table, followed by one ivit_weight_pack_multi
    over all their packs; groups that differ in lr, betas or eps launch separately. Bit-identical to
    the per-group form."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, fuse_groups=False):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.fuse_groups = bool(fuse_groups)
        self._tables = {}

    @torch.no_grad()
    def step(self, closure=None, finite=None, grad_scale=None):
        """One AdamW update. ``grad_scale``: optional device scalar (f32, e.g. ``grad_norm(...).coef``);
        every gradient element is multiplied by it as the launch loads it (``.grad`` stays as it is):
        the update of ``clip_grad_norm_`` + ``step`` without the pass that rewrites the gradients.
        ``finite``: optional device scalar (f32); when it holds 0 the launch
        updates nothing — the guard of loss.py:190-198 without a host sync (trainer.Trainer passes
        the loss's flag when it does not sync). On that path the step counts live on the device
        (``state['step']`` is a 0-d f32 device tensor, as torch's capturable AdamW keeps it) and a
        skipped update does not advance them, so the bias correction of every later step is the one
        torch.optim.AdamW applies when the reference's disconnected zero loss left no gradient."""
        return self._step(closure, finite, grad_scale, None)

    @torch.no_grad()
    def step_ema(self, ema, closure=None, finite=None, grad_scale=None):
        """``step`` that also moves ``ema`` (a ModelEMA; None = ``step``) in the same launch: every
        updated parameter that ``ema`` tracks has its average moved towards the new weight,
        e += (1 - d) * (p_new - e) with d = ``ema.decay_at(n)`` at the parameter's step count n after
        this update. A parameter without a gradient, one ``ema`` does not track and an update that
        ``finite`` = 0 skips all leave the average as it is. Weights, moments, counts and shadows
        are the bits of ``step``."""
        return self._step(closure, finite, grad_scale, ema)

    def _step(self, closure, finite, grad_scale, ema):
        if ema is not None and ema._swapped:
            raise RuntimeError("FusedAdamW: the ModelEMA is swapped into the model (leave swapped() first)")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        merged = {}  # fuse_groups: (lr, betas, eps) -> [first group, parameters, (lr_scale, weight_decay, count) runs]
        for group in self.param_groups:
            live = [p for p in group["params"] if p.grad is not None]
            for p in live:
                if p.dtype != torch.float32 or p.grad.dtype != torch.float32 or not p.is_contiguous() \
                        or not p.grad.is_contiguous():
                    raise TypeError("FusedAdamW: contiguous f32 params/grads required")
            self._init_state([p for p in live if not self.state[p]])
            if not live:
                continue
            if self.fuse_groups:
                key = (float(group["lr"]), tuple(float(b) for b in group["betas"]), float(group["eps"]))
                m = merged.setdefault(key, [group, [], []])
                m[1] += live
                m[2].append((float(group.get("lr_scale", 1.0)), float(group["weight_decay"]), len(live)))
            else:
                self._update(group, live, None, finite, grad_scale, ema)
        for group, live, hyper in merged.values():
            self._update(group, live, hyper, finite, grad_scale, ema)
        return loss

    def _update(self, group, live, hyper, finite, grad_scale, ema):
        """The launch(es) of one group's live parameters, or with ``hyper`` (runs of (lr_scale,
        weight_decay, count) over ``live``) of the merged groups that share ``group``'s lr, betas and eps."""
        if finite is None:
            each = None if hyper is None else [(s, w) for s, w, n in hyper for _ in range(n)]
            by_step = {}
            for i, p in enumerate(live):
                st = self.state[p]
                st["step"] = int(st["step"]) + 1  # a device count (sync-free path) is read once
                ps, hy = by_step.setdefault(st["step"], ([], []))
                ps.append(p)
                if each is not None:
                    if hy and hy[-1][:2] == each[i]:
                        hy[-1] = each[i] + (hy[-1][2] + 1,)
                    else:
                        hy.append(each[i] + (1,))
            for step, (ps, hy) in by_step.items():
                b1, b2 = group["betas"]
                self._launch(group, ps, 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step), None, None, None, grad_scale,
                             ema, step, hy if hyper is not None else None)
        else:
            sin, sout = self._device_steps(live)
            self._launch(group, live, 1.0, 1.0, finite, sin, sout, grad_scale, ema, None, hyper)
            for i, p in enumerate(live):
                self.state[p]["step"] = sout[i]  # 0-d view; the other buffer is next step's output

    @torch.no_grad()
    def grad_norm(self, max_norm, finite=None, stats=None):
        """Global L2 norm of the live gradients of ALL parameter groups (ivit_grad_norm: two launches,
        f64 sums, no host read) -> GradNorm (``norm``, ``coef``, ``finite`` as 0-d device views).
        ``finite``: optional device flag folded into the record's (the loss guard); ``stats``:
        optional device f64 [5] accumulator (STATS_FIELDS). Pass ``coef`` and ``finite`` to ``step``."""
        grads = [p.grad for g in self.param_groups for p in g["params"] if p.grad is not None]
        return self._norm_launch(grads, max_norm, finite, stats)

    def _device_steps(self, ps):
        """(steps_in, steps_out) device f32 buffers for this parameter list: steps_in holds every
        parameter's current count. Reused across steps (the two buffers alternate), rebuilt from the
        state (one host read) when the list changes or a count was set elsewhere."""
        key = ("steps",) + tuple(id(p) for p in ps)
        bufs = self._tables.get(key)
        cur = [self.state[p]["step"] for p in ps]
        if bufs is not None:
            for b in bufs:
                if all(torch.is_tensor(c) and c.data_ptr() == b[i].data_ptr() for i, c in enumerate(cur)):
                    other = bufs[1] if b is bufs[0] else bufs[0]
                    return b, other
        dev = ps[0].device
        sin = torch.tensor([float(c) for c in cur], dtype=torch.float32, device=dev)
        bufs = (sin, torch.empty_like(sin))
        if len(self._tables) > 64:
            self._tables.clear()
        self._tables[key] = bufs
        return bufs

    def _launch(self, group, ps, bc1, bc2s, finite, sin, sout, grad_scale=None, ema=None, host_step=None, hyper=None):
        """The update of ``ps`` through the chunked streaming kernel (live bf16 compute copies,
        ops.cast_weight, rewritten in it), then every live row-panel weight pack (ops.packed_weight /
        packed_weight_t) rebuilt from the updated f32 weights in ONE launch: the pointer-table update
        moves no version counter, so without it the packs would stay at the old weights.
        ``ema`` (ModelEMA): its table goes to ivit_adamw_chunked_ema; with device counts the launch
        forms the decay from steps_in, with host counts (``host_step``: the count after this update)
        the host does and passes it with the warmup off. ``hyper`` (runs of (lr_scale, weight_decay, count)
        over ``ps``, fuse_groups): the table of ivit_adamw_chunked_pt, which takes the group's lr as it is;
        without it a group's ``lr_scale`` is folded into the lr scalar on the host (effective_lr)."""
        b1, b2 = group["betas"]
        dev = ps[0].device
        st = [self.state[p] for p in ps]
        tp = self._table(ps, dev)
        tg = self._table([p.grad for p in ps], dev)
        tm = self._table([s["exp_avg"] for s in st], dev)
        tv = self._table([s["exp_avg_sq"] for s in st], dev)
        sizes = self._table_sizes(ps, dev)
        shadows, jobs, big = self._followers(ps)
        chunks, nch = self._table_chunks(ps, dev)
        lr = group["lr"] if hyper is not None or "lr_scale" not in group else effective_lr(group["lr"], group["lr_scale"])
        args = (len(ps), ptr(tp), ptr(tg), ptr(tm), ptr(tv), ptr(self._table_ptrs(shadows, dev)), ptr(sizes),
                ptr(chunks), nch, lr, b1, b2, group["eps"], group["weight_decay"], bc1, bc2s, ptr(finite),
                ptr(sin), ptr(sout))
        if hyper is not None:
            if sum(n for _, _, n in hyper) != len(ps):  # the kernel reads one table row per tensor
                raise RuntimeError("FusedAdamW: the (lr_scale, weight_decay) runs do not cover the launch's tensors")
            te, decay, warm = None, 0.0, 0
            if ema is not None:
                te = self._table_ptrs(ema._ptrs(ps), dev)
                decay, warm = (ema.decay, int(ema.warmup)) if sin is not None else (ema.decay_at(host_step), 0)
            lib.ivit_adamw_chunked_pt(*args, ptr(grad_scale), ptr(te), decay, warm,
                                      ptr(self._table_hyper(hyper, dev)), stream())
        elif ema is not None:
            te = self._table_ptrs(ema._ptrs(ps), dev)
            decay, warm = (ema.decay, int(ema.warmup)) if sin is not None else (ema.decay_at(host_step), 0)
            lib.ivit_adamw_chunked_ema(*args, ptr(grad_scale), ptr(te), decay, warm, stream())
        elif grad_scale is None:
            lib.ivit_adamw_chunked(*args, stream())
        else:
            lib.ivit_adamw_chunked_scaled(*args, ptr(grad_scale), stream())
        if jobs:
            lib.ivit_weight_pack_multi(len(jobs), ptr(self._pack_jobs(jobs, dev)), big, stream())

    def _init_state(self, fresh):
        """Zero moments of the parameters seen for the first time: views into one flat buffer per
        device and moment (a single fill each, not two per parameter)."""
        by_dev = {}
        for p in fresh:
            by_dev.setdefault(p.device, []).append(p)
        for dev, ps in by_dev.items():
            n = sum(p.numel() for p in ps)
            flat = torch.zeros((2, n), dtype=torch.float32, device=dev)
            o = 0
            for p in ps:
                k = p.numel()
                self.state[p].update(step=0, exp_avg=flat[0, o:o + k].view_as(p), exp_avg_sq=flat[1, o:o + k].view_as(p))
                o += k


class ModelEMA(_Tables):
    """Exponential moving average of a model's parameters, kept by the optimiser's own launch
    (FusedAdamW.step_ema / Trainer(ema=...)): e += (1 - d) (p - e) after every update, with
    d = decay, or under ``warmup`` min(decay, (1 + n) / (10 + n)) at the parameter's step count n
    (the usual ramp: a young average follows the weights closely). One flat f32 device buffer holds
    every average, each starting at a multiple of 4 elements (16 bytes), initialised to the weights.
    Buffers (BatchNorm statistics) are not averaged: ``state_dict`` takes them live from the model."""

    def __init__(self, model_or_params, decay=0.9998, warmup=True):
        super().__init__()
        decay = float(decay)
        if not 0.0 <= decay < 1.0:  # NaN fails too
            raise ValueError(f"ModelEMA: decay must be in [0, 1) (got {decay})")
        self.decay, self.warmup = decay, bool(warmup)
        ps = model_or_params.parameters() if isinstance(model_or_params, torch.nn.Module) else model_or_params
        self.params = [p for p in ps]
        if not self.params:
            raise ValueError("ModelEMA: no parameters")
        dev = self.params[0].device
        offs, n = [], 0
        for p in self.params:
            if not p.is_cuda:
                raise RuntimeError("ivit ops take device tensors (no CPU fallback)")
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
                raise TypeError("ModelEMA: contiguous f32 parameters on one device required")
            offs.append(n)
            n += (p.numel() + 3) // 4 * 4
        self.flat = torch.zeros(n, dtype=torch.float32, device=dev)
        self._views = {id(p): self.flat[o:o + p.numel()].view_as(p) for p, o in zip(self.params, offs)}
        with torch.no_grad():
            torch._foreach_copy_([self._views[id(p)] for p in self.params], [p.detach() for p in self.params])
        self._swapped = False

    def decay_at(self, n):
        """The decay of the update that brings a parameter to step count n (f64, as the launch forms it)."""
        n = float(n)
        return min(self.decay, (1.0 + n) / (10.0 + n)) if self.warmup else self.decay

    def ema_of(self, p):
        """The average of parameter p: a view of the flat buffer, shaped like p."""
        return self._views[id(p)]

    def _ptrs(self, ps):
        """Average pointer per parameter of ``ps`` for the launch's table (0 = not tracked)."""
        return [v.data_ptr() if v is not None else 0 for v in (self._views.get(id(p)) for p in ps)]

    def _named(self, model):
        return [(k, p) for k, p in model.named_parameters() if id(p) in self._views]

    def state_dict(self, model):
        """``model.state_dict()`` with every tracked parameter replaced by its average (a detached
        view, as the model's own entries are); buffers are the model's, live."""
        sd = model.state_dict()
        for k, p in self._named(model):
            if k not in sd:
                raise KeyError(f"ModelEMA.state_dict: parameter {k} is not in the model's state dict")
            sd[k] = self._views[id(p)].detach()
        return sd

    @torch.no_grad()
    def load_state_dict(self, sd, model):
        """The averages from ``sd`` (what ``state_dict`` returned; buffers are not read)."""
        for k, p in self._named(model):
            v = sd[k]
            if tuple(v.shape) != tuple(p.shape):
                raise ValueError(f"ModelEMA.load_state_dict: {k} has shape {tuple(v.shape)}, expected {tuple(p.shape)}")
            self._views[id(p)].copy_(v)

    def _swap(self, ps):
        dev = ps[0].device
        shadows, jobs, big = self._followers(ps)
        chunks, nch = self._table_chunks(ps, dev)
        lib.ivit_swap_chunked(len(ps), ptr(self._table(ps, dev)), ptr(self._table_ptrs(self._ptrs(ps), dev)),
                              ptr(self._table_sizes(ps, dev)), ptr(chunks), nch, ptr(self._table_ptrs(shadows, dev)),
                              stream())
        if jobs:
            lib.ivit_weight_pack_multi(len(jobs), ptr(self._pack_jobs(jobs, dev)), big, stream())

    @contextlib.contextmanager
    def swapped(self, model):
        """Inside the block the model's tracked parameters hold the averages and this buffer holds the
        live weights (ivit_swap_chunked, in place); the live bf16 shadows and row-panel packs are
        rewritten from the new weights as FusedAdamW's launch rewrites them, so the forward inside
        is the averaged model's. Swapped back on exit, also when the block raises. Not re-entrant,
        and no optimiser step belongs inside."""
        if self._swapped:
            raise RuntimeError("ModelEMA.swapped: already swapped (nested use)")
        ps = [p for _, p in self._named(model)]
        if not ps:
            raise ValueError("ModelEMA.swapped: the model has none of the tracked parameters")
        with torch.no_grad():
            self._swap(ps)
        self._swapped = True
        try:
            yield self
        finally:
            with torch.no_grad():
                self._swap(ps)
            self._swapped = False


_clip_tables = _Tables()


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False):
    """torch.nn.utils.clip_grad_norm_ (L2 only) on the device: ivit_grad_norm then ivit_grad_scale, no
    host read; returns the total norm before clipping as a 0-d device tensor. The norm is summed in
    f64 and does not depend on the gradients' layout. A non-finite norm leaves the gradients as they
    are (torch would multiply them by a NaN coefficient); ``error_if_nonfinite=True`` costs one host
    read and raises as torch does."""
    if float(norm_type) != 2.0:
        raise ValueError(f"clip_grad_norm_: only norm_type 2 is built (got {norm_type})")
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.0)
    rec = _clip_tables._norm_launch(grads, max_norm, None, None)
    if error_if_nonfinite and not bool(torch.isfinite(rec.norm)):
        raise RuntimeError(f"The total norm of order {float(norm_type)} for gradients from `parameters` is "
                           "non-finite, so it cannot be clipped. To disable this error and scale the gradients "
                           "by the non-finite norm anyway, set `error_if_nonfinite=False`")
    _clip_tables._scale_launch(grads, rec.coef)
    return rec.norm


NO_DECAY_NAMES = ("pos_embed", "cls_token", "mask_token", "decoder_pos_embed")


def layer_decay_param_groups(model, layer_decay=1.0, weight_decay=0.0, no_decay_1d=True):
    """Parameter groups for fine-tuning with layer-wise learning-rate decay (the rule of timm's
    ``param_groups_layer_decay``; BEiT / MAE fine-tuning), for FusedAdamW(..., fuse_groups=True).

    Every vit.VisionTransformer inside ``model`` is a stream of depth L = len(blocks): its
    ``patch_embed.*``, ``cls_token`` and ``pos_embed`` have layer id 0, ``blocks.i.*`` has id i + 1, and
    the rest of it (the final ``norm``) the top id L + 1. Everything outside the streams (adapters,
    fusion block, heads; all of IntentNetCNN) has the top id. A parameter's group carries
    ``lr_scale = layer_decay ** (L + 1 - id)`` (f64) and ``layer_id``; the top id has scale 1.
    ``no_decay_1d``: parameters with ndim <= 1, names ending ``.bias``, and ``pos_embed`` / ``cls_token`` /
    ``mask_token`` / ``decoder_pos_embed`` get ``weight_decay`` 0, the others ``weight_decay``.
    Parameters with equal (lr_scale, weight_decay) share a group; groups appear in the order of their
    first parameter in ``model.named_parameters()`` and keep that order inside, so every construction
    (every DDP rank) builds the same groups. Frozen parameters are left out.
    ``layer_decay=1, no_decay_1d=False`` is the single group of ``model.parameters()``."""
    import vit
    layer_decay, weight_decay = float(layer_decay), float(weight_decay)
    if not 0.0 < layer_decay <= 1.0:  # NaN fails too
        raise ValueError(f"layer_decay must be in (0, 1] (got {layer_decay})")
    streams = [(name + "." if name else "", len(m.blocks)) for name, m in model.named_modules()
               if isinstance(m, vit.VisionTransformer)]
    top = max((depth for _, depth in streams), default=0) + 1
    groups = {}
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        lid, depth = top, top - 1
        for prefix, d in streams:
            if name.startswith(prefix):
                rest, depth = name[len(prefix):], d
                if rest in ("cls_token", "pos_embed") or rest.startswith("patch_embed."):
                    lid = 0
                elif rest.startswith("blocks."):
                    lid = int(rest.split(".")[1]) + 1
                else:
                    lid = d + 1
                break
        scale = layer_decay ** (depth + 1 - lid)
        leaf = name.rsplit(".", 1)[-1]
        no_decay = no_decay_1d and (p.ndim <= 1 or name.endswith(".bias") or leaf in NO_DECAY_NAMES)
        wd = 0.0 if no_decay else weight_decay
        g = groups.setdefault((scale, wd), {"params": [], "lr_scale": scale, "weight_decay": wd, "layer_id": lid})
        g["params"].append(p)
    return list(groups.values())


def group_summary(param_groups):
    """[(layer_id, lr_scale, tensors, elements)] per distinct lr_scale of ``param_groups``, smallest
    scale first: the lines train_vit.py logs."""
    rows = {}
    for g in param_groups:
        r = rows.setdefault(float(g.get("lr_scale", 1.0)), [0, 0, 0])
        r[0] = max(r[0], g.get("layer_id", 0))
        r[1] += len(g["params"])
        r[2] += sum(p.numel() for p in g["params"])
    return [(r[0], s, r[1], r[2]) for s, r in sorted(rows.items())]


class WarmupCosineLR:
    """Linear warmup then cosine decay of every group's ``lr``, stepped once per optimiser update.
    For update k (counted from 0), with W = ``warmup_steps``, T = ``total_steps`` and ``base`` the
    group's lr at construction (kept as the group's ``initial_lr``), in f64:
        k < W:  warmup_init_lr + (base - warmup_init_lr) * k / W
        else:   min_lr + 0.5 * (base - min_lr) * (1 + cos(pi * (k - W) / max(1, T - W))), min_lr once k >= T
    The constructor writes the lr of update 0; ``step()`` (after each ``optimizer.step``) moves to the
    next update. A group's ``lr_scale`` is not touched: it multiplies this lr in the optimiser (the
    kernel's table, with ``fuse_groups``), so a schedule step uploads nothing. The lr is a function of
    the update index alone, hence the same on every rank. An update the device skips (``finite`` = 0)
    still advances the schedule: the host does not read the flag."""

    def __init__(self, optimizer, warmup_steps, total_steps, min_lr=0.0, warmup_init_lr=0.0):
        warmup_steps, total_steps = int(warmup_steps), int(total_steps)
        if warmup_steps < 0 or total_steps <= 0 or warmup_steps > total_steps:
            raise ValueError(f"WarmupCosineLR: need 0 <= warmup_steps <= total_steps, total_steps > 0 "
                             f"(got {warmup_steps}, {total_steps})")
        self.optimizer = optimizer
        self.warmup_steps, self.total_steps = warmup_steps, total_steps
        self.min_lr, self.warmup_init_lr = float(min_lr), float(warmup_init_lr)
        # torch's convention: the base lr stays in the group, so a second schedule on the same optimizer
        # (or one built after load_state_dict) starts from it and not from a scheduled value
        self.base_lrs = [float(g.setdefault("initial_lr", g["lr"])) for g in optimizer.param_groups]
        self.last_step = 0
        self._write()

    def lr_at(self, k, base):
        """The closed form above for update k and a group's base lr."""
        W, T = self.warmup_steps, self.total_steps
        if k < W:
            return self.warmup_init_lr + (base - self.warmup_init_lr) * k / W
        if k >= T:
            return self.min_lr
        return self.min_lr + 0.5 * (base - self.min_lr) * (1.0 + math.cos(math.pi * (k - W) / max(1, T - W)))

    def _write(self):
        for g, base in zip(self.optimizer.param_groups, self.base_lrs):
            g["lr"] = self.lr_at(self.last_step, base)

    def get_last_lr(self):
        return [g["lr"] for g in self.optimizer.param_groups]

    def step(self):
        self.last_step += 1
        self._write()

    def state_dict(self):
        return {k: v for k, v in self.__dict__.items() if k != "optimizer"}

    def load_state_dict(self, sd):
        if len(sd["base_lrs"]) != len(self.optimizer.param_groups):
            raise ValueError(f"WarmupCosineLR.load_state_dict: {len(sd['base_lrs'])} groups saved, the optimizer has "
                             f"{len(self.optimizer.param_groups)}")
        self.__dict__.update(sd)
        self.base_lrs = list(sd["base_lrs"])
        self._write()
