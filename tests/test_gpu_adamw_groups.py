"""Parameter groups in one AdamW launch on the MI355X: ivit_adamw_chunked_pt through
FusedAdamW(fuse_groups=True), optim.layer_decay_param_groups, optim.WarmupCosineLR and the
--layer-decay / --no-decay-1d / --sched cosine entry points.

The comparisons between the fused launch, the launch per group and the existing entry called per group
are bitwise: the table launch forms lr_t = lr * lr_scale as one f32 multiply (the product the host passes
for a group) and keep = fma(-lr_t, wd, 1) as the existing kernels form 1 - lr * wd, so there is no
tolerance to choose. Only the comparison with torch.optim.AdamW has one: relative 1e-6, the bar of
test_adamw_matches_torch (torch multiplies lr and scale in f64; the f32 product is one rounding away).
"""
import math
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

# the storage layout of test_adamw_chunked_bit_identical_to_guarded: several chunks with a ragged last
# one (9000, 12289), exactly one chunk (4096), smaller than a chunk ((37, 5), 384, 1), two views at
# 4-byte offsets (13289, and 13287 for the single element), bf16 shadows on every other tensor
SHAPES = [(9000,), (4096,), (37, 5), (1,), (12289,), (384,)]
OFFS = [0, 9004, 13100, 13287, 13289, 25580]
SIZES = [int(np.prod(s)) for s in SHAPES]
STEPS0 = [3, 3, 7, 3, 7, 5]  # host counts: launches of tensors {0, 1, 3}, {2, 4}, {5} across the groups
GROUPS = [((0, 1), 1.0, 0.0), ((2, 3), 0.75, 1e-2), ((4, 5), 0.75 ** 13, 0.05)]  # (tensors, lr_scale, weight_decay)
LR, B1, B2, EPS = 1e-2, 0.9, 0.999, 1e-8
EMA_DECAY = 0.99
FINITE = (1.0, 0.0, 1.0)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


class _State:
    """One copy of the layout on the device: flat p / g / m / v storage, the views as leaf parameters
    with gradients, shadows on tensors 0, 2, 4 and (optionally) a ModelEMA of the parameters."""

    def __init__(self, ema):
        import ops
        from optim import ModelEMA
        g0 = torch.Generator().manual_seed(3)
        flat = [torch.randn(4 * 20000 + 7, generator=g0) for _ in range(4)]
        self.P, self.G, self.M, self.V = [f.clone().to(DEV) for f in flat]
        self.M.abs_().mul_(0.1)
        self.V.abs_().mul_(0.01)
        view = lambda T: [T[o:o + n].view(sh) for o, n, sh in zip(OFFS, SIZES, SHAPES)]
        self.ps = [v.detach().requires_grad_(True) for v in view(self.P)]
        for p, g in zip(self.ps, view(self.G)):
            p.grad = g
        self.ms, self.vs = view(self.M), view(self.V)
        assert self.ps[4].data_ptr() % 16 == 4 and self.ps[5].data_ptr() % 16 == 0 and self.ps[0].data_ptr() % 16 == 0
        self.shadows = [ops.cast_weight(p, torch.bfloat16) if i % 2 == 0 else None for i, p in enumerate(self.ps)]
        assert all(ops.shadow_of(p) is s for p, s in zip(self.ps, self.shadows) if s is not None)
        self.ema = ModelEMA(self.ps, decay=EMA_DECAY, warmup=True) if ema else None
        self.steps = [float(s) for s in STEPS0]

    def optimizer(self, fuse):
        from optim import FusedAdamW
        opt = FusedAdamW([{"params": [self.ps[i] for i in idx], "lr_scale": sc, "weight_decay": wd}
                          for idx, sc, wd in GROUPS], lr=LR, betas=(B1, B2), eps=EPS, fuse_groups=fuse)
        for p, m, v, s in zip(self.ps, self.ms, self.vs, STEPS0):
            opt.state[p] = {"step": s, "exp_avg": m, "exp_avg_sq": v}
        return opt

    def next_grads(self):
        self.G.mul_(-0.7).add_(0.01)

    def result(self, opt=None):
        torch.cuda.synchronize()
        steps = self.steps if opt is None else [float(opt.state[p]["step"]) for p in self.ps]
        return dict(P=self.P, M=self.M, V=self.V, shadows=[s for s in self.shadows if s is not None], steps=steps,
                    ema=None if self.ema is None else self.ema.flat)


def _raw(st, idx, lr, wd, bc1, bc2s, finite, sin, sout, gs, ema_decay, ema_warm, hyper="existing"):
    """One launch of the tensors ``idx`` of ``st`` through the C ABI. hyper = "existing": the entry
    FusedAdamW calls for these options today; otherwise ivit_adamw_chunked_pt with that table (None = null)."""
    from _lib import lib, ptr, stream
    t64 = lambda vals: torch.tensor(vals, dtype=torch.int64, device=DEV)
    tabs = [t64([T[i].data_ptr() for i in idx]) for T in (st.ps, [p.grad for p in st.ps], st.ms, st.vs)]
    tsh = t64([st.shadows[i].data_ptr() if st.shadows[i] is not None else 0 for i in idx])
    tsz = t64([SIZES[i] for i in idx])
    ce = lib.ivit_adamw_chunk_elems()
    rec = [(t, c) for t, i in enumerate(idx) for c in range(-(-SIZES[i] // ce))]
    ch = torch.tensor(rec, dtype=torch.int32, device=DEV)
    args = (len(idx), *[ptr(t) for t in tabs], ptr(tsh), ptr(tsz), ptr(ch), len(rec), lr, B1, B2, EPS, wd, bc1, bc2s,
            ptr(finite), ptr(sin), ptr(sout))
    te = t64(st.ema._ptrs([st.ps[i] for i in idx])) if st.ema is not None else None
    if hyper != "existing":
        lib.ivit_adamw_chunked_pt(*args, ptr(gs), ptr(te), ema_decay if te is not None else 0.0,
                                  ema_warm if te is not None else 0, ptr(hyper), stream())
    elif te is not None:
        lib.ivit_adamw_chunked_ema(*args, ptr(gs), ptr(te), ema_decay, ema_warm, stream())
    elif gs is not None:
        lib.ivit_adamw_chunked_scaled(*args, ptr(gs), stream())
    else:
        lib.ivit_adamw_chunked(*args, stream())
    torch.cuda.synchronize()  # the tables above are temporaries


def _raw_update(st, counts, fin, gs, groups, hyper_of=None):
    """One update of ``st`` by a raw launch per (tensors, lr, wd) of ``groups``: device counts in one launch
    per group, host counts in one launch per group and distinct count (as FusedAdamW's by_step)."""
    for idx, lr, wd in groups:
        hyper = "existing" if hyper_of is None else hyper_of(idx)
        if counts == "device":
            sin = torch.tensor([st.steps[i] for i in idx], device=DEV)
            sout = torch.empty_like(sin)
            _raw(st, idx, lr, wd, 1.0, 1.0, torch.tensor(fin, device=DEV), sin, sout, gs, EMA_DECAY, 1, hyper)
            for i, s in zip(idx, sout.tolist()):
                st.steps[i] = s
        else:
            finite = torch.tensor(fin, device=DEV)
            by_step = {}
            for i in idx:
                by_step.setdefault(int(st.steps[i]) + 1, []).append(i)
            for step, sub in by_step.items():
                d = st.ema.decay_at(step) if st.ema is not None else 0.0
                hy = "existing" if hyper_of is None else hyper_of(sub)
                _raw(st, sub, lr, wd, 1.0 - B1 ** step, math.sqrt(1.0 - B2 ** step), finite, None, None, gs, d, 0, hy)
                if fin:
                    for i in sub:
                        st.steps[i] = float(step)


def _assert_same(a, b, what):
    for k in ("P", "M", "V"):
        assert torch.equal(a[k], b[k]), (what, k)
    assert len(a["shadows"]) == len(b["shadows"]) == 3
    assert all(torch.equal(x, y) for x, y in zip(a["shadows"], b["shadows"])), (what, "shadows")
    assert a["steps"] == b["steps"], (what, a["steps"], b["steps"])
    assert (a["ema"] is None) == (b["ema"] is None)
    if a["ema"] is not None:
        assert torch.equal(a["ema"], b["ema"]), (what, "ema")


@pytest.mark.parametrize("ema", [False, True], ids=["noema", "ema"])
@pytest.mark.parametrize("scale", [None, 0.37], ids=["noscale", "scale"])
@pytest.mark.parametrize("counts", ["host", "device"])
def test_fused_equals_per_group_bitwise(counts, scale, ema):
    """Run 1 FusedAdamW(fuse_groups=False), run 2 fuse_groups=True, run 3 the existing entry called per
    group with lr = float(np.float32(lr) * np.float32(lr_scale)): three updates with finite = 1, 0, 1 and
    the same bits everywhere. With host counts FusedAdamW has no flag to pass (the host decides, and a
    skipped update is no call at all), so runs 1 and 2 make no call for the middle update while run 3
    passes finite = 0 to the entry with host counts, which must then write nothing."""
    results = []
    for fuse in (False, True):
        st = _State(ema)
        opt = st.optimizer(fuse)
        gs = None if scale is None else torch.tensor(scale, device=DEV)
        for fin in FINITE:
            kw = {} if gs is None else {"grad_scale": gs}
            if counts == "device":
                kw["finite"] = torch.tensor(fin, device=DEV)
            if counts == "device" or fin:
                opt.step_ema(st.ema, **kw) if st.ema is not None else opt.step(**kw)
            st.next_grads()
        results.append(st.result(opt))
    st = _State(ema)
    gs = None if scale is None else torch.tensor(scale, device=DEV)
    groups = [(list(idx), float(np.float32(LR) * np.float32(sc)), wd) for idx, sc, wd in GROUPS]
    assert groups[1][1] != LR * 0.75 or groups[2][1] != LR * 0.75 ** 13  # the f32 products are not the f64 ones
    for fin in FINITE:
        _raw_update(st, counts, fin, gs, groups)
        st.next_grads()
    results.append(st.result())
    _assert_same(results[0], results[1], "unfused vs fused")
    _assert_same(results[0], results[2], "unfused vs existing entry per group")
    fresh = _State(False)
    assert not torch.equal(results[0]["P"], fresh.P) and not torch.equal(results[0]["shadows"][0], fresh.shadows[0])
    want = [s + 2.0 for s in STEPS0]
    assert results[0]["steps"] == want  # the skipped update did not count


@pytest.mark.parametrize("counts", ["host", "device"])
def test_identity_table_and_null_table(counts):
    """ivit_adamw_chunked_pt with (1.0, wd) for every tensor, and with a null table, against
    ivit_adamw_chunked_ema with the scalar wd: the same bits (grad_scale and EMA on, finite = 1, 0, 1)."""
    wd = 1e-2
    allt = list(range(len(SHAPES)))
    results = []
    for mode in ("existing", "identity", "null"):
        st = _State(True)
        gs = torch.tensor(0.37, device=DEV)
        if mode == "existing":
            hyper_of = None
        elif mode == "identity":
            hyper_of = lambda sub: torch.tensor([[1.0, wd]] * len(sub), dtype=torch.float32, device=DEV)
        else:
            hyper_of = lambda sub: None
        for fin in FINITE:
            # the identity table carries the decay: the scalar must then be ignored
            _raw_update(st, counts, fin, gs, [(allt, LR, 7.0 if mode == "identity" else wd)], hyper_of)
            st.next_grads()
        results.append(st.result())
    _assert_same(results[0], results[1], "identity table")
    _assert_same(results[0], results[2], "null table")
    assert not torch.equal(results[0]["P"], _State(False).P)


def test_groups_against_torch_adamw():
    from optim import FusedAdamW
    g = torch.Generator().manual_seed(5)
    init = [torch.randn(*s, generator=g) for s in SHAPES]
    grads = [[torch.randn(*s, generator=g) for s in SHAPES] for _ in range(3)]
    ref = [p.clone().requires_grad_(True) for p in init]
    o_ref = torch.optim.AdamW([{"params": [ref[i] for i in idx], "lr": 1e-3 * sc, "weight_decay": wd}
                               for idx, sc, wd in GROUPS], lr=1e-3)
    devs = []
    for fuse in (False, True):
        dev = [p.clone().to(DEV).requires_grad_(True) for p in init]
        devs.append((dev, FusedAdamW([{"params": [dev[i] for i in idx], "lr_scale": sc, "weight_decay": wd}
                                      for idx, sc, wd in GROUPS], lr=1e-3, fuse_groups=fuse)))
    for step in grads:
        for i, gr in enumerate(step):
            ref[i].grad = gr.clone()
            for dev, _ in devs:
                dev[i].grad = gr.clone().to(DEV)
        o_ref.step()
        for _, o in devs:
            o.step()
    for dev, o in devs:
        for p, q in zip(ref, dev):
            err = _rel(q.detach(), p.detach())
            print(f"fuse_groups={o.fuse_groups} {tuple(p.shape)}: rel {err:.3e}")
            assert err < 1e-6
            assert _rel(o.state[q]["exp_avg_sq"], o_ref.state[p]["exp_avg_sq"]) < 1e-6
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(devs[0][0], devs[1][0]))


@pytest.mark.parametrize("fuse", [False, True], ids=["pergroup", "fused"])
def test_frozen_scale(fuse):
    """lr_scale = 0: the parameter's and the shadow's bits stay, the moments move and the count
    advances; the neighbouring group trains."""
    import ops
    from optim import FusedAdamW
    g = torch.Generator().manual_seed(7)
    frozen = torch.randn(4096 + 37, generator=g)
    frozen[:2] = 0.0
    ps = [frozen.clone().to(DEV).requires_grad_(True), torch.randn(300, generator=g).to(DEV).requires_grad_(True)]
    sh = ops.cast_weight(ps[0], torch.bfloat16)
    sh0 = sh.clone()
    opt = FusedAdamW([{"params": [ps[0]], "lr_scale": 0.0, "weight_decay": 0.05}, {"params": [ps[1]], "lr_scale": 1.0}],
                     lr=1e-2, weight_decay=0.05, fuse_groups=fuse)
    one = torch.ones((), device=DEV)
    before1 = ps[1].detach().clone()
    for k in range(2):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g).to(DEV)
        opt.step(finite=one)
    torch.cuda.synchronize()
    assert torch.equal(ps[0].detach().cpu().view(torch.int32), frozen.view(torch.int32))
    assert torch.equal(sh.view(torch.int16), sh0.view(torch.int16)) and ops.shadow_of(ps[0]) is sh
    st = opt.state[ps[0]]
    assert float(st["step"]) == 2.0 and float(st["exp_avg"].abs().max()) > 0 and float(st["exp_avg_sq"].min()) > 0
    assert not torch.equal(ps[1].detach(), before1)


# ------------------------------------------------------------------ model level
class _Counting:
    """optim.lib with every call counted by entry name."""

    def __init__(self, real):
        self._real, self.calls = real, {}

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not callable(fn):
            return fn

        def counted(*a, **k):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a, **k)
        return counted


@pytest.fixture(scope="module")
def small():
    """The 32x48 bf16 IntentNetViT case of test_gpu_ema.py / test_gpu_grad_clip.py with the
    --layer-decay 0.75 --no-decay-1d groups."""
    import loss as L
    import model_vit
    import utils
    from optim import FusedAdamW, ModelEMA, layer_decay_param_groups
    from oracle import ivit_oracle as O
    from oracle.weights import make_state_dict, model_cfg
    from trainer import Trainer
    sd = make_state_dict(model_cfg(img_size=(32, 48)), seed=0)
    lidar, mp_, gts = O.synthetic_batch(2, (32, 48), seed=1234, box_region=(54.0, 60.0, -72.0, -62.0))
    batch = {"lidar_bev": lidar.to(DEV), "map_bev": mp_.to(DEV), "gt_list": gts}
    anchors = utils.generate_anchors(32, 48, 8, device=DEV)

    def trainer(fuse, ema=False, **kw):
        m = model_vit.IntentNetViT(backbone_cfg={"img_size": (32, 48), "drop_path_rate_lidar": 0.0,
                                                 "drop_path_rate_map": 0.0})
        m.load_state_dict(sd, strict=True)
        m = m.to(DEV).set_compute_dtype(torch.bfloat16).train()
        groups = layer_decay_param_groups(m, 0.75, 0.05, no_decay_1d=True)
        opt = FusedAdamW(groups, lr=1e-3, fuse_groups=fuse)
        e = ModelEMA(m, decay=0.9, warmup=True) if ema else None
        lf = L.DetectionIntentionLoss(apply_intention_downsampling=False)
        return m, Trainer(m, lf, opt, anchors, ema=e, **kw), e

    return dict(batch=batch, trainer=trainer)


@pytest.mark.parametrize("check_nan", [True, False], ids=["hostcounts", "devicecounts"])
def test_one_launch_for_all_groups(small, monkeypatch, check_nan):
    import optim
    counts = {}
    for fuse in (True, False):
        m, tr, _ = small["trainer"](fuse, check_nan=check_nan)
        proxy = _Counting(optim.lib)
        monkeypatch.setattr(optim, "lib", proxy)
        assert tr.step(small["batch"]) is not None
        torch.cuda.synchronize()
        monkeypatch.undo()
        n_groups = len(tr.optimizer.param_groups)
        assert n_groups == 28 and all(p.grad is not None for g in tr.optimizer.param_groups for p in g["params"][:1])
        upd = {k: v for k, v in proxy.calls.items() if k.startswith("ivit_adamw_chunked")}
        import ops
        packed = sum(any(pk is not None for p in g["params"] for pk in ops.packs_of(p)) for g in tr.optimizer.param_groups)
        counts[fuse] = (upd, proxy.calls.get("ivit_weight_pack_multi", 0), packed)
    assert counts[True][:2] == ({"ivit_adamw_chunked_pt": 1}, 1), counts[True]
    upd, packs, packed = counts[False]
    assert sum(upd.values()) == 28 and "ivit_adamw_chunked_pt" not in upd, upd
    # and one pack launch per group that holds packed weights (the groups of 1-D tensors hold none)
    assert packs == packed == counts[True][2] and 12 <= packed <= 28, (packs, packed)


def test_packs_shadows_and_ema_follow_the_fused_update(small):
    """Three Trainer steps with max_grad_norm and the EMA on, fused and per group: weights, bf16 shadows,
    row-panel packs and averages are the same bits, and the shadows / packs are the updated weights'."""
    import ops
    runs = []
    for fuse in (True, False):
        m, tr, ema = small["trainer"](fuse, ema=True, check_nan=False, max_grad_norm=1e-3)
        norms = [tr.step(small["batch"])["grad_norm"].clone() for _ in range(3)]
        torch.cuda.synchronize()
        ps = list(m.parameters())
        shadows = [ops.shadow_of(p) for p in ps]
        packs = [ops.packs_of(p) for p in ps]
        assert sum(s is not None for s in shadows) > 0 and sum(a is not None or b is not None for a, b in packs) > 10
        for p, s in zip(ps, shadows):
            if s is not None:
                assert torch.equal(s, p.detach().to(torch.bfloat16))
        assert tr.clipped == 3
        runs.append((ps, shadows, packs, [ema.ema_of(p) for p in ps], norms))
    (pa, sa, ka, ea, na), (pb, sb, kb, eb, nb) = runs
    assert all(torch.equal(x, y) for x, y in zip(na, nb))
    moved = 0
    for i in range(len(pa)):
        assert torch.equal(pa[i].detach(), pb[i].detach()), i
        assert torch.equal(ea[i], eb[i]), i
        assert (sa[i] is None) == (sb[i] is None) and (sa[i] is None or torch.equal(sa[i], sb[i])), i
        for x, y in zip(ka[i], kb[i]):
            assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), i
        moved += not torch.equal(ea[i], pa[i].detach())
    assert moved > 100


# ------------------------------------------------------------------ entry points
TINY = ["--synthetic", "--epochs", "2", "--batches-per-epoch", "2", "--batch", "2", "--grid", "32x48", "--dtype", "bf16"]


def test_train_vit_finetuning_flags(tmp_path, capsys):
    import eval_vit
    import train_vit
    rc = train_vit.main(TINY + ["--layer-decay", "0.75", "--no-decay-1d", "--sched", "cosine", "--warmup-epochs", "1",
                                "--save-dir", str(tmp_path)])
    assert rc == 0
    out = capsys.readouterr().out
    rows = re.findall(r"layer\s+(\d+): lr scale ([0-9.]+), (\d+) tensors, (\d+) elements", out)
    assert [int(r[0]) for r in rows] == list(range(14)), out
    assert all(abs(float(r[1]) - 0.75 ** (13 - i)) < 6e-7 for i, r in enumerate(rows))
    assert sum(int(r[2]) for r in rows) == 327
    lrs = [float(v) for v in re.findall(r"Summary: .* LR: ([0-9.e+-]+)", out)]
    # 4 updates, 2 of warmup: after epoch 1 the lr of update 2 (the peak), after epoch 2 that of update 4 (the floor)
    assert len(lrs) == 2 and lrs[0] == 1e-4 and lrs[1] < lrs[0], lrs
    d = eval_vit.load_checkpoint(str(tmp_path / "vit_model.pth"), torch.device("cuda"))
    groups = d["optimizer_state_dict"]["param_groups"]
    assert len(groups) == 28 and all("lr_scale" in g for g in groups)
    assert sorted({g["lr_scale"] for g in groups}) == sorted(0.75 ** k for k in range(14))
    assert {g["weight_decay"] for g in groups} == {0.0, train_vit.WEIGHT_DECAY}
    s = d["lr_schedule_state_dict"]
    assert (s["last_step"], s["warmup_steps"], s["total_steps"]) == (4, 2, 4)
    assert all(torch.isfinite(v).all() for v in d["model_state_dict"].values() if v.is_floating_point())


def _entry_as_it_was(argv, seed):
    """The body of train_vit.main before the fine-tuning flags existed, for ``argv``: one parameter group
    through FusedAdamW(model.parameters(), lr 1e-4, wd 1e-4), ReduceLROnPlateau on the epoch mean."""
    import train_vit as T
    from constants import ANCHOR_CONFIGS_PAPER, DOMINANT_CLASSES_FOR_DOWNSAMPLING, INTENTION_DOWNSAMPLE_RATIO
    from loss import DetectionIntentionLoss
    from model_vit import IntentNetViT
    from optim import FusedAdamW
    from synthetic import SyntheticBEVLoader
    from trainer import Trainer
    from utils import generate_anchors
    args = T.parse_args(argv)
    torch.manual_seed(seed)
    device = torch.device("cuda", torch.cuda.current_device())
    H, W = (int(v) for v in args.grid.split("x"))
    loader = SyntheticBEVLoader(args.batch, args.batches_per_epoch, (H, W), rank=0, device=device, resident=True,
                                augment=False)
    model = IntentNetViT(backbone_cfg=T.backbone_cfg((H, W))).to(device)
    model.set_compute_dtype(torch.bfloat16)
    loss_fn = DetectionIntentionLoss(use_rotated_iou=T.USE_ROTATED_IOU, intention_class_weights=None,
                                     apply_intention_downsampling=T.APPLY_INTENTION_DOWNSAMPLING,
                                     dominant_intentions=DOMINANT_CLASSES_FOR_DOWNSAMPLING,
                                     intention_downsample_ratio=INTENTION_DOWNSAMPLE_RATIO).to(device)
    optimizer = FusedAdamW(model.parameters(), lr=1e-4, weight_decay=1e-4)
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, mode='min', factor=0.1, patience=3)
    anchors = generate_anchors(H, W, 8, ANCHOR_CONFIGS_PAPER, device=device)
    trainer = Trainer(model, loss_fn, optimizer, anchors, world=1, bucket_mb=args.bucket_mb, check_nan=True,
                      max_grad_norm=args.clip_grad_norm)
    for _ in range(args.epochs):
        model.train()
        losses = []
        for batch in loader:
            d = trainer.step(batch)
            if d is not None:
                losses.append(float(d["loss"].detach()))
        if losses:
            scheduler.step(sum(losses) / len(losses))
    torch.cuda.synchronize()
    return model.state_dict(), optimizer.state_dict()


def test_train_vit_default_path_is_undisturbed(tmp_path):
    import eval_vit
    import train_vit
    torch.manual_seed(11)
    assert train_vit.main(TINY + ["--save-dir", str(tmp_path)]) == 0
    d = eval_vit.load_checkpoint(str(tmp_path / "vit_model.pth"), torch.device("cuda"))
    assert set(d) == {"epoch", "model_state_dict", "optimizer_state_dict", "backbone_cfg"}
    g = d["optimizer_state_dict"]["param_groups"]
    assert len(g) == 1 and "lr_scale" not in g[0] and (g[0]["lr"], g[0]["weight_decay"]) == (1e-4, 1e-4)
    want, want_opt = _entry_as_it_was(TINY, 11)
    assert list(want) == list(d["model_state_dict"])
    for k, v in want.items():
        assert torch.equal(v, d["model_state_dict"][k].to(v.device)), k
    assert want_opt["param_groups"] == g


def test_pretrain_mae_cosine_and_no_decay(tmp_path, capsys):
    import pretrain_mae
    args = pretrain_mae.parse_args(["--synthetic", "--grid", "32x48", "--batch", "2", "--epochs", "1", "--batches-per-epoch",
                                    "4", "--sched", "cosine", "--warmup-epochs", "0.5", "--no-decay-1d",
                                    "--save-dir", str(tmp_path)])
    out = pretrain_mae.run(args)
    assert len(out["losses"]) == 4 and all(math.isfinite(v) for v in out["losses"])
    text = capsys.readouterr().out
    assert "LR schedule: 2 warmup + cosine over 4 updates" in text and "Weight decay: " in text
    d = torch.load(tmp_path / "mae_lidar.pth", map_location="cpu", weights_only=False)
    groups = d["optimizer_state_dict"]["param_groups"]
    assert sorted(g["weight_decay"] for g in groups) == [0.0, 0.05] and all(g["lr_scale"] == 1.0 for g in groups)
    assert d["lr_schedule_state_dict"]["last_step"] == 4 and groups[0]["lr"] == 0.0
