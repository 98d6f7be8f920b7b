"""Weight EMA on the MI355X: ivit_adamw_chunked_ema / ivit_swap_chunked through optim.ModelEMA and
FusedAdamW.step_ema, Trainer(ema=...), and the --ema-decay / --ema entry points.

Every comparison is bitwise. The launch computes e + omd * (p_new - e) as three f32 operations that
are never fused, with omd = (float)(1 - d) and d formed in f64; the host repeats exactly those three
operations (separate torch ops on CPU tensors) on the weights a twin optimiser without the average
produced, so there is no tolerance to choose.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(2 * 4096 + 5,), (37, 5), (1,), (96, 64), (4097,)]


# ------------------------------------------------------------------ helpers
def _opt_sets(n_sets, seed=2):
    """n_sets identical (params, FusedAdamW, shadow) sets: several chunks with a ragged end, tiny
    tensors, one parameter with a live bf16 shadow, one gradient slot that is a 4-byte-offset view."""
    import ops
    from optim import FusedAdamW
    g = torch.Generator().manual_seed(seed)
    init = [torch.randn(*s, generator=g) for s in SHAPES]
    sets = []
    for _ in range(n_sets):
        ps = [p.clone().to(DEV).requires_grad_(True) for p in init]
        sh = ops.cast_weight(ps[3], torch.bfloat16)
        slot = torch.zeros(4097 + 1, device=DEV)
        ps[4].grad = slot[1:]
        sets.append((ps, FusedAdamW(ps, lr=1e-2, weight_decay=1e-2), sh))
    return sets, init


def _set_grads(ps, grads):
    for p, g in zip(ps, grads):
        if g is None:
            p.grad = None
        elif p.grad is not None and p.grad.data_ptr() % 16 != 0:
            p.grad.copy_(g)  # keep the unaligned view
        else:
            p.grad = g.clone().to(DEV)


def _same_state(a, b):
    (pa, oa, sa), (pb, ob, sb) = a, b
    torch.cuda.synchronize()
    for p, q in zip(pa, pb):
        assert torch.equal(p.detach(), q.detach())
        assert bool(oa.state[p]) == bool(ob.state[q])
        if oa.state[p]:
            for k in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(oa.state[p][k], ob.state[q][k]), k
            assert float(oa.state[p]["step"]) == float(ob.state[q]["step"])
    assert torch.equal(sa, sb)
    assert torch.equal(sa, pa[3].detach().to(torch.bfloat16))


def _host_ema(e, p, d):
    """e + omd * (p - e) on the host: three separate f32 ops, omd = float32(1 - d) with d in f64."""
    omd = torch.tensor(np.float32(1.0 - d))
    assert omd.dtype == torch.float32
    diff = p - e
    mv = diff * omd
    return e + mv


def _ema_with_offset_view(ps, decay, warmup):
    """ModelEMA over ps whose average of ps[0] (two full chunks + a ragged one) is replaced by a view
    4 bytes off a 16-byte boundary: those chunks must leave the 16-byte path."""
    from optim import ModelEMA
    ema = ModelEMA(ps, decay=decay, warmup=warmup)
    assert all(ema.ema_of(p).data_ptr() % 16 == 0 and ema.ema_of(p).shape == p.shape for p in ps)
    assert all(torch.equal(ema.ema_of(p), p.detach()) for p in ps)
    slot = torch.zeros(ps[0].numel() + 1, device=DEV)
    assert slot.data_ptr() % 16 == 0
    slot[1:].copy_(ps[0].detach())
    ema._views[id(ps[0])] = slot[1:].view_as(ps[0])
    assert ema.ema_of(ps[0]).data_ptr() % 16 == 4
    return ema


def _emas(ema, ps):
    torch.cuda.synchronize()
    return [ema.ema_of(p).detach().cpu().clone() for p in ps]


# ------------------------------------------------------------------ 1. bits against the recurrence
@pytest.mark.parametrize("decay,warmup", [(0.5, True), (0.5, False), (0.9998, True), (0.9998, False), (0.1, True)])
def test_ema_bits_against_the_recurrence(decay, warmup):
    sets, init = _opt_sets(6)
    (Ad, Bd, Ah, Bh, As, Bs) = sets  # A: with the average, B: its twin without; device / host counts / scaled
    emas = {id(S): _ema_with_offset_view(S[0], decay, warmup) for S in (Ad, Ah, As)}
    ref = {id(S): [t.clone() for t in init] for S in (Ad, Ah, As)}
    one = torch.ones((), device=DEV)
    g = torch.Generator().manual_seed(9)
    bound = []
    for n in (1, 2, 3):
        grads = [torch.randn(*s, generator=g) for s in SHAPES]
        for S in sets:
            _set_grads(S[0], grads)
        Ad[1].step_ema(emas[id(Ad)], finite=one)
        Bd[1].step(finite=one)
        Ah[1].step_ema(emas[id(Ah)])
        Bh[1].step()
        gn = As[1].grad_norm(20.0, finite=one)
        As[1].step_ema(emas[id(As)], finite=gn.finite, grad_scale=gn.coef)
        gn2 = Bs[1].grad_norm(20.0, finite=one)
        Bs[1].step(finite=gn2.finite, grad_scale=gn2.coef)
        assert float(gn.coef) < 1.0  # the scaled path did scale
        d = emas[id(Ad)].decay_at(n)
        bound.append(d < decay)
        for A, B in ((Ad, Bd), (Ah, Bh), (As, Bs)):
            _same_state(A, B)
            assert all(float(A[1].state[p]["step"]) == n for p in A[0])
            got = _emas(emas[id(A)], A[0])
            ref[id(A)] = [_host_ema(e, q.detach().cpu(), d) for e, q in zip(ref[id(A)], B[0])]
            for k, (x, y) in enumerate(zip(got, ref[id(A)])):
                assert torch.equal(x, y), (n, k, float((x - y).abs().max()))
        for x, y in zip(_emas(emas[id(Ad)], Ad[0]), _emas(emas[id(Ah)], Ah[0])):  # device counts == host counts
            assert torch.equal(x, y)
    assert not torch.equal(Ad[0][0].detach(), As[0][0].detach())  # clipping changed the update
    assert not torch.equal(ref[id(Ad)][0], init[0])  # and the average moved
    # the ramp binds exactly where it should: this parametrisation covers both cases
    if warmup and decay == 0.9998:
        assert bound == [True, True, True]
    if warmup and decay == 0.5:
        assert bound == [True, True, True]  # (1 + n) / (10 + n) < 1/2 up to n = 7
    if not warmup or decay == 0.1:
        assert bound == [False, False, False]


# ------------------------------------------------------------------ 2. skips
def test_skipped_updates_leave_the_average_alone():
    from optim import ModelEMA
    (A, B), init = _opt_sets(2)
    decay = 0.9998  # the ramp binds, so the decay of a step tells which count the launch used
    ema = ModelEMA(A[0], decay=decay, warmup=True)
    one = torch.ones((), device=DEV)
    g = torch.Generator().manual_seed(4)
    ref = [t.clone() for t in init]

    def both(grads):
        _set_grads(A[0], grads)
        _set_grads(B[0], grads)
        gn = A[1].grad_norm(20.0, finite=one)
        A[1].step_ema(ema, finite=gn.finite, grad_scale=gn.coef)
        gb = B[1].grad_norm(20.0, finite=one)
        B[1].step(finite=gb.finite, grad_scale=gb.coef)
        return float(gn.finite)

    # step 1, clean: n = 1
    assert both([torch.randn(*s, generator=g) for s in SHAPES]) == 1.0
    ref = [_host_ema(e, q.detach().cpu(), ema.decay_at(1)) for e, q in zip(ref, B[0])]
    assert all(torch.equal(x, y) for x, y in zip(_emas(ema, A[0]), ref))
    # step 2, a poisoned gradient: finite = 0, nothing moves, the count stays at 1
    grads = [torch.randn(*s, generator=g) for s in SHAPES]
    grads[1][17, 3] = float("inf")
    before = _emas(ema, A[0])
    assert both(grads) == 0.0
    _same_state(A, B)
    assert all(torch.equal(x, y) for x, y in zip(_emas(ema, A[0]), before))
    assert all(float(A[1].state[p]["step"]) == 1.0 for p in A[0])
    # step 3, clean: the launch uses n = 2 (3/12), not 3 (4/13)
    assert both([torch.randn(*s, generator=g) for s in SHAPES]) == 1.0
    _same_state(A, B)
    assert ema.decay_at(2) != ema.decay_at(3)
    ref = [_host_ema(e, q.detach().cpu(), ema.decay_at(2)) for e, q in zip(ref, B[0])]
    assert all(torch.equal(x, y) for x, y in zip(_emas(ema, A[0]), ref))
    # step 4: a parameter without a gradient keeps its average (and its count, 2; the others reach 3)
    grads = [torch.randn(*s, generator=g) for s in SHAPES]
    grads[1] = None
    before = _emas(ema, A[0])
    assert both(grads) == 1.0
    _same_state(A, B)
    got = _emas(ema, A[0])
    assert torch.equal(got[1], before[1]) and float(A[1].state[A[0][1]]["step"]) == 2.0
    ref = [e if k == 1 else _host_ema(e, q.detach().cpu(), ema.decay_at(3)) for k, (e, q) in enumerate(zip(ref, B[0]))]
    assert all(torch.equal(x, y) for x, y in zip(got, ref))
    assert not torch.equal(got[0], before[0])
    # the same two cases on the host-count path
    (C, D), init = _opt_sets(2)
    emc = ModelEMA(C[0], decay=decay, warmup=True)
    refc = [t.clone() for t in init]
    for n, drop in ((1, None), (2, 1)):
        grads = [torch.randn(*s, generator=g) for s in SHAPES]
        if drop is not None:
            grads[drop] = None
        _set_grads(C[0], grads)
        _set_grads(D[0], grads)
        C[1].step_ema(emc)
        D[1].step()
        _same_state(C, D)
        refc = [e if k == drop else _host_ema(e, q.detach().cpu(), emc.decay_at(n))
                for k, (e, q) in enumerate(zip(refc, D[0]))]
        assert all(torch.equal(x, y) for x, y in zip(_emas(emc, C[0]), refc))


def test_null_entry_leaves_that_tensor_unaveraged():
    from optim import ModelEMA
    (A, B), init = _opt_sets(2)
    tracked = [p for k, p in enumerate(A[0]) if k != 3]  # the shadowed weight is not averaged
    ema = ModelEMA(tracked, decay=0.5, warmup=False)
    assert ema._ptrs(A[0])[3] == 0 and all(v != 0 for k, v in enumerate(ema._ptrs(A[0])) if k != 3)
    with pytest.raises(KeyError):
        ema.ema_of(A[0][3])
    flat0 = ema.flat.clone()
    one = torch.ones((), device=DEV)
    g = torch.Generator().manual_seed(6)
    for finite in (one, None):
        grads = [torch.randn(*s, generator=g) for s in SHAPES]
        _set_grads(A[0], grads)
        _set_grads(B[0], grads)
        A[1].step_ema(ema, finite=finite)
        B[1].step(finite=finite)
        _same_state(A, B)
    assert not torch.equal(ema.flat, flat0)
    for p in tracked:  # the others did move, and (decay 0.5) lag behind the weights
        assert not torch.equal(ema.ema_of(p), p.detach())
    # ema=None is step
    A[1].step_ema(None, finite=one)
    B[1].step(finite=one)
    _same_state(A, B)


# ------------------------------------------------------------------ 3. layout
def _vit(sd):
    import model_vit
    m = model_vit.IntentNetViT(backbone_cfg={"img_size": (32, 48), "drop_path_rate_lidar": 0.0,
                                             "drop_path_rate_map": 0.0})
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).set_compute_dtype(torch.bfloat16).train()


def _weights(m):
    torch.cuda.synchronize()
    return torch.cat([p.detach().reshape(-1) for p in m.parameters()]).clone()


def _averages(ema, m):
    torch.cuda.synchronize()
    return torch.cat([ema.ema_of(p).detach().reshape(-1) for p in m.parameters()]).clone()


@pytest.fixture(scope="module")
def small():
    """The 32x48 bf16 IntentNetViT case and the run without the average on the device-count path:
    its weights at the start and after one and two steps."""
    import loss as L
    import utils
    from optim import FusedAdamW
    from oracle import ivit_oracle as O
    from oracle.weights import make_state_dict, model_cfg
    from trainer import Trainer
    sd = make_state_dict(model_cfg(img_size=(32, 48)), seed=0)
    lidar, mp_, gts = O.synthetic_batch(2, (32, 48), seed=1234, box_region=(54.0, 60.0, -72.0, -62.0))
    batch = {"lidar_bev": lidar.to(DEV), "map_bev": mp_.to(DEV), "gt_list": gts}
    anchors = utils.generate_anchors(32, 48, 8, device=DEV)

    def trainer(ema=None, **kw):
        """ema: None, or (decay, warmup) for a ModelEMA of the new model."""
        from optim import ModelEMA
        m = _vit(sd)
        lf = L.DetectionIntentionLoss(apply_intention_downsampling=False)
        e = None if ema is None else ModelEMA(m, decay=ema[0], warmup=ema[1])
        return m, Trainer(m, lf, FusedAdamW(m.parameters(), lr=1e-4, weight_decay=1e-4), anchors, ema=e, **kw), e

    m, tr, _ = trainer(check_nan=False)
    w0 = _weights(m)
    tr.step(batch)
    w1 = _weights(m)
    tr.step(batch)
    return dict(sd=sd, batch=batch, anchors=anchors, trainer=trainer, w0=w0, w1=w1, w2=_weights(m))


def test_layout_of_the_flat_buffer(small):
    from optim import ModelEMA
    m = _vit(small["sd"])
    ema = ModelEMA(m)
    assert ema.decay == 0.9998 and ema.warmup is True
    ps = list(m.parameters())
    assert len(ps) > 100 and any(p.numel() % 4 for p in ps)  # odd sizes are there to be padded
    spans = []
    for p in ps:
        v = ema.ema_of(p)
        assert v.data_ptr() % 16 == 0 and v.shape == p.shape and v.dtype == torch.float32 and v.is_contiguous()
        assert v.untyped_storage().data_ptr() == ema.flat.untyped_storage().data_ptr()
        spans.append((v.data_ptr(), v.data_ptr() + 4 * v.numel()))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    assert spans[0][0] >= ema.flat.data_ptr() and spans[-1][1] <= ema.flat.data_ptr() + 4 * ema.flat.numel()
    sd, se = m.state_dict(), ema.state_dict(m)
    assert list(sd) == list(se)
    names = {k for k, _ in m.named_parameters()}
    for k in sd:
        assert torch.equal(sd[k], se[k]) and sd[k].shape == se[k].shape and sd[k].dtype == se[k].dtype, k
        assert (se[k].data_ptr() == sd[k].data_ptr()) == (k not in names), k  # buffers live, parameters averaged
    # load_state_dict puts averages back
    other = {k: (v + 1.0 if k in names else v) for k, v in se.items()}
    ema.load_state_dict(other, m)
    assert all(torch.equal(ema.ema_of(p), p.detach() + 1.0) for p in ps)


# ------------------------------------------------------------------ 4. Trainer
@pytest.mark.parametrize("check_nan", [False, True])
def test_trainer_ema(small, check_nan):
    batch = small["batch"]
    m, tr, ema = small["trainer"](ema=(0.9, False), check_nan=check_nan)
    assert torch.equal(_averages(ema, m), small["w0"])
    d = tr.step(batch)
    assert d is not None and "grad_norm" not in d
    assert torch.equal(_weights(m), small["w1"])
    e1 = _host_ema(small["w0"].cpu(), small["w1"].cpu(), 0.9)
    assert torch.equal(_averages(ema, m).cpu(), e1)
    tr.step(batch)
    assert torch.equal(_weights(m), small["w2"])
    e2 = _host_ema(e1, small["w2"].cpu(), 0.9)
    assert torch.equal(_averages(ema, m).cpu(), e2)
    assert not torch.equal(e2, small["w2"].cpu()) and tr.skipped == 0 and tr.nonfinite == 0


def test_trainer_ema_with_clipping_and_buckets(small):
    batch = small["batch"]
    # with max_grad_norm: the clipped run's weights, and the average of those
    mc, trc, _ = small["trainer"](check_nan=False, max_grad_norm=1e-3)
    m, tr, ema = small["trainer"](ema=(0.9, False), check_nan=False, max_grad_norm=1e-3)
    e = small["w0"].cpu()
    for _ in range(2):
        dc, d = trc.step(batch), tr.step(batch)
        assert torch.equal(d["grad_norm"], dc["grad_norm"])
        w = _weights(mc)
        assert torch.equal(_weights(m), w)
        e = _host_ema(e, w.cpu(), 0.9)
        assert torch.equal(_averages(ema, m).cpu(), e)
    assert tr.clipped == 2 and not torch.equal(_weights(m), small["w2"])
    # gradient buckets (other gradient addresses): the same weights, the same average
    mb, trb, emb = small["trainer"](ema=(0.9, False), check_nan=False, force_buckets=True, bucket_mb=8)
    assert trb.buckets is not None and len(trb.buckets.buckets) > 1
    trb.step(batch)
    trb.step(batch)
    assert torch.equal(_weights(mb), small["w2"])
    e2 = _host_ema(_host_ema(small["w0"].cpu(), small["w1"].cpu(), 0.9), small["w2"].cpu(), 0.9)
    assert torch.equal(_averages(emb, mb).cpu(), e2)


# ------------------------------------------------------------------ 5. swap
def _eval_outputs(m, batch):
    m.eval()
    with torch.no_grad():  # the shadows this forward caches are read by the training steps that follow
        out = m(batch["lidar_bev"], batch["map_bev"])
    torch.cuda.synchronize()
    m.train()
    return [o.clone() for o in out]


def test_swapped_puts_the_average_into_the_model(small):
    import ops
    batch = small["batch"]
    m, tr, ema = small["trainer"](ema=(0.9, False), check_nan=False)
    m2, tr2, ema2 = small["trainer"](ema=(0.9, False), check_nan=False)  # never swapped
    for t in (tr, tr2):
        t.step(batch)
        t.step(batch)
    live_w, avg = _weights(m), _averages(ema, m)
    assert not torch.equal(live_w, avg)
    live_out = _eval_outputs(m, batch)
    fresh = _vit({k: v.clone() for k, v in ema.state_dict(m).items()})
    ref_out = _eval_outputs(fresh, batch)
    assert not all(torch.equal(a, b) for a, b in zip(live_out, ref_out))  # the two models do differ
    # the training and eval forwards above left live shadows and row-panel packs behind: they must follow
    shadowed = [p for p in m.parameters() if ops.shadow_of(p) is not None]
    packed = [p for p in m.parameters() if any(x is not None for x in ops.packs_of(p))]
    assert shadowed and packed
    with ema.swapped(m) as inside:
        assert inside is ema
        assert torch.equal(_weights(m), avg) and torch.equal(_averages(ema, m), live_w)
        for p in shadowed:
            assert torch.equal(ops.shadow_of(p), p.detach().to(torch.bfloat16))
        out = _eval_outputs(m, batch)
        for k, (a, b) in enumerate(zip(out, ref_out)):
            assert torch.equal(a, b), (k, float((a.float() - b.float()).abs().max()))
        with pytest.raises(RuntimeError, match="nested"):
            with ema.swapped(m):
                pass
        with pytest.raises(RuntimeError, match="swapped"):
            tr.optimizer.step_ema(ema)  # no optimiser step while the live weights sit in the EMA buffer
    assert torch.equal(_weights(m), live_w) and torch.equal(_averages(ema, m), avg)
    for a, b in zip(_eval_outputs(m, batch), live_out):
        assert torch.equal(a, b)
    # an exception inside the block still swaps back
    with pytest.raises(ZeroDivisionError):
        with ema.swapped(m):
            assert torch.equal(_weights(m), avg)
            1 / 0
    assert torch.equal(_weights(m), live_w) and torch.equal(_averages(ema, m), avg)
    with ema.swapped(m):  # and it can be entered again
        pass
    # one further train step: the bits of the run that never swapped
    tr.step(batch)
    tr2.step(batch)
    assert torch.equal(_weights(m), _weights(m2))
    assert torch.equal(_averages(ema, m), _averages(ema2, m2))


# ------------------------------------------------------------------ 6. raw swap
def test_raw_swap():
    from _lib import lib, ptr, stream
    g = torch.Generator().manual_seed(12)
    va = [torch.randn(*s, generator=g) for s in SHAPES]
    vb = [torch.randn(*s, generator=g) for s in SHAPES]
    a = [v.clone().to(DEV) for v in va]
    b = [v.clone().to(DEV) for v in vb]
    slot = torch.zeros(4097 + 1, device=DEV)  # b of the 4097-element tensor: 4 bytes off, so it goes scalar;
    # the three-chunk tensor takes the 16-byte path without a shadow, the 96x64 one with
    slot[1:].copy_(vb[4])
    b[4] = slot[1:]
    sh = [None, torch.zeros(37, 5, dtype=torch.bfloat16, device=DEV), None,
          torch.zeros(96, 64, dtype=torch.bfloat16, device=DEV), torch.zeros(4097, dtype=torch.bfloat16, device=DEV)]
    ce = lib.ivit_adamw_chunk_elems()
    rec = [(t, c) for t, x in enumerate(a) for c in range(-(-x.numel() // ce))]
    ch = torch.tensor(rec, dtype=torch.int32, device=DEV).reshape(len(rec), 2)
    tab = lambda ts: torch.tensor([0 if x is None else x.data_ptr() for x in ts], dtype=torch.int64, device=DEV)
    ta, tb, tsh = tab(a), tab(b), tab(sh)
    sz = torch.tensor([x.numel() for x in a], dtype=torch.int64, device=DEV)

    def swap(shadows):
        assert lib.ivit_swap_chunked(len(a), ptr(ta), ptr(tb), ptr(sz), ptr(ch), len(rec), ptr(shadows), stream()) == 0
        torch.cuda.synchronize()

    swap(tsh)
    for k in range(len(a)):
        assert torch.equal(a[k].cpu(), vb[k]) and torch.equal(b[k].cpu(), va[k]), k
        if sh[k] is not None:
            assert torch.equal(sh[k].cpu(), vb[k].to(torch.bfloat16)), k
    assert float(slot[0]) == 0.0  # nothing written in front of the offset view
    swap(None)  # no shadow table at all; twice is the identity
    for k in range(len(a)):
        assert torch.equal(a[k].cpu(), va[k]) and torch.equal(b[k].cpu(), vb[k]), k
        if sh[k] is not None:
            assert torch.equal(sh[k].cpu(), vb[k].to(torch.bfloat16)), k  # untouched by the second call


# ------------------------------------------------------------------ 7. entry points
def test_entry_points_save_and_evaluate_the_average(tmp_path, capsys):
    import eval_vit
    import train_vit
    common = ["--synthetic", "--dtype", "bf16", "--grid", "32x48", "--epochs", "1", "--batches-per-epoch", "2",
              "--batch", "2"]
    with_ema, without = tmp_path / "ema", tmp_path / "plain"
    assert train_vit.main(common + ["--ema-decay", "0.9", "--save-dir", str(with_ema)]) == 0
    assert "Weight EMA: decay 0.9, warmup True" in capsys.readouterr().out
    ck = eval_vit.load_checkpoint(str(with_ema / "vit_model.pth"), torch.device("cuda"))
    assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "backbone_cfg", "ema_state_dict",
                       "ema_decay", "ema_warmup"}
    assert ck["ema_decay"] == 0.9 and ck["ema_warmup"] is True
    sd, se = ck["model_state_dict"], ck["ema_state_dict"]
    assert list(sd) == list(se) and all(sd[k].shape == se[k].shape and sd[k].dtype == se[k].dtype for k in sd)
    moved = [k for k in sd if not torch.equal(sd[k], se[k])]
    assert len(moved) > 100 and all("running_" not in k and "num_batches" not in k for k in moved)
    ev = ["--synthetic", "--batch", "2", "--batches", "1", "--grid", "32x48"]
    assert eval_vit.main_eval_vit(ev + ["--ema", "--checkpoint", str(with_ema / "vit_model.pth")]) == 0
    out = capsys.readouterr().out
    assert "Evaluating the EMA weights ('ema_state_dict', decay 0.9, warmup True)" in out and "Finished" in out
    # without the flag: today's four keys, and --ema on that checkpoint is an error, not a fallback
    assert train_vit.main(common + ["--save-dir", str(without)]) == 0
    assert "Weight EMA" not in capsys.readouterr().out
    ck = eval_vit.load_checkpoint(str(without / "vit_model.pth"), torch.device("cuda"))
    assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "backbone_cfg"}
    assert eval_vit.main_eval_vit(ev + ["--ema", "--checkpoint", str(without / "vit_model.pth")]) == 1
    out = capsys.readouterr().out
    assert "ERROR: --ema: no 'ema_state_dict'" in out and "Detection Results" not in out


def test_cnn_step_moves_the_average():
    import loss as L
    import model_cnn
    import utils
    from optim import FusedAdamW, ModelEMA
    from oracle import ivit_oracle as O
    from oracle.weights import fill_state_dict
    from trainer import Trainer
    m = model_cnn.IntentNetCNN()
    m.load_state_dict(fill_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed=0), strict=True)
    m = m.to(DEV).set_compute_dtype(torch.bfloat16).train()
    lidar, mp_, gts = O.synthetic_batch(2, (32, 48), seed=1234)
    w0 = _weights(m)
    ema = ModelEMA(m, decay=0.9, warmup=False)
    tr = Trainer(m, L.DetectionIntentionLoss(), FusedAdamW(m.parameters(), lr=1e-4, weight_decay=1e-4),
                 utils.generate_anchors(32, 48, 8, device=DEV), check_nan=True, ema=ema)
    d = tr.step({"lidar_bev": lidar.to(DEV), "map_bev": mp_.to(DEV), "gt_list": gts})
    assert d is not None and tr.nonfinite == 0
    w1 = _weights(m)
    assert not torch.equal(w1, w0)
    assert torch.equal(_averages(ema, m).cpu(), _host_ema(w0.cpu(), w1.cpu(), 0.9))
