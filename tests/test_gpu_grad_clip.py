"""Gradient-norm clipping on the MI355X: ivit_grad_norm / ivit_grad_scale / ivit_adamw_chunked_scaled
through the C ABI, optim.clip_grad_norm_ and FusedAdamW.grad_norm / step(grad_scale=...), and
Trainer(max_grad_norm=...) on one GPU and on two ranks.

Bounds used below, and where they come from:
* norm: 2 f32 ulps of the f64 reference. The kernel's f64 sum of exact squares is good to ~1e-12
  relative; then one rounding in the f64 sqrt and one in the cast to f32.
* coef = fl(max_norm / fl(norm + 1e-6)): a norm off by <= 2 ulps (<= 2 * 2^-23 relative) moves the
  rounded sum by at most that plus two half-ulp roundings (3 * 2^-23), and the rounded quotient by
  that plus two more half-ulp roundings: 4 * 2^-23 = 2^-21 relative.
"""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))

SIZES = [0, 1, 3, 4095, 4096, 4097, 2 * 4096 + 5, 37 * 5]
SCALES = [1.0, 1e-30, 1e-20, 1e-5, 1.0, 1e10, 1e25, 1e20]


def _values(sizes=SIZES, scales=SCALES, seed=11):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, generator=g, dtype=torch.float64) * s).float() for n, s in zip(sizes, scales)]


def _ref_norm(vals):
    return float(torch.linalg.vector_norm(torch.cat([v.double().reshape(-1) for v in vals])))


def _within_ulps(got, ref64, ulps=2):
    r32 = np.float32(ref64)
    return abs(float(got) - ref64) <= ulps * float(np.spacing(r32))


def _ref_coef(ref64, max_norm):
    with np.errstate(over="ignore"):
        q = np.float32(max_norm) / (np.float32(ref64) + np.float32(1e-6))
    return float(min(np.float32(1.0), q))


def _separate(vals):
    """Each tensor in its own allocation, but the 4097-element one as a view 4 bytes off a 16-byte
    boundary."""
    out = []
    for v in vals:
        if v.numel() == 4097:
            flat = torch.zeros(v.numel() + 1, device=DEV)
            assert flat.data_ptr() % 16 == 0
            flat[1:].copy_(v)
            out.append(flat[1:])
        else:
            out.append(v.clone().to(DEV))
    return out


def _flat(vals, aligned):
    """Views of one flat buffer: every view on a 16-byte boundary, or packed end to end behind a
    one-float lead (so most views start 4, 8 or 12 bytes off)."""
    offs, n = [], 0 if aligned else 1
    for v in vals:
        offs.append(n)
        n += (v.numel() + 3) // 4 * 4 if aligned else v.numel()
    flat = torch.zeros(n + 4, device=DEV)
    views = []
    for v, o in zip(vals, offs):
        flat[o:o + v.numel()].copy_(v)
        views.append(flat[o:o + v.numel()])
    if not aligned:
        assert any(t.data_ptr() % 16 != 0 for t in views if t.numel())
    else:
        assert all(t.data_ptr() % 16 == 0 for t in views if t.numel())
    return views


def _raw_norm(tensors, max_norm, finite=None, stats=None):
    """ivit_grad_norm straight through the C ABI -> the [norm, coef, finite, 0] record."""
    from _lib import lib, ptr, stream
    ce = lib.ivit_adamw_chunk_elems()
    rec = [(t, c) for t, x in enumerate(tensors) for c in range(-(-x.numel() // ce))]
    ch = torch.tensor(rec, dtype=torch.int32, device=DEV).reshape(len(rec), 2)
    tab = torch.tensor([x.data_ptr() for x in tensors], dtype=torch.int64, device=DEV)
    sz = torch.tensor([x.numel() for x in tensors], dtype=torch.int64, device=DEV)
    nb = lib.ivit_grad_norm_workspace(len(rec))
    ws = torch.empty(nb // 8, dtype=torch.float64, device=DEV)
    out = torch.full((4,), -7.0, device=DEV)
    assert lib.ivit_grad_norm(len(tensors), ptr(tab), ptr(sz), ptr(ch) if rec else None, len(rec), max_norm,
                              ptr(finite), ptr(ws), nb, ptr(out), ptr(stats), stream()) == 0
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------ 1. norm against f64
def test_norm_and_coef_against_f64():
    vals = _values()
    ref = _ref_norm(vals)
    assert ref > 1e26 and ref * ref > float(np.finfo(np.float32).max)  # an f32 sum of squares would overflow
    ts = _separate(vals)
    for max_norm in (1e20, 3e38):  # clipped hard / not clipped
        r = _raw_norm(ts, max_norm).cpu()
        print(f"norm {float(r[0]):.9e} ref {ref:.9e} coef {float(r[1]):.9e} ref {_ref_coef(ref, max_norm):.9e}")
        assert _within_ulps(r[0], ref), (float(r[0]), ref)
        rc = _ref_coef(ref, max_norm)
        assert abs(float(r[1]) - rc) <= 2.0 ** -21 * rc, (float(r[1]), rc)
        assert float(r[2]) == 1.0 and float(r[3]) == 0.0
    assert float(_raw_norm(ts, 3e38)[1]) == 1.0
    # the small tensors alone: their squares (1e-60, 1e-40) are below f32's range, the norm is not
    small = [t for t, s in zip(ts, SCALES) if s <= 1e-20]
    rs = _ref_norm([v for v, s in zip(vals, SCALES) if s <= 1e-20])
    assert 1e-21 < rs < 1e-18
    r = _raw_norm(small, 1.0).cpu()
    assert _within_ulps(r[0], rs), (float(r[0]), rs)
    assert float(r[1]) == 1.0
    # nothing to sum: pass 2 alone writes norm 0, coef 1 (no tensors; one empty tensor)
    for empty in ([], [ts[0]]):
        r = _raw_norm(empty, 2.0).cpu()
        assert r.tolist() == [0.0, 1.0, 1.0, 0.0]
    # the incoming flag is folded into the record's
    assert float(_raw_norm(ts, 1.0, finite=torch.zeros((), device=DEV))[2]) == 0.0
    assert float(_raw_norm(ts, 1.0, finite=torch.ones((), device=DEV))[2]) == 1.0


# ------------------------------------------------------------------ 2. layout independence
def test_norm_bits_do_not_depend_on_layout():
    vals = _values()
    recs = []
    for layout in (_separate(vals), _flat(vals, aligned=False), _flat(vals, aligned=True)):
        for _ in range(2):
            recs.append(_raw_norm(layout, 1e20).view(torch.int32).cpu())
    for r in recs[1:]:
        assert torch.equal(r, recs[0]), (r, recs[0])
    # values of ordinary size too (every partial matters to the low bits here)
    vals = _values(scales=[1.0] * len(SIZES), seed=5)
    recs = [_raw_norm(lay, 10.0).view(torch.int32).cpu()
            for lay in (_separate(vals), _flat(vals, aligned=False), _flat(vals, aligned=True))]
    assert torch.equal(recs[0], recs[1]) and torch.equal(recs[0], recs[2])
    assert _within_ulps(recs[0].view(torch.float32)[0], _ref_norm(vals))


def test_norm_many_partials():
    """More chunks than pass 2 has threads (1024), and than one round of its eight-deep loads (8192):
    8300 tiny tensors, one chunk each, packed with and without 16-byte alignment."""
    vals = _values(sizes=[(1, 2, 3, 5, 7)[i % 5] for i in range(8300)], scales=[1.0] * 8300, seed=3)
    recs = [_raw_norm(lay, 10.0).view(torch.int32).cpu()
            for lay in (_flat(vals, aligned=False), _flat(vals, aligned=True), _flat(vals[:1500], aligned=False))]
    assert torch.equal(recs[0], recs[1])
    assert _within_ulps(recs[0].view(torch.float32)[0], _ref_norm(vals))
    assert _within_ulps(recs[2].view(torch.float32)[0], _ref_norm(vals[:1500]))


# ------------------------------------------------------------------ 3. clip_grad_norm_ against torch
def _rel_l2(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float((a - b).norm() / b.norm())


def test_clip_grad_norm_matches_torch():
    import optim
    torch.manual_seed(0)
    ps = [torch.randn(1000), torch.randn(37, 5), torch.randn(4097)]
    gs = [[torch.randn_like(p) * (1e-3 if k == 2 else 1.0) for p in ps] for k in range(3)]
    max_norm = 30.0  # ||g|| ~ sqrt(5282) = 72.7: steps 1, 2 clip (coef ~0.41), the 1e-3 step does not
    r32 = [p.clone().requires_grad_(True) for p in ps]
    r64 = [p.double().clone().requires_grad_(True) for p in ps]
    dev = [p.clone().to(DEV).requires_grad_(True) for p in ps]
    o32 = torch.optim.AdamW(r32, lr=1e-3, weight_decay=1e-2)
    o64 = torch.optim.AdamW(r64, lr=1e-3, weight_decay=1e-2)
    od = optim.FusedAdamW(dev, lr=1e-3, weight_decay=1e-2)
    for k, step in enumerate(gs):
        for p, p64, q, g in zip(r32, r64, dev, step):
            p.grad, p64.grad, q.grad = g.clone(), g.double().clone(), g.clone().to(DEV)
        n64 = float(torch.nn.utils.clip_grad_norm_(r64, max_norm))
        torch.nn.utils.clip_grad_norm_(r32, max_norm)
        n = optim.clip_grad_norm_(dev, max_norm)
        assert n.is_cuda and n.dim() == 0
        assert _within_ulps(n, n64), (k, float(n), n64)
        coef = max_norm / (n64 + 1e-6)
        assert (coef < 0.5) if k == 0 else True
        assert (coef > 1.0) if k == 2 else True
        if k == 2:  # not clipped: the gradients are untouched
            assert all(torch.equal(q.grad.cpu(), g) for q, g in zip(dev, step))
        o32.step()
        o64.step()
        od.step()
    for p, p64, q in zip(r32, r64, dev):
        d32, dours = _rel_l2(p, p64), _rel_l2(q, p64)
        print(f"{tuple(p.shape)}: |f32 ref - f64| {d32:.3e}  |ours - f64| {dours:.3e}")
        assert dours <= 2 * d32 + 1e-7, (tuple(p.shape), dours, d32)
    with pytest.raises(RuntimeError, match="non-finite"):
        dev[0].grad[3] = float("inf")
        optim.clip_grad_norm_(dev, max_norm, error_if_nonfinite=True)
    single = optim.clip_grad_norm_(dev[1], 1e9)  # a single tensor, as torch takes it
    assert _within_ulps(single, float(dev[1].grad.double().norm()))


# ------------------------------------------------------------------ 4. fused == unfused, bitwise
def _opt_state(n_sets, seed=2):
    """n_sets identical (params, FusedAdamW) sets: several chunks with a ragged end, tiny tensors, one
    parameter with a live bf16 shadow, one gradient slot that is a 4-byte-offset view."""
    import ops
    from optim import FusedAdamW
    g = torch.Generator().manual_seed(seed)
    shapes = [(2 * 4096 + 5,), (37, 5), (1,), (96, 64), (4097,)]
    init = [torch.randn(*s, generator=g) for s in shapes]
    sets = []
    for _ in range(n_sets):
        ps = [p.clone().to(DEV).requires_grad_(True) for p in init]
        sh = ops.cast_weight(ps[3], torch.bfloat16)
        slot = torch.zeros(4097 + 1, device=DEV)
        ps[4].grad = slot[1:]
        sets.append((ps, FusedAdamW(ps, lr=1e-2, weight_decay=1e-2), sh))
    return sets, shapes


def _set_grads(ps, grads):
    for p, g in zip(ps, grads):
        if p.grad is not None and p.grad.data_ptr() % 16 != 0:
            p.grad.copy_(g)  # keep the unaligned view
        else:
            p.grad = g.clone().to(DEV)


def _same_state(a, b):
    (pa, oa, sa), (pb, ob, sb) = a, b
    torch.cuda.synchronize()
    for p, q in zip(pa, pb):
        assert torch.equal(p.detach(), q.detach())
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(oa.state[p][k], ob.state[q][k]), k
        assert float(oa.state[p]["step"]) == float(ob.state[q]["step"])
    assert torch.equal(sa, sb)


def test_fused_scale_equals_unfused_bitwise():
    import ops
    import optim
    (A, B, C, D, E), shapes = _opt_state(5)
    one = torch.ones((), device=DEV)
    g = torch.Generator().manual_seed(9)
    for it, max_norm in enumerate((20.0, 1e6, 50.0)):  # clipped, not clipped, clipped
        grads = [torch.randn(*s, generator=g) for s in shapes]
        for S in (A, B, C, D, E):
            _set_grads(S[0], grads)
        gn = A[1].grad_norm(max_norm, finite=one)
        A[1].step(finite=gn.finite, grad_scale=gn.coef)
        for p, gr in zip(A[0], grads):  # the fused form leaves .grad alone
            assert torch.equal(p.grad.cpu(), gr)
        n = optim.clip_grad_norm_(B[0], max_norm)
        B[1].step(finite=one)
        assert torch.equal(n, gn.norm)
        assert (float(gn.coef) < 1.0) == (max_norm < 1e5)
        _same_state(A, B)
        assert torch.equal(A[2], A[0][3].detach().to(torch.bfloat16)) and ops.shadow_of(A[0][3]) is A[2]
        # a scale of exactly 1, and no scale at all, are today's step
        C[1].step(finite=one, grad_scale=one)
        D[1].step(finite=one)
        E[1].step(finite=one, grad_scale=None)
        _same_state(C, D)
        _same_state(E, D)
    assert not torch.equal(A[0][0].detach(), D[0][0].detach())  # clipping did change the update
    # the host-count path (finite=None) takes the scale too
    (F, G), _ = _opt_state(2)
    grads = [torch.randn(*s, generator=g) for s in shapes]
    _set_grads(F[0], grads)
    _set_grads(G[0], grads)
    gn = F[1].grad_norm(20.0)
    F[1].step(grad_scale=gn.coef)
    optim.clip_grad_norm_(G[0], 20.0)
    G[1].step()
    _same_state(F, G)


# ------------------------------------------------------------------ 5. non-finite gradient
def test_nonfinite_gradient_skips_the_update():
    from optim import STATS_FIELDS, FusedAdamW
    torch.manual_seed(1)
    ps = [torch.randn(1000), torch.randn(37, 5)]
    gs = [[torch.randn_like(p) for p in ps] for _ in range(5)]
    poison = {1: float("inf"), 2: float("nan")}
    max_norm = 30.0  # ||g|| ~ sqrt(1185) = 34.4: the clean steps clip
    ref = [p.clone().requires_grad_(True) for p in ps]
    dev = [p.clone().to(DEV).requires_grad_(True) for p in ps]
    o1 = torch.optim.AdamW(ref, lr=1e-3, weight_decay=1e-2)
    o2 = FusedAdamW(dev, lr=1e-3, weight_decay=1e-2)
    one = torch.ones((), device=DEV)  # the loss itself stayed finite
    stats = torch.zeros(len(STATS_FIELDS), dtype=torch.float64, device=DEV)
    norms, clipped = [], 0
    for k, step in enumerate(gs):
        for p, q, g in zip(ref, dev, step):
            p.grad = None if k in poison else g.clone()
            q.grad = g.clone().to(DEV)
        if k in poison:
            dev[1].grad[17, 3] = poison[k]
            before = [(q.detach().clone(), o2.state[q]["exp_avg"].clone(), o2.state[q]["exp_avg_sq"].clone(),
                       float(o2.state[q]["step"])) for q in dev]
            gn = o2.grad_norm(max_norm, finite=one, stats=stats)
            o2.step(finite=gn.finite, grad_scale=gn.coef)
            assert float(gn.finite) == 0.0 and float(gn.coef) == 1.0 and not np.isfinite(float(gn.norm))
            for q, (w, m, v, s) in zip(dev, before):
                assert torch.equal(q.detach(), w) and torch.equal(o2.state[q]["exp_avg"], m)
                assert torch.equal(o2.state[q]["exp_avg_sq"], v) and float(o2.state[q]["step"]) == s
        else:
            n = float(torch.nn.utils.clip_grad_norm_(ref, max_norm))
            norms.append(n)
            clipped += n > max_norm
            o1.step()
            gn = o2.grad_norm(max_norm, finite=one, stats=stats)
            o2.step(finite=gn.finite, grad_scale=gn.coef)
            assert float(gn.finite) == 1.0
    for p, q in zip(ref, dev):
        assert float(o2.state[q]["step"]) == 3.0 and float(o1.state[p]["step"]) == 3.0
        assert float((q.detach().cpu().double() - p.detach().double()).abs().max() / p.detach().abs().max()) < 1e-6
        e = (o2.state[q]["exp_avg_sq"].cpu().double() - o1.state[p]["exp_avg_sq"].double()).abs().max()
        assert float(e / o1.state[p]["exp_avg_sq"].abs().max()) < 1e-6
    st = dict(zip(STATS_FIELDS, stats.tolist()))
    assert st["steps"] == 5 and st["nonfinite"] == 2 and st["clipped"] == clipped == 3
    assert st["norm_sum"] == pytest.approx(sum(norms), rel=1e-6) and st["norm_max"] == pytest.approx(max(norms), rel=1e-6)


# ------------------------------------------------------------------ 6. Trainer
def _vit(sd):
    import model_vit
    m = model_vit.IntentNetViT(backbone_cfg={"img_size": (32, 48), "drop_path_rate_lidar": 0.0,
                                             "drop_path_rate_map": 0.0})
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).set_compute_dtype(torch.bfloat16).train()


def _weights(m):
    torch.cuda.synchronize()
    return torch.cat([p.detach().reshape(-1) for p in m.parameters()]).clone()


@pytest.fixture(scope="module")
def small():
    """The 32x48 bf16 IntentNetViT case, and the run without clipping on the device-count path: its
    weights after one and two steps, and the first step's gradients."""
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

    def trainer(**kw):
        m = _vit(sd)
        lf = L.DetectionIntentionLoss(apply_intention_downsampling=False)
        return m, Trainer(m, lf, FusedAdamW(m.parameters(), lr=1e-4, weight_decay=1e-4), anchors, **kw)

    m, tr = trainer(check_nan=False)
    d = tr.step(batch)
    assert "grad_norm" not in d  # today's dict
    g1 = [p.grad.detach().clone() for p in m.parameters()]
    w1 = _weights(m)
    tr.step(batch)
    return dict(sd=sd, batch=batch, anchors=anchors, trainer=trainer, g1=g1, w1=w1, w2=_weights(m))


@pytest.mark.parametrize("check_nan", [False, True])
def test_trainer_clipping(small, check_nan):
    import optim
    batch = small["batch"]
    # far above the norm: coef is exactly 1, the weights are those of the run without clipping
    m, tr = small["trainer"](check_nan=check_nan, max_grad_norm=1e30)
    d1 = tr.step(batch)
    n1 = d1["grad_norm"]
    tr.step(batch)
    assert torch.equal(_weights(m), small["w2"])
    assert n1.is_cuda and n1.dim() == 0 and tr.clipped == 0 and tr.nonfinite_grad == 0
    # the norm of the first step: clip_grad_norm_ on a copy of the (untouched) gradients; it stays
    # valid after the later step
    copies = [torch.nn.Parameter(g.clone()) for g in small["g1"]]
    for c, g in zip(copies, small["g1"]):
        c.grad = g.clone()
    ref = optim.clip_grad_norm_(copies, 1e30)
    assert torch.equal(n1, ref)
    assert _within_ulps(n1, _ref_norm(small["g1"]))
    norm = float(n1)
    assert np.isfinite(norm) and norm > 0
    # half the first step's norm: the step clips, and equals clip_grad_norm_ + step(finite=...)
    half = 0.5 * norm
    m, tr = small["trainer"](check_nan=check_nan, max_grad_norm=half)
    d = tr.step(batch)
    assert torch.equal(d["grad_norm"], ref)
    assert all(torch.equal(p.grad, g) for p, g in zip(m.parameters(), small["g1"]))  # .grad unscaled
    m2, tr2 = small["trainer"](check_nan=False)
    tr2.zero_grad()
    c, b, i = m2(batch["lidar_bev"], batch["map_bev"])
    from loss import device_guard
    with device_guard():
        d2 = tr2.loss_fn(c, b, i, small["anchors"], batch["gt_list"])
    d2["loss"].backward()
    optim.clip_grad_norm_(m2.parameters(), half)
    tr2.optimizer.step(finite=tr2.loss_fn.last_finite)
    w = _weights(m)
    assert torch.equal(w, _weights(m2))
    assert not torch.equal(w, small["w1"])  # and it is not the unclipped update
    assert tr.clipped == 1 and tr.nonfinite_grad == 0
    st = tr.grad_stats()
    assert st["steps"] == 1 and st["norm_max"] == norm and st["norm_sum"] == norm


def test_trainer_bucket_views_give_the_same_norm(small):
    m, tr = small["trainer"](check_nan=False, max_grad_norm=1e30)
    mb, trb = small["trainer"](check_nan=False, max_grad_norm=1e30, force_buckets=True, bucket_mb=8)
    assert trb.buckets is not None and len(trb.buckets.buckets) > 1
    for _ in range(2):
        d, db = tr.step(small["batch"]), trb.step(small["batch"])
        assert next(iter(mb.parameters())).grad.data_ptr() != next(iter(m.parameters())).grad.data_ptr()
        assert torch.equal(d["grad_norm"], db["grad_norm"])
    assert torch.equal(_weights(m), _weights(mb))


def test_cnn_step_with_clipping():
    import loss as L
    import model_cnn
    import utils
    from optim import FusedAdamW
    from oracle import ivit_oracle as O
    from oracle.weights import fill_state_dict
    from trainer import Trainer
    m = model_cnn.IntentNetCNN()
    m.load_state_dict(fill_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed=0), strict=True)
    m = m.to(DEV).set_compute_dtype(torch.bfloat16).train()
    lidar, mp_, gts = O.synthetic_batch(2, (32, 48), seed=1234)
    w0 = _weights(m)
    tr = Trainer(m, L.DetectionIntentionLoss(), FusedAdamW(m.parameters(), lr=1e-4, weight_decay=1e-4),
                 utils.generate_anchors(32, 48, 8, device=DEV), check_nan=True, max_grad_norm=1.0)
    d = tr.step({"lidar_bev": lidar.to(DEV), "map_bev": mp_.to(DEV), "gt_list": gts})
    assert d is not None and np.isfinite(float(d["grad_norm"])) and float(d["grad_norm"]) > 0
    assert tr.grad_stats()["steps"] == 1 and not torch.equal(_weights(m), w0)


def test_train_vit_clip_flag_reports_the_epoch(capsys):
    import re
    import train_vit
    rc = train_vit.main(["--synthetic", "--epochs", "2", "--batches-per-epoch", "2", "--batch", "2", "--grid", "32x48",
                         "--dtype", "bf16", "--no-save", "--clip-grad-norm", "1e-3"])
    assert rc == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "Grad norm (clip 0.001)" in ln]
    assert len(lines) == 2, lines
    for ln in lines:  # the accumulator is reset every epoch
        m = re.search(r"mean (\S+), max (\S+), clipped 2/2 steps, skipped 0 ", ln)
        assert m and 0 < float(m.group(1)) <= float(m.group(2)), ln


# ------------------------------------------------------------------ 7. two ranks
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    try:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK="0")
        for p in (os.path.join(HERE, ".."), os.path.join(HERE, "..", "visiontransformer-intention-prediction_amd")):
            sys.path.insert(0, p)
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        import loss as L
        import utils
        from optim import FusedAdamW
        from oracle import ivit_oracle as O
        from oracle.weights import make_state_dict, model_cfg
        from trainer import Trainer
        H, W = 32, 48
        m = _vit(make_state_dict(model_cfg(img_size=(H, W)), seed=0))
        lidar, mp_, gts = O.synthetic_batch(2, (H, W), seed=100 + rank, box_region=(54.0, 60.0, -72.0, -62.0))
        batch = {"lidar_bev": lidar.cuda(), "map_bev": mp_.cuda(), "gt_list": gts}
        anchors = utils.generate_anchors(H, W, 8, device="cuda")
        tr = Trainer(m, L.DetectionIntentionLoss(apply_intention_downsampling=False),
                     FusedAdamW(m.parameters(), lr=1e-4, weight_decay=1e-4), anchors, world=world, bucket_mb=1,
                     check_nan=False, max_grad_norm=1e-3)
        init = _weights(m)
        norms = torch.stack([tr.step(batch)["grad_norm"] for _ in range(2)])
        flat = _weights(m)
        others = [torch.empty_like(flat) for _ in range(world)]
        dist.all_gather(others, flat)
        allnorms = [torch.empty_like(norms) for _ in range(world)]
        dist.all_gather(allnorms, norms)
        q.put((rank, bool(all(torch.equal(o, flat) for o in others)),
               bool(all(torch.equal(a.view(torch.int32), norms.view(torch.int32)) for a in allnorms)),
               float((flat - init).abs().max()), norms.tolist(), tr.clipped, None))
        dist.destroy_process_group()
    except Exception:  # report to the parent instead of hanging the spawn
        import traceback
        q.put((rank, None, None, None, None, None, traceback.format_exc()))


def test_two_ranks_same_norm_identical_replicas():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for rank, same_w, same_n, moved, norms, clipped, exc in res:
        assert exc is None, (rank, exc)
        assert same_w and same_n, rank
        assert moved > 0.0 and all(np.isfinite(n) and n > 0 for n in norms), (rank, norms)
        assert clipped == 2, (rank, clipped, norms)
