"""Rotated-IoU box regression on the device: ops.rotated_iou_pairs and the iou_loss_weight term of
DetectionIntentionLoss against the torch f64 reference of tests/riou_cases.py (autograd through a
Sutherland-Hodgman clip), with positives and matches from oracle.ivit_oracle.assign_targets."""
import functools

import numpy as np
import pytest
import torch

import riou_cases as R
from oracle import ivit_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rel(a, b):
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


# ----------------------------------------------------------------------------- the element-wise op
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_pairs_forward_backward(n):
    import ops
    boxes, targets, iou, grad = R.pool()
    b = torch.tensor(boxes[:n], dtype=torch.float32, device=DEV).requires_grad_(True)
    t = torch.tensor(targets[:n], dtype=torch.float32, device=DEV)
    v = ops.rotated_iou_pairs(b, t)
    assert v.shape == (n,) and v.dtype == torch.float32
    w = torch.linspace(0.5, 1.5, n, device=DEV)  # a non-trivial upstream gradient
    (v * w).sum().backward()
    np.testing.assert_allclose(v.detach().cpu().numpy(), iou[:n], rtol=2e-6)
    g = (b.grad / w[:, None]).double().cpu().numpy()
    err = np.abs(g - grad[:n]).max(axis=1) / np.abs(grad[:n]).max(axis=1)
    print(f"n={n}: iou rel {np.abs(v.detach().cpu().numpy() / iou[:n] - 1).max():.3g}, gradient {err.max():.3g}")
    assert err.max() <= 1e-5


def test_pairs_edge_cases():
    import ops
    cases = R.edge_cases()
    names = list(cases)
    b = torch.tensor(np.array([cases[k][0] for k in names]), dtype=torch.float32, device=DEV).requires_grad_(True)
    t = torch.tensor(np.array([cases[k][1] for k in names]), dtype=torch.float32, device=DEV)
    v = ops.rotated_iou_pairs(b, t)
    (g,) = torch.autograd.grad(v, b, torch.ones_like(v))
    v, g = v.detach().cpu(), g.cpu()
    for i, k in enumerate(names):
        if k in R.ZERO_CASES:
            assert float(v[i]) == 0.0 and torch.count_nonzero(g[i]).item() == 0, k
        elif k in R.FINITE_CASES:
            assert bool(torch.isfinite(v[i])) and bool(torch.isfinite(g[i]).all()), k
        else:
            assert k in R.NAN_CASES and bool(torch.isnan(v[i])), k
    assert abs(float(v[names.index("identical")]) - 1.0) <= 2e-6


def test_pairs_empty():
    import ops
    b = torch.zeros((0, 5), device=DEV, requires_grad=True)
    v = ops.rotated_iou_pairs(b, torch.zeros((0, 5), device=DEV))
    assert v.shape == (0,)
    v.sum().backward()
    assert b.grad is not None and b.grad.shape == (0, 5)
    with pytest.raises(ValueError):
        ops.rotated_iou_pairs(torch.zeros((3, 4), device=DEV), torch.zeros((3, 5), device=DEV))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rotated_iou_pairs(torch.zeros((3, 5)), torch.zeros((3, 5)))


# ----------------------------------------------------------------------------- the loss term
B, K = 2, 8
BOX_W = 1.5  # box_weight: not 1, so its place in the chain shows
POS_THR, NEG_THR = 0.6, 0.45


def _rot_iou(a, b):
    return torch.from_numpy(O.rotated_iou_numpy(a.numpy(), b.numpy()))


@functools.lru_cache(maxsize=None)
def _scene(NA, variant, seed=0):
    """Hand-built anchors: jittered copies of the GT boxes (positives), two shifted copies of one
    yaw-0 GT at IoU ~0.52 / ~0.54 under both IoUs (its best anchor is force-matched), fillers far away.
    -> (anchors (NA, 5), gt_list, [cls (B, NA, 1), box (B, NA, 6), intent (B, NA, K)]) on the CPU."""
    g = torch.Generator().manual_seed(1000 + seed + NA)

    def u(lo, hi, *shape):
        return lo + (hi - lo) * torch.rand(shape, generator=g)
    counts = [3, 4] if NA == 300 else [2, 1]
    gts, k = [], 0
    for n in counts:
        ctr = torch.tensor([[-30.0 + 14.0 * (k + j), 10.0 * ((k + j) % 3) - 10.0] for j in range(n)])
        k += n
        boxes = torch.cat([ctr + u(-1, 1, n, 2), u(1.5, 2.5, n, 1), u(3.5, 6.0, n, 1), u(-3.1, 3.1, n, 1)], dim=1)
        gts.append({"boxes_xywha": boxes.float(), "intentions": torch.randint(0, 8, (n,), generator=g)})
    gts[0]["boxes_xywha"][0, 4] = 0.0  # the force-matched GT: axis-aligned, so both IoUs agree on it
    rows = []
    if variant != "no_pos":
        for b in range(B):
            for j, gb in enumerate(gts[b]["boxes_xywha"]):
                if b == 0 and j == 0:
                    for f in (0.316, 0.30):  # IoU (1 - f) / (1 + f) = 0.520, 0.538: in [neg_thr, pos_thr)
                        rows.append(gb + torch.tensor([f * float(gb[2]), 0.0, 0.0, 0.0, 0.0]))
                    continue
                for _ in range(5):
                    jit = torch.randn(5, generator=g) * torch.tensor([0.08, 0.08, 0.05, 0.08, 0.03])
                    rows.append(gb + jit)
    nfill = NA - len(rows)
    fill = torch.cat([200.0 + 9.0 * torch.arange(nfill).float()[:, None], u(-50, 50, nfill, 1), u(1.5, 2.5, nfill, 1),
                      u(3.5, 6.0, nfill, 1), u(-3.1, 3.1, nfill, 1)], dim=1)
    anchors = torch.cat([torch.stack(rows), fill]) if rows else fill
    anchors = anchors[torch.randperm(NA, generator=g)].float().contiguous()
    if variant == "no_gt1":
        gts[1] = {"boxes_xywha": torch.zeros((0, 5)), "intentions": torch.zeros((0,), dtype=torch.long)}
    cls = torch.randn((B, NA, 1), generator=g)
    box = torch.randn((B, NA, 6), generator=g) * torch.tensor([0.08, 0.04, 0.06, 0.06, 0.0, 0.0])
    dyaw = 0.08 * torch.randn((B, NA), generator=g)
    r = u(0.7, 1.3, B, NA)
    box[..., 4], box[..., 5] = r * torch.sin(dyaw), r * torch.cos(dyaw)
    intent = torch.randn((B, NA, K), generator=g)
    return anchors, gts, [cls, box.float().contiguous(), intent]


@functools.lru_cache(maxsize=None)
def _reference(NA, variant, rot):
    """Positives and matches from the oracle's assignment; per positive the reference IoU and its
    gradient w.r.t. the six raw outputs. -> (pos (B, NA) bool, forced count, sum(1 - IoU), sum IoU,
    dIoU/draw (B, NA, 6) f64)."""
    anchors, gts, (_, box, _) = _scene(NA, variant)
    iou_fn = _rot_iou if rot else O.axis_aligned_iou
    cls_t, _, _ = O.assign_targets(anchors, gts, pos_thr=POS_THR, neg_thr=NEG_THR, iou_fn=iou_fn)
    pos = cls_t == 1
    forced, s1, s2 = 0, 0.0, 0.0
    graw = np.zeros((B, NA, 6))
    for b in range(B):
        if gts[b]["boxes_xywha"].shape[0] == 0:
            continue
        iou = iou_fn(anchors, gts[b]["boxes_xywha"].float())
        mx, arg = iou.max(dim=1)
        for a in torch.where(pos[b])[0].tolist():
            forced += float(mx[a]) < POS_THR
            v, gr = R.riou_ref_decoded(box[b, a].numpy(), anchors[a].numpy(), gts[b]["boxes_xywha"][arg[a]].numpy())
            s1 += 1.0 - v
            s2 += v
            graw[b, a] = gr
    return pos, forced, s1, s2, graw


def _run(NA, variant, rot, lam, sync_guard=False, box=None, **kw):
    import loss as L
    anchors, gts, ts = _scene(NA, variant)
    ts = [t.clone() for t in ts]
    if box is not None:
        ts[1] = box
    ts = [t.to(DEV).requires_grad_(True) for t in ts]
    args = dict(apply_intention_downsampling=False, use_rotated_iou=rot, box_weight=BOX_W, sync_guard=sync_guard)
    if lam is not None:
        args["iou_loss_weight"] = lam
    args.update(kw)
    lf = L.DetectionIntentionLoss(**args)
    d = lf(*ts, anchors.to(DEV), gts)
    d["loss"].backward()
    torch.cuda.synchronize()
    return lf, d, ts


@pytest.mark.parametrize("rot", [False, True])
@pytest.mark.parametrize("variant", ["base", "no_gt1", "no_pos"])
@pytest.mark.parametrize("NA", [70, 300])
def test_loss_term_vs_reference(NA, variant, rot):
    pos, forced, s1, s2, graw = _reference(NA, variant, rot)
    npos = int(pos.sum())
    if variant == "no_pos":
        assert npos == 0
    else:
        assert npos >= 5 and forced >= 1, (npos, forced)
        assert int(pos[1].sum()) == 0 if variant == "no_gt1" else int(pos[1].sum()) > 0
    _, d0, t0 = _run(NA, variant, rot, 0.0)
    assert int(d0["num_pos_anchors"]) == npos
    assert "iou_loss" not in d0 and "pos_iou" not in d0
    for lam in (0.5, 2.0):
        _, d, t = _run(NA, variant, rot, lam)
        assert int(d["num_pos_anchors"]) == npos
        assert torch.equal(t[0].grad, t0[0].grad) and torch.equal(t[2].grad, t0[2].grad)
        assert torch.equal(d["cls_loss"], d0["cls_loss"]) and torch.equal(d["intent_loss"], d0["intent_loss"])
        term = lam * s1 / max(1, npos)
        got = (float(d["loss"].detach()) - float(d0["loss"].detach()), float(d["box_loss"]) - float(d0["box_loss"]),
               float(d["iou_loss"]), float(d["pos_iou"]))
        want = (BOX_W * term, term, term, s2 / max(1, npos))
        print(f"NA={NA} {variant} rot={rot} lam={lam}: npos {npos} forced {forced} got {got} want {want}")
        if npos == 0:
            assert got == (0.0, 0.0, 0.0, 0.0)
            assert torch.equal(t[1].grad, t0[1].grad)
            continue
        np.testing.assert_allclose(got, want, rtol=2e-5)
        ref = torch.from_numpy(-BOX_W * lam * graw / npos)
        assert float(ref.abs().max()) > 0
        assert _rel(t[1].grad.double().cpu() - t0[1].grad.double().cpu(), ref) < 1e-4
        assert torch.count_nonzero((t[1].grad - t0[1].grad).cpu()[~pos]).item() == 0


def test_weight_zero_is_todays_loss():
    _, d0, t0 = _run(300, "base", True, None)
    _, d1, t1 = _run(300, "base", True, 0.0)
    assert sorted(d0) == sorted(d1) == ["box_loss", "cls_loss", "intent_loss", "loss", "num_pos_anchors"]
    for k in d0:
        assert torch.equal(d0[k], d1[k]), k
    for a, b in zip(t0, t1):
        assert torch.equal(a.grad, b.grad)


def _poisoned_box(NA, variant, rot, what, on_positive):
    pos = _reference(NA, variant, rot)[0]
    box = _scene(NA, variant)[2][1].clone()
    b, a = [int(v) for v in torch.nonzero(pos if on_positive else ~pos)[0]]
    if what == "inf_d2":
        box[b, a, 2] = float("inf")
    else:
        box[b, a, 0] = float("nan")
    return box


@pytest.mark.parametrize("what", ["inf_d2", "nan_d0"])
def test_guard_device_form(what):
    NA, variant, rot = 300, "base", True
    npos = int(_reference(NA, variant, rot)[0].sum())
    lf, d, t = _run(NA, variant, rot, 1.0, box=_poisoned_box(NA, variant, rot, what, True))
    assert float(lf.last_finite) == 0.0
    for k in ("loss", "cls_loss", "box_loss", "intent_loss", "iou_loss", "pos_iou"):
        assert float(d[k]) == 0.0, k
    assert int(d["num_pos_anchors"]) == npos
    for x in t:
        assert x.grad is not None and torch.count_nonzero(x.grad).item() == 0  # exact zeros, no NaN
    # the same poison on a non-positive anchor: nothing reads it, the term stays finite
    lf, d, t = _run(NA, variant, rot, 1.0, box=_poisoned_box(NA, variant, rot, what, False))
    _, dref, _ = _run(NA, variant, rot, 1.0)
    assert float(lf.last_finite) == 1.0
    for k in ("loss", "box_loss", "iou_loss", "pos_iou"):
        assert torch.equal(d[k], dref[k]) and bool(torch.isfinite(d[k])), k
    assert bool(torch.isfinite(t[1].grad).all())


@pytest.mark.parametrize("what", ["inf_d2", "nan_d0"])
def test_guard_reference_form(what, capsys):
    NA, variant, rot = 300, "base", True
    npos = int(_reference(NA, variant, rot)[0].sum())
    lf, d, t = _run(NA, variant, rot, 1.0, sync_guard=True, box=_poisoned_box(NA, variant, rot, what, True))
    out = capsys.readouterr().out
    assert "NaN or Inf DETECTED IN LOSS!" in out and "IoU:" in out
    assert d["loss"].is_leaf and d["loss"].requires_grad and d["loss"].grad_fn is None
    for k in ("loss", "cls_loss", "box_loss", "intent_loss", "iou_loss", "pos_iou"):
        assert float(d[k]) == 0.0, k
    assert type(d["num_pos_anchors"]) is int and d["num_pos_anchors"] == npos
    for x in t:
        assert x.grad is None
    _, d, _ = _run(NA, variant, rot, 1.0, sync_guard=True)
    _, dref, _ = _run(NA, variant, rot, 1.0)
    assert type(d["num_pos_anchors"]) is int and "IoU:" not in capsys.readouterr().out
    for k in ("loss", "box_loss", "iou_loss", "pos_iou"):
        assert torch.equal(d[k], dref[k]), k


def test_repeatable_bits():
    runs = [_run(300, "base", True, 2.0) for _ in range(2)]
    (_, da, ta), (_, db, tb) = runs
    for k in da:
        assert torch.equal(da[k], db[k]), k
    for a, b in zip(ta, tb):
        assert torch.equal(a.grad, b.grad)


# ----------------------------------------------------------------------------- the train step
class _PoisonBox:
    """A loss whose box prediction d2 is forced to +Inf on one (positive) anchor."""

    def __init__(self, inner, b, a):
        self.inner, self.b, self.a = inner, b, a

    @property
    def last_finite(self):
        return self.inner.last_finite

    def __call__(self, c, bx, i, anchors, gts):
        mask = torch.zeros(bx.shape, dtype=bx.dtype, device=bx.device)
        mask.view(bx.shape[0], -1, 6)[self.b, self.a, 2] = float("inf")
        return self.inner(c, bx + mask, i, anchors, gts)


def test_train_step_with_iou_term():
    """Trainer + FusedAdamW at the 64 x 96 grid with iou_loss_weight = 1: a step changes the weights;
    the same step with a poisoned positive leaves weights and optimiser state bit-identical."""
    import loss as L
    import model_vit
    import utils
    from optim import FusedAdamW
    from oracle.weights import make_state_dict, model_cfg
    from trainer import Trainer
    H, W = 64, 96
    cfg = model_cfg(img_size=(H, W))
    m = model_vit.IntentNetViT(backbone_cfg={"img_size": (H, W)})
    m.load_state_dict(make_state_dict(cfg, seed=0), strict=True)
    m = m.to(DEV).set_compute_dtype(torch.bfloat16).train()
    lidar, mp, _ = O.synthetic_batch(2, (H, W), seed=3, grid_scale=H / 400.0)
    anchors = utils.generate_anchors(H, W, 8, device=DEV)
    # GT boxes next to chosen anchors, so the small grid has positives
    g = torch.Generator().manual_seed(5)
    gts = []
    for idx in ([17, 203, 388], [64, 131, 290, 455]):
        jit = torch.randn((len(idx), 5), generator=g) * torch.tensor([0.15, 0.15, 0.1, 0.15, 0.05])
        gts.append({"boxes_xywha": (anchors.cpu()[idx] + jit).float(),
                    "intentions": torch.randint(0, 8, (len(idx),), generator=g)})
    batch = {"lidar_bev": lidar.to(DEV), "map_bev": mp.to(DEV), "gt_list": gts}
    pos = O.assign_targets(anchors.cpu(), gts)[0] == 1
    assert int(pos.sum()) >= 7
    pb, pa = [int(v) for v in torch.nonzero(pos)[0]]
    opt = FusedAdamW(m.parameters(), lr=1e-4, weight_decay=1e-4)
    lf = L.DetectionIntentionLoss(iou_loss_weight=1.0)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    good = Trainer(m, lf, opt, anchors, check_nan=True)
    d = good.step(batch)
    torch.cuda.synchronize()
    assert d is not None and float(d["loss"]) > 0 and float(d["iou_loss"]) > 0 and 0.0 <= float(d["pos_iou"]) <= 1.0
    assert int(d["num_pos_anchors"]) == int(pos.sum())
    w0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    assert any(not torch.equal(w0[k], before[k]) for k in w0 if k.endswith("weight"))
    s0 = {id(p): {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state[p].items()}
          for p in m.parameters()}
    bad = Trainer(m, _PoisonBox(lf, pb, pa), opt, anchors, check_nan=True)
    d = bad.step(batch)
    torch.cuda.synchronize()
    assert d is not None and float(d["loss"]) == 0.0 and bad.nonfinite == 1
    for k, v in m.state_dict().items():
        if "num_batches_tracked" in k or "running_" in k:
            continue  # BN statistics move in the forward, as in the reference
        assert torch.equal(v, w0[k]), k
    for p in m.parameters():
        for k, v in opt.state[p].items():
            ref = s0[id(p)][k]
            assert (torch.equal(v, ref) if torch.is_tensor(v) else v == ref), k
