"""Attention maps for chosen BEV cells on the GPU: the ivit_attn_rows kernel through ops.attn_rows
against an f64 softmax of the same inputs, VisionTransformer.attention_rows / IntentNetViT.
attention_maps against an f64 restatement of the timm blocks, and eval_vit's --attn-maps dump."""
import functools
import glob
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden
from oracle import ivit_oracle as O
from oracle.weights import VIT_ARCH, make_state_dict, model_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"
Q2 = math.log2(math.e) / 8.0  # log2(e) / sqrt(64): ops.Q2_SCALE

SHAPES = [(1, 1, 1), (1, 33, 1), (2, 257, 3), (1, 4501, 2)]
FORMS = ["f32", "bf16", "bf16q"]


def _rel(a, b):
    """tests/test_gpu_model.py's norm: max |a - b| / max |b|."""
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _requests(B, N, kind):
    """"one": R = 1, token 0. "many": R = 19 over all samples, token 0, token N - 1, other tokens and
    a duplicated request."""
    if kind == "one":
        return [0], [0]
    sample = [i % B for i in range(19)]
    token = [(5 + 7 * i) % N for i in range(19)]
    token[0], token[1] = 0, N - 1
    sample[18], token[18] = sample[2], token[2]
    return sample, token


def _softmax_rows(qkv64, B, N, H, sample, token, exp2):
    """f64 [R, H, N]: softmax over the keys of q . k / 8 (exp2 = False), or 2^(q . k) normalised
    when q already carries log2(e) / 8 (exp2 = True)."""
    v = qkv64.reshape(B, N, 3, H, 64)
    rows = []
    for s, t in zip(sample, token):
        u = torch.einsum("hd,nhd->hn", v[s, t, 0], v[s, :, 1])
        u = u if exp2 else u / 8.0
        u = u - u.max(dim=1, keepdim=True).values
        p = torch.exp2(u) if exp2 else torch.exp(u)
        rows.append(p / p.sum(dim=1, keepdim=True))
    return torch.stack(rows)


@functools.lru_cache(maxsize=None)
def _case(B, N, H, form, kind, qmul=1.0):
    """(device qkv, compute dtype code, prescaled, sample, token, f64 reference [R, H, N]) — built
    once per case and shared; the reference sees exactly the values the kernel reads."""
    import _lib
    g = torch.Generator().manual_seed(1000 * N + 10 * H + B)
    x = torch.randn((B * N, 3, H, 64), generator=g)
    x[:, 0] *= qmul
    if form == "bf16q":
        x[:, 0] *= Q2  # in f32, then rounded to bf16 with the rest: what ivit_linear_fwd_qs stores
    x = x.reshape(B * N, 3 * H * 64)
    dev = x.to(DEV) if form == "f32" else x.bfloat16().to(DEV)
    sample, token = _requests(B, N, kind)
    ref = _softmax_rows(dev.cpu().double(), B, N, H, sample, token, exp2=form == "bf16q")
    return dev, (_lib.F32 if form == "f32" else _lib.BF16), form == "bf16q", sample, token, ref


@pytest.mark.parametrize("head_mean", [False, True])
@pytest.mark.parametrize("kind", ["one", "many"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_attn_rows_vs_f64_softmax(shape, form, kind, head_mean):
    import ops
    B, N, H = shape
    qkv, cdt, pre, sample, token, ref = _case(B, N, H, form, kind)
    out = ops.attn_rows(qkv, B, N, H, cdt, sample, token, head_mean=head_mean, prescaled=pre)
    want = ref.mean(dim=1) if head_mean else ref
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(want.shape)
    got = out.double().cpu()
    err = float(((got - want).abs() / want.abs().clamp_min(1e-300)).max())
    print(f"attn_rows {shape} {form} {kind} mean={head_mean}: max rel err {err:.3e}")
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-12)
    assert float((got.sum(dim=-1) - 1.0).abs().max()) < 1e-5


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", [(2, 257, 3), (1, 4501, 2)])
def test_attn_rows_large_logits(shape, form):
    """Q times 30: scores of about +-127, so exp without the max subtraction overflows f32."""
    import ops
    B, N, H = shape
    qkv, cdt, pre, sample, token, ref = _case(B, N, H, form, "many", 30.0)
    v = qkv.cpu().double().reshape(B, N, 3, H, 64)
    dots = max(float(torch.einsum("hd,nhd->hn", v[s, t, 0], v[s, :, 1]).abs().max()) for s, t in zip(sample, token))
    smax = dots / (Q2 * 8.0) if pre else dots / 8.0  # |q . k| / sqrt(64) of the requested rows
    assert smax > 89.0, smax  # exp(89) > f32 max
    out = ops.attn_rows(qkv, B, N, H, cdt, sample, token, prescaled=pre)
    assert bool(torch.isfinite(out).all())
    got = out.double().cpu()
    big = ref >= 1e-6
    rel = float(((got - ref).abs() / ref.clamp_min(1e-300))[big].max())
    small = float((got - ref).abs()[~big].max()) if bool((~big).any()) else 0.0
    print(f"attn_rows large logits {shape} {form}: |score| max {smax:.1f}, rel {rel:.3e}, abs (small) {small:.3e}")
    assert rel < 1e-3 and small < 1e-9


@pytest.mark.parametrize("head_mean", [False, True])
def test_attn_rows_bitwise_repeatable(head_mean):
    import ops
    qkv, cdt, pre, sample, token, _ = _case(2, 257, 3, "bf16", "many")
    a = ops.attn_rows(qkv, 2, 257, 3, cdt, sample, token, head_mean=head_mean)
    b = ops.attn_rows(qkv, 2, 257, 3, cdt, sample, token, head_mean=head_mean)
    assert torch.equal(a, b)


@pytest.mark.parametrize("head_mean", [0, 1])
def test_attn_rows_out_of_range_request_gives_zero_row(head_mean):
    """The C entry point itself (ops.attn_rows refuses such indices): bad requests among good ones
    get zero rows, the good rows are what they are without them, and the device is fine afterwards."""
    import ops
    from _lib import lib, ptr, stream
    B, N, H = 2, 257, 3
    qkv, cdt, _, sample, token, _ = _case(B, N, H, "f32", "many")
    good = ops.attn_rows(qkv, B, N, H, cdt, sample, token, head_mean=bool(head_mean))
    bad = {3: (B, 5), 7: (0, N), 11: (-1, 0), 15: (1, -1)}  # request -> (sample, token)
    s2, t2 = list(sample), list(token)
    for r, (s, t) in bad.items():
        s2[r], t2[r] = s, t
    idx = torch.tensor([s2, t2], dtype=torch.int32, device=DEV)
    out = torch.full_like(good, float("nan"))
    lib.ivit_attn_rows(cdt, ptr(qkv), B, N, H, 64, 0, ptr(idx[0]), ptr(idx[1]), len(s2), head_mean, ptr(out), stream())
    torch.cuda.synchronize()
    keep = torch.tensor([r not in bad for r in range(len(s2))], device=DEV)
    assert torch.equal(out[keep], good[keep])
    assert bool((out[~keep] == 0).all())
    again = ops.attn_rows(qkv, B, N, H, cdt, sample, token, head_mean=bool(head_mean))  # the next HIP call
    torch.cuda.synchronize()
    assert torch.equal(again, good)


def test_attn_rows_op_refuses_bad_indices_without_a_launch():
    import ops
    B, N, H = 2, 257, 3
    qkv, cdt, _, _, _, _ = _case(B, N, H, "f32", "many")
    for sample, token in (([0, B], [0, 0]), ([0, 0], [0, N]), ([-1], [0]), ([0], [-1]), ([0, 1], [0])):
        with pytest.raises(ValueError):
            ops.attn_rows(qkv, B, N, H, cdt, sample, token)
    with pytest.raises(ValueError):
        ops.attn_rows(qkv, B, N, H, cdt, [0], [0], prescaled=True)  # f32 has no prescaled form
    assert ops.attn_rows(qkv, B, N, H, cdt, [], []).shape == (0, H, N)
    assert ops.attn_rows(qkv, B, N, H, cdt, torch.tensor([1]), torch.tensor([N - 1], device=DEV)).shape == (1, H, N)


def test_attn_rows_800x1440_grid():
    """N = 18001 (the 800 x 1440 grid), bf16: against torch's f32 softmax on the device."""
    import _lib
    import ops
    N = 18001
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn((N, 192), generator=g).bfloat16().to(DEV)
    token = [0, 9000, N - 1]
    out = ops.attn_rows(qkv, 1, N, 1, _lib.BF16, [0, 0, 0], token)[:, 0]
    x = qkv.float()
    ref = torch.softmax(x[token, :64] @ x[:, 64:128].T / 8.0, dim=-1)
    assert float((out.double().sum(dim=-1) - 1.0).abs().max()) < 1e-5
    big = ref >= 1e-6
    assert bool(big.any())
    rel = float(((out - ref).abs() / ref.clamp_min(1e-30))[big].max())
    print(f"attn_rows N=18001 bf16: rel {rel:.3e} on {int(big.sum())} entries >= 1e-6")
    assert rel < 1e-3


# ------------------------------------------------------------------------------------- model
def _model(cfg, cd=torch.float32, dp=0.0, **kw):
    import model_vit
    m = model_vit.IntentNetViT(backbone_cfg={"img_size": tuple(cfg["img_size"]), "drop_path_rate_lidar": dp,
                                             "drop_path_rate_map": dp, **kw})
    m.load_state_dict(make_state_dict(cfg, seed=0), strict=True)
    return m.to(DEV).set_compute_dtype(cd)


def _model_requests(N):
    """token 0 (CLS), one interior token per sample, the last token."""
    return [0, 0, 1, 1], [0, N // 2, N // 3 + 1, N - 1]


def _stream_maps(sd, prefix, x, heads, depth, sample, token):
    """[depth, R, heads, N] attention rows of a timm stream, in the dtype of ``sd`` / ``x`` (under
    torch.autocast: in its dtypes): block input -> layer_norm (eps 1e-6) -> qkv linear -> explicit
    softmax; the residual stream advanced by the oracle's block."""
    w = sd[prefix + "patch_embed.proj.weight"]
    t = F.conv2d(x, w, sd[prefix + "patch_embed.proj.bias"], stride=w.shape[-1]).flatten(2).transpose(1, 2)
    B, _, D = t.shape
    t = torch.cat([sd[prefix + "cls_token"].expand(B, -1, -1).to(t.dtype), t], dim=1) + sd[prefix + "pos_embed"]
    N = t.shape[1]
    maps = []
    for i in range(depth):
        b = f"{prefix}blocks.{i}."
        h = F.layer_norm(t, (D,), sd[b + "norm1.weight"], sd[b + "norm1.bias"], 1e-6)
        qkv = F.linear(h, sd[b + "attn.qkv.weight"], sd[b + "attn.qkv.bias"]).reshape(B, N, 3, heads, D // heads)
        rows = []
        for s, tk in zip(sample, token):
            u = torch.einsum("hd,nhd->hn", qkv[s, tk, 0], qkv[s, :, 1]) * ((D // heads) ** -0.5)
            rows.append(torch.softmax(u, dim=-1))
        maps.append(torch.stack(rows))
        t = O._vit_block(sd, b, t, heads, None, 1e-6, "explicit")
    return torch.stack(maps)


@functools.lru_cache(maxsize=None)
def _model_ref(img_size):
    """cfg, inputs, requests and the f64 reference maps {stream: [12, R, H, N]} of the seeded model."""
    cfg = model_cfg(img_size=img_size)
    lidar, mp, _ = O.synthetic_batch(2, img_size, seed=1234)
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in make_state_dict(cfg, seed=0).items()}
    N = (img_size[0] // 8) * (img_size[1] // 8) + 1
    sample, token = _model_requests(N)
    ref = {}
    for name, x in (("lidar", lidar), ("map", mp)):
        a = VIT_ARCH[cfg["vit_" + name]]
        ref[name] = _stream_maps(sd, f"backbone.vit_{name}.", x.double(), a["num_heads"], a["depth"], sample, token)
    return cfg, lidar, mp, sample, token, ref


@pytest.mark.parametrize("img_size", [(32, 48), (64, 96)])
def test_attention_rows_fp32_vs_f64_blocks(img_size):
    cfg, lidar, mp, sample, token, ref = _model_ref(img_size)
    m = _model(cfg).eval()
    for name, vit, x in (("lidar", m.backbone.vit_lidar, lidar), ("map", m.backbone.vit_map, mp)):
        got = vit.attention_rows(x.to(DEV), sample, token, head_mean=False)
        want = ref[name]
        assert tuple(got.shape) == tuple(want.shape) and got.shape[0] == 12
        N = want.shape[-1]
        # not flat: a kernel that returned uniform rows (1 / N everywhere) cannot pass
        assert float(want.max()) > 2.0 / N
        errs = [_rel(got[i], want[i]) for i in range(12)]
        print(f"attention_rows fp32 {img_size} {name}: rel per block max {max(errs):.3e}; "
              f"row maxima {float(want.amax(dim=-1).min()):.3f}..{float(want.amax(dim=-1).max()):.3f}")
        assert max(errs) < 1e-3, errs
        # the head mean and a block subset (negative indices) are the same rows
        sub = vit.attention_rows(x.to(DEV), sample, token, blocks=[-1, 0, 5], head_mean=True)
        assert tuple(sub.shape) == (3, len(sample), N)
        for k, b in enumerate((11, 0, 5)):
            assert _rel(sub[k], want[b].mean(dim=1)) < 1e-3


def test_attention_rows_bf16_vs_autocast():
    """bf16 streams: per block, the distance to the f64 maps is at most 1.5x (the margin
    tests/test_gpu_model.py grants the bf16 step) the distance of a torch CPU bf16-autocast
    computation of the same maps to the same f64 maps."""
    cfg, lidar, mp, sample, token, ref = _model_ref((32, 48))
    m = _model(cfg, torch.bfloat16).eval()
    sd = make_state_dict(cfg, seed=0)
    for name, vit, x in (("lidar", m.backbone.vit_lidar, lidar), ("map", m.backbone.vit_map, mp)):
        a = VIT_ARCH[cfg["vit_" + name]]
        with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
            amp = _stream_maps(sd, f"backbone.vit_{name}.", x, a["num_heads"], a["depth"], sample, token)
        got = vit.attention_rows(x.to(DEV), sample, token, head_mean=False)
        ours = [_rel(got[i], ref[name][i]) for i in range(12)]
        base = [_rel(amp[i].float(), ref[name][i]) for i in range(12)]
        print(f"attention_rows bf16 {name}: ours    " + " ".join(f"{e:.2e}" for e in ours))
        print(f"attention_rows bf16 {name}: autocast " + " ".join(f"{e:.2e}" for e in base))
        for i in range(12):
            assert ours[i] <= 1.5 * base[i], (name, i, ours[i], base[i])


def _cell_centres(cells, stride=8):
    """Metric centres of (gy, gx) cells of a stride-8 grid (the oracle's anchor-centre formula)."""
    gy, gx = torch.tensor(cells, dtype=torch.float64).unbind(1)
    px, py = gx * stride + stride / 2.0, gy * stride + stride / 2.0
    return torch.stack([(300.0 - py) * 0.2, (px - 360.0) * 0.2], dim=1).float()


@pytest.mark.parametrize("cd", [torch.float32, torch.bfloat16])
def test_attention_maps_on_a_training_model(cd):
    cfg, lidar, mp, _, _, _ = _model_ref((32, 48))
    m = _model(cfg, cd, dp=0.1)
    lidar, mp = lidar.to(DEV), mp.to(DEV)
    m.train()
    m(lidar, mp)  # a training forward: the blocks now hold drawn DropPath factors (and BatchNorm has moved)
    m.eval()
    with torch.no_grad():
        before = [t.clone() for t in m(lidar, mp)]
    m.train()
    vl = m.backbone.vit_lidar
    vl.blocks[3].drop_path_scales = (torch.ones(2), torch.zeros(2))
    scales = [blk.last_scales for blk in vl.blocks]
    cells = [(0, 0), (2, 3), (3, 5), (1, 4)]
    sample = [0, 1, 1, 0]
    for head_mean in (True, False):
        out = m.attention_maps(lidar, mp, sample, _cell_centres(cells), blocks=(-1, 4), head_mean=head_mean)
        hs = () if head_mean else (6,)
        for s in ("lidar", "map"):
            assert tuple(out[s].shape) == (2, 4) + hs + (4, 6) and out[s].dtype == torch.float32
            assert tuple(out[s + "_cls"].shape) == (2, 4) + hs
            assert out[s + "_cells"].tolist() == [list(c) for c in cells]
            total = out[s].double().sum(dim=(-2, -1)) + out[s + "_cls"].double()
            assert float((total - 1.0).abs().max()) < 1e-5
    assert m.training and all(mod.training for mod in m.modules())
    assert vl.blocks[3].drop_path_scales[1].tolist() == [0.0, 0.0]
    assert all(a[0] is b[0] and a[1] is b[1] for a, b in zip(scales, (blk.last_scales for blk in vl.blocks)))
    vl.blocks[3].drop_path_scales = None
    m.eval()
    with torch.no_grad():
        after = m(lidar, mp)
    for a, b in zip(before, after):
        assert torch.equal(a, b)


def test_attention_maps_patch16_map_stream():
    """A patch-16 map stream (as in test_regrid_patch16_map_vs_golden): its own, coarser grid and cells."""
    import model_vit
    z = golden("model_regrid.npz")
    cfg = json.loads(str(z["cfg"]))
    cfg["img_size"] = tuple(cfg["img_size"])
    with pytest.warns(UserWarning, match="differ"):
        m = model_vit.IntentNetViT(backbone_cfg={"img_size": cfg["img_size"], "drop_path_rate_lidar": 0.0,
                                                 "drop_path_rate_map": 0.0,
                                                 "vit_model_name_map": "vit_small_patch16_224"})
    m.load_state_dict(make_state_dict(cfg, seed=0), strict=True)
    m = m.to(DEV).train()
    lidar, mp, _ = O.synthetic_batch(2, cfg["img_size"], seed=1234)
    cells = [(0, 0), (2, 3), (3, 5)]
    out = m.attention_maps(lidar.to(DEV), mp.to(DEV), [0, 1, 1], _cell_centres(cells), blocks=(0, -1))
    assert tuple(out["lidar"].shape) == (2, 3, 4, 6) and tuple(out["map"].shape) == (2, 3, 2, 3)
    assert out["lidar_cells"].tolist() == [[0, 0], [2, 3], [3, 5]]
    assert out["map_cells"].tolist() == [[0, 0], [1, 1], [1, 2]]
    for s in ("lidar", "map"):
        total = out[s].double().sum(dim=(-2, -1)) + out[s + "_cls"].double()
        assert float((total - 1.0).abs().max()) < 1e-5
    assert m.training


def test_attention_maps_bf16_tiny_map_stream():
    """The bf16 widths off the row-panel path (vit_tiny, D = 192: qkv_fwd_q2) give normalised maps too."""
    import model_vit
    torch.manual_seed(0)
    m = model_vit.IntentNetViT(backbone_cfg={"img_size": (32, 48), "vit_model_name_map": "vit_tiny_patch8_224"})
    m = m.to(DEV).set_compute_dtype(torch.bfloat16).eval()
    lidar, mp, _ = O.synthetic_batch(2, (32, 48), seed=1234)
    out = m.attention_maps(lidar.to(DEV), mp.to(DEV), [0, 1], _cell_centres([(1, 1), (3, 0)]), head_mean=False)
    assert tuple(out["lidar"].shape) == (1, 2, 6, 4, 6) and tuple(out["map"].shape) == (1, 2, 3, 4, 6)
    for s in ("lidar", "map"):
        total = out[s].double().sum(dim=(-2, -1)) + out[s + "_cls"].double()
        assert float((total - 1.0).abs().max()) < 1e-5


# ------------------------------------------------------------------------------------- eval dump
def test_eval_vit_attn_maps_dump(tmp_path, monkeypatch):
    import eval_vit
    recorded = []
    real = eval_vit.run_inference

    def recording(*a, **kw):
        recorded.append(real(*a, **kw))
        return recorded[-1]

    monkeypatch.setattr(eval_vit, "run_inference", recording)
    monkeypatch.chdir(tmp_path)
    out_dir = tmp_path / "maps"
    base = ["--synthetic", "--checkpoint", "/nonexistent.pth", "--batch", "2", "--batches", "2", "--grid", "32x48"]
    torch.manual_seed(0)  # the random-init weights of the run
    assert eval_vit.main_eval_vit(base) == 0
    assert not out_dir.exists() and not glob.glob(str(tmp_path / "**" / "*.npz"), recursive=True)
    torch.manual_seed(0)
    assert eval_vit.main_eval_vit(base + ["--attn-maps", str(out_dir), "--attn-top", "3"]) == 0
    files = sorted(os.listdir(out_dir))
    assert files == ["attn_batch_00000.npz", "attn_batch_00001.npz"]
    for f in files:
        z = np.load(out_dir / f)
        R = z["scores"].shape[0]
        assert 1 <= R <= 6 and z["sample"].tolist() == sorted(z["sample"].tolist())
        assert all(z["sample"].tolist().count(b) <= 3 for b in (0, 1)) and set(z["sample"].tolist()) <= {0, 1}
        assert z["blocks"].tolist() == [-1]
        for s in ("lidar", "map"):
            assert z[s].shape == (1, R, 4, 6) and z[s].dtype == np.float32
            assert z[s + "_cls"].shape == (1, R) and z[s + "_cells"].shape == (R, 2)
            total = z[s].astype(np.float64).sum(axis=(-2, -1)) + z[s + "_cls"]
            assert np.abs(total - 1.0).max() < 1e-5
        assert z["boxes_xywha"].shape == (R, 5)
        for b in (0, 1):  # best first inside a sample
            sc = z["scores"][z["sample"] == b]
            assert np.all(sc[:-1] >= sc[1:])
    # the detections do not depend on the flag
    plain, dumped = recorded
    assert len(plain) == len(dumped) == 4
    for p, d in zip(plain, dumped):
        assert p.keys() == d.keys()
        for k in p:
            assert torch.equal(p[k], d[k]), k

