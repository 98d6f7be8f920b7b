"""Windowed attention at model level: vit.VisionTransformer(window_size=, global_attn_indexes=) against a
plain-torch f64 module with a masked softmax; the default model unchanged bit for bit; the bf16
row-panel path (ops.ViTBlockPanelFn) with DropPath against its own f32 run, judged by what the same
model with windows off does; attention_rows, the MAE refusal, and IntentNetViT with vit_window_size
(train step, checkpoint round trip, --init-from a global checkpoint)."""
import math

import pytest
import torch
import torch.nn.functional as F

import win_attn_cases as wc

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _eq(a, b):
    return bool((a == b).all())


def _rel(got, ref):
    ref = ref.double()
    s = float(ref.abs().max())
    return float((got.double() - ref).abs().max()) / (s if s > 0 else 1.0)


def _randomise(m, seed):
    """Parameters of a size that makes every branch matter (the default init leaves cls / biases at 0)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            v = torch.randn(p.shape, generator=g) * (0.02 if name in ("cls_token", "pos_embed") else 0.05)
            if p.dim() == 1 and name.endswith("weight"):  # LayerNorm gains around 1
                v += 1.0
            p.copy_(v.to(p.device))
    return m


# ------------------------------------------------------------------------------- f32 stream vs torch f64
def _torch_stream(sd, x, depth, heads, grid, windows):
    """forward_features of the stream in plain torch f64. sd: f64 leaves keyed as the state dict;
    windows[i]: (wh, ww) or None."""
    gh, gw = grid
    N = 1 + gh * gw
    B = x.shape[0]
    D = sd["cls_token"].shape[-1]
    t = F.conv2d(x, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=8).flatten(2).transpose(1, 2)
    t = torch.cat([sd["cls_token"].expand(B, -1, -1), t], 1) + sd["pos_embed"]
    for i in range(depth):
        p = lambda k: sd[f"blocks.{i}.{k}"]
        h = F.layer_norm(t, (D,), p("norm1.weight"), p("norm1.bias"), 1e-6)
        qkv = (h @ p("attn.qkv.weight").T + p("attn.qkv.bias")).reshape(B, N, 3, heads, 64).permute(2, 0, 3, 1, 4)
        if windows[i] is None:
            mask = torch.ones(N, N, dtype=torch.bool)
        else:
            ids = wc.window_ids(gh, gw, *windows[i])
            mask = ids.view(N, 1) == ids.view(1, N)
        o = wc.masked_attention(qkv[0], qkv[1], qkv[2], mask)[0].permute(0, 2, 1, 3).reshape(B, N, D)
        t = t + o @ p("attn.proj.weight").T + p("attn.proj.bias")
        h = F.layer_norm(t, (D,), p("norm2.weight"), p("norm2.bias"), 1e-6)
        h = F.gelu(h @ p("mlp.fc1.weight").T + p("mlp.fc1.bias"))
        t = t + h @ p("mlp.fc2.weight").T + p("mlp.fc2.bias")
    return F.layer_norm(t, (D,), sd["norm.weight"], sd["norm.bias"], 1e-6)


def test_f32_stream_vs_torch_f64():
    """grid 5 x 7, window 2 x 3 (ragged both ways), block 0 windowed, block 1 global: forward within
    1e-4 of scale, every parameter gradient within 1e-3 of its own scale."""
    import vit
    m = vit.VisionTransformer(img_size=(40, 56), patch_size=8, in_chans=3, embed_dim=128, depth=2, num_heads=2,
                              window_size=(2, 3), global_attn_indexes=(1,))
    assert [b.window_size for b in m.blocks] == [(2, 3), None]
    m = _randomise(m, 3).to(DEV).train()
    g = torch.Generator().manual_seed(4)
    x = torch.randn((2, 3, 40, 56), generator=g)
    gy = torch.randn((2, 36, 128), generator=g)
    y = m.forward_features(x.to(DEV))
    y.backward(gy.to(DEV))
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in m.named_parameters()}
    ry = _torch_stream(sd, x.double(), 2, 2, (5, 7), [(2, 3), None])
    ry.backward(gy.double())
    e = _rel(y.detach().cpu(), ry.detach())
    print(f"win_model f32 forward {e:.3e}")
    assert e <= 1e-4, e
    bad = {}
    for k, p in m.named_parameters():
        ge = _rel(p.grad.cpu(), sd[k].grad)
        if not ge <= 1e-3:
            bad[k] = ge
    assert not bad, bad


def test_default_is_todays_model():
    import vit
    kw = dict(img_size=(40, 56), patch_size=8, in_chans=3, embed_dim=128, depth=2, num_heads=2, drop_path_rate=0.0)
    a = _randomise(vit.VisionTransformer(**kw), 5).to(DEV)
    b = _randomise(vit.VisionTransformer(**kw, window_size=None), 5).to(DEV)
    assert a.windowed_blocks() == [] and b.windowed_blocks() == []
    x = torch.randn((2, 3, 40, 56), generator=torch.Generator().manual_seed(6)).to(DEV)
    for mode in (True, False):
        a.train(mode), b.train(mode)
        with torch.no_grad():
            assert _eq(a.forward_features(x), b.forward_features(x))


# ------------------------------------------------------------------------------- bf16 row-panel path
KEEP = 1.0 / (1.0 - 0.1)


def _panel_model(seed):
    import vit
    m = vit.VisionTransformer(img_size=(40, 56), patch_size=8, in_chans=3, embed_dim=384, depth=2, num_heads=6,
                              drop_path_rate=0.1, window_size=(2, 3), global_attn_indexes=(1,))
    return _randomise(m, seed).to(DEV).train()


def _panel_run(m, dtype, windowed):
    """forward_features + parameter gradients with injected DropPath factors that drop sample 1 in the
    attention branch of block 0 (the windowed one)."""
    m.compute_dtype = dtype
    m.blocks[0].window_size = (2, 3) if windowed else None
    m.set_drop_path_scales([(torch.tensor([KEEP, 0.0]), torch.tensor([KEEP, KEEP])),
                            (torch.tensor([KEEP, KEEP]), torch.tensor([0.0, KEEP]))])
    m.zero_grad(set_to_none=True)
    g = torch.Generator().manual_seed(8)
    x = torch.randn((2, 3, 40, 56), generator=g).to(DEV)
    gy = torch.randn((2, 36, 384), generator=g).to(DEV)
    y = m.forward_features(x)
    y.backward(gy)
    torch.cuda.synchronize()
    return y.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()}


def test_bf16_panel_path_vs_own_f32():
    """bf16 on ops.ViTBlockPanelFn (D = 384) with DropPath: the windowed model's distance from its own
    f32 run is at most 1.5 x that of the same model with windows off (forward; and the worst parameter
    gradient, each on its own scale). Both are measured here; the yardstick is the existing path."""
    import ops
    from _lib import BF16
    assert ops.block_on_panel(BF16, 384)
    m = _panel_model(7)
    err = {}
    for windowed in (True, False):
        y32, g32 = _panel_run(m, torch.float32, windowed)
        y16, g16 = _panel_run(m, torch.bfloat16, windowed)
        assert bool(torch.isfinite(y16).all()) and all(bool(torch.isfinite(v).all()) for v in g16.values())
        per = {k: _rel(g16[k], g32[k]) for k in g32}
        err[windowed] = (_rel(y16, y32), max(per.values()))
        print(f"win_model bf16 windowed={windowed}: forward {err[windowed][0]:.3e} worst gradient "
              f"{err[windowed][1]:.3e} ({max(per, key=per.get)})")
    assert err[True][0] <= 1.5 * err[False][0], err
    assert err[True][1] <= 1.5 * err[False][1], err


def test_dropped_sample_attention_branch_is_zero():
    """A block on the row-panel path, sample 1 dropped in the attention branch: its rows of the output do
    not depend on the attention at all — bitwise the same from the windowed and from the global block, and
    unchanged when the qkv weights change — while sample 0's rows differ."""
    import vit
    from _lib import BF16
    B, gh, gw = 2, 5, 7
    N = 1 + gh * gw
    blk = _randomise(vit.Block(384, 6, 4.0, 0.1), 9).to(DEV).train()
    blk.drop_path_scales = (torch.tensor([KEEP, 0.0]), torch.tensor([KEEP, KEEP]))
    x = torch.randn((B * N, 384), generator=torch.Generator().manual_seed(10)).to(DEV)
    runs = []
    for win, bump in (((2, 3), False), (None, False), ((2, 3), True)):
        blk.window_size = win
        if bump:
            with torch.no_grad():
                blk.attn.qkv.weight.mul_(1.5)
        xi = x.clone().requires_grad_(True)
        y = blk.forward_flat(xi, B, N, BF16, grid=(gh, gw))[0]
        y.sum().backward()
        assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(xi.grad).all())
        runs.append(y.detach().reshape(B, N, 384).clone())
    assert _eq(runs[0][1], runs[1][1]) and _eq(runs[0][1], runs[2][1])
    assert not _eq(runs[0][0], runs[1][0]) and not _eq(runs[0][0], runs[2][0])
    with pytest.raises(ValueError):
        blk.forward_flat(x, B, N, BF16)  # a windowed block needs the grid


# ------------------------------------------------------------------------------- the model's other doors
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_attention_rows(dtype):
    m = _panel_model(11).eval()
    m.compute_dtype = dtype
    m.blocks[0].window_size = (2, 3)
    x = torch.randn((2, 3, 40, 56), generator=torch.Generator().manual_seed(12)).to(DEV)
    with pytest.raises(ValueError, match=r"block\(s\) \[0\].*global blocks available: \[1\]"):
        m.attention_rows(x, [0, 1], [3, 0], blocks=[0])
    with pytest.raises(ValueError):
        m.attention_rows(x, [0, 1], [3, 0])  # all blocks: block 0 is windowed
    rows = m.attention_rows(x, [0, 1], [3, 0], blocks=[-1])
    assert rows.shape == (1, 2, 36)
    assert float((rows.sum(-1) - 1).abs().max()) < 1e-5


def test_mae_refuses_windowed_encoder():
    import mae
    import vit
    enc = vit.VisionTransformer(img_size=(40, 56), patch_size=8, in_chans=3, embed_dim=384, depth=2, num_heads=6,
                                window_size=(2, 3), global_attn_indexes=(1,)).to(DEV)  # no DropPath, as create_mae
    with pytest.raises(ValueError, match="windowed"):
        mae.MaskedAutoencoderViT(enc)
    enc.blocks[0].window_size = None
    mae.MaskedAutoencoderViT(enc)  # the same encoder with every block global is accepted


def test_set_input_size_moves_the_window_grid():
    """The window grid is read from patch_embed.grid_size at call time."""
    m = _panel_model(14).eval()
    m.compute_dtype = torch.bfloat16
    m.set_input_size((48, 64))
    x = torch.randn((2, 3, 48, 64), generator=torch.Generator().manual_seed(15)).to(DEV)
    with torch.no_grad():
        y = m.forward_features(x)
    assert y.shape == (2, 49, 384) and bool(torch.isfinite(y).all())


# ------------------------------------------------------------------------------- IntentNetViT
def _intentnet(window, seed=0):
    import model_vit
    import train_vit
    torch.manual_seed(seed)
    cfg = train_vit.backbone_cfg((32, 48), window, None)
    return model_vit.IntentNetViT(backbone_cfg=cfg).to(DEV), cfg


def test_intentnet_train_step():
    import loss as L
    import utils
    from oracle import ivit_oracle as O
    m, _ = _intentnet((2, 3))
    assert m.backbone.vit_lidar.windowed_blocks() == [0, 1, 3, 4, 6, 7, 9, 10] == m.backbone.vit_map.windowed_blocks()
    m.set_compute_dtype(torch.bfloat16).train()
    lidar, mp, gts = O.synthetic_batch(2, (32, 48), seed=3, grid_scale=32 / 400.0)
    anchors = utils.generate_anchors(32, 48, 8, device=DEV)
    c, b, i = m(lidar.to(DEV), mp.to(DEV))
    d = L.DetectionIntentionLoss()(c, b, i, anchors, gts)
    d["loss"].backward()
    assert bool(torch.isfinite(d["loss"]))
    bad = [k for k, p in m.named_parameters() if p.grad is None or not bool(torch.isfinite(p.grad).all())]
    assert not bad, bad


def test_intentnet_checkpoint_round_trip(tmp_path):
    import eval_vit
    import model_vit
    from oracle import ivit_oracle as O
    m, cfg = _intentnet((2, 3), seed=1)
    m.eval()
    path = str(tmp_path / "win.pth")
    torch.save({"epoch": 1, "model_state_dict": m.state_dict(), "backbone_cfg": cfg}, path)
    ck = eval_vit.load_checkpoint(path, torch.device(DEV))
    assert tuple(ck["backbone_cfg"]["vit_window_size"]) == (2, 3)
    assert ck["backbone_cfg"]["vit_global_attn_indexes"] is None
    m2 = model_vit.IntentNetViT(backbone_cfg=eval_vit.default_cfg(dict(ck["backbone_cfg"]), (32, 48))).to(DEV).eval()
    m2.load_state_dict(ck["model_state_dict"], strict=True)
    assert m2.backbone.vit_lidar.windowed_blocks() == m.backbone.vit_lidar.windowed_blocks() != []
    lidar, mp, _ = O.synthetic_batch(2, (32, 48), seed=4, grid_scale=32 / 400.0)
    with torch.no_grad():
        a, b = m(lidar.to(DEV), mp.to(DEV)), m2(lidar.to(DEV), mp.to(DEV))
    assert all(_eq(u, v) for u, v in zip(a, b))
    # a global model of the same weights computes something else
    g, _ = _intentnet(None, seed=1)
    g.load_state_dict(m.state_dict(), strict=True)
    with torch.no_grad():
        c = g.eval()(lidar.to(DEV), mp.to(DEV))
    assert not _eq(a[0], c[0])


def test_entry_points_window_flags(tmp_path, capsys):
    """train_vit.py --window (log line, checkpoint cfg), --init-from a GLOBAL checkpoint into a windowed
    model (strict load), eval_vit.py from the checkpoint's cfg and with the flags on a synthetic run."""
    import eval_vit
    import train_vit
    common = ["--synthetic", "--epochs", "1", "--batches-per-epoch", "1", "--batch", "2", "--dtype", "bf16", "--grid",
              "32x48"]
    d1, d2 = tmp_path / "global", tmp_path / "win"
    assert train_vit.main(common + ["--save-dir", str(d1)]) == 0
    assert "Windowed attention" not in capsys.readouterr().out
    ck = eval_vit.load_checkpoint(str(d1 / "vit_model.pth"), torch.device("cpu"))
    assert "vit_window_size" not in ck["backbone_cfg"]
    assert train_vit.main(common + ["--window", "2x3", "--global-blocks", "5,-1", "--init-from",
                                    str(d1 / "vit_model.pth"), "--save-dir", str(d2)]) == 0
    out = capsys.readouterr().out
    assert "Windowed attention: 2x3 patches, global blocks [5, 11], 4 windows per stream on the 4x6 grid" in out
    assert "Initialised from" in out
    ck2 = eval_vit.load_checkpoint(str(d2 / "vit_model.pth"), torch.device("cpu"))
    assert tuple(ck2["backbone_cfg"]["vit_window_size"]) == (2, 3)
    assert tuple(ck2["backbone_cfg"]["vit_global_attn_indexes"]) == (5, -1)
    assert sorted(ck2["model_state_dict"]) == sorted(ck["model_state_dict"])
    ev = ["--synthetic", "--grid", "32x48", "--batch", "2", "--batches", "1"]
    assert eval_vit.main_eval_vit(ev + ["--checkpoint", str(d2 / "vit_model.pth")]) == 0
    assert "Windowed attention: 2x3 patches, global blocks [5, 11]" in capsys.readouterr().out
    # --global-blocks alone overrides the global blocks of the checkpoint's window
    assert eval_vit.main_eval_vit(ev + ["--checkpoint", str(d2 / "vit_model.pth"), "--global-blocks", "3"]) == 0
    assert "Windowed attention: 2x3 patches, global blocks [3]" in capsys.readouterr().out
    with pytest.raises(SystemExit, match="--global-blocks"):
        eval_vit.main_eval_vit(ev + ["--checkpoint", str(d1 / "vit_model.pth"), "--global-blocks", "3"])
    capsys.readouterr()
    assert eval_vit.main_eval_vit(ev + ["--checkpoint", str(tmp_path / "none.pth"), "--window", "4x3"]) == 0
    assert "Windowed attention: 4x3 patches, global blocks [2, 5, 8, 11], 2 windows" in capsys.readouterr().out
