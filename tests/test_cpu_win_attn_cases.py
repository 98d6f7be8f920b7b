"""The windowed-attention cases prove themselves (tests/win_attn_cases.py): every token is in exactly
one window, ragged cases have short edge windows, the f64 reference's rows sum to 1 over their window
and are 0 outside it, a 1 x 1 window gives o = v, a window covering the grid is plain global attention
over the patch tokens; and the CPU side of the feature: the default global-block rule and the parsing
of --window / --global-blocks."""
import pytest
import torch

import win_attn_cases as wc


@pytest.mark.parametrize("name", sorted(wc.CASES))
def test_partition(name):
    gh, gw, wh, ww, _ = wc.CASES[name]
    ids = wc.window_ids(gh, gw, wh, ww)
    toks = wc.window_tokens(gh, gw, wh, ww)
    seen = torch.cat(toks + [torch.tensor([0])])
    assert sorted(seen.tolist()) == list(range(1 + gh * gw))  # each token once
    assert int((ids == ids[0]).sum()) == 1  # CLS alone
    assert len(toks) == (-(-gh // wh)) * (-(-gw // ww))
    for t in toks:
        r, c = (t - 1) // gw, (t - 1) % gw
        assert int(r.max() - r.min()) < wh and int(c.max() - c.min()) < ww
        assert len(t) == int(r.max() - r.min() + 1) * int(c.max() - c.min() + 1) <= 256


def test_ragged_cases_are_ragged():
    sizes = lambda n: sorted({len(t) for t in wc.window_tokens(*wc.CASES[n][:4])})
    assert sizes("exact_4x6_w2x3") == [6]
    assert sizes("ragged_5x7_w2x3") == [1, 2, 3, 6]
    assert sizes("ragged_5x7_w3x7") == [14, 21]
    assert sizes("nw100_20x30_w10x10") == [100]
    assert sizes("nw256_16x32_w16x16") == [256]
    assert sizes("nw256_17x17_w16x16") == [1, 16, 256]
    assert sizes("nw1_3x3_w1x1") == [1]
    assert sizes("single_4x6_w4x6") == [24] and sizes("larger_4x6_w8x8") == [24]


@pytest.mark.parametrize("name", ["ragged_5x7_w2x3", "exact_4x6_w2x3", "nw1_3x3_w1x1"])
@pytest.mark.parametrize("q2", [False, True])
def test_reference_rows(name, q2):
    gh, gw, wh, ww, H = wc.CASES[name]
    qkv, dout = wc.make_inputs(name)
    ref = wc.reference(wc.q2_inputs(qkv, H) if q2 else qkv, dout, gh, gw, wh, ww, H, q2=q2)
    ids = wc.window_ids(gh, gw, wh, ww)
    same = ids.view(-1, 1) == ids.view(1, -1)
    p = ref["p"]
    assert float((p.sum(-1) - 1).abs().max()) < 1e-12
    assert float(p[..., ~same].abs().max()) == 0.0
    N, D = 1 + gh * gw, H * 64
    # CLS: o = v, dv = dout, dq = dk = 0
    cls = torch.arange(wc.B) * N
    assert torch.equal(ref["out"][cls], qkv[cls, 2 * D:].double())
    assert torch.equal(ref["dqkv"][cls, 2 * D:], dout[cls].double())
    assert float(ref["dqkv"][cls, :2 * D].abs().max()) == 0.0
    if name == "nw1_3x3_w1x1":
        assert torch.equal(ref["out"], qkv[:, 2 * D:].double())
        assert torch.equal(ref["dqkv"][:, 2 * D:], dout.double())
        assert float(ref["dqkv"][:, :2 * D].abs().max()) == 0.0


def test_q2_reference_matches_plain():
    """The q2 reference on exactly scaled inputs is the plain one (lse in log2 units)."""
    name = "ragged_5x7_w2x3"
    gh, gw, wh, ww, H = wc.CASES[name]
    qkv, dout = wc.make_inputs(name)
    D = H * 64
    q2 = qkv.double().clone()
    q2[:, :D] *= wc.C2
    a = wc.reference(qkv, dout, gh, gw, wh, ww, H)
    b = wc.reference(q2, dout, gh, gw, wh, ww, H, q2=True)
    assert float((a["out"] - b["out"]).abs().max()) < 1e-12
    assert float((a["dqkv"] - b["dqkv"]).abs().max()) < 1e-11
    assert float((a["lse"] / wc.LN2 - b["lse"]).abs().max()) < 1e-12


@pytest.mark.parametrize("name", ["single_4x6_w4x6", "larger_4x6_w8x8"])
def test_whole_grid_window_is_global_attention(name):
    gh, gw, wh, ww, H = wc.CASES[name]
    qkv, dout = wc.make_inputs(name)
    ref = wc.reference(qkv, dout, gh, gw, wh, ww, H)
    N, D = 1 + gh * gw, H * 64
    x = qkv.double().reshape(wc.B, N, 3, H, 64)[:, 1:].permute(2, 0, 3, 1, 4)
    full = torch.ones(N - 1, N - 1, dtype=torch.bool)
    out = wc.masked_attention(x[0], x[1], x[2], full)[0].permute(0, 2, 1, 3).reshape(wc.B, N - 1, D)
    assert float((ref["out"].reshape(wc.B, N, D)[:, 1:] - out).abs().max()) < 1e-12


# ------------------------------------------------------------------------------- the CPU side
def test_default_global_indexes():
    import vit
    assert vit.default_global_attn_indexes(12) == (2, 5, 8, 11) == wc.default_global_indexes(12)
    assert vit.default_global_attn_indexes(8) == (1, 3, 5, 7)
    assert vit.default_global_attn_indexes(2) == (1,)
    assert vit.resolve_global_attn_indexes(12, None) == (2, 5, 8, 11)
    assert vit.resolve_global_attn_indexes(12, (-1, 3, 3)) == (3, 11)
    for bad in [(12,), (-13,)]:
        with pytest.raises(ValueError):
            vit.resolve_global_attn_indexes(12, bad)


def test_model_keywords_cpu():
    """Block modes of a stream built on the host; state_dict keys do not change."""
    import vit
    kw = dict(img_size=(40, 56), patch_size=8, in_chans=3, embed_dim=128, depth=12, num_heads=2)
    plain = vit.VisionTransformer(**kw)
    assert plain.windowed_blocks() == [] and all(b.window_size is None for b in plain.blocks)
    win = vit.VisionTransformer(**kw, window_size=(2, 3))
    assert win.windowed_blocks() == [0, 1, 3, 4, 6, 7, 9, 10]
    assert win.blocks[0].window_size == (2, 3) and win.blocks[11].window_size is None
    assert list(win.state_dict()) == list(plain.state_dict())
    win.load_state_dict(plain.state_dict(), strict=True)
    assert vit.VisionTransformer(**kw, window_size=(2, 3), global_attn_indexes=(-1,)).windowed_blocks() == list(range(11))
    with pytest.raises(ValueError):
        vit.VisionTransformer(**kw, window_size=(2, 3), global_attn_indexes=(12,))
    with pytest.raises(ValueError):
        vit.VisionTransformer(**kw, window_size=(17, 16))
    m = vit.create_model("vit_tiny_patch8_224", in_chans=3, img_size=(40, 56), window_size=(2, 3))
    assert m.windowed_blocks() == [0, 1, 3, 4, 6, 7, 9, 10]


def test_mae_refuses_windowed_encoder():
    import mae
    import vit
    enc = vit.VisionTransformer(img_size=(40, 56), patch_size=8, in_chans=3, embed_dim=128, depth=2, num_heads=2,
                                window_size=(2, 3), global_attn_indexes=(1,))
    with pytest.raises(ValueError, match="windowed"):
        mae.MaskedAutoencoderViT(enc)


def test_window_flags():
    import eval_vit
    import train_cnn
    import train_vit
    assert train_vit.parse_window("10x10") == (10, 10) and train_vit.parse_window("2X3") == (2, 3)
    assert train_vit.parse_window("16") == (16, 16)
    for bad in ["", "x", "0x4", "17x16", "2x3x4", "axb", "-2x3"]:
        with pytest.raises(ValueError):
            train_vit.parse_window(bad)
    assert train_vit.parse_global_blocks("2,5,-1") == (2, 5, -1)
    for bad in ["", "a,b", "1;2"]:
        with pytest.raises(ValueError):
            train_vit.parse_global_blocks(bad)
    a = train_vit.parse_args(["--synthetic", "--window", "10x10"])
    assert a.window_size == (10, 10) and a.global_attn_indexes is None
    a = train_vit.parse_args(["--synthetic", "--window", "2x3", "--global-blocks", "1,-1"])
    assert a.window_size == (2, 3) and a.global_attn_indexes == (1, -1)
    a = train_vit.parse_args(["--synthetic"])
    assert a.window_size is None and a.global_attn_indexes is None
    for bad in [["--window", "17x16"], ["--window", "ten"], ["--global-blocks", "1"],
                ["--window", "2x3", "--global-blocks", "x"]]:
        with pytest.raises(SystemExit):
            train_vit.parse_args(["--synthetic"] + bad)
    e = eval_vit.parse_args(["--synthetic", "--window", "5x9", "--global-blocks", "11"])
    assert e.window_size == (5, 9) and e.global_attn_indexes == (11,)
    assert eval_vit.parse_args(["--synthetic"]).window_size is None
    e = eval_vit.parse_args(["--synthetic", "--global-blocks", "3,7"])  # alone: the checkpoint's window
    assert e.window_size is None and e.global_attn_indexes == (3, 7)
    with pytest.raises(SystemExit, match="--window"):
        train_cnn.main(["--synthetic", "--window", "10x10"])
    cfg = train_vit.backbone_cfg((40, 56))
    assert "vit_window_size" not in cfg and "vit_global_attn_indexes" not in cfg
    cfg = train_vit.backbone_cfg((40, 56), (2, 3), (1,))
    assert cfg["vit_window_size"] == (2, 3) and cfg["vit_global_attn_indexes"] == (1,)
