"""Pretrained and cross-grid checkpoint loading on the GPU: ivit_pos_resample against torch's own
CPU f64 ``F.interpolate(mode='bicubic', antialias=True)``, ivit_adapt_input_conv against timm's
formula computed by torch on the CPU, and the load paths built on them (resample_abs_pos_embed,
create_model(pretrained=True), load_pretrained, set_input_size, load_state_dict_regrid, the
train_vit / eval_vit flags).

The resample limit is max|dst - ref64| <= 1e-6 max|src|: weights and sums are f64, so the only error
is the final rounding to f32, at most 2^-24 |y| with |y| <= ~1.3 max|src| (the cubic's negative
lobes), about 8e-8; the limit leaves about 10x over that and is below what an f32 evaluation of the
same formula gives (3e-7) or torch's own f32 CPU path (2.4e-6 on the (28, 28) -> (50, 90) case)."""
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

LIMIT = 1e-6
TINY = "vit_tiny_patch8_224"
SMALL = "vit_small_patch8_224"

# (h, w), (oh, ow), D
CASES = [((7, 5), (3, 11), 6),  # mixed up / down, odd D
         ((28, 28), (50, 90), 384),  # the pretrained case
         ((50, 90), (25, 45), 384),  # 8 taps
         ((14, 14), (4, 6), 192),  # 12 and 10 taps
         ((4, 6), (4, 6), 8),  # identity weights
         ((1, 9), (1, 4), 8)]  # one axis of length 1


def ref64(src, size):
    """torch CPU f64 bicubic antialiased interpolate of a channels-last [h, w, D] field -> [oh, ow, D] f64."""
    x = src.detach().cpu().double().permute(2, 0, 1)[None]
    y = F.interpolate(x, size=tuple(size), mode="bicubic", antialias=True, align_corners=False)
    return y[0].permute(1, 2, 0).contiguous()


def torch_f32_resample(pos, old, new, prefix=1):
    """timm's resample_abs_pos_embed as torch computes it on the CPU in f32."""
    D = pos.shape[-1]
    grid = pos[:, prefix:].reshape(1, old[0], old[1], D).permute(0, 3, 1, 2)
    grid = F.interpolate(grid, size=tuple(new), mode="bicubic", antialias=True, align_corners=False)
    return torch.cat([pos[:, :prefix], grid.permute(0, 2, 3, 1).reshape(1, -1, D)], 1)


def adapt_formula(w, C):
    """timm adapt_input_conv for 3 -> C channels (C not 1), torch on the CPU in f32."""
    r = -(-C // 3)
    return w.repeat(1, r, 1, 1)[:, :C] * (3 / C)


def seeded(shape, seed):
    return 0.02 * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def rel_err(got, ref, src):
    return float((got.detach().cpu().double() - ref).abs().max() / src.detach().cpu().double().abs().max())


@pytest.mark.parametrize("hw,ohw,D", CASES, ids=[f"{a[0]}x{a[1]}-{b[0]}x{b[1]}-D{d}" for a, b, d in CASES])
def test_op_parity(hw, ohw, D):
    import ops
    src = seeded((hw[0], hw[1], D), 7)
    got = ops.pos_resample(src.cuda(), ohw)
    assert got.shape == (ohw[0], ohw[1], D) and got.dtype == torch.float32
    err = rel_err(got, ref64(src, ohw), src)
    print(f"pos_resample {hw} -> {ohw}, D {D}: max|dst - ref64| / max|src| = {err:.3e}")
    assert err <= LIMIT
    if hw == ohw:
        assert torch.equal(got.cpu(), src)  # weights (0, 1, 0, 0): the source itself
    again = ops.pos_resample(src.cuda(), ohw)
    assert torch.equal(got, again)


@pytest.mark.parametrize("c", [0.37, -3.0])
def test_constant_field_stays_constant(c):
    import ops
    for hw, ohw, D in CASES:
        got = ops.pos_resample(torch.full((hw[0], hw[1], D), c).cuda(), ohw).cpu().double()
        assert float((got - c).abs().max()) <= LIMIT * abs(c), (hw, ohw)


def test_resample_abs_pos_embed():
    import vit
    pos = seeded((1, 1 + 28 * 28, 384), 11)
    out = vit.resample_abs_pos_embed(pos.cuda(), (50, 90))
    assert out.shape == (1, 4501, 384) and out.is_cuda
    assert torch.equal(out[0, 0].cpu(), pos[0, 0])
    ref = ref64(pos[0, 1:].reshape(28, 28, 384), (50, 90)).reshape(-1, 384)
    assert rel_err(out[0, 1:], ref, pos[0, 1:]) <= LIMIT
    # explicit old_size, and no prefix row
    out2 = vit.resample_abs_pos_embed(pos.cuda(), (50, 90), old_size=(28, 28))
    assert torch.equal(out, out2)
    nopre = vit.resample_abs_pos_embed(pos[:, 1:].cuda(), (50, 90), num_prefix_tokens=0)
    assert nopre.shape == (1, 4500, 384) and torch.equal(nopre[0], out[0, 1:])
    # a non-square old grid
    rect = seeded((1, 1 + 4 * 6, 8), 12)
    out3 = vit.resample_abs_pos_embed(rect.cuda(), (6, 8), old_size=(4, 6))
    assert out3.shape == (1, 49, 8) and torch.equal(out3[0, 0].cpu(), rect[0, 0])
    assert rel_err(out3[0, 1:], ref64(rect[0, 1:].reshape(4, 6, 8), (6, 8)).reshape(-1, 8), rect[0, 1:]) <= LIMIT


def test_adapt_input_conv():
    import ops
    import vit
    w = torch.randn(192, 3, 8, 8, generator=torch.Generator().manual_seed(3)) * 0.05
    for C in (290, 9):
        got = ops.adapt_input_conv(w.cuda(), C)
        assert got.shape == (192, C, 8, 8)
        assert torch.equal(got.cpu(), adapt_formula(w, C)), C
    assert torch.equal(ops.adapt_input_conv(w.cuda(), 3).cpu(), w)
    one = ops.adapt_input_conv(w.cuda(), 1).cpu()
    ref = w.sum(1, keepdim=True)
    assert one.shape == (192, 1, 8, 8)
    assert float((one - ref).abs().max() / ref.abs().max()) <= 1e-6
    with pytest.raises(RuntimeError, match="only 3-channel weights"):
        ops.adapt_input_conv(torch.randn(192, 4, 8, 8).cuda(), 9)
    # timm's argument order, for a host tensor too (the result comes back to its device)
    host = vit.adapt_input_conv(9, w)
    assert not host.is_cuda and torch.equal(host, adapt_formula(w, 9))


@pytest.fixture(scope="module")
def tiny_source(tmp_path_factory):
    """A 'timm checkpoint': vit_tiny_patch8_224 at 56 x 56 (a 7 x 7 grid), 3 channels, with a
    classifier head, wrapped as {'model': sd}. -> (state dict, .pth path)."""
    import vit
    torch.manual_seed(21)
    sd = {k: v.detach().clone() for k, v in vit.create_model(TINY, in_chans=3, img_size=(56, 56)).state_dict().items()}
    # pos_embed / cls_token / biases away from their init values, so a missed copy shows
    for k in sd:
        if k.endswith(".bias") or k == "cls_token":
            sd[k] = 0.02 * torch.randn(sd[k].shape)
    full = dict(sd)
    full["head.weight"], full["head.bias"] = torch.randn(1000, 192) * 0.01, torch.zeros(1000)
    path = tmp_path_factory.mktemp("pretrained") / (TINY + ".pth")
    torch.save({"model": full}, str(path))
    return sd, str(path)


def _check_loaded(m, sd):
    got = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    assert set(got) == set(sd)
    assert got["pos_embed"].shape == (1, 1 + 4 * 6, 192)
    assert torch.equal(got["pos_embed"][0, 0], sd["pos_embed"][0, 0])
    ref = ref64(sd["pos_embed"][0, 1:].reshape(7, 7, 192), (4, 6)).reshape(-1, 192)
    assert rel_err(got["pos_embed"][0, 1:], ref, sd["pos_embed"][0, 1:]) <= LIMIT
    assert torch.equal(got["patch_embed.proj.weight"], adapt_formula(sd["patch_embed.proj.weight"], 9))
    for k in sd:
        if k not in ("pos_embed", "patch_embed.proj.weight"):
            assert torch.equal(got[k], sd[k]), k
    return got


def test_pretrained_into_a_stream(tiny_source):
    import vit
    sd, path = tiny_source
    m = vit.create_model(TINY, pretrained=True, in_chans=9, img_size=(32, 48), pretrained_cfg_overlay={"file": path})
    _check_loaded(m, sd)
    x = torch.randn(2, 9, 32, 48, generator=torch.Generator().manual_seed(5)).cuda()
    m = m.cuda().eval()
    with torch.no_grad():
        y = m.forward_features(x)
    assert y.shape == (2, 25, 192) and bool(torch.isfinite(y).all())
    # a second stream from a state dict prepared by torch on the CPU in f32
    ref_sd = dict(sd)
    ref_sd["pos_embed"] = torch_f32_resample(sd["pos_embed"], (7, 7), (4, 6))
    ref_sd["patch_embed.proj.weight"] = adapt_formula(sd["patch_embed.proj.weight"], 9)
    r = vit.create_model(TINY, in_chans=9, img_size=(32, 48))
    r.load_state_dict(ref_sd)
    r = r.cuda().eval()
    with torch.no_grad():
        yr = r.forward_features(x)
    err = float((y - yr).abs().max() / yr.abs().max())
    print(f"forward, device-prepared vs torch-f32-prepared weights: {err:.3e}")
    assert err <= 1e-3
    # load_pretrained on a stream already on the device, from the file and from the dict
    for src in (path, {"state_dict": dict(sd)}):
        d = vit.create_model(TINY, in_chans=9, img_size=(32, 48)).cuda()
        info = d.load_pretrained(src)
        assert info["old_grid"] == (7, 7) and info["new_grid"] == (4, 6) and info["in_chans"] == (3, 9)
        assert all(torch.equal(v.cpu(), m.state_dict()[k].cpu()) for k, v in d.state_dict().items())


def test_other_pretrained_routes(tiny_source, monkeypatch, tmp_path):
    import vit
    sd, path = tiny_source
    first = _check_loaded(vit.create_model(TINY, pretrained=True, in_chans=9, img_size=(32, 48),
                                           pretrained_cfg_overlay={"file": path}), sd)
    monkeypatch.setenv("IVIT_PRETRAINED_DIR", os.path.dirname(path))
    env = vit.create_model(TINY, pretrained=True, in_chans=9, img_size=(32, 48)).state_dict()
    assert all(torch.equal(env[k], first[k]) for k in first)
    st = pytest.importorskip("safetensors.torch")
    full = dict(sd)
    full["head.weight"], full["head.bias"] = torch.zeros(1000, 192), torch.zeros(1000)
    st.save_file({k: v.contiguous() for k, v in full.items()}, str(tmp_path / (TINY + ".safetensors")))
    # by file, and through the directory (where .safetensors comes before .pth)
    by_file = vit.create_model(TINY, pretrained=True, in_chans=9, img_size=(32, 48),
                               pretrained_cfg_overlay={"file": str(tmp_path / (TINY + ".safetensors"))}).state_dict()
    assert all(torch.equal(by_file[k], first[k]) for k in first)
    monkeypatch.setenv("IVIT_PRETRAINED_DIR", str(tmp_path))
    by_dir = vit.create_model(TINY, pretrained=True, in_chans=9, img_size=(32, 48)).state_dict()
    assert all(torch.equal(by_dir[k], first[k]) for k in first)


def test_backbone_pretrained_file_kwargs(tiny_source):
    import model_vit
    sd, path = tiny_source
    bb = model_vit.TwoStreamViTBackbone(vit_model_name_lidar=TINY, vit_model_name_map=TINY, img_size=(32, 48),
                                        map_input_channels=9, lidar_input_channels=9, pretrained_map_file=path)
    _check_loaded(bb.vit_map, sd)
    assert not torch.equal(bb.vit_lidar.blocks[0].attn.qkv.weight, sd["blocks.0.attn.qkv.weight"])  # left at its init


def _small_model(img_size, seed):
    import model_vit
    torch.manual_seed(seed)
    return model_vit.IntentNetViT(backbone_cfg={"img_size": img_size, "vit_model_name_map": TINY,
                                                "drop_path_rate_lidar": 0.0, "drop_path_rate_map": 0.0}).cuda().eval()


def test_cross_grid_model():
    import model_vit
    from constants import LIDAR_TOTAL_CHANNELS, MAP_CHANNELS
    A, B = _small_model((32, 48), 31), _small_model((48, 64), 32)
    sdA = {k: v.detach().clone() for k, v in A.state_dict().items()}
    with pytest.raises(RuntimeError, match="size mismatch"):
        B.load_state_dict(sdA)  # the plain load is as strict as before
    done = model_vit.load_state_dict_regrid(B, sdA, (32, 48))
    assert done == {"backbone.vit_lidar.pos_embed": ((4, 6), (6, 8)), "backbone.vit_map.pos_embed": ((4, 6), (6, 8))}
    sdB = B.state_dict()
    assert set(sdB) == set(sdA)
    for k in sdA:
        if k in done:
            D = sdA[k].shape[-1]
            assert sdB[k].shape == (1, 49, D)
            assert torch.equal(sdB[k][0, 0], sdA[k][0, 0])
            ref = ref64(sdA[k][0, 1:].reshape(4, 6, D), (6, 8)).reshape(-1, D)
            assert rel_err(sdB[k][0, 1:], ref, sdA[k][0, 1:]) <= LIMIT
        else:
            assert torch.equal(sdB[k], sdA[k]), k
    g = torch.Generator().manual_seed(9)
    lidar = torch.randn(2, LIDAR_TOTAL_CHANNELS, 48, 64, generator=g).cuda()
    mp = torch.randn(2, MAP_CHANNELS, 48, 64, generator=g).cuda()
    with torch.no_grad():
        outB = B(lidar, mp)
    na = 6 * 8 * B.det_head.num_anchors
    assert [tuple(o.shape) for o in outB] == [(2, na, 1), (2, na, 6), (2, na, B.intention_head.num_classes)]
    assert all(bool(torch.isfinite(o).all()) for o in outB)
    # the same move on the model itself
    old = A.backbone.vit_lidar.pos_embed
    A.set_input_size((48, 64))
    assert A.backbone.vit_lidar.pos_embed is not old and isinstance(A.backbone.vit_lidar.pos_embed, torch.nn.Parameter)
    sdA2 = A.state_dict()
    assert all(torch.equal(sdA2[k], sdB[k]) for k in sdB)
    bb = A.backbone
    assert bb.img_size == (48, 64) and bb.lidar_grid_size == (6, 8) and bb.map_grid_size == (6, 8)
    assert (bb.feature_map_grid_h, bb.feature_map_grid_w) == (6, 8)
    assert bb.vit_lidar.patch_embed.img_size == (48, 64) and bb.vit_map.patch_embed.num_patches == 48
    with torch.no_grad():
        outA = A(lidar, mp)
    assert all(torch.equal(a, b) for a, b in zip(outA, outB))
    with pytest.raises(ValueError, match="timm strict size"):
        A(lidar[:, :, :32, :48].contiguous(), mp[:, :, :32, :48].contiguous())
    # the same grid: nothing resampled, a plain strict load
    assert model_vit.load_state_dict_regrid(A, sdB, (48, 64)) == {}


def test_bf16_shadows_and_packs_follow_a_load():
    """A bf16 stream that has run (its bf16 shadows and weight packs exist) and is then loaded: the
    next forward uses the loaded weights, as a freshly built stream loaded the same way does."""
    import vit
    torch.manual_seed(41)
    src = {k: v.detach().clone() for k, v in vit.create_model(SMALL, in_chans=3, img_size=(56, 56)).state_dict().items()}
    x = torch.randn(2, 9, 32, 48, generator=torch.Generator().manual_seed(6)).cuda()

    def stream():
        s = vit.create_model(SMALL, in_chans=9, img_size=(32, 48)).cuda().eval()
        for mod in s.modules():
            mod.compute_dtype = torch.bfloat16
        return s

    used = stream()
    with torch.no_grad():
        before = used.forward_features(x)
    used.load_pretrained(src)
    fresh = stream()
    fresh.load_pretrained(src)
    with torch.no_grad():
        after, want = used.forward_features(x), fresh.forward_features(x)
    assert torch.equal(after, want)
    assert not torch.equal(after, before)


def _anchor_count(text):
    line = [ln for ln in text.splitlines() if ln.startswith("Anchors for ViT evaluation")][-1]
    return int(line.split("shape: (")[1].split(",")[0])


def test_entry_points(tmp_path, capsys):
    import eval_vit
    import train_vit
    import vit
    torch.manual_seed(51)
    P = str(tmp_path / "timm_small.pth")
    src = vit.create_model(SMALL, in_chans=3, img_size=(56, 56)).state_dict()
    torch.save({"model": dict(src, **{"head.weight": torch.zeros(10, 384), "head.bias": torch.zeros(10)})}, P)
    common = ["--synthetic", "--epochs", "1", "--batches-per-epoch", "1", "--batch", "2", "--dtype", "fp32"]
    d1, d2 = tmp_path / "a", tmp_path / "b"
    assert train_vit.main(common + ["--grid", "32x48", "--pretrained-lidar", P, "--save-dir", str(d1)]) == 0
    out = capsys.readouterr().out
    from constants import LIDAR_TOTAL_CHANNELS
    assert "Pretrained vit_lidar from" in out and "7x7 -> 4x6" in out
    assert f"3 -> {LIDAR_TOTAL_CHANNELS} channels" in out
    ck = eval_vit.load_checkpoint(str(d1 / "vit_model.pth"), torch.device("cpu"))
    assert ck["backbone_cfg"]["pretrained_lidar"] is False and ck["backbone_cfg"]["pretrained_map"] is False
    assert tuple(ck["backbone_cfg"]["img_size"]) == (32, 48)
    assert train_vit.main(common + ["--grid", "48x64", "--init-from", str(d1 / "vit_model.pth"),
                                    "--save-dir", str(d2)]) == 0
    out = capsys.readouterr().out
    assert "Initialised from" in out and "vit_lidar pos_embed 4x6 -> 6x8" in out and "vit_map pos_embed 4x6 -> 6x8" in out
    ck2 = eval_vit.load_checkpoint(str(d2 / "vit_model.pth"), torch.device("cpu"))
    assert ck2["model_state_dict"]["backbone.vit_lidar.pos_embed"].shape == (1, 49, 384)
    ev = ["--synthetic", "--grid", "48x64", "--batch", "2", "--batches", "1", "--checkpoint", str(d1 / "vit_model.pth")]
    assert eval_vit.main_eval_vit(ev + ["--regrid"]) == 0
    out = capsys.readouterr().out
    assert "--regrid: backbone.vit_lidar.pos_embed 4x6 -> 6x8" in out
    n_regrid = _anchor_count(out)
    assert eval_vit.main_eval_vit(ev) == 0  # as before: the checkpoint's own 32 x 48
    out = capsys.readouterr().out
    assert "--regrid" not in out
    assert n_regrid == 2 * _anchor_count(out)  # 6 x 8 cells against 4 x 6
