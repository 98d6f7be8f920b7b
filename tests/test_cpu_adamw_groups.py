"""Fine-tuning parameter groups and schedule, the parts that need no GPU: the layer ids, lr scales and
no-decay set of optim.layer_decay_param_groups against a table written out here, optim.WarmupCosineLR
against its closed form, the new flags of the training parsers, and the argument refusals of
ivit_adamw_chunked_pt (before any device call, with a message). No kernel is launched."""
import ctypes
import math
import os

import pytest
import torch

import _lib
from conftest import REPO

LIB = os.path.join(REPO, "visiontransformer-intention-prediction_amd", "libivit_hip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libivit_hip.so not built (run __graft_entry__.build())")

DECAY, WD, DEPTH = 0.75, 0.05, 12


def _vit():
    import model_vit
    return model_vit.IntentNetViT(backbone_cfg={"img_size": (32, 48), "drop_path_rate_lidar": 0.0,
                                                "drop_path_rate_map": 0.0})


def _expected_layer(name):
    """The rule, written out for IntentNetViT's names (two streams of depth 12)."""
    for stream in ("backbone.vit_lidar.", "backbone.vit_map."):
        if name.startswith(stream):
            rest = name[len(stream):]
            if rest in ("pos_embed", "cls_token") or rest.startswith("patch_embed."):
                return 0
            if rest.startswith("blocks."):
                return int(rest.split(".")[1]) + 1
            assert rest in ("norm.weight", "norm.bias"), rest
            return DEPTH + 1
    assert name.split(".")[0] in ("det_head", "intention_head") or \
        name.split(".")[1] in ("adapter_lidar", "adapter_map", "fusion_block"), name
    return DEPTH + 1


def _by_param(groups):
    out = {}
    for gi, g in enumerate(groups):
        for p in g["params"]:
            assert id(p) not in out  # every parameter exactly once
            out[id(p)] = (gi, g)
    return out


def test_vit_layer_ids_scales_and_no_decay_set():
    import optim
    m = _vit()
    assert len(m.backbone.vit_lidar.blocks) == len(m.backbone.vit_map.blocks) == DEPTH
    groups = optim.layer_decay_param_groups(m, DECAY, WD, no_decay_1d=True)
    where = _by_param(groups)
    named = list(m.named_parameters())
    assert len(where) == len(named) == sum(len(g["params"]) for g in groups)
    seen_nodecay = 0
    for name, p in named:
        _, g = where[id(p)]
        lid = _expected_layer(name)
        assert g["lr_scale"] == DECAY ** (DEPTH + 1 - lid), name  # f64, exact
        nodecay = p.ndim <= 1 or name.endswith(".bias") or name.endswith("pos_embed") or name.endswith("cls_token")
        assert g["weight_decay"] == (0.0 if nodecay else WD), name
        seen_nodecay += nodecay
    # spot values of the table: embeddings lowest, block 0 one step up, last block 0.75, the rest 1
    scale = {n: where[id(p)][1]["lr_scale"] for n, p in named}
    for s in ("backbone.vit_lidar.", "backbone.vit_map."):
        assert scale[s + "pos_embed"] == scale[s + "cls_token"] == scale[s + "patch_embed.proj.weight"] == 0.75 ** 13
        assert scale[s + "blocks.0.attn.qkv.weight"] == 0.75 ** 12
        assert scale[s + "blocks.11.mlp.fc2.bias"] == 0.75
        assert scale[s + "norm.weight"] == 1.0
    for n in ("backbone.adapter_lidar.0.weight", "backbone.fusion_block.1.bn2.bias", "det_head.conv.weight",
              "intention_head.conv.bias"):
        assert scale[n] == 1.0
    wd = {n: where[id(p)][1]["weight_decay"] for n, p in named}
    assert wd["backbone.vit_map.pos_embed"] == wd["backbone.vit_map.cls_token"] == 0.0  # 3-D, by name
    assert wd["backbone.fusion_block.0.bn1.weight"] == wd["backbone.vit_lidar.blocks.3.norm1.weight"] == 0.0
    assert wd["det_head.conv.bias"] == 0.0 and wd["det_head.conv.weight"] == WD
    assert wd["backbone.vit_lidar.blocks.3.attn.qkv.weight"] == WD
    assert 0 < seen_nodecay < len(named)
    # 14 distinct scales, decayed and not: 28 groups, all distinct in (lr_scale, weight_decay)
    assert len({g["lr_scale"] for g in groups}) == DEPTH + 2
    assert len({(g["lr_scale"], g["weight_decay"]) for g in groups}) == len(groups) == 2 * (DEPTH + 2)
    # inside a group: named_parameters() order
    order = {id(p): i for i, (_, p) in enumerate(named)}
    for g in groups:
        idx = [order[id(p)] for p in g["params"]]
        assert idx == sorted(idx)
    rows = optim.group_summary(groups)
    assert [r[0] for r in rows] == list(range(DEPTH + 2)) and rows[-1][1] == 1.0
    assert sum(r[2] for r in rows) == len(named) and sum(r[3] for r in rows) == sum(p.numel() for _, p in named)


def test_two_constructions_give_the_same_groups():
    import optim
    a = optim.layer_decay_param_groups(_vit(), DECAY, WD)
    m = _vit()
    b = optim.layer_decay_param_groups(m, DECAY, WD)
    assert [(g["lr_scale"], g["weight_decay"], g["layer_id"], [tuple(p.shape) for p in g["params"]]) for g in a] == \
        [(g["lr_scale"], g["weight_decay"], g["layer_id"], [tuple(p.shape) for p in g["params"]]) for g in b]
    names = {id(p): n for n, p in m.named_parameters()}
    c = optim.layer_decay_param_groups(m, DECAY, WD)
    assert [[names[id(p)] for p in g["params"]] for g in b] == [[names[id(p)] for p in g["params"]] for g in c]


def test_single_group_when_everything_is_off():
    import optim
    m = _vit()
    groups = optim.layer_decay_param_groups(m, 1.0, 1e-4, no_decay_1d=False)
    assert len(groups) == 1
    g = groups[0]
    assert g["lr_scale"] == 1.0 and g["weight_decay"] == 1e-4
    assert [id(p) for p in g["params"]] == [id(p) for p in m.parameters()]
    # layer decay alone: one group per scale; no-decay alone: two groups
    assert len(optim.layer_decay_param_groups(m, DECAY, 1e-4, no_decay_1d=False)) == DEPTH + 2
    two = optim.layer_decay_param_groups(m, 1.0, 1e-4, no_decay_1d=True)
    assert sorted(g["weight_decay"] for g in two) == [0.0, 1e-4] and all(g["lr_scale"] == 1.0 for g in two)
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="layer_decay"):
            optim.layer_decay_param_groups(m, bad, 1e-4)


def test_cnn_has_scale_one_everywhere():
    import optim
    import train_vit
    from model_cnn import IntentNetCNN
    m = IntentNetCNN(backbone_cfg=train_vit.cnn_backbone_cfg())
    groups = optim.layer_decay_param_groups(m, DECAY, WD, no_decay_1d=True)
    assert len(groups) == 2 and all(g["lr_scale"] == 1.0 for g in groups)
    where = _by_param(groups)
    for name, p in m.named_parameters():
        g = where[id(p)][1]
        assert g["weight_decay"] == (0.0 if p.ndim <= 1 or name.endswith(".bias") else WD), name
    assert len(where) == len(list(m.parameters()))


def test_mae_mask_token_and_encoder_embeddings_are_not_decayed():
    import optim
    from mae import create_mae
    m = create_mae("vit_small_patch8_224", 9, (32, 48), decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=1)
    groups = optim.layer_decay_param_groups(m, 1.0, WD, no_decay_1d=True)
    assert len(groups) == 2 and all(g["lr_scale"] == 1.0 for g in groups)
    where = _by_param(groups)
    wd = {n: where[id(p)][1]["weight_decay"] for n, p in m.named_parameters()}
    assert len(wd) == len(where)
    assert m.mask_token.ndim == 3 and wd["mask_token"] == 0.0
    assert wd["encoder.pos_embed"] == wd["encoder.cls_token"] == wd["decoder_norm.weight"] == wd["decoder_pred.bias"] == 0.0
    assert wd["decoder_embed.weight"] == wd["encoder.blocks.0.mlp.fc1.weight"] == wd["decoder_pred.weight"] == WD
    assert "decoder_pos_embed" not in wd  # a buffer here; the rule names it for models that train it
    # the encoder is a stream: with a decay its embeddings sit 13 layers below the decoder
    lay = optim.layer_decay_param_groups(m, DECAY, WD)
    sc = {n: _by_param(lay)[id(p)][1]["lr_scale"] for n, p in m.named_parameters()}
    assert sc["encoder.pos_embed"] == 0.75 ** 13 and sc["encoder.norm.weight"] == sc["mask_token"] == 1.0


# ------------------------------------------------------------------ schedule
def _closed_form(k, W, T, base, mn, init):
    if k < W:
        return init + (base - init) * k / W
    if k >= T:
        return mn
    return mn + 0.5 * (base - mn) * (1.0 + math.cos(math.pi * (k - W) / max(1, T - W)))


def _sgd(groups):
    return torch.optim.SGD(groups, lr=1.0)


def test_warmup_cosine_values_and_state():
    import optim
    W, T, mn, init = 5, 45, 1e-6, 1e-7
    ps = [torch.nn.Parameter(torch.zeros(2)) for _ in range(2)]
    opt = _sgd([{"params": [ps[0]], "lr": 1e-3, "lr_scale": 0.75 ** 13}, {"params": [ps[1]], "lr": 2e-4, "lr_scale": 1.0}])
    s = optim.WarmupCosineLR(opt, W, T, min_lr=mn, warmup_init_lr=init)
    seen = {}
    for k in range(T + 6):
        seen[k] = [g["lr"] for g in opt.param_groups]
        assert seen[k] == s.get_last_lr()
        s.step()
    for k in (0, W - 1, W, (W + T) // 2, T, T + 5):
        assert seen[k] == [_closed_form(k, W, T, b, mn, init) for b in (1e-3, 2e-4)], k  # f64, the same expression
    assert seen[0] == [init, init] and seen[W] == [1e-3, 2e-4] and seen[T] == seen[T + 5] == [mn, mn]
    mid = (W + T) // 2  # exactly half way: cos(pi / 2)
    assert seen[mid][0] == pytest.approx(mn + 0.5 * (1e-3 - mn), rel=1e-12)
    assert all(a[0] < b[0] for a, b in zip([seen[k] for k in range(W)], [seen[k] for k in range(1, W + 1)]))
    assert all(a[0] > b[0] for a, b in zip([seen[k] for k in range(W, T)], [seen[k] for k in range(W + 1, T + 1)]))
    assert [g["lr_scale"] for g in opt.param_groups] == [0.75 ** 13, 1.0]  # not the schedule's to touch
    # state_dict round trip into a fresh optimizer at its base lr
    t = optim.WarmupCosineLR(opt, W, T, min_lr=mn, warmup_init_lr=init)
    for _ in range(17):
        t.step()
    sd = t.state_dict()
    assert "optimizer" not in sd and sd["last_step"] == 17 and sd["base_lrs"] == [1e-3, 2e-4]
    opt2 = _sgd([{"params": [ps[0]], "lr": 9.0}, {"params": [ps[1]], "lr": 9.0}])
    u = optim.WarmupCosineLR(opt2, 1, 2)
    u.load_state_dict(sd)
    assert [g["lr"] for g in opt2.param_groups] == seen[17]
    u.step()
    assert [g["lr"] for g in opt2.param_groups] == seen[18]
    with pytest.raises(ValueError, match="groups"):
        optim.WarmupCosineLR(_sgd([{"params": [ps[0]]}]), 1, 2).load_state_dict(sd)
    # no warmup, and a span of one update
    opt3 = _sgd([{"params": [ps[0]], "lr": 0.5}])
    v = optim.WarmupCosineLR(opt3, 0, 1)
    assert opt3.param_groups[0]["lr"] == 0.5
    v.step()
    assert opt3.param_groups[0]["lr"] == 0.0
    for bad in ((-1, 4), (5, 4), (0, 0)):
        with pytest.raises(ValueError, match="warmup_steps"):
            optim.WarmupCosineLR(opt3, *bad)


def test_fused_adamw_keeps_lr_scale_in_its_state_dict():
    import optim
    ps = [torch.nn.Parameter(torch.zeros(3)) for _ in range(2)]
    opt = optim.FusedAdamW([{"params": [ps[0]], "lr_scale": 0.75 ** 13, "weight_decay": 0.0},
                            {"params": [ps[1]], "lr_scale": 1.0}], lr=1e-3, weight_decay=0.05, fuse_groups=True)
    assert opt.fuse_groups is True and optim.FusedAdamW([ps[0]]).fuse_groups is False
    assert "lr_scale" not in optim.FusedAdamW([ps[0]]).param_groups[0]  # a plain group stays as it was
    sd = opt.state_dict()
    assert [g["lr_scale"] for g in sd["param_groups"]] == [0.75 ** 13, 1.0]
    fresh = optim.FusedAdamW([{"params": [ps[0]]}, {"params": [ps[1]]}], lr=1.0)
    fresh.load_state_dict(sd)
    assert [(g["lr_scale"], g["weight_decay"], g["lr"]) for g in fresh.param_groups] == \
        [(0.75 ** 13, 0.0, 1e-3), (1.0, 0.05, 1e-3)]
    # the group's learning rate: one f32 rounding of the product of the two f32 values
    import numpy as np
    for lr, sc in ((1e-3, 0.75 ** 13), (1e-4, 0.75), (3e-4, 1.0), (1.5e-4, 0.0)):
        assert optim.effective_lr(lr, sc) == float(np.float32(lr) * np.float32(sc))


# ------------------------------------------------------------------ parsers
def test_train_parser_defaults_and_errors(capsys):
    import train_cnn
    import train_vit
    a = train_vit.parse_args([])
    assert (a.lr, a.weight_decay, a.layer_decay, a.no_decay_1d, a.sched, a.warmup_epochs, a.min_lr) == \
        (train_vit.LEARNING_RATE, train_vit.WEIGHT_DECAY, None, False, "plateau", 0.0, 0.0)
    assert not train_vit.param_groups_requested(a) and train_vit.build_schedule(None, a, 16) is None
    m = torch.nn.Linear(3, 2)
    opt = train_vit.build_optimizer(m, a)
    assert len(opt.param_groups) == 1 and opt.fuse_groups is False and "lr_scale" not in opt.param_groups[0]
    assert (opt.param_groups[0]["lr"], opt.param_groups[0]["weight_decay"]) == (1e-4, 1e-4)
    assert capsys.readouterr().out == ""
    b = train_cnn.parse_args(["--layer-decay", "0.75", "--no-decay-1d", "--sched", "cosine", "--warmup-epochs", "1",
                              "--min-lr", "1e-6", "--lr", "5e-4", "--weight-decay", "0.05", "--epochs", "4"])
    assert train_vit.param_groups_requested(b) and train_vit.param_groups_requested(train_vit.parse_args(["--no-decay-1d"]))
    opt = train_vit.build_optimizer(m, b)
    out = capsys.readouterr().out
    assert opt.fuse_groups is True and len(opt.param_groups) == 2 and "lr scale 1.000000, 2 tensors, 8 elements" in out
    s = train_vit.build_schedule(opt, b, 8)
    assert (s.warmup_steps, s.total_steps, s.min_lr) == (8, 32, 1e-6) and opt.param_groups[0]["lr"] == 0.0
    # a cosine schedule needs its total from --epochs and the loader
    for argv in (["--sched", "cosine", "--epochs", "0"], ["--sched", "cosine", "--epochs", "2", "--warmup-epochs", "3"],
                 ["--layer-decay", "1.5"], ["--layer-decay", "0"], ["--sched", "linear"]):
        with pytest.raises(SystemExit):
            train_vit.parse_args(argv)
        assert "error" in capsys.readouterr().err
    with pytest.raises(SystemExit, match="no updates to schedule"):
        train_vit.build_schedule(opt, b, 0)


def test_pretrain_parser():
    import pretrain_mae
    a = pretrain_mae.parse_args([])
    assert (a.sched, a.warmup_epochs, a.min_lr, a.no_decay_1d) == ("constant", 0.0, 0.0, False)
    b = pretrain_mae.parse_args(["--sched", "cosine", "--warmup-epochs", "1", "--no-decay-1d", "--min-lr", "1e-6"])
    assert (b.sched, b.warmup_epochs, b.min_lr, b.no_decay_1d) == ("cosine", 1.0, 1e-6, True)
    assert not hasattr(b, "layer_decay")
    with pytest.raises(SystemExit):
        pretrain_mae.parse_args(["--sched", "cosine", "--epochs", "0"])


# ------------------------------------------------------------------ ABI
@needs_lib
def test_header_declares_the_entry():
    protos = _lib.parse_header()
    assert hasattr(_lib.lib.load(), "ivit_adamw_chunked_pt")
    ema, pt = protos["ivit_adamw_chunked_ema"][1], protos["ivit_adamw_chunked_pt"][1]
    assert pt == ema[:-1] + [ctypes.c_void_p] + ema[-1:]  # the EMA entry's arguments plus hyper, before the stream


@needs_lib
def test_adamw_pt_refusals():
    dll = _lib.lib.load()
    buf = (ctypes.c_double * 8)()
    b = ctypes.addressof(buf)
    tabs = (b, b, b, b, None, b)
    rest = (0.9, 0.999, 1e-8, 1e-2, 1.0, 1.0)

    def call(hyper, lr=1e-3, chunks=b, nch=1, steps=(None, None), emas=None, decay=0.0, warm=0):
        return dll.ivit_adamw_chunked_pt(1, *tabs, chunks, nch, lr, *rest, None, *steps, None, emas, decay, warm, hyper, None)

    assert call(b + 4) != 0
    assert b"ivit_adamw_chunked_pt: misaligned hyper table" in dll.ivit_last_error()
    for bad in (float("nan"), float("inf"), -1e-3):
        assert call(b, lr=bad) != 0
        assert b"ivit_adamw_chunked_pt: lr must be finite and >= 0" in dll.ivit_last_error(), dll.ivit_last_error()
        assert call(b, lr=bad, nch=0) != 0  # an empty launch does not hide a bad lr
    # the siblings' checks, under this entry's name
    for kw, msg in ((dict(chunks=None), b"bad chunk table"), (dict(chunks=b + 4), b"misaligned chunk table"),
                    (dict(steps=(b, None)), b"steps_in / steps_out pair"), (dict(steps=(b, b)), b"aliases"),
                    (dict(emas=b, decay=1.0), b"ema_decay must be in [0, 1)"),
                    (dict(emas=b, decay=0.9, warm=1), b"ema_warmup needs the device step counts"),
                    (dict(emas=b + 4, decay=0.9), b"misaligned ema table")):
        assert call(b, **kw) != 0
        assert msg in dll.ivit_last_error() and b"ivit_adamw_chunked_pt" in dll.ivit_last_error(), dll.ivit_last_error()
    assert call(b, nch=0) == 0 and call(b, lr=0.0, nch=0) == 0
    # a null table is the EMA entry (which does not look at lr), and through it the plain one
    assert call(None, lr=float("nan"), nch=0) == 0
    assert call(None, chunks=None) != 0
    assert b"ivit_adamw_chunked: bad chunk table" in dll.ivit_last_error()
    with pytest.raises(RuntimeError, match="ivit_adamw_chunked_pt failed"):
        _lib.lib.ivit_adamw_chunked_pt(1, *tabs, b, 1, 1e-3, *rest, None, None, None, None, None, 0.0, 0, b + 4, None)
