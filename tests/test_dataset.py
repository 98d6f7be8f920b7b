"""The Argoverse-2 frame loader (dataset.py, preprocess_intent_labels.py, the --data-dir mode of the
entry points) on the two-log tree of tests/golden/av2_tiny.npz, against what the REFERENCE's own
preprocess_intent_labels / dataset modules produced for it (tools/make_golden_labels.py)."""
import os
import random

import numpy as np
import pytest

from conftest import golden

pd = pytest.importorskip("pandas")
pytest.importorskip("pyarrow")

from tools.make_golden_labels import ANN_COLUMNS, write_tree  # noqa: E402

NUM_SWEEPS = 5
TAGS = ("a", "b")


@pytest.fixture(scope="module")
def tiny():
    z = golden("av2_tiny.npz")
    return {k: z[k] for k in z.files}


def _write_labelled(tiny, root):
    """The tree with the recorded heuristic_intent column already in place (no device needed)."""
    root = str(root)
    os.makedirs(root, exist_ok=True)
    for tag, d in zip(TAGS, write_tree(tiny, root)):
        df = pd.read_feather(os.path.join(d, "annotations.feather"))
        df["heuristic_intent"] = tiny[f"{tag}_heuristic_intent"]
        df.to_feather(os.path.join(d, "annotations_with_intent.feather"))
    return root


@pytest.fixture(scope="module")
def tree(tiny, tmp_path_factory):
    return _write_labelled(tiny, tmp_path_factory.mktemp("av2") / "val")


@pytest.fixture(scope="module")
def dataset(tree):
    import dataset as D
    return D.ArgoverseIntentNetDataset(tree, num_sweeps=NUM_SWEEPS, is_train=False)


def _recorded_index(tiny, seq):
    """The recorded sequence a dataset sequence corresponds to (the reference enumerates the logs
    in os.scandir order, this build in name order)."""
    hit = np.flatnonzero((tiny["seq_log"] == seq["log_id"]) & (tiny["seq_current_ts"] == seq["current_ts_ns"]))
    assert hit.size == 1
    return int(hit[0])


def _dense(tiny, prefix):
    out = np.zeros(int(np.prod(tiny[f"{prefix}_shape"])), np.float32)
    out[tiny[f"{prefix}_idx"]] = tiny[f"{prefix}_val"]
    return out.reshape(tuple(tiny[f"{prefix}_shape"]))


def _check_gt(gt, tiny, j):
    boxes, want = gt["boxes_xywha"].cpu().numpy(), tiny[f"item{j}_boxes"]
    assert boxes.dtype == np.float32 and boxes.shape == want.shape
    assert np.array_equal(boxes[:, :4], want[:, :4])
    # two f64-accurate yaws differ by at most one f32 ulp after the cast: 2.4e-7 at pi
    d = np.abs(boxes[:, 4].astype(np.float64) - want[:, 4].astype(np.float64))
    print("max heading difference", d.max() if d.size else 0.0)
    assert np.all(d <= 5e-7)
    assert gt["intentions"].dtype.is_floating_point is False
    assert np.array_equal(gt["intentions"].cpu().numpy(), tiny[f"item{j}_intentions"])


# ------------------------------------------------------------------------------------------- CPU
def test_validator_sequences_and_collate(tiny, tree, dataset, tmp_path):
    import torch
    import dataset as D
    # an empty directory, a log without sweeps and a stray file are not scenarios
    os.makedirs(os.path.join(tree, "zz-empty"), exist_ok=True)
    open(os.path.join(tree, "README"), "w").close()
    found = D.ScenarioValidator(tree).find_valid_scenarios()
    assert [os.path.basename(s.log_dir) for s in found] == sorted(tiny["logs"].tolist())
    for s in found:
        log = os.path.basename(s.log_dir)
        assert os.path.basename(s.map_path).startswith(f"log_map_archive_{log}")
        assert s.annotations_path == os.path.join(s.log_dir, "annotations.feather")
    assert D.ScenarioValidator(str(tmp_path / "nowhere")).find_valid_scenarios() == []
    # the recorded sequence list, whatever the order of the logs
    assert len(dataset) == len(tiny["seq_log"])
    seen = set()
    for seq in dataset.sequences:
        j = _recorded_index(tiny, seq)
        seen.add(j)
        assert seq["sweep_ts_list"] == tiny["seq_sweep_ts"][j].tolist()
        assert seq["current_ts_ns"] == seq["sweep_ts_list"][-1]
    assert len(seen) == len(dataset)
    with pytest.raises(IndexError):
        dataset.load_sample(len(dataset))
    with pytest.raises(ValueError, match="No valid scenarios"):
        D.ArgoverseIntentNetDataset(str(tmp_path), num_sweeps=NUM_SWEEPS)
    with pytest.raises(ValueError, match="Could not create any valid sequences"):
        D.ArgoverseIntentNetDataset(tree, num_sweeps=8)
    # collate_fn
    assert D.collate_fn([None, None]) is None
    items = [{"lidar_bev": torch.full((2, 3, 4), float(k)), "map_bev": torch.zeros((1, 3, 4)),
              "gt": {"boxes_xywha": torch.zeros((k, 5)), "intentions": torch.zeros((k,), dtype=torch.long)}}
             for k in range(2)]
    b = D.collate_fn([items[0], None, items[1]])
    assert b["lidar_bev"].shape == (2, 2, 3, 4) and b["map_bev"].shape == (2, 1, 3, 4)
    assert [g["boxes_xywha"].shape[0] for g in b["gt_list"]] == [0, 1]


def test_host_half_follows_the_reference_skip_rules_and_ground_truth(tiny, dataset):
    """load_sample (no device): None exactly where the reference's __getitem__ is None; a sweep
    without a pose is skipped inside its sample; the ground truth is the recorded one."""
    for i, seq in enumerate(dataset.sequences):
        j = _recorded_index(tiny, seq)
        s = dataset.load_sample(i)
        assert (s is not None) == bool(tiny["seq_valid"][j])
        if s is None:
            continue
        _check_gt(s["gt"], tiny, j)
        tag = TAGS[tiny["logs"].tolist().index(seq["log_id"])]
        have_pose = np.isin(seq["sweep_ts_list"], tiny[f"{tag}_pose_ts"])
        assert [p is not None for p in s["points"]] == have_pose.tolist()
        assert [t is not None for t in s["transforms"]] == have_pose.tolist()
        assert np.allclose(s["transforms"][-1], np.eye(4), atol=1e-12)  # the current sweep
    assert not tiny["seq_valid"].all() and tiny["seq_valid"].any()


def test_missing_intent_file_gives_no_samples(tiny, tmp_path):
    import dataset as D
    root = str(tmp_path / "val")
    os.makedirs(root)
    write_tree(tiny, root)  # unlabelled
    ds = D.ArgoverseIntentNetDataset(root, num_sweeps=NUM_SWEEPS)
    assert all(ds.load_sample(i) is None for i in range(len(ds)))


def test_loader_sharding_covers_each_sequence_once(dataset):
    import dataset as D
    n = len(dataset)
    for shuffle in (False, True):
        parts = [D.FrameBatchLoader(dataset, 2, shuffle=shuffle, seed=5, rank=r, world=2).indices(0) for r in (0, 1)]
        assert sorted(parts[0] + parts[1]) == list(range(n)) and not set(parts[0]) & set(parts[1])
    state = random.getstate()
    a = D.FrameBatchLoader(dataset, 2, shuffle=True, seed=5).indices(0)
    assert a == D.FrameBatchLoader(dataset, 2, shuffle=True, seed=5).indices(0)
    assert random.getstate() == state  # the augmentation's random stream is left alone
    assert len(D.FrameBatchLoader(dataset, 3)) == -(-n // 3)
    with pytest.raises(ValueError):
        D.FrameBatchLoader(dataset, 2, rank=2, world=2)


# ------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_preprocess_main_writes_the_recorded_column(tiny, tmp_path):
    import preprocess_intent_labels as P
    root = tmp_path / "data"
    os.makedirs(root / "val")
    dirs = write_tree(tiny, str(root / "val"))
    assert P.main(str(root), ["train", "val"], False) == {"processed": 2, "skipped": 0, "failed": 0}
    for tag, d in zip(TAGS, dirs):
        src = pd.read_feather(os.path.join(d, "annotations.feather"))
        out = pd.read_feather(os.path.join(d, P.OUTPUT_ANNOTATION_FILENAME))
        assert list(out.columns) == list(ANN_COLUMNS) + ["heuristic_intent"]
        assert np.array_equal(out["heuristic_intent"].to_numpy(), tiny[f"{tag}_heuristic_intent"])
        pd.testing.assert_frame_equal(out[list(ANN_COLUMNS)], src)
    assert P.main(str(root), ["val"], False) == {"processed": 0, "skipped": 2, "failed": 0}
    victim = os.path.join(dirs[0], P.OUTPUT_ANNOTATION_FILENAME)
    bad = pd.read_feather(victim)
    bad["heuristic_intent"] = 3
    bad.to_feather(victim)
    assert P.main(str(root), ["val"], True) == {"processed": 2, "skipped": 0, "failed": 0}
    assert np.array_equal(pd.read_feather(victim)["heuristic_intent"].to_numpy(), tiny["a_heuristic_intent"])


@pytest.mark.gpu
def test_loader_batches_equal_the_reference_items(tiny, dataset):
    import dataset as D
    loader = D.FrameBatchLoader(dataset, 2, augment=False)
    kept = [i for i in loader.indices() if tiny["seq_valid"][_recorded_index(tiny, dataset.sequences[i])]]
    chunks = [[i for i in loader.indices()[k: k + 2] if i in kept] for k in range(0, len(dataset), 2)]
    chunks = [c for c in chunks if c]
    batches = list(loader)
    assert [b["lidar_bev"].shape[0] for b in batches] == [len(c) for c in chunks]  # the None sample is dropped
    for b, chunk in zip(batches, chunks):
        assert b["lidar_bev"].is_cuda and b["map_bev"].is_cuda
        assert b["lidar_bev"].shape[1:] == (290, 400, 720) and b["map_bev"].shape[1:] == (9, 400, 720)
        for k, i in enumerate(chunk):
            j = _recorded_index(tiny, dataset.sequences[i])
            assert np.array_equal(b["lidar_bev"][k].cpu().numpy(), _dense(tiny, f"item{j}_lidar"))
            assert np.array_equal(b["map_bev"][k].cpu().numpy(), _dense(tiny, f"item{j}_map"))
            _check_gt(b["gt_list"][k], tiny, j)


@pytest.mark.gpu
def test_getitem_and_in_process_labels(tiny, dataset, tmp_path):
    import dataset as D
    i = next(i for i, s in enumerate(dataset.sequences) if s["log_id"] == tiny["logs"][1])
    j = _recorded_index(tiny, dataset.sequences[i])
    item = dataset[i]
    assert np.array_equal(item["lidar_bev"].cpu().numpy(), _dense(tiny, f"item{j}_lidar"))
    assert np.array_equal(item["map_bev"].cpu().numpy(), _dense(tiny, f"item{j}_map"))
    _check_gt(item["gt"], tiny, j)
    # an unlabelled tree, labelled in this process: the kernel's labels and yaw feed the ground truth
    root = str(tmp_path / "val")
    os.makedirs(root)
    write_tree(tiny, root)
    ds = D.ArgoverseIntentNetDataset(root, num_sweeps=NUM_SWEEPS, label_missing=True)
    for i, seq in enumerate(ds.sequences):
        j = _recorded_index(tiny, seq)
        s = ds.load_sample(i)
        assert (s is not None) == bool(tiny["seq_valid"][j])
        if s is not None:
            _check_gt(s["gt"], tiny, j)


@pytest.mark.gpu
def test_ranks_of_a_world_of_two_cover_the_valid_samples_once(tiny, dataset):
    import dataset as D
    n_valid = int(tiny["seq_valid"].sum())
    sizes = [sum(b["lidar_bev"].shape[0] for b in D.FrameBatchLoader(dataset, 1, rank=r, world=2)) for r in (0, 1)]
    assert sum(sizes) == n_valid


@pytest.mark.gpu
def test_augmented_batch_equals_augment_bev_batch_under_the_same_seed(dataset):
    import torch
    import dataset as D
    import utils
    plain = next(iter(D.FrameBatchLoader(dataset, 2, augment=False)))
    random.seed(1234)
    aug = next(iter(D.FrameBatchLoader(dataset, 2, augment=True)))
    random.seed(1234)
    lo, mo, gts, params = utils.augment_bev_batch(plain["lidar_bev"], plain["map_bev"], plain["gt_list"])
    assert any(p["flip"] or p["angle"] is not None or p["scale"] is not None for p in params)
    assert torch.equal(aug["lidar_bev"], lo) and torch.equal(aug["map_bev"], mo)
    assert not torch.equal(aug["lidar_bev"], plain["lidar_bev"])
    for a, b in zip(aug["gt_list"], gts):
        assert torch.equal(a["boxes_xywha"], b["boxes_xywha"]) and torch.equal(a["intentions"], b["intentions"])


@pytest.mark.gpu
def test_train_vit_on_a_data_dir(tree):
    import train_vit
    assert train_vit.main(["--data-dir", tree, "--epochs", "1", "--batch", "1", "--no-save",
                           "--num-sweeps", str(NUM_SWEEPS)]) == 0
    with pytest.raises(SystemExit):
        train_vit.main(["--data-dir", tree, "--grid", "32x48", "--no-save"])


@pytest.mark.gpu
def test_eval_vit_on_a_data_dir(tree, tmp_path):
    import torch
    import eval_vit
    import train_vit
    from model_vit import IntentNetViT
    cfg = train_vit.backbone_cfg()
    ck = tmp_path / "vit_model.pth"
    torch.save({"epoch": 0, "model_state_dict": IntentNetViT(backbone_cfg=cfg).state_dict(),
                "optimizer_state_dict": {}, "backbone_cfg": cfg}, ck)
    assert eval_vit.main_eval_vit(["--data-dir", tree, "--checkpoint", str(ck), "--batch", "2",
                                   "--num-sweeps", str(NUM_SWEEPS)]) == 0
