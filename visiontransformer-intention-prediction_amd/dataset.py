"""Argoverse-2 sensor logs -> IntentNet batches: the reference's dataset.py:27-366 with the
rasters built on the GPU.

``ScenarioValidator``, ``collate_fn`` and ``ArgoverseIntentNetDataset`` keep the reference's
interface, sequence enumeration and skip rules (dataset.py:262-361). What differs:

* the LiDAR raster (with the sweeps' ego transforms fused, dataset.py:336-340) and the map raster
  come from this build's kernels, so ``lidar_bev`` / ``map_bev`` are device tensors;
* the ground truth is gathered on arrays (utils.prepare_gt_for_frame), not row by row;
* scenario directories are visited in name order (the reference takes os.scandir's order), so
  every rank of a data-parallel run enumerates the same sequence list;
* ``FrameBatchLoader`` builds whole batches: one lidar_bev_batch, one rasterize_map_batch and,
  when asked, one augment_bev_batch launch set per batch, while one background host thread
  reads the next batch's files.

Map context (``av2``) is not used: ``map_api`` is always None, as in the reference without av2.
"""
from __future__ import annotations

import json
import os
import random
import threading
import time
import traceback
from collections import namedtuple
from pathlib import Path

import numpy as np
import pandas as pd
import pyarrow
import torch
from scipy.spatial.transform import Rotation as R

from constants import GRID_HEIGHT_PX, GRID_WIDTH_PX, LIDAR_HEIGHT_CHANNELS, LIDAR_SWEEPS, MAP_CHANNELS
from utils import (augment_bev, augment_bev_batch, create_intentnet_lidar_bev, gt_columns, lidar_bev_batch,
                   load_ego_poses, prepare_gt_for_frame, rasterize_map_batch, rasterize_map_ego_centric)

INTENT_ANNOTATION_FILENAME = "annotations_with_intent.feather"


class ScenarioValidator:
    """dataset.py:27-134: finds the scenario directories that hold a non-empty sensors/lidar
    directory with *.feather sweeps, annotations.feather, city_SE3_egovehicle.feather (each at
    least ``min_feather_size_bytes``) and a map directory with a log_map_archive_*.json."""

    def __init__(self, base_path: str, skip_known_corrupted: bool = True, min_feather_size_bytes: int = 1024):
        self.base_path = Path(base_path)
        self.ScenarioPaths = namedtuple("ScenarioPaths", ["log_dir", "map_path", "annotations_path"])
        self.skip_known_corrupted = skip_known_corrupted
        self.min_feather_size_bytes = min_feather_size_bytes
        self.KNOWN_CORRUPTED_LOGS = {}

    def find_valid_scenarios(self) -> list:
        print(f"ScenarioValidator: Searching for scenarios in: {self.base_path}")
        if not self.base_path.is_dir():
            print(f"Error: Base path does not exist or is not a directory: {self.base_path}")
            return []
        t0 = time.time()
        try:
            entries = sorted((e for e in os.scandir(self.base_path) if e.is_dir()), key=lambda e: e.name)
        except OSError as e:
            print(f"Error: Cannot scan directory {self.base_path}: {e}")
            return []
        valid, reasons, corrupted = [], {}, 0
        for n, entry in enumerate(entries, 1):
            if n % 50 == 0:
                print(f"  Scanned {n} directories...")
            if self.skip_known_corrupted and entry.name in self.KNOWN_CORRUPTED_LOGS:
                corrupted += 1
                continue
            res = self._validate_scenario(Path(entry.path))
            if isinstance(res, self.ScenarioPaths):
                valid.append(res)
            else:
                reasons[res] = reasons.get(res, 0) + 1
        print(f"\nScenario Scan Summary (took {time.time() - t0:.2f} seconds):")
        print(f"  Total directories scanned: {len(entries)}")
        if self.skip_known_corrupted:
            print(f"  Skipped (known corrupted): {corrupted}")
        if reasons:
            print(f"  Skipped (invalid structure/files): {sum(reasons.values())}")
            print("  Skip Reasons:")
            for reason, count in reasons.items():
                print(f"    - {reason}: {count}")
        print(f"  Found {len(valid)} valid scenarios for processing.")
        return valid

    def _validate_scenario(self, scenario_dir: Path):
        """-> ScenarioPaths, or the reason (str) the directory is not a usable scenario."""
        lidar_dir = scenario_dir / "sensors" / "lidar"
        annotation_file = scenario_dir / "annotations.feather"
        map_dir = scenario_dir / "map"
        log_id = scenario_dir.name
        required = {"Lidar directory": lidar_dir, "Annotations file": annotation_file, "Map directory": map_dir,
                    "Ego pose file": scenario_dir / "city_SE3_egovehicle.feather"}
        small = self.min_feather_size_bytes
        for name, p in required.items():
            if not p.exists() or (p.is_dir() and not any(p.iterdir())) \
                    or (p.is_file() and small > 0 and p.stat().st_size < small):
                return f"Missing or invalid {name.lower()} ({p.name})"
        if not any(lidar_dir.glob("*.feather")):
            return "No *.feather files in lidar directory"
        map_files = sorted(map_dir.glob(f"log_map_archive_{log_id}*.json")) or sorted(map_dir.glob("log_map_archive_*.json"))
        if not map_files:
            return f"No 'log_map_archive_{log_id}*.json' or generic map file found in map directory"
        return self.ScenarioPaths(log_dir=str(scenario_dir), map_path=str(map_files[0]),
                                  annotations_path=str(annotation_file))


def collate_fn(batch: list) -> dict | None:
    """dataset.py:137-150: drop the None items, stack the rasters, keep the GT dicts as a list."""
    batch = [item for item in batch if item is not None]
    if not batch:
        return None
    return {"lidar_bev": torch.stack([item["lidar_bev"] for item in batch]),
            "map_bev": torch.stack([item["map_bev"] for item in batch]),
            "gt_list": [item["gt"] for item in batch]}


def _se3(quat_xyzw, t):
    m = np.eye(4)
    m[:3, :3] = R.from_quat(quat_xyzw).as_matrix()
    m[:3, 3] = t
    return m


class ArgoverseIntentNetDataset(torch.utils.data.Dataset):
    """dataset.py:153-366. ``__getitem__`` returns {"lidar_bev": (290, 400, 720), "map_bev":
    (9, 400, 720), "gt": {"boxes_xywha", "intentions"}} with the rasters on ``device``, or None
    where the reference returns None. ``load_sample`` is its host half (files, poses, ground
    truth), which FrameBatchLoader runs on its prefetch thread.

    ``label_missing=True`` labels a log whose annotations_with_intent.feather is absent in this
    process (heuristic_labeling.label_annotations on annotations.feather, nothing written); the
    reference's behaviour (such a log yields no samples) is the default."""

    def __init__(self, data_dir: str, num_sweeps: int = LIDAR_SWEEPS, is_train: bool = False, device=None,
                 label_missing: bool = False):
        self.data_dir = Path(data_dir)
        self.num_sweeps = num_sweeps
        self.is_train = is_train
        self.device = device
        self.label_missing = label_missing
        self.valid_scenario_paths = ScenarioValidator(str(self.data_dir)).find_valid_scenarios()
        if not self.valid_scenario_paths:
            raise ValueError(f"No valid scenarios found in {self.data_dir}. Please check the path and data integrity.")
        self.log_data_cache = {}
        self._cache_lock = threading.Lock()
        self.sequences = self._create_sequences()
        if not self.sequences:
            raise ValueError(f"Could not create any valid sequences from the provided scenarios in {self.data_dir}.")
        print(f"Dataset Initialized: {'Train' if is_train else 'Validation'}. Found {len(self.sequences)} sequences.")

    def _create_sequences(self) -> list:
        """dataset.py:174-211: every window of num_sweeps consecutive sweeps of every log."""
        sequences = []
        print("Creating sequences from valid scenarios...")
        for info in self.valid_scenario_paths:
            log_dir = Path(info.log_dir)
            lidar_dir = log_dir / "sensors" / "lidar"
            try:
                if not lidar_dir.is_dir():
                    print(f"  Warning (_create_sequences): LiDAR directory missing for {log_dir.name}. Skipping.")
                    continue
                timestamps = sorted(int(p.stem) for p in lidar_dir.glob("*.feather"))
                for i in range(len(timestamps) - self.num_sweeps + 1):
                    sweeps = timestamps[i: i + self.num_sweeps]
                    sequences.append({"log_id": log_dir.name, "log_dir": str(log_dir), "map_json_path": info.map_path,
                                      "annotations_path": info.annotations_path, "current_ts_ns": sweeps[-1],
                                      "sweep_ts_list": sweeps})
            except ValueError as e:
                print(f"  Warning (_create_sequences): Error converting timestamp filename in {log_dir.name}: {e}. "
                      "Skipping.")
        print(f"Created {len(sequences)} sequences in total.")
        return sequences

    def _load_log(self, log_id, log_dir, annotations_path, map_json_path):
        intent_path = Path(log_dir) / INTENT_ANNOTATION_FILENAME
        yaw = None
        if intent_path.is_file():
            gt_df = pd.read_feather(intent_path)
        elif self.label_missing:
            from heuristic_labeling import label_annotations
            gt_df = pd.read_feather(annotations_path)
            gt_df["heuristic_intent"], yaw = label_annotations(gt_df, device=self.device, return_yaw=True)
        else:
            print(f"FATAL ERROR: Pre-computed intent file missing for log {log_id} at {intent_path}. "
                  "Please run the intention pre-computation script.")
            return None
        poses = load_ego_poses(log_dir)
        pose_cols = {k: poses[k].to_numpy() for k in ("timestamp_ns", "tx_m", "ty_m", "tz_m", "qx", "qy", "qz", "qw")}
        first = {}
        for row, ts in enumerate(pose_cols["timestamp_ns"].tolist()):  # the first row of a timestamp (.iloc[0])
            first.setdefault(ts, row)
        try:
            with open(map_json_path, "r") as f:
                map_data = json.load(f)
        except Exception as e:  # noqa: BLE001  (utils.py:111-116: an unreadable map is an empty map)
            print(f"Error loading map JSON {map_json_path}: {e}. Returning empty map.")
            map_data = None
        return {"ego_poses": poses, "pose_cols": pose_cols, "pose_row": first, "gt_df": gt_df,
                "gt": gt_columns(gt_df, yaw), "map_api": None, "map_data": map_data}

    def _get_log_data(self, log_id: str, log_dir: str, annotations_path: str, map_json_path: str | None = None):
        """dataset.py:213-257: the log's poses and labelled annotations, read once."""
        with self._cache_lock:
            if log_id not in self.log_data_cache:
                try:
                    self.log_data_cache[log_id] = self._load_log(log_id, log_dir, annotations_path, map_json_path)
                except Exception as e:  # noqa: BLE001
                    print(f"Error loading data cache for log {log_id}: {e}")
                    traceback.print_exc()
                    self.log_data_cache[log_id] = None
            return self.log_data_cache[log_id]

    def __len__(self) -> int:
        return len(self.sequences)

    @staticmethod
    def _pose(log, ts):
        row = log["pose_row"].get(ts)
        if row is None:
            return None
        return {k: v[row] for k, v in log["pose_cols"].items()}

    def load_sample(self, idx: int):
        """The host half of dataset.py:262-350 -> None (the reference's None) or {"points",
        "intensity", "transforms" (per-sweep rel_tf, None entries for skipped sweeps), "map"
        (parsed JSON or None), "pose", "gt"}."""
        if not (0 <= idx < len(self.sequences)):
            raise IndexError(f"Index {idx} out of bounds for dataset with size {len(self.sequences)}")
        seq = self.sequences[idx]
        log_id, current_ts_ns = seq["log_id"], seq["current_ts_ns"]
        try:
            log = self._get_log_data(log_id, seq["log_dir"], seq["annotations_path"], seq["map_json_path"])
            if log is None:
                print(f"Warning: No log data found for log_id {log_id} in __getitem__ for index {idx}. Skipping item.")
                return None
            pose = self._pose(log, current_ts_ns)
            if pose is None:
                return None
            try:
                world_SE3_ego = _se3([pose['qx'], pose['qy'], pose['qz'], pose['qw']],
                                     [pose['tx_m'], pose['ty_m'], pose['tz_m']])
            except ValueError:
                print(f"Warning: Invalid quaternion for ego pose at ts {current_ts_ns} in log {log_id}. Skipping item.")
                return None
            ego_SE3_world = np.linalg.inv(world_SE3_ego)
            points, intensity, transforms = [], [], []
            lidar_dir = Path(seq["log_dir"]) / "sensors" / "lidar"
            for ts_sweep in seq["sweep_ts_list"]:
                points.append(None)
                intensity.append(None)
                transforms.append(None)
                sweep_path = lidar_dir / f"{ts_sweep}.feather"
                if not sweep_path.is_file():
                    continue
                try:
                    sweep_df = pd.read_feather(sweep_path, columns=['x', 'y', 'z', 'intensity'])
                except pyarrow.ArrowInvalid:
                    print(f"Warning: Corrupt LiDAR sweep file: {sweep_path}. Skipping sweep.")
                    continue
                if sweep_df.empty:
                    continue
                sp = self._pose(log, ts_sweep)
                if sp is None:
                    continue
                try:
                    sweep_tf = _se3(np.array([sp['qx'], sp['qy'], sp['qz'], sp['qw']]),
                                    [sp['tx_m'], sp['ty_m'], sp['tz_m']])
                except ValueError:
                    continue
                points[-1] = np.ascontiguousarray(sweep_df[['x', 'y', 'z']].values)
                intensity[-1] = sweep_df['intensity'].values.astype(np.float32)
                transforms[-1] = ego_SE3_world @ sweep_tf  # dataset.py:339; applied in the voxelisation kernel
            if all(p is None for p in points):
                return None
            return {"points": points, "intensity": intensity, "transforms": transforms, "map": log["map_data"],
                    "pose": pose, "gt": prepare_gt_for_frame(current_ts_ns, log["gt"], None)}
        except Exception:  # noqa: BLE001  (dataset.py:363-367)
            print(f"!!! UNHANDLED ERROR in __getitem__ for index {idx}, log_id {log_id}, timestamp {current_ts_ns} !!!")
            print(f"Sequence Info: {seq}")
            traceback.print_exc()
            return None

    def __getitem__(self, idx: int):
        s = self.load_sample(idx)
        if s is None:
            return None
        lidar = create_intentnet_lidar_bev(s["points"], s["intensity"], transforms=s["transforms"], device=self.device)
        mp = _map_items([s], self.device)[0]
        gt = s["gt"]
        if self.is_train:
            lidar, mp, gt = augment_bev(lidar, mp, gt, device=self.device)
        return {"lidar_bev": lidar, "map_bev": mp,
                "gt": {'boxes_xywha': gt['boxes_xywha'].float(), 'intentions': gt['intentions'].long()}}


def _map_items(samples, device, out=None):
    """The samples' map rasters; a log without a readable map JSON gives empty planes (utils.py:111-116)."""
    items = [(s["map"] if s["map"] is not None else {}, s["pose"]) for s in samples]
    if out is None and len(items) == 1:
        return rasterize_map_ego_centric(items[0][0], items[0][1], device=device)[None]
    return rasterize_map_batch(items, out=out, device=device)


class FrameBatchLoader:
    """Batches of a dataset in collate_fn's format ({"lidar_bev": (B, 290, H, W), "map_bev":
    (B, 9, H, W), "gt_list"}), rasters on the device, each batch built by one lidar_bev_batch, one
    rasterize_map_batch and, with ``augment``, one augment_bev_batch call.

    The sequence list (shuffled by ``random.Random(seed + epoch)`` when asked, so the module-level
    ``random`` state that the augmentation draws from is left alone) is dealt to the ranks in
    strides: rank r takes entries r, r + world, ...; every sequence goes to exactly one rank.
    Samples the dataset gives up on (its ``__getitem__`` would be None) are dropped from their
    batch, as collate_fn drops them; a batch left empty is not yielded. One background host
    thread reads the next batch's files while this one is built (prefetch depth 1)."""

    def __init__(self, dataset, batch: int, shuffle: bool = False, seed: int = 0, rank: int = 0, world: int = 1,
                 augment: bool = False, device=None):
        if batch < 1 or world < 1 or not (0 <= rank < world):
            raise ValueError(f"bad loader geometry: batch {batch}, rank {rank} of {world}")
        self.dataset, self.batch, self.shuffle, self.seed = dataset, batch, shuffle, seed
        self.rank, self.world, self.augment = rank, world, augment
        self.device = device if device is not None else getattr(dataset, "device", None)
        self.epoch = 0

    def indices(self, epoch: int | None = None) -> list:
        """This rank's sequence indices for an epoch, in loading order."""
        order = list(range(len(self.dataset)))
        if self.shuffle:
            random.Random(self.seed + (self.epoch if epoch is None else epoch)).shuffle(order)
        return order[self.rank:: self.world]

    def __len__(self) -> int:
        return -(-len(self.indices()) // self.batch)

    def _start(self, idxs):
        box = {}

        def work():
            try:
                box["samples"] = [self.dataset.load_sample(i) for i in idxs]
            except BaseException as e:  # noqa: BLE001  (re-raised on the consumer's side)
                box["error"] = e
        t = threading.Thread(target=work, name="ivit-frame-prefetch", daemon=True)
        t.start()
        return t, box

    def build(self, samples) -> dict | None:
        """Device batch from load_sample results (None entries dropped)."""
        samples = [s for s in samples if s is not None]
        if not samples:
            return None
        dev = torch.device(self.device if self.device is not None else "cuda")
        B = len(samples)
        lidar = torch.empty((B, LIDAR_HEIGHT_CHANNELS * LIDAR_SWEEPS, GRID_HEIGHT_PX, GRID_WIDTH_PX),
                            dtype=torch.float32, device=dev)
        mp = torch.empty((B, MAP_CHANNELS, GRID_HEIGHT_PX, GRID_WIDTH_PX), dtype=torch.float32, device=dev)
        lidar_bev_batch([(s["points"], s["intensity"], s["transforms"]) for s in samples], out=lidar)
        _map_items(samples, dev, out=mp)
        gts = [{'boxes_xywha': s["gt"]['boxes_xywha'].float(), 'intentions': s["gt"]['intentions'].long()}
               for s in samples]
        if self.augment:
            lidar, mp, gts, _ = augment_bev_batch(lidar, mp, gts)
        return {"lidar_bev": lidar, "map_bev": mp, "gt_list": gts}

    def __iter__(self):
        idx = self.indices()
        self.epoch += 1
        chunks = [idx[i: i + self.batch] for i in range(0, len(idx), self.batch)]
        pending = self._start(chunks[0]) if chunks else None
        for k in range(len(chunks)):
            thread, box = pending
            thread.join()
            pending = self._start(chunks[k + 1]) if k + 1 < len(chunks) else None
            if "error" in box:
                if pending is not None:
                    pending[0].join()
                raise box["error"]
            b = self.build(box["samples"])
            if b is not None:
                yield b
