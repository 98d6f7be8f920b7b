"""Heuristic intention labels — the reference's heuristic_labeling.py:10-124 on the GPU.

The reference labels one (track, timestamp) per call and filters and sorts the whole annotation
table inside every call, so labelling a log is quadratic in its rows. Here a whole table (one
log, or several concatenated) is labelled in one launch of ``ivit_intent_labels``
(csrc/labels.hip): the host sorts the rows by (track, timestamp) once, the kernel gives every
row its label and its yaw, and the result is scattered back to the table's row order.

Only the reference's map-free branch exists: what it computes when ``av2`` cannot be imported
(``AV2_MAP_AVAILABLE`` false / ``static_map`` None). A ``static_map`` is refused, not ignored.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np
import pandas as pd
import torch

from _lib import lib, ptr, stream
from constants import (HEADING_CHANGE_THRESH_LANE_KEEP, HEADING_CHANGE_THRESH_TURN, INTENTION_HORIZON_STEPS,
                       INTENTIONS_MAP, KEEP_LANE_MAX_LAT_DIST_FALLBACK, MIN_SPEED_MOVING, MIN_SPEED_STOPPED,
                       PARKED_MAX_DISP_M, VEHICLE_CATEGORIES)


@dataclass
class LabelParams:
    """The keyword defaults of heuristic_labeling.py:15-23 (values from constants.py)."""
    horizon_steps: int = INTENTION_HORIZON_STEPS
    min_future_points: int = 5
    stopped_speed_thresh: float = MIN_SPEED_STOPPED
    moving_speed_thresh: float = MIN_SPEED_MOVING
    turn_heading_thresh_rad: float = HEADING_CHANGE_THRESH_TURN
    keep_heading_thresh_rad: float = HEADING_CHANGE_THRESH_LANE_KEEP
    parked_max_disp_m: float = PARKED_MAX_DISP_M
    keep_lane_max_lat_dist_fallback: float = KEEP_LANE_MAX_LAT_DIST_FALLBACK


class _CParams(ctypes.Structure):  # ivit_label_params (include/ivit.h)
    _fields_ = [("horizon_steps", ctypes.c_int), ("min_future_points", ctypes.c_int),
                ("stopped_speed", ctypes.c_double), ("moving_speed", ctypes.c_double),
                ("turn_heading", ctypes.c_double), ("keep_heading", ctypes.c_double),
                ("parked_max_disp", ctypes.c_double), ("keep_lane_max_lat", ctypes.c_double)]


def _cparams(p: LabelParams | None) -> _CParams:
    p = LabelParams() if p is None else p
    return _CParams(int(p.horizon_steps), int(p.min_future_points), float(p.stopped_speed_thresh),
                    float(p.moving_speed_thresh), float(p.turn_heading_thresh_rad), float(p.keep_heading_thresh_rad),
                    float(p.parked_max_disp_m), float(p.keep_lane_max_lat_dist_fallback))


def intent_labels_sorted(ts, xy, quat, is_vehicle, track_off, params: LabelParams | None = None, device=None):
    """``ivit_intent_labels`` on rows already sorted by (track, timestamp_ns).

    ts [n] int64, xy [n, 2] f64, quat [n, 4] f64 (qx, qy, qz, qw), is_vehicle [n] bool,
    track_off [n_tracks + 1] int64 -> (intent [n] int32, yaw [n] f64) as numpy arrays."""
    ts = np.ascontiguousarray(ts, np.int64)
    n = ts.shape[0]
    xy = np.ascontiguousarray(xy, np.float64).reshape(n, 2)
    quat = np.ascontiguousarray(quat, np.float64).reshape(n, 4)
    veh = np.ascontiguousarray(is_vehicle).astype(np.uint8).reshape(n)
    off = np.ascontiguousarray(track_off, np.int64)
    n_tracks = off.shape[0] - 1
    if n_tracks < 0 or off[0] != 0 or off[-1] != n or (n and np.any(np.diff(off) <= 0)):
        raise ValueError("track_off must rise strictly from 0 to the row count")
    cp = _cparams(params)
    if n == 0:
        lib.ivit_intent_labels(None, None, None, None, None, 0, n_tracks, ctypes.byref(cp), None, None, None)
        return np.empty((0,), np.int32), np.empty((0,), np.float64)
    dev = torch.device(device if device is not None else "cuda")
    if dev.type != "cuda":
        raise RuntimeError("intention labelling runs on the GPU (no CPU fallback)")
    with torch.cuda.device(dev):
        d = [torch.from_numpy(a).to(dev) for a in (ts, xy, quat, veh, off)]
        intent = torch.empty((n,), dtype=torch.int32, device=dev)
        yaw = torch.empty((n,), dtype=torch.float64, device=dev)
        lib.ivit_intent_labels(ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(d[4]), n, n_tracks, ctypes.byref(cp),
                               ptr(intent), ptr(yaw), stream())
        return intent.cpu().numpy(), yaw.cpu().numpy()


def sort_rows(track_codes, ts):
    """-> (order, track_off): the (track, timestamp) order of the rows and the tracks' offsets in
    it. Raises ValueError on a duplicate (track, timestamp) pair, for which the reference's label
    depends on the sort's tie order."""
    track_codes = np.asarray(track_codes, np.int64)
    ts = np.asarray(ts, np.int64)
    order = np.lexsort((ts, track_codes))
    tr, t = track_codes[order], ts[order]
    if tr.shape[0] > 1:
        dup = (tr[1:] == tr[:-1]) & (t[1:] == t[:-1])
        if dup.any():
            k = int(np.flatnonzero(dup)[0])
            raise ValueError(f"duplicate (track, timestamp_ns) pair in the annotation table: rows {int(order[k])} and "
                             f"{int(order[k + 1])} (timestamp_ns {int(t[k])})")
    starts = np.flatnonzero(np.concatenate([[True], tr[1:] != tr[:-1]])) if tr.shape[0] else np.zeros((0,), np.int64)
    return order, np.concatenate([starts, [tr.shape[0]]]).astype(np.int64)


def label_columns(track_codes, ts, xy, quat, is_vehicle, params: LabelParams | None = None, device=None):
    """Label rows given in any order: sort on the host, one launch, scatter back.
    -> (intent [n] int64, yaw [n] f64) in the rows' own order."""
    order, off = sort_rows(track_codes, ts)  # before any device call
    ts, xy, quat = np.asarray(ts, np.int64), np.asarray(xy, np.float64), np.asarray(quat, np.float64)
    veh = np.asarray(is_vehicle, bool)
    si, sy = intent_labels_sorted(ts[order], xy[order], quat[order], veh[order], off, params, device)
    intent = np.empty(order.shape[0], np.int64)
    yaw = np.empty(order.shape[0], np.float64)
    intent[order], yaw[order] = si, sy
    return intent, yaw


def label_annotations(df: pd.DataFrame, params: LabelParams | None = None, device=None, return_yaw: bool = False,
                      log_codes=None, is_vehicle=None):
    """The ``heuristic_intent`` column of preprocess_intent_labels.py:54-57 for a whole annotation
    table (columns track_uuid, timestamp_ns, category, tx_m, ty_m, qx, qy, qz, qw) in one launch:
    int64 per row, -1 for non-vehicle categories. ``log_codes`` (one integer per row) keeps the
    tracks of concatenated logs apart; ``is_vehicle`` overrides the category test.

    One reference quirk is kept: heuristic_labeling.py:32-34 tests ``current_idx_loc.any()``, which
    is false for the index label 0, so a vehicle row whose DataFrame index label is 0 reads OTHER."""
    codes, _ = pd.factorize(df["track_uuid"], sort=False)
    codes = codes.astype(np.int64)
    if log_codes is not None:
        lc = np.asarray(log_codes, np.int64)
        codes = np.unique(np.stack([lc, codes], 1), axis=0, return_inverse=True)[1].reshape(-1).astype(np.int64)
    if is_vehicle is None:
        is_vehicle = df["category"].isin(VEHICLE_CATEGORIES).to_numpy()
    is_vehicle = np.asarray(is_vehicle, bool)
    intent, yaw = label_columns(codes, df["timestamp_ns"].to_numpy(), df[["tx_m", "ty_m"]].to_numpy(np.float64),
                                df[["qx", "qy", "qz", "qw"]].to_numpy(np.float64), is_vehicle, params, device)
    try:
        label0 = np.asarray(df.index == 0)
    except TypeError:
        label0 = np.zeros(len(df), bool)
    intent[label0 & is_vehicle] = INTENTIONS_MAP["OTHER"]
    return (intent, yaw) if return_yaw else intent


def get_vehicle_intention_heuristic_enhanced(
        track_id: str,
        current_ts_ns: int,
        all_log_gt_boxes_df: pd.DataFrame,
        static_map=None,
        horizon_steps: int = INTENTION_HORIZON_STEPS,
        min_future_points: int = 5,
        stopped_speed_thresh: float = MIN_SPEED_STOPPED,
        moving_speed_thresh: float = MIN_SPEED_MOVING,
        turn_heading_thresh_rad: float = HEADING_CHANGE_THRESH_TURN,
        keep_heading_thresh_rad: float = HEADING_CHANGE_THRESH_LANE_KEEP,
        map_search_radius: float = 5.0,
        parked_max_disp_m: float = PARKED_MAX_DISP_M,
        keep_lane_max_lat_dist_fallback: float = KEEP_LANE_MAX_LAT_DIST_FALLBACK) -> int:
    """heuristic_labeling.py:10-124 for one (track, timestamp): the reference's signature over the
    same kernel path (the track's rows only, every one of them treated as a vehicle, as the
    reference's function does not look at the category). To label a table, call
    label_annotations once instead of this once per row."""
    if static_map is not None:
        raise NotImplementedError("map context is not implemented: only the reference's map-free branch "
                                  "(static_map=None) exists in this build")
    df = all_log_gt_boxes_df
    track = df[df["track_uuid"] == track_id]
    hit = np.flatnonzero(track["timestamp_ns"].to_numpy() == current_ts_ns)
    if hit.size == 0:
        return INTENTIONS_MAP["OTHER"]
    p = LabelParams(horizon_steps, min_future_points, stopped_speed_thresh, moving_speed_thresh,
                    turn_heading_thresh_rad, keep_heading_thresh_rad, parked_max_disp_m,
                    keep_lane_max_lat_dist_fallback)
    intent = label_annotations(track, p, is_vehicle=np.ones(len(track), bool))
    return int(intent[hit[0]])
