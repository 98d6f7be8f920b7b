"""Generator of tests/golden/intent_labels.npz and tests/golden/av2_tiny.npz.

Both fixtures are outputs of the REFERENCE's own modules (heuristic_labeling,
preprocess_intent_labels, dataset), imported through oracle.refshim; nothing of this build runs
here. Needs the reference checkout (--reference) and pandas / pyarrow / scipy; the tests need
only the two .npz files. ``write_tree`` (no reference needed) is also what the tests use to put
av2_tiny.npz's two logs back on disk.

  python tools/make_golden_labels.py [--reference DIR] [labels] [tiny]

intent_labels.npz  ~1500 annotation rows (shuffled; track lengths 1, 5, 6, 30, 31, 35, > 64 and
    > 256; timestamp jitter and gaps; non-vehicle tracks; zero, negated and unnormalised
    quaternions; headings across +-pi; a vehicle at index label 0) and the reference's label of
    every row. The generator asserts that all eight classes and -1 occur and that no compared
    quantity lies within 1e-6 of its threshold, so a test may demand equality on every row.
av2_tiny.npz  a two-log Argoverse-2-style tree (12 sweeps, poses, annotations, a small map JSON
    string), the reference's heuristic_intent column for both logs, its sequence list for
    num_sweeps = 5, and its __getitem__ output for every sequence (rasters sparse).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")
ANN_COLUMNS = ("timestamp_ns", "track_uuid", "category", "length_m", "width_m", "height_m", "qw", "qx", "qy", "qz",
               "tx_m", "ty_m", "tz_m", "num_interior_pts")
POSE_COLUMNS = ("timestamp_ns", "qw", "qx", "qy", "qz", "tx_m", "ty_m", "tz_m")
TINY_NUM_SWEEPS = 5
MARGIN = 1e-6


# ------------------------------------------------------------------------------- synthetic tracks
def _yaw_quat(yaw, roll=0.0, pitch=0.0):
    from scipy.spatial.transform import Rotation
    e = np.stack([np.broadcast_to(roll, np.shape(yaw)), np.broadcast_to(pitch, np.shape(yaw)), yaw], 1)
    return Rotation.from_euler("xyz", e).as_quat()  # x y z w


def _track(rng, n, kind, t0=315_000_000_000_000_000, jitter=2_000_000, gap_prob=0.0, yaw0=None, tilt=False):
    """n rows of one object at ~10 Hz: (ts int64, xy, quat xyzw). kind picks the motion."""
    steps = np.ones(n, np.int64)
    steps[rng.random(n) < gap_prob] += rng.integers(1, 4)  # dropped frames
    ts = t0 + np.cumsum(steps) * 100_000_000 + rng.integers(-jitter, jitter + 1, n)
    t = (ts - ts[0]) * 1e-9
    yaw0 = rng.uniform(-3.0, 3.0) if yaw0 is None else yaw0
    speed = {"parked": 0.0, "creep": 0.3, "slow": 0.75, "keep": 8.0, "left": 6.0, "right": 6.0, "lcl": 8.0,
             "lcr": 8.0, "slide": 5.0, "accel": None}[kind]
    rate = {"left": 0.2, "right": -0.2, "lcl": 0.06, "lcr": -0.06}.get(kind, 0.0)
    yaw = yaw0 + rate * t
    if kind == "accel":  # 0 -> 4 m/s: the average speed crosses both speed thresholds
        s = 0.5 * 0.4 * t * t
    else:
        s = speed * t
    if rate != 0.0:  # arc
        x = speed / rate * (np.sin(yaw) - np.sin(yaw0))
        y = -speed / rate * (np.cos(yaw) - np.cos(yaw0))
    else:
        mv = yaw0 + (np.pi / 2 if kind == "slide" else 0.0)  # "slide": moving across its heading
        x, y = s * np.cos(mv), s * np.sin(mv)
    xy = np.stack([x, y], 1) + rng.uniform(-50, 50, 2) + rng.normal(0, 1e-3, (n, 2))
    roll, pitch = (rng.normal(0, 0.02, n), rng.normal(0, 0.02, n)) if tilt else (0.0, 0.0)
    return ts.astype(np.int64), xy, _yaw_quat(yaw, roll, pitch)


def _table(tracks):
    """[(uuid, category, ts, xy, quat)] -> DataFrame with the Argoverse-2 annotation columns."""
    import pandas as pd
    cols = {k: [] for k in ANN_COLUMNS}
    for k, (uuid, cat, ts, xy, q) in enumerate(tracks):
        n = len(ts)
        cols["timestamp_ns"].append(ts)
        cols["track_uuid"].append(np.full(n, uuid, dtype=object))
        cols["category"].append(np.full(n, cat, dtype=object))
        cols["length_m"].append(np.full(n, 4.0 + 0.1 * k))
        cols["width_m"].append(np.full(n, 1.8 + 0.01 * k))
        cols["height_m"].append(np.full(n, 1.5))
        for j, c in enumerate(("qx", "qy", "qz", "qw")):
            cols[c].append(q[:, j])
        cols["tx_m"].append(xy[:, 0])
        cols["ty_m"].append(xy[:, 1])
        cols["tz_m"].append(np.zeros(n))
        cols["num_interior_pts"].append(np.full(n, 10 + k, np.int64))
    return pd.DataFrame({k: np.concatenate(v) for k, v in cols.items()})


def make_label_table(seed):
    rng = np.random.default_rng(seed)
    spec = [("keep", 1), ("keep", 5), ("keep", 6), ("left", 30), ("right", 31), ("lcl", 35), ("keep", 70),
            ("left", 100), ("accel", 300), ("lcr", 280), ("parked", 45), ("creep", 45), ("slow", 40), ("right", 48),
            ("lcl", 50), ("lcr", 44), ("slide", 40), ("accel", 60), ("keep", 42), ("left", 46), ("parked", 38),
            ("creep", 41)]
    cats = ["REGULAR_VEHICLE", "BUS", "TRUCK", "BICYCLE", "LARGE_VEHICLE", "MOTORCYCLIST"]
    tracks = []
    for k, (kind, n) in enumerate(spec):
        yaw0 = {7: 2.9, 13: -2.95}.get(k)  # a left turn across +pi, a right turn across -pi
        ts, xy, q = _track(rng, n, kind, gap_prob=0.08 if k % 3 == 0 else 0.0, yaw0=yaw0, tilt=k % 2 == 1)
        if k % 4 == 2:  # -q is the same rotation
            q[::3] *= -1.0
        if k % 5 == 3:  # unnormalised
            q *= rng.uniform(0.3, 3.0, (len(q), 1))
        tracks.append((f"track-{k:02d}-{rng.integers(1 << 30):08x}", cats[k % len(cats)], ts, xy, q))
    tracks[6][4][3] = 0.0    # zero quaternion at a current row (also the end row of row 3 - 30 < 0: none)
    tracks[18][4][35] = 0.0  # zero quaternion that is the end row of row 5 and a current row itself
    for k, (kind, n) in enumerate([("keep", 40), ("parked", 35)]):  # not vehicles: -1
        ts, xy, q = _track(rng, n, kind)
        tracks.append((f"ped-{k}", ["PEDESTRIAN", "BOLLARD"][k], ts, xy, q))
    df = _table(tracks)
    perm = rng.permutation(len(df))
    # index label 0 goes to a vehicle row that the rules would label KEEP_LANE (row 2 of track 6)
    first = int(np.flatnonzero((df["track_uuid"] == tracks[6][0]).to_numpy())[2])
    perm = np.concatenate([[first], perm[perm != first]])
    return df.iloc[perm].reset_index(drop=True)


def rule_quantities(df, horizon, min_future):
    """Independent NumPy restatement of the rules on rows sorted by (track, timestamp): per row
    (in table order) the quantities the reference compares with thresholds, NaN where a rule
    does not reach the comparison."""
    from scipy.spatial.transform import Rotation
    n = len(df)
    tr = df["track_uuid"].to_numpy()
    ts = df["timestamp_ns"].to_numpy()
    xy = df[["tx_m", "ty_m"]].to_numpy()
    q = df[["qx", "qy", "qz", "qw"]].to_numpy()
    codes = np.unique(tr, return_inverse=True)[1]
    order = np.lexsort((ts, codes))
    out = {k: np.full(n, np.nan) for k in ("speed", "dist", "dh", "lat", "yaw")}
    nz = np.linalg.norm(q, axis=1) > 0
    out["yaw"][nz] = Rotation.from_quat(q[nz]).as_euler("xyz")[:, 2]
    c = codes[order]
    ends = np.searchsorted(c, c, side="right")  # end of each sorted row's track
    for pos, i in enumerate(order):
        used = min(horizon, ends[pos] - 1 - pos)
        if used < min_future:
            continue
        e = order[pos + used]
        d = xy[e] - xy[i]
        out["dist"][i] = np.linalg.norm(d)
        out["speed"][i] = out["dist"][i] / ((ts[e] - ts[i]) * 1e-9 + 1e-9)
        if not (nz[i] and nz[e]):
            continue
        dd = out["yaw"][e] - out["yaw"][i]
        out["dh"][i] = np.arctan2(np.sin(dd), np.cos(dd))
        h = np.array([np.cos(out["yaw"][i]), np.sin(out["yaw"][i])])
        out["lat"][i] = np.linalg.norm(d - np.dot(d, h) * h)
    return out


def restated_labels(df, Q, C):
    """Labels from rule_quantities (vehicle rows; -1 elsewhere), index label 0 forced to OTHER."""
    M = C.INTENTIONS_MAP
    veh = df["category"].isin(C.VEHICLE_CATEGORIES).to_numpy()
    out = np.full(len(df), M["OTHER"], np.int64)
    sp, di, dh, lat = Q["speed"], Q["dist"], Q["dh"], Q["lat"]
    ok = ~np.isnan(dh)
    stop = ok & (sp < C.MIN_SPEED_STOPPED)
    out[stop & (di < C.PARKED_MAX_DISP_M)] = M["PARKED"]
    out[stop & ~(di < C.PARKED_MAX_DISP_M)] = M["STOPPING_STOPPED"]
    mv = ok & (sp >= C.MIN_SPEED_MOVING)
    T, K = C.HEADING_CHANGE_THRESH_TURN, C.HEADING_CHANGE_THRESH_LANE_KEEP
    out[mv & (dh > T)] = M["TURN_LEFT"]
    out[mv & (dh < -T)] = M["TURN_RIGHT"]
    lc = mv & (np.abs(dh) > K) & (np.abs(dh) < T)
    out[lc & (dh > 0)] = M["LEFT_CHANGE_LANE"]
    out[lc & (dh < 0)] = M["RIGHT_CHANGE_LANE"]
    out[mv & (np.abs(dh) <= K) & (lat < C.KEEP_LANE_MAX_LAT_DIST_FALLBACK)] = M["KEEP_LANE"]
    out[df.index.to_numpy() == 0] = M["OTHER"]
    out[~veh] = -1
    return out


def check_margins(Q, C):
    """Smallest distance of any compared quantity to its threshold; asserts it is > MARGIN."""
    gaps = []
    for v, thr in ((Q["speed"], (C.MIN_SPEED_STOPPED, C.MIN_SPEED_MOVING)), (Q["dist"], (C.PARKED_MAX_DISP_M,)),
                   (np.abs(Q["dh"]), (C.HEADING_CHANGE_THRESH_TURN, C.HEADING_CHANGE_THRESH_LANE_KEEP, 0.0)),
                   (Q["lat"], (C.KEEP_LANE_MAX_LAT_DIST_FALLBACK,)), (np.abs(Q["yaw"]), (np.pi,))):
        v = v[~np.isnan(v)]
        for t in thr:
            if t == 0.0:  # the sign of dh matters only for lane changes
                v = v[v > C.HEADING_CHANGE_THRESH_LANE_KEEP]
            gaps.append(float(np.abs(v - t).min()))
    assert min(gaps) > MARGIN, f"a compared quantity lies within {MARGIN} of its threshold: {gaps}"
    return min(gaps)


def reference_labels(df, ref):
    """The loop of preprocess_intent_labels.py:41-57 with the reference's own function."""
    C, H = ref["constants"], ref["heuristic_labeling"]

    def one(row):
        if row["category"] in C.VEHICLE_CATEGORIES:
            return H.get_vehicle_intention_heuristic_enhanced(track_id=row["track_uuid"],
                                                              current_ts_ns=row["timestamp_ns"],
                                                              all_log_gt_boxes_df=df, static_map=None)
        return -1
    return df.apply(one, axis=1).to_numpy().astype(np.int64)


def gen_labels(ref, seed=7):
    C = ref["constants"]
    assert not C.AV2_MAP_AVAILABLE, "the fixture pins the reference's map-free branch"
    df = make_label_table(seed)
    t0 = time.perf_counter()
    labels = reference_labels(df, ref)
    dt = time.perf_counter() - t0
    Q = rule_quantities(df, C.INTENTION_HORIZON_STEPS, 5)
    gap = check_margins(Q, C)
    mine = restated_labels(df, Q, C)
    assert np.array_equal(mine, labels), f"restated rules differ from the reference on {(mine != labels).sum()} rows"
    assert set(np.unique(labels)) == set(range(-1, 8)), np.unique(labels, return_counts=True)
    assert labels[0] == C.INTENTIONS_MAP["OTHER"] and df["category"][0] in C.VEHICLE_CATEGORIES
    lens = df.groupby("track_uuid").size().to_numpy()
    assert {1, 5, 6, 30, 31, 35} <= set(lens) and (lens > 64).sum() >= 2 and (lens > 256).sum() >= 2
    np.savez_compressed(os.path.join(OUT, "intent_labels.npz"),
                        **{k: _col(df[k]) for k in ANN_COLUMNS}, heuristic_intent=labels, yaw_scipy=Q["yaw"],
                        min_threshold_gap=np.float64(gap), reference_seconds=np.float64(dt))
    print(f"intent_labels.npz: {len(df)} rows, {len(lens)} tracks, classes "
          f"{dict(zip(*[a.tolist() for a in np.unique(labels, return_counts=True)]))}, smallest threshold gap "
          f"{gap:.3g}, reference {dt:.2f} s ({1e3 * dt / len(df):.2f} ms/row)")


def _col(s):
    a = s.to_numpy()
    return a.astype(str) if a.dtype == object else a


# ------------------------------------------------------------------------------------ tiny tree
def make_tiny_arrays(seed=11):
    """The arrays of a two-log tree: log a (7 sweeps, the last one without a pose) and log b
    (5 sweeps, the second one without a pose)."""
    rng = np.random.default_rng(seed)
    A = {"logs": np.array(["log-a-0001", "log-b-0002"])}
    lanes, cross = {}, {}
    for k in range(3):  # three straight lanes side by side along +x, one an intersection, one a bus lane
        y0, y1 = 3.5 * k - 5.0, 3.5 * k - 1.5
        xs = np.linspace(-12.0, 40.0, 6)
        lanes[str(100 + k)] = {
            "id": 100 + k, "is_intersection": k == 1, "lane_type": "BUS" if k == 2 else "VEHICLE",
            "left_lane_boundary": [{"x": float(x), "y": y1 + 0.05 * float(x), "z": 0.0} for x in xs],
            "left_lane_mark_type": ["DASHED_WHITE", "SOLID_YELLOW", "NONE"][k],
            "right_lane_boundary": [{"x": float(x), "y": y0 + 0.05 * float(x), "z": 0.0} for x in xs],
            "right_lane_mark_type": ["SOLID_WHITE", "DASHED_WHITE", "SOLID_WHITE"][k]}
    cross["7"] = {"id": 7, "polygon": [{"x": 20.0, "y": -5.0, "z": 0.0}, {"x": 23.0, "y": -5.0, "z": 0.0},
                                      {"x": 23.5, "y": 6.0, "z": 0.0}, {"x": 20.5, "y": 6.0, "z": 0.0}]}
    A["map_json"] = np.array(json.dumps({"lane_segments": lanes, "pedestrian_crossings": cross, "drivable_areas": {}}))
    for li, (tag, n_sweeps, no_pose) in enumerate((("a", 7, 6), ("b", 5, 1))):
        t0 = 315_000_000_000_000_000 + li * 10_000_000_000
        sweep_ts = t0 + np.arange(n_sweeps) * 100_000_000 + rng.integers(-1_000_000, 1_000_000, n_sweeps)
        A[f"{tag}_sweep_ts"] = sweep_ts.astype(np.int64)
        counts = rng.integers(200, 400, n_sweeps)
        A[f"{tag}_sweep_counts"] = counts.astype(np.int64)
        # the ego drives along +x with a slow left bend; the sweeps hold points in each sweep's ego frame
        tt = np.arange(n_sweeps) * 0.1
        yaw = 0.05 * li + 0.03 * tt
        pose_q = _yaw_quat(yaw, rng.normal(0, 0.003, n_sweeps), rng.normal(0, 0.003, n_sweeps))
        pose_t = np.stack([5.0 * tt + li, 0.1 * tt - li, np.full(n_sweeps, 0.3)], 1)
        keep = np.arange(n_sweeps) != no_pose
        A[f"{tag}_pose"] = np.concatenate([pose_q[keep][:, [3, 0, 1, 2]], pose_t[keep]], 1)  # qw qx qy qz tx ty tz
        A[f"{tag}_pose_ts"] = sweep_ts[keep].astype(np.int64)
        pts = np.concatenate([rng.uniform([-25, -80, -3], [70, 80, 5], (c, 3)) for c in counts]).astype(np.float32)
        A[f"{tag}_points"] = pts
        A[f"{tag}_intensity"] = rng.integers(0, 256, len(pts)).astype(np.uint8)
        # annotations: the sweeps' timestamps and 32 more frames, so that the sweeps' rows have a future
        ann_ts = np.concatenate([sweep_ts, sweep_ts[-1] + (1 + np.arange(32)) * 100_000_000])
        tracks = []
        for k, (kind, cat) in enumerate((("keep", "REGULAR_VEHICLE"), ("left", "BUS"), ("parked", "TRUCK"),
                                         ("lcr", "BICYCLE"), ("creep", "LARGE_VEHICLE"), ("keep", "PEDESTRIAN"))):
            ts, xy, q = _track(rng, len(ann_ts), kind, tilt=k % 2 == 0)
            xy = xy - xy[0] + rng.uniform([-10, -30], [50, 30])
            tracks.append((f"{tag}-obj-{k}", cat, ann_ts.copy(), xy, q))
        tracks[2][4][n_sweeps - 2] = 0.0  # a zero quaternion at a current frame: no GT box
        df = _table(tracks)
        df.loc[df["track_uuid"] == f"{tag}-obj-1", "width_m"] *= -1.0  # |w|
        df = df.iloc[rng.permutation(len(df))].reset_index(drop=True)
        for c in ANN_COLUMNS:
            A[f"{tag}_ann_{c}"] = _col(df[c])
    return A


def write_tree(A, root):
    """Write the two logs of av2_tiny.npz (``A``: its arrays) as an Argoverse-2 sensor split under
    ``root``: <log>/sensors/lidar/<ts>.feather, annotations.feather, city_SE3_egovehicle.feather,
    map/log_map_archive_<log>.json. -> the log directories."""
    import pandas as pd
    dirs = []
    for tag, log in zip(("a", "b"), A["logs"].tolist()):
        d = os.path.join(str(root), log)
        os.makedirs(os.path.join(d, "sensors", "lidar"))
        os.makedirs(os.path.join(d, "map"))
        with open(os.path.join(d, "map", f"log_map_archive_{log}____city_0.json"), "w") as f:
            f.write(str(A["map_json"]))
        pose = pd.DataFrame({"timestamp_ns": A[f"{tag}_pose_ts"]})
        for j, c in enumerate(POSE_COLUMNS[1:]):
            pose[c] = A[f"{tag}_pose"][:, j]
        pose.to_feather(os.path.join(d, "city_SE3_egovehicle.feather"), compression="uncompressed")
        ann = pd.DataFrame({c: A[f"{tag}_ann_{c}"] for c in ANN_COLUMNS})
        ann.to_feather(os.path.join(d, "annotations.feather"), compression="uncompressed")
        off = np.concatenate([[0], np.cumsum(A[f"{tag}_sweep_counts"])])
        for s, ts in enumerate(A[f"{tag}_sweep_ts"].tolist()):
            p = A[f"{tag}_points"][off[s]:off[s + 1]]
            sw = pd.DataFrame({"x": p[:, 0], "y": p[:, 1], "z": p[:, 2],
                               "intensity": A[f"{tag}_intensity"][off[s]:off[s + 1]],
                               "laser_number": np.zeros(len(p), np.uint8),
                               "offset_ns": np.zeros(len(p), np.int32)})
            sw.to_feather(os.path.join(d, "sensors", "lidar", f"{ts}.feather"), compression="uncompressed")
        dirs.append(d)
    return dirs


def _sparse(prefix, arr, out, val_dtype):
    flat = np.asarray(arr).reshape(-1)
    idx = np.flatnonzero(flat)
    out[f"{prefix}_idx"], out[f"{prefix}_val"] = idx.astype(np.int64), flat[idx].astype(val_dtype)
    out[f"{prefix}_shape"] = np.array(arr.shape, np.int64)


def gen_tiny(ref, seed=11):
    import tempfile
    import pandas as pd
    A = make_tiny_arrays(seed)
    with tempfile.TemporaryDirectory() as tmp:
        split = os.path.join(tmp, "val")
        os.makedirs(split)
        write_tree(A, split)
        ref["preprocess_intent_labels"].main(tmp, ["val"], False)
        for tag, log in zip(("a", "b"), A["logs"].tolist()):
            got = pd.read_feather(os.path.join(split, log, "annotations_with_intent.feather"))
            assert list(got.columns) == list(ANN_COLUMNS) + ["heuristic_intent"]
            A[f"{tag}_heuristic_intent"] = got["heuristic_intent"].to_numpy().astype(np.int64)
        ds = ref["dataset"].ArgoverseIntentNetDataset(split, num_sweeps=TINY_NUM_SWEEPS, is_train=False)
        A["num_sweeps"] = np.int64(TINY_NUM_SWEEPS)
        A["seq_log"] = np.array([s["log_id"] for s in ds.sequences])
        A["seq_current_ts"] = np.array([s["current_ts_ns"] for s in ds.sequences], np.int64)
        A["seq_sweep_ts"] = np.array([s["sweep_ts_list"] for s in ds.sequences], np.int64)
        valid = []
        for i in range(len(ds)):
            item = ds[i]
            valid.append(item is not None)
            if item is None:
                continue
            _sparse(f"item{i}_lidar", item["lidar_bev"].numpy(), A, np.float32)
            _sparse(f"item{i}_map", item["map_bev"].numpy(), A, np.uint8)
            A[f"item{i}_boxes"] = item["gt"]["boxes_xywha"].numpy()
            A[f"item{i}_intentions"] = item["gt"]["intentions"].numpy()
        A["seq_valid"] = np.array(valid)
    assert 0 < sum(valid) < len(valid), "the tree must hold both a kept and a dropped sequence"
    assert any(len(A[f"item{i}_boxes"]) for i, v in enumerate(valid) if v)
    path = os.path.join(OUT, "av2_tiny.npz")
    np.savez_compressed(path, **A)
    print(f"av2_tiny.npz: {len(valid)} sequences ({sum(valid)} items), {os.path.getsize(path)} bytes; GT boxes per item "
          f"{[len(A[f'item{i}_boxes']) for i, v in enumerate(valid) if v]}")


def load_reference(reference_dir):
    """Import the reference's modules (oracle.refshim stand-ins for what is not installed)."""
    import builtins
    import collections
    import importlib
    sys.path.insert(0, REPO)
    from oracle import refshim
    refshim.install(*([reference_dir] if reference_dir else []))
    # heuristic_labeling.py:14 and preprocess_intent_labels.py:16 name these in annotations
    # without importing them
    builtins.ArgoverseStaticMap = type("ArgoverseStaticMap", (), {})
    builtins.namedtuple = collections.namedtuple
    return {m: importlib.import_module(m) for m in ("constants", "heuristic_labeling", "dataset",
                                                    "preprocess_intent_labels")}


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reference", default=os.environ.get("IVIT_REFERENCE"),
                    help="the reference checkout (default: oracle.refshim's)")
    ap.add_argument("what", nargs="*", default=["labels", "tiny"])
    args = ap.parse_args()
    ref = load_reference(args.reference)
    os.makedirs(OUT, exist_ok=True)
    if "labels" in args.what:
        gen_labels(ref)
    if "tiny" in args.what:
        gen_tiny(ref)
