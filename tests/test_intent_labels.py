"""Intention labelling on the device (csrc/labels.hip, heuristic_labeling.py) against the labels
the REFERENCE's heuristic_labeling.py gave every row of tests/golden/intent_labels.npz
(tools/make_golden_labels.py). The generator keeps every compared quantity at least 1e-6 away
from its threshold, so the labels must be equal on every row."""
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, golden

OTHER = 7


@pytest.fixture(scope="module")
def table():
    z = golden("intent_labels.npz")
    return {k: z[k] for k in z.files}


def _frame(t, rows=None):
    pd = pytest.importorskip("pandas")
    cols = [k for k in t if t[k].ndim == 1 and t[k].shape[0] == t["timestamp_ns"].shape[0]
            and k not in ("heuristic_intent", "yaw_scipy")]
    df = pd.DataFrame({k: t[k] for k in cols})
    return df if rows is None else df.iloc[rows]


def _sorted_inputs(t):
    """The kernel's inputs: rows sorted by (track, timestamp) and the track offsets."""
    codes = np.unique(t["track_uuid"], return_inverse=True)[1]
    order = np.lexsort((t["timestamp_ns"], codes))
    c = codes[order]
    off = np.concatenate([[0], np.flatnonzero(c[1:] != c[:-1]) + 1, [len(c)]]).astype(np.int64)
    xy = np.stack([t["tx_m"], t["ty_m"]], 1)[order]
    quat = np.stack([t["qx"], t["qy"], t["qz"], t["qw"]], 1)[order]
    import constants
    veh = np.isin(t["category"], sorted(constants.VEHICLE_CATEGORIES))[order]
    return order, t["timestamp_ns"][order], xy, quat, veh, off


# ------------------------------------------------------------------------------------------- CPU
def test_golden_table_is_self_consistent(table):
    import constants
    lab = table["heuristic_intent"]
    n = lab.shape[0]
    assert 1400 <= n <= 1600
    assert set(np.unique(lab).tolist()) == set(range(-1, 8))  # every class and -1
    veh = np.isin(table["category"], sorted(constants.VEHICLE_CATEGORIES))
    assert np.array_equal(lab == -1, ~veh)
    assert veh[0] and lab[0] == OTHER  # the vehicle at index label 0 (heuristic_labeling.py:32-34)
    lens = np.unique(table["track_uuid"], return_counts=True)[1]
    assert {1, 5, 6, 30, 31, 35} <= set(lens.tolist())
    assert (lens > 64).sum() >= 2 and (lens > 256).sum() >= 2
    quat = np.stack([table["qx"], table["qy"], table["qz"], table["qw"]], 1)
    norm = np.linalg.norm(quat, axis=1)
    assert (norm == 0).sum() >= 2 and (np.abs(norm[norm > 0] - 1) > 0.1).any() and (table["qw"] < 0).any()
    assert np.isnan(table["yaw_scipy"]).sum() == (norm == 0).sum()
    yaw = table["yaw_scipy"][norm > 0]
    assert yaw.max() > 3.0 and yaw.min() < -3.0 and (np.pi - np.abs(yaw)).min() >= 1e-6
    assert float(table["min_threshold_gap"]) > 1e-6
    # shuffled rows, jittered timestamps with gaps
    codes = np.unique(table["track_uuid"], return_inverse=True)[1]
    assert (np.diff(codes) != 0).sum() > n // 2
    order = np.lexsort((table["timestamp_ns"], codes))
    dt = np.diff(table["timestamp_ns"][order])[np.diff(codes[order]) == 0]
    assert dt.min() > 0 and (dt % 100_000_000 != 0).any() and (dt > 150_000_000).any()


def test_duplicate_track_timestamp_raises_before_any_device_call(table, monkeypatch):
    import heuristic_labeling as hl

    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError(f"device entry {name} reached")
    monkeypatch.setattr(hl, "lib", NoDevice())
    df = _frame(table, np.r_[0:40, 17])
    with pytest.raises(ValueError, match="duplicate"):
        hl.label_annotations(df.reset_index(drop=True))
    with pytest.raises(ValueError, match="duplicate"):
        hl.sort_rows([0, 1, 0], [5, 5, 5])
    order, off = hl.sort_rows([1, 0, 1, 0], [9, 5, 3, 7])
    assert order.tolist() == [1, 3, 2, 0] and off.tolist() == [0, 2, 4]


def test_static_map_is_refused(table):
    import heuristic_labeling as hl
    with pytest.raises(NotImplementedError, match="map-free"):
        hl.get_vehicle_intention_heuristic_enhanced("t", 0, _frame(table, np.r_[0:4]), static_map=object())


def test_importing_utils_does_not_import_pandas():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import utils, trainer, loss, synthetic; "
            "bad = [m for m in ('pandas', 'pyarrow') if m in sys.modules]; assert not bad, bad")
    subprocess.run([sys.executable, "-c", code, PKG], check=True)


# ------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_kernel_labels_equal_the_reference_on_every_row(table):
    import heuristic_labeling as hl
    order, ts, xy, quat, veh, off = _sorted_inputs(table)
    intent, yaw = hl.intent_labels_sorted(ts, xy, quat, veh, off)
    assert intent.dtype == np.int32 and yaw.dtype == np.float64
    want = table["heuristic_intent"][order]
    # the bare kernel knows no index labels: the row at index label 0, which the reference reads
    # as OTHER through its index quirk (applied by label_annotations, next test), is a
    # straight-driving row that the rules label KEEP_LANE; every other row is equal
    quirk = order == 0
    assert np.array_equal(intent[~quirk], want[~quirk]), np.flatnonzero(intent != want)
    assert intent[quirk].tolist() == [0] and want[quirk].tolist() == [OTHER]
    ok = ~np.isnan(table["yaw_scipy"][order])
    err = np.abs(yaw[ok] - table["yaw_scipy"][order][ok])
    print("max |yaw - scipy| =", err.max())
    assert err.max() <= 1e-12
    assert np.all(yaw[~ok] == 0.0)


@pytest.mark.gpu
def test_label_annotations_in_table_order_and_in_a_second_order(table):
    import heuristic_labeling as hl
    df = _frame(table)
    got, yaw = hl.label_annotations(df, return_yaw=True)
    assert got.dtype == np.int64
    assert np.array_equal(got, table["heuristic_intent"])
    ok = ~np.isnan(table["yaw_scipy"])
    assert np.abs(yaw[ok] - table["yaw_scipy"][ok]).max() <= 1e-12
    # the same rows in a second random order, index labels kept: the scatter-back
    perm = np.random.default_rng(3).permutation(len(df))
    assert np.array_equal(hl.label_annotations(df.iloc[perm]), table["heuristic_intent"][perm])


@pytest.mark.gpu
def test_empty_and_single_row(table):
    import heuristic_labeling as hl
    intent, yaw = hl.intent_labels_sorted(np.zeros(0, np.int64), np.zeros((0, 2)), np.zeros((0, 4)), np.zeros(0, bool),
                                          np.zeros(1, np.int64))
    assert intent.shape == (0,) and yaw.shape == (0,)
    assert hl.label_annotations(_frame(table, np.r_[0:0])).shape == (0,)
    intent, yaw = hl.intent_labels_sorted([5], [[1.0, 2.0]], [[0.0, 0.0, np.sin(0.25), np.cos(0.25)]], [True], [0, 1])
    assert intent.tolist() == [OTHER] and abs(yaw[0] - 0.5) <= 1e-12
    intent, _ = hl.intent_labels_sorted([5], [[1.0, 2.0]], [[0.0, 0.0, 0.0, 1.0]], [False], [0, 1])
    assert intent.tolist() == [-1]


@pytest.mark.gpu
def test_two_logs_concatenated_give_the_labels_twice(table):
    pd = pytest.importorskip("pandas")
    import heuristic_labeling as hl
    df = _frame(table)
    n = len(df)
    both = pd.concat([df, df])  # the same track ids and index labels in both logs
    got = hl.label_annotations(both, log_codes=np.repeat([0, 1], n))
    assert np.array_equal(got[:n], table["heuristic_intent"]) and np.array_equal(got[n:], table["heuristic_intent"])
    # the kernel itself on the doubled, sorted table
    order, ts, xy, quat, veh, off = _sorted_inputs(table)
    one, _ = hl.intent_labels_sorted(ts, xy, quat, veh, off)
    two, _ = hl.intent_labels_sorted(np.tile(ts, 2), np.tile(xy, (2, 1)), np.tile(quat, (2, 1)), np.tile(veh, 2),
                                     np.concatenate([off, off[1:] + n]))
    assert np.array_equal(two, np.tile(one, 2))


@pytest.mark.gpu
def test_reference_signature_wrapper(table):
    import heuristic_labeling as hl
    df = _frame(table)
    lab = table["heuristic_intent"]
    rows = [int(np.flatnonzero(lab == c)[1]) for c in range(8)] + [0]
    for r in rows:
        got = hl.get_vehicle_intention_heuristic_enhanced(df["track_uuid"][r], int(df["timestamp_ns"][r]), df, None)
        assert got == lab[r], (r, got, lab[r])
    assert hl.get_vehicle_intention_heuristic_enhanced("no-such-track", 0, df, None) == OTHER
