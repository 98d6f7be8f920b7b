"""Rotated NMS, the parts that need no GPU: the four C-ABI entry points exist, their workspace
queries are pure host arithmetic, their argument checks run before any device call, and the
eval entry point has the ``--rotated-nms`` switch (off by default)."""
import ctypes
import os

import pytest

import _lib
from conftest import REPO

LIB = os.path.join(REPO, "visiontransformer-intention-prediction_amd", "libivit_hip.so")

pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libivit_hip.so not built (run __graft_entry__.build())")

NEW = ["ivit_nms_rotated_batched_workspace", "ivit_nms_rotated_batched", "ivit_eval_post_rotated_workspace",
       "ivit_eval_post_rotated"]


def test_new_symbols_declared_and_exported():
    dll = ctypes.CDLL(LIB)
    protos = _lib.parse_header()
    for name in NEW:
        assert name in protos, name
        assert hasattr(dll, name), name
    # same signatures as the axis-aligned entry points
    assert protos["ivit_nms_rotated_batched"] == protos["ivit_nms_batched"]
    assert protos["ivit_eval_post_rotated"] == protos["ivit_eval_post"]


def test_workspace_queries_are_pure_host():
    dll = _lib.lib.load()
    assert dll.ivit_nms_rotated_batched_workspace(0, 0, 0) == 64
    assert dll.ivit_nms_rotated_batched_workspace(3, 0, 0) == 64
    assert dll.ivit_eval_post_rotated_workspace(0, 22500) == 64
    assert dll.ivit_eval_post_rotated_workspace(4, 0) == 64
    prev = 64
    for n in (1, 63, 64, 65, 1300, 22500):
        words = n * ((n + 63) // 64)
        rot, axis = dll.ivit_nms_rotated_batched_workspace(1, n, words), dll.ivit_nms_batched_workspace(1, n, words)
        assert rot >= axis + 112 * n  # the polygons (80 B) and prefilter records (32 B) of every row
        assert rot > prev
        prev = rot
    prev = 64
    for B, NA in ((1, 1), (1, 64), (2, 64), (2, 4500), (8, 22500), (32, 22500)):
        rot, axis = dll.ivit_eval_post_rotated_workspace(B, NA), dll.ivit_eval_post_workspace(B, NA)
        assert rot >= axis + 112 * B * NA
        assert rot > prev
        prev = rot
    # the eval form still reserves the worst-case suppression masks
    assert dll.ivit_eval_post_rotated_workspace(32, 22500) >= 32 * 22500 * 352 * 8


def _al16(x):
    return (x + 15) // 16 * 16


def test_workspace_values_are_the_documented_formulas():
    """The batched and eval workspace queries, value for value (callers size their buffers with
    them; the layouts behind them may be reorganised, the numbers may not move)."""
    dll = _lib.lib.load()
    for ns in ([1], [64], [10, 65, 65], [22500]):  # (S, T, W) = (1, 1, 1), (1, 64, 64), (3, 140, 270), ...
        S, T = len(ns), sum(ns)
        W = sum(n * ((n + 63) // 64) for n in ns)
        axis = _al16(4 * T) + _al16(20 * T) + _al16(8 * W) + 4 * _al16(4 * T) + 64
        assert dll.ivit_nms_batched_workspace(S, T, W) == axis, ns
        assert dll.ivit_nms_rotated_batched_workspace(S, T, W) == axis + _al16(80 * T) + _al16(32 * T), ns
    for B, NA in ((1, 1), (2, 64), (8, 22500)):
        R, nw = B * NA, (NA + 63) // 64
        sizes = [4 * B, 4 * R, 4 * R, 20 * R, 4 * R, 4 * R, 4 * R, 4 * R, 4 * R, 20 * R, 8 * R, 8 * R * nw]
        axis = sum(_al16(s) for s in sizes) + 16
        assert dll.ivit_eval_post_workspace(B, NA) == axis, (B, NA)
        assert dll.ivit_eval_post_rotated_workspace(B, NA) == axis + _al16(80 * R) + _al16(32 * R), (B, NA)
    for fn in (dll.ivit_nms_batched_workspace, dll.ivit_nms_rotated_batched_workspace):
        assert fn(0, 0, 0) == fn(3, 0, 0) == fn(0, 5, 5) == 64
    for fn in (dll.ivit_eval_post_workspace, dll.ivit_eval_post_rotated_workspace):
        assert fn(0, 64) == fn(4, 0) == 64


def test_argument_validation_names_the_axis_entries_too():
    dll = _lib.lib.load()
    rc = dll.ivit_nms_batched(None, None, None, None, 1, 131073, 131073, 131073 * 2049, 0.2, None, None, None, 1 << 62,
                              None)
    assert rc < 0 and dll.ivit_last_error().startswith(b"ivit_nms_batched: n=131073")
    rc = dll.ivit_nms(None, None, 131073, 0.2, None, None, None, 1 << 62, None)
    assert rc < 0 and dll.ivit_last_error().startswith(b"ivit_nms: n=131073")
    rc = dll.ivit_eval_post(None, None, None, None, 1, 64, 0, 0.1, 0.2, None, None, None, None, None, 1 << 62, None)
    assert rc < 0 and dll.ivit_last_error().startswith(b"ivit_eval_post: bad sizes") and b"K 0" in dll.ivit_last_error()
    rc = dll.ivit_nms_batched(None, None, None, None, 1, 64, 64, 64, 0.2, None, None, None, 64, None)
    assert rc < 0 and dll.ivit_last_error() == b"ivit_nms_batched: workspace too small"


def test_argument_validation_without_device():
    dll = _lib.lib.load()
    rc = dll.ivit_nms_rotated_batched(None, None, None, None, 1, 131073, 131073, 131073 * 2049, 0.2, None, None, None,
                                      1 << 62, None)
    assert rc < 0
    assert b"ivit_nms_rotated_batched" in dll.ivit_last_error() and b"131073" in dll.ivit_last_error()
    rc = dll.ivit_eval_post_rotated(None, None, None, None, 1, 64, 0, 0.1, 0.2, None, None, None, None, None, 1 << 62,
                                    None)
    assert rc < 0
    assert b"ivit_eval_post_rotated" in dll.ivit_last_error() and b"K 0" in dll.ivit_last_error()
    # a workspace that is too small is refused as well
    rc = dll.ivit_eval_post_rotated(None, None, None, None, 1, 64, 8, 0.1, 0.2, None, None, None, None, None,
                                    dll.ivit_eval_post_workspace(1, 64), None)
    assert rc < 0 and b"workspace too small" in dll.ivit_last_error()
    with pytest.raises(RuntimeError, match="ivit_eval_post_rotated failed"):
        _lib.lib.ivit_eval_post_rotated(None, None, None, None, 1, 64, 0, 0.1, 0.2, None, None, None, None, None, 0,
                                        None)


def test_eval_flag_and_constant():
    import constants
    import eval_vit
    assert constants.EVAL_USE_ROTATED_NMS is False
    assert eval_vit.parse_args(["--rotated-nms"]).rotated_nms is True
    assert eval_vit.parse_args([]).rotated_nms is False
    a = eval_vit.parse_args(["--rotated-nms"])
    assert a.rotated is False  # independent of --rotated
    assert eval_vit.parse_args(["--rotated"]).rotated_nms is False


def test_python_keywords_default_off():
    import inspect

    import utils
    for fn, kw in ((utils.apply_nms, "rotated"), (utils.nms_batched, "rotated"),
                   (utils.postprocess_batch, "rotated_nms"), (utils.PostPipeline.__init__, "rotated_nms"),
                   (__import__("eval_vit").run_inference, "rotated_nms")):
        assert inspect.signature(fn).parameters[kw].default is False, fn
