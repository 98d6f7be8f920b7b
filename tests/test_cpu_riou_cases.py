"""Rotated-IoU regression, CPU side: the torch reference of tests/riou_cases.py against the
oracle's own f64 helpers and their central differences, the closed forms, the host build of
csrc/geom_ad.h under AddressSanitizer + UBSan (a stand-alone program, run as a child process),
the new C-ABI entries' validation without a device, and the training flag."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import riou_cases as R
from conftest import PKG, REPO

LIB = os.path.join(PKG, "libivit_hip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libivit_hip.so not built (run __graft_entry__.build())")


def _gerr(got, ref):
    """max |got - ref| in units of max(|ref|_max, 1e-3), per case."""
    return float(np.abs(np.asarray(got) - np.asarray(ref)).max() / max(float(np.abs(ref).max()), 1e-3))


# ----------------------------------------------------------------------------- the reference itself
def test_reference_value_matches_oracle_helpers():
    boxes, targets = R.smooth_cases(0, 200)
    _, _, ref, _ = R.pool()
    n = 0
    for b, t, v in zip(boxes, targets, ref[2:202]):
        assert abs(v - R.oracle_iou(b, t)) <= 1e-12
        n += v > 0.05
    assert n > 150  # the law overlaps: the comparison is not one of zeros


def test_reference_gradient_matches_central_differences():
    boxes, targets = R.smooth_cases(0, 200)
    _, _, _, gref = R.pool()
    h, worst = 1e-5, 0.0
    for b, t, g in zip(boxes, targets, gref[2:202]):
        fd = np.zeros(5)
        for k in range(5):
            e = np.zeros(5)
            e[k] = h
            fd[k] = (R.oracle_iou(b + e, t) - R.oracle_iou(b - e, t)) / (2 * h)
        worst = max(worst, _gerr(g, fd))
    print(f"reference gradient vs central differences: {worst:.3g}")
    assert worst <= 1e-6


def test_redraw_share_under_cap():
    for seed in range(5):
        share = R.redraw_share(seed, 200)
        print(f"seed {seed}: redrew {share:.1%}")
        assert share < 0.2


def test_closed_forms():
    for box, target, iou, grad in R.closed_form_cases():
        v, g = R.riou_ref_grad(box, target)
        assert abs(v - iou) <= 1e-12
        assert np.abs(g - grad).max() <= 1e-12


# ----------------------------------------------------------------------------- host build of geom_ad.h
def _host_compiler():
    import importlib.util
    spec = importlib.util.spec_from_file_location("asan_abi", os.path.join(REPO, "tools", "asan_abi.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    cxx = os.path.join(os.path.dirname(os.path.realpath(m.HIPCC)), "..", "lib", "llvm", "bin", "clang++")
    if not os.path.exists(cxx):
        cxx = "/opt/rocm/lib/llvm/bin/clang++"
    return cxx if os.path.exists(cxx) else None


@pytest.fixture(scope="module")
def riou_host(tmp_path_factory):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host compiler (the ROCm clang++ that tools/asan_abi.py links with)")
    exe = str(tmp_path_factory.mktemp("riou_host") / "riou_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-ffp-contract=off", "-I", os.path.join(PKG, "csrc"), os.path.join(REPO, "tools", "riou_host.cpp"),
                    "-o", exe], check=True)

    def run(rows, tmp):
        path = os.path.join(str(tmp), "cases.txt")
        with open(path, "w") as fh:
            for r in rows:
                fh.write(" ".join(repr(float(x)) for x in r) + "\n")
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
        p = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        assert "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-2000:]
        return np.array([[float(x) for x in ln.split()] for ln in p.stdout.splitlines()])
    return run


def test_host_build_matches_reference(riou_host, tmp_path):
    boxes, targets, iou, grad = R.pool()
    out = riou_host(np.concatenate([boxes, targets], axis=1), tmp_path)
    assert out.shape == (len(boxes), 6)
    assert np.abs(out[:, 0] - iou).max() <= 1e-12
    worst = max(_gerr(o[1:], g) for o, g in zip(out, grad))
    print(f"host geom_ad.h vs reference: iou {np.abs(out[:, 0] - iou).max():.3g}, gradient {worst:.3g}")
    assert worst <= 1e-9
    for (_, _, v, g), o in zip(R.closed_form_cases(), out):
        assert abs(o[0] - v) <= 1e-12 and np.abs(o[1:] - g).max() <= 1e-9 * max(np.abs(g).max(), 1e-3)


def test_host_build_edge_cases(riou_host, tmp_path):
    cases = R.edge_cases()
    names = list(cases)
    out = riou_host([np.concatenate(cases[k]) for k in names], tmp_path)
    got = dict(zip(names, out))
    for k in R.ZERO_CASES:
        assert np.array_equal(got[k], np.zeros(6)), (k, got[k])
    for k in R.FINITE_CASES:
        assert np.isfinite(got[k]).all(), (k, got[k])
    assert abs(got["identical"][0] - 1.0) <= 1e-12
    for k in R.NAN_CASES:
        assert math.isnan(got[k][0]), (k, got[k])


def test_host_build_decode_chain(riou_host, tmp_path):
    raw, anchor, target = (R._f32(v) for v in R.ZERO_ANGLE_CASE)
    rows = [np.concatenate([raw, anchor, target])]
    raw2 = raw.copy()
    raw2[4:] = R._f32([0.3, 0.9])
    rows.append(np.concatenate([raw2, anchor, target]))
    out = riou_host(rows, tmp_path)
    # d4 = d5 = 0: yaw = the anchor's, the two angle derivatives are exact zeros, the rest finite
    assert out[0][0] > 0.3 and np.isfinite(out[0]).all() and out[0][5] == 0.0 and out[0][6] == 0.0
    assert np.abs(out[0][1:5]).min() > 0
    v, g = R.riou_ref_decoded(raw2, anchor, target)
    assert abs(out[1][0] - v) <= 1e-12 and _gerr(out[1][1:], g) <= 1e-9


# ----------------------------------------------------------------------------- C ABI without a device
NEW = ("ivit_riou_pairs_fwd", "ivit_riou_pairs_bwd", "ivit_det_iou_loss_workspace", "ivit_det_iou_loss_fwd",
       "ivit_det_iou_loss_bwd")


@needs_lib
def test_new_symbols_declared_and_exported():
    import _lib
    protos = _lib.parse_header()
    dll = ctypes.CDLL(LIB)
    for n in NEW:
        assert n in protos and hasattr(dll, n), n


@needs_lib
def test_workspace_query_is_host_arithmetic_and_monotone():
    import _lib
    dll = _lib.lib.load()
    ws = dll.ivit_det_iou_loss_workspace
    assert ws(0, 100) == 0 and ws(-1, -1) == 0
    # six f32 gradients per anchor + two f64 partials per 256-anchor block, each 256-byte aligned
    assert ws(8, 22500) == 8 * 22500 * 24 + 704 * 16  # 704 blocks; both parts are multiples of 256
    assert ws(1, 8) == 256 + 256
    prev = 0
    for B, NA in ((1, 1), (1, 70), (2, 70), (2, 300), (8, 300), (8, 22500), (32, 22500)):
        cur = ws(B, NA)
        assert cur > prev, (B, NA)
        prev = cur


@needs_lib
def test_validation_before_any_device_call():
    import _lib
    dll = _lib.lib.load()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    assert dll.ivit_riou_pairs_fwd(None, None, 0, None, None, None) == 0  # n = 0: a no-op
    assert dll.ivit_riou_pairs_bwd(None, None, 0, None, None) == 0
    assert dll.ivit_riou_pairs_fwd(p, p, -1, p, p, None) < 0 and b"n >= 0" in dll.ivit_last_error()
    assert dll.ivit_riou_pairs_bwd(p, p, -1, p, None) < 0
    assert dll.ivit_riou_pairs_fwd(None, None, 4, None, None, None) < 0 and b"null" in dll.ivit_last_error()
    assert dll.ivit_riou_pairs_bwd(None, None, 4, None, None) < 0
    need = dll.ivit_det_iou_loss_workspace(1, 8)
    assert need <= ctypes.sizeof(buf)
    assert dll.ivit_det_iou_loss_fwd(p, p, 0, 8, p, p, 1, 1, 1.0, 1.0, p, 32, p, p, need, None) == 0
    assert dll.ivit_det_iou_loss_fwd(p, p, -1, 8, p, p, 1, 1, 1.0, 1.0, p, 32, p, p, need, None) < 0
    assert dll.ivit_det_iou_loss_fwd(None, None, 1, 8, None, None, 1, 1, 1.0, 1.0, None, 0, None, None, 0, None) < 0
    assert dll.ivit_det_iou_loss_fwd(p, p, 1, 8, p, p, 1, 1, 1.0, 1.0, p, 32, p, p, need - 1, None) < 0
    assert b"workspace too small" in dll.ivit_last_error()
    assert dll.ivit_det_iou_loss_fwd(p, p, 1, 8, p, p, 1, 1, 1.0, 1.0, p, 31, p, p, need, None) < 0
    assert dll.ivit_det_iou_loss_bwd(0, 0, 1.0, 1.0, None, None, None, 0, None, 0, None, None) == 0
    assert dll.ivit_det_iou_loss_bwd(1, -8, 1.0, 1.0, p, p, p, 32, p, need, p, None) < 0
    assert dll.ivit_det_iou_loss_bwd(1, 8, 1.0, 1.0, None, None, None, 32, None, need, None, None) < 0
    assert dll.ivit_det_iou_loss_bwd(1, 8, 1.0, 1.0, p, p, p, 32, p, need - 1, p, None) < 0


# ----------------------------------------------------------------------------- flag and constructor
def test_train_flag_parses():
    import constants
    import train_vit
    assert constants.BOX_IOU_LOSS_WEIGHT == 0.0
    assert train_vit.parse_args([]).iou_loss_weight == 0.0
    assert train_vit.parse_args(["--iou-loss-weight", "0.5"]).iou_loss_weight == 0.5
    import train_cnn
    assert train_cnn.parse_args(["--iou-loss-weight", "2"]).iou_loss_weight == 2.0
    with pytest.raises(SystemExit):
        train_vit.parse_args(["--iou-loss-weight", "-1"])


def test_loss_constructor_argument():
    import loss as L
    assert L.DetectionIntentionLoss().iou_loss_weight == 0.0
    assert L.DetectionIntentionLoss(iou_loss_weight=0.5).iou_loss_weight == 0.5
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            L.DetectionIntentionLoss(iou_loss_weight=bad)
