"""Attention maps for chosen BEV cells, the parts that need no GPU: ivit_attn_rows validates its
arguments before any HIP call, and utils.bev_cells inverts generate_anchors' centre formula."""
import os

import pytest
import torch

import _lib
from conftest import REPO
from oracle import ivit_oracle as O

LIB = os.path.join(REPO, "visiontransformer-intention-prediction_amd", "libivit_hip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libivit_hip.so not built (run __graft_entry__.build())")


@needs_lib
def test_attn_rows_rejects_head_dim_before_any_hip_call():
    dll = _lib.lib.load()
    rc = dll.ivit_attn_rows(_lib.BF16, None, 1, 16, 1, 32, 0, None, None, 1, 0, None, None)
    assert rc < 0
    assert b"head dim" in dll.ivit_last_error()
    with pytest.raises(RuntimeError, match="ivit_attn_rows failed"):
        _lib.lib.ivit_attn_rows(_lib.BF16, None, 1, 16, 1, 32, 0, None, None, 1, 0, None, None)


@needs_lib
def test_attn_rows_rejects_prescaled_f32_and_negative_sizes():
    dll = _lib.lib.load()
    assert dll.ivit_attn_rows(_lib.F32, None, 1, 16, 1, 64, 1, None, None, 1, 0, None, None) < 0
    assert b"q_prescaled" in dll.ivit_last_error()
    for B, N, H, R in ((-1, 16, 1, 1), (1, -16, 1, 1), (1, 16, -1, 1), (1, 16, 1, -1)):
        assert dll.ivit_attn_rows(_lib.BF16, None, B, N, H, 64, 0, None, None, R, 0, None, None) < 0
        assert b"negative" in dll.ivit_last_error()
    # no requests: 0 without a launch (no device here, so a launch would fail)
    assert dll.ivit_attn_rows(_lib.BF16, None, 1, 16, 1, 64, 0, None, None, 0, 0, None, None) == 0
    # requests but null arrays: refused on the host
    assert dll.ivit_attn_rows(_lib.BF16, None, 1, 16, 1, 64, 0, None, None, 1, 0, None, None) < 0


@pytest.mark.parametrize("H,W,stride", [(400, 720, 8), (400, 720, 16), (32, 48, 8)])
def test_bev_cells_round_trip(H, W, stride):
    import utils
    A = len(O.ANCHOR_CONFIGS)
    centres = O.generate_anchors(H, W, stride)[::A, :2]  # one centre per location, location-major
    Hf, Wf = H // stride, W // stride
    assert centres.shape == (Hf * Wf, 2)
    cells = utils.bev_cells(centres, (Hf, Wf), stride)
    assert cells.dtype == torch.int64 and cells.shape == (Hf * Wf, 2)
    n = torch.arange(Hf * Wf)
    assert torch.equal(cells[:, 0], n // Wf) and torch.equal(cells[:, 1], n % Wf)
    # not only the centre: the two opposite corners just inside cell (gy, gx)
    for dy, dx in ((0.01, 0.01), (stride - 0.01, stride - 0.01)):
        py, px = (n // Wf) * stride + dy, (n % Wf) * stride + dx
        xy = torch.stack([(300.0 - py) * 0.2, (px - 360.0) * 0.2], dim=1)
        assert torch.equal(utils.bev_cells(xy, (Hf, Wf), stride), cells)


def test_bev_cells_clamps_to_the_border():
    import utils
    Hf, Wf = 50, 90
    far = torch.tensor([[1e4, 1e4], [1e4, -1e4], [-1e4, 1e4], [-1e4, -1e4]])
    # x (forward) far ahead -> the top row gy = 0; px = y / voxel + offset_x: large y -> the last column
    want = torch.tensor([[0, Wf - 1], [0, 0], [Hf - 1, Wf - 1], [Hf - 1, 0]])
    assert torch.equal(utils.bev_cells(far, (Hf, Wf), 8), want)
    assert utils.bev_cells(torch.empty(0, 2), (Hf, Wf), 8).shape == (0, 2)


def test_eval_cnn_refuses_attn_maps(tmp_path):
    """The CNN has no attention: a clear exit before anything is created or any device is asked for."""
    import eval_cnn
    with pytest.raises(SystemExit, match="no attention"):
        eval_cnn.main_eval_cnn(["--synthetic", "--attn-maps", str(tmp_path / "maps")])
    assert not (tmp_path / "maps").exists()
