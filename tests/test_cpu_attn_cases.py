"""The peaked attention cases of tests/attn_cases.py, judged without a GPU: each case must do, under
the kernel's own constants, what it exists for (move the forward's lazy maximum, or not), and a
faithful CPU model of the algorithm must meet every bound the GPU tests assert, so the inputs and
bounds are satisfiable by a correct implementation."""
import functools
import math

import pytest
import torch

import attn_cases as AC

AK, TAU = AC.kernel_constants()
N = 449  # 7 full key tiles and a 1-key ragged one


@functools.lru_cache(maxsize=None)
def _case(name, n=N):
    q, k, v = AC.make_case(name, n)
    return q, k, v, AC.fwd_ref(q, k, v)


@functools.lru_cache(maxsize=None)
def _trace(name, n=N):
    return AC.lazy_max_trace(_case(name, n)[3]["S"], AK, TAU)


def test_kernel_constants_are_the_ones_the_cases_were_built_for():
    # the stair heights (9, 7, 4 per 64 keys) bracket TAU = 8 on tiles of 64 keys
    assert (AK, TAU) == (64, 8.0)


@pytest.mark.parametrize("name", AC.CASES)
def test_inputs_are_bf16_exact_and_bumps_exact(name):
    q, k, v, ref = _case(name)
    for t in (q, k, v):
        assert torch.equal(t, t.to(torch.bfloat16).float())
    assert float(ref["S"].abs().max()) <= 128.0  # the 2^-16 exponent term of the backward bound
    if name.startswith("stair") or name == "down9":
        base = q[:, :62].double() @ k[:, :62].double().T
        assert torch.equal(ref["S"], base + k[:, 63].double()[None, :])
        assert float(base.abs().max()) < 2.5


def test_stair9_moves_the_maximum_at_every_step():
    """Every one of the 7 tile steps moves the maximum, through both pipeline stage bodies. A step is
    9 + (the tile's largest base score - the running one), so at the 6 full-tile steps all rows move
    but the odd one whose base scores spread by more than 1 (a long q' row), and at the ragged 1-key
    tile, where one base score stands against the maximum of 64, only part of the rows."""
    moved, _ = _trace("stair9")
    assert moved.shape == (7, N)
    assert bool((moved[:6].sum(dim=1) >= N - 2).all())
    assert bool((moved[:6].sum(dim=0) >= 5).all())  # every row: at 5 of the 6 full-tile steps at least
    last = int(moved[6].sum())
    assert 0 < last < N
    # within a 32-query wave both outcomes occur: the per-lane "moved ? mt : 0" under __any
    assert any(0 < int(moved[6, w:w + 32].sum()) < 32 for w in range(0, N - 32, 32))


def test_stair7_stays_under_tau_then_jumps():
    moved, pexp = _trace("stair7")
    assert not bool(moved[0].any()) and bool(moved[1].all())
    assert pexp >= 7.0 - 1.0 and pexp <= TAU


def test_stair4_moves_every_third_tile_at_most():
    moved, pexp = _trace("stair4")
    assert not bool(moved[0].any()) and bool(moved[1].any() or moved[2].any())
    assert int(moved.any(dim=1).sum()) >= 2
    assert 7.0 <= pexp <= TAU


def test_spike_odd_moves_odd_rows_only():
    moved, _ = _trace("spike_odd")
    rows = moved.any(dim=0)
    assert bool(rows[1::2].all()) and not bool(rows[0::2].any())
    assert int(moved.any(dim=1).sum()) == 2  # key N // 2 (+20), then the last key (+40)
    assert bool(moved[6, 1::2].all())  # the ragged tile


def test_spike_last_moves_every_row_at_the_ragged_tile():
    moved, _ = _trace("spike_last")
    assert bool(moved[6].all()) and not bool(moved[:6].any())
    assert float(_case("spike_last")[3]["P"][:, N - 1].min()) > 0.999999


@pytest.mark.parametrize("name", ["rand", "down9", "shift96", "spike_first"])
def test_control_cases_never_move(name):
    moved, _ = _trace(name)
    assert not bool(moved.any())


def test_down9_underflows_later_tiles():
    P = _case("down9")[3]["P"]
    assert float(P[:, 3 * AK:].max()) < 2.0 ** -24 and float(P[:, 6 * AK:].max()) < 2.0 ** -50


def test_perm_is_one_hot_and_moves_lanes_at_different_tiles():
    q, k, v, ref = _case("perm")
    assert float(ref["P"].max(dim=1).values.min()) > 0.999
    assert len(set(ref["P"].argmax(dim=1).tolist())) == N  # a permutation: every key is some row's
    moved, _ = _trace("perm")
    assert bool(moved.any(dim=1).all())  # some lane moves at every step
    assert int(moved.sum(dim=0).max()) >= 1 and not bool(moved.all(dim=1).any())


def test_gain6_is_peaked_and_moves():
    ref = _case("gain6")[3]
    assert float(ref["P"].max(dim=1).values.mean()) > 0.4
    assert bool(_trace("gain6")[0].any())


def test_some_case_reaches_two_to_the_seven_unrescaled():
    assert max(_trace(n)[1] for n in AC.CASES) >= 7.0
    assert all(_trace(n)[1] <= TAU for n in AC.CASES)


@pytest.mark.parametrize("n", [65, 130, 449])
@pytest.mark.parametrize("name", AC.CASES)
def test_model_meets_every_bound(name, n):
    q, k, v, ref = _case(name, n)
    dout = AC.make_dout(n)
    o, lse, dq, dk, dv = AC.flash_model(q, k, v, dout, AK, TAU)
    r = AC.fwd_ratios(o, lse, ref)
    bref, bound = AC.bwd_ref(q, k, v, o, lse, dout)
    r.update(AC.bwd_ratios(dq, dk, dv, bref, bound))
    print(f"model {name} N={n}: " + " ".join(f"{a} {b:.3f}" for a, b in r.items()))
    AC.assert_ratios(r, f"model {name} N={n}")


@pytest.mark.parametrize("name", AC.CASES)
def test_torch_f32_figures_are_finite_and_nonzero(name):
    """The f32 parity test measures the kernel against torch's own f32 error: that yardstick must
    exist on every case."""
    q, k, v, _ = _case(name)
    dout = AC.make_dout(N)
    qf, kf, vf = AC.f32_inputs(q, k, v)
    ref, scale = AC.f32_ref(qf, kf, vf, dout)
    fig = AC.f32_metric(AC.torch_sdpa_f32(qf, kf, vf, dout), ref, scale)
    print(f"torch f32 {name}: " + " ".join(f"{a} {b:.3e}" for a, b in fig.items()))
    assert all(math.isfinite(x) and x > 0.0 for x in fig.values()), fig
