"""Windowed attention kernels (csrc/attn_window.hip) at op level, per case of win_attn_cases.CASES and
per entry: "f32" / "bf16" = ivit_attn_win_fwd / _bwd with that dtype, "q2" = ivit_attn_win_fwd_q2 /
_bwd_q2 (bf16, Q prescaled by log2(e)/8, dqkv w.r.t. the unscaled q).

Against the f64 reference every tensor (out, dq, dk, dv) is judged on the scale of its own maximum
magnitude. f32: 1e-5 (the project's f32 op-level bound, tests/test_gpu_det_loss.py). bf16 / q2: no
number fixed in advance — the existing GLOBAL bf16 kernels run on each window's tokens gathered into a
sequence of their own (one batched call per window size) through ivit_attn_fwd_q2 / _bwd_q2, which take
any N — for the plain bf16 entry on the same q, k, v with the Q block prescaled and rounded as the qkv GEMM
writes it, their error taken against the entry's own f64 reference — and the windowed kernel's error must
be at most 2 x theirs + one bf16 rounding of the output (2^-9 x scale).
Both errors and their ratio are printed per case ("win_attn_parity ..." lines; profiles/
win_attn_parity.txt is that output).

Exact facts, no tolerance: Nw = 1 windows and the CLS row of every case (out == v, dv == dout,
dq == dk == 0); locality / NaN poison; sample and head permutations; repeatability; guard rows; skip.
"""
import functools

import pytest
import torch

import win_attn_cases as wc

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = wc.B
GUARD = 3  # sentinel rows in front of and behind every output
SENT = 12345.0
ENTRIES = ("f32", "bf16", "q2")
BF16_ROUND = 2.0 ** -9


def _eq(a, b):
    return bool((a == b).all())


def _guarded(rows, cols, dtype):
    t = torch.full((rows + 2 * GUARD, cols), SENT, dtype=dtype, device=DEV)
    return t, t[GUARD:GUARD + rows]


def _guards_ok(t):
    return _eq(t[:GUARD], torch.full_like(t[:GUARD], SENT)) and _eq(t[-GUARD:], torch.full_like(t[-GUARD:], SENT))


def _dev(x, entry):
    return x.to(torch.float32 if entry == "f32" else torch.bfloat16).to(DEV).contiguous()


def run_win(entry, geom, H, qkv, dout, skip=None):
    """-> (out, lse, dqkv) of the windowed entry on device tensors; guard rows checked."""
    from _lib import BF16, F32, lib, ptr, stream
    gh, gw, wh, ww = geom
    N = 1 + gh * gw
    Bn = qkv.shape[0] // N
    D = H * 64
    og, out = _guarded(Bn * N, D, qkv.dtype)
    lg, lse = _guarded(Bn * H, N, torch.float32)
    gg, dqkv = _guarded(Bn * N, 3 * D, qkv.dtype)
    sk = ptr(skip) if skip is not None else None
    if entry == "q2":
        lib.ivit_attn_win_fwd_q2(ptr(qkv), Bn, N, gh, gw, wh, ww, H, 64, ptr(out), ptr(lse), sk, stream())
        lib.ivit_attn_win_bwd_q2(ptr(qkv), ptr(out), ptr(dout), ptr(lse), Bn, N, gh, gw, wh, ww, H, 64, ptr(dqkv), sk,
                                 stream())
    else:
        assert skip is None
        code = F32 if entry == "f32" else BF16
        lib.ivit_attn_win_fwd(code, ptr(qkv), Bn, N, gh, gw, wh, ww, H, 64, ptr(out), ptr(lse), stream())
        lib.ivit_attn_win_bwd(code, ptr(qkv), ptr(out), ptr(dout), ptr(lse), Bn, N, gh, gw, wh, ww, H, 64, ptr(dqkv),
                              stream())
    torch.cuda.synchronize()
    assert _guards_ok(og) and _guards_ok(lg) and _guards_ok(gg), "a guard row was overwritten"
    return out, lse.reshape(Bn, H, N), dqkv


def run_global(entry, H, qkv, dout, Bn, N):
    """The existing global entries on [Bn * N] tokens -> (out, dqkv): "f32" ivit_attn_fwd / _bwd, "q2"
    ivit_attn_fwd_q2 / _bwd_q2 (qkv holds the prescaled Q block)."""
    from _lib import BF16, F32, lib, ptr, stream, workspace
    D = H * 64
    out = torch.empty((Bn * N, D), dtype=qkv.dtype, device=DEV)
    lse = torch.empty((Bn, H, N), dtype=torch.float32, device=DEV)
    dqkv = torch.empty_like(qkv)
    assert entry in ("f32", "q2")
    code = F32 if entry == "f32" else BF16
    ws = workspace(lib.ivit_attn_workspace(code, Bn, N, H, 64, 1), DEV)
    if entry == "q2":
        lib.ivit_attn_fwd_q2(ptr(qkv), Bn, N, H, 64, ptr(out), ptr(lse), None, 0, stream())
        lib.ivit_attn_bwd_q2(ptr(qkv), ptr(out), ptr(dout), ptr(lse), Bn, N, H, 64, ptr(dqkv), ptr(ws), ws.numel(),
                             stream())
    else:
        lib.ivit_attn_fwd(code, ptr(qkv), Bn, N, H, 64, ptr(out), ptr(lse), ptr(ws), ws.numel(), stream())
        lib.ivit_attn_bwd(code, ptr(qkv), ptr(out), ptr(dout), ptr(lse), Bn, N, H, 64, ptr(dqkv), ptr(ws), ws.numel(),
                          stream())
    torch.cuda.synchronize()
    return out, dqkv


@functools.lru_cache(maxsize=None)
def problem(name, entry):
    """-> dict: host inputs of the entry (q2: prescaled Q block), the f64 reference, the windowed run."""
    gh, gw, wh, ww, H = wc.CASES[name]
    qkv, dout = wc.make_inputs(name)
    if entry == "q2":
        qkv = wc.q2_inputs(qkv, H)
    ref = wc.reference(qkv, dout, gh, gw, wh, ww, H, q2=entry == "q2")
    dq, dd = _dev(qkv, entry), _dev(dout, entry)
    out, lse, dqkv = run_win(entry, (gh, gw, wh, ww), H, dq, dd)
    return dict(qkv=qkv, dout=dout, ref=ref, qkv_dev=dq, dout_dev=dd, out=out, lse=lse, dqkv=dqkv)


def _global_operands(entry, H, pr, rows):
    """(entry, H, qkv, dout) of run_global for the rows of a problem: the bf16 entries both go through the
    global q2 kernels, the plain one with its Q block prescaled here."""
    if entry == "f32":
        return "f32", H, _dev(pr["qkv"][rows], "f32"), _dev(pr["dout"][rows], "f32")
    qkv = pr["qkv"][rows] if entry == "q2" else wc.q2_inputs(pr["qkv"][rows], H)
    return "q2", H, _dev(qkv, "q2"), _dev(pr["dout"][rows], "q2")


def _parts(dqkv, D):
    return {"dq": dqkv[:, :D], "dk": dqkv[:, D:2 * D], "dv": dqkv[:, 2 * D:]}


def _tensors(out, dqkv, D):
    return {"out": out, **_parts(dqkv, D)}


@functools.lru_cache(maxsize=None)
def global_errors(name, entry):
    """Errors of the GLOBAL bf16 kernels on the same problem, windows gathered into sequences of their
    own (one batched call per window size): {tensor: max |err| over all patch tokens / scale of the
    reference tensor over the patch tokens}."""
    gh, gw, wh, ww, H = wc.CASES[name]
    pr = problem(name, entry)
    N, D = 1 + gh * gw, H * 64
    ref = _tensors(pr["ref"]["out"], pr["ref"]["dqkv"], D)
    patch = torch.ones(B * N, dtype=torch.bool)
    patch[torch.arange(B) * N] = False
    scale = {k: float(v[patch].abs().max()) or 1.0 for k, v in ref.items()}
    err = {k: 0.0 for k in ref}
    toks = wc.window_tokens(gh, gw, wh, ww)
    for nw in sorted({len(t) for t in toks}):
        group = [t for t in toks if len(t) == nw]
        rows = torch.cat([b * N + t for b in range(B) for t in group])  # [B * windows * nw]
        out, dqkv = run_global(*_global_operands(entry, H, pr, rows), B * len(group), nw)
        got = _tensors(out.cpu(), dqkv.cpu(), D)
        for k in ref:
            err[k] = max(err[k], float((got[k].double() - ref[k][rows]).abs().max()) / scale[k])
    return err, scale, patch


# ------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("name", sorted(wc.CASES))
def test_f32_parity(name):
    gh, gw, wh, ww, H = wc.CASES[name]
    pr = problem(name, "f32")
    D = H * 64
    got, ref = _tensors(pr["out"], pr["dqkv"], D), _tensors(pr["ref"]["out"], pr["ref"]["dqkv"], D)
    errs = {k: wc.rel_err(got[k], ref[k]) for k in ref}
    errs["lse"] = float((pr["lse"].cpu().double() - pr["ref"]["lse"]).abs().max())
    print(f"win_attn_parity {name} f32 " + " ".join(f"{k}={v:.3e}" for k, v in errs.items()))
    for k in ref:
        assert errs[k] <= 1e-5, (name, k, errs[k])
    assert errs["lse"] <= 1e-5 * max(1.0, float(pr["ref"]["lse"].abs().max())), errs["lse"]


@pytest.mark.parametrize("entry", ["bf16", "q2"])
@pytest.mark.parametrize("name", sorted(wc.CASES))
def test_bf16_parity(name, entry):
    gh, gw, wh, ww, H = wc.CASES[name]
    pr = problem(name, entry)
    D = H * 64
    gerr, scale, patch = global_errors(name, entry)
    got, ref = _tensors(pr["out"].cpu(), pr["dqkv"].cpu(), D), _tensors(pr["ref"]["out"], pr["ref"]["dqkv"], D)
    bad = []
    for k in ref:
        werr = float((got[k].double() - ref[k])[patch].abs().max()) / scale[k]
        bound = 2.0 * gerr[k] + BF16_ROUND
        print(f"win_attn_parity {name} {entry} {k}: windowed {werr:.3e} global {gerr[k]:.3e} "
              f"ratio {werr / gerr[k] if gerr[k] > 0 else float('inf'):.2f} bound {bound:.3e}")
        if not werr <= bound:
            bad.append((k, werr, bound))
    # lse: f32 in the entry's units; the scores are f32 sums of bf16 products, so f32 accuracy holds
    lerr = float((pr["lse"].cpu().double() - pr["ref"]["lse"]).abs().max())
    assert lerr <= 1e-4 * max(1.0, float(pr["ref"]["lse"].abs().max())), lerr
    assert not bad, (name, entry, bad)


# ------------------------------------------------------------------------------- exact facts
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", sorted(wc.CASES))
def test_single_token_windows_exact(name, entry):
    """CLS of every case and every one-token window: out == v, dv == dout, dq == dk == 0, bitwise."""
    gh, gw, wh, ww, H = wc.CASES[name]
    pr = problem(name, entry)
    N, D = 1 + gh * gw, H * 64
    ones = [t for t in wc.window_tokens(gh, gw, wh, ww) if len(t) == 1] + [torch.tensor([0])]
    if name == "nw1_3x3_w1x1":
        assert len(ones) == N
    rows = torch.cat([b * N + t for b in range(B) for t in ones]).to(DEV)
    qkv, dout = pr["qkv_dev"], pr["dout_dev"]
    assert _eq(pr["out"][rows], qkv[rows, 2 * D:])
    assert _eq(pr["dqkv"][rows, 2 * D:], dout[rows])
    assert _eq(pr["dqkv"][rows, :2 * D], torch.zeros_like(pr["dqkv"][rows, :2 * D]))


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", sorted(wc.CASES))
def test_locality_and_poison(name, entry):
    """q, k, v of every token outside one window (CLS included) replaced by other values, then by NaN:
    the window's rows of out and dqkv keep their bits."""
    gh, gw, wh, ww, H = wc.CASES[name]
    pr = problem(name, entry)
    N = 1 + gh * gw
    toks = wc.window_tokens(gh, gw, wh, ww)
    full = [i for i, t in enumerate(toks) if len(t) == max(len(u) for u in toks)]
    w = full[len(full) // 2]  # a full-size window (the 256-token one where there is one)
    inside = torch.zeros(B * N, dtype=torch.bool)
    inside[torch.cat([b * N + toks[w] for b in range(B)])] = True
    other = wc.bf16_exact(tuple(pr["qkv"].shape), 999)
    for fill in (other, torch.full_like(other, float("nan"))):
        q = pr["qkv"].clone()
        q[~inside] = fill[~inside]
        out, _, dqkv = run_win(entry, (gh, gw, wh, ww), H, _dev(q, entry), pr["dout_dev"])
        rows = inside.to(DEV)
        assert _eq(out[rows], pr["out"][rows])
        assert _eq(dqkv[rows], pr["dqkv"][rows])


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", sorted(wc.CASES))
def test_sample_and_head_permutation(name, entry):
    gh, gw, wh, ww, H = wc.CASES[name]
    pr = problem(name, entry)
    N, D = 1 + gh * gw, H * 64
    geom = (gh, gw, wh, ww)
    # samples swapped
    flip = lambda t: t.reshape(B, N, -1).flip(0).reshape(B * N, -1).contiguous()
    out, lse, dqkv = run_win(entry, geom, H, flip(pr["qkv_dev"]), flip(pr["dout_dev"]))
    assert _eq(flip(out), pr["out"]) and _eq(lse.flip(0), pr["lse"]) and _eq(flip(dqkv), pr["dqkv"])
    # heads rotated by one
    hq = lambda t: t.reshape(B * N, 3, H, 64).roll(1, 2).reshape(B * N, 3 * D).contiguous()
    ho = lambda t: t.reshape(B * N, H, 64).roll(1, 1).reshape(B * N, D).contiguous()
    out, lse, dqkv = run_win(entry, geom, H, hq(pr["qkv_dev"]), ho(pr["dout_dev"]))
    assert _eq(out, ho(pr["out"])) and _eq(lse, pr["lse"].roll(1, 1)) and _eq(dqkv, hq(pr["dqkv"]))


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", sorted(wc.CASES))
def test_repeatable(name, entry):
    gh, gw, wh, ww, H = wc.CASES[name]
    pr = problem(name, entry)
    out, lse, dqkv = run_win(entry, (gh, gw, wh, ww), H, pr["qkv_dev"], pr["dout_dev"])
    assert _eq(out, pr["out"]) and _eq(lse, pr["lse"]) and _eq(dqkv, pr["dqkv"])


@pytest.mark.parametrize("knob", [1, 0])
@pytest.mark.parametrize("name", sorted(wc.CASES))
def test_skip(name, knob, request):
    """Factors [1/(1-p), 0]: the dropped sample's out and dqkv are exact zeros and its lse unwritten, the
    kept sample bit-identical to skip = None; with IVIT_DROP_SKIP at 0 everything is computed."""
    from _lib import KNOB_DROP_SKIP, lib
    gh, gw, wh, ww, H = wc.CASES[name]
    pr = problem(name, "q2")
    N = 1 + gh * gw
    back = int(lib.ivit_get_knob(KNOB_DROP_SKIP))
    lib.ivit_set_knob(KNOB_DROP_SKIP, knob)
    request.addfinalizer(lambda: lib.ivit_set_knob(KNOB_DROP_SKIP, back))
    skip = torch.tensor([1.0 / (1.0 - 0.1), 0.0], dtype=torch.float32, device=DEV)
    out, lse, dqkv = run_win("q2", (gh, gw, wh, ww), H, pr["qkv_dev"], pr["dout_dev"], skip=skip)
    v = lambda t: t.reshape(B, N, -1)
    assert _eq(v(out)[0], v(pr["out"])[0]) and _eq(lse[0], pr["lse"][0]) and _eq(v(dqkv)[0], v(pr["dqkv"])[0])
    if knob:
        assert _eq(v(out)[1], torch.zeros_like(v(out)[1])) and _eq(v(dqkv)[1], torch.zeros_like(v(dqkv)[1]))
        assert _eq(lse[1], torch.full_like(lse[1], SENT))
    else:
        assert _eq(v(out)[1], v(pr["out"])[1]) and _eq(lse[1], pr["lse"][1]) and _eq(v(dqkv)[1], v(pr["dqkv"])[1])


# ------------------------------------------------------------------------------- the code that exists
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", ["single_4x6_w4x6", "larger_4x6_w8x8"])
def test_whole_grid_window_matches_global_entry(name, entry):
    """A window covering the grid: the patch rows equal the global entry run on the patch tokens alone.
    f32 within 1e-5 of scale; bf16 within the bf16 bound of test_bf16_parity, 2 e_global + 2^-9."""
    gh, gw, wh, ww, H = wc.CASES[name]
    pr = problem(name, entry)
    N, D = 1 + gh * gw, H * 64
    rows = torch.cat([b * N + torch.arange(1, N) for b in range(B)])
    out, dqkv = run_global(*_global_operands(entry, H, pr, rows), B, N - 1)
    got = _tensors(pr["out"][rows.to(DEV)], pr["dqkv"][rows.to(DEV)], D)
    glob = _tensors(out, dqkv, D)
    gerr = global_errors(name, entry)[0] if entry != "f32" else None
    for k in got:
        diff = wc.rel_err(got[k].cpu(), glob[k].cpu().double())
        bound = 1e-5 if entry == "f32" else 2.0 * gerr[k] + BF16_ROUND
        print(f"win_attn_parity {name} {entry} {k}: windowed vs global entry {diff:.3e} bound {bound:.3e}")
        assert diff <= bound, (name, entry, k, diff, bound)


# ------------------------------------------------------------------------------- argument errors
BAD_ARGS = {"too_large": dict(wh=1, ww=257), "zero": dict(wh=0), "n_mismatch": dict(N=26), "head_dim": dict(Dh=32)}


@pytest.mark.parametrize("bad", sorted(BAD_ARGS))
def test_argument_errors(bad):
    """Each returns an error code from the C entries with nothing launched (outputs still sentinel), and
    the ops raise ValueError."""
    import ops
    from _lib import BF16, F32, lib, ptr, stream
    a = dict(gh=4, gw=6, wh=2, ww=3, N=25, Dh=64, H=2)
    a.update(BAD_ARGS[bad])
    gh, gw, wh, ww, N, Dh, H = (a[k] for k in ("gh", "gw", "wh", "ww", "N", "Dh", "H"))
    D = H * 64
    dll = lib.load()
    for dtype in (torch.float32, torch.bfloat16):
        qkv = torch.zeros((B * 25, 3 * D), dtype=dtype, device=DEV)
        dout = torch.zeros((B * 25, D), dtype=dtype, device=DEV)
        out = torch.full((B * 25, D), SENT, dtype=dtype, device=DEV)
        lse = torch.full((B, H, 25), SENT, dtype=torch.float32, device=DEV)
        dqkv = torch.full((B * 25, 3 * D), SENT, dtype=dtype, device=DEV)
        code = F32 if dtype == torch.float32 else BF16
        rcs = [dll.ivit_attn_win_fwd(code, ptr(qkv), B, N, gh, gw, wh, ww, H, Dh, ptr(out), ptr(lse), stream()),
               dll.ivit_attn_win_bwd(code, ptr(qkv), ptr(out), ptr(dout), ptr(lse), B, N, gh, gw, wh, ww, H, Dh,
                                     ptr(dqkv), stream())]
        if dtype == torch.bfloat16:
            rcs += [dll.ivit_attn_win_fwd_q2(ptr(qkv), B, N, gh, gw, wh, ww, H, Dh, ptr(out), ptr(lse), None, stream()),
                    dll.ivit_attn_win_bwd_q2(ptr(qkv), ptr(out), ptr(dout), ptr(lse), B, N, gh, gw, wh, ww, H, Dh,
                                             ptr(dqkv), None, stream())]
        torch.cuda.synchronize()
        assert all(rc != 0 for rc in rcs), rcs
        assert lib.ivit_last_error()
        for t in (out, lse, dqkv):
            assert _eq(t, torch.full_like(t, SENT))
    # the ops refuse before any launch (head dim: a qkv that is not [B*N, 3*H*64])
    Hq = H if Dh == 64 else 1
    qkv = torch.zeros((B * 25, 3 * Hq * Dh), dtype=torch.bfloat16, device=DEV)
    dout = torch.zeros((B * 25, Hq * Dh), dtype=torch.bfloat16, device=DEV)
    win = (gh, gw, wh, ww)
    with pytest.raises(ValueError):
        ops.attn_win_fwd_q2(qkv, B, N, H, win)
    with pytest.raises(ValueError):
        ops.attn_win_bwd_q2(qkv, dout, dout, None, B, N, H, win)
    with pytest.raises(ValueError):
        ops.attn_win_fwd(qkv, B, N, H, BF16, win)
    with pytest.raises(ValueError):
        ops.attn_win_bwd(qkv, dout, dout, None, B, N, H, BF16, win)


def test_ops_match_raw_entries():
    """ops.attn_win_* return what the raw entries write."""
    import ops
    from _lib import BF16
    name = "ragged_5x7_w2x3"
    gh, gw, wh, ww, H = wc.CASES[name]
    N = 1 + gh * gw
    win = (gh, gw, wh, ww)
    pr = problem(name, "q2")
    out, lse = ops.attn_win_fwd_q2(pr["qkv_dev"], B, N, H, win)
    dqkv = ops.attn_win_bwd_q2(pr["qkv_dev"], out, pr["dout_dev"], lse, B, N, H, win)
    assert _eq(out, pr["out"]) and _eq(lse, pr["lse"]) and _eq(dqkv, pr["dqkv"])
    pr = problem(name, "bf16")
    out, lse = ops.attn_win_fwd(pr["qkv_dev"], B, N, H, BF16, win)
    dqkv = ops.attn_win_bwd(pr["qkv_dev"], out, pr["dout_dev"], lse, B, N, H, BF16, win)
    assert _eq(out, pr["out"]) and _eq(lse, pr["lse"]) and _eq(dqkv, pr["dqkv"])
