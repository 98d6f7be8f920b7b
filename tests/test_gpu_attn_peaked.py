"""The bf16 flash attention (attn_fwd_bf16_v6_kernel, attn_bwd_dq_v4_kernel / attn_bwd_dkv_v4_kernel)
on peaked scores: the cases of tests/attn_cases.py, which move the forward's lazy running maximum,
put the row's mass on the key the ragged-tile padding clamps to, and make P one-hot, against f64
references on exactly the tensors the kernels read, under elementwise derived bounds
(max err / bound <= 1; attn_cases.fwd_ratios / bwd_ref state them)."""
import functools

import pytest
import torch

import attn_cases as AC

pytestmark = pytest.mark.gpu
DEV = "cuda"
N0 = 449  # 7 full key tiles + a 1-key ragged one; the last workgroup has one live wave out of four
AK, TAU = AC.kernel_constants()


@functools.lru_cache(maxsize=None)
def _case(name, n):
    """(q', k, v, dO, forward reference): built once per (case, N), shared and left unchanged."""
    q, k, v = AC.make_case(name, n)
    return q, k, v, AC.make_dout(n), AC.fwd_ref(q, k, v)


def _flash_bf16(names, B, n, H):
    """One forward and one backward launch with case names[z] in slot z = b*H + h. Returns the
    per-slot ratios of every bound and the raw outputs."""
    import ops
    cases = [_case(name, n) for name in names]
    qkv = AC.pack_qkv([c[:3] for c in cases], B, n, H).to(DEV)
    dout = AC.pack_rows([c[3] for c in cases], B, n, H).to(DEV)
    o, lse = ops.attn_fwd_q2(qkv, B, n, H)
    dqkv = ops.attn_bwd_q2(qkv, o, dout, lse, B, n, H)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(lse).all())
    assert bool(torch.isfinite(dqkv.float()).all())
    out = []
    for z, (q, k, v, do, ref) in enumerate(cases):
        oz, lz = AC.slot_rows(o, B, n, H, z), lse.reshape(B * H, n)[z].double().cpu()
        r = AC.fwd_ratios(oz, lz, ref)
        bref, bound = AC.bwd_ref(q, k, v, oz, lz, do)
        r.update(AC.bwd_ratios(*AC.slot_qkv(dqkv, B, n, H, z), bref, bound))
        print(f"attn peaked {names[z]} (B,N,H)=({B},{n},{H}) slot {z}: "
              + " ".join(f"{a} {b:.3f}" for a, b in r.items()))
        out.append(r)
    return out, (qkv, o, lse, dout, dqkv)


@pytest.mark.parametrize("name", AC.CASES)
def test_peaked_case_forward_lse_backward(name):
    """Every case at (B, N, H) = (1, 449, 1). Measured max err / bound on an MI355X (the CPU model of
    attn_cases.flash_model gives the same to two digits):
                    o      lse    dQ     dK     dV
      stair9       0.318  0.645  0.680  0.210  0.160
      stair7       0.332  0.664  0.736  0.192  0.152
      stair4       0.288  0.244  0.568  0.182  0.172
      down9        0.203  0.167  0.416  0.204  0.150
      spike_last   0.000  0.002  0.040  0.217  0.148
      spike_first  0.000  0.001  0.022  0.217  0.180
      spike_odd    0.101  0.082  0.643  0.299  0.256
      shift96      0.139  0.140  0.340  0.311  0.315
      perm         0.314  0.001  0.041  0.031  0.475
      gain6        0.505  0.829  0.760  0.793  0.804
      rand         0.157  0.108  0.345  0.324  0.297"""
    (r,), _ = _flash_bf16([name], 1, N0, 1)
    AC.assert_ratios(r, name)


def test_batch_head_slots_hold_different_cases():
    """z = b*H + h: six different cases in the six (batch, head) slots of one launch; a head / batch
    mix-up or state leaking from one slot to the next fails the slot's own reference."""
    names = ["stair9", "rand", "spike_odd", "perm", "down9", "gain6"]
    rs, _ = _flash_bf16(names, 2, N0, 3)
    for name, r in zip(names, rs):
        AC.assert_ratios(r, f"slot {name}")


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 193])
@pytest.mark.parametrize("name", ["spike_last", "spike_first", "stair9"])
def test_tile_edge_sweep(name, n):
    """Key counts around the 32-key fragment and 64-key tile edges. With the row's mass on key N-1
    (spike_last) a clamped padding key that escapes the mask leaves o right and lse off by ln 2 or
    more, against a bound of 2^-8."""
    (r,), _ = _flash_bf16([name], 1, n, 1)
    AC.assert_ratios(r, f"{name} N={n}")


@pytest.mark.parametrize("name", ["stair9", "spike_odd", "gain6"])
def test_plain_entry_is_the_prescaled_pair_on_peaked_scores(name):
    """test_attention_plain_entry_is_the_v4_pair's claim on scores that move the maximum: ivit_attn_fwd
    / ivit_attn_bwd (bf16) on q = bf16(q' / c2) are bitwise ivit_attn_fwd_q2 / ivit_attn_bwd_q2 on
    the Q block bf16(q * c2)."""
    import ops
    from _lib import BF16
    q, k, v, do, _ = _case(name, N0)
    qkv = AC.pack_qkv([((q / AC.f32_const(AC.C2)).to(torch.bfloat16).float(), k, v)], 1, N0, 1).to(DEV)
    dod = AC.pack_rows([do], 1, N0, 1).to(DEV)
    qs = qkv.clone()
    qs[:, :64] = (qkv[:, :64].float() * ops.Q2_SCALE).to(torch.bfloat16)
    # rounding q twice leaves the case what it is: the maximum still moves
    moved, _ = AC.lazy_max_trace(qs[:, :64].double().cpu() @ k.double().T, AK, TAU)
    assert bool(moved.any())
    o, lse = ops.attn_fwd(qkv, 1, N0, 1, BF16)
    o2, l2 = ops.attn_fwd_q2(qs, 1, N0, 1)
    assert torch.equal(o, o2) and torch.equal(lse, l2)
    d_plain = ops.attn_bwd(qkv, o, dod, lse, 1, N0, 1, BF16)
    d_q2 = ops.attn_bwd_q2(qs, o, dod, lse, 1, N0, 1)
    assert torch.equal(d_plain, d_q2)


@pytest.mark.parametrize("name", ["stair9", "spike_odd", "perm"])
def test_flash_agrees_with_attn_rows(name):
    """Two kernels, one softmax: the probabilities ivit_attn_rows returns for 8 query rows match
    P_ref (tests/test_gpu_attn_rows.py's tolerance), and rows @ v agrees with the flash forward's o
    within the forward bound."""
    import ops
    from _lib import BF16
    q, k, v, _, ref = _case(name, N0)
    qkv = AC.pack_qkv([(q, k, v)], 1, N0, 1).to(DEV)
    token = [0, 1, 63, N0 // 2, N0 // 2 + 1, 320, N0 - 2, N0 - 1]
    rows = ops.attn_rows(qkv, 1, N0, 1, BF16, [0] * len(token), token, prescaled=True)[:, 0].double().cpu()
    torch.testing.assert_close(rows, ref["P"][token], rtol=1e-4, atol=1e-12)
    o, _ = ops.attn_fwd_q2(qkv, 1, N0, 1)
    err = (o.double().cpu()[token] - rows @ v.double()).abs()
    ratio = float((err / (2 * AC.U * ref["A"][token] + AC.U * ref["o"][token].abs())).max())
    print(f"attn peaked {name}: flash o vs attn_rows @ v, max err / bound {ratio:.3f}")
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("name", AC.CASES)
def test_f32_parity_path_within_4x_of_torch_f32(name):
    """ivit_attn_fwd / ivit_attn_bwd with F32 on q = q' / c2: err / abs-product (attn_cases.f32_ref)
    against an f64 reference on the f32 inputs, per output at most 4 times what torch's own f32
    scaled_dot_product_attention and its autograd make of the same inputs on the CPU (both plain
    f32; the factor is for the accumulation order).

    Measured, kernel (torch), in units of 1e-7:
                    o              dQ              dK              dV
      stair9       5.56 (6.19)    1.14 (1.86)     0.56 (0.77)     4.08 (4.64)
      stair7       8.05 (7.82)    1.08 (1.93)     0.53 (0.60)     3.32 (4.68)
      stair4       5.47 (5.02)    0.85 (1.92)     0.46 (0.31)     1.89 (1.89)
      down9        4.75 (4.60)    0.83 (0.94)     0.70 (0.85)     4.23 (3.31)
      spike_last   0.043 (0.043)  0.0017 (0.37)   0.40 (0.31)     2.44 (1.92)
      spike_first  0.057 (0.057)  0.0013 (0.39)   0.39 (0.31)     2.26 (1.99)
      spike_odd    1.47 (1.61)    0.46 (1.60)     0.30 (0.43)     1.78 (1.60)
      shift96      15.4 (17.5)    2.14 (4.64)     2.44 (4.71)     14.4 (17.5)
      perm         17.0 (18.7)    0.57 (0.57)     0.57 (0.57)     13.2 (14.7)
      gain6        51.8 (48.3)    5.94 (6.85)     10.7 (12.4)     55.2 (57.3)
      rand         4.37 (4.03)    0.71 (0.50)     0.96 (0.62)     4.66 (3.04)
    With P recomputed as exp(S - lse) from the f32 lse (the backward before this test) perm's dQ
    and dK stood at 2.56 (0.57), 4.5 times torch's, and stair9's dQ at 4.74 (1.86)."""
    import ops
    from _lib import F32
    q, k, v, do, _ = _case(name, N0)
    qf, kf, vf = AC.f32_inputs(q, k, v)
    ref, scale = AC.f32_ref(qf, kf, vf, do)
    base = AC.f32_metric(AC.torch_sdpa_f32(qf, kf, vf, do), ref, scale)
    qkv = AC.pack_qkv([(qf, kf, vf)], 1, N0, 1, torch.float32).to(DEV)
    dod = AC.pack_rows([do], 1, N0, 1, torch.float32).to(DEV)
    o, lse = ops.attn_fwd(qkv, 1, N0, 1, F32)
    dqkv = ops.attn_bwd(qkv, o, dod, lse, 1, N0, 1, F32)
    dq, dk, dv = AC.slot_qkv(dqkv, 1, N0, 1, 0)
    got = AC.f32_metric({"o": o.cpu(), "dq": dq, "dk": dk, "dv": dv}, ref, scale)
    lse_err = float((lse.reshape(-1).double().cpu() - torch.logsumexp(qf.double() @ kf.double().T / 8.0, 1)).abs().max())
    print(f"attn f32 {name}: " + " ".join(f"{n} {got[n]:.3e} (torch {base[n]:.3e})" for n in got)
          + f" lse abs {lse_err:.3e}")
    bad = {n: (got[n], base[n]) for n in got if not got[n] <= 4.0 * base[n]}
    assert not bad, bad
