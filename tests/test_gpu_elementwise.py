"""The element-wise kernels of csrc/elementwise.hip and ivit_colsum (csrc/gemm_ops.hip), op by op:
the casts bit for bit against torch's CPU rounding, the activation gradients against f64 with the exact
erf, the column sums under the per-column bound of tests/norm_cases.py, the copies and the head
split / merge exactly.

Dispatch branches of ivit_add_act_grad and the tests that reach them: add_act_grad8_kernel (n % 8 == 0,
row_elems % 8 == 0 when there is a row_scale, 16-B aligned operands) at n = 296 with row_elems 8 and
24; the scalar add_act_grad_kernel at n = 299, at row_elems = 12 with a row_scale, and on a
4-byte-offset operand (test_add_act_grad, test_add_act_grad_8wide_and_scalar_agree_bitwise)."""
import itertools
import math

import numpy as np
import pytest
import torch

import norm_cases as NC

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16T = torch.float32, torch.bfloat16
K = NC.kernel_constants()
SENTINEL = -777.25
ACT_TOL = 1e-6  # the existing activation test's bound; torch's own f32 CPU gelu' is 2e-7 on [-12, 12]


def _put(t, dtype=F32):
    return None if t is None else t.to(dtype).to(DEV)


def _off(t, dtype=F32):
    """t on the device at a 4-byte offset into a larger buffer."""
    k = 4 // torch.empty((), dtype=dtype).element_size()
    buf = torch.empty(t.numel() + 8, dtype=dtype, device=DEV)
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t.to(dtype))
    assert v.data_ptr() % 16 == 4
    return v


def _exact(t, dtype):
    return NC.bf16_exact(t) if dtype == BF16T else t


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _act_ratio(got, ref):
    """|err| <= 1e-6 max(1, |ref|), plus one bf16 ulp (2^-8 |ref| rounding + the tie side) for a bf16
    output."""
    bound = ACT_TOL * ref.abs().clamp_min(1.0)
    if got.dtype == BF16T:
        bound = bound + NC.U * ref.abs()
    return NC._ratio((got.detach().cpu().double() - ref).abs(), bound)


# ----------------------------------------------------------------------------- casts
def _f32_from_bits(bits):
    return torch.from_numpy(np.asarray(bits, dtype=np.uint32).view(np.float32).copy())


def _normal_bf16_patterns():
    h = np.arange(65536, dtype=np.uint32)
    e = (h >> 7) & 0xFF
    return h[(e != 0) & (e != 255)]


def test_cast_f32_to_bf16_rounds_to_nearest_even_bit_for_bit():
    """ops.cast f32 -> bf16 against torch's CPU .to(bfloat16), int16 views equal: every finite normal
    bf16 value widened (must round-trip), every tie (value + half an ulp, both parities of the kept
    bit), the f32 neighbours one ulp either side of each tie, +-0, +-f32 max (-> +-inf), +-inf, NaN (as
    "is NaN"), 100 001 randn; an odd element count. Magnitudes below 2^-126 are left out: flushing
    denormals is a build mode, not a property of this kernel."""
    import ops
    base = _normal_bf16_patterns() << 16
    special = np.array([0x0, 0x80000000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000], dtype=np.uint32)
    x = torch.cat([_f32_from_bits(np.concatenate([base, base | 0x8000, base | 0x7FFF, base | 0x8001, special])),
                   torch.randn(100001, generator=torch.Generator().manual_seed(11))])
    if x.numel() % 2 == 0:
        x = torch.cat([x, torch.tensor([1.0 + 2.0 ** -8])])  # one more tie
    assert x.numel() % 2 == 1
    nz = x[x != 0]
    assert float(nz[torch.isfinite(nz)].abs().min()) >= 2.0 ** -126
    want = x.to(BF16T)
    got = ops.cast(x.to(DEV), BF16T).cpu()
    nan = torch.isnan(x)
    assert int(nan.sum()) == 1 and bool(torch.isnan(got[nan].float()).all())
    bad = (got.view(torch.int16) != want.view(torch.int16)) & ~nan
    assert not bool(bad.any()), (int(bad.sum()), x[bad][:5], got[bad][:5].float(), want[bad][:5].float())
    n = base.size
    assert torch.equal(got[:n].float(), x[:n])  # the round trip, said directly


def test_cast_bf16_to_f32_is_exact_and_same_dtype_returns_input():
    import ops
    bits = np.concatenate([_normal_bf16_patterns(), np.array([0x0, 0x8000, 0x7F80, 0xFF80, 0x3F80], dtype=np.uint32)])
    b = torch.from_numpy(bits.astype(np.uint16).view(np.int16).copy()).view(BF16T)
    assert b.numel() % 2 == 1
    got = ops.cast(b.to(DEV), F32).cpu()
    assert torch.equal(got.view(torch.int32), b.float().view(torch.int32))
    xd = b.to(DEV)
    assert ops.cast(xd, BF16T) is xd
    fd = got.to(DEV)
    assert ops.cast(fd, F32) is fd


# ----------------------------------------------------------------------------- add_act_grad
def _aag_inputs(n, re):
    g = torch.Generator().manual_seed(97 * n + re)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    pre = torch.cat([torch.linspace(-12, 12, n // 2), 2.0 * torch.randn(n - n // 2, generator=g)])
    pre = pre[torch.randperm(n, generator=g)]
    rows = -(-n // re)
    rs = torch.tensor([0.0, 0.5, 2.0])[torch.arange(rows) % 3] + 0.25 * torch.rand(rows, generator=g)
    return a, b, pre, rs


@pytest.mark.parametrize("re", [8, 24, 12])
@pytest.mark.parametrize("n", [8 * 37, 8 * 37 + 3])
def test_add_act_grad(n, re):
    """out = (a [+ b]) [* gelu'(pre)] [* row_scale[i / row_elems]] with b, pre and row_scale each present
    or absent and a, b, pre, out each f32 or bf16, against f64 with the exact erf. n = 296 with
    row_elems 8 or 24 (or no row_scale) takes add_act_grad8_kernel; n = 299, and row_elems = 12 with a
    row_scale, take add_act_grad_kernel. pre holds linspace(-12, 12) as well as randn.

    Measured on an MI355X: the f32 GELU gradient (erff and __expf) stands at 1.3e-7 max(1, |ref|) over
    [-12, 12] (test_activation_modules_over_the_range), inside the 1e-6 bound; the worst err / bound here,
    0.996, is a bf16 output's half ulp."""
    import ops
    a0, b0, p0, rs = _aag_inputs(n, re)
    worst = 0.0
    for hb, hp, hs in itertools.product((False, True), repeat=3):
        for da, db, dp, do in itertools.product((F32, BF16T), repeat=4):
            if (not hb and db == BF16T) or (not hp and dp == BF16T):
                continue  # an absent operand has no dtype
            a, b, p = _exact(a0, da), _exact(b0, db), _exact(p0, dp)
            ref = a.double() + (b.double() if hb else 0.0)
            if hp:
                ref = ref * _gelu_grad(p.double())
            if hs:
                ref = ref * rs.double()[torch.arange(n) // re]
            out = ops.add_act_grad(_put(a, da), _put(b, db) if hb else None, _put(p, dp) if hp else None,
                                   _put(rs) if hs else None, re, out_dtype=do)
            r = _act_ratio(out, ref)
            worst = max(worst, r)
            assert r <= 1.0, (hb, hp, hs, da, db, dp, do, r)
    print(f"add_act_grad n={n} row_elems={re}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("dtype", [F32, BF16T])
@pytest.mark.parametrize("re", [8, 24])
def test_add_act_grad_8wide_and_scalar_agree_bitwise(re, dtype):
    """add_act_grad8_kernel (aligned operands) and add_act_grad_kernel (forced by a 4-byte offset of a)
    on the same data give the same bits."""
    import ops
    n = 8 * 37
    a, b, p, rs = _aag_inputs(n, re)
    args = (_put(b, dtype), _put(p, dtype), _put(rs), re)
    wide = ops.add_act_grad(_put(a, dtype), *args, out_dtype=dtype)
    scalar = ops.add_act_grad(_off(a, dtype), *args, out_dtype=dtype)
    assert torch.equal(wide, scalar)
    wide32 = ops.add_act_grad(_put(a, dtype), *args, out_dtype=F32)
    scalar32 = ops.add_act_grad(_off(a, dtype), *args, out_dtype=F32)
    assert torch.equal(wide32, scalar32)


# ----------------------------------------------------------------------------- standalone activations
@pytest.mark.parametrize("dtype", [F32, BF16T])
@pytest.mark.parametrize("act", ["gelu", "relu"])
def test_activation_modules_over_the_range(act, dtype):
    """layers.GELU / layers.ReLU (ivit_act_fwd / _bwd) forward and backward on linspace(-12, 12, 4801)
    plus +-0 with a random dy: n = 4803, a ragged last workgroup; f32 and bf16."""
    import layers
    x = _exact(torch.cat([torch.linspace(-12, 12, 4801), torch.tensor([0.0, -0.0])]), dtype)
    dy = _exact(torch.randn(x.numel(), generator=torch.Generator().manual_seed(3)), dtype)
    assert x.numel() == 4803
    xd = _put(x, dtype).requires_grad_(True)
    y = (layers.GELU() if act == "gelu" else layers.ReLU())(xd)
    y.backward(_put(dy, dtype))
    x64, dy64 = x.double(), dy.double()
    if act == "gelu":
        yref, gref = _gelu(x64), dy64 * _gelu_grad(x64)
    else:
        yref, gref = x64.clamp_min(0.0), torch.where(x64 > 0, dy64, torch.zeros_like(dy64))
    assert y.dtype == dtype and xd.grad.dtype == dtype
    rf, rb = _act_ratio(y, yref), _act_ratio(xd.grad, gref)
    print(f"act {act} {dtype}: fwd {rf:.3f} bwd {rb:.3f}")
    assert rf <= 1.0 and rb <= 1.0, (rf, rb)


# ----------------------------------------------------------------------------- column sums
def _colsum(x, ld, rowmap, M, N, out, acc):
    from _lib import dt, lib, ptr, stream, workspace
    ws = workspace(lib.ivit_colsum_workspace(M, N), DEV)
    lib.ivit_colsum(ptr(x), dt(x), ld, rowmap[0], rowmap[1], rowmap[2], M, N, ptr(out), acc, ptr(ws), ws.numel(),
                    stream())
    torch.cuda.synchronize()


def _colsum_shapes():
    cs = K["CS_ROWS"]
    return [(1, 35), (cs - 1, 70), (cs + 1, 64), (cs * (16 * K["CR_COLS"] + 1) + 300, 5)]


@pytest.mark.parametrize("dtype", [F32, BF16T])
@pytest.mark.parametrize("M,N", _colsum_shapes())
def test_colsum(M, N, dtype):
    """ivit_colsum on a column slice of a wider tensor (ld = N + 3 > N), accumulate 0 (over a NaN
    pre-fill) and 1; the last shape's partial list runs past colreduce_kernel's first batch. Per column
    |err| <= 1e-5 sum |x|."""
    g = torch.Generator().manual_seed(M + N)
    full = _exact(torch.randn(M, N + 3, generator=g) + 0.25, dtype)
    xd = _put(full, dtype)[:, 2:2 + N]
    x64 = full[:, 2:2 + N].double()
    pre = torch.randn(N, generator=g)
    for acc in (0, 1):
        out = _put(pre) if acc else torch.full((N,), float("nan"), device=DEV)
        _colsum(xd, N + 3, (0, 0, 0), M, N, out, acc)
        ref = x64.sum(0) + (pre.double() if acc else 0.0)
        r = NC.col_ratio(out, ref, x64.abs().sum(0) + (pre.double().abs() if acc else 0.0))
        print(f"colsum ({M},{N}) {dtype} acc={acc}: {r:.3f}")
        assert r <= 1.0, r


@pytest.mark.parametrize("dtype", [F32, BF16T])
def test_colsum_row_map(dtype):
    """The row map (23, 24, 1) with B = 3: the three CLS rows (0, 24, 48), filled with 1e6, stay out."""
    M, N = NC.NECK_B * NC.NECK_NP, 35
    idx = NC.rowmap_index(M, NC.NECK_MAP)
    full = _exact(torch.randn(NC.NECK_B * (NC.NECK_NP + 1), N, generator=torch.Generator().manual_seed(2)), dtype)
    full[torch.arange(NC.NECK_B) * (NC.NECK_NP + 1)] = 1e6
    out = torch.full((N,), float("nan"), device=DEV)
    _colsum(_put(full, dtype), N, NC.NECK_MAP, M, N, out, 0)
    x64 = full[idx].double()
    r = NC.col_ratio(out, x64.sum(0), x64.abs().sum(0))
    assert r <= 1.0, r


# ----------------------------------------------------------------------------- copies and heads
@pytest.mark.parametrize("dtype", [F32, BF16T])
def test_copy_cols_strided_both_sides(dtype):
    """ivit_copy_cols from a column slice into a column slice: bit-exact, and the destination outside
    the copied columns keeps its sentinel."""
    from _lib import dt, lib, ptr, stream
    rows, cols, lds, ldd = 37, 21, 29, 40
    src = _put(torch.randn(rows, lds, generator=torch.Generator().manual_seed(4)), dtype)
    dst = torch.full((rows, ldd), SENTINEL, dtype=dtype, device=DEV)
    sv, dv = src[:, 5:5 + cols], dst[:, 8:8 + cols]
    lib.ivit_copy_cols(ptr(sv), lds, ptr(dv), ldd, rows, cols, dt(sv), stream())
    torch.cuda.synchronize()
    assert torch.equal(dv, sv)
    assert bool((dst[:, :8] == SENTINEL).all()) and bool((dst[:, 8 + cols:] == SENTINEL).all())


@pytest.mark.parametrize("M", [7, 300])
def test_split_and_merge_heads(M):
    """ivit_split_heads / ivit_merge_heads_grad with A = 5, K = 8, ldh = 80: the split is the view /
    permute of heads.py; the merge into f32 is exact with the pad columns 75..79 zero, None for dcls /
    dbox / dint gives zeros in its columns, a bf16 dh is torch's rounding, and merge(split(h)) = h on
    columns 0..74."""
    from _lib import BF16, F32 as CF32, lib, ptr, stream
    A, Kc, ldh = 5, 8, 80
    Cd, Ci = A * 7, A * Kc
    h = torch.randn(M, ldh, generator=torch.Generator().manual_seed(M))
    hd = h.to(DEV)
    cls, box, intent = (torch.full(s, SENTINEL, device=DEV) for s in ((M * A,), (M * A, 6), (M * A, Kc)))
    lib.ivit_split_heads(ptr(hd), ldh, M, A, Kc, ptr(cls), ptr(box), ptr(intent), stream())
    conv = h.t().reshape(1, ldh, M, 1)  # the heads' conv output, NCHW with Hf = M, Wf = 1
    det = conv[:, :Cd].reshape(1, A, 7, M, 1).permute(0, 3, 4, 1, 2).contiguous()
    itn = conv[:, Cd:Cd + Ci].reshape(1, A, Kc, M, 1).permute(0, 3, 4, 1, 2).contiguous()
    assert torch.equal(cls.cpu(), det[..., 0].reshape(M * A))
    assert torch.equal(box.cpu(), det[..., 1:].reshape(M * A, 6))
    assert torch.equal(intent.cpu(), itn.reshape(M * A, Kc))

    def merge(dc, dbx, di, dtype):
        dh = torch.full((M, ldh), SENTINEL, dtype=dtype, device=DEV)
        lib.ivit_merge_heads_grad(ptr(dc), ptr(dbx), ptr(di), M, A, Kc, ptr(dh), ldh, BF16 if dtype == BF16T else CF32,
                                  stream())
        torch.cuda.synchronize()
        return dh.cpu()

    back = merge(cls, box, intent, F32)
    assert torch.equal(back[:, :Cd + Ci], h[:, :Cd + Ci]) and bool((back[:, Cd + Ci:] == 0).all())
    assert torch.equal(merge(cls, box, intent, BF16T), back.to(BF16T))
    j = torch.arange(Cd) % 7
    for drop in range(3):
        parts = [cls, box, intent]
        parts[drop] = None
        want = back.clone()
        if drop == 0:
            want[:, :Cd][:, j == 0] = 0
        elif drop == 1:
            want[:, :Cd][:, j != 0] = 0
        else:
            want[:, Cd:Cd + Ci] = 0
        assert torch.equal(merge(*parts, F32), want), drop
