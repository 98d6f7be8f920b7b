"""The convolution kernels op by op on inputs whose answer has no rounding (tests/conv_cases.py): every
f32 output must equal the f64 reference (torch.equal) and every bf16 output its round-to-nearest-even,
bit for bit, whatever kernel, tile or split the dispatch picks. The only tolerances are the two of the
BatchNorm statistics of ivit_conv_bn_fwd, which run on Gaussian data.

Paths and the tests that reach them (conv_cases.coverage() lists the cases per path and edge):
  ivit_conv_fwd          conv_panel_kernel, the engine on LdConv's DMA and gather loaders, the f32 engine:
                         test_conv_exact (both settings of IVIT_KNOB_CONV_PANEL), test_conv_fwd_into_column_slice
  ivit_conv_dgrad / _t   test_conv_exact, test_head_dgrad_exact, test_conv_grads_read_dy_from_column_slice
  ivit_conv_wgrad        conv_wgrad_panel_kernel and the engine with its split-K: test_conv_exact,
                         test_conv_wgrad_accumulates
  packs                  test_conv_exact, test_pack_conv_pair
  ivit_conv_bn_fwd       test_conv_bn_fwd, test_conv_bn_fwd_large_offset
  ivit_im2col / _col2im  test_im2col, test_im2col_rejects, test_col2im, test_col2im_order, test_strided_conv_exact
"""
import functools

import pytest
import torch

import conv_cases as CC

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32T, BF16T = torch.float32, torch.bfloat16
NAN = float("nan")


def _set_knob(request, value):
    from _lib import KNOB_CONV_PANEL, lib
    lib.ivit_set_knob(KNOB_CONV_PANEL, value)
    request.addfinalizer(lambda: lib.ivit_set_knob(KNOB_CONV_PANEL, 1))


def _cd(c):
    from _lib import BF16, F32
    return (BF16T, BF16) if c.dtype == "bf16" else (F32T, F32)


def _exact(got, ref):
    """f32: equal to the f64 reference; bf16: the bits of its round-to-nearest-even."""
    if got.dtype == BF16T:
        return CC.same_bits(got, CC.rne_bf16(ref).reshape(got.shape))
    return torch.equal(got.detach().cpu().double().reshape(ref.shape), ref)


@functools.lru_cache(maxsize=None)
def _dev(name):
    """A case's operands on the device in its compute dtype: uploaded once, left unchanged."""
    c = CC.head_case() if name == "head" else CC.conv_case(name)
    cd, _ = _cd(c)
    d = {"w": c.w.to(DEV), "dy": c.dy.to(cd).to(DEV)}
    if name != "head":
        d.update(x=c.x.to(cd).to(DEV), dyw=c.dyw.to(cd).to(DEV), bias=c.bias.to(DEV))
    return d


def _outs(c):
    return (F32T, BF16T) if c.dtype == "bf16" else (F32T,)


def _run_all(c, d, knob, t_packs):
    """Every stride-1 op of one case under the current knob; returns what failed. t_packs: the list
    the spy on ops.pack_conv_t appends to."""
    import ops
    from _lib import dt, lib, ptr, stream
    cd, cdt = _cd(c)
    B, H, W, M = c.B, c.H, c.W, c.M
    bad = []
    wp = ops.pack_conv(d["w"], cdt)
    if not CC.same_bits(wp, CC.pack_ref(c.w).to(cd)):
        bad.append("pack_conv")
    for od in _outs(c):
        for bias, ref in ((d["bias"], c.ref["y"]), (None, c.ref["y0"])):
            if not _exact(ops.conv_fwd(d["x"], B, H, W, wp, bias, cdt, od), ref):
                bad.append(f"fwd {od} bias={bias is not None}")
        if not _exact(ops.conv_dgrad(d["dy"], B, H, W, wp, cdt, od), c.ref["dx"]):
            bad.append(f"dgrad engine {od}")
        # with w= ops.conv_dgrad must take ivit_conv_dgrad_t exactly where the mirror says (it packs the
        # transposed weight on that branch only), and the entry point is also called directly
        want_t = CC.dgrad_t_ok(c.dtype, M, c.Cin, c.Cout, c.Cout, c.k, knob)
        n0 = len(t_packs)
        if not _exact(ops.conv_dgrad(d["dy"], B, H, W, wp, cdt, od, w=d["w"]), c.ref["dx"]):
            bad.append(f"dgrad w= {od}")
        if (len(t_packs) > n0) != want_t:
            bad.append(f"dgrad w= {od}: panel taken {len(t_packs) > n0}, mirror {want_t}")
        if CC.dgrad_t_ok(c.dtype, M, c.Cin, c.Cout, c.Cout, c.k):  # the entry point ignores the knob
            dx = torch.full((M, c.Cin), NAN, dtype=od, device=DEV)
            lib.ivit_conv_dgrad_t(cdt, ptr(d["dy"]), c.Cout, B, H, W, c.Cout, ptr(ops.pack_conv_t(d["w"], cdt)), c.Cin,
                                  c.k, ptr(dx), dt(dx), stream())
            if not _exact(dx, c.ref["dx"]):
                bad.append(f"ivit_conv_dgrad_t {od}")
    wt = ops.pack_conv_t(d["w"], cdt)
    if not CC.same_bits(wt, CC.pack_t_ref(c.w).to(cd)):
        bad.append("pack_conv_t")
    gp, db = ops.conv_wgrad(d["dyw"], d["x"], B, H, W, c.Cin, c.Cout, c.k, cdt, want_bias=True)
    if not torch.equal(gp.cpu().double(), CC.pack_ref(c.ref["dw"])):
        bad.append("wgrad (packed)")
    if not _exact(ops.unpack_conv_grad(gp, c.Cout, c.Cin, c.k), c.ref["dw"]):
        bad.append("unpack_conv_grad")
    if not _exact(db, c.ref["db"]):
        bad.append("dbias")
    gp2, none = ops.conv_wgrad(d["dyw"], d["x"], B, H, W, c.Cin, c.Cout, c.k, cdt)
    if none is not None or not torch.equal(gp2, gp):
        bad.append("wgrad without bias")
    return bad


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_conv_exact(name, request, monkeypatch):
    """Forward (f32 and bf16 output, with and without bias), data gradient (engine, and the panel on
    the transposed pack where it admits the shape), weight and bias gradient and the packs of one case;
    a bf16 case the panel admits for any of them runs under both settings of the knob."""
    c, d = CC.conv_case(name), _dev(name)
    knobs = (1, 0) if any(p.endswith(("panel", "panel_t")) for p in CC.paths(name)) else (1,)
    import ops
    bad, t_packs, pack_t = [], [], ops.pack_conv_t
    monkeypatch.setattr(ops, "pack_conv_t", lambda *a, **kw: (t_packs.append(1), pack_t(*a, **kw))[1])
    for knob in knobs:
        _set_knob(request, knob)
        bad += [f"knob {knob}: {b}" for b in _run_all(c, d, bool(knob), t_packs)]
    assert not bad, (name, sorted(CC.paths(name)), bad)


def test_head_dgrad_exact(request, monkeypatch):
    """The head's data gradient: 75 channels, forward pack padded to 80, dy zero-padded to 128 channels
    (lddy = 128) - the panel on the transposed pack padded to 128, and the engine reading 80 channels."""
    import ops
    from _lib import BF16
    h, d = CC.head_case(), _dev("head")
    wp = ops.pack_conv(d["w"], BF16, cout_pad=h.Cp)
    assert CC.same_bits(wp, CC.pack_ref(h.w, h.Cp).bfloat16())
    assert CC.same_bits(ops.pack_conv_t(d["w"], BF16, cout_pad=h.Cq), CC.pack_t_ref(h.w, h.Cq).bfloat16())
    t_packs, pack_t = [], ops.pack_conv_t
    monkeypatch.setattr(ops, "pack_conv_t", lambda *a, **kw: (t_packs.append(1), pack_t(*a, **kw))[1])
    for knob in (1, 0):
        _set_knob(request, knob)
        for od in (F32T, BF16T):
            n0 = len(t_packs)
            assert _exact(ops.conv_dgrad(d["dy"], h.B, h.H, h.W, wp, BF16, od, w=d["w"], dy_zero_pad=True),
                          h.ref["dx"]), (knob, od)
            assert (len(t_packs) > n0) == bool(knob)  # the panel on the pack padded to 128 iff the knob is on
            assert _exact(ops.conv_dgrad(d["dy"], h.B, h.H, h.W, wp, BF16, od), h.ref["dx"]), (knob, od)


@pytest.mark.parametrize("name", ["m289_k1", "m128_g", "m129_f"])
def test_pack_conv_pair(name):
    import ops
    c, d = CC.conv_case(name), _dev(name)
    cd, cdt = _cd(c)
    C0 = c.Cout // 2 + 1
    got = ops.pack_conv_pair(d["w"][:C0].contiguous(), d["w"][C0:].contiguous(), cdt, c.Cout + 8)
    assert CC.same_bits(got, CC.pack_ref(c.w, c.Cout + 8).to(cd))


def test_wgrad_split_mirror_holds_on_the_device():
    """The engine's split-K choice depends on the CU count: the mirror's (and with it the coverage
    table's "more than one split" cases) is the device's, and the workspace size agrees."""
    from _lib import lib
    assert 2 * torch.cuda.get_device_properties(0).multi_processor_count == CC.ENGINE_SLOTS
    for name in ("border37_f_k5", "border5_f_k5", "empty_split", "m129_f", "m128_g"):
        g = CC._geom(name)
        s = CC.wgrad_workspace_splits(g.M, g.Cout, g.K)
        assert lib.ivit_conv_wgrad_workspace(g.B, g.H, g.W, g.Cin, g.Cout, g.k) == \
            s * g.Cout * g.K * 4 + max(s * g.Cout * 4, lib.ivit_colsum_workspace(g.M, g.Cout)), name
    assert CC.wgrad_engine_splits(333, 8, 200, False) > 1 and CC.wgrad_engine_splits(1600, 128, 144, True) > 1


# ----------------------------------------------------------------------------- the ABI's strides and accumulate
ABI_CASES = ["m289_k3", "m129_d", "m129_f"]  # panel (and the engine with the knob off), bf16 engine, f32 engine


def _slice(t, width, fill, off=0):
    """t [M, C] as columns off .. off + C - 1 of a [M, width] buffer filled with ``fill``."""
    buf = torch.full((t.shape[0], width), fill, dtype=t.dtype, device=DEV)
    if t.numel():
        buf[:, off:off + t.shape[1]] = t
    return buf


@pytest.mark.parametrize("name", ABI_CASES)
def test_conv_fwd_into_column_slice(name, request):
    """ivit_conv_fwd with ldy = Cout + 8: exact inside the column slice, the NaN outside untouched."""
    import ops
    from _lib import dt, lib, ptr, stream
    c, d = CC.conv_case(name), _dev(name)
    _, cdt = _cd(c)
    wp = ops.pack_conv(d["w"], cdt)
    for knob in ((1, 0) if c.dtype == "bf16" else (1,)):
        _set_knob(request, knob)
        assert CC.fwd_path(c.dtype, c.M, c.Cin, c.Cout, c.k, bool(knob), c.Cout + 8) == \
            CC.fwd_path(c.dtype, c.M, c.Cin, c.Cout, c.k, bool(knob))
        for od in _outs(c):
            for off in (0, 8):
                buf = torch.full((c.M, c.Cout + 8), NAN, dtype=od, device=DEV)
                y = buf[:, off:]
                lib.ivit_conv_fwd(cdt, ptr(d["x"]), c.B, c.H, c.W, c.Cin, ptr(wp), ptr(d["bias"]), c.Cout, c.k, ptr(y),
                                  c.Cout + 8, dt(buf), stream())
                assert _exact(buf[:, off:off + c.Cout].contiguous(), c.ref["y"]), (knob, od, off)
                rest = torch.cat([buf[:, :off], buf[:, off + c.Cout:]], dim=1)
                assert bool(torch.isnan(rest).all()), (knob, od, off)


@pytest.mark.parametrize("name", ABI_CASES)
def test_conv_grads_read_dy_from_column_slice(name, request):
    """ivit_conv_dgrad, ivit_conv_dgrad_t and ivit_conv_wgrad with lddy = Cout + 8; the 8 columns past
    Cout hold 7, which any of the sums would show."""
    import ops
    from _lib import dt, lib, ptr, stream, workspace
    c, d = CC.conv_case(name), _dev(name)
    _, cdt = _cd(c)
    ld = c.Cout + 8
    wp = ops.pack_conv(d["w"], cdt)
    dy, dyw = _slice(d["dy"], ld, 7.0), _slice(d["dyw"], ld, 7.0)
    for knob in ((1, 0) if c.dtype == "bf16" else (1,)):
        _set_knob(request, knob)
        for od in _outs(c):
            dx = torch.full((c.M, c.Cin), NAN, dtype=od, device=DEV)
            lib.ivit_conv_dgrad(cdt, ptr(dy), ld, c.B, c.H, c.W, c.Cout, ptr(wp), c.Cin, c.k, ptr(dx), dt(dx), stream())
            assert _exact(dx, c.ref["dx"]), (knob, od)
            if CC.dgrad_t_ok(c.dtype, c.M, c.Cin, c.Cout, ld, c.k, bool(knob)):
                wt = ops.pack_conv_t(d["w"], cdt)
                dx.fill_(NAN)
                lib.ivit_conv_dgrad_t(cdt, ptr(dy), ld, c.B, c.H, c.W, c.Cout, ptr(wt), c.Cin, c.k, ptr(dx), dt(dx),
                                      stream())
                assert _exact(dx, c.ref["dx"]), (knob, od, "dgrad_t")
        gp = torch.full((c.Cout, c.k, c.k, c.Cin), NAN, device=DEV)
        db = torch.full((c.Cout,), NAN, device=DEV)
        ws = workspace(lib.ivit_conv_wgrad_workspace(c.B, c.H, c.W, c.Cin, c.Cout, c.k), DEV)
        lib.ivit_conv_wgrad(cdt, ptr(dyw), ld, ptr(d["x"]), c.B, c.H, c.W, c.Cin, c.Cout, c.k, ptr(gp), ptr(db), 0,
                            ptr(ws), ws.numel(), stream())
        assert torch.equal(gp.cpu().double(), CC.pack_ref(c.ref["dw"])), knob
        assert _exact(db, c.ref["db"]), knob


@pytest.mark.parametrize("name", ABI_CASES)
def test_conv_wgrad_accumulates(name, request):
    """accumulate = 1 in ivit_conv_wgrad (dWp and dbias) and ivit_unpack_conv_grad, onto integer-valued
    priors: prior + reference, exactly (|prior| <= 8 stays inside the case's budget of 2^24 units)."""
    from _lib import lib, ptr, stream, workspace
    c, d = CC.conv_case(name), _dev(name)
    _, cdt = _cd(c)
    g = torch.Generator().manual_seed(99)
    p_gp = torch.randint(-8, 9, (c.Cout, c.k, c.k, c.Cin), generator=g).float()
    p_db = torch.randint(-8, 9, (c.Cout,), generator=g).float()
    p_dw = torch.randint(-8, 9, tuple(c.w.shape), generator=g).float()
    assert c.budget["dw"] + 8 * 512 < CC.LIMIT and c.budget["db"] + 8 * 512 < CC.LIMIT
    for knob in ((1, 0) if c.dtype == "bf16" else (1,)):
        _set_knob(request, knob)
        gp, db = p_gp.to(DEV), p_db.to(DEV)
        ws = workspace(lib.ivit_conv_wgrad_workspace(c.B, c.H, c.W, c.Cin, c.Cout, c.k), DEV)
        lib.ivit_conv_wgrad(cdt, ptr(d["dyw"]), c.Cout, ptr(d["x"]), c.B, c.H, c.W, c.Cin, c.Cout, c.k, ptr(gp), ptr(db),
                            1, ptr(ws), ws.numel(), stream())
        assert torch.equal(gp.cpu().double(), p_gp.double() + CC.pack_ref(c.ref["dw"])), knob
        assert torch.equal(db.cpu().double(), p_db.double() + c.ref["db"]), knob
    src = CC.pack_ref(c.ref["dw"]).float().to(DEV)
    out = p_dw.to(DEV)
    lib.ivit_unpack_conv_grad(ptr(src), c.Cout, c.Cin, c.k, ptr(out), 1, stream())
    assert torch.equal(out.cpu().double(), p_dw.double() + c.ref["dw"])


# ----------------------------------------------------------------------------- conv + BatchNorm statistics
def _conv_bn(shape, inputs):
    """-> y (stored), {name: got}, the f64 reference of the stored y, y of ivit_conv_fwd."""
    import ops
    from _lib import BF16
    B, H, W, Cin, Cout, k, ybf = shape
    x, w, rm, rv = inputs(B, H, W, Cin, Cout, k)
    xh = x.bfloat16().to(DEV)
    wp = ops.pack_conv(w.to(DEV), BF16)
    od = BF16T if ybf else F32T
    rm1, rv1 = rm.to(DEV), rv.to(DEV)
    y1, st = ops.conv_bn_fwd(xh, B, H, W, wp, BF16, od, rm1, rv1, True)
    y0 = ops.conv_fwd(xh, B, H, W, wp, None, BF16, od)
    got = {"mean": st.mean, "invstd": st.invstd, "rm": rm1, "rv": rv1}
    return y1, got, CC.bn_stats_ref(y1, rm, rv, 0.1, 1e-5), y0


@pytest.mark.parametrize("tag", sorted(CC.BN_SHAPES))
def test_conv_bn_fwd(tag):
    """ivit_conv_bn_fwd at a ragged channel tile (136, 384), a one-row last pixel tile (M = 289), the
    all-border map, a bf16 y and one fallback shape: y is ivit_conv_fwd's, the statistics are those of
    the stored y in f64 and the running updates follow the formula, at test_conv_bn_stats_fused's bar."""
    shape = CC.BN_SHAPES[tag]
    B, H, W, Cin, Cout, k, _ = shape
    assert CC.fwd_path("bf16", B * H * W, Cin, Cout, k) == ("engine_gather" if tag == "fallback" else "panel")
    y1, got, ref, y0 = _conv_bn(shape, CC.bn_inputs)
    assert CC.same_bits(y1, y0)
    errs = {n: CC.rel(got[n], ref[n]) for n in got}
    print(tag, errs)
    assert all(e < CC.BN_TOL for e in errs.values()), (tag, errs)


def test_conv_bn_fwd_large_offset():
    """Channel means about 100 standard deviations (a one-pass variance would lose it): the bar is
    max(1e-5, 4 * e_torch), e_torch the error of torch's own f32 CPU statistics of the same stored y."""
    y1, got, ref, y0 = _conv_bn(CC.BN_OFFSET_SHAPE, CC.bn_offset_inputs)
    assert CC.same_bits(y1, y0)
    assert float((ref["mean"].abs() * ref["invstd"]).median()) > 80
    t32 = CC.bn_stats_torch_f32(y1, 1e-5)
    e_torch = {n: CC.rel(t32[n], ref[n]) for n in t32}
    bar = {"mean": max(CC.BN_TOL, 4 * e_torch["mean"]), "invstd": max(CC.BN_TOL, 4 * e_torch["invstd"])}
    bar["rm"], bar["rv"] = bar["mean"], bar["invstd"]
    errs = {n: CC.rel(got[n], ref[n]) for n in got}
    print("e_torch", e_torch, "kernel", errs, "ratio", {n: errs[n] / bar[n] for n in errs})
    assert all(errs[n] < bar[n] for n in errs), (errs, bar, e_torch)


# ----------------------------------------------------------------------------- im2col / col2im
PAIRS = {"f32-f32": (F32T, F32T), "f32-bf16": (F32T, BF16T), "bf16-bf16": (BF16T, BF16T)}


def _code(t):
    from _lib import BF16, F32
    return BF16 if t == BF16T else F32


@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("geom", CC.COLS_GEOMS, ids=lambda g: "k%ds%dp%d" % g)
def test_im2col(geom, pair):
    """Every element of a NaN-filled cols is written: the copy of the reference (round to nearest even
    where f32 goes to bf16) and +0 in the pad columns."""
    from _lib import lib, ptr, stream
    k, s, p = geom
    ti, to = PAIRS[pair]
    B = CC.COLS_B
    for H, W in CC.COLS_MAPS:
        if CC.out_size(H, W, k, s, p) is None:
            continue
        Ho, Wo = CC.out_size(H, W, k, s, p)
        for C in CC.COLS_CS:
            x = CC.cols_x(B, H, W, C).to(ti)
            ref = CC.im2col_ref(x.float(), k, s, p).float().to(to)  # torch's CPU rounding
            xd = x.to(DEV)
            K = k * k * C
            for ldc in CC.ldcs(K):
                cols = torch.full((B * Ho * Wo, ldc), NAN, dtype=to, device=DEV)
                lib.ivit_im2col(_code(ti), ptr(xd), B, H, W, C, k, s, p, Ho, Wo, ptr(cols), ldc, _code(to), stream())
                want = torch.zeros(B * Ho * Wo, ldc, dtype=to)
                want[:, :K] = ref
                assert CC.same_bits(cols, want), (H, W, C, ldc)


def test_im2col_rejects():
    """bf16 -> f32, a wrong Ho / Wo, ldc < K and a padded map smaller than the kernel return a
    negative code and write nothing."""
    from _lib import BF16, F32, lib, ptr, stream
    dll = lib.load()
    B, H, W, C, k, s, p = 2, 7, 10, 8, 3, 2, 1
    Ho, Wo = CC.out_size(H, W, k, s, p)
    K = k * k * C
    x16 = torch.zeros(B, H, W, C, dtype=BF16T, device=DEV)
    x32 = torch.zeros(B, H, W, C, device=DEV)
    cols = torch.full((B * Ho * Wo, K + 8), NAN, device=DEV)
    st = stream()
    assert dll.ivit_im2col(BF16, ptr(x16), B, H, W, C, k, s, p, Ho, Wo, ptr(cols), K, F32, st) < 0
    assert dll.ivit_im2col(F32, ptr(x32), B, H, W, C, k, s, p, Ho + 1, Wo, ptr(cols), K, F32, st) < 0
    assert dll.ivit_im2col(F32, ptr(x32), B, H, W, C, k, s, p, Ho, Wo - 1, ptr(cols), K, F32, st) < 0
    assert dll.ivit_im2col(F32, ptr(x32), B, H, W, C, k, s, p, Ho, Wo, ptr(cols), K - 1, F32, st) < 0
    assert dll.ivit_im2col(F32, ptr(x32), B, 1, 1, C, 2, 2, 0, 1, 1, ptr(cols), 4 * C, F32, st) < 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(cols).all())


@pytest.mark.parametrize("geom", CC.COLS_GEOMS, ids=lambda g: "k%ds%dp%d" % g)
def test_col2im(geom):
    """dX (NaN-filled beforehand) equals F.fold in f64 on integer dcols, pixels no window covers
    included (0); the pad columns of dcols hold NaN and must not be read."""
    from _lib import lib, ptr, stream
    k, s, p = geom
    B = CC.COLS_B
    g = torch.Generator().manual_seed(17)
    for H, W in CC.COLS_MAPS:
        if CC.out_size(H, W, k, s, p) is None:
            continue
        Ho, Wo = CC.out_size(H, W, k, s, p)
        for C in CC.COLS_CS:
            K = k * k * C
            for ldc in CC.ldcs(K):
                d = torch.full((B * Ho * Wo, ldc), NAN)
                d[:, :K] = torch.randint(-8, 9, (B * Ho * Wo, K), generator=g).float()
                dd = d.to(DEV)
                dx = torch.full((B, H, W, C), NAN, device=DEV)
                lib.ivit_col2im(ptr(dd), ldc, B, H, W, C, k, s, p, Ho, Wo, ptr(dx), stream())
                assert torch.equal(dx.cpu().double(), CC.col2im_ref(d, B, H, W, C, k, s, p)), (H, W, C, ldc)


def test_col2im_order_and_channel_limit():
    """One Gaussian case bit-equal to the f32 sum in the documented order (ky, then kx ascending);
    C = 513 returns IVIT_ERR_ARG and writes nothing."""
    from _lib import lib, ptr, stream
    B, H, W, C, k, s, p = 2, 7, 10, 65, 5, 1, 2
    Ho, Wo = CC.out_size(H, W, k, s, p)
    d = torch.randn(B * Ho * Wo, k * k * C, generator=torch.Generator().manual_seed(23))
    dx = torch.full((B, H, W, C), NAN, device=DEV)
    lib.ivit_col2im(ptr(d.to(DEV)), k * k * C, B, H, W, C, k, s, p, Ho, Wo, ptr(dx), stream())
    assert CC.same_bits(dx, CC.col2im_ordered_f32(d, B, H, W, C, k, s, p))
    assert CC.rel(dx, CC.col2im_ref(d, B, H, W, C, k, s, p)) < 1e-6
    C = 513
    dd = torch.zeros(B * 4 * 4, C, device=DEV)
    dx = torch.full((B, 4, 4, C), NAN, device=DEV)
    assert lib.load().ivit_col2im(ptr(dd), C, B, 4, 4, C, 1, 1, 0, 4, 4, ptr(dx), stream()) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx).all())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("i", range(len(CC.STRIDED)))
def test_strided_conv_exact(i, dtype):
    """layers.Conv2d on its im2col + GEMM path (_ConvColsFn), forward and backward: y, dx, dw and db
    equal the f64 reference of nn.Conv2d's geometry."""
    import layers
    c = CC.strided_case(i, dtype)
    conv = layers.Conv2d(c.C, c.Cout, c.k, stride=c.s, padding=c.p)
    with torch.no_grad():
        conv.weight.copy_(c.w)
        conv.bias.copy_(c.bias)
    conv.compute_dtype = BF16T if dtype == "bf16" else F32T
    conv = conv.to(DEV)
    x = c.x.to(DEV).requires_grad_(True)
    y = conv(x)
    (dx,) = torch.autograd.grad(y, x, c.dy.to(DEV), retain_graph=True)
    dw, db = torch.autograd.grad(y, (conv.weight, conv.bias), c.dyw.to(DEV))  # f32: a dy that is not bf16-exact
    got = {"y": y.detach(), "dx": dx, "dw": dw, "db": db}
    bad = [n for n, t in got.items() if not torch.equal(t.cpu().double(), c.ref[n])]
    assert not bad, bad
