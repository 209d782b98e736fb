"""The convolution and Linear GEMM kernels (csrc/conv3x3.hip, csrc/thin_conv.hip, csrc/linear.hip) on INTEGER inputs, compared
for EQUALITY with fp64 on the CPU (exact_inputs.py says why any correct kernel gives exactly the fp64 result on them): one
misplaced, dropped, duplicated or stale element anywhere is a failure, at the deep K where the rings wrap and the split-K
slices multiply — what the tolerance tests of test_kernels_gpu.py (max error against tol * max|ref|) cannot see
(test_exact_inputs.py records that gap).  Every launch writes into an output that held NaN before (guarded_alloc's 0xFF
arenas, or an `out=` filled here), so an element that is never stored fails the comparison too.

The only tolerance in this file is on the GEGLU output, which is not an integer (erf): an elementwise bar in ulps of the
storage type, one above what the kernels measured (exact_inputs.GEGLU_MEASURED_ULPS).  What integer inputs do not prove:
rounding behaviour on real-valued data — that stays with test_kernels_gpu.py."""
import ctypes
import time

import pytest
import torch

import exact_inputs as E
from exact_inputs import DT, assert_exact, mismatch_report
from guarded_alloc import guarded

pytestmark = pytest.mark.gpu
NHWC = torch.channels_last


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from guided_attention_amd import ops as _ops
    _ops.load()
    return _ops


def dev(t, T, nhwc=False):
    out = t.to("cuda", T)
    return out.contiguous(memory_format=NHWC) if nhwc else out.contiguous()


def same(got, ref64, what):
    got = got.detach().double().cpu()
    assert torch.equal(got, ref64), mismatch_report(got, ref64, what)


def nan_out(shape, T):
    return torch.full(shape, float("nan"), device="cuda", dtype=T)


def tickets_zero(ops):
    return int(ops.linear_workspace(torch.device("cuda", torch.cuda.current_device()))["tickets"].abs().sum().item()) == 0


def note(what, t0, **figures):
    torch.cuda.synchronize()
    print(f"[measured] {what}: {time.perf_counter() - t0:.2f} s " + " ".join(f"{k} {v}" for k, v in figures.items()))


ids = lambda v: "x".join(map(str, v[0] if isinstance(v[0], tuple) else v)) if isinstance(v, tuple) else str(v)  # noqa: E731


# ------------------------------------------------------------------------------------------------ 3x3 convolution
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("entry", E.CONV_DEEP, ids=ids)
def test_conv3x3_deep_k_is_exact(ops, entry, dt):
    """ga_conv3x3_nhwc on every tile x split-K plan, plain / bias / bias + residual, at depths where each kernel's ring wraps
    several times.  Which kernel a shape is here for (exact_inputs.CONV_DEEP, checked against launch_tile's dispatch by
    test_exact_inputs.py): 1280 / 2560 x 8 x 8, 640 x 16 x 16 (lane_rot = 2), 1 x 640 x 32 x 32: the DMA patch kernel's DEEP
    ring; 5 x 640 x 16 x 16, 2 x 640 x 32 x 32: its 32 KB ring; 24 x 24: the register-staged patch kernel on runs of pixels
    (64-pixel tiles); 48 x 48: its WIDE 13-piece instantiation; 4 x 128: the WIDE DMA instantiation (128-pixel tiles);
    16 x 12: runs of pixels on the DMA form (64-pixel tiles); 12 x 12, 10 x 10, 9 x 7, stride 2: the per-tap kernel.
    Split-K launches are repeated three times (arrival order must not show) and leave every ticket at zero."""
    shape, variant, tiles = entry
    B, Cin, Cout, H, W, stride = shape
    T = DT[dt]
    c = E.conv_case(shape)
    for form, ref in c["refs"].items():
        assert_exact(ref, T, f"{shape} {form}")
    x, res = dev(c["x"], T, True), dev(c["res"], T, True)
    w, bias = dev(c["w"], T), dev(c["bias"], T)
    wp = ops.conv3x3_packed_weights(w, False)
    plans = E.conv_plans(ops.LIN_SLAB_FLOATS, shape)
    assert {p[:2] for p in plans} == set(E.CONV_TILES) and any(p[2] == 16 for p in plans)
    t0 = time.perf_counter()
    with guarded(ops):
        for bm, bn, splits in plans:
            for form in E.CONV_FORMS:
                b, r = {"plain": (None, None), "bias": (bias, None), "bias+residual": (bias, res)}[form]
                for rep in range(3 if splits > 1 and form == "bias+residual" else 1):
                    y = ops.conv3x3_nhwc(x, wp, Cout, stride, b, r, plan=(bm, bn, splits, 0))
                    same(y, c["refs"][form], f"conv {shape} {dt} tile {bm}x{bn} splits {splits} {form} launch {rep} "
                         f"({E.conv_variant(bm, bn, B, H, W, stride, splits, Cout)})")
    assert tickets_zero(ops)
    note(f"conv {shape} {dt} {variant}", t0, launches=sum(5 if p[2] > 1 else 3 for p in plans))


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("shape", E.CONV_AUTOGRAD, ids=ids)
def test_conv3x3_autograd_is_exact(ops, shape, dt):
    """ops.conv3x3 on the planner's own plan: the forward, and dx through the flipped, transposed pack (depth 9 Cout: an
    integer gy at that depth's density gives an integer dx); the residual's gradient is gy itself."""
    B, Cin, Cout, H, W, stride = shape
    T = DT[dt]
    c = E.conv_case(shape)
    assert_exact(c["refs"]["plain"], T, "acc"), assert_exact(c["refs"]["bias"], T, "acc + bias")
    assert_exact(c["refs"]["bias+residual"], T, "y"), assert_exact(c["dx"], T, "dx")
    xa, ra = dev(c["x"], T, True).requires_grad_(True), dev(c["res"], T, True).requires_grad_(True)
    w, bias, gy = dev(c["w"], T).contiguous(memory_format=NHWC), dev(c["bias"], T), dev(c["gy"], T, True)
    t0 = time.perf_counter()
    with guarded(ops):
        y = ops.conv3x3(xa, w, bias, ra, stride)
        same(y, c["refs"]["bias+residual"], f"autograd forward {shape} {dt}")
        y.backward(gy)
        same(xa.grad, c["dx"], f"dx {shape} {dt}")
        assert torch.equal(ra.grad, gy)
        same(ops.conv3x3(xa.detach(), w), c["refs"]["plain"], f"plain forward {shape} {dt}")
    assert tickets_zero(ops)
    note(f"conv autograd {shape} {dt}", t0)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("shape", E.UP_SHAPES, ids=ids)
def test_upsample_conv3x3_is_exact(ops, shape, dt):
    """ga_conv3x3_up2x_nhwc (the patch-DMA kernel gathering from the half-size map) on every tile x split, and the autograd
    wrapper: forward, and backward = the stride-1 backward kernel followed by the 2 x 2 sums of the up-sampling's adjoint
    (sums of four integers: exact in 16 bits while they stay <= 256, which assert_exact checks)."""
    B, Cin, Cout, H, W = shape
    T = DT[dt]
    c = E.up_case(shape)
    for k in ("acc", "y", "g_up", "dx"):
        assert_exact(c[k], T, k)
    x, w, bias, gy = dev(c["x"], T, True), dev(c["w"], T), dev(c["bias"], T), dev(c["gy"], T, True)
    wp = ops.conv3x3_packed_weights(w, False)
    ops._no_fused_upsample.clear()
    t0 = time.perf_counter()
    with guarded(ops):
        for bm, bn, splits in E.conv_plans(ops.LIN_SLAB_FLOATS, (B, Cin, Cout, 2 * H, 2 * W, 1)):
            for b, ref in ((bias, c["y"]), (None, c["acc"])):
                y = ops.conv3x3_up2x_nhwc(x, wp, Cout, b, plan=(bm, bn, splits, 0))
                assert y is not None, f"the fused up-sampling no longer serves {shape} on tile {bm}x{bn}"
                same(y, ref, f"up2x {shape} {dt} tile {bm}x{bn} splits {splits} bias {b is not None}")
        xa = x.clone().requires_grad_(True)
        y = ops.upsample_conv3x3(xa, w, bias)
        same(y, c["y"], f"upsample_conv3x3 forward {shape} {dt}")
        y.backward(gy)
        same(xa.grad, c["dx"], f"upsample_conv3x3 dx {shape} {dt}")
    assert tickets_zero(ops)
    note(f"up2x {shape} {dt}", t0)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("shape", E.GEMM_NT, ids=ids)
def test_gemm_nt_is_exact(ops, shape, dt):
    """ga_gemm_nt (the per-tap convolution kernel as a one-tap convolution): ragged M and N at K = 1280 / 2560, every tile,
    splits 1 and 4, plain / bias / bias + residual."""
    from guided_attention_amd._lib import dtype_code, load, stream_ptr
    M, K, N = shape
    T = DT[dt]
    c = E.gemm_case(shape)
    for k in ("acc", "acc+bias", "acc+bias+res"):
        assert_exact(c[k], T, k)
    x, w, bias, res = dev(c["x"], T), dev(c["w"], T), dev(c["bias"], T), dev(c["res"], T)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    t0 = time.perf_counter()
    for bm, bn in E.CONV_TILES:
        for sp in E.GEMM_NT_SPLITS:
            ws, tickets = ops.splitk_workspace(x.device, M, N, bm, bn, sp)
            for b, r, ref in ((None, None, "acc"), (bias, None, "acc+bias"), (bias, res, "acc+bias+res")):
                for rep in range(3 if sp > 1 and r is not None else 1):
                    y = nan_out((M, N), T)
                    rc = load().ga_gemm_nt(P(x), P(w), P(y), P(ws), P(tickets), P(b), P(r), M, K, N, bm, bn, sp, dtype_code(x),
                                           stream_ptr())
                    assert rc == 0
                    same(y, c[ref], f"gemm_nt {shape} {dt} tile {bm}x{bn} splits {sp} {ref} launch {rep}")
    assert tickets_zero(ops)
    note(f"gemm_nt {shape} {dt}", t0)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("tile", E.CONV_TILES, ids=ids)
@pytest.mark.parametrize("shape", E.CONV_GN, ids=ids)
def test_conv3x3_gn_epilogue_sums_are_exact(ops, shape, tile, dt):
    """ga_conv3x3_nhwc_gn: the per-(image, m tile, group) sums and sums of squares of the stored result + the per-channel
    term, folded over the blocks the way ga_group_norm_apply folds them, equal the integer sums — exactly, since every partial
    stays below 2^24 (asserted on the reference) and f32 adds of such integers do not round in any order."""
    B, Cin, Cout, H, W, groups = shape
    bm, bn = tile
    T = DT[dt]
    c = E.conv_case((B, Cin, Cout, H, W, 1))
    y_ref = c["refs"]["bias+residual"]
    assert_exact(c["refs"]["plain"], T, "acc"), assert_exact(c["refs"]["bias"], T, "acc + bias"), assert_exact(y_ref, T, "y")
    cb64 = E.t64(E.small_ints((B, Cout), 901, -4, 4))
    z = y_ref + cb64[:, :, None, None]
    assert_exact(z, T, "y + channel term")
    cg = Cout // groups
    E.assert_tile_sums_exact(z.permute(0, 2, 3, 1).reshape(B, H * W, Cout), bm, cg, "GroupNorm partials")
    zg = z.reshape(B, groups, -1)
    x, res, w, bias, cb = dev(c["x"], T, True), dev(c["res"], T, True), dev(c["w"], T), dev(c["bias"], T), dev(cb64, T)
    wp = ops.conv3x3_packed_weights(w, False)
    t0 = time.perf_counter()
    with guarded(ops):
        for splits in E.CONV_GN_SPLITS:
            y, made = ops.conv3x3_nhwc(x, wp, Cout, 1, bias, res, plan=(bm, bn, splits, 0), gn=(groups, cb))
            what = f"conv gn {shape} {dt} tile {bm}x{bn} splits {splits}"
            assert made is not None, f"{what}: the epilogue no longer serves this shape"
            same(y, y_ref, what)
            partials, blocks = made
            assert tuple(partials.shape) == (B, blocks, groups, 2)
            folded = partials.double().cpu().sum(1)
            same(folded[..., 0], zg.sum(-1), what + " sums")
            same(folded[..., 1], (zg * zg).sum(-1), what + " sums of squares")
    assert tickets_zero(ops)
    note(f"conv gn {shape} {tile} {dt}", t0)


# ------------------------------------------------------------------------------------------------ thin convolutions
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("shape", E.THIN_SHAPES, ids=ids)
def test_thin_convolutions_are_exact(ops, shape, dt):
    """ga_conv3x3_thin_in (4 -> C) and _out (C -> 4) through ops.conv3x3_thin_apply, forward and backward (each kernel is the
    other's backward), with and without bias; 74 x 112: workgroups that take two segments."""
    B, C, H, W = shape
    T = DT[dt]
    cases = E.thin_case(shape)
    t0 = time.perf_counter()
    for name in ("in", "out"):
        c = cases[name]
        for k in ("acc", "y", "dx"):
            assert_exact(c[k], T, f"thin {name} {k}")
        nhwc_in = name == "out"
        xa = dev(c["x"], T, nhwc_in).requires_grad_(True)
        w, bias, gy = dev(c["w"], T), dev(c["bias"], T), dev(c["gy"], T, not nhwc_in)
        assert ops.conv3x3_thin_supported(xa.detach(), w)
        with guarded(ops):
            y = ops.conv3x3_thin_apply(xa, w, bias)
            same(y, c["y"], f"thin {name} {shape} {dt} forward")
            y.backward(gy)
            same(xa.grad, c["dx"], f"thin {name} {shape} {dt} backward to the input")
            same(ops.conv3x3_thin_apply(xa.detach(), w, None), c["acc"], f"thin {name} {shape} {dt} no bias")
    note(f"thin {shape} {dt}", t0)


# ------------------------------------------------------------------------------------------------ Linear
def geglu_check(y, pre64, dt, what):
    """The only tolerance of this file.  -> the worst elementwise error in ulps of the storage type at the reference."""
    T = DT[dt]
    F_ = pre64.shape[1] // 2
    ref = pre64[:, :F_] * E.gelu64(pre64[:, F_:])
    err = (y.detach().double().cpu() - ref).abs()
    ulps = err / E.ulp(ref, T)
    worst = float(ulps.max())
    print(f"[measured] {what}: GEGLU worst error {worst:.3f} ulps of {dt}, max |ref| {float(ref.abs().max()):.1f}")
    measured = E.GEGLU_MEASURED_ULPS[dt]
    assert measured is not None, "no measured GEGLU bar recorded"
    bar = torch.minimum((measured + 1.0) * E.ulp(ref, T), torch.full_like(ref, E.TOL[dt] * 2 * float(ref.abs().max())))
    bad = err > bar
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} GEGLU outputs beyond {measured} + 1 ulps (worst {worst:.3f}); first "
                                 f"{[tuple(i) for i in bad.nonzero()[:4].tolist()]}")
    return worst


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("shape", E.LIN_SHAPES, ids=ids)
def test_linear_fused_is_exact(ops, shape, dt):
    """ga_linear_fused on every tile / ring pair x splits {1, 2, 5}: no bias, bias, bias + residual (lin_epilogue rounds after
    the bias and again after the residual), rows taken from a column slice of a wider tensor (ldx > K, the neighbouring
    columns non-zero); the row partial sums of the stored result per column tile; the gn= partial sums; GEGLU's pre-activation
    (the h | gate column mapping of the tile) exact and its output within the measured ulps.  Split-K launches are repeated
    and leave every ticket at zero."""
    M, K, N = shape
    T = DT[dt]
    c = E.gemm_case(shape)
    for k in ("acc", "acc+bias", "acc+bias+res"):
        assert_exact(c[k], T, k)
    x, w, bias, res = dev(c["x"], T), dev(c["w"], T), dev(c["bias"], T), dev(c["res"], T)
    wide = torch.full((M, K + 128), 3.0, device="cuda", dtype=T)
    wide[:, 64:64 + K] = x
    xs = wide[:, 64:64 + K]
    y_ref = c["acc+bias+res"]
    gn = E.LIN_GN.get(shape)
    served = 0
    t0 = time.perf_counter()
    with guarded(ops):
        for bm, bn, stages in E.LIN_PLANS:
            E.assert_tile_sums_exact(y_ref[None], bm, bn, "row / GroupNorm partials")
            for splits in E.LIN_SPLITS:
                plan = (bm, bn, splits, stages)
                what = f"linear {shape} {dt} plan {plan}"
                for form, args, ref in (("no bias", (x, w, None, None), "acc"), ("bias", (x, w, bias, None), "acc+bias"),
                                        ("bias+residual", (x, w, bias, res), "acc+bias+res"),
                                        ("sliced rows", (xs, w, bias, None), "acc+bias")):
                    for rep in range(3 if splits > 1 and form == "bias+residual" else 1):
                        y = nan_out((M, N), T)
                        out = ops.linear_fused(*args, plan=plan, out=y)
                        assert out["y"] is y
                        same(y, c[ref], f"{what} {form} launch {rep}")
                # row partial sums of the stored result, per column tile
                out = ops.linear_fused(x, w, bias, residual=res, want_row_partials=True, plan=plan, out=nan_out((M, N), T))
                same(out["y"], y_ref, what + " with row partials")
                parts = -(-N // bn)
                assert tuple(out["row_partials"].shape) == (M, parts, 2)
                padded = torch.nn.functional.pad(y_ref, (0, parts * bn - N)).reshape(M, parts, bn)
                same(out["row_partials"][..., 0], padded.sum(-1), what + " row partial sums")
                same(out["row_partials"][..., 1], (padded * padded).sum(-1), what + " row partial sums of squares")
                if gn is not None:
                    groups, hw = gn
                    out = ops.linear_fused(x, w, bias, residual=res, plan=plan, gn=gn, out=nan_out((M, N), T))
                    same(out["y"], y_ref, what + " with gn")
                    blocks = ops.load().ga_linear_gn_blocks(hw, N, groups, bm, bn)
                    assert (out["gn"] is not None) == bool(blocks)
                    if blocks:
                        served += 1
                        partials, nb = out["gn"]
                        assert nb == blocks and tuple(partials.shape) == (M // hw, blocks, groups, 2)
                        yg = y_ref.reshape(M // hw, hw, groups, N // groups)
                        folded = partials.double().cpu().sum(1)
                        same(folded[..., 0], yg.sum((1, 3)), what + " gn sums")
                        same(folded[..., 1], (yg * yg).sum((1, 3)), what + " gn sums of squares")
                if N % 16 == 0:
                    out = ops.linear_fused(x, w, bias, geglu=True, want_preact=True, plan=plan, out=nan_out((M, N // 2), T))
                    same(out["preact"], c["acc+bias"], what + " geglu preact")
                    geglu_check(out["y"], c["acc+bias"], dt, what + " geglu")
                    y2 = ops.linear_fused(x, w, bias, geglu=True, plan=plan, out=nan_out((M, N // 2), T))["y"]
                    assert torch.equal(y2, out["y"]), what + ": GEGLU with and without the pre-activation copy differ"
    assert gn is None or served >= 1
    assert tickets_zero(ops)
    note(f"linear {shape} {dt}", t0)


def f32_ulps(got, ref64):
    """|got - ref| in f32 ulps at ref (ref a power of two here)."""
    return float(((got.double().cpu() - ref64).abs() / (ref64.abs() * 2.0 ** -23)).max())


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("shape", E.LIN_SHAPES, ids=ids)
def test_linear_layernorm_fold_is_exact(ops, shape, dt):
    """The LayerNorm fold rstd (acc - mean colsum) + shift on FABRICATED row statistics (exact_inputs.ln_case: the test writes
    the partial sums itself; mean in {-2 .. 2}, rstd 1 or 2 up to an f32 ulp): the result is an integer — the ulp of rstd moves
    the f32 value by less than 1e-3 and the conversion to the storage type removes that, except at a result of 0, which
    ln_case keeps out of the rows whose rstd is not exact — so the row-statistics, colsum and shift indexing is checked
    exactly, on every tile / ring pair and split.  want_ln_stats: the mean exact, rstd within 4 f32 ulps."""
    M, K, N = shape
    T = DT[dt]
    c = E.ln_case(shape, E.LN_PARTS)
    assert_exact(c["acc"], T, "acc"), assert_exact(c["ref"], T, "LayerNorm-fold result")
    x, w = dev(c["x"], T), dev(c["w"], T)
    partials, colsum, shift = dev(c["partials"], torch.float32), dev(c["colsum"], torch.float32), dev(c["shift"], torch.float32)
    worst = 0.0
    t0 = time.perf_counter()
    with guarded(ops):
        for bm, bn, stages in E.LIN_PLANS:
            for splits in E.LIN_SPLITS:
                plan = (bm, bn, splits, stages)
                what = f"LayerNorm fold {shape} {dt} plan {plan}"
                out = ops.linear_fused(x, w, None, ln=(partials, colsum, shift, E.LN_EPS), want_ln_stats=True, plan=plan,
                                       out=nan_out((M, N), T))
                same(out["y"], c["ref"], what)
                same(out["ln_stats"][:, 0], c["mean"], what + " mean")
                worst = max(worst, f32_ulps(out["ln_stats"][:, 1], c["rstd"]))
                assert worst <= 4.0, f"{what}: rstd {worst} f32 ulps from 1 or 2"
                y2 = ops.linear_fused(x, w, None, ln=(partials, colsum, shift, E.LN_EPS), plan=plan, out=nan_out((M, N), T))["y"]
                same(y2, c["ref"], what + " without the statistics output")
    assert tickets_zero(ops)
    note(f"LayerNorm fold {shape} {dt}", t0, rstd_ulps=worst)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("case", E.STREAM_CASES, ids=ids)
def test_linear_stream_form_is_exact(ops, case, dt):
    """linear_stream_kernel (plan = ops.LINEAR_STREAM_PLAN) through the same fabricated statistics, 2 / 3 / 20 partial sums per
    row: ragged M and N; one tile or fewer per workgroup; 320 tiles on 256 workgroups, so that some workgroups take two tiles
    and the ring streams across a tile boundary.  Equal to the reference and to the per-tile kernel on the same call."""
    shape, parts = case
    M, K, N = shape
    T = DT[dt]
    c = E.ln_case(shape, parts)
    assert_exact(c["acc"], T, "acc"), assert_exact(c["ref"], T, "LayerNorm-fold result")
    assert ops.linear_stream_serves(K, parts, True, None, None, False, False, False)
    x, w = dev(c["x"], T), dev(c["w"], T)
    ln = (dev(c["partials"], torch.float32), dev(c["colsum"], torch.float32), dev(c["shift"], torch.float32), E.LN_EPS)
    t0 = time.perf_counter()
    with guarded(ops):
        for rep in range(2):
            y = nan_out((M, N), T)
            assert ops.linear_fused(x, w, None, ln=ln, plan=ops.LINEAR_STREAM_PLAN, out=y)["y"] is y
            same(y, c["ref"], f"stream form {shape} {dt} {parts} partial sums per row, launch {rep}")
        tile = ops.linear_fused(x, w, None, ln=ln, plan=(128, 128, 1, 3), out=nan_out((M, N), T))["y"]
        same(tile, c["ref"], f"per-tile kernel {shape} {dt}")
        assert torch.equal(tile, y)
    note(f"stream {shape} {dt}", t0)
