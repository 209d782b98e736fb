"""CPU side of the exact GEMM tests (test_gemm_exact_gpu.py): the integer generators, the assert_exact precondition over every
case list the GPU file runs (imported, so the two files cannot drift apart), the kernel variant each convolution shape is
listed for, and — as a test — the gap the exact tests close: faults of a ring-slot or piece-index error's footprint that the
tolerance bars of test_kernels_gpu.py accept and equality on integer inputs rejects."""
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import exact_inputs as E
import hashrand
from exact_inputs import DT, assert_exact

PROFILE = Path(__file__).resolve().parent.parent / "profiles" / "gemm_exact.json"


# ------------------------------------------------------------------------------------------------ generators and checks
def test_generators_are_deterministic_integers_of_the_stated_density():
    a, b = E.ternary((3, 1000, 7), 11, 0.4), E.ternary((3, 1000, 7), 11, 0.4)
    assert a.dtype == np.float64 and np.array_equal(a, b) and not np.array_equal(a, E.ternary((3, 1000, 7), 12, 0.4))
    assert set(np.unique(a)) == {-1.0, 0.0, 1.0}
    assert abs(np.abs(a).mean() - 0.4) < 0.02 and abs(a.mean()) < 0.02
    assert set(np.unique(E.ternary((5000,), 3, 1.0))) == {-1.0, 1.0}
    s = E.small_ints((4, 5000), 5)
    assert np.array_equal(s, E.small_ints((4, 5000), 5)) and set(np.unique(s)) == set(float(v) for v in range(-8, 9))
    assert set(np.unique(E.small_ints((5000,), 6, -2, 2))) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    for K in (36, 576, 1280, 5760, 23040):
        d = E.density(K)
        assert 0 < d <= 1 and K * d * d <= 900 * (1 + 1e-12) and K * d * E.partner_density(K, d) <= 900 * (1 + 1e-12)
    assert E.density(36) == 1.0 and E.partner_density(2880, 1.0) == 900 / 2880


def test_assert_exact_is_a_precondition_that_rejects():
    ok = torch.tensor([-256.0, -3.0, 0.0, 255.0, 256.0], dtype=torch.float64)
    for T in DT.values():
        assert assert_exact(ok, T) == 256.0
    with pytest.raises(AssertionError):
        assert_exact(torch.tensor([257.0], dtype=torch.float64), torch.bfloat16)     # does not survive bf16
    with pytest.raises(AssertionError):
        assert_exact(torch.tensor([258.0], dtype=torch.float64), torch.float16)      # survives f16, above the limit
    with pytest.raises(AssertionError):
        assert_exact(torch.tensor([100.03], dtype=torch.float64), torch.float16)
    with pytest.raises(AssertionError):
        E.assert_f32_sums_exact(torch.full((2 ** 12 + 1,), 64.0, dtype=torch.float64))
    E.assert_f32_sums_exact(torch.full((2 ** 12 - 1,), 64.0, dtype=torch.float64))
    with pytest.raises(AssertionError):
        E.assert_tile_sums_exact(torch.full((1, 130, 70), 64.0, dtype=torch.float64), 128, 64)


def test_mismatch_report_names_count_first_elements_and_the_box():
    ref = torch.zeros(300, 200, dtype=torch.float64)
    got = ref.clone()
    got[130:134, 72:80] = 5.0
    got[131, 73] = float("nan")
    msg = E.mismatch_report(got, ref, "case")
    assert "32 of 60000 elements differ (1 NaN)" in msg and "(130, 72, 5.0, 0.0)" in msg
    assert "rows 130..133 (mod 128: 2..5, mod 64: 2..5)" in msg and "columns 72..79 (mod 128: 72..79, mod 64: 8..15)" in msg
    assert "no element differs" in E.mismatch_report(ref, ref)
    nchw = torch.zeros(1, 8, 4, 4, dtype=torch.float64)
    bad = nchw.clone()
    bad[0, 5, 2, 3] = 1.0
    assert "(11, 5, 1.0, 0.0)" in E.mismatch_report(bad, nchw)          # (pixel, channel) of a channels-last result


def test_ulp_is_the_spacing_of_the_storage_type():
    v = torch.tensor([0.0, 1.0, 1.5, 300.0, 2.0 ** -20], dtype=torch.float64)
    assert E.ulp(v, torch.float16).tolist() == [2.0 ** -24, 2.0 ** -10, 2.0 ** -10, 0.25, 2.0 ** -24]
    assert E.ulp(v, torch.bfloat16).tolist() == [2.0 ** -133, 2.0 ** -7, 2.0 ** -7, 2.0, 2.0 ** -27]


# ------------------------------------------------------------------------------------------------ the precondition, per list
@pytest.mark.parametrize("entry", E.CONV_DEEP, ids=lambda e: "x".join(map(str, e[0])))
def test_precondition_convolution_cases(entry):
    shape = entry[0]
    c = E.conv_case(shape)
    for T in DT.values():
        for form in E.CONV_FORMS:
            assert_exact(c["refs"][form], T, f"{shape} {form}")
    assert c["refs"]["bias+residual"].unique().numel() >= 150       # a wrong index does not give the right sum by chance
    assert E.conv_plans(64 * 2 ** 20, shape)


def test_precondition_autograd_upsample_gemm_gn_and_thin_cases():
    for T in DT.values():
        for shape in E.CONV_AUTOGRAD:
            c = E.conv_case(shape)
            for ref in list(c["refs"].values()) + [c["dx"]]:
                assert_exact(ref, T, str(shape))
        for shape in E.UP_SHAPES:
            c = E.up_case(shape)
            for k in ("acc", "y", "g_up", "dx"):
                assert_exact(c[k], T, f"{shape} {k}")
        for shape in E.GEMM_NT:
            c = E.gemm_case(shape)
            for k in ("acc", "acc+bias", "acc+bias+res"):
                assert_exact(c[k], T, f"{shape} {k}")
        for B, Cin, Cout, H, W, groups in E.CONV_GN:
            c = E.conv_case((B, Cin, Cout, H, W, 1))
            z = c["refs"]["bias+residual"] + E.t64(E.small_ints((B, Cout), 901, -4, 4))[:, :, None, None]
            for ref in list(c["refs"].values()) + [z]:
                assert_exact(ref, T, "conv gn")
            for bm, bn in E.CONV_TILES:
                assert H * W % bm == 0 and 8 <= Cout // groups <= bn
                E.assert_tile_sums_exact(z.permute(0, 2, 3, 1).reshape(B, H * W, Cout), bm, Cout // groups)
        for shape in E.THIN_SHAPES:
            for name, c in E.thin_case(shape).items():
                for k in ("acc", "y", "dx"):
                    assert_exact(c[k], T, f"thin {shape} {name} {k}")


def test_precondition_linear_cases():
    for T in DT.values():
        for shape in E.LIN_SHAPES:
            c = E.gemm_case(shape)
            for k in ("acc", "acc+bias", "acc+bias+res"):
                assert_exact(c[k], T, f"{shape} {k}")
            for bm, bn, _ in E.LIN_PLANS:
                E.assert_tile_sums_exact(c["acc+bias+res"][None], bm, bn)
            c = E.ln_case(shape, E.LN_PARTS)
            assert_exact(c["acc"], T, "acc"), assert_exact(c["ref"], T, f"LayerNorm fold {shape}")
        for shape, parts in E.STREAM_CASES:
            c = E.ln_case(shape, parts)
            assert_exact(c["acc"], T, "acc"), assert_exact(c["ref"], T, f"stream {shape}")
    for shape, (groups, hw) in E.LIN_GN.items():
        assert shape in E.LIN_SHAPES and shape[0] % hw == 0 and shape[2] % groups == 0
    assert any(s[2] % 16 == 0 for s in E.LIN_SHAPES)                     # GEGLU runs somewhere


def test_fabricated_layernorm_statistics_are_what_they_claim():
    for shape, parts in [(s, E.LN_PARTS) for s in E.LIN_SHAPES] + E.STREAM_CASES:
        M, K, N = shape
        c = E.ln_case(shape, parts)
        p = c["partials"]
        assert tuple(p.shape) == (M, parts, 2) and torch.equal(p, p.round()) and torch.equal(p.float().double(), p)
        mean = p[:, :, 0].sum(1) / K
        var = p[:, :, 1].sum(1) / K - mean * mean
        assert torch.equal(mean, c["mean"]) and torch.equal(1.0 / torch.sqrt(var + E.LN_EPS), c["rstd"])
        assert set(c["mean"].tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0} and set(c["rstd"].tolist()) == {1.0, 2.0}
        # rows whose rstd the kernels cannot form exactly (mean != 0) have no zero result for the f32 ulp to show in
        with_mean = c["mean"] != 0
        assert bool((c["rstd"][with_mean] == 2.0).all()) and bool((c["shift"] % 2 == 1).all())
        assert bool((c["ref"][with_mean] != 0).all()) and bool((c["ref"][~with_mean] == 0).any())
        # an f32 ulp or four of rstd moves the f32 result by far less than the half spacing of the storage types at 256
        assert 4 * 2.0 ** -22 * float((c["acc"].abs().max() + 2 * c["colsum"].abs().max())) < 1e-3


def test_each_convolution_shape_reaches_the_kernel_it_is_listed_for():
    reached = set()
    for shape, want, tiles in E.CONV_DEEP:
        B, Cin, Cout, H, W, stride = shape
        for bm, bn, splits in E.conv_plans(64 * 2 ** 20, shape):
            got = E.conv_variant(bm, bn, B, H, W, stride, splits, Cout)
            reached.add(got)
            if (bm, bn) in tiles:
                assert got == want, (shape, bm, bn, splits, got)
            else:
                assert got == "per-tap", (shape, bm, bn, splits, got)
        assert Cin // 64 >= 5                                        # several chunks: every ring wraps
    assert reached == {"per-tap", "patch", "patch-wide", "patch-dma", "patch-dma-deep", "patch-dma-wide"}
    for B, Cin, Cout, H, W in E.UP_SHAPES:                           # the fused up-sampling needs a DMA patch form on every tile
        for bm, bn in E.CONV_TILES:
            assert E.conv_variant(bm, bn, B, 2 * H, 2 * W, 1, 1, Cout).startswith("patch-dma")


# ------------------------------------------------------------------------------------------------ the gap, as a test
GAP_SHAPE = (1, 1280, 128, 8, 8)        # B, Cin, Cout, H, W
FAULTS = {"one element": 1, "one 16-byte piece": 8, "one 64-channel k-step row": 64}
SITE = (4, 4, 1, 1)                     # output pixel (y, x) and the tap (ty, tx) whose input goes wrong


def _pixel(x, w, extra, site, lost):
    """fp64 output (Cout,) of one pixel, with the input channels `lost` of one tap read as zero (what a stale, cleared or
    never-filled LDS piece leaves)."""
    py, px, ty, tx = site
    patch = torch.nn.functional.pad(x, (1, 1, 1, 1))[0, :, py:py + 3, px:px + 3].clone()
    patch[lost, ty, tx] = 0.0
    return (w * patch[None]).sum((1, 2, 3)) + extra[:, py, px]


def _first_group(active, width):
    """First aligned group of `width` channels in which `active` holds (the fault site is taken from the non-zero inputs)."""
    for c0 in range(0, active.numel(), width):
        if bool(active[c0:c0 + width].any()):
            return slice(c0, c0 + width)
    raise AssertionError("no non-zero input at the fault site")


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_the_tolerance_bars_accept_small_faults_that_equality_rejects(dt):
    """test_conv3x3_implicit_gemm's recipe (normalish data, close()'s rule: max error <= tol * max|ref|, tol = 2 TOL[dt]) at
    (1, 1280, 128, 8, 8), bars 0.024 (f16) and 0.195 (bf16).  Over 180 fault sites of one output pixel, the worst error over its
    128 channels: one lost input element 0.017 at the median site (up to 0.077), a lost 16-byte piece 0.071 (0.026 .. 0.156), a
    lost 64-channel k-step row 0.205 (0.145 .. 0.322).  The f16 bar accepts the single element at two sites in three and
    neither of the others; the bf16 bar accepts every element, every piece, and the whole k-step row at a third of the sites.
    The same faults in the integer recipe change an output value, which equality rejects in both types."""
    B, Cin, Cout, H, W = GAP_SHAPE
    T = DT[dt]
    rt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(T).double()  # noqa: E731  what dev() hands the kernel
    x = rt(hashrand.normalish((B, Cin, H, W), 61 + Cin))
    w = rt(hashrand.normalish((Cout, Cin, 3, 3), 62 + Cout) * (1.0 / math.sqrt(9 * Cin)))
    bias, res = rt(hashrand.normalish((Cout,), 63) * 0.3), rt(hashrand.normalish((B, Cout, H, W), 64))
    ref = torch.nn.functional.conv2d(x, w, bias, padding=1) + res
    extra = bias[:, None, None] + res[0]
    py, px, ty, tx = SITE
    assert torch.allclose(_pixel(x, w, extra, SITE, slice(0, 0)), ref[0, :, py, px], rtol=0, atol=1e-12)
    bar = 2 * E.TOL[dt] * float(ref.abs().max())
    accepted = {}
    for name, width in FAULTS.items():
        # 180 sites of this pixel: 9 taps x the first channels of each 64-channel chunk
        errs = torch.stack([(_pixel(x, w, extra, (py, px, a, b), slice(c0, c0 + width)) - ref[0, :, py, px]).abs().max()
                            for a in range(3) for b in range(3) for c0 in range(0, Cin, 64)])
        accepted[name] = float((errs <= bar).double().mean())
        print(f"[measured] {dt} normalish recipe, {name}: worst error over the channels {float(errs.median()):.4f} at the median "
              f"site ({float(errs.min()):.4f} .. {float(errs.max()):.4f}), the bar {bar:.4f} accepts {accepted[name]:.0%} of the sites")
    if dt == "f16":
        assert accepted["one element"] >= 0.5 and accepted["one 16-byte piece"] == 0.0 and accepted["one 64-channel k-step row"] == 0.0
    else:
        assert accepted["one element"] == 1.0 and accepted["one 16-byte piece"] == 1.0 and accepted["one 64-channel k-step row"] >= 0.25
    # the integer recipe: the same faults, each at the first channels of that tap whose inputs are non-zero
    c = E.conv_case((B, Cin, Cout, H, W, 1))
    xi, wi, ref_i = c["x"], c["w"], c["refs"]["bias+residual"]
    assert_exact(ref_i, T, "integer recipe")
    extra_i = c["bias"][:, None, None] + c["res"][0]
    assert torch.equal(_pixel(xi, wi, extra_i, SITE, slice(0, 0)), ref_i[0, :, py, px])
    active = (xi[0, :, py + ty - 1, px + tx - 1] != 0) & (wi[:, :, ty, tx] != 0).any(0)
    for name, width in FAULTS.items():
        got = _pixel(xi, wi, extra_i, SITE, _first_group(active, width)).to(T).double()
        assert not torch.equal(got, ref_i[0, :, py, px]), f"{name}: the fault left the integer result unchanged"


# ------------------------------------------------------------------------------------------------ the record
def test_profile_agrees_with_the_case_lists():
    rec = json.loads(PROFILE.read_text())
    key = lambda s: "x".join(map(str, s))  # noqa: E731
    assert set(rec["conv"]) == {key(e[0]) for e in E.CONV_DEEP}
    for shape, variant, tiles in E.CONV_DEEP:
        entry = rec["conv"][key(shape)]
        assert entry["kernel"] == variant and entry["tiles"] == [list(t) for t in tiles]
        ref = E.conv_case(shape)["refs"]["bias+residual"]
        assert entry["max_abs_ref"] == float(ref.abs().max()) and entry["distinct_ref_values"] == ref.unique().numel()
    assert set(rec["linear"]) == {key(s) for s in E.LIN_SHAPES}
    assert set(rec["stream"]) == {key(s) for s, _ in E.STREAM_CASES}
    assert set(rec["thin"]) == {key(s) for s in E.THIN_SHAPES}
    assert set(rec["gemm_nt"]) == {key(s) for s in E.GEMM_NT}
    assert set(rec["upsample"]) == {key(s) for s in E.UP_SHAPES}
    assert {k: v["worst"] for k, v in rec["geglu_ulps"].items()} == E.GEGLU_MEASURED_ULPS
