"""GroupNorm (csrc/group_norm.hip) on EVERY launch form the host can choose, on inputs that cannot hide a fault
(norm_inputs.py says which form each case is there for, and test_norm_inputs.py proves on the CPU what these inputs show):

  distinct groups   every (image, group) has its own mean and scale: forward, backward and the with_alias backward against fp64
                    torch.nn.functional.group_norm at the bars of test_group_norm_act, on f32 / f16 / bf16, with and without SiLU
                    and channel bias; the saved (mean, rstd) against fp64 at a derived roundoff bar.
  exact statistics  integer inputs: the forward workspace [B][NB][G][2] (and the producers' partial sums) folded in fp64 must
                    EQUAL the integer sums, (mean, rstd) are held to 2^-22 and measured + 1 ulp, the 16-bit affine output (no
                    SiLU) must be the correctly ROUNDED fp64 value wherever that value lies further than 4 * 2^-24 |value| from
                    a rounding boundary of the type (>= 95 % of every case), the backward's first reduction
                    must equal n c exactly in its workspace, its second one must EQUAL the fp64 sum when the statistics
                    handed in are the integer centre and 1/2, and with a constant cotangent per group (true dx = 0) |dx| stays
                    under a derived roundoff bound, with and without the skip connection's gradient (the one-launch
                    backward has no workspace: there that bound is what sees a lost element, at a quarter of its effect).
  producers         ga_cat_group_norm_fwd, ga_cat_channels_gn + ga_group_norm_apply, ga_conv3x3_nhwc_gn + ga_group_norm_apply
                    on the same inputs: bit-identical to the plain norm where the existing tests require it."""
import time

import pytest
import torch

import exact_inputs as E
import norm_inputs as N
from norm_inputs import DT, EPS, TOL
from test_kernels_gpu import close
from test_output_bounds_gpu import gn_blocks_in_use

pytestmark = pytest.mark.gpu
NHWC = torch.channels_last
ALL = ["f32", "f16", "bf16"]
HALF = ["f16", "bf16"]
CODE = {"f16": 0, "bf16": 1, "f32": 2}
CASES = [c for c, _ in N.CASES]


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


def f64(t):
    return t.detach().double().cpu()


def nan(shape, T, nhwc=False):
    t = torch.full(shape, float("nan"), device="cuda", dtype=T)
    return t.contiguous(memory_format=NHWC) if nhwc else t


def group_stats64(a, G):
    s1, s2 = N.group_sums(a, G)
    n = a[0].numel() // G
    mean = s1 / n
    return mean, torch.sqrt((s2 / n - mean * mean).clamp_min(0.0)), n


def check_real_stats(stats, a64, G, D, what):
    """The kernel's (mean, rstd) (B, G, 2) f32 against fp64 of the same (rounded) inputs at norm_inputs.real_stats_bars."""
    mean, std, _ = group_stats64(a64, G)
    bm, br = N.real_stats_bars(mean, std, D + 1)              # + 1: x + channel bias is one more f32 rounding per element
    got = f64(stats)
    em, er = (got[..., 0] - mean).abs(), (got[..., 1] - 1.0 / torch.sqrt(std * std + EPS)).abs()
    assert bool((em <= bm).all()) and bool((er <= br).all()), \
        f"{what}: mean off by {float((em / bm).max()):.2f} bars, rstd by {float((er / br).max()):.2f} bars"
    return float((em / bm).max()), float((er / br).max())


# ------------------------------------------------------------------------------------------------ the mirror
def test_mirror_agrees_with_the_library(ops):
    """norm_inputs.gn_form against the library's own queries (ga_group_norm_one_launch, _two_launch, ga_cat_channels_gn_blocks)
    and against the NB of test_output_bounds_gpu's workspace mask, over every case of this file and the older tests' shapes."""
    lib = ops.load()
    shapes = CASES + [(B, C1 + C2, H, W, G) for B, C1, C2, H, W, G in N.CAT_SMALL + N.CAT_WIDE]
    shapes += [(1, 320, 64, 64, 32), (1, 640, 32, 32, 32), (1, 1920, 32, 32, 32), (2, 2560, 16, 16, 32), (2, 96, 3, 5, 32), (1, 256, 20, 20, 32)]
    for B, C, H, W, G in shapes:
        HW = H * W
        for dt in ALL:
            form = N.gn_form(HW, C, G, dt)
            nb = N.stats_blocks(HW, C, G, dt)[0]
            assert bool(lib.ga_group_norm_one_launch(HW, C, G, CODE[dt])) == (form[0] == "small"), (B, C, H, W, G, dt)
            assert bool(lib.ga_group_norm_two_launch(HW, C, G, CODE[dt])) == (form[0] == "wide"), (B, C, H, W, G, dt)
            assert lib.ga_cat_channels_gn_blocks(HW, C, G, CODE[dt]) == (nb if form[0] == "wide" else 0), (B, C, H, W, G, dt)
            for bwd in (False, True):
                assert N.stats_blocks(HW, C, G, dt, bwd)[0] == gn_blocks_in_use(HW, C, G, DT[dt], bwd)


# ------------------------------------------------------------------------------------------------ distinct groups
@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("case", CASES, ids=N.case_id)
def test_forms_on_distinct_groups(ops, case, dt):
    """Forward, backward and with_alias backward (non-zero skip gradient) against fp64 torch.nn.functional.group_norm at the bars
    of test_group_norm_act (2 TOL on y, 3 TOL on dx), with and without SiLU and channel bias; the saved statistics against fp64."""
    B, C, H, W, G = case
    T = DT[dt]
    t0 = time.perf_counter()
    d = N.distinct_groups(*case)
    x, g, g2 = (dev(d[k], T, True) for k in ("x", "g", "g2"))
    w, b, cb = dev(d["gamma"], T), dev(d["beta"], T), dev(d["cb"], T)
    D = max(N.sum_depth(H * W, C, G, dt), N.sum_depth(H * W, C, G, dt, True))
    worst = {}
    for with_cb in (False, True):
        bias = cb if with_cb else None
        a64 = f64(x) + (f64(cb)[:, :, None, None] if with_cb else 0.0)
        xr = a64.clone().requires_grad_(True)
        lin = torch.nn.functional.group_norm(xr, G, f64(w), f64(b), EPS)
        for act in (False, True):
            yr = torch.nn.functional.silu(lin) if act else lin
            (dxr,) = torch.autograd.grad(yr, xr, f64(g), retain_graph=True)
            xa = x.clone().requires_grad_(True)
            y = ops.group_norm_act(xa, w, b, G, EPS, act, bias)
            stats = y.grad_fn.saved_tensors[3]
            y.backward(g)
            xc = x.clone().requires_grad_(True)
            y2, alias = ops.group_norm_act(xc, w, b, G, EPS, act, bias, True)
            torch.autograd.backward([y2, alias], [g, g2])
            what = f"{case} {dt} act {act} bias {with_cb}"
            assert torch.equal(y2, y), what
            figs = {"y": float((f64(y) - yr.detach()).abs().max() / yr.detach().abs().max()) / (2 * TOL[dt]),
                    "dx": float((f64(xa.grad) - dxr).abs().max() / dxr.abs().max()) / (3 * TOL[dt])}
            ref2 = dxr + f64(g2)
            figs["dx+skip"] = float((f64(xc.grad) - ref2).abs().max() / ref2.abs().max()) / (3 * TOL[dt])
            figs["mean"], figs["rstd"] = check_real_stats(stats, a64, G, D, what)
            for k, v in figs.items():
                worst[k] = max(worst.get(k, 0.0), v)
            close(y, yr.detach().numpy(), TOL[dt] * 2, what + " y")
            close(xa.grad, dxr.numpy(), TOL[dt] * 3, what + " dx")
            close(xc.grad, ref2.numpy(), TOL[dt] * 3, what + " dx + skip-connection gradient")
    torch.cuda.synchronize()
    print(f"[measured] distinct {N.case_id(case)} {dt} {N.gn_form(H * W, C, G, dt)}: {time.perf_counter() - t0:.2f} s, share of the bar: "
          + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------ exact statistics
def check_exact_stats(stats, s1, s2, n, what, eps=EPS):
    """(mean, rstd) of a kernel on exact sums: mean within 2^-22 max(|ref|, 1), rstd within measured + 1 ulp.  Returns the
    worst rstd difference in f32 ulps of the reference (the figure norm_inputs.RSTD_MEASURED_ULPS records)."""
    mean, rstd = N.stats_of(s1, s2, n, eps)
    got = f64(stats)
    em, er = (got[..., 0] - mean).abs(), (got[..., 1] - rstd).abs()
    ulps = float((er / torch.exp2(torch.floor(torch.log2(rstd)) - 23)).max())
    print(f"[measured] rstd {what}: {ulps:.3f} ulps, mean {float((em / N.mean_bar(mean)).max()):.3f} of its bar")
    assert bool((em <= N.mean_bar(mean)).all()), f"{what}: mean off by {float((em / N.mean_bar(mean)).max()):.2f} bars"
    assert bool((er <= N.rstd_bar(rstd)).all()), f"{what}: rstd off by {ulps:.2f} ulps"
    return ulps


def same(got, ref, what):
    got, ref = f64(got), f64(ref)
    assert torch.equal(got, ref), f"{what}: {int((got != ref).sum())} of {ref.numel()} differ, first at {(got != ref).nonzero()[:4].tolist()}: " \
                                  f"{got[got != ref][:4].tolist()} against {ref[got != ref][:4].tolist()}"


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("case", CASES, ids=N.case_id)
def test_forms_on_exact_statistics(ops, case, dt):
    """ga_group_norm_fwd / _bwd called with workspaces this test owns, on integer_groups(): see the header.  gamma = 1, beta = 0,
    no SiLU for the exact parts; one SiLU forward at the TOL bar."""
    B, C, H, W, G = case
    HW, T, cg = H * W, DT[dt], C // G
    lib = ops.load()
    d = N.integer_groups(*case)
    s1, s2 = N.check_integer_case(d, G)
    n = HW * cg
    mean64, rstd64 = N.stats_of(s1, s2, n)
    ones, zeros = torch.ones(C, device="cuda", dtype=T), torch.zeros(C, device="cuda", dtype=T)
    cot = dev(d["cot"].repeat_interleave(cg, 1)[:, :, None, None].expand(B, C, H, W), T, True)
    skip = dev(d["skip"], T, True)
    ymax = (d["t"].reshape(B, G, -1) - mean64[:, :, None]).abs().amax(-1) * rstd64
    per_elem = lambda t: t.repeat_interleave(cg, 1)[:, :, None, None]          # noqa: E731  (B, G) -> (B, C, 1, 1)
    t0 = time.perf_counter()
    for with_cb in (False, True):
        x = dev(d["x_cb"] if with_cb else d["t"], T, True)
        cb = dev(d["cb"], T) if with_cb else None
        what = f"{case} {dt} bias {with_cb}"
        # ---- forward: partial sums and statistics
        nb = N.stats_blocks(HW, C, G, dt)[0]
        ws = nan((B * 257 * G * 2,), torch.float32)
        y, stats = nan((B, C, H, W), T, True), nan((B, G, 2), torch.float32)
        rc = lib.ga_group_norm_fwd(ops._ptr(x), ops._ptr(cb), ops._ptr(ones), ops._ptr(zeros), ops._ptr(y), ops._ptr(stats), ops._ptr(ws),
                                   B, HW, C, G, EPS, 0, CODE[dt], ops.stream_ptr())
        assert rc == 0, what
        if nb:
            part = f64(ws[:B * nb * G * 2]).reshape(B, nb, G, 2)
            assert not bool(torch.isnan(part).any()), f"{what}: a partial sum in use was never written"
            same(part[..., 0].sum(1), s1, what + " sums")
            same(part[..., 1].sum(1), s2, what + " sums of squares")
        else:
            assert bool(torch.isnan(ws).all()), f"{what}: the one-launch path touched the workspace"
        check_exact_stats(stats, s1, s2, n, f"{N.case_id(case)} {dt} bias {with_cb}")
        yr = (d["t"] - per_elem(mean64)) * per_elem(rstd64)
        close(y, yr.numpy(), TOL[dt] * 2, what + " y")
        if dt != "f32":     # the affine output has no approximate function behind the statistics: the correctly rounded value
            ok = N.rounding_qualifies(yr, T)
            bad = ok & (y.cpu() != yr.to(T))
            assert float(ok.double().mean()) >= 0.95, what
            assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {int(ok.sum())} outputs away from a rounding boundary differ from " \
                                        f"the rounded fp64 value, first at {bad.nonzero()[:4].tolist()}"
        if with_cb:
            ya = nan((B, C, H, W), T, True)
            assert lib.ga_group_norm_fwd(ops._ptr(x), ops._ptr(cb), ops._ptr(ones), ops._ptr(zeros), ops._ptr(ya), ops._ptr(stats),
                                         ops._ptr(ws), B, HW, C, G, EPS, 1, CODE[dt], ops.stream_ptr()) == 0
            close(ya, torch.nn.functional.silu(yr).numpy(), TOL[dt] * 2, what + " silu(y)")
        # ---- backward: true dx = 0
        nbb = N.stats_blocks(HW, C, G, dt, True)[0]
        D = N.sum_depth(HW, C, G, dt, True)
        bound = per_elem(N.bwd_zero_bound(d["cot"], rstd64, mean64, ymax, D, dt))
        for g_res in (None, skip):
            wsb = nan((B * 257 * G * 2,), torch.float32)
            dx = nan((B, C, H, W), T, True)
            rc = lib.ga_group_norm_bwd(ops._ptr(x), ops._ptr(cb), ops._ptr(cot), ops._ptr(ones), ops._ptr(zeros), ops._ptr(stats),
                                       ops._ptr(g_res), ops._ptr(dx), ops._ptr(wsb), B, HW, C, G, 0, CODE[dt], ops.stream_ptr())
            assert rc == 0, what
            if nbb:
                part = f64(wsb[:B * nbb * G * 2]).reshape(B, nbb, G, 2)
                same(part[..., 0].sum(1), n * d["cot"], what + " backward: sum of dyhat")
            want = f64(skip) if g_res is not None else torch.zeros(B, C, H, W, dtype=torch.float64)
            err = (f64(dx) - want).abs()
            allow = bound + (2.0 ** -23 * want.abs() if g_res is not None else 0.0)
            share = float((err / allow).nan_to_num(nan=float("inf")).max())
            print(f"[measured] dx {N.case_id(case)} {dt} bias {with_cb} skip {g_res is not None}: {share:.4f} of the bound "
                  f"(max |dx - ref| {float(err.nan_to_num(nan=float('inf')).max()):.3e})")
            assert share <= 1.0, f"{what} skip {g_res is not None}: |dx - ref| reaches {share:.3f} of the roundoff bound"
        if nbb:
            # ---- backward, SECOND reduction exactly: the statistics are an input, so hand in mean = the integer centre and
            # rstd = 1/2 (norm_inputs.second_reduction_exact): sum(dyhat yhat) must EQUAL the fp64 sum, at any group size
            fake = torch.stack([d["c"], torch.full_like(d["c"], N.FAKE_RSTD)], -1).to("cuda", torch.float32).contiguous()
            wsb, dx = nan((B * 257 * G * 2,), torch.float32), nan((B, C, H, W), T, True)
            rc = lib.ga_group_norm_bwd(ops._ptr(x), ops._ptr(cb), ops._ptr(cot), ops._ptr(ones), ops._ptr(zeros), ops._ptr(fake),
                                       None, ops._ptr(dx), ops._ptr(wsb), B, HW, C, G, 0, CODE[dt], ops.stream_ptr())
            assert rc == 0, what
            part = f64(wsb[:B * nbb * G * 2]).reshape(B, nbb, G, 2)
            assert not bool(torch.isnan(part).any()), f"{what}: a backward partial sum in use was never written"
            same(part[..., 0].sum(1), n * d["cot"], what + " backward: sum of dyhat (fabricated statistics)")
            same(part[..., 1].sum(1), N.second_reduction_exact(d, G), what + " backward: sum of dyhat * yhat")
    torch.cuda.synchronize()
    print(f"[measured] exact {N.case_id(case)} {dt}: {time.perf_counter() - t0:.2f} s")


# ------------------------------------------------------------------------------------------------ producer-fed forms
def cat_inputs(kind, case, T):
    B, C1, C2, H, W, G = case
    C = C1 + C2
    if kind == "distinct":
        d = N.distinct_groups(B, C, H, W, G)
        x64, gamma, beta = d["x"], d["gamma"], d["beta"]
    else:
        d = N.integer_groups(B, C, H, W, G)
        x64, gamma, beta = d["t"], torch.ones(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    x = dev(x64, T, True)
    a, b = (h.contiguous(memory_format=NHWC) for h in N.halves(x, C1))
    return d, x, a, b, dev(gamma, T), dev(beta, T)


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("kind", ["distinct", "exact"])
@pytest.mark.parametrize("case", N.CAT_SMALL, ids=N.case_id)
def test_cat_group_norm_one_launch(ops, case, kind, dt):
    """ga_cat_group_norm_fwd (through ops.cat_channels(norm=...)): the concatenation bit-exact, the norm's output and statistics
    BIT-IDENTICAL to ga_group_norm_fwd on the concatenated tensor, against fp64, and (exact inputs) the statistics at the exact bars."""
    B, C1, C2, H, W, G = case
    T = DT[dt]
    d, x, a, b, gamma, beta = cat_inputs(kind, case, T)
    for act in (True, False):
        plain = ops.group_norm_act(x.clone().requires_grad_(True), gamma, beta, G, EPS, act)
        with ops.census_scope() as cs:
            y = ops.cat_channels(a, b, gn_for=G, norm=(gamma, beta, EPS, act))
            made = dict(getattr(y, "_ga_gn", None) or {})
            z = ops.group_norm_act(y.requires_grad_(True), gamma, beta, G, EPS, act)
        assert "done" in made and {k[0]: v for k, v in cs.launches.items()}.get("group_norm_fwd") == 1, "not served as one launch"
        assert torch.equal(y.detach(), x) and torch.equal(z, plain)
        assert torch.equal(z.grad_fn.saved_tensors[3], plain.grad_fn.saved_tensors[3])
        ref = torch.nn.functional.group_norm(f64(x), G, f64(gamma), f64(beta), EPS)
        close(z, (torch.nn.functional.silu(ref) if act else ref).numpy(), TOL[dt] * 2, f"{case} {kind} {dt} act {act}")
        if kind == "exact":
            s1, s2 = N.check_integer_case(d, G)
            check_exact_stats(z.grad_fn.saved_tensors[3], s1, s2, H * W * ((C1 + C2) // G), f"cat {N.case_id(case)} {dt}")
        else:
            check_real_stats(z.grad_fn.saved_tensors[3], f64(x), G, N.sum_depth(H * W, C1 + C2, G, dt), f"{case} {dt}")


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("kind", ["distinct", "exact"])
@pytest.mark.parametrize("case", N.CAT_WIDE, ids=N.case_id)
def test_cat_channels_gn_then_apply(ops, case, kind, dt):
    """ga_cat_channels_gn + ga_group_norm_apply: the concatenation bit-exact, the partial sums (exact inputs) EQUAL to the
    integer sums, the norm's output and statistics BIT-IDENTICAL to the two-launch ga_group_norm_fwd, and against fp64."""
    B, C1, C2, H, W, G = case
    T = DT[dt]
    C, HW = C1 + C2, H * W
    d, x, a, b, gamma, beta = cat_inputs(kind, case, T)
    t0 = time.perf_counter()
    for act in (True, False):
        plain = ops.group_norm_act(x.clone().requires_grad_(True), gamma, beta, G, EPS, act)
        with ops.census_scope() as cs:
            y = ops.cat_channels(a, b, gn_for=G)
            made = dict(getattr(y, "_ga_gn", None) or {})
            z = ops.group_norm_act(y.requires_grad_(True), gamma, beta, G, EPS, act)
        assert "partials" in made and {k[0]: v for k, v in cs.launches.items()}.get("group_norm_apply") == 1, "not served by the pair"
        assert made["blocks"] == N.stats_blocks(HW, C, G, dt)[0]
        assert torch.equal(y.detach(), x) and torch.equal(z, plain)
        assert torch.equal(z.grad_fn.saved_tensors[3], plain.grad_fn.saved_tensors[3])
        ref = torch.nn.functional.group_norm(f64(x), G, f64(gamma), f64(beta), EPS)
        close(z, (torch.nn.functional.silu(ref) if act else ref).numpy(), TOL[dt] * 2, f"{case} {kind} {dt} act {act}")
        if kind == "exact":
            s1, s2 = N.check_integer_case(d, G)
            part = f64(made["partials"])
            same(part[..., 0].sum(1), s1, f"{case} {dt} sums")
            same(part[..., 1].sum(1), s2, f"{case} {dt} sums of squares")
            check_exact_stats(z.grad_fn.saved_tensors[3], s1, s2, HW * (C // G), f"cat {N.case_id(case)} {dt}")
        else:
            check_real_stats(z.grad_fn.saved_tensors[3], f64(x), G, N.sum_depth(HW, C, G, dt), f"{case} {dt}")
    torch.cuda.synchronize()
    print(f"[measured] cat {N.case_id(case)} {kind} {dt}: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("dt", HALF)
def test_conv_epilogue_then_apply(ops, dt):
    """ga_conv3x3_nhwc_gn + ga_group_norm_apply on one plan, on exact_inputs' integer convolution (its partial sums are compared
    for equality by test_gemm_exact_gpu): the one-launch norm against fp64 at 2 TOL and against the two-launch norm at TOL (the
    epilogue groups its partial sums by m tile, and this case's group totals pass 2^24: the f32 fold rounds), statistics against
    fp64 at the roundoff bar."""
    B, Cin, Cout, H, W, G = N.CONV_GN
    T = DT[dt]
    c = E.conv_case((B, Cin, Cout, H, W, 1))
    cb64 = E.t64(E.small_ints((B, Cout), 901, -4, 4))
    x, res, w, bias, cb = dev(c["x"], T, True), dev(c["res"], T, True), dev(c["w"], T), dev(c["bias"], T), dev(cb64, T)
    gamma64, beta64 = (torch.from_numpy(v) for v in N.channel_params(Cout, 5))
    gamma, beta = dev(gamma64, T), dev(beta64, T)
    wp = ops.conv3x3_packed_weights(w, False)
    y, made = ops.conv3x3_nhwc(x, wp, Cout, 1, bias, res, plan=N.CONV_GN_PLAN, gn=(G, cb))
    assert made is not None and torch.equal(f64(y), c["refs"]["bias+residual"])
    a64 = f64(y) + cb64[:, :, None, None]
    for act in (True, False):
        out = ops.GroupNormAct.apply(y.requires_grad_(True), gamma, beta, G, EPS, act, cb, False, made)
        two = ops.group_norm_act(y, gamma, beta, G, EPS, act, cb)
        ref = torch.nn.functional.group_norm(a64, G, f64(gamma), f64(beta), EPS)
        ref = torch.nn.functional.silu(ref) if act else ref
        close(out, ref.numpy(), TOL[dt] * 2, f"conv + apply {dt} act {act}")
        close(out, f64(two).numpy(), TOL[dt], f"conv + apply against two launches {dt} act {act}")
        # additions a term passes through: the epilogue sums a 128-pixel m tile's rows per group in the tile (at most one add
        # per row: 128) and leaves 2 (H W / 128) blocks per image, which fold_partials adds 8 lanes wide (blocks / 8, + 3)
        D = 128 + 2 * (H * W // 128) // 8 + 3
        check_real_stats(out.grad_fn.saved_tensors[3], a64, G, D, f"conv + apply {dt}")
