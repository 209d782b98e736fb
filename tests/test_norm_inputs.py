"""CPU checks of norm_inputs.py, the helper of test_group_norm_forms_gpu.py: the case table lands on the launch forms it is
there for (and the mirror of the host dispatch agrees with the older hand copy in test_output_bounds_gpu.py), the generators
meet their stated conditions, every deliberately wrong statistic fails the bars the GPU file applies — and the inputs of the
older GroupNorm tests let the two swap mutants through, which is the gap this closes."""
import pytest
import torch

import norm_inputs as N
from test_output_bounds_gpu import gn_blocks_in_use

ALL = ["f32", "f16", "bf16"]
CASE_IDS = [N.case_id(c) for c, _ in N.CASES]
# the two largest shapes the table is asked to hold (SD-2.1 768 and the two-round 1280-channel block) at B = 2; every other case
# stays under 5 M elements.  B = 2 is kept for them because "another image's statistics / partial block" can only go wrong, and
# the image-swap mutant only exists, with a second image — and these are the two-round forms nothing else runs at B = 2
LARGE = {(2, 1280, 33, 63, 32): 5322240, (2, 1920, 48, 48, 32): 8847360}
OLD_SHAPES = [(1, 320, 64, 64), (2, 320, 64, 64), (1, 640, 32, 32), (1, 960, 64, 64), (1, 1920, 32, 32), (1, 256, 20, 20),
              (2, 512, 17, 19), (2, 2560, 16, 16), (1, 1920, 16, 16), (2, 1280, 16, 16), (1, 1280, 8, 8), (1, 64, 4, 4),
              (1, 32, 4, 4), (2, 96, 3, 5), (2, 288, 9, 9), (1, 64, 25, 41)]


# ------------------------------------------------------------------------------------------------ the case table
def test_case_table_lands_on_its_forms():
    reached = set()
    for shape, want in N.CASES:
        B, C, H, W, G = shape
        n = B * C * H * W
        assert n <= 5_000_000 or LARGE.get(shape) == n, (shape, n)
        for dt in ALL:
            f = N.gn_form(H * W, C, G, dt)
            assert f == want[dt], (shape, dt, f)
            fb = N.gn_form(H * W, C, G, dt, backward=True)
            assert fb == N.BWD_FORMS.get((shape, dt), f), (shape, dt, fb)
            for form in (f, fb):
                if form[0] == "small":
                    reached.add(form[:3])
                elif form[0] == "narrow":
                    reached.add(form[:3])
                    if dt != "f32" and form[1:3] in ((4, 3), (2, 5), (2, 3), (1, 2)):
                        reached.add("narrow NPT > 1 in 16 bits")
                else:
                    _, RP, full, aligned, NB, rounds = form
                    reached.add("wide RP=1" if RP == 1 else ("wide RP>1 full" if full else "wide RP>1 idle"))
                    reached.add("wide aligned" if aligned else "wide straddling")
                    if rounds == 2:
                        reached.add("wide two rounds")
                        # the second round of the block is real data: more than 16 RP pixels per statistics block
                        assert N.stats_blocks(H * W, C, G, dt)[1] > 16 * RP
            if G > 32:
                reached.add("two fold passes")
    for B, C1, C2, H, W, G in N.CAT_SMALL:
        f = N.gn_form(H * W, C1 + C2, G, "f16")
        assert f[0] == "small" and C1 % ((C1 + C2) // G) != 0, "the seam lies inside a group"
        reached.add(f[:3])
    assert N.gn_form(16, 64, 4, "f16")[1] == 256 and N.gn_form(256, 640, 32, "f16")[1] == 1024
    for (B, C1, C2, H, W, G), rounds, inside in zip(N.CAT_WIDE, (2, 1), (False, True)):
        f = N.gn_form(H * W, C1 + C2, G, "f16")
        assert f[0] == "wide" and f[5] == rounds and (C1 % ((C1 + C2) // G) != 0) == inside and C1 % 8 == 0
    B, Cin, Cout, H, W, G = N.CONV_GN
    assert N.gn_form(H * W, Cout, G, "f16")[0] == "wide"
    missing = [f for f in N.FORMS_WANTED + ["narrow NPT > 1 in 16 bits"] if f not in reached]
    assert not missing, missing
    # the f32 backward of 1028 x 3 x 13 is the unbatched IT = 24 form; 640 x 32 x 32 leaves the one-launch path in f32 only
    assert N.gn_form(39, 1028, 2, "f32", True) == ("small", 1024, 24, True)
    assert N.gn_form(1024, 640, 32, "f32", True)[0] == "narrow" and N.gn_form(1024, 640, 32, "f16", True)[0] == "small"


def test_what_the_older_shapes_never_launch():
    """The gaps the table is for, from the same mirror: over the shapes of test_group_norm_act, _on_offset_groups and
    test_output_bounds_gpu.test_group_norm (32 groups; 8 where 32 do not divide) no launch has IT = 24, two rounds of
    statistics loads, a full-lane wide map above RP = 1, or more than 32 groups."""
    forms = set()
    for B, C, H, W in OLD_SHAPES:
        G = 32 if C % 32 == 0 else 8
        for dt in ALL:
            forms.add(N.gn_form(H * W, C, G, dt))
            forms.add(N.gn_form(H * W, C, G, dt, True))
    assert not [f for f in forms if f[0] == "small" and f[2] == 24]
    assert not [f for f in forms if f[0] == "wide" and (f[5] > 1 or (f[2] and 1 < f[1] < 32))]
    assert {f[1:3] for f in forms if f[0] == "narrow"}.isdisjoint({(1, 5), (2, 3), (2, 4), (2, 5)})


def test_mirror_agrees_with_the_workspace_mask():
    """gn_form / stats_blocks against the NB that test_output_bounds_gpu.gn_blocks_in_use derives.  Both are hand copies of the
    same host arithmetic, so this compares a copy with a copy and only keeps the two from drifting apart; the proof of either is
    on the GPU: the library's own queries (test_group_norm_forms_gpu.test_mirror_agrees_with_the_library) and the NaN-filled
    workspaces, whose slots in use must all be written and sum to the exact totals."""
    shapes = [c for c, _ in N.CASES] + [(B, C, H, W, 32 if C % 32 == 0 else 8) for B, C, H, W in OLD_SHAPES]
    shapes += [(B, C1 + C2, H, W, G) for B, C1, C2, H, W, G in N.CAT_SMALL + N.CAT_WIDE]
    for B, C, H, W, G in shapes:
        for dt in ALL:
            for bwd in (False, True):
                assert N.stats_blocks(H * W, C, G, dt, bwd)[0] == gn_blocks_in_use(H * W, C, G, N.DT[dt], bwd), (B, C, H, W, G, dt, bwd)


def test_reference_is_torch_group_norm():
    d = N.distinct_groups(2, 24, 3, 5, 4)
    for act in (False, True):
        xr = (d["x"] + d["cb"][:, :, None, None]).requires_grad_(True)
        yr = torch.nn.functional.group_norm(xr, 4, d["gamma"], d["beta"], N.EPS)
        yr = torch.nn.functional.silu(yr) if act else yr
        yr.backward(d["g"])
        y, _ = N.gn_forward(d["x"], d["cb"], d["gamma"], d["beta"], 4, act)
        dx = N.gn_backward(d["x"], d["cb"], d["gamma"], d["beta"], 4, act, d["g"])
        assert float((y - yr.detach()).abs().max()) < 1e-12 and float((dx - xr.grad).abs().max()) < 1e-12


# ------------------------------------------------------------------------------------------------ preconditions
@pytest.mark.parametrize("case", [c for c, _ in N.CASES], ids=CASE_IDS)
def test_generators_meet_their_conditions(case):
    B, C, H, W, G = case
    d = N.distinct_groups(*case)
    for with_cb in (False, True):
        N.check_distinct_case(d, G, with_cb)
    di = N.integer_groups(*case)
    s1, s2 = N.check_integer_case(di, G)
    # the exact-output check of the GPU file leaves out elements within 4 * 2^-24 |value| of a rounding boundary: at most 5 %
    mean, rstd = N.stats_of(s1, s2, H * W * (C // G))
    ref = (di["t"] - mean.repeat_interleave(C // G, 1)[:, :, None, None]) * rstd.repeat_interleave(C // G, 1)[:, :, None, None]
    for dt in ("f16", "bf16"):
        share = float(N.rounding_qualifies(ref, N.DT[dt]).double().mean())
        assert share >= 0.95, (case, dt, share)


@pytest.mark.parametrize("case", N.CAT_SMALL + N.CAT_WIDE, ids=N.case_id)
def test_generators_meet_their_conditions_on_the_concatenations(case):
    B, C1, C2, H, W, G = case
    N.check_distinct_case(N.distinct_groups(B, C1 + C2, H, W, G), G, False)
    N.check_integer_case(N.integer_groups(B, C1 + C2, H, W, G), G)


# ------------------------------------------------------------------------------------------------ sensitivity, distinct groups
def _swap_mutants_vs_bars(d, G, cb, act):
    """For the two swap mutants: (|y_mut - y| max) / max|y| and the same for dx, computed on image 0 (the reference over both
    images gives the scale of the bar)."""
    x, gamma, beta, g = d["x"], d["gamma"], d["beta"], d["g"]
    B, C = x.shape[:2]
    y, stats = N.gn_forward(x, cb, gamma, beta, G, act)
    dx = N.gn_backward(x, cb, gamma, beta, G, act, g)
    ymax, dmax = float(y.abs().max()), float(dx.abs().max())
    out = {}
    muts = {"group swap": N.mutant_group_swap(stats, C, G // 2 - 1 if G > 1 else 0)} if G > 1 else {}
    if B > 1:
        muts["image swap"] = N.mutant_image_swap(stats)
    cb0 = None if cb is None else cb[:1]
    for name, st in muts.items():
        st0 = tuple(t[:1] for t in st)
        ym, _ = N.gn_forward(x[:1], cb0, gamma, beta, G, act, stats=st0)
        dm = N.gn_backward(x[:1], cb0, gamma, beta, G, act, g[:1], stats=st0)     # the reductions taken with the wrong statistics
        out[name] = (float((ym - y[:1]).abs().max()) / ymax, float((dm - dx[:1]).abs().max()) / dmax)
    return out


@pytest.mark.parametrize("case", [c for c, _ in N.CASES], ids=CASE_IDS)
def test_swapped_statistics_fail_the_bars_on_distinct_groups(case):
    """Group g + 1's statistics on the straddling channels of group g, and the other image's statistics: both move y by more than
    2 TOL max|y| and dx by more than 3 TOL max|dx| at the loosest type (bf16), with and without SiLU."""
    B, C, H, W, G = case
    d = N.distinct_groups(*case)
    for act in (True, False):
        got = _swap_mutants_vs_bars(d, G, d["cb"], act)
        assert len(got) == (G > 1) + (B > 1)
        for name, (ey, ed) in got.items():
            assert ey > 2 * N.TOL["bf16"] and ed > 3 * N.TOL["bf16"], (case, act, name, ey, ed)


def test_the_older_inputs_let_swapped_statistics_pass():
    """The gap: on normalish * 1.7 + 0.3 at (2, 320, 64, 64) in f16, as test_group_norm_act feeds it, neighbouring groups and the
    two images differ by sampling noise only.  Group g + 1's statistics on a straddling vector stay UNDER the f16 bars (2 TOL on
    y, 3 TOL on dx: 1.8e-3 against 4e-3).  The other image's statistics on ALL 32 groups at once reach 1.0e-2 of max|y| (the
    worst of 32 draws of the noise): over the f16 bar, under the bf16 one (3.2e-2) — so in bf16 neither swap is seen, and in f16
    only the swap of every group at once is."""
    d = N.old_inputs(2, 320, 64, 64)
    for act in (True, False):
        for name, (ey, ed) in _swap_mutants_vs_bars(d, 32, None, act).items():
            print(f"[recorded] old inputs, {name}, act {act}: y {ey:.2e} of max|y|, dx {ed:.2e} of max|dx|")
            seen_by = "f16" if name == "group swap" else "bf16"
            assert ey < 2 * N.TOL[seen_by] and ed < 3 * N.TOL[seen_by], (name, act, ey, ed)


@pytest.mark.parametrize("case", [c for c, _ in N.CASES], ids=CASE_IDS)
def test_swapped_statistics_fail_the_statistics_bars_on_distinct_groups(case):
    """The derived roundoff bars on (mean, rstd) of real-valued inputs (real_stats_bars) are far under what a swap changes."""
    B, C, H, W, G = case
    d = N.distinct_groups(*case)
    mean, std = N.check_distinct_case(d, G, True)
    rstd = 1.0 / torch.sqrt(std * std + N.EPS)
    D = max(N.sum_depth(H * W, C, G, dt) for dt in ALL)
    bm, br = N.real_stats_bars(mean, std, D)
    assert float((br / rstd).max()) < 0.02 and float((bm / std).max()) < 0.01
    if G > 1:
        assert bool(((mean[:, 1:] - mean[:, :-1]).abs() > 4 * torch.maximum(bm[:, 1:], bm[:, :-1])).all())
        assert bool(((rstd[:, 1:] - rstd[:, :-1]).abs() > 4 * torch.maximum(br[:, 1:], br[:, :-1])).all())
    if B > 1:
        assert bool(((mean[0] - mean[1]).abs() > 4 * torch.maximum(bm[0], bm[1])).all())


@pytest.mark.parametrize("case", [c for c, _ in N.CASES], ids=CASE_IDS)
def test_a_lost_block_fails_the_statistics_bars_on_distinct_groups(case):
    """The last pixel block's partial left out, on distinct groups: the mean or rstd moves by more than real_stats_bars.  (The
    one-launch path has no blocks.)  The two single-element mutants, drop and double, CANNOT fail on real-valued inputs — one
    element of n moves the statistics by 1 / n of a scale, under any roundoff bar of a one-pass f32 sum — and are carried by the
    exact inputs alone (test_every_mutant_fails_the_exact_statistics_bars)."""
    B, C, H, W, G = case
    HW = H * W
    d = N.distinct_groups(*case)
    x = d["x"] + d["cb"][:, :, None, None]
    mean, std = N.check_distinct_case(d, G, True)
    n = HW * (C // G)
    ran = 0
    for dt in ALL:
        nb, pb = N.stats_blocks(HW, C, G, dt)
        if nb == 0:
            continue
        ran += 1
        b, g = B - 1, G // 2
        m1, m2 = N.mutant_sums(x, G, "last block", b, g, ((nb - 1) * pb, HW))
        mm, rm = N.stats_of(m1, m2, n)
        bm, br = N.real_stats_bars(mean, std, N.sum_depth(HW, C, G, dt) + 1)
        rstd = 1.0 / torch.sqrt(std * std + N.EPS)
        assert float((mm[b, g] - mean[b, g]).abs()) > bm[b, g] or float((rm[b, g] - rstd[b, g]).abs()) > br[b, g], (case, dt)
    assert ran or "last block" in left_out(case)


# ------------------------------------------------------------------------------------------------ sensitivity, exact inputs
# mutators a case leaves out (at most one each): the one-launch path has no pixel blocks; one group or one image has no neighbour
def left_out(case):
    B, C, H, W, G = case
    out = []
    if N.gn_form(H * W, C, G, "f16")[0] == "small" and N.gn_form(H * W, C, G, "f32")[0] == "small":
        out.append("last block")
    if B == 1:
        out.append("image swap")
    return out


@pytest.mark.parametrize("case", [c for c, _ in N.CASES], ids=CASE_IDS)
def test_every_mutant_fails_the_exact_statistics_bars(case):
    """On integer_groups(): each mutant's sums differ from the fp64 sums (the GPU test asserts equality), and its mean differs
    from the reference by at least FOUR times mean_bar — the bar is at most a quarter of the least visible single-element
    shift.  The rstd bar (measured + 1 ulp = 11.9 ulps) does NOT meet that condition: losing an element e moves the
    variance by ((e - mean)^2 - mean^2) / n, which is 0 for e = 2 mean and close to it for the nearest integer, so the least
    visible single-element mutant moves rstd by less than any bar.  By the issue's wording the MEAN check (and the exact sums)
    therefore carry every case alone; the rstd bar is kept as a check of rsqrtf and the variance arithmetic, and this test only
    prints whether it happens to see the mutants it evaluates."""
    B, C, H, W, G = case
    HW = H * W
    d = N.integer_groups(*case)
    s1, s2 = N.check_integer_case(d, G)
    n = HW * (C // G)
    mean, rstd = N.stats_of(s1, s2, n)
    skipped = left_out(case)
    assert len(skipped) <= 1, skipped
    b, g = B - 1, G // 2
    carried_by_rstd = True
    for kind in N.MUTATORS:
        if kind in skipped:
            continue
        if kind == "group swap":
            m_mut, r_mut = N.mutant_group_swap((mean, rstd), C, g - 1 if g else 0)
            lo, _ = N.straddling_channels(C, G, g - 1 if g else 0)
            dm = (m_mut[:, lo] - mean[:, (g - 1 if g else 0)]).abs().min()
            assert float(dm) >= 1.0
            continue
        if kind == "image swap":
            m_mut, _ = N.mutant_image_swap((mean, rstd))
            assert float((m_mut - mean).abs().min()) >= 1.0
            continue
        if kind == "last block":
            dt = "f16" if N.gn_form(HW, C, G, "f16")[0] != "small" else "f32"
            nb, pb = N.stats_blocks(HW, C, G, dt)
            block = ((nb - 1) * pb, HW)
        else:
            block = None
        m1, m2 = N.mutant_sums(d["t"], G, kind, b, g, block)
        assert float(m1[b, g]) != float(s1[b, g]) and float(m2[b, g]) != float(s2[b, g]), kind
        mm, rm = N.stats_of(m1, m2, n)
        shift = float((mm[b, g] - mean[b, g]).abs())
        assert shift >= 4 * float(N.mean_bar(mean[b, g])), (case, kind, shift, float(N.mean_bar(mean[b, g])))
        if float((rm[b, g] - rstd[b, g]).abs()) < 4 * float(N.rstd_bar(rstd[b, g])):
            carried_by_rstd = False
    # the least visible single element over EVERY group: |e| = 1 exists nearly everywhere, so the shift is 1 / n
    assert 1.0 / n >= 4 * float(N.mean_bar(mean).max()), (case, n)
    print(f"[recorded] {N.case_id(case)}: n {n}, mean bar / (1 / n) = {float(N.mean_bar(mean).max()) * n:.3f}, "
          f"rstd bar happens to see the evaluated mutants: {carried_by_rstd}")


@pytest.mark.parametrize("case", [c for c, _ in N.CASES], ids=CASE_IDS)
def test_one_lost_element_of_the_backward_reductions_is_seen(case):
    """A backward reduction that loses or double counts one element leaves |c| rstd / n in the whole group.  Two checks of the GPU
    file see that, and each (case, type) has one of them:
      two-launch backward (a workspace exists): both columns of the workspace are compared for EQUALITY with fp64 — the second
        with the fabricated statistics of second_reduction_exact, whose preconditions are asserted here; one element moves the
        sum by >= 1/2, at any group size;
      one-launch backward (no workspace): |dx| against bwd_zero_bound, which must be at most a QUARTER of |c| rstd / n."""
    B, C, H, W, G = case
    HW = H * W
    d = N.integer_groups(*case)
    s1, s2 = N.check_integer_case(d, G)
    n = HW * (C // G)
    mean, rstd = N.stats_of(s1, s2, n)
    ymax = ((d["t"].reshape(B, G, -1) - mean[:, :, None]).abs().amax(-1) * rstd)
    for dt in ALL:
        if N.gn_form(HW, C, G, dt, True)[0] == "small":
            bound = N.bwd_zero_bound(d["cot"], rstd, mean, ymax, N.sum_depth(HW, C, G, dt, True), dt)
            worst = float((bound * n / (d["cot"].abs() * rstd)).max())
            print(f"[recorded] {N.case_id(case)} {dt}: n {n}, bound / (|c| rstd / n) = {worst:.3g}")
            assert worst <= 0.25, (case, dt, worst)
        else:
            ref = N.second_reduction_exact(d, G)                       # asserts exactness in f32
            lost = ref.clone()
            lost[B - 1, G // 2] -= d["cot"][B - 1, G // 2] * (d["t"][B - 1, (G // 2) * (C // G), 0, 0] - d["c"][B - 1, G // 2]) * N.FAKE_RSTD
            assert abs(float(lost[B - 1, G // 2] - ref[B - 1, G // 2])) >= 0.5
            assert float(d["cot"].abs().max()) * n < N.F32_EXACT      # first column: n c, an integer below 2^24
