"""Inputs, case lists and references for the GroupNorm launch-form tests (csrc/group_norm.hip).  A plain helper module: numpy and
CPU torch only, no GPU.  test_norm_inputs.py proves what is claimed here; test_group_norm_forms_gpu.py runs the kernels.

Three things the older GroupNorm tests could not see, and what answers each:

  gn_form()          a hand copy of the host dispatch (small_path / small_wide / small_iters / wide_ok / WideGeom / geometry /
                     GA_GN_NPT): which of the ~30 template instances a shape runs.  CASES lists shapes for every instance and
                     loop, with the form each must land on.
  distinct_groups()  real-valued inputs in which every (image, group) has its OWN mean and scale, so statistics taken from a
                     neighbouring group, another image or a wrong fold pass show far above the tolerance bars (with one
                     distribution for the whole tensor they differ by sampling noise only).
  integer_groups()   integer inputs whose sums and sums of squares are exact in f32 in any order: the partial sums must EQUAL
                     the fp64 ones, and one lost or twice-counted element moves a mean by >= 1 / n, four times the allowed error.

The mutators at the end return deliberately wrong statistics from fp64; test_norm_inputs.py shows that each fails the bars the
GPU file applies, and that the old inputs let the two swap mutants pass."""
import functools

import numpy as np
import torch

import hashrand

DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
TOL = {"f32": 2e-5, "f16": 2e-3, "bf16": 1.6e-2}     # test_kernels_gpu.TOL: y is held to 2 TOL max|ref|, dx to 3 TOL max|ref|
U32 = 2.0 ** -24                                     # unit roundoff of f32
F32_EXACT = 2 ** 24
EPS = 1e-5

# Worst |rstd - fp64| of the kernels on integer_groups() over every case and type, in f32 ulps of the reference, as measured on
# an MI355X (profiles/group_norm_forms.json holds the per-case figures).  rsqrtf is approximate and the variance is
# sum2 * fl32(1 / n) - mean^2 with an inexact 1 / n, so this is a measured figure, not a derived one; the test allows one ulp more.
RSTD_MEASURED_ULPS = 10.886


# ------------------------------------------------------------------------------------------------ the host dispatch, mirrored
def small_path(HW, C, G, slab_bytes):
    cg = C // G
    return HW <= 1024 and cg % 2 == 0 and cg <= 2048 and HW * cg <= 20480 and 128 + slab_bytes * HW * cg <= 160 * 1024


def gn_form(HW, C, G, dt, backward=False):
    """The launch form ga_group_norm_fwd (backward: ga_group_norm_bwd) takes, as a hashable tuple:
      ("small", NT, IT, idle)                 one launch; NT threads, IT slab pieces per thread, idle: lanes without a channel pair
      ("wide", RP, full, aligned, NB, rounds) 16-byte two-launch form; RP pixel rows per block pass, full: 256 % (C / 8) == 0 (no
                                              idle lanes), aligned: (C / G) % 8 == 0 (no vector straddles two groups), NB
                                              statistics blocks per image, rounds of 16 loads per thread in a forward statistics
                                              block (the backward statistics kernel loads 8 at a time: twice the rounds)
      ("narrow", W, NPT, NB)                  W channels per lane, the INSTANTIATED channel items per thread (GA_GN_NPT rounds 3
                                              and 4 up to 5 at W = 1, and anything over 2 to 3 at W = 4), NB statistics blocks"""
    assert C % G == 0 and 1 <= G <= 64
    eb = 4 if dt == "f32" else 2
    cg = C // G
    if small_path(HW, C, G, 4 + (eb if backward else 0)):
        hp = cg // 2
        NT = 1024 if (hp > 256 or HW * hp >= 2048) else 256
        rows = NT // hp
        it = -(-HW // rows)
        assert it <= 24
        return ("small", NT, min(v for v in (4, 8, 12, 24) if it <= v), rows * hp < NT)
    fill = -(-HW // 128)
    if eb == 2 and C % 8 == 0 and cg >= 8 and C <= 2048:
        VP = C // 8
        RP = 256 // VP
        PBs = max(fill, 8 * RP)
        return ("wide", RP, 256 % VP == 0, cg % 8 == 0, -(-HW // PBs), -(-PBs // (16 * RP)))
    W = 4 if cg % 4 == 0 else (1 if cg % 2 else 2)
    npt = -(-(C // W) // 256)
    assert npt <= 5
    inst = {1: 1, 2: 2}.get(npt, 5 if W == 1 else (3 if W == 4 else npt))
    assert W != 4 or npt <= 3, "GA_GN_NPT has no W = 4 instance above 3 items: 768 lanes x 4 channels"
    return ("narrow", W, inst, -(-HW // max(fill, 8)))


def stats_blocks(HW, C, G, dt, backward=False):
    """(NB, pixels per block) of the statistics launch; (0, 0) on the one-launch path."""
    f = gn_form(HW, C, G, dt, backward)
    if f[0] == "small":
        return 0, 0
    fill = -(-HW // 128)
    pb = max(fill, 8 * f[1]) if f[0] == "wide" else max(fill, 8)
    return -(-HW // pb), pb


def sum_depth(HW, C, G, dt, backward=False):
    """An upper bound on the number of f32 additions any one element's contribution passes through on its way into a group's
    sum (the D of the roundoff bounds below: |fl(sum) - sum| <= D u sum|terms|), read off the kernels: the per-thread chain,
    the in-block fold, then fold_partials (16 per lane + 3 butterfly steps)."""
    f = gn_form(HW, C, G, dt, backward)
    cg = C // G
    if f[0] == "small":
        return f[2] + 1 + 6 + f[1] // 64                       # pieces (+ the pair add), wave_sum, one add per wave
    nb, pb = stats_blocks(HW, C, G, dt, backward)
    if f[0] == "wide":
        return -(-pb // f[1]) + 8 + (cg // 8 + 2) * f[1] + 19  # pixels of a lane, 8 channels, vectors x rows of a group, fold
    return pb * f[1] + cg // f[1] + 19                         # pixels x W of a lane, channel items of a group, fold


# ------------------------------------------------------------------------------------------------ the case table
# (B, C, H, W, G) -> {type: forward form}.  The backward takes the same form except where BWD_FORMS says otherwise.
CASES = [
    # one launch
    ((2, 64, 4, 4, 8), {"f32": ("small", 256, 4, False), "f16": ("small", 256, 4, False), "bf16": ("small", 256, 4, False)}),
    ((2, 516, 3, 5, 2), {"f32": ("small", 256, 24, True), "f16": ("small", 256, 24, True), "bf16": ("small", 256, 24, True)}),
    ((2, 1028, 3, 13, 2), {"f32": ("small", 1024, 24, True), "f16": ("small", 1024, 24, True), "bf16": ("small", 1024, 24, True)}),
    ((2, 640, 32, 32, 32), {"f32": ("small", 1024, 12, True), "f16": ("small", 1024, 12, True), "bf16": ("small", 1024, 12, True)}),
    ((2, 80, 8, 9, 2), {"f32": ("small", 256, 8, True), "f16": ("small", 256, 8, True), "bf16": ("small", 256, 8, True)}),
    ((2, 12, 3, 227, 2), {"f32": ("small", 256, 12, True), "f16": ("small", 256, 12, True), "bf16": ("small", 256, 12, True)}),
    ((2, 1920, 16, 16, 32), {"f32": ("small", 1024, 8, True), "f16": ("small", 1024, 8, True), "bf16": ("small", 1024, 8, True)}),
    # wide in 16 bits, narrow in f32
    ((2, 320, 64, 64, 32), {"f32": ("narrow", 2, 1, 128), "f16": ("wide", 6, False, False, 86, 1), "bf16": ("wide", 6, False, False, 86, 1)}),
    ((2, 1280, 33, 63, 32), {"f32": ("narrow", 4, 2, 123), "f16": ("wide", 1, False, True, 123, 2), "bf16": ("wide", 1, False, True, 123, 2)}),
    ((1, 1024, 65, 64, 32), {"f32": ("narrow", 4, 1, 127), "f16": ("wide", 2, True, True, 127, 2), "bf16": ("wide", 2, True, True, 127, 2)}),
    ((2, 1920, 48, 48, 32), {"f32": ("narrow", 4, 2, 128), "f16": ("wide", 1, False, False, 128, 2), "bf16": ("wide", 1, False, False, 128, 2)}),
    ((2, 512, 25, 41, 64), {"f32": ("narrow", 4, 1, 114), "f16": ("wide", 4, True, True, 33, 1), "bf16": ("wide", 4, True, True, 33, 1)}),
    ((2, 288, 9, 9, 32), {"f32": ("narrow", 1, 2, 11), "f16": ("wide", 7, False, False, 2, 1), "bf16": ("wide", 7, False, False, 2, 1)}),
    ((2, 64, 25, 41, 8), {"f32": ("narrow", 4, 1, 114), "f16": ("wide", 32, True, True, 5, 1), "bf16": ("wide", 32, True, True, 5, 1)}),
    ((2, 640, 25, 41, 64), {"f32": ("narrow", 2, 2, 114), "f16": ("wide", 3, False, False, 43, 1), "bf16": ("wide", 3, False, False, 43, 1)}),
    # narrow in every type
    ((2, 99, 5, 7, 33), {"f32": ("narrow", 1, 1, 5), "f16": ("narrow", 1, 1, 5), "bf16": ("narrow", 1, 1, 5)}),
    ((2, 297, 5, 7, 33), {"f32": ("narrow", 1, 2, 5), "f16": ("narrow", 1, 2, 5), "bf16": ("narrow", 1, 2, 5)}),
    ((2, 1275, 3, 3, 51), {"f32": ("narrow", 1, 5, 2), "f16": ("narrow", 1, 5, 2), "bf16": ("narrow", 1, 5, 2)}),
    ((2, 1290, 27, 27, 43), {"f32": ("narrow", 2, 3, 92), "f16": ("narrow", 2, 3, 92), "bf16": ("narrow", 2, 3, 92)}),
    ((2, 1860, 27, 27, 62), {"f32": ("narrow", 2, 4, 92), "f16": ("narrow", 2, 4, 92), "bf16": ("narrow", 2, 4, 92)}),
    ((2, 2108, 25, 25, 62), {"f32": ("narrow", 2, 5, 79), "f16": ("narrow", 2, 5, 79), "bf16": ("narrow", 2, 5, 79)}),
    ((2, 2560, 17, 16, 32), {"f32": ("narrow", 4, 3, 34), "f16": ("narrow", 4, 3, 34), "bf16": ("narrow", 4, 3, 34)}),
]
# backward forms that differ from the forward's: 4 + 4 bytes per slab element no longer fit the LDS
BWD_FORMS = {((2, 640, 32, 32, 32), "f32"): ("narrow", 4, 1, 128)}

# Every form the host can choose (the "what" the table is for); test_norm_inputs.py checks that CASES reaches each.
FORMS_WANTED = (
    [("small", nt, it) for nt in (256, 1024) for it in (4, 8, 12, 24)] +
    [("narrow", 1, n) for n in (1, 2, 5)] + [("narrow", 2, n) for n in (1, 2, 3, 4, 5)] + [("narrow", 4, n) for n in (1, 2, 3)] +
    ["wide RP=1", "wide RP>1 full", "wide RP>1 idle", "wide aligned", "wide straddling", "wide two rounds", "two fold passes"])

# concatenating and producer-fed forms: (B, C1, C2, H, W, G)
CAT_SMALL = [(2, 24, 40, 4, 4, 4),              # 256 threads; the seam (24) inside group 1 of 16 channels
             (2, 328, 312, 16, 16, 32)]         # 1024 threads; the seam (328) inside group 16 of 20 channels
CAT_WIDE = [(2, 640, 640, 33, 63, 32),          # two load rounds (the seam falls on a group boundary: 16 groups each)
            (2, 320, 640, 64, 64, 32)]          # straddling vectors, the seam (320) inside group 10 of 30 channels
CONV_GN = (1, 128, 256, 64, 64, 32)             # B, Cin, Cout, H, W, G: exact_inputs.CONV_GN, one plan
CONV_GN_PLAN = (128, 128, 1, 0)


def case_id(c):
    return "x".join(map(str, c))


# ------------------------------------------------------------------------------------------------ generators
def _u(shape, seed):
    return hashrand.uniform(shape, seed).astype(np.float64)


def group_table(B, G, seed):
    """Target mean m[b, g] and scale s[b, g].  Scales 2^-2 .. 2^2 step through the five powers so that neighbours in g (3 steps
    mod 5) and in b (2 steps) differ; means alternate in sign between neighbours in g and in b with 2.5 <= |m| <= min(6, 12 s):
    neighbouring means differ by >= 5 > 4 = the largest scale, and |m| / s <= 12 (<= 16 on the sample statistics of the smallest
    groups, which check_distinct_case asserts)."""
    b, g = np.meshgrid(np.arange(B), np.arange(G), indexing="ij")
    s = 2.0 ** (((3 * g + 2 * b + seed) % 5) - 2)
    mag = np.minimum(2.5 + 3.5 * _u((B, G), seed + 1), 12.0 * s)
    return np.where((g + b) % 2 == 0, 1.0, -1.0) * mag, s


def channel_params(C, seed):
    """gamma, beta (C,): neighbouring channels never equal."""
    c = np.arange(C)
    gamma = 1.0 + np.where(c % 2 == 0, 1.0, -1.0) * (0.2 + 0.5 * _u((C,), seed))
    beta = ((c % 3) - 1) * 0.3 + 0.1 * _u((C,), seed + 1)
    return gamma, beta


@functools.lru_cache(maxsize=2)
def distinct_groups(B, C, H, W, G, seed=1):
    """fp64 CPU tensors (NCHW): x, cb (B, C), gamma, beta, g (cotangent of y), g2 (the skip connection's gradient).
    Element (b, c, h, w) of x is m[b, g] + s[b, g] * normalish; the channel bias is s[b, g] * (+-)(0.25 .. 0.75) alternating in
    sign from channel to channel; the cotangents are a per-channel scale (0.5 .. 2) times uniform noise plus a per-channel offset."""
    cg = C // G
    m, s = group_table(B, G, seed)
    rep = lambda t: np.repeat(t, cg, axis=1)                                   # noqa: E731  (B, G) -> (B, C)
    x = rep(m)[:, :, None, None] + rep(s)[:, :, None, None] * hashrand.normalish((B, C, H, W), seed + 2).astype(np.float64)
    c = np.arange(C)
    cb = rep(s) * np.where(c % 2 == 0, 1.0, -1.0)[None, :] * (0.25 + 0.5 * _u((B, C), seed + 3))
    gamma, beta = channel_params(C, seed + 4)
    gs, go = 0.5 + 0.5 * (c % 4), ((c % 5) - 2) * 0.1
    g = gs[None, :, None, None] * (2.0 * _u((B, C, H, W), seed + 6) - 1.0) + go[None, :, None, None]
    g2 = 0.8 * gs[::-1].copy()[None, :, None, None] * (2.0 * _u((B, C, H, W), seed + 7) - 1.0) - go[None, :, None, None]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))                    # noqa: E731
    return {"x": t(x), "cb": t(cb), "gamma": t(gamma), "beta": t(beta), "g": t(g), "g2": t(g2), "m": t(m), "s": t(s)}


def old_inputs(B, C, H, W):
    """What test_group_norm_act feeds (one distribution for the whole tensor), as fp64 of the f16 values."""
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).half().double()    # noqa: E731
    return {"x": f(hashrand.normalish((B, C, H, W), 7 + C) * 1.7 + 0.3), "gamma": f(hashrand.normalish((C,), 8) * 0.5 + 1.0),
            "beta": f(hashrand.normalish((C,), 9) * 0.2), "g": f(hashrand.normalish((B, C, H, W), 10)), "cb": None}


@functools.lru_cache(maxsize=2)
def integer_groups(B, C, H, W, G, seed=1):
    """Integer inputs with exact statistics.  t = x + cb (what the kernels sum) is c[b, g] + d with an integer centre
    c = ((3 g + 5 b + seed) mod 11) - 5 in -5 .. 5 (neighbours in g differ by 3 mod 11, in b by 5 mod 11) and a deviation d drawn
    evenly from D \\ {+c, -c}, D = {+-1} or {+-1, +-2, +-3} alternating with (g + b) (two scales; {+-2} where D \\ {+-c} is
    empty): t is never 0, |t| <= 8, and the deviations are symmetric, so a group's mean stays within 0.5 of c and every element is
    >= 0.5 away from it (asserted by check_integer_case).  cb in {-1, +1} alternates from channel to channel; x = t - cb with the
    bias, x = t without: both have the SAME statistics.
    Cotangents: cot[b, g] a non-zero integer constant per group (differs between neighbours), skip: small non-zero integers."""
    cg = C // G
    b, g = np.meshgrid(np.arange(B), np.arange(G), indexing="ij")
    c = ((3 * g + 5 * b + seed) % 11) - 5
    wide_set = (g + b) % 2 == 0
    h = hashrand.hash_u32(B * C * H * W, seed + 11).reshape(B, G, cg * H * W) >> np.uint32(8)
    t = np.empty((B, G, cg * H * W), np.float64)
    for bi in range(B):
        for gi in range(G):
            ci = int(c[bi, gi])
            devs = [d for d in ((-3, -2, -1, 1, 2, 3) if wide_set[bi, gi] else (-1, 1)) if abs(d) != abs(ci)] or [-2, 2]
            t[bi, gi] = ci + np.asarray(devs, np.float64)[h[bi, gi] % np.uint32(len(devs))]
    t = t.reshape(B, C, H, W)
    cb = np.broadcast_to(np.where(np.arange(C) % 2 == 0, 1.0, -1.0)[None, :], (B, C)) * np.where(np.arange(B) % 2 == 0, 1.0, -1.0)[:, None]
    cot = np.where((g + b) % 2 == 0, 1.0, -1.0) * (1 + (2 * g + b) % 5)
    skip = 1.0 + (hashrand.hash_u32(B * C * H * W, seed + 12).reshape(B, C, H, W) >> np.uint32(8)) % np.uint32(4)
    skip = skip * np.where(np.arange(C) % 2 == 0, 1.0, -1.0)[None, :, None, None]
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
    return {"t": f(t), "cb": f(cb), "x_cb": f(t - cb[:, :, None, None]), "c": f(c), "cot": f(cot), "skip": f(skip)}


def group_sums(t, G):
    """(sum, sum of squares) per (image, group) of an NCHW fp64 tensor: (B, G) each."""
    tg = t.reshape(t.shape[0], G, -1)
    return tg.sum(-1), (tg * tg).sum(-1)


def stats_of(s1, s2, n, eps=EPS):
    mean = s1 / n
    return mean, 1.0 / torch.sqrt((s2 / n - mean * mean).clamp_min(0.0) + eps)


def check_integer_case(d, G):
    """The stated conditions of integer_groups(), as assertions; returns the per-(image, group) fp64 sums."""
    t, x = d["t"], d["x_cb"]
    B, C = t.shape[:2]
    n = t[0].numel() // G
    assert bool((t == t.round()).all()) and bool((x == x.round()).all()) and float(t.abs().max()) <= 8 and float(t.abs().min()) >= 1
    assert float(x.abs().max()) <= 9
    s1, s2 = group_sums(t, G)
    assert float(s2.max()) < F32_EXACT and n <= 262144, "a sum of squares reaches 2^24: partial sums would round"
    mean, _ = stats_of(s1, s2, n)
    away = (t.reshape(B, G, -1) - mean[:, :, None]).abs().min()
    assert float(away) >= 0.5, f"an element lies {float(away)} from its group's mean"
    assert float((mean - d["c"]).abs().max()) <= 0.5
    assert float((mean[:, 1:] - mean[:, :-1]).abs().min()) >= 1.0 if G > 1 else True
    assert B == 1 or float((mean[0] - mean[1]).abs().min()) >= 1.0
    assert float(d["cot"].abs().min()) >= 1 and float(d["cot"].abs().max()) * n < F32_EXACT
    assert G == 1 or bool((d["cot"][:, 1:] != d["cot"][:, :-1]).all())
    return s1, s2


FAKE_RSTD = 0.5


def second_reduction_exact(d, G):
    """The backward's SECOND reduction made exact.  ga_group_norm_bwd takes (mean, rstd) as an input, so the test hands it the
    integer centre c[b, g] as the mean and FAKE_RSTD = 1/2 as rstd: yhat = (t - c) / 2 is a non-zero multiple of 1/2 with
    |yhat| <= 1.5, dyhat = cot (no SiLU, gamma = 1), every product dyhat yhat is a multiple of 1/2 and every partial sum stays
    below 2^23 in magnitude (asserted), where f32 holds all multiples of 1/2: the kernels' sum equals the fp64 sum in any order,
    and one lost or twice-counted element changes it by |cot yhat| >= 1/2.  -> (B, G) fp64 sums of dyhat * yhat."""
    t, c, cot = d["t"], d["c"], d["cot"]
    B = t.shape[0]
    yh = (t.reshape(B, G, -1) - c[:, :, None]) * FAKE_RSTD
    assert float(yh.abs().min()) >= 0.5 and float(yh.abs().max()) <= 1.5
    terms = cot[:, :, None] * yh
    assert float(terms.abs().sum(-1).max()) < 2 ** 23 and bool((terms * 2 == (terms * 2).round()).all())
    return terms.sum(-1)


def halves(x, C1):
    """The two sources of a concatenation case: x[:, :C1], x[:, C1:] (the case lists choose C1: off a group boundary wherever
    the issue's shapes allow; a multiple of 8 for the wide form, whose sources are whole 16-byte vectors)."""
    return x[:, :C1], x[:, C1:]


def check_distinct_case(d, G, with_cb):
    """The stated conditions of distinct_groups() on the ACTUAL statistics of x (+ cb)."""
    x = d["x"] + (d["cb"][:, :, None, None] if with_cb else 0.0)
    B = x.shape[0]
    s1, s2 = group_sums(x, G)
    n = x[0].numel() // G
    mean = s1 / n
    std = torch.sqrt(s2 / n - mean * mean)
    assert float((mean.abs() / std).max()) <= 16.0, float((mean.abs() / std).max())
    assert float(mean.abs().max()) <= 7.0 and float(std.min()) >= 0.18 and float(std.max()) <= 6.0
    if G > 1:
        gap = (mean[:, 1:] - mean[:, :-1]).abs() / torch.maximum(std[:, 1:], std[:, :-1])
        assert float(gap.min()) >= 1.0, float(gap.min())
        assert float((std[:, 1:] / std[:, :-1] - 1.0).abs().min()) >= 0.3
    if B > 1:
        gap = (mean[0] - mean[1]).abs() / torch.maximum(std[0], std[1])
        assert float(gap.min()) >= 1.0, float(gap.min())
    for k in ("gamma", "beta"):
        assert bool((d[k][1:] != d[k][:-1]).all())
    assert bool((d["cb"][:, 1:] != d["cb"][:, :-1]).all())
    return mean, std


# ------------------------------------------------------------------------------------------------ fp64 reference with hooks
def _per_channel(t, C):
    """(B, G) or (B, C) statistics -> (B, C, 1, 1)."""
    return (t if t.shape[1] == C else t.repeat_interleave(C // t.shape[1], 1))[:, :, None, None]


def gn_forward(x, cb, gamma, beta, G, act, eps=EPS, stats=None):
    """y (and the (mean, rstd) used) of GroupNorm(+SiLU) on an NCHW fp64 tensor; stats = (mean, rstd) (B, G) overrides the
    statistics — the hook the mutators use.  With stats=None this is torch.nn.functional.group_norm (test_norm_inputs.py
    checks that)."""
    B, C = x.shape[:2]
    a = x + (cb[:, :, None, None] if cb is not None else 0.0)
    if stats is None:
        s1, s2 = group_sums(a, G)
        stats = stats_of(s1, s2, a[0].numel() // G, eps)
    mean, rstd = (_per_channel(t, C) for t in stats)
    yh = (a - mean) * rstd
    z = yh * gamma[None, :, None, None] + beta[None, :, None, None]
    return (z * torch.sigmoid(z) if act else z), stats


def gn_backward(x, cb, gamma, beta, G, act, dy, eps=EPS, stats=None, red=None):
    """dx of the same; stats as above, red = (mean of dyhat, mean of dyhat * yhat) (B, G) overrides the two reductions."""
    B, C = x.shape[:2]
    a = x + (cb[:, :, None, None] if cb is not None else 0.0)
    if stats is None:
        s1, s2 = group_sums(a, G)
        stats = stats_of(s1, s2, a[0].numel() // G, eps)
    mean, rstd = (_per_channel(t, C) for t in stats)
    yh = (a - mean) * rstd
    dz = dy
    if act:
        z = yh * gamma[None, :, None, None] + beta[None, :, None, None]
        s = torch.sigmoid(z)
        dz = dy * s * (1.0 + z * (1.0 - s))
    dh = dz * gamma[None, :, None, None]
    if red is None:
        n = a[0].numel() // G
        r1, r2 = group_sums(dh, G)[0] / n, group_sums(dh * yh, G)[0] / n
    else:
        r1, r2 = red
    m1, m2 = (_per_channel(t, C) for t in (r1, r2))
    return rstd * (dh - m1 - yh * m2)


# ------------------------------------------------------------------------------------------------ bars
def mean_bar(ref_mean):
    """|mean - ref| allowed on exact sums: fl32(sum * fl32(1 / n)) is two f32 roundings of a value <= max(|ref|, 1), one more
    for slack, each 2^-24 relative: 2^-22 max(|ref|, 1)."""
    return 2.0 ** -22 * ref_mean.abs().clamp_min(1.0)


def rstd_bar(ref_rstd):
    """measured worst difference + one f32 ulp (of the reference's binade)."""
    return (RSTD_MEASURED_ULPS + 1.0) * torch.exp2(torch.floor(torch.log2(ref_rstd)) - 23)


def real_stats_bars(mean, std, D, eps=EPS):
    """Allowed |mean - ref| and |rstd - ref| on REAL-valued inputs (distinct_groups), from f32 roundoff of the one-pass sums with
    u = 2^-24 and D = sum_depth():  |fl(S1) - S1| <= D u n E|a| <= D u n (|m| + s),  |fl(S2) - S2| <= (D + 1) u n (m^2 + s^2)
    (one more for the square), mean = fl32(S1 fl32(1 / n)): two more roundings of |m|.  var = S2 / n - mean^2 in fp64 from those:
    |dvar| <= u [(D + 2) (m^2 + s^2) + 2 |m| (D + 2) (|m| + s) + 2 m^2], and rstd = rsqrtf(fl32(var) + eps) moves by
    rstd dvar / (2 (s^2 + eps)) plus four ulps for the cast, the add and the approximate rsqrtf.  Worst-case bounds: a few 1e-3
    relative at |m| / s = 16 — two orders above what random rounding gives, and far below the >= 30 % by which neighbouring
    groups' scales and the >= 1 scale by which their means differ."""
    m, v = mean.abs(), std * std
    bm = U32 * ((D + 2) * (m + std) + 2 * m)
    dvar = U32 * ((D + 2) * (m * m + v) + 2 * m * (D + 2) * (m + std) + 2 * m * m)
    rstd = 1.0 / torch.sqrt(v + eps)
    return bm, rstd * (dvar / (2 * (v + eps)) + 4 * 2.0 ** -23)


def rounding_qualifies(ref64, T):
    """Elements of the fp64 reference further than 4 * 2^-24 |value| from a rounding boundary of the 16-bit type T: the whole
    interval value (1 -+ 4 u) rounds to ONE value of T (rounding is monotone, so a boundary inside the interval splits it)."""
    return (ref64 * (1.0 - 4 * U32)).to(T) == (ref64 * (1.0 + 4 * U32)).to(T)


def bwd_zero_bound(c, rstd, mean, ymax, D, dtype):
    """|dx| allowed where the true dx is 0 (act off, gamma = 1, cotangent = the constant c over the group), per group, with
    u = 2^-24, e_mu = mean_bar (what the statistics test allows the kernel's mean to be off by), Y = ymax = max|yhat|:
      dyhat = c exactly;  S0 = n c exactly (an integer below 2^24);  m1 = fl32(S0 fl32(1 / n)):  |c - m1| <= 2 u |c|
      yhat_i = fl32(fl32(t_i - mu) rs):  two roundings, and sum_i (t_i - mu) rs = n (m - mu) rs  (the residual of sum(yhat))
      S1 = fl-sum of fl32(c yhat_i): |S1| <= |c| rs n e_mu + (D + 3) u |c| sum|yhat_i|,  sum|yhat_i| <= 1.01 n  (rms yhat <= 1)
      m2 = fl32(S1 fl32(1 / n)):  |m2| <= 1.01 |c| (rs e_mu + (D + 3) u)
      dx = fl32(rs (c - m1 - yhat m2)):  |dx| <= 1.01 rs |c| (2 u + Y (rs e_mu + (D + 3) u))
    then the store: a relative rounding of the type (inside the 1.01 for f32; + 2^-8 relative for the 16-bit types) and, in f16,
    flush to its subnormal step: + 2^-25.  With the skip connection's gradient k added in f32 before the store, |dx - k| gets
    one more f32 rounding of |k|: + 2^-23 |k|, added by the caller."""
    rel = 1.01 * (1.0 + (2.0 ** -7 if dtype != "f32" else 0.0))
    return rel * rstd * c.abs() * (2 * U32 + ymax * (rstd * mean_bar(mean) + (D + 3) * U32)) + 2.0 ** -25


# ------------------------------------------------------------------------------------------------ mutators (on the statistics)
def straddling_channels(C, G, g):
    """The channels of group g that share an 8-channel vector with group g + 1 (the first `split` lanes of the straddling
    vector); where the boundary falls on a vector boundary, the whole last vector of g (or all of g if it is narrower)."""
    cg = C // G
    end = (g + 1) * cg
    lo = (end // 8) * 8 if end % 8 else end - min(8, cg)
    return max(lo, g * cg), end


def mutant_group_swap(stats, C, g):
    """Per-channel (B, C) statistics in which straddling_channels(g) of group g carry group g + 1's (mean, rstd)."""
    G = stats[0].shape[1]
    lo, hi = straddling_channels(C, G, g)
    out = [t.repeat_interleave(C // G, 1).clone() for t in stats]
    for o, t in zip(out, stats):
        o[:, lo:hi] = t[:, g + 1:g + 2]
    return tuple(out)


def mutant_image_swap(stats):
    """image b's statistics used for image b ^ 1."""
    idx = torch.arange(stats[0].shape[0]) ^ 1
    return stats[0][idx], stats[1][idx]


def mutant_sums(t, G, kind, b, g, block=None):
    """(S1, S2) (B, G) fp64 with ONE fault in group g of image b: "drop" / "double": the group's element of LEAST magnitude left
    out / counted twice (the least visible choice for the mean); "last block": the pixels [block[0], block[1]) left out."""
    B, C, H, W = t.shape
    cg = C // G
    s1, s2 = (v.clone() for v in group_sums(t, G))
    slab = t[b, g * cg:(g + 1) * cg].reshape(cg, H * W)
    if kind == "last block":
        lost = slab[:, block[0]:block[1]]
        s1[b, g] -= lost.sum()
        s2[b, g] -= (lost * lost).sum()
        return s1, s2
    e = slab.reshape(-1)[slab.abs().reshape(-1).argmin()]
    sign = -1.0 if kind == "drop" else 1.0
    s1[b, g] += sign * e
    s2[b, g] += sign * e * e
    return s1, s2


MUTATORS = ["group swap", "image swap", "drop", "double", "last block"]
