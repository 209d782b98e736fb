"""Integer inputs on which the convolution and Linear GEMM kernels must be right to the last bit, the case lists the exact
tests run, and their fp64 references.  A plain helper module: numpy and CPU torch only, no GPU.

Why integers.  The operands of these kernels are f16 / bf16, the MFMA accumulates in f32, split-K slabs are f32 summed in f32,
and the epilogues are f32 adds followed by one round-to-nearest-even conversion (twice in conv_epilogue / lin_epilogue: after the
accumulator or the bias, and again after the residual).  When every input is a small integer and every partial and final value
is an integer of magnitude <= 256 — which f16 (11 significant bits) and bf16 (8) both hold — no step rounds, so ANY correct
kernel gives exactly the fp64 result whatever its tile, split, ring depth, arrival order or rounding sequence, and one
misplaced, dropped, duplicated or stale element anywhere changes an output.  What this does not test: rounding behaviour on
real-valued data (that stays with the tolerance tests of test_kernels_gpu.py).

Density rule.  ternary() values are in {-1, 0, +1}; a product of two operands of densities da, db over depth K is non-zero
with probability da db, so the accumulator's variance is K da db.  Both operands of a depth-K product get
density(K) = min(1, sqrt(900 / K)): standard deviation <= 30, maxima of 94 - 154 over the case lists with bias and residual.
Where one operand's density is already fixed (the weights, in a backward product of another depth), partner_density() gives
the other so that K da db <= 900 still.  The LayerNorm-fold cases multiply the accumulator by rstd = 2, so they are built for
a standard deviation of 15 (LN_STD).

assert_exact() is the PRECONDITION of every comparison: it is run on every reference and on every intermediate a kernel rounds
(accumulator, + bias, + residual); a case that violates it is a bug in these inputs, never something to filter."""
import functools
import math

import numpy as np
import torch

import hashrand

DT = {"f16": torch.float16, "bf16": torch.bfloat16}
TOL = {"f16": 2e-3, "bf16": 1.6e-2}       # test_kernels_gpu.TOL (the bars the gap demonstration restates)
STD = 30.0                                # accumulator standard deviation the density rule aims at
LN_STD = 15.0                             # ... where the epilogue doubles the accumulator (rstd = 2)
LIMIT = 256                               # at and below it f16 and bf16 hold every integer
F32_EXACT = 2 ** 24                       # below it f32 holds every integer: partial sums stay exact in any order


# ------------------------------------------------------------------------------------------------ generators
def density(K, std=STD):
    return min(1.0, math.sqrt(std * std / K))


def partner_density(K, d_other, std=STD):
    """Density of the second operand of a depth-K product whose first operand has density d_other already."""
    return min(1.0, std * std / (K * d_other))


def ternary(shape, seed, density):
    """float64 array of `shape` with values in {-1, 0, +1}: non-zero with probability `density`, sign by a fair coin, both
    from one hashrand.hash_u32 word per element (its top 24 bits against the density, its lowest bit the sign)."""
    n = int(np.prod(shape))
    u = hashrand.hash_u32(n, seed)
    nonzero = (u >> np.uint32(8)).astype(np.float64) * 2.0 ** -24 < density
    sign = 1.0 - 2.0 * (u & np.uint32(1)).astype(np.float64)
    return (nonzero * sign).reshape(shape)


def small_ints(shape, seed, lo=-8, hi=8):
    """float64 array of `shape` with integers uniform in [lo, hi] (bias, residual, column sums, shifts)."""
    n = int(np.prod(shape))
    return (lo + ((hashrand.hash_u32(n, seed) >> np.uint32(8)) % np.uint32(hi - lo + 1)).astype(np.float64)).reshape(shape)


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


# ------------------------------------------------------------------------------------------------ checks
def assert_exact(ref64, dtype, what=""):
    """Every element of the fp64 tensor survives the round trip through `dtype` unchanged and is an integer-range value
    |v| <= 256.  A precondition of the exact tests, not a filter."""
    ref64 = ref64 if torch.is_tensor(ref64) else t64(ref64)
    assert ref64.dtype == torch.float64, what
    back = ref64.to(dtype).double()
    bad = int((back != ref64).sum())
    assert bad == 0, f"{what}: {bad} of {ref64.numel()} reference values do not survive {dtype}"
    worst = float(ref64.abs().max()) if ref64.numel() else 0.0
    assert worst <= LIMIT, f"{what}: max |reference| {worst} > {LIMIT}"
    return worst


def assert_f32_sums_exact(values64, what=""):
    """Sums and sums of squares over ANY subset of `values64` (integers) are exact in f32: the sum of squares of all of them
    stays below 2^24, and |a sum of integers| <= the sum of their squares."""
    total = float((values64 * values64).sum())
    assert total < F32_EXACT, f"{what}: sum of squares {total} >= 2^24"


def assert_tile_sums_exact(rows64, bm, width, what=""):
    """rows64 (images, pixels or 1, rows, channels): every (bm rows) x (width channels) block — what one epilogue partial sum
    covers at most — satisfies assert_f32_sums_exact."""
    B, R, C = rows64.shape
    padr, padc = -R % bm, -C % width
    sq = torch.nn.functional.pad(rows64 * rows64, (0, padc, 0, padr))
    worst = float(sq.reshape(B, (R + padr) // bm, bm, (C + padc) // width, width).sum((2, 4)).max())
    assert worst < F32_EXACT, f"{what}: a partial sum of squares reaches {worst} >= 2^24"
    return worst


def as_rows(t):
    """(M, N) view for the report: a channels-last (B, C, H, W) result becomes (B H W, C), anything else (-1, last)."""
    if t.dim() == 4:
        return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])
    return t.reshape(-1, t.shape[-1]) if t.dim() > 1 else t.reshape(1, -1)


def mismatch_report(got, ref, what=""):
    """Failure message of an exact comparison: how many elements differ, the first few (m, n, got, ref), and the bounding box
    of the differences in rows and columns, absolute and modulo the tile sizes 128 and 64 — the pattern says which tile, piece
    or k-step went wrong.  NaN in `got` (an element never written) counts as a difference."""
    got, ref = as_rows(got.detach().double().cpu()), as_rows(ref.detach().double().cpu())
    if got.shape != ref.shape:
        return f"{what}: shape {tuple(got.shape)} != reference {tuple(ref.shape)}"
    diff = ~(got == ref)
    n = int(diff.sum())
    if n == 0:
        return f"{what}: no element differs"
    idx = diff.nonzero()
    rows, cols = idx[:, 0], idx[:, 1]
    first = [(int(m), int(c), float(got[m, c]), float(ref[m, c])) for m, c in idx[:6].tolist()]
    box = lambda v, q: f"{int((v % q).min())}..{int((v % q).max())}"  # noqa: E731
    return (f"{what}: {n} of {got.numel()} elements differ ({int(torch.isnan(got).sum())} NaN); first (m, n, got, ref): {first}; "
            f"rows {int(rows.min())}..{int(rows.max())} (mod 128: {box(rows, 128)}, mod 64: {box(rows, 64)}), "
            f"columns {int(cols.min())}..{int(cols.max())} (mod 128: {box(cols, 128)}, mod 64: {box(cols, 64)}); "
            f"max |got - ref| {float((got - ref)[diff].abs().nan_to_num(nan=float('inf')).max())}")


def ulp(ref64, dtype):
    """Spacing of `dtype` at |ref| (fp64 tensor), with the subnormal spacing below the smallest normal."""
    mant, emin = {torch.float16: (10, -14), torch.bfloat16: (7, -126)}[dtype]
    e = torch.floor(torch.log2(ref64.abs().clamp_min(2.0 ** emin)))
    return torch.exp2(e - mant)


def gelu64(g):
    return 0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0)))


# GEGLU outputs are not integers (erf): worst elementwise error of the kernels' h * gelu(g) against fp64 on the exact integer
# h and g, in ulps of the storage type at the reference value, as measured on an MI355X over LIN_SHAPES
# (profiles/gemm_exact.json holds the same figures); the tests assert one ulp above it — the margin is the result's own
# rounding step — and never looser than test_kernels_gpu's TOL[dt] * 2 * max|ref|.
GEGLU_MEASURED_ULPS = {"f16": 131.92, "bf16": 254.25}


# ------------------------------------------------------------------------------------------------ case lists
CONV_TILES = [(128, 128), (128, 64), (64, 64)]
CONV_SPLITS = [1, 2, 4, 16]
CONV_FORMS = ["plain", "bias", "bias+residual"]

# (B, Cin, Cout, H, W, stride) -> the kernel variant the shape is in the list for, and the tiles that reach it
# (conv_variant() restates launch_tile's dispatch; test_exact_inputs.py checks this table against it).
# Every launch of at most 1024 pixels and 384 workgroups takes the DEEP ring, so the patch-DMA rows here are DEEP unless the
# batch lifts them over 1024 pixels.
CONV_DEEP = [
    ((1, 1280, 64, 8, 8, 1), "patch-dma-deep", CONV_TILES),          # 20 chunks; two whole images (128) / one (64) per tile
    ((1, 2560, 64, 8, 8, 1), "patch-dma-deep", CONV_TILES),          # 40 chunks: the up-blocks' concatenated input
    ((2, 640, 128, 16, 16, 1), "patch-dma-deep", CONV_TILES),        # lane_rot = 2 on 16-wide maps
    ((5, 640, 128, 16, 16, 1), "patch-dma", CONV_TILES),             # ... and on the 32 KB ring (1280 pixels)
    ((1, 640, 64, 32, 32, 1), "patch-dma-deep", CONV_TILES),         # whole-row tiles
    ((2, 640, 64, 32, 32, 1), "patch-dma", CONV_TILES),              # whole-row tiles, 2048 pixels: the 32 KB ring
    ((1, 640, 64, 24, 24, 1), "patch", [(64, 64)]),                  # geometry 3: runs of 64 pixels (128-pixel tiles: per-tap)
    ((1, 640, 64, 48, 48, 1), "patch-wide", CONV_TILES),             # the WIDE 13-piece instantiation, register-staged (runs)
    ((1, 320, 64, 4, 128, 1), "patch-dma-wide", [(128, 128), (128, 64)]),   # WIDE: one 128-wide row per tile (64: per-tap)
    ((2, 640, 64, 16, 12, 1), "patch-dma-deep", [(64, 64)]),         # runs of pixels below 16 columns: only the DMA form
    ((2, 640, 64, 12, 12, 1), "per-tap", CONV_TILES),                # 144 pixels per image: no tile divides them
    ((1, 640, 64, 10, 10, 1), "per-tap", CONV_TILES),                # no tile divides the map
    ((2, 640, 64, 9, 7, 1), "per-tap", CONV_TILES),                  # ragged, narrower than 8
    ((1, 640, 128, 16, 16, 2), "per-tap", CONV_TILES),               # stride 2
]
CONV_AUTOGRAD = [(1, 640, 320, 16, 16, 1), (2, 320, 640, 9, 7, 1)]
UP_SHAPES = [(1, 640, 64, 8, 8), (2, 320, 64, 16, 16)]               # B, Cin, Cout, H, W of the half-size input
GEMM_NT = [(130, 1280, 72), (200, 2560, 64)]                         # M, K, N
GEMM_NT_SPLITS = [1, 4]
CONV_GN = [(1, 128, 256, 64, 64, 32)]                                # B, Cin, Cout, H, W, groups: served by every tile
CONV_GN_SPLITS = [1, 2]
THIN_SHAPES = [(2, 320, 5, 16), (1, 320, 16, 16), (2, 256, 74, 112)]   # B, wide channels, H, W (last: two segments per workgroup)

LIN_PLANS = [(128, 128, 0), (128, 128, 2), (128, 64, 0), (128, 64, 3), (64, 128, 0), (64, 64, 0), (64, 64, 5)]   # bm, bn, stages
LIN_SPLITS = [1, 2, 5]
LIN_SHAPES = [(64, 5120, 64), (130, 2560, 264), (200, 1280, 72), (256, 1280, 1280)]   # M, K, N
LIN_FORMS = ["no bias", "bias", "bias+residual", "sliced rows"]
LIN_GN = {(64, 5120, 64): (8, 64), (256, 1280, 1280): (32, 128)}      # shape -> (groups, hw) of the gn= epilogue
LN_PARTS = 3                                                           # partial sums per row of the per-tile LayerNorm-fold cases
LN_EPS = 2.0 ** -6                                                     # var = 1 - eps or 1/4 - eps: K var is an integer
STREAM_CASES = [((1000, 320, 1008), 2), ((130, 1280, 264), 3), ((4096, 320, 1280), 20)]   # (M, K, N), partial sums per row


def conv_variant(bm, bn, B, H, W, stride, splits, cout, threads=256, kc=64):
    """Which kernel launch_tile (csrc/conv3x3.hip) runs for a tile on a shape (the FastDiv limits, far above these sizes,
    left out): per-tap | patch | patch-wide | patch-dma | patch-dma-deep | patch-dma-wide."""
    def geometry(wide):
        if bm % W == 0 and (H * W) % bm == 0:
            nseg, srows = 1, bm // W
        elif bm % (H * W) == 0:
            nseg, srows = bm // (H * W), H
        elif (H * W) % bm == 0:
            nseg, srows = 1, (W + bm - 2) // W + 1
        else:
            return False
        pieces = 13 if wide else (9 if bm >= 128 else 7)
        return nseg * (srows + 2) * (W + 2) * (kc // 8) <= pieces * threads
    geom_ok = stride == 1 and W >= 8
    patch = geom_ok and geometry(False)
    patch_wide = geom_ok and not patch and (bn <= 64 or bm == 128) and geometry(True)
    run_geom = bm % W != 0 and bm % (H * W) != 0
    dma = not (run_geom and W >= 16)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    M = B * Ho * Wo
    if patch_wide:
        return "patch-dma-wide" if dma else "patch-wide"
    if patch and dma:
        return "patch-dma-deep" if M <= 1024 and -(-M // bm) * -(-cout // bn) * splits <= 384 else "patch-dma"
    return "patch" if patch else "per-tap"


def conv_plans(ops_slab_floats, shape):
    """The (bm, bn, splits) a conv case runs: every tile x {1, 2, 4, 16} under test_conv3x3_implicit_gemm's guards."""
    B, Cin, Cout, H, W, stride = shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    steps = 9 * Cin // 64
    out = []
    for bm, bn in CONV_TILES:
        for splits in CONV_SPLITS:
            if splits > steps:
                continue
            if splits > 1 and splits * (-(-B * Ho * Wo // bm) * bm) * (-(-Cout // bn) * bn) > ops_slab_floats:
                continue
            out.append((bm, bn, splits))
    return out


# ------------------------------------------------------------------------------------------------ inputs and fp64 references
def _conv_seed(shape):
    return 1000 + sum((i + 1) * 7919 * v for i, v in enumerate(shape)) % 100000


@functools.lru_cache(maxsize=None)
def conv_case(shape):
    """Inputs (fp64 CPU tensors, NCHW) and the references of every rounding point of conv_epilogue: acc, acc + bias,
    acc + bias + residual.  gy / dx: the backward to the input (stride 1), gy at the density the depth 9 Cout asks for given
    the weights' density."""
    B, Cin, Cout, H, W, stride = shape
    s = _conv_seed(shape)
    d = density(9 * Cin)
    x, w = t64(ternary((B, Cin, H, W), s, d)), t64(ternary((Cout, Cin, 3, 3), s + 1, d))
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    bias, res = t64(small_ints((Cout,), s + 2)), t64(small_ints((B, Cout, Ho, Wo), s + 3))
    acc = torch.nn.functional.conv2d(x, w, None, stride=stride, padding=1)
    with_bias = acc + bias[None, :, None, None]
    case = {"x": x, "w": w, "bias": bias, "res": res, "refs": {"plain": acc, "bias": with_bias, "bias+residual": with_bias + res}}
    if stride == 1:
        gy = t64(ternary((B, Cout, Ho, Wo), s + 4, partner_density(9 * Cout, d)))
        case["gy"] = gy
        case["dx"] = torch.nn.functional.conv_transpose2d(gy, w, None, stride=1, padding=1)
    return case


@functools.lru_cache(maxsize=None)
def up_case(shape):
    B, Cin, Cout, H, W = shape
    s = _conv_seed(shape) + 50
    d = density(9 * Cin)
    x, w = t64(ternary((B, Cin, H, W), s, d)), t64(ternary((Cout, Cin, 3, 3), s + 1, d))
    bias = t64(small_ints((Cout,), s + 2))
    up = torch.nn.functional.interpolate(x, scale_factor=2.0, mode="nearest")
    acc = torch.nn.functional.conv2d(up, w, None, padding=1)
    gy = t64(ternary((B, Cout, 2 * H, 2 * W), s + 4, partner_density(9 * Cout, d)))
    g_up = torch.nn.functional.conv_transpose2d(gy, w, None, stride=1, padding=1)
    dx = g_up.reshape(B, Cin, H, 2, W, 2).sum((3, 5))
    return {"x": x, "w": w, "bias": bias, "acc": acc, "y": acc + bias[None, :, None, None], "gy": gy, "g_up": g_up, "dx": dx}


@functools.lru_cache(maxsize=None)
def gemm_case(shape, std=STD):
    """X (M, K), W (N, K), bias (N,), residual (M, N) and acc = X W^T, + bias, + residual."""
    M, K, N = shape
    s = 3000 + (M * 31 + K * 17 + N) % 100000
    d = density(K, std)
    x, w = t64(ternary((M, K), s, d)), t64(ternary((N, K), s + 1, d))
    bias, res = t64(small_ints((N,), s + 2)), t64(small_ints((M, N), s + 3))
    acc = x @ w.T
    return {"x": x, "w": w, "bias": bias, "res": res, "acc": acc, "acc+bias": acc + bias, "acc+bias+res": acc + bias + res}


@functools.lru_cache(maxsize=None)
def thin_case(shape):
    """Both edge convolutions on one map: 4 -> C ("in") and C -> 4 ("out"), each with its backward to the input."""
    B, C, H, W = shape
    s = 5000 + (B * 13 + C * 7 + H * 3 + W) % 100000
    conv, convt = torch.nn.functional.conv2d, torch.nn.functional.conv_transpose2d
    out = {}
    for name, cin, cout, k in (("in", 4, C, 0), ("out", C, 4, 10)):
        d = density(9 * cin)
        x, w = t64(ternary((B, cin, H, W), s + k, d)), t64(ternary((cout, cin, 3, 3), s + k + 1, d))
        bias = t64(small_ints((cout,), s + k + 2))
        gy = t64(ternary((B, cout, H, W), s + k + 3, partner_density(9 * cout, d)))
        acc = conv(x, w, None, padding=1)
        out[name] = {"x": x, "w": w, "bias": bias, "gy": gy, "acc": acc, "y": acc + bias[None, :, None, None],
                     "dx": convt(gy, w, None, stride=1, padding=1)}
    return out


@functools.lru_cache(maxsize=None)
def ln_case(shape, parts):
    """The LayerNorm fold with FABRICATED row statistics: row m has mean in {-2 .. 2} and var + eps in {1, 1/4} (rstd 1 or 2),
    written as `parts` partial (sum, sum of squares) pairs per row whose totals are K mean and K (var + mean^2) — integers,
    spread unevenly (one part negative in the sums) so that a part read twice, skipped or taken from a neighbouring row
    changes the statistics.  colsum and shift are small integers; the reference rstd (acc - mean colsum) + shift is an
    integer.  The statistics need not be those of x: the kernel only ever sees the partial sums.

    Where the result is 0 nothing removes the f32 ulp of rstd (2^-24 (acc - mean colsum) is a value both storage types hold),
    and with mean != 0 the kernels' rstd IS an ulp off: var = s2 (1 / K) - mean^2 contracts into one fma, 1 / K is not an f32
    number for K = 5 * 2^n, and s2 / K is up to 5 times the variance.  So rows with mean != 0 all take rstd = 2 and every
    shift is odd — their results are odd, never 0 — and rows with mean = 0 (var = s2 (1 / K) rounds to the exact value, rstd
    is exactly 1 or 2) take either rstd.  Everywhere else the ulp moves the f32 value by less than 2^-21 * 264 = 1.3e-4,
    under the half spacing of f16 (2^-12 below 1) and bf16 at every non-zero integer."""
    M, K, N = shape
    c = gemm_case(shape, LN_STD)
    s = 7000 + (M * 31 + K * 17 + N + parts) % 100000
    mean = small_ints((M,), s, -2, 2)
    rstd = np.where(mean != 0, 2.0, 1.0 + (hashrand.hash_u32(M, s + 1) >> np.uint32(31)).astype(np.float64))
    var = 1.0 / (rstd * rstd) - LN_EPS
    tot1, tot2 = K * mean, K * (var + mean * mean)
    assert np.all(tot2 == np.round(tot2))
    partials = np.zeros((M, parts, 2))
    w1 = small_ints((M, parts), s + 2, -3, 3)
    w2 = small_ints((M, parts), s + 3, 0, 5)
    partials[:, :, 0], partials[:, :, 1] = w1, w2                          # arbitrary integers, the last part makes up the total
    partials[:, -1, 0] = tot1 - w1[:, :-1].sum(1)
    partials[:, -1, 1] = tot2 - w2[:, :-1].sum(1)
    assert np.all(partials[:, -1, 1] >= 0) and np.abs(partials).max() < F32_EXACT
    colsum, shift = small_ints((N,), s + 4, -4, 4), 2.0 * small_ints((N,), s + 5, -4, 3) + 1.0
    ref = t64(rstd)[:, None] * (c["acc"] - t64(mean)[:, None] * t64(colsum)[None, :]) + t64(shift)[None, :]
    return {"x": c["x"], "w": c["w"], "acc": c["acc"], "partials": t64(partials), "colsum": t64(colsum), "shift": t64(shift),
            "mean": t64(mean), "rstd": t64(rstd), "ref": ref}
