"""The same launch on the same bits gives the same bits: every entry point of the package, eight launches each.

Procedure of every case (`repeats`): the inputs are built once (hashrand); the entry point is launched eight times into freshly
allocated outputs; between two consecutive launches it is launched once on the same shapes with every floating input multiplied
by -3, so that scratch slabs, partial-sum workspaces, statistics buffers and the allocator's recycled blocks hold foreign values
when the next repeat starts; every returned tensor of every repeat — results, LSE, statistics, partial sums handed to a consumer,
absmean, packed maxima — must be `repro_trace.same_bits` with the first launch's.  Then one control: the lowest mantissa bit of one
input element is flipped and some output must NOT be same_bits (the comparison can fail).  Afterwards every arrival-ticket word is
zero.  Plans and shapes are the smallest members of the existing tests' lists that still put two or more workgroups on a reduction.

The one intended exception: `bias_grad`, the paint-with-words d loss / d coef that ga_attn_capture_bwd_biased(_grouped) sums with
float atomics — and with it the one D-vector per image that ga_attn_pww_max_grad adds to dQ FROM that sum.  They are the two
names in ATOMIC_OUTPUTS; the dQ the backward launch writes itself, and ga_attn_pww_max_grad on a fixed bias_grad, are compared."""
import ctypes
import math

import numpy as np
import pytest
import torch

import hashrand
import norm_inputs as N
import repro_trace as rt

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
HALF = ["f16", "bf16"]
LAUNCHES = 8
ATOMIC_OUTPUTS = ("bias_grad", "dq + max grad from bias_grad")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from guided_attention_amd import ops as _ops
    _ops.load()
    return _ops


def dev(a, dtype, nhwc=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)
    return t.contiguous(memory_format=torch.channels_last) if nhwc else t


def rnd(shape, seed, dtype, scale=1.0, shift=0.0, nhwc=False):
    return dev(hashrand.normalish(tuple(shape), seed) * scale + shift, dtype, nhwc)


def foreign(x):
    """Every floating tensor times -3 (same shape, strides' memory format and dtype); everything else as it is."""
    if torch.is_tensor(x):
        if not x.is_floating_point():
            return x
        y = (x.float() * -3.0).to(x.dtype)
        return y.contiguous(memory_format=torch.channels_last) if x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last) \
            else y
    if isinstance(x, (list, tuple)):
        return type(x)(foreign(v) for v in x)
    return x


def flip_lowest_mantissa_bit(t, element=0):
    ints = {2: torch.int16, 4: torch.int32}[t.element_size()]
    out = t.clone(memory_format=torch.preserve_format)
    flat = out.view(ints).reshape(-1) if out.is_contiguous() else out.permute(0, 2, 3, 1).view(ints).reshape(-1)
    flat[element] ^= 1
    assert not rt.same_bits(out, t.clone(memory_format=torch.preserve_format))
    return out


def named(out):
    """A launch's result -> {name: tensor}, None entries dropped."""
    if torch.is_tensor(out):
        out = {"out": out}
    elif not isinstance(out, dict):
        out = {f"out{i}": t for i, t in enumerate(out)}
    return {k: v.detach() for k, v in out.items() if v is not None}


def repeats(ops, what, launch, args, flip=0, exclude=(), control=True):
    """`launch(*args)` -> tensor, tuple or dict of fresh tensors.  See the module docstring.  control: False (another case of the
    family carries it), True, or the flat indices of input `flip` to try."""
    args = list(args)
    other = foreign(args)
    first = named(launch(*args))
    assert first and all(t.numel() for t in first.values()), what
    for i in range(1, LAUNCHES):
        named(launch(*other))
        again = named(launch(*args))
        assert sorted(again) == sorted(first), what
        bad = [f"{k} ({rt.differing_elements(first[k], again[k])} of {first[k].numel()} elements)"
               for k in first if k not in exclude and not rt.same_bits(first[k], again[k])]
        assert not bad, f"{what}: launch {i + 1} is not the first launch's bits in {', '.join(bad)}"
    if control:
        assert flipped_bit_shows(launch, args, first, flip, exclude, control), \
            f"{what}: no flipped input bit changed an output: the comparison cannot fail"
    assert ops.tickets_are_zero(), f"{what}: an arrival-ticket word is left non-zero"
    return first


CANDIDATES = 256


def flipped_bit_shows(launch, args, first, flip, exclude, elements):
    """The control: ONE input element's lowest mantissa bit flipped, everything else as it was -> some compared output is not
    same_bits with the first launch.  A result rounded to 16 bits, or a sum of hundreds of terms, absorbs most single-ulp changes
    of one operand, so elements are tried one at a time — those of `elements` when it is a list, else CANDIDATES spread over
    input `flip`, then over the other floating inputs — until one shows."""
    order = [flip] + [i for i in range(len(args)) if i != flip]
    for i in order:
        target = args[i][0] if isinstance(args[i], (list, tuple)) else args[i]
        if not (torch.is_tensor(target) and target.is_floating_point()):
            continue
        n = target.numel()
        picks = elements if isinstance(elements, (list, tuple)) and i == flip else \
            sorted({(j * n) // CANDIDATES for j in range(CANDIDATES)})
        for e in picks:
            moved = list(args)
            bent = flip_lowest_mantissa_bit(target, e)
            moved[i] = type(args[i])([bent] + list(args[i][1:])) if isinstance(args[i], (list, tuple)) else bent
            changed = named(launch(*moved))
            if any(not rt.same_bits(first[k], changed[k]) for k in first if k not in exclude):
                return True
    return False


# ------------------------------------------------------------------------------------------------ 3x3 convolution, GEMM
def conv_inputs(shape, T, stride=1):
    B, Cin, Cout, H, W = shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = rnd((B, Cin, H, W), 61 + Cin, T, nhwc=True)
    w = rnd((Cout, Cin, 3, 3), 62 + Cout, T, 1.0 / math.sqrt(9 * Cin))
    bias = rnd((Cout,), 63, T, 0.3)
    res = rnd((B, Cout, Ho, Wo), 64, T, nhwc=True)
    return x, w, bias, res


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("plan", [(64, 64, 4), (64, 64, 16), (128, 128, 2)], ids=lambda p: "x".join(map(str, p)))
def test_conv3x3_split_k(ops, plan, dt):
    """ga_conv3x3_nhwc with bias + residual: 4, 16 and 2 slices of the depth per tile handed over through slabs and tickets."""
    shape = (2, 128, 64, 16, 16)
    x, w, bias, res = conv_inputs(shape, DT[dt])
    wp = ops.conv3x3_packed_weights(w, False)
    ws = plan[2] * 2 * 16 * 16 * 64
    repeats(ops, f"conv3x3 {shape} {plan} {dt}",
            lambda x, wp, bias, res: ops.conv3x3_nhwc(x, wp, 64, 1, bias, res, plan=plan + (ws,)), (x, wp, bias, res))


@pytest.mark.parametrize("dt", HALF)
def test_conv3x3_stride_2(ops, dt):
    shape = (1, 64, 64, 16, 16)
    x, w, bias, res = conv_inputs(shape, DT[dt], 2)
    wp = ops.conv3x3_packed_weights(w, False)
    plan = (64, 64, 2, 2 * 8 * 8 * 64)
    repeats(ops, f"conv3x3 stride 2 {dt}", lambda x, wp, bias, res: ops.conv3x3_nhwc(x, wp, 64, 2, bias, res, plan=plan),
            (x, wp, bias, res))


@pytest.mark.parametrize("dt", HALF)
def test_conv3x3_group_norm_epilogue(ops, dt):
    """ga_conv3x3_nhwc_gn: the partial sums for the consuming GroupNorm are an output, and ga_group_norm_apply runs on them (the
    apply-from-partials form of the norm: y and its saved statistics)."""
    B, Cin, Cout, H, W, G = N.CONV_GN
    T = DT[dt]
    x, w, bias, res = conv_inputs((B, Cin, Cout, H, W), T)
    cb = rnd((B, Cout), 164, T, 0.7)
    gamma, beta = rnd((Cout,), 165, T, 0.3, 1.0), rnd((Cout,), 166, T, 0.2)
    wp = ops.conv3x3_packed_weights(w, False)
    plan = (128, 128, 2, 2 * B * H * W * Cout)

    def launch(x, wp, bias, res, cb, gamma, beta):
        y, made = ops.conv3x3_nhwc(x, wp, Cout, 1, bias, res, plan=plan, gn=(G, cb))
        assert made is not None, "the epilogue form does not serve this shape"
        z = ops.GroupNormAct.apply(y.requires_grad_(True), gamma, beta, G, N.EPS, True, cb, False, made)
        return {"y": y, "partials": made[0], "norm": z, "stats": z.grad_fn.saved_tensors[3]}

    repeats(ops, f"conv3x3 gn epilogue + apply {dt}", launch, (x, wp, bias, res, cb, gamma, beta))


@pytest.mark.parametrize("dt", HALF)
def test_conv3x3_backward_pack(ops, dt):
    """The transposed, flipped pack (ga_conv3x3_pack_weights) and the backward-to-input launch on it, through the autograd
    wrapper with the planner's own plan."""
    T = DT[dt]
    x, w, bias, res = conv_inputs((2, 128, 64, 16, 16), T)
    gy = rnd((2, 64, 16, 16), 65, T, nhwc=True)

    def launch(x, w, gy):
        w = w.clone()                   # a new tensor: the pack cache is keyed on the tensor object, so the pack is made again
        pack = ops.conv3x3_packed_weights(w, True)
        xa = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
        ops.conv3x3(xa, w, None, None, 1).backward(gy)
        return {"pack": pack, "dx": xa.grad}

    repeats(ops, f"conv3x3 backward {dt}", launch, (x, w, gy), flip=1)


@pytest.mark.parametrize("dt", HALF)
def test_conv3x3_up2x(ops, dt):
    T = DT[dt]
    x, w, bias, _ = conv_inputs((1, 128, 64, 8, 8), T)
    wp = ops.conv3x3_packed_weights(w, False)

    def launch(x, wp, bias):
        y = ops.conv3x3_up2x_nhwc(x, wp, 64, bias)
        assert y is not None, "the up-sampling patch kernel does not serve this shape"
        return y

    repeats(ops, f"conv3x3_up2x {dt}", launch, (x, wp, bias))


@pytest.mark.parametrize("dt", HALF)
def test_gemm_nt_split_k(ops, dt):
    from guided_attention_amd._lib import dtype_code, load, stream_ptr
    M, K, Nn, splits = 130, 192, 264, 3
    T = DT[dt]
    x, w = rnd((M, K), 71, T), rnd((Nn, K), 72, T, 1.0 / math.sqrt(K))
    bias, res = rnd((Nn,), 73, T, 0.3), rnd((M, Nn), 74, T)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731

    for bm, bn in ((128, 128), (64, 64)):
        def launch(x, w, bias, res):
            y = torch.empty(M, Nn, device="cuda", dtype=T)
            ws, tickets = ops.splitk_workspace(x.device, M, Nn, bm, bn, splits)
            assert load().ga_gemm_nt(P(x), P(w), P(y), P(ws), P(tickets), P(bias), P(res), M, K, Nn, bm, bn, splits, dtype_code(x),
                                     stream_ptr()) == 0
            return y

        repeats(ops, f"gemm_nt {bm}x{bn} splits {splits} {dt}", launch, (x, w, bias, res))


# ------------------------------------------------------------------------------------------------ Linear
LIN = (130, 192, 264)            # the smallest member of test_kernels_gpu.LIN_SHAPES whose depth (3 steps of 64) can be split
# the smallest member of test_kernels_gpu.STREAM_CASES, and the smallest with GEGLU
STREAM = [(130, 384, 264, (128, 128), False), (1000, 320, 1008, (64, 64), True)]


def fold(w, bias, gamma, beta, T):
    wg = (w.float() * gamma.float()[None, :]).to(T)
    return wg, wg.float().sum(1), (w.float() @ beta.float()) + bias.float()


@pytest.mark.parametrize("dt", HALF)
def test_linear_fused_split_k(ops, dt):
    """ga_linear_fused, two slices of the depth: bias + residual with the row partial sums it leaves for a LayerNorm (an output
    handed to a consumer), GEGLU with the pre-activation copy, and the LayerNorm fold with its (mean, rstd) output."""
    M, K, Nn = LIN
    T = DT[dt]
    x = rnd((M, K), 70 + M, T, 1.5, 0.3)
    w, bias = rnd((Nn, K), 71 + Nn, T, K ** -0.5), rnd((Nn,), 72, T, 0.3)
    res = rnd((M, Nn), 73, T)
    w0 = rnd((K, K), 76, T, K ** -0.5)
    gamma, beta = rnd((K,), 74, T, 0.2, 1.0), rnd((K,), 75, T, 0.2)
    w2, bias2 = rnd((256, K), 78, T, K ** -0.5), rnd((256,), 79, T, 0.3)      # GEGLU takes N % 16 == 0
    for plan in ((64, 64, 2, 0), (128, 128, 2, 2)):
        def plain(x, w, bias, res):
            return ops.linear_fused(x, w, bias, residual=res, plan=plan)["y"]

        def producer(x, w0):
            out = ops.linear_fused(x, w0, None, residual=x, want_row_partials=True, plan=plan)
            return {"y": out["y"], "row_partials": out["row_partials"]}

        def geglu(x, w, bias):
            out = ops.linear_fused(x, w, bias, geglu=True, want_preact=True, plan=plan)
            return {"y": out["y"], "preact": out["preact"]}

        repeats(ops, f"linear bias + residual {plan} {dt}", plain, (x, w, bias, res))
        made = repeats(ops, f"linear row partials {plan} {dt}", producer, (x, w0))
        repeats(ops, f"linear geglu {plan} {dt}", geglu, (x, w2, bias2))
        h, partials = made["y"], made["row_partials"]
        wg, colsum, shift = fold(w, bias, gamma, beta, T)
        wg2, colsum2, shift2 = fold(w2, bias2, gamma, beta, T)

        def folded(h, wg, partials, colsum, shift):
            out = ops.linear_fused(h, wg, None, ln=(partials, colsum, shift, 1e-5), want_ln_stats=True, plan=plan)
            return {"y": out["y"], "ln_stats": out["ln_stats"]}

        def folded_geglu(h, wg, partials, colsum, shift):
            return ops.linear_fused(h, wg, None, geglu=True, ln=(partials, colsum, shift, 1e-5), plan=plan)["y"]

        repeats(ops, f"linear LayerNorm fold {plan} {dt}", folded, (h, wg, partials, colsum, shift))
        repeats(ops, f"linear LayerNorm fold + geglu {plan} {dt}", folded_geglu, (h, wg2, partials, colsum2, shift2))


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("case", STREAM, ids=lambda c: "x".join(map(str, c[:3])) + ("-geglu" if c[4] else ""))
def test_linear_stream_form(ops, case, dt):
    M, K, Nn, ptile, geglu = case
    T = DT[dt]
    x0 = rnd((M, K), 150 + M, T, 1.3, 0.4)
    w0 = rnd((K, K), 151, T, K ** -0.5)
    prod = ops.linear_fused(x0, w0, None, residual=x0, want_row_partials=True, plan=ptile + (1,))
    h, partials = prod["y"], prod["row_partials"]
    assert ops.linear_stream_serves(K, partials.shape[1], True, None, None, False, False, False)
    gamma, beta = rnd((K,), 152, T, 0.2, 1.0), rnd((K,), 153, T, 0.2)
    w, bias = rnd((Nn, K), 154, T, K ** -0.5), rnd((Nn,), 155, T, 0.3)
    wg, colsum, shift = fold(w, bias, gamma, beta, T)
    repeats(ops, f"linear stream form {case} {dt}",
            lambda h, wg, partials, colsum, shift: ops.linear_fused(h, wg, None, geglu=geglu, ln=(partials, colsum, shift, 1e-5),
                                                                    plan=ops.LINEAR_STREAM_PLAN)["y"],
            (h, wg, partials, colsum, shift))


@pytest.mark.parametrize("dt", HALF)
def test_linear_group_norm_row_partials(ops, dt):
    """ga_linear_fused with gn_partials: the per-(image, m tile, group) sums for the consuming GroupNorm, with split-K."""
    B, HW, K, Nn, groups = 2, 256, 128, 192, 8      # the smallest case of test_linear_epilogue_takes_the_consuming_group_norm_...
    T = DT[dt]
    x, w = rnd((B * HW, K), 180 + K, T), rnd((Nn, K), 181, T, 1.0 / math.sqrt(K))
    bias, res = rnd((Nn,), 182, T, 0.3), rnd((B * HW, Nn), 183, T, 1.5, 0.3)
    served = 0
    for plan in ((128, 128, 2, 2), (64, 64, 2, 4)):
        if not ops.load().ga_linear_gn_blocks(HW, Nn, groups, plan[0], plan[1]):
            continue
        served += 1

        def launch(x, w, bias, res):
            out = ops.linear_fused(x, w, bias, residual=res, plan=plan, gn=(groups, HW))
            return {"y": out["y"], "gn_partials": out["gn"][0]}

        repeats(ops, f"linear gn partials {plan} {dt}", launch, (x, w, bias, res))
    assert served


@pytest.mark.parametrize("dt", HALF)
def test_linear_autograd_backward(ops, dt):
    """The Linear's backward through its autograd wrapper (fused_linear.linear): dX = dY W on the same kernel (N a multiple of
    64: it is the depth of that product), under the planner's own plans."""
    from guided_attention_amd import fused_linear
    M, K, Nn = 130, 192, 256
    T = DT[dt]
    x, w, bias = rnd((1, M, K), 70 + M, T, 1.5, 0.3), rnd((Nn, K), 71 + Nn, T, K ** -0.5), rnd((Nn,), 72, T, 0.3)
    gy = rnd((1, M, Nn), 77, T)
    assert fused_linear.supported(x, K, Nn)

    def launch(x, w, bias, gy):
        xa = x.clone().requires_grad_(True)
        y, _ = fused_linear.linear(xa, w, bias)
        y.backward(gy)
        return {"y": y, "dx": xa.grad}

    repeats(ops, f"fused_linear.linear forward + backward {dt}", launch, (x, w, bias, gy))


# ------------------------------------------------------------------------------------------------ GroupNorm
GN_SHAPES = [((2, 64, 4, 4, 8), "one launch"), ((2, 288, 9, 9, 32), "two launches, wide"), ((2, 99, 5, 7, 33), "two launches, narrow")]


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("case", GN_SHAPES, ids=lambda c: c[1])
def test_group_norm_forward_and_backward(ops, case, dt):
    """ga_group_norm_fwd (y and the saved statistics) and ga_group_norm_bwd with the skip connection's gradient (g_res), one
    shape per launch form of tests/norm_inputs.py (the apply-from-partials form: test_conv3x3_group_norm_epilogue)."""
    (B, C, H, W, G), form = case
    T = DT[dt]
    assert (N.gn_form(H * W, C, G, dt)[0] == "small") == (form == "one launch")
    x, g, g2 = (rnd((B, C, H, W), 200 + i, T, nhwc=True) for i in range(3))
    w, b, cb = rnd((C,), 203, T, 0.3, 1.0), rnd((C,), 204, T, 0.2), rnd((B, C), 205, T, 0.7)

    def launch(x, w, b, cb, g, g2):
        xa = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
        y, alias = ops.group_norm_act(xa, w, b, G, N.EPS, True, cb, True)
        stats = y.grad_fn.saved_tensors[3]
        torch.autograd.backward([y, alias], [g, g2])
        return {"y": y, "stats": stats, "dx": xa.grad}

    repeats(ops, f"group norm {form} {dt}", launch, (x, w, b, cb, g, g2))


@pytest.mark.parametrize("dt", HALF)
def test_cat_group_norm_one_launch(ops, dt):
    B, C1, C2, H, W, G = N.CAT_SMALL[0]
    T = DT[dt]
    a, b = rnd((B, C1, H, W), 210, T, nhwc=True), rnd((B, C2, H, W), 211, T, 1.7, 0.4, nhwc=True)
    gamma, beta = rnd((C1 + C2,), 212, T, 0.3, 1.0), rnd((C1 + C2,), 213, T, 0.2)

    def launch(a, b, gamma, beta):
        y = ops.cat_channels(a, b, gn_for=G, norm=(gamma, beta, N.EPS, True))
        out, stats = y._ga_gn["done"]
        return {"cat": y, "norm": out, "stats": stats}

    repeats(ops, f"cat + group norm, one launch {dt}", launch, (a, b, gamma, beta))


@pytest.mark.parametrize("dt", HALF)
def test_cat_channels_gn(ops, dt):
    B, C1, C2, H, W, G = N.CAT_WIDE[1]
    T = DT[dt]
    a, b = rnd((B, C1, H, W), 214, T, nhwc=True), rnd((B, C2, H, W), 215, T, 1.7, 0.4, nhwc=True)

    def launch(a, b):
        y = ops.cat_channels(a, b, gn_for=G)
        return {"cat": y, "partials": y._ga_gn["partials"]}

    repeats(ops, f"cat_channels_gn {dt}", launch, (a, b))


# ------------------------------------------------------------------------------------------------ flash self-attention
@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("shape", [(1, 2, 130, 64), (2, 3, 77, 40)], ids=lambda s: "x".join(map(str, s)))
def test_self_attention(ops, shape, dt):
    """ga_self_attn_fwd / _capture_fwd / _probs / _bwd / _bwd_dp: O, LSE, P, dQ, dK, dV."""
    B, H, Nq, D = shape
    T = DT[dt]
    scale = D ** -0.5
    q, k, v, d_o = (rnd((B, Nq, H * D), 300 + i, T) for i in range(4))
    dp = rnd((B * H, Nq, Nq), 304, T, 0.5)
    what = f"self attention {shape} {dt}"
    fwd = repeats(ops, what + " fwd", lambda q, k, v: dict(zip(("o", "lse"), ops.self_attn_fwd(q, k, v, H, scale))), (q, k, v))
    cap = repeats(ops, what + " capture fwd",
                  lambda q, k, v: dict(zip(("o", "lse", "p"), ops.self_attn_capture_fwd(q, k, v, H, scale))), (q, k, v))
    o, lse = fwd["o"], fwd["lse"]
    assert rt.same_bits(cap["lse"], lse.clone())
    repeats(ops, what + " probs", lambda q, k, lse: ops.self_attn_probs(q, k, lse, H, scale), (q, k, lse))
    repeats(ops, what + " bwd", lambda q, k, v, o, d_o, lse: dict(zip(("dq", "dk", "dv"),
                                                                     ops.self_attn_bwd(q, k, v, o, d_o, lse, H, scale))),
            (q, k, v, o, d_o, lse))
    repeats(ops, what + " bwd_dp", lambda q, k, v, o, d_o, lse, dp: dict(zip(("dq", "dk", "dv"),
                                                                            ops.self_attn_bwd(q, k, v, o, d_o, lse, H, scale, dp))),
            (q, k, v, o, d_o, lse, dp))


@pytest.mark.parametrize("dt", HALF)
def test_attn_wide_fwd(ops, dt):
    B, H, Nq, D = 2, 1, 200, 512
    q, k, v = (rnd((B, Nq, H * D), 310 + i, DT[dt], 0.5) for i in range(3))
    repeats(ops, f"attn_wide_fwd {dt}", lambda q, k, v: ops.attn_wide_fwd(q, k, v, H), (q, k, v))


# ------------------------------------------------------------------------------------------------ cross-attention capture
CAP = dict(B=3, H=2, N=80, Kt=77, D=40, G=3)


def capture_inputs(T):
    c = CAP
    C = c["H"] * c["D"]
    q, d_o = rnd((c["B"], c["N"], C), 320, T, 0.6), rnd((c["B"], c["N"], C), 323, T)
    k, v = rnd((c["B"], c["Kt"], C), 321, T, 0.6), rnd((c["B"], c["Kt"], C), 322, T)
    dp = rnd((c["B"] * c["H"], c["N"], c["Kt"]), 324, T, 0.5)
    mask = dev(np.stack([(hashrand.uniform((c["N"], c["Kt"]), 330 + g) > 0.6).astype(np.float32) * (0.8 - 0.2 * g)
                         for g in range(c["G"])]), T)
    return q, k, v, d_o, dp, mask


@pytest.mark.parametrize("dt", ["f32"] + HALF)
def test_attn_capture_plain(ops, dt):
    H, scale = CAP["H"], CAP["D"] ** -0.5
    q, k, v, d_o, dp, _ = capture_inputs(DT[dt])
    repeats(ops, f"attn_capture_fwd {dt}", lambda q, k, v: dict(zip(("o", "p"), ops.attn_capture_fwd(q, k, v, H, scale, True))),
            (q, k, v))
    repeats(ops, f"attn_capture_bwd {dt}", lambda q, k, v, d_o, dp: ops.attn_capture_bwd(q, k, v, d_o, dp, H, scale),
            (q, k, v, d_o, dp))
    # the maximum moves only with the query row (and head) it lies in: the control flips that row's elements.  In f32 one ulp of
    # one of 40 products is below the rounding of their sum, and in bf16 below the rounding of the score (the kernels round the
    # scores to the operands' type, as the reference's half-precision baddbmm does): the f16 case carries these two entries' control
    bh, rest = divmod(int(ops.attn_scores_max(q, k, H, scale)[1]), CAP["N"] * CAP["Kt"])
    b, h, n = bh // H, bh % H, rest // CAP["Kt"]
    row = [(b * CAP["N"] + n) * H * CAP["D"] + h * CAP["D"] + d for d in range(CAP["D"])] if dt == "f16" else False
    repeats(ops, f"attn_scores_max {dt}", lambda q, k: dict(zip(("value", "index"), ops.attn_scores_max(q, k, H, scale))), (q, k),
            control=row)
    repeats(ops, f"attn_scores_max_grouped {dt}", lambda q, k: ops.attn_scores_max_grouped(q, k, H, scale, CAP["G"]), (q, k),
            control=row)


@pytest.mark.parametrize("dt", ["f32"] + HALF)
def test_attn_capture_biased(ops, dt):
    """The paint-with-words forms.  bias_grad (d loss / d coef) is summed with float atomics — the one intended exception — and
    is not compared; dQ as the backward launch writes it does not depend on it and is."""
    H, G, scale = CAP["H"], CAP["G"], CAP["D"] ** -0.5
    q, k, v, d_o, dp, mask = capture_inputs(DT[dt])
    coef = torch.tensor([0.7], dtype=torch.float32, device="cuda")
    mult = torch.tensor([0.5, 0.3, 0.8], dtype=torch.float32, device="cuda")
    packed = ops.attn_scores_max_grouped(q, k, H, scale, G)
    fixed_grad = torch.tensor([0.25, -1.5, 0.75], dtype=torch.float32, device="cuda")

    def bwd_biased(q, k, v, d_o, dp, bias, coef):
        dq, gsum = ops.attn_capture_bwd_biased(q, k, v, d_o, dp, H, scale, bias, coef)
        return {"dq": dq, "bias_grad": gsum}

    def bwd_grouped(q, k, v, d_o, dp, bias, mult):
        dq, gsum = ops.attn_capture_bwd_biased_grouped(q, k, v, d_o, dp, H, scale, bias, packed, mult)
        full = ops.attn_pww_max_grad(dq.clone(), k, packed, gsum, mult, H, scale)
        return {"dq": dq, "bias_grad": gsum, "dq + max grad from bias_grad": full}

    repeats(ops, f"capture fwd biased {dt}",
            lambda q, k, v, bias, coef: dict(zip(("o", "p"), ops.attn_capture_fwd_biased(q, k, v, H, scale, True, bias, coef))),
            (q, k, v, mask[0], coef))
    repeats(ops, f"capture bwd biased {dt}", bwd_biased, (q, k, v, d_o, dp, mask[0], coef), exclude=ATOMIC_OUTPUTS)
    repeats(ops, f"capture fwd grouped {dt}",
            lambda q, k, v, bias, mult: dict(zip(("o", "p"), ops.attn_capture_fwd_biased_grouped(q, k, v, H, scale, True, bias, packed,
                                                                                                mult))), (q, k, v, mask, mult))
    repeats(ops, f"capture bwd grouped {dt}", bwd_grouped, (q, k, v, d_o, dp, mask, mult), exclude=ATOMIC_OUTPUTS)
    # the in-place launch itself, on a bias_grad that is an input: every bit
    dq0 = ops.attn_capture_bwd_biased_grouped(q, k, v, d_o, dp, H, scale, mask, packed, mult)[0]
    repeats(ops, f"attn_pww_max_grad {dt}",
            lambda dq, k, grad, mult: ops.attn_pww_max_grad(dq.clone(), k, packed, grad, mult, H, scale), (dq0, k, fixed_grad, mult),
            flip=2)


# ------------------------------------------------------------------------------------------------ loss
RES, KT = 16, 77
LAYOUT = (8, 8, 5)       # head-maps per stored map


def loss_maps(S, T, seed=400):
    from test_loss_plans_gpu import softmax_maps
    return [softmax_maps((S * h, RES * RES, KT), seed + i, 3.0).to("cuda", T) for i, h in enumerate(LAYOUT)]


def loss_plan(ops, T=3):
    from test_loss_plans_gpu import entries_of, plans_of
    return plans_of(ops, entries_of(T))[0]


@pytest.mark.parametrize("dt", ["f32"] + HALF)
@pytest.mark.parametrize("aligned", [True, False], ids=["plan 1x256", "misaligned: plan 1x0"])
def test_loss_solo(ops, aligned, dt):
    """ga_aggregate_loss_fwd / ga_smooth_loss_fwd / ga_smooth_loss_bwd at res 16 under both LDS plans a res-16 launch can take
    (the columns resident and the rows staged; a misaligned A: nothing staged)."""
    from test_loss_plans_gpu import BWD, FWD, expect_plan, misaligned_copy
    T = DT[dt]
    plan, maps = loss_plan(ops), loss_maps(1, T)
    repeats(ops, f"aggregate_loss_fwd {dt}", lambda maps: dict(zip(("A", "terms", "loss"),
                                                                  ops.aggregate_loss_fwd(list(maps), RES, 1, KT - 1, plan))), (maps,))
    A = ops.aggregate_loss_fwd(maps, RES, 1, KT - 1, plan)[0]
    dloss = torch.tensor([1.5], dtype=torch.float32, device="cuda")

    def place(A):
        return A.contiguous() if aligned else misaligned_copy(A)

    want = (1, 256) if aligned else (1, 0)
    expect_plan(ops, "res 16", FWD, want, res=RES, Kt=KT, slots=3, A=place(A))
    expect_plan(ops, "res 16", BWD, want, res=RES, Kt=KT, slots=3, A=place(A))
    # every term is a sum over the 256 pixels of a guided column: the control flips that column's elements, one pixel at a time
    column = [p * KT + 2 for p in range(RES * RES)]
    repeats(ops, f"smooth_loss_fwd {want} {dt}",
            lambda A: dict(zip(("terms", "loss"), ops.smooth_loss_fwd(place(A), RES, 1, KT - 1, plan))), (A,), control=column)
    repeats(ops, f"smooth_loss_bwd {want} {dt}",
            lambda A, dloss: dict(zip(("dA", "dP"), ops.smooth_loss_bwd(place(A), RES, 1, KT - 1, plan, dloss, T, .125))), (A, dloss))


@pytest.mark.parametrize("dt", ["f32"] + HALF)
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "misaligned"])
def test_loss_batched_and_tables(ops, aligned, dt):
    """The batched, image-table and relation-table launches, S = 3 at res 16, forward and backward; the backward also on a
    misaligned A (the plan that stages nothing)."""
    from test_loss_plans_gpu import REL_ENTRIES, REL_RELATIONS, TABLE_ROWS, misaligned_copy, plans_of
    T, S = DT[dt], 3
    maps = loss_maps(S, T, 410)
    plan = loss_plan(ops)
    dloss = torch.tensor([1.5, 0.0, 0.75], dtype=torch.float32, device="cuda")
    names = ("A", "terms", "loss", "rel_terms", "rel_loss")

    def place(A):
        return A.contiguous() if aligned else misaligned_copy(A)

    rows = TABLE_ROWS[:S]
    table = ops.ImageTable(S, 4, RES, True, .5, 3, torch.device("cuda", torch.cuda.current_device())).set(
        [plans_of(ops, e, over, avg)[0] for e, over, _, avg in rows], [(1, last) for _, _, last, _ in rows])
    rel_table = ops.ImageTable(S, 4, RES, True, .5, 3, torch.device("cuda", torch.cuda.current_device()), Q_max=4).set(
        [plans_of(ops, REL_ENTRIES)[0]] * S, [(1, KT - 1)] * S, [ops.RelationPlan(REL_RELATIONS), None, ops.RelationPlan(REL_RELATIONS[:1])])
    forms = {
        "batched": (lambda maps: ops.aggregate_loss_fwd_batched(list(maps), S, RES, 1, KT - 1, plan),
                    lambda A, dl: ops.smooth_loss_bwd_batched(place(A), RES, 1, KT - 1, plan, dl, T, .125)),
        "images": (lambda maps: ops.aggregate_loss_fwd_images(list(maps), table),
                   lambda A, dl: ops.smooth_loss_bwd_images(place(A), table, dl, T, .125)),
        "relation": (lambda maps: ops.aggregate_loss_rel_fwd_images(list(maps), rel_table),
                     lambda A, dl: ops.smooth_loss_rel_bwd_images(place(A), rel_table, dl, T, .125)),
    }
    for form, (fwd, bwd) in forms.items():
        if aligned:    # the forward allocates its own (aligned) A
            repeats(ops, f"loss {form} fwd {dt}", lambda maps: dict(zip(names, fwd(maps))), (maps,))
        A = fwd(maps)[0]
        repeats(ops, f"loss {form} bwd {dt}", lambda A, dl: dict(zip(("dA", "dP"), bwd(A, dl))), (A, dloss))


# ------------------------------------------------------------------------------------------------ elementwise and the rest
@pytest.mark.parametrize("dt", ["f32"] + HALF)
def test_layer_norm_geglu_and_adds(ops, dt):
    T = DT[dt]
    a, x, g1, g2 = (rnd((3, 5, 64), 500 + i, T) for i in range(4))
    w, b = rnd((64,), 504, T, 0.3, 1.0), rnd((64,), 505, T, 0.2)

    def add_ln(a, x, w, b, g1, g2):
        aa, xa = a.clone().requires_grad_(True), x.clone().requires_grad_(True)
        xnew, y = ops.add_layer_norm(aa, xa, w, b, 1e-5)
        torch.autograd.backward([xnew, y], [g1, g2])
        return {"xnew": xnew, "y": y, "da": aa.grad}

    repeats(ops, f"add_layer_norm {dt}", add_ln, (a, x, w, b, g1, g2))
    proj, dy = rnd((3, 7, 64), 506, T), rnd((3, 7, 32), 507, T)
    repeats(ops, f"geglu {dt}", lambda x, dy: {"y": ops.geglu(x), "dx": ops.geglu_backward(x, dy)}, (proj, dy))
    y, res = rnd((1, 64, 3, 5), 508, T, nhwc=True), rnd((1, 64, 3, 5), 509, T, nhwc=True)
    repeats(ops, f"bias_residual_add {dt}", lambda y, bias, res: ops.bias_residual_add(y, bias, res), (y, b, res))
    c1, c2 = rnd((1, 8, 3, 5), 510, T, nhwc=True), rnd((1, 16, 3, 5), 511, T, nhwc=True)
    assert ops.cat_channels_supported(c1, c2)
    repeats(ops, f"cat_channels {dt}", lambda a, b: ops.cat_channels(a, b), (c1, c2))


@pytest.mark.parametrize("dt", HALF)
def test_thin_convolutions(ops, dt):
    B, C, H, W = 2, 64, 5, 16
    T = DT[dt]
    for cin, cout in ((4, C), (C, 4)):
        x = rnd((B, cin, H, W), 520 + cin, T, nhwc=cin == C)
        w, bias = rnd((cout, cin, 3, 3), 521, T, 1.0 / math.sqrt(9 * cin)), rnd((cout,), 522, T, 0.3)
        gy = rnd((B, cout, H, W), 523, T, nhwc=cout == C)
        assert ops.conv3x3_thin_supported(x, w)

        def launch(x, w, bias, gy):
            xa = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
            y = ops.conv3x3_thin_apply(xa, w.clone(), bias)
            y.backward(gy)
            return {"y": y, "dx": xa.grad}

        repeats(ops, f"thin convolution {cin} -> {cout} {dt}", launch, (x, w, bias, gy))


@pytest.mark.parametrize("dt", ["f32"] + HALF)
def test_latent_entries(ops, dt):
    """The latent update, renoise and CFG + DDIM entries: solo at n = 4 * 128 * 128 + 3 (absmean is a reduction over every
    block), batched and masked at S = 3, every prediction type, eta = 0 and eta > 0."""
    T = DT[dt]
    n = 4 * 128 * 128 + 3
    x, g, e0, e1, noise = (rnd((n,), 600 + i, T) for i in range(5))
    repeats(ops, f"latent_axpy {dt}", lambda x, g: dict(zip(("out", "absmean"), ops.latent_axpy(x, g, 20.0, True))), (x, g))
    repeats(ops, f"latent_axpby {dt}", lambda x, y: ops.latent_axpby(x, y, 0.9, 0.4), (x, g))
    vel = rnd((n,), 605, torch.float32)

    def momentum(x, g, vel):
        vel = vel.clone()
        return {"out": ops.latent_sgd_momentum(x, g, vel, 0.1, 0.9, False), "velocity": vel}

    repeats(ops, f"latent_sgd_momentum {dt}", momentum, (x, g, vel))
    xs, gs, e0s, e1s, ns = (rnd((3, 4, 16, 16), 610 + i, T) for i in range(5))
    vels = rnd((3, 4, 16, 16), 615, torch.float32)
    active = torch.tensor([1, 0, 1], dtype=torch.int32, device="cuda")
    step = torch.tensor([20.0, 5.0, 10.0], dtype=torch.float32, device="cuda")
    first = torch.tensor([0, 0, 1], dtype=torch.int32, device="cuda")
    repeats(ops, f"latent_axpy_batched {dt}",
            lambda x, g, step: dict(zip(("out", "absmean"), ops.latent_axpy_batched(x, g, step, active, True))), (xs, gs, step))
    repeats(ops, f"latent_axpby_masked {dt}", lambda x, y: ops.latent_axpby_masked(x, y, 0.9, 0.4, active), (xs, gs))

    def momentum_batched(x, g, vel, lr):
        vel = vel.clone()
        return {"out": ops.latent_sgd_momentum_batched(x, g, vel, lr, 0.9, first, active), "velocity": vel}

    repeats(ops, f"latent_sgd_momentum_batched {dt}", momentum_batched, (xs, gs, vels, step))
    for prediction in ("epsilon", "v_prediction", "sample"):
        for eta in (0.0, 0.5):
            kw = dict(want_x0=True, prediction=prediction, eta=eta)
            repeats(ops, f"cfg_ddim_step {prediction} eta {eta} {dt}",
                    lambda e0, e1, x, z: dict(zip(("prev", "x0"), ops.cfg_ddim_step(e0, e1, 7.5, x, 0.4, 0.6, noise=z, **kw))),
                    (e0, e1, x, noise))
            repeats(ops, f"cfg_ddim_step_masked {prediction} eta {eta} {dt}",
                    lambda e0, e1, x, z: dict(zip(("prev", "x0"), ops.cfg_ddim_step_masked(e0, e1, 7.5, x, 0.4, 0.6, active, noise=z,
                                                                                         **kw))), (e0s, e1s, xs, ns))
    lat = rnd((2, 4, 8, 8), 620, T)
    w4, b4 = rnd((4, 4, 1, 1), 621, T, 0.5), rnd((4,), 622, T, 0.3)
    repeats(ops, f"latent_affine4 {dt}", lambda x, w, b: ops.latent_affine4(x, w, b, 1.0 / 0.18215), (lat, w4, b4))
