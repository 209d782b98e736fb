"""The wiring of the attention fronts: each public Function (AttnCapture*, SelfAttention*) is one private Function over one
forward and one backward launch helper per family.  What is pinned here is that wiring, not the kernels' arithmetic: a front
gives, bit for bit, what the functional wrappers give when they are called by hand in the documented order, and it makes the
launches — as the census sees them — that are written out below as literals.  Needs an MI355X.

Cross-attention shapes (B, H, N, Kt, D): (4, 2, 70, 77, 40) f16 — a partial second 64-row tile, NK = 3, two groups of two batch
rows, image stride != head stride; (2, 1, 64, 77, 16) bf16 — a square map, which the batched loss needs.  The per-image
cotangent is the one a batched _FusedLoss.backward hands over through the image-broadcast table; the loss refuses a map of 70
pixels (not a square), so at that shape the table entry is made by hand, laid out as _FusedLoss.backward lays it out.
Everything is compared bit for bit except the one row of dq per image that takes the gradient through the maximum: that
gradient is a multiple of d loss / d coef, which the backward kernels accumulate with float atomics (two runs of one wrapper
on the same inputs differ in its last bits, on this change and before it); those rows are held to two roundings of the dtype.

Self-attention shapes (B, H, N, D): (2, 3, 100, 16) and (1, 2, 64, 40), f16, as in test_self_attn_bwd_dp_gpu.  The fused and
the separate layouts are bit-equal for the capture forward and the backward with a cotangent on the probabilities, as they are
for the plain kernels (test_self_attention_fused_qkv_matches_separate), so torch.equal is what is asserted."""
import numpy as np
import pytest
import torch

import hashrand
from oracle import loss as oloss
from test_kernels_gpu import DT, dev, make_qkv
from test_output_bounds_gpu import ENTRIES
from test_self_attn_capture_gpu import qkv_inputs

pytestmark = pytest.mark.gpu

ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)  # noqa: E731


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from guided_attention_amd import ops as _ops
    _ops.load()
    _ops.prepare_device("cuda")
    return _ops


# ===================================================================================== cross-attention capture
CROSS = [((4, 2, 70, 77, 40), "f16"), ((2, 1, 64, 77, 16), "bf16")]
FRONTS = {"AttnCapture": ("none", "dense", "stride0", "per_image"),
          "AttnCapturePaintWithWords": ("none", "dense", "stride0"),          # the solo form's entry takes no image stride
          "AttnCapturePaintWithWordsImages": ("none", "dense", "stride0", "per_image")}
CROSS_CASES = [(s, dt, f, want, c) for s, dt in CROSS for f, cots in FRONTS.items()
               for want, c in [(False, "none")] + [(True, c) for c in cots]]
MULT = 0.3


def _masks(G, N, Kt, T):
    m = np.zeros((G, N, Kt), np.float32)
    for g in range(G):
        m[g, 3:13, 2 + g:9 + g] = 1.0
    return dev(m, T)


def _max_rows(idx, H, N, Kt):
    """Flat indices into [B*heads][N][Kt] -> the rows of dq, viewed (B*N*heads, D), that get the gradient through a maximum."""
    bh, n = idx // (N * Kt), idx % (N * Kt) // Kt
    return (bh // H * N + n) * H + bh % H


def _by_hand(ops, front, q, k, v, H, scale, want, bias, mult):
    """-> (o, probs, backward(d_o, d_probs) -> (dq, dq before the gradient through the maximum, the rows that gradient lands
    on)): the functional wrappers in the order the front documents."""
    B, N, C = q.shape
    Kt, D = k.shape[1], C // H
    if front == "AttnCapture":
        o, p = ops.attn_capture_fwd(q, k, v, H, scale, want)

        def bwd(d_o, d_p):
            dq = ops.attn_capture_bwd(q, k, v, d_o, d_p, H, scale)
            return dq, dq, None
        return o, p, bwd
    if front == "AttnCapturePaintWithWords":
        smax, arg = ops.attn_scores_max(q, k, H, scale)
        coef = smax * float(mult)
        o, p = ops.attn_capture_fwd_biased(q, k, v, H, scale, want, bias, coef)

        def bwd(d_o, d_p):
            dq, gsum = ops.attn_capture_bwd_biased(q, k, v, d_o, d_p, H, scale, bias, coef)
            before = dq.clone()
            # the gradient that reaches the scores through `.max()`: (mult * sum dS * mask) at the maximum's position
            bh, rem = arg // (N * Kt), arg % (N * Kt)
            n, kk = rem // Kt, rem % Kt
            b, h = bh // H, bh % H
            krow = k.view(B * Kt * H, D).index_select(0, (b * Kt + kk) * H + h)
            add = (krow.float() * (gsum * (float(mult) * scale))).to(dq.dtype)
            dq.view(B * N * H, D).index_add_(0, (b * N + n) * H + h, add)
            return dq, before, _max_rows(arg, H, N, Kt)
        return o, p, bwd
    packed = ops.attn_scores_max_grouped(q, k, H, scale, mult.numel())
    o, p = ops.attn_capture_fwd_biased_grouped(q, k, v, H, scale, want, bias, packed, mult)

    def bwd(d_o, d_p):
        dq, gsum = ops.attn_capture_bwd_biased_grouped(q, k, v, d_o, d_p, H, scale, bias, packed, mult)
        before = dq.clone()
        ops.attn_pww_max_grad(dq, k, packed, gsum, mult, H, scale)
        return dq, before, _max_rows(ops.unpack_scores_max(packed)[1], H, N, Kt)
    return o, p, bwd


@pytest.mark.parametrize("shape,dt,front,want,cot", CROSS_CASES, ids=ids)
def test_cross_attention_front(ops, shape, dt, front, want, cot):
    B, H, N, Kt, D = shape
    T, scale, dts = DT[dt], D ** -0.5, str(DT[dt])
    q, k, v = make_qkv(B, H, N, Kt, D, T, 900, 0.6)
    d_o = dev(hashrand.normalish((B, N, H * D), 903), T)
    G = 2
    if front == "AttnCapture":
        extra, bias, mult = (), None, None
    elif front == "AttnCapturePaintWithWords":
        bias, mult = _masks(1, N, Kt, T)[0], MULT
        extra = (bias, mult)
    else:
        bias, mult = _masks(G, N, Kt, T), torch.tensor([MULT, 0.7 * MULT], device="cuda")
        extra = (bias, mult)
    qa = q.clone().requires_grad_(True)
    with ops.census_scope() as fwd:
        o, p = getattr(ops, front).apply(qa, k, v, H, scale, want, *extra)
    ro, rp, rbwd = _by_hand(ops, front, q, k, v, H, scale, want, bias, mult)
    assert torch.equal(o, ro), "o"
    assert (p.numel() == 0 and rp is None) if not want else torch.equal(p, rp), "probs"

    # the cotangent on the probabilities, for the front (`d_p`) and for the wrappers called by hand (`hand_p()`)
    loss_bwd, per_image = {}, None
    if cot == "none":      # autograd materialises the missing cotangent of a wanted `probs` as zeros; the placeholder has none
        d_p, hand_p = None, (lambda: torch.zeros_like(rp)) if want else (lambda: None)
    elif cot == "dense":
        d_p = dev(hashrand.normalish((B * H, N, Kt), 904) * 0.1, T)
        hand_p = lambda: d_p  # noqa: E731
    elif cot == "stride0":
        d_p = dev(hashrand.normalish((N, Kt), 905) * 0.1, T).unsqueeze(0).expand(B * H, N, Kt)
        hand_p = lambda: d_p  # noqa: E731
    else:
        res = int(round(N ** 0.5))
        if res * res == N:     # from the batched loss itself: one image per batch row
            plan = ops.LossPlan(ENTRIES, oloss.DEFAULT_HYPER)
            A, _, loss = ops.AggregateSmoothLossBatched.apply(B, res, 1, Kt - 1, plan, p)
            _, per_image = ops.smooth_loss_bwd_batched(A, res, 1, Kt - 1, plan, torch.ones(B, device="cuda"), T, 1.0 / H)
            loss_bwd = {("smooth_loss_bwd_batched", plan.T, B, N, Kt, 0, True, dts): 1}
        else:
            per_image = dev(hashrand.normalish((B, N, Kt), 906) * 0.1, T)

        def hand_p():
            ops._image_broadcasts[per_image.data_ptr()] = [B, N * Kt, per_image, 1]
            return per_image[0].unsqueeze(0).expand(B * H, N, Kt)
        d_p = hand_p() if res * res != N else None

    with ops.census_scope() as bwd:
        if cot == "per_image" and d_p is None:
            (dq,) = torch.autograd.grad([o, loss.sum()], [qa], [d_o, None])
        elif d_p is None:
            (dq,) = torch.autograd.grad([o], [qa], [d_o])
        else:
            (dq,) = torch.autograd.grad([o, p], [qa], [d_o, d_p])
    ops.end_image_broadcasts()
    rdq, before, rows = rbwd(d_o, hand_p())
    ops.end_image_broadcasts()
    if rows is not None:
        # d loss / d coef is a sum of float atomics and not bit-reproducible from one launch to the next (two runs of the same
        # wrapper differ in its last bits), and the gradient through the maximum is T(k row * that sum * mult * scale) added
        # in T to one row of dq per image.  Those rows — and no others — may therefore differ by the two roundings to T
        # (of the addend, |addend| <= |before| + |after|, and of the sum); everything else is bit-equal.
        got, ref, b4 = (t.view(B * N * H, D).index_select(0, rows).float() for t in (dq, rdq, before))
        assert not torch.equal(ref, b4), "the gradient through the maximum is part of the case"
        bar = 2 * torch.finfo(T).eps * (b4.abs() + ref.abs())
        assert bool(((got - ref).abs() <= bar).all()), f"rows of the maxima: {(got - ref).abs().max().item():.3e}"
        dq, rdq = dq.clone(), rdq.clone()
        for t in (dq, rdq):
            t.view(B * N * H, D).index_fill_(0, rows, 0)
    assert torch.equal(dq, rdq), f"dq: {int((dq != rdq).sum())} elements differ"

    # written from the structure the fronts had before they shared one Function: only the plain forward and backward count
    if front == "AttnCapture":
        flag = want      # a wanted `probs` always has a cotangent by the time the backward runs (zeros when the loss skipped it)
        assert fwd.launches == {("attn_capture_fwd", B, H, N, Kt, D, want, dts): 1}
        assert bwd.launches == {("attn_capture_bwd", B, H, N, Kt, D, flag, dts): 1, **loss_bwd}
    else:
        assert fwd.launches == {}
        assert bwd.launches == loss_bwd


# ===================================================================================== flash self-attention
SELF = [(2, 3, 100, 16), (1, 2, 64, 40)]
SELF_COTS = {"plain": ("o",), "capture": ("o", "probs-dense", "probs-stride0", "o+probs")}
SELF_CASES = [(s, f, c) for s in SELF for f, cots in SELF_COTS.items() for c in cots]


def _self_fronts(ops, capture):
    """(the front that takes q, k, v; the one that takes the fused tensor)"""
    return (ops.SelfAttentionCapture, ops.SelfAttentionCaptureFusedQKV) if capture else (ops.SelfAttention, ops.SelfAttentionFusedQKV)


@pytest.mark.parametrize("shape,family,cot", SELF_CASES, ids=ids)
def test_self_attention_fronts(ops, shape, family, cot):
    B, H, N, D = shape
    T, scale, dts, C = DT["f16"], D ** -0.5, str(DT["f16"]), H * D
    q, k, v = qkv_inputs(shape, "f16")
    d_o = dev(hashrand.normalish((B, N, C), 44 + N), T) if cot in ("o", "o+probs") else None
    d_p = None
    if cot == "probs-dense":
        d_p = dev(hashrand.normalish((B * H, N, N), 45 + N) * 0.1, T)
    elif cot in ("probs-stride0", "o+probs"):
        d_p = dev(hashrand.normalish((N, N), 46 + N) * 0.1, T).unsqueeze(0).expand(B * H, N, N)
    capture = family == "capture"
    sep, fus = _self_fronts(ops, capture)
    key = lambda kind, flag: (kind, B, H, N, N, D, flag, dts)  # noqa: E731
    fwd_key = key("self_attn_capture_fwd", True) if capture else key("self_attn_fwd", True)
    bwd_key = key("self_attn_bwd", True) if d_p is None else key("self_attn_bwd_dp", d_o is not None)

    def run(front, leaves):
        with ops.census_scope() as fwd:
            out = front.apply(*leaves, H, scale)
        o, p = out if capture else (out, None)
        outs, cots = zip(*[(t, g) for t, g in ((o, d_o), (p, d_p)) if g is not None])
        with ops.census_scope() as bwd:
            grads = torch.autograd.grad(outs, leaves, cots)
        assert fwd.launches == {fwd_key: 1} and bwd.launches == {bwd_key: 1}, (front.__name__, fwd.launches, bwd.launches)
        return o, p, grads

    o1, p1, g1 = run(sep, [t.clone().requires_grad_(True) for t in (q, k, v)])
    o2, p2, (g2,) = run(fus, [torch.cat([q, k, v], dim=-1).contiguous().requires_grad_(True)])
    # the wrappers by hand
    if capture:
        ro, lse, rp = ops.self_attn_capture_fwd(q, k, v, H, scale)
        assert torch.equal(p1, rp) and torch.equal(p2, rp), "probs"
    else:
        ro, lse = ops.self_attn_fwd(q, k, v, H, scale)
    assert torch.equal(o1, ro) and torch.equal(o2, ro), "o"
    rg = ops.self_attn_bwd(q, k, v, ro, d_o, lse, H, scale, d_probs=d_p)
    assert g2.shape == (B, N, 3 * C)
    for name, a, b, r in zip(("dq", "dk", "dv"), g1, g2.split(C, dim=-1), rg):
        assert torch.equal(a, r), f"{name}: the separate front and the wrappers differ"
        assert torch.equal(b, r), f"{name}: fused and separate layouts differ"


@pytest.mark.parametrize("capture", [False, True], ids=["plain", "capture"])
def test_self_attention_forward_without_gradients(ops, capture):
    """No input needs a gradient: the plain fronts ask for no lse (census flag False); the capture fronts always compute it."""
    B, H, N, D = shape = SELF[1]
    q, k, v = qkv_inputs(shape, "f16")
    scale, dts = D ** -0.5, str(torch.float16)
    qkv = torch.cat([q, k, v], dim=-1).contiguous()
    sep, fus = _self_fronts(ops, capture)
    expected = {(("self_attn_capture_fwd" if capture else "self_attn_fwd"), B, H, N, N, D, capture, dts): 1}
    for front, args in ((sep, (q, k, v)), (fus, (qkv,))):
        with ops.census_scope() as c:
            out = front.apply(*args, H, scale)
        assert c.launches == expected, (front.__name__, c.launches)
        assert not (out[0] if capture else out).requires_grad
