"""ga_self_attn_bwd_dp — the flash backward with a cotangent on the stored self-attention probabilities — through
ops.self_attn_bwd(d_probs=...), ops.SelfAttentionCapture* and the public route (aggregate_attention(..., is_cross=False)),
against float64 autograd on inputs rounded to the test dtype first.  Needs an MI355X.

Bars: the flash backward's (3 x test_kernels_gpu.TOL of the reference gradient's maximum) for dq, dk, dv; the processor test's
own (4 x 2 x TOL["f16"]) for the gradient that reaches the layer's input.  Everything else is a bit identity."""
import numpy as np
import pytest
import torch

import hashrand
from guarded_alloc import assert_intact, guarded, snapshot
from test_kernels_gpu import DT, TOL, close, dev
from test_self_attn_capture_gpu import _processor_case, _raise, autograd_reference, qkv_inputs

pytestmark = pytest.mark.gpu

ids = lambda v: v if isinstance(v, str) else "x".join(map(str, v))  # noqa: E731


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from guided_attention_amd import ops as _ops
    _ops.load()
    _ops.prepare_device("cuda")
    return _ops


def weights(shape, dt, pattern, cot, mul=1.0):
    """(w_o or None, w_p): the cotangents of o and of P.  cot = "dense": one value per element of P; "broadcast": ONE (N, N)
    map expanded over the B * H head-maps (what a mean over heads sends back)."""
    B, H, N, D = shape
    T = DT[dt]
    w_o = dev(hashrand.normalish((B, N, H * D), 14 + N) * np.float32(mul), T) if pattern == "o+probs" else None
    if cot == "dense":
        w_p = dev(hashrand.normalish((B * H, N, N), 15 + N) * np.float32(mul), T)
    else:
        w_p = dev(hashrand.normalish((N, N), 16 + N) * np.float32(mul), T).unsqueeze(0).expand(B * H, N, N)
    return w_o, w_p


_REF = {}


def reference(shape, dt, pattern, cot, mul=1.0):
    """(q, k, v, w_o, w_p on the device, float64 dq, dk, dv): computed once per case, shared, never modified."""
    key = (shape, dt, pattern, cot, mul)
    if key not in _REF:
        _REF.clear()
        B, H, N, D = shape
        q, k, v = qkv_inputs(shape, dt)
        w_o, w_p = weights(shape, dt, pattern, cot, mul)
        _REF[key] = (q, k, v, w_o, w_p, autograd_reference(q, k, v, H, D ** -0.5, w_o, w_p))
    return _REF[key]


def scalar(o, P, w_o, w_p):
    total = (P.float() * w_p.float()).sum()
    return total if w_o is None else total + (o.float() * w_o.float()).sum()


def both_forms(ops, q, k, v, H, scale, w_o, w_p):
    """dq, dk, dv through SelfAttentionCapture and through SelfAttentionCaptureFusedQKV."""
    C = q.shape[-1]
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    scalar(*ops.SelfAttentionCapture.apply(*leaves, H, scale), w_o, w_p).backward()
    qkv = torch.cat([q, k, v], dim=-1).contiguous().requires_grad_(True)
    scalar(*ops.SelfAttentionCaptureFusedQKV.apply(qkv, H, scale), w_o, w_p).backward()
    return {"SelfAttentionCapture": [t.grad for t in leaves], "SelfAttentionCaptureFusedQKV": list(qkv.grad.split(C, dim=-1))}


def check_against(ops, shape, dt, pattern, cot, mul=1.0):
    B, H, N, D = shape
    q, k, v, w_o, w_p, ref = reference(shape, dt, pattern, cot, mul)
    for form, grads in both_forms(ops, q, k, v, H, D ** -0.5, w_o, w_p).items():
        for name, got, r in zip(("dq", "dk", "dv"), grads, ref):
            assert torch.isfinite(got).all(), f"{form} {name}"
            err = np.abs(got.double().cpu().numpy() - r).max() / max(np.abs(r).max(), 1e-30)
            print(f"{form} {name} [{pattern}, {cot}] err {err:.3e} (bar {3 * TOL[dt]:.1e})")
            close(got, r, 3 * TOL[dt], f"{form} {name}")


# B, H, N, D: one tile, odd k-chunk; partial query and key tiles, dP rows not 16-byte aligned in the 16-bit types; smaller than
# any tile; several tiles, partial last; the widest head (16 bit only); the 32^2 layer (f16 only, once)
SHAPES = [(1, 2, 64, 40), (2, 3, 100, 16), (1, 1, 25, 8), (1, 1, 200, 64), (1, 2, 256, 160)]
CASES = [(s, dt, p, c) for s in SHAPES for dt in ("f32", "f16", "bf16") if not (dt == "f32" and s[3] > 80)
         for p in ("o+probs", "probs") for c in ("dense", "broadcast")] + [((1, 2, 1024, 80), "f16", "o+probs", "broadcast")]


@pytest.mark.parametrize("shape,dt,pattern,cot", CASES, ids=ids)
def test_against_float64_autograd(ops, shape, dt, pattern, cot):
    """Measured on an MI355X, worst case over the shapes, forms and patterns (fraction of the reference gradient's maximum):
    f32 4.6e-6 (bar 6e-5), f16 2.0e-3 (bar 6e-3), bf16 1.3e-2 (bar 4.8e-2)."""
    check_against(ops, shape, dt, pattern, cot)


@pytest.mark.parametrize("cot", ["dense", "broadcast"])
@pytest.mark.parametrize("pattern", ["o+probs", "probs"])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_small_cotangents(ops, dt, pattern, cot):
    """Both cotangents scaled by 2^-8 (exact in f16 and bf16; the size of a guidance gradient in test_blocks_gpu): the same
    relative bar — the power-of-two scale of dS for the 16-bit MFMA is taken after dP - r has entered."""
    check_against(ops, (1, 2, 256, 40), dt, pattern, cot, mul=2.0 ** -8)


@pytest.mark.parametrize("shape,dt", [(s, dt) for s in [(2, 3, 100, 16), (1, 2, 64, 40), (1, 2, 256, 160)]
                                      for dt in ("f16", "f32") if not (dt == "f32" and s[3] > 80)], ids=ids)
def test_bit_identities(ops, shape, dt):
    B, H, N, D = shape
    T, scale = DT[dt], D ** -0.5
    q, k, v = qkv_inputs(shape, dt)
    o, lse, P = ops.self_attn_capture_fwd(q, k, v, H, scale)
    d_o = dev(hashrand.normalish((B, N, H * D), 24 + N), T)
    one = dev(hashrand.normalish((N, N), 25 + N), T)
    shared = one.unsqueeze(0).expand(B * H, N, N)
    assert shared.stride() == (0, N, 1)
    # a zero cotangent on the probabilities: the plain flash backward
    plain = ops.self_attn_bwd(q, k, v, o, d_o, lse, H, scale)
    zero = ops.self_attn_bwd(q, k, v, o, d_o, lse, H, scale, d_probs=torch.zeros_like(P))
    for name, a, b in zip(("dq", "dk", "dv"), zero, plain):
        assert torch.equal(a, b), f"{name}: a zero cotangent changes the flash backward"
    # one map shared through a zero stride = its dense copy; two runs of the same call agree
    first = ops.self_attn_bwd(q, k, v, o, d_o, lse, H, scale, d_probs=shared)
    again = ops.self_attn_bwd(q, k, v, o, d_o, lse, H, scale, d_probs=shared)
    dense = ops.self_attn_bwd(q, k, v, o, d_o, lse, H, scale, d_probs=shared.contiguous())
    for name, a, b, c in zip(("dq", "dk", "dv"), first, again, dense):
        assert torch.equal(a, b), f"{name}: two runs differ"
        assert torch.equal(a, c), f"{name}: the stride-0 map and its dense copy differ"
    assert not torch.equal(first[0], plain[0])
    # the loss read the probabilities only: dO = None is dO = 0, and dv is zero
    none = ops.self_attn_bwd(q, k, v, o, None, lse, H, scale, d_probs=shared)
    zeros = ops.self_attn_bwd(q, k, v, o, torch.zeros_like(d_o), lse, H, scale, d_probs=shared)
    assert torch.equal(none[0], zeros[0]) and torch.equal(none[1], zeros[1])
    assert torch.equal(none[2], torch.zeros_like(v))
    # the fused form on the same data: the same three launches on column slices
    qkv = torch.cat([q, k, v], dim=-1).contiguous()
    fused = ops.self_attn_bwd(*qkv.split(H * D, dim=-1), o, d_o, lse, H, scale, d_probs=shared)
    assert fused[0].stride() == qkv.split(H * D, dim=-1)[0].stride()
    for name, a, b in zip(("dq", "dk", "dv"), fused, first):
        assert torch.equal(a, b), f"{name}: fused and separate layouts differ"


def _boom(*a, **kw):
    raise AssertionError("the backward of a captured self-attention layer left the kernels for the framework")


def test_backward_stays_off_the_framework(ops, monkeypatch):
    """The backward of SelfAttentionCaptureFusedQKV with a cotangent on the probabilities: no framework product, no f32 copies,
    one ga_self_attn_bwd_dp call in the census, and no N x N tensor kept by the forward for it."""
    shape = B, H, N, D = (1, 2, 256, 40)
    T, scale = DT["f16"], D ** -0.5
    q, k, v = qkv_inputs(shape, "f16")
    w_o, w_p = weights(shape, "f16", "o+probs", "broadcast")
    qkv = torch.cat([q, k, v], dim=-1).contiguous().requires_grad_(True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(tuple(t.shape)), t)[1], lambda t: t):
        o, P = ops.SelfAttentionCaptureFusedQKV.apply(qkv, H, scale)
        leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
        o2, P2 = ops.SelfAttentionCapture.apply(*leaves, H, scale)
    assert saved and all(int(np.prod(s)) != N * N * B * H for s in saved), saved
    d_o, d_P = torch.autograd.grad(scalar(o, P, w_o, w_p), (o, P), retain_graph=True)
    ops.start_census()
    with monkeypatch.context() as m:
        for mod, name in ((torch, "mm"), (torch, "bmm"), (torch, "matmul"), (torch.Tensor, "float")):
            m.setattr(mod, name, _boom)
        torch.autograd.backward([o, P], [d_o, d_P])
        torch.cuda.synchronize()
    kinds = {}
    for key, n in ops.stop_census().items():
        kinds[key[0]] = kinds.get(key[0], 0) + n
    assert kinds.get("self_attn_bwd_dp") == 1 and "self_attn_bwd" not in kinds, kinds
    ref = autograd_reference(q, k, v, H, scale, w_o, w_p)
    for name, got, r in zip(("dq", "dk", "dv"), qkv.grad.split(H * D, dim=-1), ref):
        close(got, r, 3 * TOL["f16"], name)


@pytest.mark.parametrize("with_do", [True, False], ids=["dO", "no-dO"])
@pytest.mark.parametrize("shape,dt", [(s, dt) for s in [(2, 3, 100, 16), (1, 2, 64, 40)] for dt in ("f16", "f32")], ids=ids)
def test_output_bounds(ops, shape, dt, with_do):
    """dq, dk, dv, delta and rowdot written in full (dv too when there is no dO), no red-zone byte touched, every input
    bit-identical afterwards."""
    B, H, N, D = shape
    T, scale = DT[dt], D ** -0.5
    q, k, v = qkv_inputs(shape, dt)
    o, lse, P = ops.self_attn_capture_fwd(q, k, v, H, scale)
    d_o = dev(hashrand.normalish((B, N, H * D), 34 + N), T) if with_do else None
    d_p = dev(hashrand.normalish((B * H, N, N), 35 + N), T)
    snap = snapshot(q, k, v, o, d_o, lse, d_p)
    with guarded(ops) as g:
        dq, dk, dv = ops.self_attn_bwd(q, k, v, o, d_o, lse, H, scale, d_probs=d_p)
        for t, what in ((dq, "dq"), (dk, "dk"), (dv, "dv")):
            g.assert_written(t, what)
        g.assert_all_written()                      # delta and rowdot are among the arenas
        assert len(g.arenas) == 5 and g.large_passthroughs == 0
    assert_intact(snap)
    ref = autograd_reference(q, k, v, H, scale, d_o, d_p)
    for name, got, r in zip(("dq", "dk", "dv"), (dq, dk, dv), ref):
        close(got, r, 3 * TOL[dt], name)


def _processor_reference_with_maps(attn, norm, x, folded, w, w_a):
    """test_self_attn_capture_gpu._processor_reference's float64 arithmetic with the aggregate term: the scalar is
    sum(out * w) + sum(mean over heads of P * w_a)."""
    d = lambda t: t.detach().double().cpu()  # noqa: E731
    x64 = d(x).requires_grad_(True)
    h = torch.nn.functional.layer_norm(x64, (x64.shape[-1],), d(norm.weight), d(norm.bias), norm.eps) if folded else x64
    H, (B, N, C) = attn.heads, x64.shape
    split = lambda t: t.view(B, N, H, C // H).transpose(1, 2).reshape(B * H, N, C // H)  # noqa: E731
    P = torch.softmax(torch.bmm(split(h @ d(attn.to_q.weight).T), split(h @ d(attn.to_k.weight).T).transpose(1, 2)) * attn.scale, -1)
    o = torch.bmm(P, split(h @ d(attn.to_v.weight).T)).view(B, H, N, C // H).transpose(1, 2).reshape(B, N, C)
    out = o @ d(attn.to_out[0].weight).T + d(attn.to_out[0].bias)
    if folded:
        out = out + x64
    ((out * d(w)).sum() + (P.mean(0) * d(w_a).view(N, N)).sum()).backward()
    return x64.grad.numpy()


@pytest.mark.parametrize("folded", [False, True], ids=["plain", "folded"])
@pytest.mark.parametrize("N", [64, 256])
def test_through_the_public_route(ops, monkeypatch, N, folded):
    """A loss on aggregate_attention(store, res, ("up",), False, 0) of a stored self-attention layer: the gradient reaches the
    layer's input through ga_self_attn_bwd_dp, which receives AggregateMaps.backward's zero-stride view as it is."""
    from guided_attention_amd.utils import ptp_utils
    monkeypatch.setattr(ptp_utils, "_materialised_attention", _raise)
    T, res = torch.float16, int(round(N ** 0.5))
    attn, norm, x, kw = _processor_case(N, folded, 900 + N)
    store = ptp_utils.AttentionStore(capture="reference")
    store.num_att_layers = 1
    proc = ptp_utils.AttendExciteCrossAttnProcessor(attnstore=store, place_in_unet="up")
    seen = []
    real = ops.self_attn_bwd

    def spy(*a, **kwargs):
        seen.append(kwargs.get("d_probs", a[8] if len(a) > 8 else None))
        return real(*a, **kwargs)
    monkeypatch.setattr(ops, "self_attn_bwd", spy)
    ops.start_census()
    with torch.enable_grad():
        out = proc(attn, x, **kw)
        out = out[0] if folded else out
        A = ptp_utils.aggregate_attention(store, res, ("up",), False, 0)
        assert A.shape == (res, res, N) and A.dtype == torch.float32
        w = dev(hashrand.normalish(tuple(out.shape), 1000 + N), T)
        w_a = dev(hashrand.normalish((res, res, N), 1100 + N), torch.float32)
        ((out.float() * w.float()).sum() + (A * w_a).sum()).backward()
    kinds = {}
    for key, n in ops.stop_census().items():
        kinds[key[0]] = kinds.get(key[0], 0) + n
    assert kinds.get("self_attn_capture_fwd") == 1 and kinds.get("self_attn_bwd_dp") == 1 and "self_attn_bwd" not in kinds, kinds
    assert len(seen) == 1 and seen[0] is not None and seen[0].shape == (attn.heads, N, N)
    assert seen[0].stride(0) == 0 and seen[0].dtype == T          # the zero-stride view itself, no copy
    dx_ref = _processor_reference_with_maps(attn, norm, x, folded, w, w_a)
    err = np.abs(x.grad.double().cpu().numpy() - dx_ref).max() / np.abs(dx_ref).max()
    print(f"dx err {err:.3e} (bar {4 * 2 * TOL['f16']:.1e})")
    close(x.grad, dx_ref, 4 * 2 * TOL["f16"], "dx")


def test_forward_and_backward_can_be_captured(ops):
    """Forward + backward with cotangents on o and on the probabilities inside one hipGraph: two replays give the eager bits."""
    shape = B, H, N, D = (1, 2, 256, 40)
    scale = D ** -0.5
    q, k, v = qkv_inputs(shape, "f16")
    w_o, w_p = weights(shape, "f16", "o+probs", "dense")
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]

    def step():
        return torch.autograd.grad(scalar(*ops.SelfAttentionCapture.apply(*leaves, H, scale), w_o, w_p), leaves)

    eager = [g.clone() for g in step()]
    side = ops.side_stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                     # warm-up on the capture stream
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with ops.no_gc(), torch.cuda.graph(graph, stream=side):
            captured = step()
        for _ in range(2):
            for g in captured:
                g.zero_()
            graph.replay()
            side.synchronize()
            for name, a, b in zip(("dq", "dk", "dv"), captured, eager):
                assert torch.equal(a, b), f"{name}: a replay differs from the eager run"
    torch.cuda.current_stream().wait_stream(side)
