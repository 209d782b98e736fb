"""Self-attention maps from the flash kernels (ga_self_attn_probs / ga_self_attn_capture_fwd, ops.SelfAttentionCapture*, the
processor's reference-capture branch) against float64 on inputs rounded to the test dtype first.  Needs an MI355X.

Bars are the project's per-kernel ones (test_kernels_gpu.TOL: f32 2e-5, f16 2e-3, bf16 1.6e-2 of the tensor's maximum; a
probability is <= 1, so for P they are absolute), the flash backward's (3 x TOL) for gradients, and the g6 processor test's
for the processor (out 2 x tol, dx 4 x tol with tol = TOL, doubled for the 16-bit types)."""
import math

import numpy as np
import pytest
import torch

import hashrand
from conftest import load_json, load_npz
from guarded_alloc import assert_intact, guarded, snapshot
from test_kernels_gpu import DT, TOL, _g6_attention, close, dev, from_bh, to_bh

pytestmark = pytest.mark.gpu

ALL = ["f32", "f16", "bf16"]
ids = lambda v: v if isinstance(v, str) else "x".join(map(str, v))  # noqa: E731
UNIT = {"f32": 2.0 ** -24, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}     # one rounding to T of a value <= 1


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from guided_attention_amd import ops as _ops
    _ops.load()
    _ops.prepare_device("cuda")
    return _ops


def softmax64(Q, K, scale):
    S = scale * np.einsum("bnd,bmd->bnm", Q, K)
    E = np.exp(S - S.max(-1, keepdims=True))
    return E / E.sum(-1, keepdims=True)


def qkv_inputs(shape, dt, spread=1.5):
    B, H, N, D = shape
    return tuple(dev(hashrand.normalish((B, N, H * D), s + N) * sp, DT[dt])
                 for s, sp in ((11, spread), (12, spread), (13, 1.0)))


_REF = {}


def reference(shape, dt):
    """(q, k, v on the device, P and O in float64) for a case: computed once, shared by the layouts, never modified."""
    key = (shape, dt)
    if key not in _REF:
        _REF.clear()                      # one case's reference at a time (the 32^2 layer's is 2 x 8 MB)
        B, H, N, D = shape
        q, k, v = qkv_inputs(shape, dt)
        P = softmax64(to_bh(q, H), to_bh(k, H), D ** -0.5)
        _REF[key] = (q, k, v, P, P @ to_bh(v, H))
    return _REF[key]


# B, H, N, D: one key tile; partial query and key tiles with element-by-element stores (N * 2 is no multiple of 16); several
# tiles, partial last, 16-byte stores; the 32^2 layer; the 16^2 layer (16 bit only); a map smaller than any tile
P_SHAPES = [(1, 2, 64, 40), (2, 3, 100, 16), (1, 1, 200, 64), (1, 2, 1024, 80), (1, 2, 256, 160), (1, 1, 25, 8)]
P_CASES = [(s, lay, dt) for s in P_SHAPES for lay in ("separate", "fused") for dt in ALL if not (dt == "f32" and s[3] > 80)]


@pytest.mark.parametrize("shape,layout,dt", P_CASES, ids=ids)
def test_probabilities_against_float64_softmax(ops, shape, layout, dt):
    B, H, N, D = shape
    T, scale = DT[dt], D ** -0.5
    q, k, v, Pref, Oref = reference(shape, dt)
    if layout == "fused":
        qkv = torch.cat([q, k, v], dim=-1).contiguous()
        o, P = ops.SelfAttentionCaptureFusedQKV.apply(qkv, H, scale)
        o_flash = ops.SelfAttentionFusedQKV.apply(qkv.clone().requires_grad_(True), H, scale).detach()
    else:
        o, lse, P = ops.self_attn_capture_fwd(q, k, v, H, scale)
        o_flash, lse_flash = ops.self_attn_fwd(q, k, v, H, scale)
        # the capture entry's O and LSE are the flash forward's; the probabilities entry alone, on that LSE, gives the same P
        assert torch.equal(lse, lse_flash)
        assert torch.equal(ops.self_attn_probs(q, k, lse_flash, H, scale), P)
    assert torch.equal(o, o_flash)
    assert P.shape == (B * H, N, N) and P.dtype == T and o.shape == (B, N, H * D)
    P64 = P.double().cpu().numpy()
    assert np.isfinite(P64).all()
    err = np.abs(P64 - Pref).max()
    print(f"P err {err:.3e} (bar {TOL[dt]:.1e}), row sums off by {np.abs(P64.sum(-1) - 1).max():.3e} (bar {N * UNIT[dt]:.1e})")
    assert err <= TOL[dt], f"P: max err {err:.3e}"
    close(o, from_bh(Oref, B, H), TOL[dt], "O")
    # the stored map is the one the output was made from: rows sum to 1 within N roundings of T, and P.V from it is O
    assert np.abs(P64.sum(-1) - 1).max() <= N * UNIT[dt]
    close(o, from_bh(P64 @ to_bh(v, H), B, H), TOL[dt], "O against the stored P times V")


@pytest.mark.parametrize("dt", ALL)
def test_peaked_and_flat_rows(ops, dt):
    """Rows whose one score lies 30 above the rest in the exponent's (base 2) units, and rows whose scores are all equal."""
    B, H, N, D = 1, 1, 100, 16
    scale = D ** -0.5
    q, k = np.zeros((B, N, D), np.float32), np.zeros((B, N, D), np.float32)
    # keys 0..15 are one-hot (coordinate j of key j), the rest zero; query n < N/2 reads coordinate n % 16 only: its one non-zero
    # score is key n % 16's; queries N/2.. are zero: every score equal
    for n in range(N // 2):
        q[0, n, n % D] = 8.0
    peak = 30.0 / (scale * math.log2(math.e) * 8.0)
    for j in range(N):
        k[0, j, j % D] = peak if j < D else 0.0
    qt, kt = dev(q, DT[dt]), dev(k, DT[dt])
    vt = dev(hashrand.normalish((B, N, D), 6), DT[dt])
    o, lse, P = ops.self_attn_capture_fwd(qt, kt, vt, H, scale)
    Pref = softmax64(to_bh(qt, H), to_bh(kt, H), scale)
    gap = (scale * math.log2(math.e) * to_bh(qt, H)[0, 0] @ to_bh(kt, H)[0, 0])
    assert abs(gap - 30.0) < 0.2                               # the construction: 30 in the exponent's units, as rounded to T
    P64 = P.double().cpu().numpy()
    assert np.isfinite(P64).all() and torch.isfinite(o).all() and torch.isfinite(lse).all()
    assert Pref[0, 0].max() > 0.999 and abs(Pref[0, N - 1].max() - 1.0 / N) < 1e-12
    assert np.abs(P64 - Pref).max() <= TOL[dt]
    close(o, from_bh(Pref @ to_bh(vt, H), B, H), TOL[dt], "O")


@pytest.mark.parametrize("shape,dt", [(s, dt) for s in [(2, 3, 100, 16), (1, 2, 64, 40)] for dt in ("f16", "f32")], ids=ids)
def test_output_bounds(ops, shape, dt):
    """Every element of O, LSE and P written, no red-zone byte touched, inputs bit-identical afterwards; a P that starts off
    a 16-byte boundary gets the same values through the element-by-element stores."""
    B, H, N, D = shape
    T, scale = DT[dt], D ** -0.5
    q, k, v = qkv_inputs(shape, dt)
    snap = snapshot(q, k, v)
    with guarded(ops) as g:
        o, lse, P = ops.self_attn_capture_fwd(q, k, v, H, scale)
        for t, what in ((o, "O"), (lse, "lse"), (P, "P")):
            g.assert_written(t, what)
        n_own = len(g.arenas)
        flat = g.carve((B * H * N * N + 1,), T, q.device)
        odd = flat[1:].view(B * H, N, N)
        assert odd.data_ptr() % 16 != 0
        o2, lse2, P2 = ops.self_attn_capture_fwd(q, k, v, H, scale, out=odd)
        assert P2.data_ptr() == odd.data_ptr()
        g.assert_all_written(lambda a: (torch.arange(a.shape[0]) == 0) if a.index == n_own else None)
        P3 = ops.self_attn_probs(q, k, lse, H, scale)
        g.assert_written(P3, "P of ga_self_attn_probs")
    assert n_own == 3 and g.large_passthroughs == 0
    assert_intact(snap)
    assert torch.equal(P2, P) and torch.equal(P3, P) and torch.equal(o2, o) and torch.equal(lse2, lse)
    assert np.abs(P.double().cpu().numpy() - softmax64(to_bh(q, H), to_bh(k, H), scale)).max() <= TOL[dt]


def test_probabilities_past_two_to_the_31_elements(ops):
    """B * H * N * N = 30 * 9216^2 > 2^31 elements (5.1 GB of fp16 P): 64 sampled rows, the first, the last and the rows on
    either side of element 2^31 among them, against float64.  Not guarded (>= 32 MiB)."""
    B, H, N, D = 3, 10, 9216, 64
    scale = D ** -0.5
    base = hashrand.normalish((2, N, H * D), 41)              # one image's worth; the batch entries are row rotations of it
    q = dev(np.stack([np.roll(base[0], 37 * b, axis=0) for b in range(B)]), torch.float16)
    k = dev(np.stack([np.roll(base[1], 11 * b, axis=0) for b in range(B)]), torch.float16)
    assert B * H * N * N > 2 ** 31
    o, lse, P = ops.self_attn_capture_fwd(q, k, k, H, scale)
    edge = 2 ** 31 // N                                        # the row that holds element 2^31
    rows = sorted({0, B * H * N - 1, edge - 1, edge, edge + 1} |
                  {int(r) for r in hashrand.hash_u32(59, 43).astype(np.int64) % (B * H * N)})
    got = P.view(B * H * N, N)[torch.tensor(rows, device=P.device)].double().cpu().numpy()
    del P, o
    torch.cuda.empty_cache()
    Q, K = to_bh(q, H), to_bh(k, H)
    worst = 0.0
    for i, r in enumerate(rows):
        bh, n = divmod(r, N)
        ref = softmax64(Q[bh:bh + 1, n:n + 1], K[bh:bh + 1], scale)[0, 0]
        worst = max(worst, np.abs(got[i] - ref).max() / ref.max())
    print(f"64-bit addressing: worst row error {worst:.3e} of the row's maximum (bar {TOL['f16']:.1e})")
    assert len(rows) == 64 and worst <= TOL["f16"]


# ------------------------------------------------------------------------------------------------ autograd
def autograd_reference(q, k, v, H, scale, w_o, w_p):
    """float64 autograd of sum(o * w_o) + sum(P * w_p) on the CPU; a None weight drops its term."""
    B, N, C = q.shape
    leaves = [t.detach().double().cpu().requires_grad_(True) for t in (q, k, v)]
    qh, kh, vh = (t.view(B, N, H, C // H).transpose(1, 2).reshape(B * H, N, C // H) for t in leaves)
    P = torch.softmax(torch.bmm(qh, kh.transpose(1, 2)) * scale, -1)
    o = torch.bmm(P, vh).view(B, H, N, C // H).transpose(1, 2).reshape(B, N, C)
    total = 0.0
    if w_o is not None:
        total = total + (o * w_o.double().cpu()).sum()
    if w_p is not None:
        total = total + (P * w_p.double().cpu()).sum()
    total.backward()
    return [t.grad.numpy() if t.grad is not None else np.zeros(tuple(t.shape)) for t in leaves]


@pytest.mark.parametrize("pattern", ["o", "o+probs", "probs"])
@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("shape", [(2, 3, 100, 16), (1, 2, 256, 40)], ids=ids)
def test_autograd_against_float64_autograd(ops, shape, dt, pattern):
    B, H, N, D = shape
    T, scale, C = DT[dt], D ** -0.5, H * D
    q, k, v = qkv_inputs(shape, dt)
    w_o = dev(hashrand.normalish((B, N, C), 14 + N), T) if "o" in pattern.split("+") else None
    w_p = dev(hashrand.normalish((B * H, N, N), 15 + N), T) if "probs" in pattern else None
    ref = autograd_reference(q, k, v, H, scale, w_o, w_p)

    def scalar(o, P):
        total = 0.0
        if w_o is not None:
            total = total + (o.float() * w_o.float()).sum()
        if w_p is not None:
            total = total + (P.float() * w_p.float()).sum()
        return total

    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    scalar(*ops.SelfAttentionCapture.apply(*leaves, H, scale)).backward()
    qkv = torch.cat([q, k, v], dim=-1).contiguous().requires_grad_(True)
    scalar(*ops.SelfAttentionCaptureFusedQKV.apply(qkv, H, scale)).backward()
    separate = [t.grad for t in leaves]
    fused = list(qkv.grad.split(C, dim=-1))
    for name, a, b, r in zip(("dq", "dk", "dv"), separate, fused, ref):
        for form, got in (("SelfAttentionCapture", a), ("SelfAttentionCaptureFusedQKV", b)):
            err = np.abs(got.double().cpu().numpy() - r).max() / max(np.abs(r).max(), 1e-30)
            print(f"{form} {name} [{pattern}] err {err:.3e} (bar {3 * TOL[dt]:.1e})")
            close(got, r, 3 * TOL[dt], f"{form} {name}")
    if pattern == "o":     # no cotangent on the probabilities: exactly the flash backward
        plain = qkv.detach().clone().requires_grad_(True)
        (ops.SelfAttentionFusedQKV.apply(plain, H, scale).float() * w_o.float()).sum().backward()
        assert torch.equal(qkv.grad, plain.grad)
        assert torch.equal(torch.cat(separate, dim=-1), plain.grad)


# ------------------------------------------------------------------------------------------------ the processor
def _raise(*a, **kw):
    raise AssertionError("_materialised_attention was called: a self-attention layer inside the envelope left the kernels")


def _processor_case(N, folded, seed, C=64, H=4, T=torch.float16):
    from guided_attention_amd import fused_linear as fl
    from guided_attention_amd.unet import Attention
    attn = Attention(C, None, H, C // H)
    shapes = {"to_q.weight": (C, C), "to_k.weight": (C, C), "to_v.weight": (C, C), "to_out.0.weight": (C, C), "to_out.0.bias": (C,)}
    attn.load_state_dict({n: torch.from_numpy(hashrand.normalish(s, seed + i) * np.float32(1.0 / math.sqrt(s[-1])))
                          for i, (n, s) in enumerate(shapes.items())})
    attn = attn.to("cuda", T)
    norm = torch.nn.LayerNorm(C)
    with torch.no_grad():
        norm.weight.copy_(torch.from_numpy(1.0 + 0.2 * hashrand.normalish((C,), seed + 7)))
        norm.bias.copy_(torch.from_numpy(0.2 * hashrand.normalish((C,), seed + 8)))
    norm = norm.to("cuda", T)
    for prm in list(attn.parameters()) + list(norm.parameters()):
        prm.requires_grad_(False)
    x = dev(hashrand.normalish((1, N, C), seed + 9), T)
    kw = {}
    if folded:   # the residual stream with its row partial sums, as the projection in front of the block leaves them
        eye = torch.eye(C, device="cuda", dtype=T)
        with torch.no_grad():
            x, partials = fl.linear(x, eye, None, want_partials=True)
        x = x.detach().requires_grad_(True)
        kw["folded"] = {"partials": partials, "norm": norm, "residual": x, "want_partials": False}
    else:
        x = x.requires_grad_(True)
    return attn, norm, x, kw


def _processor_reference(attn, norm, x, folded, w):
    """float64 restatement of the layer: [LayerNorm ->] q, k, v -> softmax -> out projection [+ residual]."""
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
    (out * d(w)).sum().backward()
    return out.detach().numpy(), x64.grad.numpy(), P.detach().numpy()


# a user-written controller (the base class's wants_probs: True for every map) takes the same branch: one size is enough
# and so does an AttentionStore whose global store is on (save_global_store=True under the default capture policy)
PROC_CASES = [(N, f, "AttentionStore") for N in (64, 256, 1024) for f in (False, True)] + \
    [(256, False, "custom"), (256, True, "custom"), (256, False, "global-store")]


@pytest.mark.parametrize("N,folded,controller", PROC_CASES, ids=lambda v: {True: "folded", False: "plain"}.get(v, str(v)))
def test_processor_captures_self_attention_on_the_kernels(ops, monkeypatch, N, folded, controller):
    from guided_attention_amd.utils import ptp_utils
    monkeypatch.setattr(ptp_utils, "_materialised_attention", _raise)
    T, H = torch.float16, 4
    attn, norm, x, kw = _processor_case(N, folded, 700 + N)
    if controller == "custom":
        class Keeper(ptp_utils.AttentionControl):
            def __init__(self):
                super().__init__()
                self.maps = []

            def forward(self, a, is_cross, place):
                self.maps.append((a, is_cross, place))
                return a
        store = Keeper()
        assert store.wants_probs(False, N)
    elif controller == "global-store":
        store = ptp_utils.AttentionStore(save_global_store=True)
    else:
        store = ptp_utils.AttentionStore(capture="reference")
    store.num_att_layers = 1
    proc = ptp_utils.AttendExciteCrossAttnProcessor(attnstore=store, place_in_unet="up")
    ops.start_census()
    with torch.enable_grad():
        out = proc(attn, x, **kw)
        out = out[0] if folded else out
        w = dev(hashrand.normalish(tuple(out.shape), 800 + N), T)
        (out.float() * w.float()).sum().backward()
    kinds = {}
    for key, n in ops.stop_census().items():
        kinds[key[0]] = kinds.get(key[0], 0) + n
    assert kinds.get("self_attn_capture_fwd") == 1 and kinds.get("self_attn_bwd") == 1, kinds
    assert "add_layer_norm_fwd" not in kinds and "self_attn_fwd" not in kinds, kinds     # no LayerNorm launch, no plain flash forward
    P = store.maps[0][0] if controller == "custom" else store.attention_store["up_self"][0]
    assert P.shape == (1 * H, N, N) and P.dtype == T                 # the reference's layout and dtype
    out_ref, dx_ref, P_ref = _processor_reference(attn, norm, x, folded, w)
    tol = 2 * TOL["f16"]
    close(P, P_ref, tol, "P")
    close(out, out_ref, 2 * tol, "out")
    close(x.grad, dx_ref, 4 * tol, "dx")
    if controller == "global-store":      # a second forward of the same batch accumulates into the first one's maps
        proc(attn, x.detach())
        assert store.cur_step == 2
        close(store.get_average_global_attention()["up_self"][0], P_ref, tol, "global store average")


@pytest.mark.parametrize("dt", ["f32", "f16"])
@pytest.mark.parametrize("meta", [m for m in load_json("g6_processor.json") if m["ctx_len"] is None], ids=lambda m: m["name"])
def test_capture_function_against_reference_self_fixture(ops, meta, dt):
    """P, out and dx of the reference's own processor on its self-attention cases (scalar = sum(out * R1) + sum(P * R2)), through
    ops.SelfAttentionCapture; tolerances of test_product_processor_against_reference_fixture."""
    g = load_npz("g6_processor.npz")
    n, H, seed = meta["name"], meta["heads"], meta["seed"]
    B, N, C = meta["batch"], meta["N"], meta["C"]
    attn = _g6_attention(meta, DT[dt])
    x = dev(hashrand.normalish((B, N, C), seed), DT[dt]).requires_grad_(True)
    o, P = ops.SelfAttentionCapture.apply(attn.to_q(x), attn.to_k(x), attn.to_v(x), H, meta["scale"])
    out = attn.to_out[1](attn.to_out[0](o))
    tol = TOL[dt] * (1 if dt == "f32" else 2)
    close(out, g[f"{n}.out"], tol * 2, "out vs reference")
    close(P, g[f"{n}.P"], tol, "P vs reference")
    R1 = dev(hashrand.normalish((B, N, C), seed + 8), DT[dt])
    R2 = dev(hashrand.normalish(tuple(P.shape), seed + 9), DT[dt])
    ((out.float() * R1.float()).sum() + (P.float() * R2.float()).sum()).backward()
    close(x.grad, g[f"{n}.dx"], tol * 4, "dx vs reference")


def test_pipeline_with_reference_capture_stays_on_the_kernels(ops, monkeypatch):
    """The tiny fp32 UNet, 2 guided steps under capture='reference', no materialising self-attention allowed, against the
    loss-only run (5e-3, the bar test_pipeline_gpu uses for that comparison); the stored self maps aggregate.

    Without save_global_store: a guided call alternates batch-1 guidance passes with batch-2 classifier-free-guidance passes,
    and the global store adds each pass's maps onto the first pass's (`global_store[key][i] += ...`, the reference's code,
    utils/ptp_utils.py:232-241), so it raises on the first batch-2 pass in the reference and here alike, on any attention path.
    What save_global_store=True changes for the processor is wants_probs only, the same answer capture='reference' gives; the
    global store itself is exercised on the processor (test_processor_captures_self_attention_on_the_kernels, global-store)."""
    from guided_attention_amd.utils import ptp_utils
    from test_oracle_loop import G9, g9_setup
    from test_pipeline_gpu import build_product, run_product
    meta = dict(G9[1], steps=2)
    unet, embeds, lat0, noise, thr = g9_setup(meta)
    pipe = build_product(unet, torch.float32)
    base, _ = run_product(pipe, meta, embeds, lat0, noise, thr)
    assert base.census.get("self_attn_capture_fwd", 0) == 0
    monkeypatch.setattr(ptp_utils, "_materialised_attention", _raise)
    out, ctrl = run_product(pipe, meta, embeds, lat0, noise, thr, capture="reference")
    assert out.census.get("self_attn_capture_fwd", 0) > 0 and out.census.get("self_attn_fwd", 0) == 0, out.census
    assert out.unet_calls["bwd"] > 0
    err = (out.latents - base.latents).abs().max().item() / base.latents.abs().max().item()
    print(f"latents: reference capture against loss-only {err:.3e} (bar 5e-3)")
    assert err < 5e-3, err
    A = ptp_utils.aggregate_attention(ctrl, 16, ("up", "down", "mid"), False, 0)
    assert A.shape == (16, 16, 256)
    # every stored row sums to 1 within N roundings (test_probabilities_against_float64_softmax); their f32 mean adds one more
    assert (A.double().sum(-1) - 1).abs().max().item() <= 2 * 256 * UNIT["f32"]
