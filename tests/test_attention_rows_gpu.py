"""The attention kernels (attn_capture.hip and the flash family in self_attn.hip: forward, backward, the stored-P capture and the
dP-cotangent backward) on the score rows a trained checkpoint produces — peaked rows, rows with a large common offset, a
BOS / sink column, a row maximum that moves in every key tile — against float64 on inputs rounded to the test dtype first.
Needs an MI355X.  The rows, the float64 restatements and the bars are attention_rows.py's; test_attention_rows.py shows on the
CPU that the kernels' documented arithmetic meets every bar used here with 1.25 x headroom.

Per tensor (test_kernels_gpu.close): the larger of the existing parity test's bar (TOL for O, 3 x TOL for the flash gradients,
2 x TOL for the capture dQ) and the error, against the same float64 result, of the reference's own arithmetic in that dtype on
the CPU (f32: 4 e_s, the f32 dot-product bound).  Element by element: the stored probabilities and the LSE.  Every case prints
`[measured]` lines; profiles/attention_rows.json holds those of one run."""
import numpy as np
import pytest
import torch

import attention_rows as ar
from test_kernels_gpu import DT, TOL, close, dev, from_bh, to_bh  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from guided_attention_amd import ops as _ops
    _ops.load()
    _ops.prepare_device("cuda")
    return _ops


def note(key, name, got, ref, ref_err, bar):
    err = ar.rel_err(got.detach().double().cpu().numpy() if torch.is_tensor(got) else got, ref)
    print(f"[measured] {key[0]} {key[1]} {key[2]} {ar.ids(key[3])} {name}: kernel {err:.3e}  reference arithmetic {ref_err:.3e}  "
          f"bar {bar:.3e}")
    return err


def flash_case(kind, dt, shape, with_dp=False):
    """Inputs on the CPU, float64 result, bars and the model's LSE / P of one self-attention case."""
    B, H, N, D = shape
    scale = D ** -0.5
    q, k, v, d_o = ar.self_inputs(kind, dt, shape)
    d_p = ar.self_dp(dt, shape) if with_dp else None
    Q, K, V, dO = (ar.heads(t, H) for t in (q, k, v, d_o))
    ref = ar.exact(Q, K, V, scale, dO, None if d_p is None else d_p.double().numpy())
    e_s = ar.dot_bound(Q, K, scale)
    bars, ref_err = ar.bars(dt, ref, ar.reference_arithmetic(q, k, v, d_o, H, scale, d_p), e_s)
    S2 = ar.scaled_operand(torch.from_numpy(Q).to(DT[dt]), scale, dt) @ K.transpose(0, 2, 1)
    m = S2.max(-1, keepdims=True)
    lse = (m + np.log2(np.exp2(S2 - m).sum(-1, keepdims=True)))
    return dict(q=q, k=k, v=v, d_o=d_o, d_p=d_p, ref=ref, bars=bars, ref_err=ref_err, e_s=e_s, lse=lse[..., 0],
                P=np.exp2(S2 - lse), scale=scale)


def run_flash(ops, case, H):
    q, k, v, d_o = (case[n].cuda() for n in ("q", "k", "v", "d_o"))
    o, lse = ops.self_attn_fwd(q, k, v, H, case["scale"])
    d_p = None if case["d_p"] is None else case["d_p"].cuda()
    dq, dk, dv = ops.self_attn_bwd(q, k, v, o, d_o, lse, H, case["scale"], d_probs=d_p)
    return {"O": o, "dQ": dq, "dK": dk, "dV": dv, "LSE": lse}


def check_flash(key, case, got, B, H):
    """Everything finite; O, dQ, dK, dV per tensor against float64; LSE element by element against the model's."""
    dt = key[2]
    for name, t in got.items():
        assert torch.isfinite(t).all(), f"{name} is not finite"
    failed = []
    for name in ("O", "dQ", "dK", "dV"):
        ref, bar = from_bh(case["ref"][name], B, H), case["bars"][name]
        if note(key, name, got[name], ref, case["ref_err"][name], bar) > bar:
            failed.append(name)
    lse = got["LSE"].double().cpu().numpy()
    atol = ar.lse_atol(dt, case["e_s"], case["lse"])
    worst = float((np.abs(lse - case["lse"]) / atol).max())
    print(f"[measured] {key[0]} {key[1]} {dt} {ar.ids(key[3])} LSE: worst |got - model| / atol {worst:.3f} (atol {atol.min():.2e} ... "
          f"{atol.max():.2e} log2 units)")
    assert not failed, f"{failed} above the bar (the [measured] lines hold the figures)"
    assert worst <= 1.0, f"LSE: {worst:.3f} x atol"


# ------------------------------------------------------------------------------------------------ flash self-attention
@pytest.mark.parametrize("kind,dt,shape", ar.SELF_CASES, ids=ar.ids)
def test_flash_forward_and_backward(ops, kind, dt, shape):
    """Measured on an MI355X (profiles/attention_rows.json): the largest kernel error / bar over all cases is 0.69 (sink8 f16
    (1,2,320,40) dQ, 4.1e-3 against 6e-3).  While the dK/dV kernel scaled its K fragments by scale log2e instead of taking the
    forward's rounded Q operand, ten 16-bit cases were above their bars in dK / dV — all four peaked shapes in f16 and bf16,
    shifted bf16 (1,2,320,40), sink8 bf16 (4,64,130,40); peaked bf16 (1,2,320,40) dV: 6.1e-2 against 4.8e-2, now 7.4e-3."""
    B, H, N, D = shape
    case = flash_case(kind, dt, shape)
    check_flash(("flash", kind, dt, shape), case, run_flash(ops, case, H), B, H)


@pytest.mark.parametrize("kind", ar.SELF_KINDS)
def test_fused_qkv_form_gives_the_same_bits(ops, kind):
    """Once through SelfAttentionFusedQKV: the bits of the separate-tensor entry points, which the test above holds to the bars."""
    shape = B, H, N, D = ar.SELF_SHAPES[0]
    q, k, v, d_o = (t.cuda() for t in ar.self_inputs(kind, "f16", shape))
    scale = D ** -0.5
    qkv = torch.cat([q, k, v], dim=-1).contiguous().requires_grad_(True)
    o = ops.SelfAttentionFusedQKV.apply(qkv, H, scale)
    o.backward(d_o)
    o2, lse = ops.self_attn_fwd(q, k, v, H, scale)
    grads = ops.self_attn_bwd(q, k, v, o2, d_o, lse, H, scale)
    assert torch.isfinite(o).all() and torch.isfinite(qkv.grad).all()
    assert torch.equal(o, o2) and torch.equal(qkv.grad, torch.cat(grads, dim=-1))


@pytest.mark.parametrize("dt,shape", [(dt, s) for s in ar.SELF_SHAPES[:3] for dt in ("f32", "f16", "bf16")
                                      if not (dt == "f32" and s[3] > 80)], ids=ar.ids)
def test_key_order_does_not_matter(ops, dt, shape):
    """One key set ascending, descending (every row's maximum in the first tile) and shuffled: each meets the bars (the test
    above), and O and dQ — which do not depend on the order of the keys — agree pairwise within the sum of the two bars."""
    B, H, N, D = shape
    got, bars, ref = {}, {}, None
    for kind in ("ascending", "descending", "shuffled"):
        case = flash_case(kind, dt, shape)
        got[kind], bars[kind] = run_flash(ops, case, H), case["bars"]
        if ref is not None:     # the float64 O and dQ are the same for the three orders, up to the order of float64 sums
            for name in ("O", "dQ"):
                assert ar.rel_err(case["ref"][name], ref[name]) < 1e-12
        ref = case["ref"]
    for a, b in (("ascending", "descending"), ("ascending", "shuffled"), ("descending", "shuffled")):
        for name in ("O", "dQ"):
            bar = bars[a][name] + bars[b][name]
            diff = float((got[a][name].double() - got[b][name].double()).abs().max().item() / np.abs(ref[name]).max())
            print(f"[measured] order {dt} {ar.ids(shape)} {name} {a} vs {b}: {diff:.3e} (bar {bar:.3e})")
            assert diff <= bar, f"{name}: {a} vs {b} differ by {diff:.3e} > {bar:.3e}"


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("kind", ["peaked", "sink8", "ascending"])
def test_stored_probabilities_element_by_element(ops, kind, dt):
    """self_attn_capture_fwd's P against the model's P = exp2(Q'.K - LSE) element by element: relative u_T (the store's rounding)
    + 2 ln2 x the LSE atol (the score and the row statistic), plus the floor of the type; the bits of self_attn_probs on the flash
    forward's LSE."""
    shape = B, H, N, D = ar.SELF_SHAPES[1]
    case = flash_case(kind, dt, shape)
    q, k, v = (case[n].cuda() for n in ("q", "k", "v"))
    o, lse, P = ops.self_attn_capture_fwd(q, k, v, H, case["scale"])
    o2, lse2 = ops.self_attn_fwd(q, k, v, H, case["scale"])
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    assert torch.equal(ops.self_attn_probs(q, k, lse2, H, case["scale"]), P)
    got = P.double().cpu().numpy()
    assert np.isfinite(got).all()
    rel = ar.UNIT[dt] + 2.0 * np.log(2.0) * ar.lse_atol(dt, case["e_s"], case["lse"])[..., None]
    bound = case["P"] * rel + ar.FLOOR[dt]
    worst = float((np.abs(got - case["P"]) / bound).max())
    old = float(np.abs(got - case["P"]).max())
    print(f"[measured] stored P {kind} {dt} {ar.ids(shape)}: worst |got - model| / bound {worst:.3f}; per-tensor metric {old:.3e} "
          f"(bar {TOL[dt]:.1e}); median row maximum {np.median(case['P'].max(-1)):.3f}")
    assert worst <= 1.0, f"P: {worst:.3f} x the element-wise bound"


@pytest.mark.parametrize("dt,shape", [(dt, s) for s in ar.SELF_SHAPES[:2] for dt in ("f32", "f16", "bf16")], ids=ar.ids)
def test_cotangent_on_stored_probabilities_with_sink_columns(ops, dt, shape):
    """ga_self_attn_bwd_dp on sink8 rows with a dense dP that is zero on the two sink columns: dQ, dK, dV per tensor, the
    gradients' rule (3 x TOL or the reference arithmetic's own error on sum(o dO) + sum(P dP))."""
    B, H, N, D = shape
    case = flash_case("sink8", dt, shape, with_dp=True)
    cols = ar.sink_columns(N)
    assert (case["d_p"][:, :, cols] == 0).all() and (case["d_p"] != 0).float().mean() > 0.98
    check_flash(("flash_dp", "sink8", dt, shape), case, run_flash(ops, case, H), B, H)


# ------------------------------------------------------------------------------------------------ cross-attention capture
@pytest.mark.parametrize("kind,dt,shape", ar.CROSS_CASES, ids=ar.ids)
def test_capture_forward_and_backward(ops, kind, dt, shape):
    B, H, N, Kt, D = shape
    scale = D ** -0.5
    key = ("capture", kind, dt, shape)
    q, k, v, d_o, m = ar.cross_inputs(kind, dt, shape)
    Q, K, V, dO = (ar.heads(t, H) for t in (q, k, v, d_o))
    d_p = m.unsqueeze(0).expand(B * H, N, Kt)
    ref = ar.exact(Q, K, V, scale, dO, d_p.double().numpy())
    e_s = ar.dot_bound(Q, K, scale)
    ra = ar.reference_arithmetic(q, k, v, d_o, H, scale, d_p)
    bars, ref_err = ar.bars(dt, ref, {n: ra[n] for n in ("O", "dQ")}, e_s, factor=2)
    qd, kd, vd, dod, md = (t.cuda() for t in (q, k, v, d_o, m))
    o, p = ops.attn_capture_fwd(qd, kd, vd, H, scale, True)
    dq = ops.attn_capture_bwd(qd, kd, vd, dod, md.unsqueeze(0).expand(B * H, N, Kt), H, scale)
    assert p.shape == (B * H, N, Kt)
    for name, t in (("O", o), ("P", p), ("dQ", dq)):
        assert torch.isfinite(t).all(), f"{name} is not finite"
    got = p.double().cpu().numpy()
    worst = float((np.abs(got - ref["P"]) / ar.p_bound(dt, ref["P"], e_s, Kt)).max())
    tokens = ref["P"][:, :, 1:] if Kt > 1 else ref["P"]
    print(f"[measured] capture {kind} {dt} {ar.ids(shape)} P: worst |got - fp64| / bound {worst:.3f}; per-tensor metric "
          f"{np.abs(got - ref['P']).max():.3e}; median P[:, 0] {np.median(ref['P'][:, :, 0]):.3f}, token columns median "
          f"{np.median(tokens):.1e}")
    o_err = note(key, "O", o, from_bh(ref["O"], B, H), ref_err["O"], TOL[dt])
    dq_err = note(key, "dQ", dq, from_bh(ref["dQ"], B, H), ref_err["dQ"], bars["dQ"])
    assert worst <= 1.0, f"P: {worst:.3f} x the element-wise bound"
    assert o_err <= TOL[dt], f"O: {o_err:.3e}"
    assert (p.float().sum(-1) - 1).abs().max().item() < {"f32": 1e-5, "f16": 4e-3, "bf16": 3e-2}[dt]   # as test_attn_capture_fwd
    assert dq_err <= bars["dQ"], f"dQ: {dq_err:.3e} > {bars['dQ']:.3e}"
