"""Attention inputs with the score rows a trained UNet produces, the float64 restatements the attention-row tests compare the
kernels with, and the bars those tests hold them to.  A plain helper module: numpy and CPU torch only, no GPU.

Row kinds (rows()).  u is one unit vector per head; q, k, v start as hashrand.normalish, spread 1 unless stated:
  benign      the control: q, k x 1.5 (what every other parity test feeds the kernels)
  peaked      q, k x 4: one key holds P ~ 1, |score| up to ~75
  shifted     q += 16 u, k += 16 u: every score carries a common +256 scale
  sink4/8     q += a u, k[0] += 4a u, and a second, weaker sink at key Kt // 2 + 3 (another key tile; clamped to the last key)
              whose score sits 3.5 natural-log units under key 0's: key 0 holds 0.9+ of the median row, the second a few %
  xsink4/5    the cross-attention form: q += a u, k[0] += 4a u, k[1:] -= a u / 2, with a stated at head size 40 and scaled by
              (D / 40)^1/4 elsewhere (the same score offsets at every head size) — key 0 (the BOS token) takes 0.9+ of every
              query and the token columns a loss reads sit at 1e-2 ... 1e-8
  ascending   k = 3 k + linspace(0, 40, Kt) u, q += 6 u: the row maximum rises along the key axis, tile after tile
  descending  the ascending keys and values in reverse order: the first tile holds every row's maximum
  shuffled    the ascending keys and values permuted jointly by a hashed permutation
The last three are ONE key set in three orders (key_order() gives the order): O and dQ do not depend on it.

Two bars ("Attention on trained rows"): a quantity is held, per tensor, to the larger of the bar its existing parity
test uses and the error of the reference's own arithmetic in that dtype (baddbmm(alpha=scale) -> softmax -> bmm with autograd on
the CPU, oracle.attention.attention_probs's op sequence) against the same float64 result; probabilities and LSE are held element
by element to bounds derived from the f32 dot product and one rounding to T."""
import math

import numpy as np
import torch

import hashrand
from oracle import attention as oattn

LOG2E = 1.4426950408889634
DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
TOL = {"f32": 2e-5, "f16": 2e-3, "bf16": 1.6e-2}                     # test_kernels_gpu.TOL
UNIT = {"f32": 2.0 ** -24, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}     # u_T: one rounding to T, relative
FLOOR = {"f32": 2.0 ** -126, "f16": 2.0 ** -24, "bf16": 2.0 ** -126}  # one subnormal step of f16; the smallest normal otherwise

PEAK, SHIFT, SECOND_SINK = 4.0, 16.0, 3.5
XSINK_STRONG = "xsink5"
SELF_KINDS = ["benign", "peaked", "shifted", "sink4", "sink8", "ascending", "descending", "shuffled"]
CROSS_KINDS = ["benign", "xsink4", XSINK_STRONG, "peaked"]

# B, H, N, D.  ONES row sum, 128-key tiles in 16 bit, 2.5 tiles | no ONES | NK > 5: 64-key tiles, 16 bit only |
# B * H * ceil(N / 128) = 512: the 32-query / 32-key-per-wave (CB = 2) kernels in both directions, partial last tiles
SELF_SHAPES = [(1, 2, 320, 40), (1, 2, 200, 64), (1, 2, 200, 160), (4, 64, 130, 40)]
# B, H, N, Kt, D.  the 64^2-layer form | the widest head | smaller than any tile | the 8-key-tile path
CROSS_SHAPES = [(1, 2, 256, 77, 40), (1, 2, 64, 77, 160), (1, 3, 17, 5, 8), (1, 2, 96, 128, 48)]
SELF_CASES = [(k, dt, s) for s in SELF_SHAPES for dt in ("f32", "f16", "bf16") if not (dt == "f32" and s[3] > 80)
              for k in SELF_KINDS]
CROSS_CASES = [(k, dt, s) for s in CROSS_SHAPES for dt in ("f32", "f16", "bf16") for k in CROSS_KINDS]
ids = lambda v: v if isinstance(v, str) else "x".join(map(str, v))  # noqa: E731


# ------------------------------------------------------------------------------------------------ builders
def key_order(kind, Kt, seed):
    """The order in which `kind` holds the ascending key set: kind's key j is the ascending set's key order[j]."""
    if kind == "descending":
        return np.arange(Kt)[::-1].copy()
    if kind == "shuffled":
        return np.argsort(hashrand.hash_u32(Kt, seed + 5), kind="stable")
    return np.arange(Kt)


def rows(kind, B, H, N, Kt, D, seed):
    """q (B, N, H*D), k, v (B, Kt, H*D) as float64 arrays, from hashrand only."""
    q = hashrand.normalish((B, H, N, D), seed).astype(np.float64)
    k = hashrand.normalish((B, H, Kt, D), seed + 1).astype(np.float64)
    v = hashrand.normalish((B, H, Kt, D), seed + 2).astype(np.float64)
    u = hashrand.normalish((H, D), seed + 4).astype(np.float64)
    u = (u / np.linalg.norm(u, axis=-1, keepdims=True))[None, :, None, :]          # (1, H, 1, D)
    if kind == "benign":
        q, k = q * 1.5, k * 1.5
    elif kind == "peaked":
        q, k = q * PEAK, k * PEAK
    elif kind == "shifted":
        q, k = q + SHIFT * u, k + SHIFT * u
    elif kind in ("sink4", "sink8") or kind[:5] == "xsink":
        a = float(kind[-1])
        if kind[0] == "x":
            a *= (D / 40.0) ** 0.25          # a is stated at head size 40: the same score offsets (a^2 D^-1/2) at every head size
            k[:, :, 1:] -= 0.5 * a * u
        else:
            # the second sink's score sits SECOND_SINK (natural-log units) under key 0's: e^-3.5 = 0.03 of key 0's share
            k[:, :, min(Kt // 2 + 3, Kt - 1)] += (4.0 * a - SECOND_SINK * math.sqrt(D) / a) * u[:, :, 0]
        q = q + a * u
        k[:, :, 0] += 4.0 * a * u[:, :, 0]
    elif kind in ("ascending", "descending", "shuffled"):
        order = key_order(kind, Kt, seed)
        k = (3.0 * k + np.linspace(0.0, 40.0, Kt)[None, None, :, None] * u)[:, :, order]
        v = v[:, :, order]
        q = q + 6.0 * u
    else:
        raise ValueError(kind)
    merge = lambda t: np.ascontiguousarray(t.transpose(0, 2, 1, 3).reshape(t.shape[0], t.shape[2], H * D))  # noqa: E731
    return merge(q), merge(k), merge(v)


def rounded(a, dt):
    """A float64 array as a CPU tensor of the test dtype (one rounding)."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(DT[dt])


def heads(t, H):
    """(B, N, H*D) tensor or array -> (B*H, N, D) float64 array (oracle layout)."""
    t = t.double().numpy() if torch.is_tensor(t) else np.asarray(t, np.float64)
    B, N, C = t.shape
    return np.ascontiguousarray(t.reshape(B, N, H, C // H).transpose(0, 2, 1, 3).reshape(B * H, N, C // H))


def self_inputs(kind, dt, shape, seed=500):
    """q, k, v, dO of a self-attention case as CPU tensors of the test dtype."""
    B, H, N, D = shape
    q, k, v = rows(kind, B, H, N, N, D, seed + N + D)
    d_o = hashrand.normalish((B, N, H * D), seed + 3 + N + D).astype(np.float64)
    return tuple(rounded(x, dt) for x in (q, k, v, d_o))


def sink_columns(N):
    return [0, min(N // 2 + 3, N - 1)]


def self_dp(dt, shape, seed=500):
    """A dense cotangent on the stored probabilities, zero on the two sink columns (no gradient reaches them)."""
    B, H, N, D = shape
    dp = hashrand.normalish((B * H, N, N), seed + 6 + N).astype(np.float64)
    dp[:, :, sink_columns(N)] = 0.0
    return rounded(dp, dt)


def cross_inputs(kind, dt, shape, seed=900):
    """q, k, v, dO (test dtype) and the broadcast dP map (N, Kt) of magnitude 3e-3, zero on the sink column: the shape of
    dLoss/dA."""
    B, H, N, Kt, D = shape
    q, k, v = rows(kind, B, H, N, Kt, D, seed + N + D)
    d_o = hashrand.normalish((B, N, H * D), seed + 3 + N + D).astype(np.float64)
    m = hashrand.normalish((N, Kt), seed + 6 + N).astype(np.float64) * 3e-3
    m[:, 0] = 0.0
    return tuple(rounded(x, dt) for x in (q, k, v, d_o, m))


# ------------------------------------------------------------------------------------------------ float64
def exact(Q, K, V, scale, dO, dP=None):
    """float64 O, dQ, dK, dV, P of softmax attention on (BH, N, D) arrays (oracle.attention's closed forms)."""
    P, O = oattn.capture_fwd_numpy(Q, K, V, scale)
    dQ, dK, dV = oattn.capture_bwd_numpy(Q, K, V, scale, dO, dP)
    return {"O": O, "dQ": dQ, "dK": dK, "dV": dV, "P": P}


def dot_bound(Q, K, scale):
    """e_s: the f32 dot-product bound on a score (natural-log units), (D + 2) 2^-24 scale max_nj sum_d |q_nd| |k_jd|."""
    D = Q.shape[-1]
    return (D + 2) * 2.0 ** -24 * scale * float((np.abs(Q) @ np.abs(K).transpose(0, 2, 1)).max())


def reference_arithmetic(q, k, v, d_o, H, scale, d_p=None):
    """O, dQ, dK, dV of the reference's op sequence in the tensors' own dtype on the CPU: baddbmm(alpha=scale) -> softmax -> bmm
    with autograd (oracle.attention.attention_probs); d_p (BH, N, Kt) or None: a cotangent on the probabilities.
    (BH, N, D) float64 arrays."""
    leaves = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
    qh, kh, vh = (oattn.head_split(t, H) for t in leaves)
    P = oattn.attention_probs(qh, kh, scale)
    o = torch.bmm(P, vh)
    if d_p is None:
        o.backward(oattn.head_split(d_o, H))
    else:
        torch.autograd.backward([o, P], [oattn.head_split(d_o, H), d_p])
    out = {"O": o.detach().double().numpy()}
    for name, t in zip(("dQ", "dK", "dV"), leaves):
        out[name] = heads(t.grad, H)
    return out


def rel_err(got, ref):
    """close()'s metric: the largest error as a fraction of the reference's largest magnitude."""
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def bars(dt, ref, ref_arith, e_s, factor=3):
    """The bar of each quantity, as a fraction of its float64 maximum: the larger of the existing test's (TOL for O, factor x TOL
    for gradients) and the reference arithmetic's own error (16 bit) or 4 e_s (f32).  Returns (bars, reference errors)."""
    out, ref_err = {}, {}
    for name in ref_arith:
        ref_err[name] = 4.0 * e_s if dt == "f32" else rel_err(ref_arith[name], ref[name])
        out[name] = max(TOL[dt] * (1 if name == "O" else factor), ref_err[name])
    return out, ref_err


def lse_atol(dt, e_s, lse):
    """LSE in log2 units against the model's: 2 (e_s log2e + 1.4427 u_T) + 2^-22 |LSE|."""
    return 2.0 * (e_s * LOG2E + LOG2E * UNIT[dt]) + 2.0 ** -22 * np.abs(lse)


# ------------------------------------------------------------------------------------------------ models of the kernels
def _rt(a, dt):
    """Round a float64 array to T (through f32, as the kernels' f32 accumulators are) and back."""
    return torch.from_numpy(np.ascontiguousarray(a)).float().to(DT[dt]).double().numpy()


def _pow2_rounded(dS, axis, dt):
    """dS rounded to T after a power-of-two scale that puts the largest magnitude along `axis` into [0.5, 1)."""
    amax = np.abs(dS).max(axis, keepdims=True)
    e = np.where(amax > 0, np.ceil(np.log2(np.where(amax > 0, amax, 1.0)) + 1e-12), 0.0)
    sc = 2.0 ** -e
    return _rt(dS * sc, dt) / sc


def scaled_operand(x, scale, dt):
    """round_T(x * scale * log2e): the f32 product of an operand of type T with the f32 constant, rounded to T."""
    c1 = np.float32(np.float32(scale) * np.float32(LOG2E))
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    return (t.float() * float(c1)).to(DT[dt]).double().numpy()


def flash_model(Q, K, V, scale, dt, dO, dP=None):
    """The flash kernels' documented roundings in float64, on (BH, N, D) arrays of values of T: Q' = round_T(Q scale log2e)
    in every kernel (the dK/dV kernel's Q image holds it too), P rounded to T before P.V, the row sum taken from the rounded P,
    LSE = m + log2 l, backward p = exp2(s - LSE), dS rounded to T after a per-row (dQ) or per-key (dK) power-of-two scale, outputs
    rounded to T.  Returns O, dQ, dK, dV, LSE (log2 units), P (= exp2(s - LSE), unrounded)."""
    Qs = scaled_operand(Q, scale, dt)
    S = Qs @ K.transpose(0, 2, 1)
    m = S.max(-1, keepdims=True)
    Pr = _rt(np.exp2(S - m), dt)
    l = Pr.sum(-1, keepdims=True)
    O = _rt(Pr @ V / l, dt)
    lse = m + np.log2(l)
    p = np.exp2(S - lse)
    delta = (dO * O).sum(-1, keepdims=True)
    dp = dO @ V.transpose(0, 2, 1) - delta
    if dP is not None:
        dp = dp + dP - (p * dP).sum(-1, keepdims=True)
    dQ = _rt(scale * (_pow2_rounded(p * dp, -1, dt) @ K), dt)
    dK = _rt(scale * (_pow2_rounded(p * dp, -2, dt).transpose(0, 2, 1) @ Q), dt)
    dV = _rt(_rt(p, dt).transpose(0, 2, 1) @ dO, dt)
    return {"O": O, "dQ": dQ, "dK": dK, "dV": dV, "LSE": lse[..., 0], "P": p}


def capture_model(Q, K, V, scale, dt, dO, dP):
    """attn_capture.hip in numpy: raw q.k and softmax_keys in float32 (exp2((acc - m) c1), sum, one reciprocal), P rounded to
    nearest T, O = round_T(P_T . V), dS = p (dp - sum p dp) rounded to T after the per-row power-of-two scale, dQ rounded to T."""
    acc = Q.astype(np.float32) @ K.astype(np.float32).transpose(0, 2, 1)
    c1 = np.float32(np.float32(scale) * np.float32(LOG2E))
    p = np.exp2(((acc - acc.max(-1, keepdims=True)) * c1).astype(np.float32)).astype(np.float32)
    p = (p * (np.float32(1.0) / p.sum(-1, keepdims=True, dtype=np.float32))).astype(np.float32)
    P = _rt(p, dt)
    O = _rt(P @ V, dt)
    p64 = p.astype(np.float64)
    dp = dO @ V.transpose(0, 2, 1) + (0.0 if dP is None else dP)
    dS = p64 * (dp - (dp * p64).sum(-1, keepdims=True))
    return {"P": P, "O": O, "dQ": _rt(scale * (_pow2_rounded(dS, -1, dt) @ K), dt)}


def p_bound(dt, ref, e_s, Kt):
    """Element-wise bound on a stored cross-attention probability: ref (u_T + 2 [2 e_s + (Kt + 8) 2^-24]) + floor."""
    return ref * (UNIT[dt] + 2.0 * (2.0 * e_s + (Kt + 8) * 2.0 ** -24)) + FLOOR[dt]
