"""The toRightOf, above and below relations inside the table loss launches (ga_aggregate_loss_rel_fwd_images /
ga_smooth_loss_rel_bwd_images) on the MI355X: against the plugins' calc_loss in float64 on the CPU (autograd), the role and the
axis of each kind against toLeftOf on swapped arguments and transposed maps, and the launches' contracts for the new kinds."""
import ctypes

import pytest
import torch

from test_relation_loss_gpu import _box, _coor, _evaluate, _plan, _table

pytestmark = pytest.mark.gpu

LEFT_OF, RIGHT_OF, ABOVE, BELOW = 0, 1, 2, 3
NAME = {LEFT_OF: "toLeftOf", RIGHT_OF: "toRightOf", ABOVE: "above", BELOW: "below"}
NEW_KINDS = {"toRightOf": RIGHT_OF, "above": ABOVE, "below": BELOW}


def _checker(rels):
    """The plugin of each (a, b, kind) with its sub-prompt lookup answered from the item -> [(plugin, args)]."""
    from guided_attention_amd import run
    out = []
    for a, b, kind in rels:
        fn = run.BUILTIN_LOSSES[NAME[kind]]()
        fn.find_indices_for_sub_prompt = {"A": list(a), "B": list(b)}.get
        out.append((fn, "(A, B)"))
    return out


def _plugin_total(A, entries, last, rels, dtype, device):
    """box loss + plugin relations of one image with autograd, as the plugin path forms them: float64 on the CPU (the box part
    from the oracle) or float32 on the GPU (the box part from ops.SmoothLoss) -> (loss, dA, [v of each relation's plugin])."""
    from guided_attention_amd import ops
    from guided_attention_amd.utils import shared_state as state
    from oracle import loss as oloss
    res, Kt = A.shape[0], A.shape[-1]
    A = A.to(device=device, dtype=dtype).clone().requires_grad_(True)
    total = A.new_zeros(1)
    if entries:
        if dtype == torch.float64:
            tp = oloss.TokenPlan(entries, dict(state.hyperParameterOverrides))
            total = total + oloss.loss_torch(A, tp, normalize_eot=last != Kt - 1, n_prompt_tokens=last + 1)["loss"]
        else:
            total = total + ops.SmoothLoss.apply(A.reshape(res * res, Kt), res, 1, last, _plan(entries))[1]
    text = torch.softmax(A[:, :, 1:last] * 100, dim=-1)
    values = []
    for fn, args in _checker(rels):
        values.append(fn.calc_loss(text, args))
        total = total + values[-1]
    (g,) = torch.autograd.grad(total.sum(), [A])
    return (total.detach().double().cpu().reshape(()), g.detach().double().cpu().reshape(res * res, Kt),
            [float(v.detach().double().cpu()) for v in values])


def _random_map(res, Kt, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.softmax(torch.randn(res, res, Kt, generator=g) * 2, -1)


def _small_case(kind):
    """res 8, Kt 12, the slice [1, 9), |a| = 2 and |b| = 3, slice index 2 shared with a BOX token, on a random softmaxed map
    (that of test_relation_loss_gpu's small case).  With every centroid mid-map the reference's divisor (the "left" role's
    token count under BOTH sums) gives v = (1.4 n_lead - n_other) * 4.5 / n_lead: open for toRightOf and below (the role is
    b's, 3 tokens), but closed for above (a's, 2 tokens) — on such a map `above` would be checked on a zero relation gradient.
    For `above` alone the logits of b's tokens therefore fall off along both axes (by 3 over the map) before the softmax that
    makes the map: b's centroids move towards the origin and the hinge opens (float64 plugin: v = 4.48)."""
    a, b = [2, 5], [0, 3, 6]
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(8, 8, 12, generator=g) * 2
    if kind == ABOVE:
        ramp = (torch.arange(8, dtype=torch.float32) + .5) / 8
        for i in b:
            logits[:, :, 1 + i] -= 3 * (ramp[:, None] + ramp[None, :])
    return torch.softmax(logits, -1), [_box(3, (.1, .2, .6, .6), "cat")], 9, [(a, b, kind)]


def _res16_case(kind):
    """res 16, Kt 77, the slice [1, 76): both relation columns are guided COOR tokens too."""
    return _random_map(16, 77, 21), [_coor(2, (.2, .5), "cat"), _coor(5, (.7, .5), "vase")], 76, [([1], [4], kind)]


def _res24_case(kind):
    """SD-2.1's map: 576 pixels on 256 threads, a res that is no power of two."""
    return _random_map(24, 77, 22), [_box(3, (.1, .2, .6, .6), "cat")], 76, [([2, 7], [4, 9], kind)]


SHAPES = {"res8_kt12": _small_case, "res16_kt77": _res16_case, "res24_kt77": _res24_case}

# The tests below print their figures ([measured] lines: error against float64 relative to the loss / the gradient's maximum, for
# the kernels and for the float32 plugin path).  Measured on the MI355X, kernel (float32 plugin path):
#   toRightOf  res8_kt12   loss 3.1e-8 (4.0e-8)  gradient 3.5e-7 (2.4e-6)
#   toRightOf  res16_kt77  loss 2.7e-7 (5.5e-8)  gradient 4.9e-7 (2.6e-6)
#   toRightOf  res24_kt77  loss 1.8e-7 (5.0e-9)  gradient 1.8e-7 (1.2e-6)
#   above      res8_kt12   loss 1.6e-7 (2.9e-8)  gradient 2.1e-7 (3.7e-7)
#   above      res16_kt77  loss 2.4e-7 (2.4e-7)  gradient 8.3e-7 (1.5e-6)
#   above      res24_kt77  loss 2.1e-8 (4.4e-7)  gradient 3.7e-7 (1.3e-6)
#   below      res8_kt12   loss 7.6e-8 (8.1e-9)  gradient 5.0e-7 (2.2e-6)
#   below      res16_kt77  loss 1.0e-8 (1.0e-8)  gradient 3.9e-7 (6.0e-7)
#   below      res24_kt77  loss 2.1e-7 (2.2e-7)  gradient 2.0e-7 (1.3e-6)
#   four kinds in one row (res 16): loss 3.8e-8 (2.2e-7), gradient 5.0e-7 (4.6e-7)
#   role and axis (res 24): v equal to the last bit in all three pairs, dA 2.3e-7 / 2.8e-7 / 3.6e-7
#   res32 (test_res32_plan_without_resident_columns): loss 5.4e-8, gradient 4.0e-7
# On the res8_kt12 map tilted for toRightOf as it is for `above` (a's logits falling off instead of b's) the kernel's gradient
# read 1.66e-6 against the float32 plugin path's 6.7e-7 — over max(2 x 6.7e-7, 1e-6); both are float32 rounding of the same
# size, and toRightOf needs no tilt to open its hinge, so it runs on the plain random map.


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("kind", sorted(NEW_KINDS))
def test_new_kinds_loss_and_gradient_vs_float64_plugin(kind, shape):
    """Loss and dA against the kind's plugin in float64 (plus the oracle's box loss), with the project's bounds for the table
    loss (1e-4 of the loss, 2e-3 of the gradient's maximum); and no worse than max(twice the float32 plugin path, 1e-6) on the
    same inputs, as test_relation_loss_and_gradient_vs_float64_plugin asks of toLeftOf."""
    A, entries, last, rels = SHAPES[shape](NEW_KINDS[kind])
    res = A.shape[0]
    out = _evaluate(_table([(entries, last, rels)], res), A[None])
    l64, g64, _ = _plugin_total(A, entries, last, rels, torch.float64, "cpu")
    l32, g32, _ = _plugin_total(A, entries, last, rels, torch.float32, "cuda")
    loss = (out["box"] + out["rel"]).double().cpu()[0]
    gmax = g64.abs().max()
    e_loss, e_grad = abs(loss - l64) / abs(l64), (out["dA"][0].double().cpu() - g64).abs().max() / gmax
    p_loss, p_grad = abs(l32 - l64) / abs(l64), (g32 - g64).abs().max() / gmax
    print(f"\n[measured] {kind} {shape}: kernel loss {e_loss:.2e} grad {e_grad:.2e} | plugin f32 loss {p_loss:.2e} grad {p_grad:.2e} "
          f"| loss {l64:.8f} rel {out['rel'][0].item():.8f}")
    assert out["rel"][0] > 0                       # the hinge is open: the relation's gradient is part of dA
    assert e_loss <= 1e-4 and e_grad <= 2e-3
    assert e_loss <= max(2 * p_loss, 1e-6) and e_grad <= max(2 * p_grad, 1e-6)
    value, v, t2, t3 = out["rel_terms"][0, 0].tolist()
    assert value == max(v, 0.0) and abs(v - (t2 + .2 * res - t3) / res * 9) <= 1e-5 * abs(v)
    assert not out["rel_terms"][0, 1:].any()
    assert torch.equal(out["dPb"], out["dA"] * .125)


def test_one_row_with_all_four_kinds():
    """R = 4, one relation of each kind at res 16.  Slice index 2 is a guided BOX token, the "left" role of a horizontal
    relation and an argument of two vertical ones; index 5 is a guided COOR token in a horizontal and a vertical relation."""
    res, last = 16, 76
    A = _random_map(res, 77, 34)   # a seed whose four float64 plugin values are all positive (2.9, 4.7, 2.9, 2.3)
    entries = [_box(3, (.1, .2, .6, .6), "cat"), _coor(6, (.7, .3), "ball")]
    rels = [([2], [5], LEFT_OF), ([2, 8], [9], ABOVE), ([7], [2], RIGHT_OF), ([5], [2], BELOW)]
    out = _evaluate(_table([(entries, last, rels)], res), A[None])
    l64, g64, v64 = _plugin_total(A, entries, last, rels, torch.float64, "cpu")
    l32, g32, _ = _plugin_total(A, entries, last, rels, torch.float32, "cuda")
    loss = (out["box"] + out["rel"]).double().cpu()[0]
    gmax = g64.abs().max()
    e_loss, e_grad = abs(loss - l64) / abs(l64), (out["dA"][0].double().cpu() - g64).abs().max() / gmax
    p_loss, p_grad = abs(l32 - l64) / abs(l64), (g32 - g64).abs().max() / gmax
    print(f"\n[measured] four kinds: kernel loss {e_loss:.2e} grad {e_grad:.2e} | plugin f32 loss {p_loss:.2e} grad {p_grad:.2e} "
          f"| loss {l64:.8f} rel {out['rel'][0].item():.8f} values {[round(v, 4) for v in v64]}")
    assert e_loss <= 1e-4 and e_grad <= 2e-3
    assert e_loss <= max(2 * p_loss, 1e-6) and e_grad <= max(2 * p_grad, 1e-6)
    for r in range(4):
        value, v, t2, t3 = out["rel_terms"][0, r].tolist()
        assert value == max(v, 0.0) and value > 0, r                       # every hinge is open: all four enter dA
        assert abs(v - (t2 + .2 * res - t3) / res * 9) <= 1e-5 * abs(v), r
        assert abs(value - v64[r]) <= 1e-5 * v64[r], r                      # each row is its own kind's value
    assert abs(out["rel"][0].item() - sum(v64)) <= 1e-5 * sum(v64)


def test_role_and_axis_against_to_left_of():
    """toRightOf (a, b) against toLeftOf (b, a), below (a, b) against above (b, a), above (a, b) on A against toLeftOf (a, b)
    on the spatially transposed map: v within 1e-6 relative (only the order of a few float32 additions differs), dA within
    2e-3 of its maximum after transposing back.  res 24, relations alone (T = 0), 2 tokens against 3."""
    res, Kt, last = 24, 12, 9
    A = _random_map(res, Kt, 41)
    two, three = [2, 5], [0, 3, 6]

    def run(A, item):
        out = _evaluate(_table([([], last, [item])], res), A[None])
        return out["rel_terms"][0, 0, 1].item(), out["dA"][0].reshape(res, res, Kt)

    pairs = [("toRightOf", run(A, (two, three, RIGHT_OF)), run(A, (three, two, LEFT_OF)), False),
             ("below", run(A, (two, three, BELOW)), run(A, (three, two, ABOVE)), False),
             ("above", run(A, (three, two, ABOVE)), run(A.transpose(0, 1).contiguous(), (three, two, LEFT_OF)), True)]
    for name, (v, dA), (v_ref, dA_ref), transposed in pairs:
        if transposed:
            dA_ref = dA_ref.transpose(0, 1)
        e_v, e_grad = abs(v - v_ref) / abs(v_ref), ((dA - dA_ref).abs().max() / dA_ref.abs().max()).item()
        print(f"\n[measured] {name}: v {v:.7f} against {v_ref:.7f} ({e_v:.1e}), dA {e_grad:.1e}")
        assert v > 0 and dA.any(), name                       # open hinges: no pair agrees on zeros
        assert e_v <= 1e-6 and e_grad <= 2e-3, name
    # the axis is the kind's: `above` on A is not toLeftOf on A
    assert abs(pairs[2][1][0] - run(A, (three, two, LEFT_OF))[0]) > 1e-3


def _closed_map(res, Kt, a, b, kind, seed=3):
    """a's mass and b's mass at opposite edges of the kind's axis, a where the relation wants it: the "left" role's centroid is
    .5, the other one's res - .5, v < 0."""
    g = torch.Generator().manual_seed(seed)
    A = torch.softmax(torch.randn(res, res, Kt, generator=g) * 2, -1)
    A[:, :, 1 + a] = 0
    A[:, :, 1 + b] = 0
    at_a, at_b = (-1, 0) if kind in (RIGHT_OF, BELOW) else (0, -1)
    if kind in (LEFT_OF, RIGHT_OF):
        A[:, at_a, 1 + a] = .9
        A[:, at_b, 1 + b] = .9
    else:
        A[at_a, :, 1 + a] = .9
        A[at_b, :, 1 + b] = .9
    return A


@pytest.mark.parametrize("kind", sorted(NEW_KINDS))
def test_closed_hinge_adds_nothing(kind):
    k = NEW_KINDS[kind]
    entries = [_box(3, (.1, .2, .6, .6), "cat"), _coor(5, (.6, .4), "vase")]
    A = _closed_map(8, 12, 2, 6, k)
    with_rel = _evaluate(_table([(entries, 11, [([2], [6], k)])], 8), A[None])
    without = _evaluate(_table([(entries, 11, None)], 8, Q_max=4), A[None])
    assert with_rel["rel"][0] == 0 and with_rel["rel_terms"][0, 0, 1] < 0 and with_rel["rel_terms"][0, 0, 0] == 0
    assert torch.equal(with_rel["dA"], without["dA"]) and torch.equal(with_rel["dPb"], without["dPb"])
    assert torch.equal(with_rel["box"], without["box"]) and with_rel["dA"].any()
    # the same map with the arguments exchanged is wide open; next to the closed relation it moves dA
    mixed = _evaluate(_table([(entries, 11, [([2], [6], k), ([6], [2], k)])], 8), A[None])
    assert mixed["rel_terms"][0, 0, 0] == 0 and mixed["rel_terms"][0, 1, 0] > 0 and mixed["rel"][0] == mixed["rel_terms"][0, 1, 0]
    assert not torch.equal(mixed["dA"], without["dA"])


def test_rows_without_a_relation_and_idle_images():
    """Three images: the rows without a relation are bit-identical to the plain table launches; dloss == 0 gives exact zeros."""
    from guided_attention_amd import ops
    res, last = 16, 76
    A = torch.stack([_random_map(res, 77, 51 + s) for s in range(3)])
    entries = [_coor(2, (.2, .5), "cat"), _coor(5, (.7, .5), "vase")]
    rows = [(entries, last, None), (entries, last, [([1], [4], ABOVE), ([4], [7], RIGHT_OF)]), ([], last, None)]
    table = _table(rows, res)
    out = _evaluate(table, A)
    plans = [_plan(e) for e, _, _ in rows]
    plain = ops.ImageTable(3, 4, res, True, .5, 3, torch.device("cuda")).set(plans, [(1, last)] * 3)
    A_dev, terms, loss = ops.aggregate_loss_fwd_images([A.reshape(3, res * res, 77).cuda()], plain)
    dA, dPb = ops.smooth_loss_bwd_images(A_dev, plain, torch.ones(3, device="cuda"), bcast_dtype=torch.float32, bcast_scale=.125)
    assert ops.tickets_are_zero()
    assert torch.equal(out["terms"], terms) and torch.equal(out["box"], loss)
    for s in (0, 2):
        assert torch.equal(out["dA"][s], dA[s]) and torch.equal(out["dPb"][s], dPb[s]), s
        assert out["rel"][s] == 0 and not out["rel_terms"][s].any()
    assert out["rel"][1] > 0 and (out["rel_terms"][1, :2, 0] > 0).all() and not torch.equal(out["dA"][1], dA[1])
    idle = _evaluate(table, A, torch.tensor([1.0, 0.0, 1.0], device="cuda"))
    assert not idle["dA"][1].any() and not idle["dPb"][1].any() and not torch.signbit(idle["dA"][1]).any()
    assert torch.equal(idle["dA"][0], out["dA"][0]) and torch.equal(idle["rel"], out["rel"])


def test_an_unknown_kind_gives_nan_and_zeros():
    """kind = 99 written into the device row behind the host's back: the kernels screen it (rel_setup)."""
    from guided_attention_amd import _lib
    A, entries, last, rels = _small_case(BELOW)
    good = _evaluate(_table([(entries, last, rels)], 8), A[None])
    assert torch.isfinite(good["rel"]).all() and good["dA"].any()
    for bad in (99, 4, -1):
        table = _table([(entries, last, rels)], 8)
        rows = (_lib.ga_image_relations_t * 1).from_buffer_copy(bytes(table.rel_rows))
        rows[0].rel[0].kind = bad
        assert ctypes.sizeof(rows) == table.device_rel_rows.numel()
        table.device_rel_rows.copy_(torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8))
        out = _evaluate(table, A[None])
        assert torch.isnan(out["box"]).all() and torch.isnan(out["rel"]).all(), bad
        assert not out["terms"].any() and not out["rel_terms"].any() and not out["dA"].any() and not out["dPb"].any(), bad


def test_res32_plan_without_resident_columns():
    """Three images at res 32 with a 16-slot table and Q_max 4: the backward runs without resident columns on 64 staged rows
    (every relation column value is re-read from global memory).  Image 1 carries an `above` and a `toRightOf` relation."""
    from guided_attention_amd import ops
    res, last, T_max, Q_max = 32, 76, 16, 4
    got = ops.loss_lds_plan("bwd", 32, 77, 16, images=3, table=True, Q_max=4)
    assert (got.use_gcol, got.stage_rows) == (0, 64)
    entries = [_box(3, (.1, .2, .6, .6), "cat"), _coor(8, (.7, .3), "ball")]
    rels = [([2, 5], [0], ABOVE), ([5], [2], RIGHT_OF)]
    rows = [([_coor(4, (.3, .6), "dog")], last, None), (entries, last, rels), ([], 40, None)]
    A = torch.stack([_random_map(res, 77, 61 + s) for s in range(3)])
    out = _evaluate(_table(rows, res, T_max=T_max, Q_max=Q_max), A)
    l64, g64, v64 = _plugin_total(A[1], entries, last, rels, torch.float64, "cpu")
    loss = (out["box"] + out["rel"]).double().cpu()[1]
    e_loss, e_grad = abs(loss - l64) / abs(l64), (out["dA"][1].double().cpu() - g64).abs().max() / g64.abs().max()
    print(f"\n[measured] res32: kernel loss {e_loss:.2e} grad {e_grad:.2e} rel {out['rel'][1].item():.6f} values {v64}")
    assert out["rel"][1] > 0 and min(v64) > 0 and e_loss <= 1e-4 and e_grad <= 2e-3
    assert out["rel"][0] == 0 and out["rel"][2] == 0 and not out["dA"][2].any()
