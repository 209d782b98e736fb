"""The toLeftOf relation loss inside the table loss launches (ga_aggregate_loss_rel_fwd_images / ga_smooth_loss_rel_bwd_images)
on the MI355X: against run.ToLeftOf.calc_loss itself in float64 on the CPU (autograd), and the launch's contracts — R = 0 rows
bit-identical to the plain table launches, T = 0 rows served, closed hinges, isolation between images, idle images."""
import numpy as np
import pytest
import torch

from conftest import load_json, load_npz

pytestmark = pytest.mark.gpu


def _coor(i, g, sub):
    return {"index": i, "kind": "COOR", "geom": g, "subprompt": sub}


def _box(i, g, sub):
    return {"index": i, "kind": "BOX", "geom": g, "subprompt": sub}


def _plan(entries, hyper=None):
    from guided_attention_amd import ops
    from guided_attention_amd.utils import shared_state as state
    return ops.LossPlan(entries, dict(state.hyperParameterOverrides, **(hyper or {})), True, .5, 3, False)


def _table(rows, res, T_max=None, Q_max=None):
    """rows: [(entries, last of the slice, [(left, right)] or None)] -> ImageTable with relation rows."""
    from guided_attention_amd import ops
    plans = [_plan(e) for e, _, _ in rows]
    rels = [ops.RelationPlan(r) if r else None for _, _, r in rows]
    T_max = T_max or ops.image_table_capacity(max(p.T for p in plans))
    Q_max = Q_max or ops.relation_capacity(max([len(r.columns) for r in rels if r] + [1]))
    table = ops.ImageTable(len(rows), T_max, res, True, .5, 3, torch.device("cuda"), Q_max=Q_max)
    return table.set(plans, [(1, last) for _, last, _ in rows], rels)


def _evaluate(table, A, dloss=None):
    """A (S, res, res, Kt) f32 on the CPU -> everything the two launches write (one f32 head-map per image: its mean is A)."""
    from guided_attention_amd import ops
    S, res, _, Kt = A.shape
    maps = [A.reshape(S, res * res, Kt).cuda().contiguous()]
    A_dev, terms, box, rel_terms, rel = ops.aggregate_loss_rel_fwd_images(maps, table)
    assert torch.equal(A_dev, maps[0])
    dloss = torch.ones(S, device="cuda") if dloss is None else dloss
    dA, dPb = ops.smooth_loss_rel_bwd_images(A_dev, table, dloss, bcast_dtype=torch.float32, bcast_scale=.125)
    assert ops.tickets_are_zero()
    return dict(terms=terms, box=box, rel_terms=rel_terms, rel=rel, dA=dA, dPb=dPb)


def _checker(rels):
    """run.ToLeftOf with its sub-prompt lookup answered from `rels` (calc_loss itself is the plugin's): -> [(plugin, args)]."""
    from guided_attention_amd import run
    out = []
    for left, right in rels:
        fn = run.ToLeftOf()
        fn.find_indices_for_sub_prompt = {"L": list(left), "R": list(right)}.get
        out.append((fn, "(L, R)"))
    return out


def _plugin_total(A, entries, last, rels, dtype, device):
    """box loss + plugin relations of one image with autograd, as the plugin path forms them: float64 on the CPU (the box part
    from the oracle) or float32 on the GPU (the box part from ops.SmoothLoss, the relations in torch) -> (loss, dA)."""
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
    for fn, args in _checker(rels):
        total = total + fn.calc_loss(text, args)
    (g,) = torch.autograd.grad(total.sum(), [A])
    return total.detach().double().cpu().reshape(()), g.detach().double().cpu().reshape(res * res, Kt)


def _g10_case(name):
    meta = load_json("g10_custom_loss.json")
    A = torch.from_numpy(load_npz("g10_custom_loss.npz")[f"{name}.A"])
    entries = [_coor(2, tuple(meta["meta_info"][0][2]), "cat"), _coor(5, tuple(meta["meta_info"][1][2]), "vase")]
    return A, entries, 76, [([1], [4])]     # cat and vase are guided COOR tokens AND the relation's columns


def _small_case():
    g = torch.Generator().manual_seed(5)
    A = torch.softmax(torch.randn(8, 8, 12, generator=g) * 2, -1)
    entries = [_box(3, (.1, .2, .6, .6), "cat")]      # slice index 2: shared with the relation's left side
    return A, entries, 9, [([2, 5], [0, 3, 6])]       # the SD-2.1 slice [1, 9): last < Kt - 1, |L| = 2, |R| = 3


CASES = {"g10_bos": lambda: _g10_case("bos"), "g10_sharp": lambda: _g10_case("sharp"), "res8_kt12": _small_case}

# The test below prints its figures ([measured] lines: error against float64 relative to the loss / the gradient's maximum, for the
# kernels and for the float32 plugin path).  Measured on the MI355X, kernel (float32 plugin path):
#   g10_bos    loss 8.8e-8 (1.5e-7)  gradient 4.5e-7 (1.4e-6)
#   g10_sharp  loss 1.6e-7 (9.6e-9)  gradient 8.6e-7 (1.9e-6)
#   res8_kt12  loss 3.1e-7 (3.1e-7)  gradient 5.4e-7 (2.4e-6)
#   res32 (test_res32_plan_without_resident_columns): loss 2.2e-8, gradient 3.2e-7


@pytest.mark.parametrize("case", sorted(CASES))
def test_relation_loss_and_gradient_vs_float64_plugin(case):
    """Loss and dA against run.ToLeftOf.calc_loss in float64 (plus the oracle's box loss), with the project's bounds for the table
    loss (1e-4 of the loss, 2e-3 of the gradient's maximum); and no worse than twice the float32 plugin path on the same
    inputs.  Floors of that comparison: 1e-6 of the gradient's maximum (given), and 1e-6 of the loss — a float32 sum of 256
    products carries about sqrt(256) * 2^-24 = 1e-6 of rounding, which either path may or may not happen to cancel."""
    A, entries, last, rels = CASES[case]()
    res = A.shape[0]
    out = _evaluate(_table([(entries, last, rels)], res), A[None])
    l64, g64 = _plugin_total(A, entries, last, rels, torch.float64, "cpu")
    l32, g32 = _plugin_total(A, entries, last, rels, torch.float32, "cuda")
    loss = (out["box"] + out["rel"]).double().cpu()[0]
    gmax = g64.abs().max()
    e_loss, e_grad = abs(loss - l64) / abs(l64), (out["dA"][0].double().cpu() - g64).abs().max() / gmax
    p_loss, p_grad = abs(l32 - l64) / abs(l64), (g32 - g64).abs().max() / gmax
    print(f"\n[measured] {case}: kernel loss {e_loss:.2e} grad {e_grad:.2e} | plugin f32 loss {p_loss:.2e} grad {p_grad:.2e} "
          f"| loss {l64:.8f} rel {out['rel'][0].item():.8f}")
    assert out["rel"][0] > 0                       # the hinge is open: the relation's gradient is part of dA
    assert e_loss <= 1e-4 and e_grad <= 2e-3
    assert e_loss <= max(2 * p_loss, 1e-6) and e_grad <= max(2 * p_grad, 1e-6)
    # rel_terms: (value, v, cL, cR) of relation 0, zero rows behind it
    value, v, cL, cR = out["rel_terms"][0, 0].tolist()
    assert value == max(v, 0.0) and abs(v - (cL + .2 * res - cR) / res * 9) <= 1e-5 * abs(v)
    assert not out["rel_terms"][0, 1:].any()
    assert torch.equal(out["dPb"], out["dA"] * .125)


def test_fixture_numbers_of_the_reference():
    """The reference's own loss and autograd gradient (g10) for the relation alone: T = 0, R = 1."""
    g = load_npz("g10_custom_loss.npz")
    for name in ("bos", "sharp"):
        A = torch.from_numpy(g[f"{name}.A"])
        out = _evaluate(_table([([], 76, [([1], [4])])], 16), A[None])
        assert out["box"][0] == 0 and not out["terms"].any()
        np.testing.assert_allclose(out["rel"].cpu().numpy(), g[f"{name}.loss"], rtol=2e-5, atol=1e-6)
        ref = g[f"{name}.dA"].reshape(256, 77)
        assert np.abs(out["dA"][0].cpu().numpy() - ref).max() <= 2e-3 * np.abs(ref).max()


def test_rows_without_a_relation_are_bit_identical_to_the_table_launches():
    from guided_attention_amd import ops
    A0, entries, last, rels = _g10_case("sharp")
    A = torch.stack([A0.flip(1), A0, A0.flip(0)])
    rows = [(entries, last, None), (entries, last, rels), ([], last, None)]
    out = _evaluate(_table(rows, 16), A)
    plans = [_plan(e) for e, _, _ in rows]
    plain = ops.ImageTable(3, 4, 16, True, .5, 3, torch.device("cuda")).set(plans, [(1, last)] * 3)
    maps = [A.reshape(3, 256, 77).cuda()]
    A_dev, terms, loss = ops.aggregate_loss_fwd_images(maps, plain)
    dA, dPb = ops.smooth_loss_bwd_images(A_dev, plain, torch.ones(3, device="cuda"), bcast_dtype=torch.float32, bcast_scale=.125)
    assert torch.equal(out["terms"], terms) and torch.equal(out["box"], loss)        # the box part: every image
    for s in (0, 2):
        assert torch.equal(out["dA"][s], dA[s]) and torch.equal(out["dPb"][s], dPb[s]), s
        assert out["rel"][s] == 0 and not out["rel_terms"][s].any()
    assert not out["dA"][2].any()
    assert not torch.equal(out["dA"][1], dA[1])                                      # image 1's relation is open


def test_relation_alone_equals_the_relation_part():
    """T = 0, R = 1: loss and gradient are the relation's alone (float64 plugin, at the solo kernels' bounds: 5e-5 of the loss and
    of the gradient's maximum), the box outputs are zero."""
    A, _, last, rels = _small_case()
    out = _evaluate(_table([([], last, rels)], 8), A[None])
    l64, g64 = _plugin_total(A, [], last, rels, torch.float64, "cpu")
    assert out["box"][0] == 0 and not out["terms"].any()
    assert abs(out["rel"][0].item() - l64) <= 5e-5 * abs(l64)
    assert (out["dA"][0].double().cpu() - g64).abs().max() <= 5e-5 * g64.abs().max()


def _closed_map(res, Kt, left, right, seed=3):
    """The left token's mass in column 0, the right token's in the last column: cL - cR = 1 - res, the hinge is closed."""
    g = torch.Generator().manual_seed(seed)
    A = torch.softmax(torch.randn(res, res, Kt, generator=g) * 2, -1)
    A[:, :, 1 + left] = 0
    A[:, :, 1 + right] = 0
    A[:, 0, 1 + left] = .9
    A[:, -1, 1 + right] = .9
    return A


def test_closed_hinge_adds_nothing():
    entries = [_box(3, (.1, .2, .6, .6), "cat"), _coor(5, (.6, .4), "vase")]
    A = _closed_map(8, 12, 2, 6)
    with_rel = _evaluate(_table([(entries, 11, [([2], [6])])], 8), A[None])
    without = _evaluate(_table([(entries, 11, None)], 8, Q_max=4), A[None])
    assert with_rel["rel"][0] == 0 and with_rel["rel_terms"][0, 0, 1] < 0
    assert torch.equal(with_rel["dA"], without["dA"]) and torch.equal(with_rel["dPb"], without["dPb"])
    assert torch.equal(with_rel["box"], without["box"]) and with_rel["dA"].any()


def test_images_are_isolated_and_idle_images_get_zeros():
    A0, entries, last, rels = _g10_case("bos")
    A1 = _g10_case("sharp")[0]
    rows = [(entries, last, rels), (entries[:1], last, None), ([], last, [([0, 1], [4])])]
    A = torch.stack([A0, A1, A1.flip(0)])
    table = _table(rows, 16)
    first = _evaluate(table, A)
    assert first["rel"][0] > 0 and first["rel"][1] == 0 and first["dA"][2].any()
    A2 = A.clone()
    A2[2] = A0.flip(1)
    rows2 = rows[:2] + [(entries, last, [([7], [2, 3])])]
    second = _evaluate(_table(rows2, 16), A2)       # image 2: another map and another row pair
    for k in ("terms", "box", "rel_terms", "rel", "dA", "dPb"):
        assert torch.equal(first[k][:2], second[k][:2]), k
    assert not torch.equal(first["dA"][2], second["dA"][2])
    idle = _evaluate(table, A, torch.tensor([1.0, 0.0, 1.0], device="cuda"))
    assert not idle["dA"][1].any() and not idle["dPb"][1].any() and not torch.signbit(idle["dA"][1]).any()
    assert torch.equal(idle["dA"][0], first["dA"][0]) and torch.equal(idle["dA"][2], first["dA"][2])
    # dloss enters as one factor of the last product (dloss * 100 * S * ...): doubling it doubles every element exactly, except
    # where 100 * S is below the smallest normal float32 (1.2e-38; S underflows on these maps) and loses bits that 200 * S keeps
    scaled = _evaluate(table, A, torch.tensor([2.0, 1.0, 1.0], device="cuda"))
    diff = (scaled["dA"][0] - first["dA"][0] * 2).abs().max().item()
    print(f"\n[measured] dloss 2 against twice dloss 1: max difference {diff:.2e}")
    assert diff <= 1e-30


def test_unservable_relation_rows_give_nan_and_zeros():
    """What ImageTable.set refuses on the host, written into the device rows directly: the kernels screen them (row_ok)."""
    import ctypes
    from guided_attention_amd import _lib
    A, entries, last, rels = _small_case()
    good = _evaluate(_table([(entries, last, rels)], 8), A[None])
    assert torch.isfinite(good["rel"]).all()

    def broken(edit, Q_max=None, rels=rels):
        table = _table([(entries, last, rels)], 8, Q_max=Q_max)
        rows = (_lib.ga_image_relations_t * 1).from_buffer_copy(bytes(table.rel_rows))
        edit(rows[0])
        table.device_rel_rows.copy_(torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8))
        assert ctypes.sizeof(rows) == table.device_rel_rows.numel()
        return _evaluate(table, A[None])

    def set_field(path, value):
        def edit(row):
            obj = row
            for name in path[:-1]:
                obj = getattr(obj, name) if isinstance(name, str) else obj[name]
            if isinstance(path[-1], str):
                setattr(obj, path[-1], value)
            else:
                obj[path[-1]] = value
        return edit

    for edit in (set_field(("R",), 5), set_field(("R",), -1), set_field(("rel", 0, "n_left"), 0),
                 set_field(("rel", 0, "n_right"), 9), set_field(("rel", 0, "right", 1), 8),
                 set_field(("rel", 0, "left", 0), -1)):
        out = broken(edit)
        assert torch.isnan(out["box"]).all() and torch.isnan(out["rel"]).all()
        assert not out["terms"].any() and not out["rel_terms"].any() and not out["dA"].any() and not out["dPb"].any()
    # four distinct columns on the host, a fifth written behind its back (left[1] is still 0 = right[0] until then): capacity four
    def fifth(row):
        row.rel[0].n_left, row.rel[0].left[1] = 2, 5
    out = broken(fifth, Q_max=4, rels=[([2], [0, 3, 6])])
    assert torch.isnan(out["rel"]).all() and not out["dA"].any()


def test_res32_plan_without_resident_columns():
    """res = 32 with a 16-slot table: the guided and relation columns do not fit LDS next to the tables (use_gcol = 0), every
    column value is re-read from global memory."""
    g = torch.Generator().manual_seed(11)
    A = torch.softmax(torch.randn(32, 32, 12, generator=g) * 2, -1)
    entries = [_box(3, (.1, .2, .6, .6), "cat"), _coor(8, (.7, .3), "ball")]
    rels = [([2, 5], [0, 7]), ([4], [2])]
    out = _evaluate(_table([(entries, 11, rels)], 32, T_max=8, Q_max=8), A[None])
    l64, g64 = _plugin_total(A, entries, 11, rels, torch.float64, "cpu")
    loss = (out["box"] + out["rel"]).double().cpu()[0]
    e_loss, e_grad = abs(loss - l64) / abs(l64), (out["dA"][0].double().cpu() - g64).abs().max() / g64.abs().max()
    print(f"\n[measured] res32: kernel loss {e_loss:.2e} grad {e_grad:.2e} rel {out['rel'][0].item():.6f}")
    assert out["rel"][0] > 0 and e_loss <= 1e-4 and e_grad <= 2e-3
