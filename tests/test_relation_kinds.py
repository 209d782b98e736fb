"""The toRightOf, above and below relations next to toLeftOf, without a GPU: the enum in the header against the binding, the
four plugins against each other and against the reference's recorded numbers, hand-checkable maps, and the host path that
parses a prompt and lowers its plugins into relation rows."""
import ctypes
import subprocess
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

from conftest import load_npz

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "ga_hip.h"
NAMES = ["toLeftOf", "toRightOf", "above", "below"]


def _plugin(name, a, b):
    """The registered plugin class of `name` with its sub-prompt lookup answered: "A" -> a's slice indices, "B" -> b's."""
    from guided_attention_amd import run
    fn = run.BUILTIN_LOSSES[name]()
    fn.find_indices_for_sub_prompt = {"A": list(a), "B": list(b)}.get
    return fn


def _loss_and_grad(name, maps, a, b):
    maps = maps.clone().requires_grad_(True)
    loss = _plugin(name, a, b).calc_loss(maps, "(A, B)")
    (g,) = torch.autograd.grad(loss.sum(), [maps])
    return loss.detach(), g


def _maps(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.softmax(torch.randn(*shape, generator=g, dtype=torch.float64) * 2, -1)


# ------------------------------------------------------------------------------------------------ 1: header against binding
def test_enum_values_and_struct_sizes_match_the_header(tmp_path):
    from guided_attention_amd import _lib
    src = ['#include <stdio.h>', '#include "ga_hip.h"', "int main(void) {",
           '  printf("left_of %d\\n", (int)GA_REL_LEFT_OF);', '  printf("right_of %d\\n", (int)GA_REL_RIGHT_OF);',
           '  printf("above %d\\n", (int)GA_REL_ABOVE);', '  printf("below %d\\n", (int)GA_REL_BELOW);',
           '  printf("relation %zu\\n", sizeof(ga_relation_t));', '  printf("row %zu\\n", sizeof(ga_image_relations_t));',
           "  return 0;", "}"]
    (tmp_path / "kinds.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-I", str(HEADER.parent), str(tmp_path / "kinds.c"), "-o", str(tmp_path / "kinds")], check=True)
    out = {k: int(v) for k, v in (line.split() for line in subprocess.run([str(tmp_path / "kinds")], capture_output=True,
                                                                          text=True, check=True).stdout.splitlines())}
    assert (out["left_of"], out["right_of"], out["above"], out["below"]) == (0, 1, 2, 3)
    assert (_lib.GA_REL_LEFT_OF, _lib.GA_REL_RIGHT_OF, _lib.GA_REL_ABOVE, _lib.GA_REL_BELOW) == (0, 1, 2, 3)
    assert out["relation"] == ctypes.sizeof(_lib.ga_relation_t) == 80
    assert out["row"] == ctypes.sizeof(_lib.ga_image_relations_t) == 336


# ------------------------------------------------------------------------------------------------ 2: the plugins against each other
SIDES = [([1], [4]), ([2, 5], [0, 3, 6]), ([0, 3, 6], [2, 5])]      # one token each; 2 against 3 and 3 against 2: the divisor quirk


@pytest.mark.parametrize("shape,seed", [((8, 8, 12), 5), ((24, 24, 9), 6)])
@pytest.mark.parametrize("a,b", SIDES)
def test_plugins_agree_under_swapped_roles_and_transposed_maps(shape, seed, a, b):
    maps = _maps(shape, seed)
    for mirror, name in (("toRightOf", "toLeftOf"), ("below", "above")):
        l0, g0 = _loss_and_grad(mirror, maps, a, b)
        l1, g1 = _loss_and_grad(name, maps, b, a)
        assert torch.equal(l0, l1) and torch.equal(g0, g1), mirror
    la, ga = _loss_and_grad("above", maps, a, b)
    lt, gt = _loss_and_grad("toLeftOf", maps.transpose(0, 1).contiguous(), a, b)
    # random maps: every centroid sits mid-map, so v = (|a| + .4 |a| - |b|) * 4.5 / |a| — open unless b has more tokens than a
    assert (la.item() > 0) == (len(a) >= len(b))
    assert abs(la.item() - lt.item()) <= 1e-12 and (ga - gt.transpose(0, 1)).abs().max() <= 1e-12
    # the quirk itself: with |a| != |b| the roles are not interchangeable by a sign
    if len(a) != len(b):
        assert _loss_and_grad("toRightOf", maps, a, b)[0] != _loss_and_grad("toLeftOf", maps, a, b)[0]


def test_to_left_of_is_its_own_class_and_the_four_share_one_calc_loss():
    from guided_attention_amd import run
    assert type(run.ToLeftOf()) is run.ToLeftOf
    classes = [run.BUILTIN_LOSSES[n] for n in NAMES]
    assert classes == [run.ToLeftOf, run.ToRightOf, run.Above, run.Below] and len(set(classes)) == 4
    for cls in classes[1:]:
        assert type(cls()) is not run.ToLeftOf and not isinstance(cls(), run.ToLeftOf)
    assert len({cls.calc_loss for cls in classes}) == 1


# ------------------------------------------------------------------------------------------------ 3: the reference's numbers
@pytest.mark.parametrize("name", ["bos", "sharp"])
def test_above_on_the_transposed_fixture_map_gives_the_reference_numbers(name):
    """g10 holds the reference's ToLeftOf loss and autograd gradient for (cat, vase) = slice indices 1 and 4 on a 16 x 16 x 77
    map; `above` on the spatially transposed map is the same number, its gradient the transposed one (the tolerances of
    test_relation_loss_gpu.test_fixture_numbers_of_the_reference)."""
    import numpy as np
    g = load_npz("g10_custom_loss.npz")
    A = torch.from_numpy(g[f"{name}.A"]).double().transpose(0, 1).contiguous().requires_grad_(True)
    loss = _plugin("above", [1], [4]).calc_loss(torch.softmax(A[:, :, 1:76] * 100, dim=-1), "(A, B)")
    (dA,) = torch.autograd.grad(loss.sum(), [A])
    np.testing.assert_allclose(loss.detach().numpy().reshape(-1), np.asarray(g[f"{name}.loss"]).reshape(-1), rtol=2e-5, atol=1e-6)
    ref = g[f"{name}.dA"].reshape(16, 16, 77)
    assert np.abs(dA.transpose(0, 1).numpy() - ref).max() <= 2e-3 * np.abs(ref).max()
    assert loss.item() > 0


# ------------------------------------------------------------------------------------------------ 4: hand-checkable maps
def _point_maps(res, points):
    """(res, res, len(points)) float64: token k's whole mass on pixel points[k] = (row, col)."""
    maps = torch.zeros(res, res, len(points), dtype=torch.float64)
    for k, (i, j) in enumerate(points):
        maps[i, j, k] = 1.0
    return maps


# token 0 at (row 2, col 5), token 1 at (row 6, col 3) on a 10 x 10 map: centroids 2.5 / 5.5 / 6.5 / 3.5, gap 2
#   toLeftOf (0, 1):  (5.5 + 2 - 3.5) / 10 * 9 = 3.6      toRightOf (0, 1): (3.5 + 2 - 5.5) / 10 * 9 = 0
#   above (0, 1):     (2.5 + 2 - 6.5) / 10 * 9 < 0 -> 0   below (0, 1):     (6.5 + 2 - 2.5) / 10 * 9 = 5.4
@pytest.mark.parametrize("name,expected", [("toLeftOf", 3.6), ("toRightOf", 0.0), ("above", 0.0), ("below", 5.4)])
def test_point_masses_give_exact_values(name, expected):
    maps = _point_maps(10, [(2, 5), (6, 3)])
    loss, grad = _loss_and_grad(name, maps, [0], [1])
    assert loss.item() == pytest.approx(expected, abs=1e-12)
    if name == "above":                                     # v = -1.8: the hinge is closed, value and gradient are exactly 0
        assert loss.item() == 0.0 and not grad.any()


@pytest.mark.parametrize("name,points", [("toLeftOf", [(4, 0), (4, 9)]), ("toRightOf", [(4, 9), (4, 0)]),
                                         ("above", [(0, 4), (9, 4)]), ("below", [(9, 4), (0, 4)])])
def test_closed_hinges_are_exactly_zero(name, points):
    """a where the relation wants it, b at the opposite edge: v = (0.5 + 2 - 9.5) / 10 * 9 < 0 for every kind."""
    loss, grad = _loss_and_grad(name, _point_maps(10, points), [0], [1])
    assert loss.item() == 0.0 and not grad.any()
    # and with the arguments exchanged the hinge is wide open: (9.5 + 2 - 0.5) / 10 * 9
    assert _loss_and_grad(name, _point_maps(10, points), [1], [0])[0].item() == pytest.approx(9.9, abs=1e-12)


def test_two_tokens_on_one_side_divide_both_sums_by_the_left_role_count():
    """a = tokens 0, 1 (cols 1 and 3), b = token 2 (col 8), toRightOf: the "left" role is b with ONE token, so a's centroid sum
    is (1.5 + 3.5) / 1, not their mean: v = (8.5 + 2 - 5) / 10 * 9."""
    maps = _point_maps(10, [(0, 1), (0, 3), (0, 8)])
    assert _loss_and_grad("toRightOf", maps, [0, 1], [2])[0].item() == pytest.approx(5.5 * .9, abs=1e-12)
    # toLeftOf on the same arguments: the "left" role is a with TWO tokens, and b's 8.5 is halved too — (2.5 + 2 - 4.25) / 10 * 9
    assert _loss_and_grad("toLeftOf", maps, [0, 1], [2])[0].item() == pytest.approx(.25 * .9, abs=1e-12)
    assert _loss_and_grad("below", maps.transpose(0, 1).contiguous(), [0, 1], [2])[0].item() == pytest.approx(5.5 * .9, abs=1e-12)


# ------------------------------------------------------------------------------------------------ 5: parsing and lowering
def _cpu_pipe():
    from guided_attention_amd.pipeline_guided_attention import GuidedAttention
    from guided_attention_amd.text import SyntheticTextEncoder, WordTokenizer
    from guided_attention_amd.unet import UNetConfig
    unet = SimpleNamespace(config=UNetConfig.tiny(sample_size=32, cross_attention_dim=48), device=torch.device("cpu"),
                           dtype=torch.float32)
    return GuidedAttention(unet, None, None, SyntheticTextEncoder(48), WordTokenizer())


def _config(pipe, custom, prompt="a cat and a dog near a vase"):
    return SimpleNamespace(prompt=prompt, stable=pipe, custom_loss=custom, diagnostic_level=0, token_dict={}, thresholds={0: .05},
                           only_update_on_threshold_steps=True, sub_prompt_avg_within=False)


@pytest.fixture
def shared():
    from guided_attention_amd.utils import shared_state as state
    saved = state.curHyperParams, getattr(state, "config", None)
    state.curHyperParams = dict(state.hyperParameterOverrides)
    yield state
    state.curHyperParams, state.config = saved


def test_parse_prompt_resolves_the_registered_relations(shared):
    from guided_attention_amd import run
    from guided_attention_amd.utils import helpers
    shared.config = SimpleNamespace()
    run.register_builtin_losses()
    assert list(shared.config.registered_loss_functions) == NAMES
    assert [type(f) for f in shared.config.registered_loss_functions.values()] == [run.ToLeftOf, run.ToRightOf, run.Above, run.Below]
    prompt, meta_info, custom = helpers.parse_prompt("a cat and a dog [CustomLoss:above (cat, dog)]")
    assert prompt.strip() == "a cat and a dog" and list(custom) == ["above"]
    fn, args = custom["above"]
    assert type(fn) is run.Above and args == "(cat, dog)"
    assert [m[0] for m in meta_info] == ["cat", "dog"]
    for name in NAMES:
        _, _, custom = helpers.parse_prompt(f"a cat and a dog [CustomLoss:{name} (dog, cat)]")
        assert [(n, type(f), a) for n, (f, a) in custom.items()] == [(name, run.BUILTIN_LOSSES[name], "(dog, cat)")]


def test_only_the_four_classes_themselves_are_eligible(shared):
    from guided_attention_amd import run

    class Sub(run.Above):
        pass
    pipe = _cpu_pipe()
    pipe.fused_relation_loss = True
    for name in NAMES:
        assert pipe._relations_eligible({name: (run.BUILTIN_LOSSES[name](), "(cat, dog)")}), name
    assert pipe._relations_eligible({n: (run.BUILTIN_LOSSES[n](), "(cat, dog)") for n in NAMES})
    for foreign in (Sub(), object(), run.DirectionalRelation()):
        assert not pipe._relations_eligible({"above": (foreign, "(cat, dog)")})
        assert not pipe._relations_eligible({"above": (run.Above(), "(cat, dog)"), "other": (foreign, "(cat, dog)")})
    pipe.fused_relation_loss = False
    assert not pipe._relations_eligible({"above": (run.Above(), "(cat, dog)")})


def test_relation_plan_lowers_each_plugin_to_its_kind(shared):
    from guided_attention_amd import _lib, run
    pipe = _cpu_pipe()
    pipe.fused_relation_loss = True
    custom = {"above": (run.Above(), "(a cat, vase)"), "toRightOf": (run.ToRightOf(), "(dog, cat)"),
              "below": (run.Below(), "(vase, dog)"), "toLeftOf": (run.ToLeftOf(), "(cat, dog)")}
    shared.config = _config(pipe, custom)          # slice indices behind BOS: a 0, cat 1, and 2, a 3, dog 4, near 5, a 6, vase 7
    plan = pipe._relation_plan()
    kinds = [_lib.GA_REL_ABOVE, _lib.GA_REL_RIGHT_OF, _lib.GA_REL_BELOW, _lib.GA_REL_LEFT_OF]
    assert plan.relations == [([0, 1], [7]), ([4], [1]), ([7], [4]), ([1], [4])]     # a's indices, b's indices: the prompt's order
    assert plan.kinds == kinds and plan.R == 4 and plan.columns == [0, 1, 4, 7]
    for r, kind in enumerate(kinds):
        rel = plan.row.rel[r]
        assert rel.kind == kind
        assert list(rel.left)[:rel.n_left] == plan.relations[r][0] and list(rel.right)[:rel.n_right] == plan.relations[r][1]


def test_relation_plan_items_carry_an_optional_kind():
    from guided_attention_amd import _lib, ops
    from guided_attention_amd._lib import GaError
    rp = ops.RelationPlan([([1], [4]), ([0, 1], [4, 7], _lib.GA_REL_BELOW)])
    assert rp.relations == [([1], [4]), ([0, 1], [4, 7])] and rp.kinds == [_lib.GA_REL_LEFT_OF, _lib.GA_REL_BELOW]
    assert rp.row.rel[0].kind == 0 and rp.row.rel[1].kind == 3
    assert ops.RelationPlan([]).kinds == []
    for bad in (4, -1, 99, None, "above", 2.0, True):
        with pytest.raises(GaError, match="unknown kind"):
            ops.RelationPlan([([1], [4], bad)])
    with pytest.raises(GaError, match="expected"):
        ops.RelationPlan([([1], [4], 0, 0)])


@pytest.mark.parametrize("name", ["toRightOf", "above", "below"])
def test_a_sub_prompt_outside_the_prompt_is_refused_with_the_relations_name(shared, name):
    from guided_attention_amd import run
    pipe = _cpu_pipe()
    pipe.fused_relation_loss = True
    shared.config = _config(pipe, {name: (run.BUILTIN_LOSSES[name](), "(cat, sofa)")})
    with pytest.raises(ValueError, match=rf"^{name} \(cat, sofa\): sub-prompt 'sofa' is not part of the prompt"):
        pipe._relation_plan()
    shared.config = _config(pipe, {name: (run.BUILTIN_LOSSES[name](), "(cat, dog, vase)")})
    with pytest.raises(ValueError, match=rf"^{name} takes two sub-prompts"):
        pipe._relation_plan()
    with pytest.raises(ValueError, match=rf"^{name} takes two sub-prompts"):     # a batched call checks before any launch
        pipe(prompt="a cat and a dog near a vase", attention_store=None, num_images_per_prompt=2,
             generator=[torch.Generator().manual_seed(s) for s in range(2)])
