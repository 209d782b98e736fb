"""The toLeftOf relation loss in the loss launches, without a GPU: the two entry points in the header and the binding, the struct
layouts, their host-side argument checks, the host validation of relation rows, the pipeline switch in front of the batched
calls' refusals, and the CLI flag."""
import ctypes
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "ga_hip.h"
NEW = ["ga_aggregate_loss_rel_fwd_images", "ga_smooth_loss_rel_bwd_images"]


@pytest.fixture(scope="module")
def lib():
    from guided_attention_amd import _lib
    if not _lib.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_header_and_binding_carry_the_entries(lib):
    from guided_attention_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in NEW:
        assert re.search(rf"\bint {name}\s*\(", text), name
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert int(re.search(r"#define GA_VERSION (\d+)", text).group(1)) == _lib.GA_VERSION == lib.ga_version() == 183
    # the argument counts of the prototypes against the header's
    for name in NEW:
        args = re.search(rf"\bint {name}\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert len(args.split(",")) == len(_lib.PROTOTYPES[name]), name


def test_relation_struct_layouts_match_header(tmp_path):
    from guided_attention_amd import _lib
    fields = {"ga_relation_t": ["kind", "n_left", "n_right", "left", "right"], "ga_image_relations_t": ["R", "rel"]}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "ga_hip.h"', "int main(void) {",
           '  printf("tokens %d\\n", GA_REL_MAX_TOKENS);', '  printf("relations %d\\n", GA_IMAGE_MAX_RELATIONS);',
           '  printf("left_of %d\\n", (int)GA_REL_LEFT_OF);',
           '  printf("old %zu\\n", sizeof(ga_image_loss_t) + sizeof(ga_token_t) + sizeof(ga_loss_params_t));']
    for st, fs in fields.items():
        src.append(f'  printf("{st} %zu\\n", sizeof({st}));')
        src += [f'  printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f in fs]
    src += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-I", str(HEADER.parent), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = dict(line.split() for line in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True,
                                                       check=True).stdout.splitlines())
    assert int(out["tokens"]) == _lib.GA_REL_MAX_TOKENS == 8 and int(out["relations"]) == _lib.GA_IMAGE_MAX_RELATIONS == 4
    assert int(out["left_of"]) == _lib.GA_REL_LEFT_OF
    assert int(out["old"]) == 1576 + 48 + 40                      # no existing struct moved
    for st, fs in fields.items():
        cls = getattr(_lib, st)
        assert int(out[st]) == ctypes.sizeof(cls), st
        for f in fs:
            assert int(out[f"{st}.{f}"]) == getattr(cls, f).offset, (st, f)


def test_entries_validate_on_the_host(lib):
    """Fake (never dereferenced) device pointers: every call below fails in the host checks, before any launch."""
    from guided_attention_amd import _lib
    p = ctypes.c_void_p(0x1000)
    hp = _lib.ga_loss_params_t(sigma=.5, ksize=3, smooth=1)
    maps = (ctypes.c_void_p * 1)(0x1000)
    heads = (ctypes.c_int * 1)(8)

    def fwd(images=2, res=16, table=p, T_max=4, rel=p, Q_max=4, A=p, terms=p, loss=p, rel_terms=p, rel_loss=p, tickets=p):
        return lib.ga_aggregate_loss_rel_fwd_images(maps, heads, 1, images, res, 77, table, T_max, rel, Q_max, ctypes.byref(hp),
                                                    A, terms, loss, rel_terms, rel_loss, tickets, _lib.GA_F32, None)

    def bwd(images=2, res=16, table=p, T_max=4, rel=p, Q_max=4, A=p, dloss=p, dA=p):
        return lib.ga_smooth_loss_rel_bwd_images(A, images, res, 77, table, T_max, rel, Q_max, ctypes.byref(hp), dloss, dA, None,
                                                 1.0, _lib.GA_F32, None)

    for call in (fwd, bwd):
        assert call(table=None) == -1 and call(rel=None) == -1 and call(A=None) == -1
        assert call(images=0) == -2 and call(images=65) == -2 and call(T_max=33) == -2
        assert call(Q_max=33) == -2 and call(Q_max=-1) == -2
        assert call(res=32, T_max=16, Q_max=16) == -2         # (16 + 16) * 32^2 > 24576
        assert call(res=64, T_max=4, Q_max=4) == -2           # 8 * 64^2 > 24576
    assert fwd(terms=None) == -1 and fwd(loss=None) == -1 and fwd(tickets=None) == -1
    assert fwd(rel_terms=None) == -1 and fwd(rel_loss=None) == -1
    assert bwd(dloss=None) == -1 and bwd(dA=None) == -1


def test_relation_rows_are_checked_on_the_host():
    from guided_attention_amd import ops
    from guided_attention_amd._lib import GaError
    assert [ops.relation_capacity(q) for q in (0, 1, 4, 5, 9, 17, 32)] == [0, 4, 4, 8, 16, 32, 32]
    with pytest.raises(GaError):
        ops.relation_capacity(33)
    rp = ops.RelationPlan([([1], [4]), ([0, 1], [4, 7, 9])])
    assert rp.R == 2 and rp.columns == [0, 1, 4, 7, 9]
    assert rp.row.rel[1].n_right == 3 and list(rp.row.rel[1].right)[:3] == [4, 7, 9] and rp.row.rel[0].left[0] == 1
    assert ops.RelationPlan([]).R == 0
    with pytest.raises(GaError, match="9 left tokens"):
        ops.RelationPlan([(list(range(9)), [1])])
    with pytest.raises(GaError, match="0 right tokens"):
        ops.RelationPlan([([1], [])])
    with pytest.raises(GaError, match="5 relations"):
        ops.RelationPlan([([0], [1])] * 5)
    with pytest.raises(GaError, match="not a slice index"):
        ops.RelationPlan([([-1], [1])])
    with pytest.raises(GaError, match="index 9 lies outside the text slice of 8"):
        ops.RelationPlan([([1], [9])], width=8)
    # ImageTable.set, host half only (no device buffer is touched before the rows pass)
    hp = {"inside_loss_scale": .2, "outside_loss_scale": .2, "shrink_factor": 0.0}
    plan = ops.LossPlan([{"index": 2, "kind": "COOR", "geom": (.5, .5), "subprompt": "a"}], hp)
    table = object.__new__(ops.ImageTable)
    table.images, table.T_max, table.res, table.Q_max = 2, 4, 16, 4
    with pytest.raises(GaError, match="image 1: index 75 lies outside the text slice of 75"):
        ops.ImageTable.set(table, [plan, plan], [(1, 76), (1, 76)], [None, ops.RelationPlan([([1], [75])])])
    with pytest.raises(GaError, match="image 0: 5 distinct relation columns, the table holds 4"):
        ops.ImageTable.set(table, [plan, plan], [(1, 76), (1, 76)], [rp, None])
    table.Q_max = 0
    with pytest.raises(GaError, match="without relation rows"):
        ops.ImageTable.set(table, [plan, plan], [(1, 76), (1, 76)], [None, None])
    with pytest.raises(GaError, match="Q_max"):
        ops.ImageTable(1, 16, 32, True, .5, 3, torch.device("cpu"), Q_max=16)


# ------------------------------------------------------------------------------------------------ the pipeline switch
def _cpu_pipe():
    from guided_attention_amd.pipeline_guided_attention import GuidedAttention
    from guided_attention_amd.text import SyntheticTextEncoder, WordTokenizer
    from guided_attention_amd.unet import UNetConfig
    unet = SimpleNamespace(config=UNetConfig.tiny(sample_size=32, cross_attention_dim=48), device=torch.device("cpu"),
                           dtype=torch.float32)
    return GuidedAttention(unet, None, None, SyntheticTextEncoder(48), WordTokenizer())


def _config(pipe, plugin, args="(cat, vase)", prompt="a cat and a vase"):
    return SimpleNamespace(prompt=prompt, stable=pipe, custom_loss={"toLeftOf": (plugin, args)} if plugin is not None else None,
                           diagnostic_level=0, token_dict={}, thresholds={0: .05}, only_update_on_threshold_steps=True,
                           sub_prompt_avg_within=False)


@pytest.fixture
def shared():
    from guided_attention_amd.utils import shared_state as state
    saved = state.curHyperParams, getattr(state, "config", None)
    state.curHyperParams = dict(state.hyperParameterOverrides)
    yield state
    state.curHyperParams, state.config = saved


def _seeds_call(pipe):
    return pipe(prompt="a cat and a vase", attention_store=None, num_images_per_prompt=2,
                generator=[torch.Generator().manual_seed(s) for s in range(2)])


def _states_call(pipe, cfgs, state):
    from guided_attention_amd.pipeline_guided_attention import GuidanceState
    states = [GuidanceState(c, dict(state.hyperParameterOverrides)) for c in cfgs]
    return pipe(prompt=[c.prompt for c in cfgs], attention_store=None, guidance_states=states, num_images_per_prompt=1,
                generator=[torch.Generator().manual_seed(s) for s in range(len(cfgs))])


def _plugins():
    from guided_attention_amd import run

    class Sub(run.ToLeftOf):
        pass
    return {"toLeftOf": run.ToLeftOf(), "object": object(), "subclass": Sub()}


def test_the_switch_is_off_by_default():
    from guided_attention_amd.config import RunConfig
    from guided_attention_amd.pipeline_guided_attention import GuidedAttention
    assert GuidedAttention(SimpleNamespace(), None, None, None, None).fused_relation_loss is False
    assert RunConfig(meta_prompt="a").fused_relation_loss is False


@pytest.mark.parametrize("which", ["toLeftOf", "object", "subclass"])
def test_batched_calls_accept_the_relation_plugin_only_with_the_switch_on(shared, which):
    """Accepted = the call gets as far as the device check (this machine's pipeline sits on the CPU)."""
    from guided_attention_amd._lib import GaError
    plugin = _plugins()[which]
    for on in (True, False):
        pipe = _cpu_pipe()
        pipe.fused_relation_loss = on
        shared.config = _config(pipe, plugin)
        cfgs = [_config(pipe, None, prompt="a robot"), _config(pipe, plugin)]
        if on and which == "toLeftOf":
            with pytest.raises(GaError, match="GPU only"):
                _seeds_call(pipe)
            with pytest.raises(GaError, match="GPU only"):
                _states_call(pipe, cfgs, shared)
        else:   # today's refusals, word for word
            with pytest.raises(NotImplementedError, match=r"custom-loss plugins with num_images_per_prompt > 1 is not supported"):
                _seeds_call(pipe)
            with pytest.raises(NotImplementedError,
                               match=r"prompt 1: custom-loss plugins is not supported in a call with guidance_states"):
                _states_call(pipe, cfgs, shared)


def test_a_sub_prompt_that_does_not_resolve_is_named_before_any_launch(shared):
    from guided_attention_amd import run
    pipe = _cpu_pipe()
    pipe.fused_relation_loss = True
    shared.config = _config(pipe, run.ToLeftOf(), args="(cat, sofa)")
    with pytest.raises(ValueError, match="sofa"):
        _seeds_call(pipe)
    with pytest.raises(ValueError, match="sofa"):
        _states_call(pipe, [_config(pipe, None, prompt="a robot"), shared.config], shared)
    shared.config = _config(pipe, run.ToLeftOf(), args="(a cat, vase)")
    plan = pipe._relation_plan()                       # slice indices: 0-based behind BOS, as the plugin reads its maps
    assert plan.relations == [([0, 1], [4])]
    pipe.fused_relation_loss = False
    assert pipe._relation_plan() is None


def test_fused_relation_loss_is_a_cli_flag():
    from guided_attention_amd import run
    base = ["--meta_prompt", "a [cat] and a [vase] [CustomLoss:toLeftOf (cat, vase)]", "--output_path", "/tmp/ga_test_out"]
    cfg = run._parse_cli(base + ["--fused_relation_loss", "true", "--seeds_per_pass", "4"])
    assert cfg.fused_relation_loss is True and cfg.seeds_per_pass == 4
    assert run._parse_cli(base).fused_relation_loss is False
