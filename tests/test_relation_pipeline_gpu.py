"""GuidedAttention.fused_relation_loss on the MI355X (fp32, the tiny UNet of the batched tests, 2 steps, thresholds that force
updates): a solo call with the switch on against the plugin path, a prompt whose tokens are all KEYWORDs, batched calls
(num_images_per_prompt, guidance_states) against solo plugin calls per image, graph reuse, and the launch census."""
import copy
import re

import pytest
import torch

from test_oracle_loop import G9, g9_setup
from test_pipeline_gpu import build_product

pytestmark = pytest.mark.gpu

BOXES = "a [robot:.6,.3,.4,.55] and a [blue vase:.2,.3,.4,.55] near a cat and a dog"
WITH_RELATION = BOXES + " [CustomLoss:toLeftOf (cat, dog)]"          # box terms (robot, blue vase) plus the relation
OTHER_LAYOUT = "a [robot:.1,.2,.5,.6] and a [blue vase:.5,.4,.4,.5] near a cat and a dog [CustomLoss:toLeftOf (dog, robot)]"
KEYWORDS_ONLY = "a [cat:.2,.5] and a [vase:.7,.5] [CustomLoss:toLeftOf (vase, cat)]"   # KEYWORD replaces COOR: T = 0
THR = {0: 0.0}   # no loss is <= 0: step 0 refines (up to its cap) and updates
_SETUP = {}


def _setup():
    if not _SETUP:
        meta = dict(G9[2], steps=2)
        unet, embeds, lat0, noise, _ = g9_setup(meta)
        g = torch.Generator().manual_seed(77)
        lat1 = torch.randn(lat0.shape, generator=g)
        emb1 = torch.cat([embeds[:1], torch.randn(1, 77, 48, generator=g)])
        _SETUP.update(meta=meta, unet=unet, inputs=[(embeds, lat0), (emb1, lat1)], noise=noise)
    return _SETUP


def _state(pipe, meta_prompt):
    from guided_attention_amd import run
    from guided_attention_amd.config import RunConfig
    from guided_attention_amd.pipeline_guided_attention import GuidanceState
    from guided_attention_amd.utils import shared_state as state
    cfg = RunConfig(meta_prompt=meta_prompt, output_path="/tmp/ga_test_out")
    cfg.stable = pipe
    state.config = cfg
    state.curHyperParams = dict(state.hyperParameterOverrides, thresholds=THR, recurse_steps=1)
    run.register_custom_loss("toLeftOf", run.ToLeftOf())
    run.overrideConfig(cfg)
    run.parseMetaPrompt(cfg)
    return GuidanceState(copy.copy(cfg), state.curHyperParams)


def _call(pipe, prompts, on, form="solo", graphs=False, which=(0,), embeds=None):
    """One pipeline call: form "solo" (prompts[0], inputs which[0]), "seeds" (prompts[0] for every image of `which`) or
    "states" (one prompt per image); `embeds`: the inputs whose text embeddings every image takes (default: its own).
    -> (output with .census, log lines: a list per image for the batched forms)."""
    from guided_attention_amd import ops
    from guided_attention_amd.utils import helpers, ptp_utils
    s = _setup()
    states = [_state(pipe, p) for p in prompts]
    if form != "states":
        _state(pipe, prompts[0])          # shared_state as a solo / seeds call reads it
    pipe.fused_relation_loss, pipe.use_graphs = on, graphs
    helpers.log_clear()
    ctrl = ptp_utils.AttentionStore(capture="loss-only")
    ptp_utils.register_attention_control(pipe, ctrl)
    ins = [(s["inputs"][k if embeds is None else embeds][0], s["inputs"][k][1]) for k in which]
    kw = dict(prompt=None, attention_store=ctrl, num_inference_steps=2, output_type="latent",
              prompt_embeds=torch.cat([e[1:2] for e, _ in ins]).cuda(), negative_prompt_embeds=torch.cat([e[0:1] for e, _ in ins]).cuda(),
              latents=torch.cat([lat for _, lat in ins]).clone(), thresholds=states[0].config.thresholds)
    ops.start_census()
    if form == "solo":
        out = pipe(renoise_noise=[n.clone() for n in s["noise"]], **kw)
    elif form == "seeds":
        kw["prompt_embeds"], kw["negative_prompt_embeds"] = kw["prompt_embeds"][:1], kw["negative_prompt_embeds"][:1]
        out = pipe(num_images_per_prompt=len(which), renoise_noise=[[n.clone() for n in s["noise"]] for _ in which], **kw)
    else:
        out = pipe(guidance_states=states, renoise_noise=[[n.clone() for n in s["noise"]] for _ in which], **kw)
    out.census = {}
    for key, n in ops.stop_census().items():
        out.census[key[0]] = out.census.get(key[0], 0) + n
    return out, (list(helpers.lines) if form == "solo" else out.logs)


def _mask_numbers(lines):
    return [re.sub(r"-?\d+(\.\d+)?(e-?\d+)?", "#", ln) for ln in lines]


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


def test_solo_call_with_the_switch_on_matches_the_plugin_path():
    pipe = build_product(_setup()["unet"], torch.float32)
    off, off_lines = _call(pipe, [WITH_RELATION], False)
    on, on_lines = _call(pipe, [WITH_RELATION], True)
    plain, _ = _call(pipe, [BOXES], False)
    assert off.unet_calls["bwd"] >= 1 and off.unet_calls == on.unet_calls
    assert _mask_numbers(on_lines) == _mask_numbers(off_lines) and len(on_lines) > 4
    err = _rel(on.latents, off.latents)
    print(f"\n[measured] solo on vs off: {err:.2e}; relation vs none {_rel(off.latents, plain.latents):.2e}")
    assert err < 5e-3
    assert _rel(off.latents, plain.latents) > 10 * err          # the relation is a visible part of the guidance
    # launches: the plugin path is aggregate + loss forward + loss backward, the switch makes it one launch each way
    assert off.census["smooth_loss_fwd"] == off.unet_calls["loss_evals"] and "aggregate_loss_rel_fwd_images" not in off.census
    assert on.census["aggregate_loss_rel_fwd_images"] == on.unet_calls["loss_evals"]
    assert on.census["smooth_loss_rel_bwd_images"] == on.unet_calls["bwd"]
    assert not {"smooth_loss_fwd", "smooth_loss_bwd", "aggregate_maps", "aggregate_loss_fwd"} & set(on.census)


def test_solo_call_under_graphs():
    from guided_attention_amd.graphs import GraphRunner
    pipe = build_product(_setup()["unet"], torch.float32)
    eager, eager_lines = _call(pipe, [WITH_RELATION], True)
    before = GraphRunner.captures
    graphs, graph_lines = _call(pipe, [WITH_RELATION], True, graphs=True)
    again, _ = _call(pipe, [WITH_RELATION], True, graphs=True, which=(1,))      # other inputs: replays what it has
    assert GraphRunner.captures == before + 1
    drop = lambda calls: {k: v for k, v in calls.items() if k != "joint_b3"}   # eager runs no joint pass
    assert drop(eager.unet_calls) == drop(graphs.unet_calls) and _mask_numbers(eager_lines) == _mask_numbers(graph_lines)
    assert _rel(graphs.latents, eager.latents) < 5e-3
    assert _rel(again.latents, _call(pipe, [WITH_RELATION], True, which=(1,))[0].latents) < 5e-3


def test_keyword_only_prompt_moves_the_latents():
    pipe = build_product(_setup()["unet"], torch.float32)
    on, _ = _call(pipe, [KEYWORDS_ONLY], True)
    off, _ = _call(pipe, [KEYWORDS_ONLY], False)
    plain, _ = _call(pipe, ["a cat and a vase"], False)
    assert on.unet_calls["bwd"] >= 1 and on.unet_calls == off.unet_calls and torch.isfinite(on.latents).all()
    assert "aggregate_loss_rel_fwd_images" in on.census and "smooth_loss_fwd" not in on.census
    assert (on.latents - plain.latents).abs().max() > 1e-4          # the relation alone moved the latents
    assert _rel(on.latents, off.latents) < 5e-3


@pytest.mark.parametrize("form", ["seeds", "states"])
def test_batched_calls_match_solo_plugin_calls(form):
    """Image s of a batched call with the switch on against its solo plugin call (switch off); then once under graphs, and a
    second graph call with another layout captures nothing."""
    from guided_attention_amd.graphs import GraphRunner
    pipe = build_product(_setup()["unet"], torch.float32)
    prompts = [WITH_RELATION, WITH_RELATION] if form == "seeds" else [WITH_RELATION, BOXES]
    shared = 0 if form == "seeds" else None          # the images of one prompt share its embeddings
    solo = [_call(pipe, [prompts[k]], False, which=(k,), embeds=shared) for k in (0, 1)]
    batched, logs = _call(pipe, prompts, True, form=form, which=(0, 1))
    for k in (0, 1):
        err = _rel(batched.latents[k:k + 1], solo[k][0].latents)
        print(f"\n[measured] {form} image {k} vs solo plugin: {err:.2e}")
        assert err < 5e-3, k
        assert batched.unet_calls_per_image[k] == solo[k][0].unet_calls, k
        assert _mask_numbers(logs[k]) == _mask_numbers(solo[k][1]), k
    assert "aggregate_loss_rel_fwd_images" in batched.census and "smooth_loss_rel_bwd_images" in batched.census
    before = GraphRunner.captures
    graphs, _ = _call(pipe, prompts, True, form=form, graphs=True, which=(0, 1))
    assert GraphRunner.captures == before + 1
    assert _rel(graphs.latents, batched.latents) < 5e-3
    other = [OTHER_LAYOUT, OTHER_LAYOUT] if form == "seeds" else [BOXES, OTHER_LAYOUT]
    second, _ = _call(pipe, other, True, form=form, graphs=True, which=(0, 1))
    assert GraphRunner.captures == before + 1                           # same table buffers, refilled rows
    eager_other, _ = _call(pipe, other, True, form=form, which=(0, 1))
    assert _rel(second.latents, eager_other.latents) < 5e-3
    assert _rel(second.latents, graphs.latents) > 1e-4


def test_one_guidance_evaluation_is_one_launch_each_way():
    """ops._count over ONE guidance evaluation and its backward with the switch on: one aggregate + loss launch, one loss
    backward launch, no separate loss forward."""
    from guided_attention_amd import ops
    from guided_attention_amd.utils import ptp_utils
    s = _setup()
    pipe = build_product(s["unet"], torch.float32)
    _state(pipe, WITH_RELATION)
    pipe.fused_relation_loss = True
    ctrl = ptp_utils.AttentionStore(capture="loss-only")
    ptp_utils.register_attention_control(pipe, ctrl)
    embeds, lat = s["inputs"][0]
    pipe._attention_store, pipe._truncate_at = ctrl, None
    ops.start_census()
    with torch.enable_grad():
        leaf, losses = pipe._guidance_eval(lat.cuda(), 981, embeds[1:2].cuda(), ctrl, 16, True, .5, 3, False)
        loss, _, unscaled = pipe._compute_loss(losses)
        pipe._update_latent(leaf, loss, 1.0)
    census = {}
    for key, n in ops.stop_census().items():
        census[key[0]] = census.get(key[0], 0) + n
    assert [n for k, n in census.items() if "aggregate_loss" in k] == [1]
    assert [n for k, n in census.items() if k.startswith("smooth_loss") and "bwd" in k] == [1]
    assert "smooth_loss_fwd" not in census and "aggregate_maps" not in census
    fused = losses["_fused"]
    assert fused["relation_fused"] and fused["host_custom"].item() > 0 and unscaled[-1][0] is None
    assert fused["host_total"].item() == (fused["host_loss"] + fused["host_custom"]).item() == pytest.approx(loss.item(), rel=1e-6)
