"""GuidedAttention.fused_relation_loss with the toRightOf, above and below relations on the MI355X (fp32, the tiny UNet and the
2 steps of test_relation_pipeline_gpu): a solo call with the switch on against the plugin path, graph reuse across kinds, and
batched calls (guidance_states, num_images_per_prompt) against solo plugin calls per image."""
import copy

import pytest
import torch

from test_pipeline_gpu import build_product
from test_relation_pipeline_gpu import BOXES, THR, _mask_numbers, _rel, _setup

pytestmark = pytest.mark.gpu

ABOVE = BOXES + " [CustomLoss:above (cat, dog)]"
BELOW = BOXES + " [CustomLoss:below (cat, dog)]"
RIGHT_OF = BOXES + " [CustomLoss:toRightOf (cat, dog)]"


def _state(pipe, meta_prompt):
    from guided_attention_amd import run
    from guided_attention_amd.config import RunConfig
    from guided_attention_amd.pipeline_guided_attention import GuidanceState
    from guided_attention_amd.utils import shared_state as state
    cfg = RunConfig(meta_prompt=meta_prompt, output_path="/tmp/ga_test_out")
    cfg.stable = pipe
    state.config = cfg
    state.curHyperParams = dict(state.hyperParameterOverrides, thresholds=THR, recurse_steps=1)
    run.register_builtin_losses()
    run.overrideConfig(cfg)
    run.parseMetaPrompt(cfg)
    return GuidanceState(copy.copy(cfg), state.curHyperParams)


def _call(pipe, prompts, on, form="solo", graphs=False, which=(0,), embeds=None):
    """One pipeline call, as test_relation_pipeline_gpu._call makes it, with every built-in relation registered: form "solo"
    (prompts[0], inputs which[0]), "seeds" (prompts[0] for every image of `which`) or "states" (one prompt per image).
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
    try:
        if form == "solo":
            out = pipe(renoise_noise=[n.clone() for n in s["noise"]], **kw)
        elif form == "seeds":
            kw["prompt_embeds"], kw["negative_prompt_embeds"] = kw["prompt_embeds"][:1], kw["negative_prompt_embeds"][:1]
            out = pipe(num_images_per_prompt=len(which), renoise_noise=[[n.clone() for n in s["noise"]] for _ in which], **kw)
        else:
            out = pipe(guidance_states=states, renoise_noise=[[n.clone() for n in s["noise"]] for _ in which], **kw)
    finally:
        census = ops.stop_census()
    out.census = {}
    for key, n in census.items():
        out.census[key[0]] = out.census.get(key[0], 0) + n
    return out, (list(helpers.lines) if form == "solo" else out.logs)


def test_solo_call_with_the_switch_on_matches_the_plugin_path():
    pipe = build_product(_setup()["unet"], torch.float32)
    off, off_lines = _call(pipe, [ABOVE], False)
    on, on_lines = _call(pipe, [ABOVE], True)
    plain, _ = _call(pipe, [BOXES], False)
    below, _ = _call(pipe, [BELOW], True)
    assert off.unet_calls["bwd"] >= 1 and off.unet_calls == on.unet_calls
    assert _mask_numbers(on_lines) == _mask_numbers(off_lines) and len(on_lines) > 4
    err = _rel(on.latents, off.latents)
    print(f"\n[measured] above, solo on vs off: {err:.2e}; relation vs none {_rel(off.latents, plain.latents):.2e}; "
          f"above vs below {(on.latents - below.latents).abs().max().item():.2e}")
    assert err < 5e-3
    assert _rel(off.latents, plain.latents) > 10 * err          # the relation is a visible part of the guidance
    assert (on.latents - below.latents).abs().max() > 1e-4      # and its direction is
    assert "aggregate_loss_rel_fwd_images" not in off.census
    assert on.census["aggregate_loss_rel_fwd_images"] == on.unet_calls["loss_evals"]
    assert on.census["smooth_loss_rel_bwd_images"] == on.unet_calls["bwd"]
    assert "smooth_loss_fwd" not in on.census and "smooth_loss_fwd" not in below.census
    assert "aggregate_loss_rel_fwd_images" in below.census and "smooth_loss_rel_bwd_images" in below.census


def test_solo_call_under_graphs_reuses_the_capture_for_another_kind():
    from guided_attention_amd.graphs import GraphRunner
    pipe = build_product(_setup()["unet"], torch.float32)
    eager, eager_lines = _call(pipe, [ABOVE], True)
    before = GraphRunner.captures
    graphs, graph_lines = _call(pipe, [ABOVE], True, graphs=True)
    assert GraphRunner.captures == before + 1
    drop = lambda calls: {k: v for k, v in calls.items() if k != "joint_b3"}   # eager runs no joint pass
    assert drop(eager.unet_calls) == drop(graphs.unet_calls) and _mask_numbers(eager_lines) == _mask_numbers(graph_lines)
    assert _rel(graphs.latents, eager.latents) < 5e-3
    second, _ = _call(pipe, [RIGHT_OF], True, graphs=True)
    assert GraphRunner.captures == before + 1                   # same buffers, refilled rows: nothing is captured again
    eager_second, _ = _call(pipe, [RIGHT_OF], True)
    assert _rel(second.latents, eager_second.latents) < 5e-3
    assert (second.latents - graphs.latents).abs().max() > 1e-4     # and the replay served the other kind


@pytest.mark.parametrize("form", ["seeds", "states"])
def test_batched_calls_match_solo_plugin_calls(form):
    """Image s of a batched call with the switch on against its solo plugin call (switch off): guidance_states with two prompts
    of different kinds, num_images_per_prompt = 2 with `below`.  With the switch off the same call is refused as before."""
    pipe = build_product(_setup()["unet"], torch.float32)
    prompts = [BELOW, BELOW] if form == "seeds" else [ABOVE, RIGHT_OF]
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
    with pytest.raises(NotImplementedError, match="custom-loss plugins"):
        _call(pipe, prompts, False, form=form, which=(0, 1))
