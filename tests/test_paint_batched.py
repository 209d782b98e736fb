"""Paint-with-words in batched calls without a GPU: with GuidedAttention.batched_paint_with_words on, such a call is accepted
up to the device check while every other refusal stays; the per-image mask / multiplier builder on the CPU; the four grouped
entry points in the header, the binding and their host-side argument checks; the CLI flag."""
import ctypes
import math
import re
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

from oracle import attention as oattn

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "ga_hip.h"
NEW = ["ga_attn_scores_max_grouped", "ga_attn_capture_fwd_biased_grouped", "ga_attn_capture_bwd_biased_grouped",
       "ga_attn_pww_max_grad"]


def _cpu_pipe(sdxl=False):
    from guided_attention_amd.pipeline_guided_attention import GuidedAttention
    from guided_attention_amd.text import SyntheticTextEncoder, WordTokenizer
    from guided_attention_amd.unet import UNetConfig
    cfg = UNetConfig.tiny(sample_size=32, cross_attention_dim=48)
    if sdxl:
        cfg.addition_embed_type = "text_time"
    unet = SimpleNamespace(config=cfg, device=torch.device("cpu"), dtype=torch.float32)
    pipe = GuidedAttention(unet, None, None, SyntheticTextEncoder(48), WordTokenizer())
    pipe.batched_paint_with_words = True
    return pipe


def _state(prompt="a robot", **hp):
    from guided_attention_amd.pipeline_guided_attention import GuidanceState
    from guided_attention_amd.utils import shared_state as state
    cfg = SimpleNamespace(prompt=prompt, custom_loss=None, diagnostic_level=0, token_dict={}, thresholds={0: .05},
                          only_update_on_threshold_steps=True, sub_prompt_avg_within=False)
    return GuidanceState(cfg, dict(state.hyperParameterOverrides, **hp))


def _seeds_call(pipe, **kw):
    args = dict(prompt="a robot", attention_store=None, num_images_per_prompt=3,
                generator=[torch.Generator().manual_seed(s) for s in range(3)])
    args.update(kw)
    return pipe(**args)


def _states_call(pipe, states, **kw):
    args = dict(prompt=[st.config.prompt for st in states], attention_store=None, guidance_states=states,
                num_images_per_prompt=1, generator=[torch.Generator().manual_seed(s) for s in range(len(states))])
    args.update(kw)
    return pipe(**args)


@pytest.fixture
def hp():
    from guided_attention_amd.utils import shared_state as state
    saved = state.curHyperParams, getattr(state, "config", None)
    state.curHyperParams = dict(state.hyperParameterOverrides)
    state.config = SimpleNamespace(custom_loss=None, diagnostic_level=0)
    yield state
    state.curHyperParams, state.config = saved


def test_the_switch_is_off_by_default():
    from guided_attention_amd.config import RunConfig
    from guided_attention_amd.pipeline_guided_attention import GuidedAttention
    assert GuidedAttention(SimpleNamespace(), None, None, None, None).batched_paint_with_words is False
    assert RunConfig(meta_prompt="a").batched_paint_with_words is False


def test_painting_batched_calls_reach_the_device_check(hp):
    from guided_attention_amd._lib import GaError
    hp.curHyperParams["paint_with_words_stop"] = 10
    with pytest.raises(GaError, match="GPU only"):           # three seeds of one prompt
        _seeds_call(_cpu_pipe())
    hp.curHyperParams["paint_with_words_stop"] = 0
    states = [_state("a robot"), _state("a vase", paint_with_words_stop=3, paint_with_words_weight=.5), _state("a cat")]
    with pytest.raises(GaError, match="GPU only"):           # guidance_states, one state paints
        _states_call(_cpu_pipe(), states)
    pipe = _cpu_pipe()
    pipe.batched_paint_with_words = False                    # off: today's refusals, word for word
    with pytest.raises(NotImplementedError, match=r"prompt 1: paint-with-words is not supported in a call with guidance_states"):
        _states_call(pipe, states)
    hp.curHyperParams["paint_with_words_stop"] = 10
    with pytest.raises(NotImplementedError, match=r"paint-with-words with num_images_per_prompt > 1 is not supported"):
        _seeds_call(pipe)


REFUSED = {"custom": "custom-loss plugins", "side_effects": "reference_side_effects", "diagnostic": "diagnostic_level > 0",
           "unfused": "fused_aggregate_loss = False", "optimizer": "use_optimizer", "sdxl": "added conditioning"}


@pytest.mark.parametrize("form", ["seeds", "states"])
@pytest.mark.parametrize("what", sorted(REFUSED))
def test_every_other_refusal_stays_with_the_switch_on(hp, what, form):
    pipe = _cpu_pipe(sdxl=what == "sdxl")
    states = [_state("a robot", paint_with_words_stop=5), _state("a vase")]
    hp.curHyperParams["paint_with_words_stop"] = 5
    cfg, hyper = (hp.config, hp.curHyperParams) if form == "seeds" else (states[1].config, states[1].hyper_params)
    if what == "custom":
        cfg.custom_loss = {"toLeftOf": (object(), "(a, b)")}
    elif what == "side_effects":
        pipe.reference_side_effects = True
    elif what == "diagnostic":
        cfg.diagnostic_level = 1
    elif what == "unfused":
        pipe.fused_aggregate_loss = False
    elif what == "optimizer":
        hyper["use_optimizer"] = True
    with pytest.raises(NotImplementedError, match=re.escape(REFUSED[what])):
        _seeds_call(pipe) if form == "seeds" else _states_call(pipe, states)


# ------------------------------------------------------------------------------------------- masks and multipliers
LAYOUTS = [{2: (.6, .3, .4, .55), 5: (.2, .3, .4, .55), 6: (.2, .3, .4, .55)}, {1: (.1, .2, .5, .6), 4: (.5, .4, .4, .5)}]


def _record(layout, i, **hp):
    from guided_attention_amd.utils import helpers, ptp_utils, shared_state as state
    token_dict = {idx: {"loss": helpers.Rect(*geom, 1), "loss_type": helpers.AnnotationType.BOX} for idx, geom in layout.items()}
    token_dict[3] = {"loss": (0.5, 0.5), "loss_type": helpers.AnnotationType.COOR}      # not a box: no mask column
    hyper = dict(state.hyperParameterOverrides, **hp)
    return SimpleNamespace(config=SimpleNamespace(token_dict=token_dict), hp=hyper, mult=ptp_utils.paint_multiplier(hyper, i))


@pytest.fixture
def sigmas():
    from guided_attention_amd.scheduler import DDIMScheduler
    from guided_attention_amd.utils import ptp_utils, shared_state as state
    saved = state.sigmas, state.timesteps, state.cur_time_step_iter, state.config, state.curHyperParams
    sch = DDIMScheduler()
    sch.set_timesteps(10, device="cpu")
    acp = sch.alphas_cumprod
    state.sigmas, state.timesteps = (((1 - acp) / acp) ** 0.5).numpy(), sch.timesteps
    yield state
    ptp_utils.set_paint_images(None)
    state.sigmas, state.timesteps, state.cur_time_step_iter, state.config, state.curHyperParams = saved


@pytest.mark.parametrize("hw", [8, 16])
def test_masks_and_multipliers_per_image(sigmas, hw):
    """Three images, two layouts: image s's slice is what paint_with_words_bias builds under image s's state and what the
    oracle's paint_with_words_mask gives; mult is 0.4 * log(1 + sigma_i) before and 0 from each image's own stop."""
    from guided_attention_amd.utils import ptp_utils
    state = sigmas
    settings = [(LAYOUTS[0], dict(paint_with_words_stop=2, paint_with_words_weight=.8)),
                (LAYOUTS[1], dict(paint_with_words_stop=1, paint_with_words_weight=.5, shrink_factor=.1)),
                (LAYOUTS[0], dict(paint_with_words_stop=0))]
    n = hw * hw
    for i in range(3):
        recs = [_record(lay, i, **hp) for lay, hp in settings]
        ptp_utils.set_paint_images(recs)
        got = ptp_utils.paint_with_words_bias_images(n, 77, torch.float32, "cpu")
        expect = [.4 * math.log(1 + float(state.sigmas[state.timesteps[i]])) if i < hp["paint_with_words_stop"] else 0.0
                  for _, hp in settings]
        assert [r.mult for r in recs] == expect
        if i >= 2:
            assert got is None                               # every image past its stop: the plain capture kernel runs
            continue
        bias, stride, mult = got
        assert bias.shape == (3, n, 77) and stride == n * 77 and bias.is_contiguous()
        assert mult.dtype == torch.float32 and torch.equal(mult, torch.tensor(expect, dtype=torch.float32))
        for s, (lay, hp) in enumerate(settings):
            ref = oattn.paint_with_words_mask(lay, n, recs[s].hp["shrink_factor"], hp.get("paint_with_words_weight", 1.0))
            assert torch.equal(bias[s], ref), (i, s)
            assert bias[s].count_nonzero() > 0
            if recs[s].mult:                                 # the solo builder under that image's state, at this step
                state.config, state.curHyperParams, state.cur_time_step_iter = recs[s].config, recs[s].hp, i
                solo_mask, solo_mult = ptp_utils.paint_with_words_bias(n, 77, torch.float32, "cpu")
                assert torch.equal(bias[s], solo_mask) and solo_mult == recs[s].mult
        assert not torch.equal(bias[0], bias[1])
        assert ptp_utils.paint_with_words_bias_images(n, 64, torch.float32, "cpu") is None     # 77-key layers only


def test_coinciding_layouts_share_one_mask(sigmas):
    from guided_attention_amd.utils import ptp_utils
    hp = dict(paint_with_words_stop=3, paint_with_words_weight=.8)
    ptp_utils.set_paint_images([_record(LAYOUTS[0], 1, **hp) for _ in range(3)])
    bias, stride, mult = ptp_utils.paint_with_words_bias_images(64, 77, torch.float32, "cpu")
    assert stride == 0 and bias.shape == (64, 77) and mult.shape == (3,) and (mult > 0).all()
    assert torch.equal(bias, oattn.paint_with_words_mask(LAYOUTS[0], 64, .15, .8))
    ptp_utils.set_paint_images(None)
    assert ptp_utils.paint_with_words_bias_images(64, 77, torch.float32, "cpu") is None


# ------------------------------------------------------------------------------------------- ABI and CLI
def test_header_and_binding_carry_the_grouped_entries():
    from guided_attention_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint " + name + r"\s*\(", text), name
        assert name in _lib.PROTOTYPES
    assert "#define GA_VERSION 183" in HEADER.read_text() and _lib.GA_VERSION == 183
    from guided_attention_amd import ops
    for name in ("attn_scores_max_grouped", "attn_capture_fwd_biased_grouped", "attn_capture_bwd_biased_grouped",
                 "attn_pww_max_grad", "AttnCapturePaintWithWordsImages"):
        assert hasattr(ops, name)


def test_grouped_entries_validate_on_the_host():
    from guided_attention_amd import _lib
    if not _lib.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    assert lib.ga_attn_scores_max_grouped(None, p, 3, 2, 64, 77, 16, 0.25, 2, 3, p, None) == -1
    assert lib.ga_attn_pww_max_grad(p, p, None, p, p, 3, 2, 64, 77, 16, 0.25, 2, 3, None) == -1
    for B, groups in ((4, 3), (65, 65), (3, 0)):             # B % G != 0, G > GA_MAX_IMAGES, G < 1
        assert lib.ga_attn_scores_max_grouped(p, p, B, 2, 64, 77, 16, 0.25, 2, groups, p, None) == -2
        assert lib.ga_attn_capture_fwd_biased_grouped(p, p, p, p, None, p, 0, p, p, B, 2, 64, 77, 16, 0.25, 2, groups, None) == -2
        assert lib.ga_attn_capture_bwd_biased_grouped(p, p, p, p, None, 0, 0, 0, p, p, 0, p, p, p, B, 2, 64, 77, 16, 0.25, 2,
                                                      groups, None) == -2
        assert lib.ga_attn_pww_max_grad(p, p, p, p, p, B, 2, 64, 77, 16, 0.25, 2, groups, None) == -2
    assert lib.ga_attn_scores_max_grouped(p, p, 64, 64, 16384, 77, 16, 0.25, 2, 2, p, None) == -2     # B*H*N*Kt >= 2^32
    assert lib.ga_attn_capture_fwd_biased_grouped(p, p, p, p, None, p, 0, p, p, 6, 2, 64, 81, 16, 0.25, 2, 3, None) == -6   # Kt > 80
    assert lib.ga_attn_scores_max_grouped(p, p, 6, 2, 64, 77, 16, 0.25, 9, 3, p, None) == -3


def test_batched_paint_with_words_is_a_cli_flag():
    from guided_attention_amd import run
    base = ["--meta_prompt", "a [robot:.6,.3,.4,.55]", "--output_path", "/tmp/ga_bpww"]
    cfg = run._parse_cli(base + ["--batched_paint_with_words", "true", "--seeds_per_pass", "2"])
    assert cfg.batched_paint_with_words is True and cfg.seeds_per_pass == 2
    assert run._parse_cli(base).batched_paint_with_words is False
