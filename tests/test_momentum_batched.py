"""SGD-momentum refinement (`use_optimizer`) in batched calls without a GPU: ga_latent_sgd_momentum_batched is declared, bound,
exported and validates its arguments on the host; with GuidedAttention.batched_momentum_refinement on, both batched forms accept
a `use_optimizer` state up to the device check; run.execute then chunks such jobs by the ordinary rule; the CLI flag."""
import ctypes
import re
from types import SimpleNamespace

import pytest
import torch

from conftest import ROOT
from test_momentum_refinement import _sweep

HEADER = ROOT / "include" / "ga_hip.h"
NAME = "ga_latent_sgd_momentum_batched"


@pytest.fixture(scope="module")
def lib():
    from guided_attention_amd import _lib
    if not _lib.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.fixture
def hp():
    from guided_attention_amd.utils import shared_state as state
    saved = state.curHyperParams, getattr(state, "config", None)
    state.curHyperParams = dict(state.hyperParameterOverrides)
    state.config = SimpleNamespace(custom_loss=None, diagnostic_level=0)
    yield state
    state.curHyperParams, state.config = saved


def _cpu_pipe(switch):
    from guided_attention_amd.pipeline_guided_attention import GuidedAttention
    from guided_attention_amd.text import SyntheticTextEncoder, WordTokenizer
    from guided_attention_amd.unet import UNetConfig
    unet = SimpleNamespace(config=UNetConfig.tiny(sample_size=32, cross_attention_dim=48), device=torch.device("cpu"),
                           dtype=torch.float32)
    pipe = GuidedAttention(unet, None, None, SyntheticTextEncoder(48), WordTokenizer())
    pipe.batched_momentum_refinement = switch
    return pipe


def _state(prompt="a robot", **hp):
    from guided_attention_amd.pipeline_guided_attention import GuidanceState
    from guided_attention_amd.utils import shared_state as state
    cfg = SimpleNamespace(prompt=prompt, custom_loss=None, diagnostic_level=0, token_dict={}, thresholds={0: .05},
                          only_update_on_threshold_steps=True, sub_prompt_avg_within=False)
    return GuidanceState(cfg, dict(state.hyperParameterOverrides, **hp))


def _seeds_call(pipe):
    return pipe(prompt="a robot", attention_store=None, num_images_per_prompt=3,
                generator=[torch.Generator().manual_seed(s) for s in range(3)])


def _states_call(pipe, states):
    return pipe(prompt=[st.config.prompt for st in states], attention_store=None, guidance_states=states,
                num_images_per_prompt=1, generator=[torch.Generator().manual_seed(s) for s in range(len(states))])


def test_entry_is_declared_bound_exported_and_wrapped(lib):
    from guided_attention_amd import _lib, ops
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert re.search(rf"\bint {NAME}\s*\(", text)
    assert len(_lib.PROTOTYPES[NAME]) == 12
    assert hasattr(lib, NAME)
    assert int(re.search(r"#define GA_VERSION (\d+)", text).group(1)) == _lib.GA_VERSION == 183
    with pytest.raises(ops.GaError, match="GPU only"):
        ops.latent_sgd_momentum_batched(torch.zeros(2, 4), torch.zeros(2, 4), torch.zeros(2, 4), [1.0, 1.0], 0.8, [1, 1], [1, 1])


def test_entry_validates_on_the_host(lib):
    from guided_attention_amd._lib import GA_MAX_IMAGES
    p = ctypes.c_void_p(4096)   # never dereferenced: every call below returns before a launch
    f = getattr(lib, NAME)
    for hole in range(7):       # latents, grad, momentum, lr, first, active, out
        x, g, m, lr, first, active, out = [None if k == hole else p for k in range(7)]
        assert f(x, g, m, lr, 0.8, first, active, out, 2, 16, 0, None) == -1, hole
    for images in (0, -1, GA_MAX_IMAGES + 1):
        assert f(p, p, p, p, 0.8, p, p, p, images, 16, 0, None) == -2
    for n in (0, -5):
        assert f(p, p, p, p, 0.8, p, p, p, 2, n, 0, None) == -2
    for mu in (1.0, -0.1, float("nan")):
        assert f(p, p, p, p, mu, p, p, p, 2, 16, 0, None) == -2
    for dtype in (3, -1):
        assert f(p, p, p, p, 0.8, p, p, p, 2, 16, dtype, None) == -3


def test_the_switch_is_off_by_default_and_a_cli_flag():
    from guided_attention_amd import run
    from guided_attention_amd.config import RunConfig
    from guided_attention_amd.pipeline_guided_attention import GuidedAttention
    assert GuidedAttention(SimpleNamespace(), None, None, None, None).batched_momentum_refinement is False
    assert RunConfig(meta_prompt="a").batched_momentum_refinement is False
    base = ["--meta_prompt", "a [robot:.6,.3,.4,.55]", "--output_path", "/tmp/ga_bmr"]
    cfg = run._parse_cli(base + ["--batched_momentum_refinement", "true", "--seeds_per_pass", "2"])
    assert cfg.batched_momentum_refinement is True and cfg.seeds_per_pass == 2
    assert run._parse_cli(base).batched_momentum_refinement is False


def test_use_optimizer_batched_calls_reach_the_device_check(hp):
    """Switch on: the `optimizer` entry leaves both refusal lists and the call gets as far as the next check, the CPU-device
    GaError.  Switch off: the refusals of before, word for word."""
    from guided_attention_amd._lib import GaError
    states = [_state("a robot"), _state("a vase", use_optimizer=True), _state("a cat")]
    with pytest.raises(GaError, match="GPU only"):
        _states_call(_cpu_pipe(True), states)
    with pytest.raises(NotImplementedError, match=r"prompt 1: use_optimizer is not supported in a call with guidance_states"):
        _states_call(_cpu_pipe(False), states)
    hp.curHyperParams["use_optimizer"] = True
    with pytest.raises(GaError, match="GPU only"):
        _seeds_call(_cpu_pipe(True))
    with pytest.raises(NotImplementedError, match=r"use_optimizer with num_images_per_prompt > 1 is not supported"):
        _seeds_call(_cpu_pipe(False))


def test_every_other_refusal_stays_with_the_switch_on(hp):
    pipe = _cpu_pipe(True)
    hp.curHyperParams.update(use_optimizer=True, paint_with_words_stop=5)
    with pytest.raises(NotImplementedError, match="paint-with-words"):
        _seeds_call(pipe)
    with pytest.raises(NotImplementedError, match="prompt 1: paint-with-words"):
        _states_call(pipe, [_state("a robot", use_optimizer=True), _state("a vase", use_optimizer=True, paint_with_words_stop=5)])
    hp.curHyperParams["paint_with_words_stop"] = 0
    pipe.reference_side_effects = True
    with pytest.raises(NotImplementedError, match="reference_side_effects"):
        _seeds_call(pipe)


def _sweep_on(tmp_path, monkeypatch, *args, **kw):
    """test_momentum_refinement._sweep with config.batched_momentum_refinement = True (set where the sweep hands its
    RunConfig to run.execute)."""
    from guided_attention_amd import run
    inner = run.execute

    def execute(cfg, *a, **k):
        cfg.batched_momentum_refinement = True
        return inner(cfg, *a, **k)
    with monkeypatch.context() as m:
        m.setattr(run, "execute", execute)
        return _sweep(tmp_path, m, *args, **kw)


def test_execute_batches_the_seeds_of_a_use_optimizer_state(tmp_path, monkeypatch):
    calls, folder = _sweep_on(tmp_path, monkeypatch, [{"use_optimizer": True}], [3, 1, 4], 2)
    assert calls == [([3, 1], [True, True]), ([4], [True])]
    names = sorted(p.name for p in folder.glob("*.txt"))
    assert len(names) == 3 and all("use_optimizer_True" in n for n in names)
    for s in (3, 1, 4):          # the same files as the solo sweep writes, each with its own image's log
        (txt,) = [p for p in folder.glob(f"{s}_*.txt")]
        assert f"seed {s} optimizer True" in txt.read_text()
    assert len(list(folder.glob("*use_optimizer_True*.png"))) == 3


def test_execute_batches_plain_and_use_optimizer_states_of_a_seed(tmp_path, monkeypatch):
    calls, folder = _sweep_on(tmp_path / "on", monkeypatch, [{}, {"use_optimizer": True}], [3, 1], 2, across=True)
    assert calls == [([3, 3], [False, True]), ([1, 1], [False, True])]
    assert len(list(folder.glob("*use_optimizer_True*.png"))) == 2 and len(list(folder.glob("*use_optimizer_False*.png"))) == 2
    solo, solo_folder = _sweep(tmp_path / "off", monkeypatch, [{}, {"use_optimizer": True}], [3, 1], 2, across=True)
    assert solo == [([3], [False]), ([3], [True]), ([1], [False]), ([1], [True])]          # switch off: as before
    assert sorted(p.name for p in solo_folder.iterdir()) == sorted(p.name for p in folder.iterdir())   # file names unchanged
