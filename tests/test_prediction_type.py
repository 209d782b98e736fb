"""v-prediction and sample-prediction checkpoints in the CFG + DDIM step, the parts that need no GPU: the two C entry points
(declared, bound, exported, validating on the host), the scheduler's arithmetic for the three prediction types, the wrappers'
and the pipeline's refusals, and what `from_pretrained` reads from a checkpoint folder."""
import ctypes
import json
import math
import re

import numpy as np
import pytest
import torch

import hashrand
from conftest import ROOT

HEADER = ROOT / "include" / "ga_hip.h"
TYPES = ("epsilon", "v_prediction", "sample")


@pytest.fixture(scope="module")
def lib():
    from guided_attention_amd import _lib
    if not _lib.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def reference_step(kind, m, x, a_t, a_prev):
    """The issue's table in whatever precision m and x come in (fp64 in the tests): -> (prev, x0)."""
    sa, s1 = math.sqrt(a_t), math.sqrt(1 - a_t)
    if kind == "epsilon":
        x0, eps = (x - s1 * m) / sa, m
    elif kind == "v_prediction":
        x0, eps = sa * x - s1 * m, sa * m + s1 * x
    else:
        x0, eps = m, (x - sa * m) / s1
    return math.sqrt(a_prev) * x0 + math.sqrt(1 - a_prev) * eps, x0


def test_header_binding_and_library_agree(lib):
    from guided_attention_amd import _lib
    text = HEADER.read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in (("ga_cfg_ddim_step_pred", 12), ("ga_cfg_ddim_step_pred_masked", 14)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name
        assert len(m.group(1).split(",")) == n_args
        assert len(_lib.PROTOTYPES[name]) == n_args
        assert hasattr(lib, name)
    for name, value in (("GA_PRED_EPSILON", 0), ("GA_PRED_V", 1), ("GA_PRED_SAMPLE", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), code), name
        assert getattr(_lib, name) == value
    version = int(re.search(r"#define GA_VERSION (\d+)", text).group(1))
    assert version == _lib.GA_VERSION == lib.ga_version()


def test_entries_validate_on_the_host(lib):
    p = ctypes.c_void_p(4096)   # never dereferenced: every call below returns before a launch
    nan = float("nan")

    def solo(u=p, t=p, x=p, prev=p, a_t=0.5, a_p=0.6, pred=1, n=16, dtype=0):
        return lib.ga_cfg_ddim_step_pred(u, t, 7.5, x, a_t, a_p, pred, prev, None, n, dtype, None)

    def masked(u=p, t=p, x=p, prev=p, a_t=0.5, a_p=0.6, pred=1, n=16, dtype=0, active=p, images=2):
        return lib.ga_cfg_ddim_step_pred_masked(u, t, 7.5, x, a_t, a_p, pred, active, prev, None, images, n, dtype, None)

    for f in (solo, masked):
        for missing in ("u", "t", "x", "prev"):
            assert f(**{missing: None}) == -1, (f.__name__, missing)
        assert f(n=0) == -2 and f(n=-5) == -2
        for a in (0.0, -0.1, 1.5, nan):
            assert f(a_t=a) == -2 and f(a_p=a) == -2, (f.__name__, a)
        assert f(pred=-1) == -2 and f(pred=3) == -2
        assert f(pred=2, a_t=1.0) == -2                  # sample: the division by sqrt(1 - alpha_t)
        assert f(dtype=3) == -3 and f(dtype=-1) == -3
    assert masked(active=None) == -1
    assert masked(images=0) == -2 and masked(images=65) == -2


@pytest.mark.parametrize("kind", TYPES)
def test_scheduler_step_follows_the_table(kind):
    from guided_attention_amd.scheduler import DDIMScheduler
    sch = DDIMScheduler(prediction_type=kind)
    sch.set_timesteps(50)
    m = torch.from_numpy(hashrand.normalish((4, 9, 9), 11))
    x = torch.from_numpy(hashrand.normalish((4, 9, 9), 12))
    for t in (981, 501, 1):
        assert t in sch.timesteps.tolist()
        a_t, a_prev = sch.alphas_for(t)
        out = sch.step(m, t, x)
        prev, x0 = reference_step(kind, m.double().numpy(), x.double().numpy(), a_t, a_prev)
        for got, ref in ((out.prev_sample, prev), (out.pred_original_sample, x0)):   # rtol 1e-6 of the largest element
            assert got.dtype == torch.float32
            assert np.abs(got.double().numpy() - ref).max() <= 1e-6 * np.abs(ref).max(), (kind, t)
    with pytest.raises(NotImplementedError):
        sch.step(m, 981, x, eta=0.5)


def test_wrappers_refuse_on_the_cpu():
    from guided_attention_amd import ops
    z = torch.zeros(8)
    with pytest.raises(ops.GaError, match="GPU only"):
        ops.cfg_ddim_step(z, z, 7.5, z, 0.5, 0.6, prediction="v_prediction")
    with pytest.raises(ops.GaError, match="GPU only"):
        ops.cfg_ddim_step_masked(z.reshape(2, 4), z.reshape(2, 4), 7.5, z.reshape(2, 4), 0.5, 0.6, [1, 0], prediction="sample")
    with pytest.raises(ValueError):
        ops.cfg_ddim_step(z, z, 7.5, z, 0.5, 0.6, prediction="nonsense")
    with pytest.raises(ValueError):
        ops.cfg_ddim_step_masked(z.reshape(2, 4), z.reshape(2, 4), 7.5, z.reshape(2, 4), 0.5, 0.6, [1, 0], prediction="nonsense")


def test_pipeline_refuses_an_unknown_prediction_type_before_the_device_check():
    from guided_attention_amd._lib import GaError
    from guided_attention_amd.pipeline_guided_attention import GuidedAttention
    from guided_attention_amd.unet import UNetConfig
    from guided_attention_amd.utils import shared_state as state
    from guided_attention_amd.utils.ptp_utils import AttentionStore
    state.curHyperParams = dict(state.hyperParameterOverrides)
    pipe = GuidedAttention.from_pretrained("x", random_init=True, unet_config=UNetConfig.tiny(32, 48))
    call = dict(prompt=None, prompt_embeds=torch.zeros(1, 77, 48), negative_prompt_embeds=torch.zeros(1, 77, 48),
                attention_store=AttentionStore(), latents=torch.zeros(1, 4, 32, 32), output_type="latent")
    pipe.scheduler.config.prediction_type = "nonsense"
    with pytest.raises(ValueError, match="nonsense"):
        pipe(**call)
    pipe.scheduler.config.prediction_type = "v_prediction"    # a served type gets as far as the device check
    with pytest.raises(GaError, match="GPU only"):
        pipe(**call)


def _folder(tmp_path, scheduler=None, unet=None):
    (tmp_path / "unet").mkdir(parents=True)   # an empty unet/ makes the folder a local checkpoint; weights=False reads no file
    if scheduler is not None:
        (tmp_path / "scheduler").mkdir()
        (tmp_path / "scheduler" / "scheduler_config.json").write_text(json.dumps(scheduler))
    if unet is not None:
        (tmp_path / "unet" / "config.json").write_text(json.dumps(unet))
    return tmp_path


V_CONFIG = {"_class_name": "DDIMScheduler", "beta_schedule": "scaled_linear", "beta_start": 0.00085, "beta_end": 0.012,
            "num_train_timesteps": 1000, "prediction_type": "v_prediction", "steps_offset": 1, "set_alpha_to_one": False,
            "clip_sample": False}


def test_from_pretrained_reads_the_scheduler_config(tmp_path):
    from guided_attention_amd.pipeline_guided_attention import GuidedAttention
    from guided_attention_amd.unet import UNetConfig
    pipe = GuidedAttention.from_pretrained(_folder(tmp_path / "v", V_CONFIG), weights=False, unet_config=UNetConfig.tiny(32, 48))
    c = pipe.scheduler.config
    assert (c.prediction_type, c.steps_offset, c.set_alpha_to_one, c.num_train_timesteps) == ("v_prediction", 1, False, 1000)
    assert (c.beta_start, c.beta_end) == (0.00085, 0.012)
    other = dict(V_CONFIG, prediction_type="sample", num_train_timesteps=500, beta_start=0.001, beta_end=0.02, steps_offset=0,
                 set_alpha_to_one=True)
    c = GuidedAttention.from_pretrained(_folder(tmp_path / "other", other), weights=False,
                                        unet_config=UNetConfig.tiny(32, 48)).scheduler.config
    assert (c.prediction_type, c.num_train_timesteps, c.beta_start, c.beta_end, c.steps_offset, c.set_alpha_to_one) == \
        ("sample", 500, 0.001, 0.02, 0, True)
    plain = GuidedAttention.from_pretrained(_folder(tmp_path / "plain"), weights=False, unet_config=UNetConfig.tiny(32, 48))
    c = plain.scheduler.config
    assert (c.prediction_type, c.steps_offset, c.set_alpha_to_one, c.num_train_timesteps) == ("epsilon", 1, False, 1000)
    with pytest.raises(ValueError, match="beta_schedule"):
        GuidedAttention.from_pretrained(_folder(tmp_path / "linear", dict(V_CONFIG, beta_schedule="linear")), weights=False,
                                        unet_config=UNetConfig.tiny(32, 48))


def test_from_pretrained_reads_the_unet_sample_size(tmp_path):
    from guided_attention_amd.pipeline_guided_attention import GuidedAttention
    from guided_attention_amd.unet import UNetConfig
    with torch.device("meta"):   # the full-width architecture without its memory
        pipe = GuidedAttention.from_pretrained(_folder(tmp_path / "s96", V_CONFIG, {"sample_size": 96}), weights=False)
        assert pipe.unet.config.sample_size == 96 and pipe.scheduler.config.prediction_type == "v_prediction"
        assert GuidedAttention.from_pretrained(_folder(tmp_path / "s64"), weights=False).unet.config.sample_size == 64
    # a config passed by the caller wins over the file
    pipe = GuidedAttention.from_pretrained(_folder(tmp_path / "given", None, {"sample_size": 96}), weights=False,
                                           unet_config=UNetConfig.tiny(32, 48))
    assert pipe.unet.config.sample_size == 32
