"""eta > 0 (stochastic DDIM) in the CFG + DDIM step, the parts that need no GPU: the two C entry points (declared, bound,
exported, validating on the host), the scheduler's arithmetic with a variance noise for the three prediction types, the
wrappers' and the pipeline's refusals, and the helper that draws the noise.

    var = (1 - a_p) / (1 - a_t) * (1 - a_t / a_p);  sigma = eta * sqrt(var);  c_dir = sqrt(max(0, 1 - a_p - sigma^2))
    prev = sqrt(a_p) * x0 + c_dir * eps + sigma * z          (x0, eps: the table of include/ga_hip.h)"""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

import hashrand
from conftest import ROOT

HEADER = ROOT / "include" / "ga_hip.h"
TYPES = ("epsilon", "v_prediction", "sample")
ETAS = (0.5, 1.0)


@pytest.fixture(scope="module")
def lib():
    from guided_attention_amd import _lib
    if not _lib.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def reference_step(kind, m, x, z, a_t, a_prev, eta):
    """The issue's formulas in whatever precision m, x and z come in (fp64 in the tests): -> (prev, x0)."""
    sa, s1 = math.sqrt(a_t), math.sqrt(1 - a_t)
    if kind == "epsilon":
        x0, eps = (x - s1 * m) / sa, m
    elif kind == "v_prediction":
        x0, eps = sa * x - s1 * m, sa * m + s1 * x
    else:
        x0, eps = m, (x - sa * m) / s1
    sigma = eta * math.sqrt((1 - a_prev) / (1 - a_t) * (1 - a_t / a_prev))
    c_dir = math.sqrt(max(0.0, 1 - a_prev - sigma ** 2))
    return math.sqrt(a_prev) * x0 + c_dir * eps + sigma * z, x0


# ===================================================================================== ABI
def test_header_binding_and_library_agree(lib):
    from guided_attention_amd import _lib
    text = HEADER.read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in (("ga_cfg_ddim_step_eta", 14), ("ga_cfg_ddim_step_eta_masked", 16)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == n_args
        assert args[3].endswith(" x") and args[4].endswith(" noise")               # the noise directly behind x
        assert args[6].endswith(" alpha_prev") and args[7] == "float eta"           # eta directly behind alpha_prev
        assert len(_lib.PROTOTYPES[name]) == n_args
        assert _lib.PROTOTYPES[name][4] is ctypes.c_void_p and _lib.PROTOTYPES[name][7] is ctypes.c_float
        assert hasattr(lib, name)
    version = int(re.search(r"#define GA_VERSION (\d+)", text).group(1))
    assert version == _lib.GA_VERSION == lib.ga_version() == 183


def test_entries_validate_on_the_host(lib):
    p = ctypes.c_void_p(4096)   # never dereferenced: every call below returns before a launch
    nan = float("nan")

    def solo(u=p, t=p, x=p, z=p, prev=p, a_t=0.5, a_p=0.6, eta=0.5, pred=1, n=16, dtype=0):
        return lib.ga_cfg_ddim_step_eta(u, t, 7.5, x, z, a_t, a_p, eta, pred, prev, None, n, dtype, None)

    def masked(u=p, t=p, x=p, z=p, prev=p, a_t=0.5, a_p=0.6, eta=0.5, pred=1, n=16, dtype=0, active=p, images=2):
        return lib.ga_cfg_ddim_step_eta_masked(u, t, 7.5, x, z, a_t, a_p, eta, pred, active, prev, None, images, n, dtype, None)

    for f in (solo, masked):
        for eta in (0.0, 0.5):
            for missing in ("u", "t", "x", "prev"):
                assert f(**{missing: None}, eta=eta) == -1, (f.__name__, missing, eta)
        # the noise: not needed at eta = 0 (accepted up to the next check, here the dtype), required at eta > 0
        assert f(z=None, eta=0.0, dtype=3) == -3 and f(z=None, eta=0.0, n=0) == -2
        assert f(z=None, eta=0.5) == -1 and f(z=None, eta=0.5, dtype=3) == -1 and f(z=None, eta=1.0) == -1
        for eta in (-0.1, 1.5, nan):
            assert f(eta=eta) == -2 and f(eta=eta, dtype=3) == -2, (f.__name__, eta)
        assert f(eta=0.5, a_t=1.0, a_p=1.0) == -2            # the division by 1 - alpha_t
        assert f(eta=0.5, a_t=0.6, a_p=0.5) == -2            # alpha_t > alpha_prev: a negative variance
        assert f(eta=0.5, a_t=0.5, a_p=0.5, dtype=3) == -3   # alpha_t == alpha_prev is served (sigma = 0): on to the dtype
        for eta in (0.0, 0.5):                               # the existing cases, at either eta
            assert f(eta=eta, n=0) == -2 and f(eta=eta, n=-5) == -2
            for a in (0.0, -0.1, 1.5, nan):
                assert f(eta=eta, a_t=a) == -2 and f(eta=eta, a_p=a) == -2, (f.__name__, a)
            assert f(eta=eta, pred=-1) == -2 and f(eta=eta, pred=3) == -2
            assert f(eta=eta, pred=2, a_t=1.0, a_p=1.0) == -2
            assert f(eta=eta, dtype=3) == -3 and f(eta=eta, dtype=-1) == -3
    for eta in (0.0, 0.5):
        assert masked(active=None, eta=eta) == -1
        assert masked(images=0, eta=eta) == -2 and masked(images=65, eta=eta) == -2


# ===================================================================================== the scheduler
@pytest.mark.parametrize("eta", ETAS)
@pytest.mark.parametrize("kind", TYPES)
def test_scheduler_step_follows_the_formulas(kind, eta):
    from guided_attention_amd.scheduler import DDIMScheduler
    sch = DDIMScheduler(prediction_type=kind)
    sch.set_timesteps(50)
    m = torch.from_numpy(hashrand.normalish((4, 9, 9), 11))
    x = torch.from_numpy(hashrand.normalish((4, 9, 9), 12))
    z = torch.from_numpy(hashrand.normalish((4, 9, 9), 13))
    for t in (981, 501, 1):
        assert t in sch.timesteps.tolist()
        a_t, a_prev = sch.alphas_for(t)
        out = sch.step(m, t, x, eta=eta, variance_noise=z)
        prev, x0 = reference_step(kind, m.double().numpy(), x.double().numpy(), z.double().numpy(), a_t, a_prev, eta)
        for got, ref in ((out.prev_sample, prev), (out.pred_original_sample, x0)):   # rtol 1e-6 of the largest element
            assert got.dtype == torch.float32
            assert np.abs(got.double().numpy() - ref).max() <= 1e-6 * np.abs(ref).max(), (kind, t)
        # the noise is in the result: sigma * z is 1.6e-2 (t = 1) .. 0.14 (t = 981, eta = 1) of it
        assert not torch.equal(out.prev_sample, sch.step(m, t, x, eta=eta, variance_noise=torch.zeros_like(z)).prev_sample)
        assert torch.equal(out.pred_original_sample, sch.step(m, t, x).pred_original_sample)     # x0 does not depend on eta
    with pytest.raises(NotImplementedError, match="variance_noise"):
        sch.step(m, 981, x, eta=eta)


@pytest.mark.parametrize("kind", TYPES)
def test_scheduler_step_at_eta_zero_does_not_read_the_noise(kind):
    from guided_attention_amd.scheduler import DDIMScheduler
    sch = DDIMScheduler(prediction_type=kind)
    sch.set_timesteps(50)
    m = torch.from_numpy(hashrand.normalish((4, 9, 9), 21))
    x = torch.from_numpy(hashrand.normalish((4, 9, 9), 22))
    z = torch.full((4, 9, 9), float("nan"))
    for t in (981, 501, 1):
        plain, with_noise = sch.step(m, t, x), sch.step(m, t, x, eta=0.0, variance_noise=z)
        assert torch.equal(plain.prev_sample, with_noise.prev_sample)
        assert torch.equal(plain.pred_original_sample, with_noise.pred_original_sample)


# ===================================================================================== the wrappers
def test_wrappers_refuse():
    from guided_attention_amd import ops
    z = torch.zeros(8)
    zm = z.reshape(2, 4)
    for eta in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="eta"):
            ops.cfg_ddim_step(z, z, 7.5, z, 0.5, 0.6, eta=eta, noise=z)
        with pytest.raises(ValueError, match="eta"):
            ops.cfg_ddim_step_masked(zm, zm, 7.5, zm, 0.5, 0.6, [1, 0], eta=eta, noise=zm)
    with pytest.raises(ValueError, match="noise"):
        ops.cfg_ddim_step(z, z, 7.5, z, 0.5, 0.6, eta=0.5)
    with pytest.raises(ValueError, match="noise"):
        ops.cfg_ddim_step_masked(zm, zm, 7.5, zm, 0.5, 0.6, [1, 0], eta=0.5)
    for bad in (torch.zeros(7), torch.zeros(8, dtype=torch.float16)):     # another shape, another dtype
        with pytest.raises(ValueError, match="noise"):
            ops.cfg_ddim_step(z, z, 7.5, z, 0.5, 0.6, eta=0.5, noise=bad)
    with pytest.raises(ValueError, match="noise"):
        ops.cfg_ddim_step_masked(zm, zm, 7.5, zm, 0.5, 0.6, [1, 0], eta=0.5, noise=z)
    for kind in TYPES:
        with pytest.raises(ops.GaError, match="GPU only"):
            ops.cfg_ddim_step(z, z, 7.5, z, 0.5, 0.6, prediction=kind, eta=0.5, noise=z)
        with pytest.raises(ops.GaError, match="GPU only"):
            ops.cfg_ddim_step_masked(zm, zm, 7.5, zm, 0.5, 0.6, [1, 0], prediction=kind, eta=0.5, noise=zm)


# ===================================================================================== the pipeline, on the CPU device
def cpu_pipe_and_call():
    from guided_attention_amd.pipeline_guided_attention import GuidedAttention
    from guided_attention_amd.unet import UNetConfig
    from guided_attention_amd.utils import shared_state as state
    from guided_attention_amd.utils.ptp_utils import AttentionStore
    state.curHyperParams = dict(state.hyperParameterOverrides)
    pipe = GuidedAttention.from_pretrained("x", random_init=True, unet_config=UNetConfig.tiny(32, 48))
    call = dict(prompt=None, prompt_embeds=torch.zeros(1, 77, 48), negative_prompt_embeds=torch.zeros(1, 77, 48),
                attention_store=AttentionStore(), latents=torch.zeros(1, 4, 32, 32), output_type="latent")
    return pipe, call


def test_pipeline_checks_eta_before_the_device_check():
    from guided_attention_amd._lib import GaError
    pipe, call = cpu_pipe_and_call()
    for eta in (1.5, -0.1, float("nan")):
        with pytest.raises(ValueError, match="eta"):
            pipe(**call, eta=eta)
    with pytest.raises(GaError, match="GPU only"):     # a served eta gets as far as the device check
        pipe(**call, eta=0.5)
    with pytest.raises(GaError, match="GPU only"):
        pipe(**call, eta=1.0, variance_noise=[torch.zeros(1, 4, 32, 32)])


def test_batched_call_needs_a_noise_source_per_image():
    from guided_attention_amd._lib import GaError
    pipe, call = cpu_pipe_and_call()
    call = dict(call, latents=torch.zeros(3, 4, 32, 32), num_images_per_prompt=3)
    with pytest.raises(ValueError, match="eta > 0"):    # latents given, no generators, no variance_noise
        pipe(**call, eta=0.5)
    z = torch.zeros(1, 4, 32, 32)
    with pytest.raises(ValueError, match="variance_noise"):   # the wrong outer length
        pipe(**call, eta=0.5, variance_noise=[[z], [z]])
    with pytest.raises(ValueError, match="variance_noise"):   # a flat list where per-image lists belong
        pipe(**call, eta=0.5, variance_noise=[z, z, z])
    with pytest.raises(GaError, match="GPU only"):
        pipe(**call, eta=0.5, variance_noise=[[z], [z], [z]])
    with pytest.raises(GaError, match="GPU only"):
        pipe(**dict(call, latents=None), eta=0.5, generator=[torch.Generator().manual_seed(s) for s in range(3)])
    with pytest.raises(GaError, match="GPU only"):     # eta = 0: today's call, the keyword is not looked at
        pipe(**call, variance_noise=[[z], [z]])


# ===================================================================================== the drawing helper
def test_the_helper_draws_what_the_generator_draws_next():
    from guided_attention_amd.pipeline_guided_attention import draw_variance_noise
    shape = (1, 4, 32, 32)
    for dtype in (torch.float32, torch.float16):
        g, twin = torch.Generator().manual_seed(7), torch.Generator().manual_seed(7)
        lat = torch.randn(shape, generator=g, dtype=dtype)          # what prepare_latents draws
        assert torch.equal(lat, torch.randn(shape, generator=twin, dtype=dtype))
        for k in range(3):
            z = draw_variance_noise(g, shape, dtype, torch.device("cpu"), f"image 0, CFG step {k}")
            assert z.dtype == dtype and tuple(z.shape) == shape
            assert torch.equal(z, torch.randn(shape, generator=twin, dtype=dtype)), k


def test_the_helper_pops_a_list_and_names_where_it_ran_out():
    from guided_attention_amd.pipeline_guided_attention import draw_variance_noise
    shape = (1, 4, 8, 8)
    a, b = torch.randn(shape), torch.randn(shape)
    src = [a, b]
    assert torch.equal(draw_variance_noise(src, shape, torch.float32, torch.device("cpu")), a)
    got = draw_variance_noise(src, shape, torch.float16, torch.device("cpu"))
    assert got.dtype == torch.float16 and torch.equal(got, b.half()) and src == []
    with pytest.raises(ValueError, match="image 2, CFG step 5"):
        draw_variance_noise(src, shape, torch.float32, torch.device("cpu"), "image 2, CFG step 5")
    with pytest.raises(ValueError, match="variance_noise"):
        draw_variance_noise([torch.zeros(1, 4, 4, 4)], shape, torch.float32, torch.device("cpu"))
