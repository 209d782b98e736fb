"""eta > 0 (stochastic DDIM) on the MI355X: ga_cfg_ddim_step_eta / _eta_masked against fp64 and against each other, each new term
on its own, eta = 0 against the launch it has always been, and the pipeline (solo eager, recurse rounds, hipGraphs with the
joint pass, batched, generator-drawn noise) against the CPU oracle whose DDIM step is replaced, for the test's duration, by

    m = u + g * (t - u);   x0, eps: the table of include/ga_hip.h (test_prediction_type_gpu.table64)
    var = (1 - a_p) / (1 - a_t) * (1 - a_t / a_p);  sigma = eta * sqrt(var);  c_dir = sqrt(max(0, 1 - a_p - sigma^2))
    prev = sqrt(a_p) * x0 + c_dir * eps + sigma * z

with z popped from the same list the product gets as `variance_noise`.  Kernel tolerances are the project's TOL table (f32 2e-5,
f16 2e-3, bf16 1.6e-2 of max |ref|); the alphas are those of the real 50-step schedule at t = 981, 501 and 1: f32 values
exactly, so the fp64 reference works on the numbers the entry receives.  An f32 emulation of the element function on the CPU
sits at 2e-7 .. 1e-6 of max |ref| for all 18 (t, eta, kind) cases."""
import copy
import math

import numpy as np
import pytest
import torch

import hashrand
from test_kernels_gpu import DT, TOL, close, dev
from test_oracle_loop import BASE_ENTRIES, G9, g9_setup
from test_output_bounds_gpu import bounds
from test_pipeline_gpu import build_product, wide_setup
from test_prediction_type_gpu import (ALL, CODE, GS, MAIN, TWO_TRIPS, TYPES, f64, meta4, operands, oracle_run, product,
                                      schedule_alphas, table64)
from test_seeds_per_pass_gpu import FP32_SEEDS, _per_image, _rel

pytestmark = pytest.mark.gpu

ETAS = [0.5, 1.0]
PROMPT = "a [robot:.6,.3,.4,.55] and a [blue vase:.2,.3,.4,.55]"


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from guided_attention_amd import ops as _ops
    _ops.load()
    _ops.prepare_device("cuda")
    return _ops


def coefficients(a_t, a_p, eta):
    """(sigma, c_dir) in fp64."""
    sigma = eta * math.sqrt((1 - a_p) / (1 - a_t) * (1 - a_t / a_p))
    return sigma, math.sqrt(max(0.0, 1 - a_p - sigma ** 2))


def eta64(kind, u, t, x, z, a_t, a_p, eta, gs=GS):
    """(prev, x0) of the formulas above in fp64 numpy."""
    _, x0 = table64(kind, u, t, x, a_t, a_p, gs)
    m = u + gs * (t - u)
    sa, s1 = math.sqrt(a_t), math.sqrt(1 - a_t)
    eps = m if kind == "epsilon" else sa * m + s1 * x if kind == "v_prediction" else (x - sa * m) / s1
    sigma, c_dir = coefficients(a_t, a_p, eta)
    return math.sqrt(a_p) * x0 + c_dir * eps + sigma * z, x0


def operands4(shape, dt, seed):
    return operands(shape, dt, seed) + (dev(hashrand.normalish(shape, seed + 3), DT[dt]),)


# ===================================================================================== the kernels against fp64
@pytest.mark.parametrize("eta", ETAS)
@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("n", [1, 7, 1000, 1027])
@pytest.mark.parametrize("kind", TYPES)
def test_step_vs_fp64(ops, kind, n, dt, eta):
    """n = 1: one thread; 7: a partial wave; 1000: three whole blocks and a partial one; 1027: an odd count behind whole blocks."""
    u, t, x, z = operands4((n,), dt, 131)
    for a_t, a_p in schedule_alphas():
        prev_r, x0_r = eta64(kind, f64(u), f64(t), f64(x), f64(z), a_t, a_p, eta)
        with bounds(ops, u, t, x, z) as g:
            prev, x0 = ops.cfg_ddim_step(u, t, GS, x, a_t, a_p, True, kind, eta, z)
            prev2, none = ops.cfg_ddim_step(u, t, GS, x, a_t, a_p, False, kind, eta, z)
            for out, what in ((prev, "prev"), (x0, "x0"), (prev2, "prev, no x0")):
                g.assert_written(out, what)
        assert none is None and torch.equal(prev, prev2)
        close(prev, prev_r, TOL[dt], f"{kind} prev a_t={a_t:.4f} eta={eta}")
        close(x0, x0_r, TOL[dt], f"{kind} x0 a_t={a_t:.4f} eta={eta}")


@pytest.mark.parametrize("kind", TYPES)
def test_step_second_trip_of_the_grid_stride_loop(ops, kind):
    u, t, x, z = operands4((TWO_TRIPS,), "f16", 141)
    a_t, a_p = schedule_alphas()[1]
    prev_r, x0_r = eta64(kind, f64(u), f64(t), f64(x), f64(z), a_t, a_p, 1.0)
    with bounds(ops, u, t, x, z) as g:
        prev, x0 = ops.cfg_ddim_step(u, t, GS, x, a_t, a_p, True, kind, 1.0, z)
        g.assert_written(prev, "prev")
        g.assert_written(x0, "x0")
    close(prev, prev_r, TOL["f16"], f"{kind} prev")
    close(x0, x0_r, TOL["f16"], f"{kind} x0")
    close(prev[-300:], prev_r[-300:], TOL["f16"], f"{kind} prev, the second trip")   # the 5 elements of the second trip and their block


# ===================================================================================== each new term on its own
# At t = 1 the noise term is 1.6e-2 of the result's maximum, the bf16 bar itself: the whole-tensor comparison above could pass a
# kernel that drops the noise there.
@pytest.mark.parametrize("eta", ETAS)
@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("kind", TYPES)
def test_the_noise_term_alone(ops, kind, dt, eta):
    """Model outputs and x all zero: prev = sigma * z, held to TOL of max |sigma * z|."""
    n = 1027
    zero = torch.zeros(n, device="cuda", dtype=DT[dt])
    z = dev(hashrand.normalish((n,), 151), DT[dt])
    for a_t, a_p in schedule_alphas():
        sigma, _ = coefficients(a_t, a_p, eta)
        assert sigma > 0
        prev, x0 = ops.cfg_ddim_step(zero, zero, GS, zero, a_t, a_p, True, kind, eta, z)
        close(prev, sigma * f64(z), TOL[dt], f"{kind} sigma * z a_t={a_t:.4f} eta={eta}")
        assert not x0.any()


@pytest.mark.parametrize("eta", ETAS)
@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("kind", TYPES)
def test_the_direction_term_alone(ops, kind, dt, eta):
    """z = 0: prev = sqrt(a_p) x0 + c_dir eps, held to TOL.  The fp64 value itself is away from the eta = 0 value (c_dir against
    sqrt(1 - a_p)) by more than 10 * TOL of the maximum for f32 and f16 at t = 981 and t = 501 (asserted on the references), so a
    kernel that kept the eta = 0 coefficient misses the bar there."""
    n = 1027
    u, t, x = operands((n,), dt, 161)
    zero = torch.zeros(n, device="cuda", dtype=DT[dt])
    for step, (a_t, a_p) in enumerate(schedule_alphas()):
        prev_r, _ = eta64(kind, f64(u), f64(t), f64(x), 0.0, a_t, a_p, eta)
        prev, _ = ops.cfg_ddim_step(u, t, GS, x, a_t, a_p, False, kind, eta, zero)
        close(prev, prev_r, TOL[dt], f"{kind} z = 0 a_t={a_t:.4f} eta={eta}")
        if dt != "bf16" and step < 2:
            plain_r, _ = table64(kind, f64(u), f64(t), f64(x), a_t, a_p)
            scale = np.abs(prev_r).max()
            assert np.abs(prev_r - plain_r).max() > 10 * TOL[dt] * scale          # a property of the inputs
            plain, _ = ops.cfg_ddim_step(u, t, GS, x, a_t, a_p, False, kind)
            assert float((prev.double() - plain.double()).abs().max()) > 10 * TOL[dt] * scale


# ===================================================================================== eta = 0 is the old launch
def _direct(ops, kind, u, t, x, z, a_t, a_p, eta, want_x0, active=None):
    """ga_cfg_ddim_step_eta[_masked] called on the binding itself."""
    prev = torch.empty_like(x)
    x0 = torch.empty_like(x) if want_x0 else None
    lib, p = ops.load(), ops._ptr
    if active is None:
        ops.check(lib.ga_cfg_ddim_step_eta(p(u), p(t), GS, p(x), p(z), a_t, a_p, eta, CODE[kind], p(prev), p(x0), x.numel(),
                                           ops.dtype_code(x), ops.stream_ptr()), "ga_cfg_ddim_step_eta")
    else:
        S = x.shape[0]
        ops.check(lib.ga_cfg_ddim_step_eta_masked(p(u), p(t), GS, p(x), p(z), a_t, a_p, eta, CODE[kind], p(active), p(prev),
                                                  p(x0), S, x.numel() // S, ops.dtype_code(x), ops.stream_ptr()),
                  "ga_cfg_ddim_step_eta_masked")
    return prev, x0


@pytest.mark.parametrize("n,dt", [(n, dt) for n in (7, 1027) for dt in ALL])
@pytest.mark.parametrize("kind", TYPES)
def test_eta_zero_is_the_old_launch(ops, kind, n, dt):
    u, t, x = operands((n,), dt, 171)
    S = 3
    um, tm, xm = operands((S, n), dt, 181)
    nan, nan_m = torch.full_like(x, float("nan")), torch.full_like(xm, float("nan"))
    active = torch.tensor([1, 0, 1], dtype=torch.int32, device="cuda")
    old_key = "cfg_ddim_step" if kind == "epsilon" else "cfg_ddim_step_pred"
    for a_t, a_p in schedule_alphas():
        old = ops.cfg_ddim_step(u, t, GS, x, a_t, a_p, True, kind)
        ops.start_census()
        new = [ops.cfg_ddim_step(u, t, GS, x, a_t, a_p, True, kind, eta=0.0, noise=None),
               ops.cfg_ddim_step(u, t, GS, x, a_t, a_p, True, kind, eta=0.0, noise=nan)]
        assert [k[0] for k in ops.stop_census()] == [old_key]
        new += [_direct(ops, kind, u, t, x, None, a_t, a_p, 0.0, True), _direct(ops, kind, u, t, x, nan, a_t, a_p, 0.0, True)]
        for prev, x0 in new:
            assert torch.equal(prev, old[0]) and torch.equal(x0, old[1])
        old = ops.cfg_ddim_step_masked(um, tm, GS, xm, a_t, a_p, active, True, kind)
        ops.start_census()
        new = [ops.cfg_ddim_step_masked(um, tm, GS, xm, a_t, a_p, active, True, kind, eta=0.0, noise=None),
               ops.cfg_ddim_step_masked(um, tm, GS, xm, a_t, a_p, active, True, kind, eta=0.0, noise=nan_m)]
        assert [k[0] for k in ops.stop_census()] == [old_key + "_masked"]
        new += [_direct(ops, kind, um, tm, xm, None, a_t, a_p, 0.0, True, active),
                _direct(ops, kind, um, tm, xm, nan_m, a_t, a_p, 0.0, True, active)]
        for prev, x0 in new:
            assert torch.equal(prev, old[0]) and torch.equal(x0, old[1])
        assert torch.equal(old[0][1], xm[1])


def test_census_keys_of_the_eta_launches(ops):
    u, t, x, z = operands4((2, 256), "f16", 191)
    a_t, a_p = schedule_alphas()[1]
    ops.start_census()
    ops.cfg_ddim_step(u[0], t[0], GS, x[0], a_t, a_p, False, "v_prediction", 0.5, z[0])
    ops.cfg_ddim_step_masked(u, t, GS, x, a_t, a_p, [1, 0], True, "sample", 1.0, z)
    assert sorted(ops.stop_census()) == [("cfg_ddim_step_eta", 1, 0, 256, 0, 1, False, "torch.float16"),
                                         ("cfg_ddim_step_eta_masked", 2, 0, 256, 0, 2, True, "torch.float16")]


# ===================================================================================== the masked form
@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("n", [256, 1027])
@pytest.mark.parametrize("S", [1, 2, 3, 5])
@pytest.mark.parametrize("kind", TYPES)
def test_masked_step_matches_the_single_image_launch(ops, kind, S, n, dt):
    """n = 256: every image is one block; 1027: the image boundaries fall inside a block.  Alternating flags; the noise slice of
    every inactive image is NaN."""
    u, t, x, z0 = operands4((S, n), dt, 201 + S)
    eta = 1.0 if S % 2 else 0.5
    for first_on in (1, 0):
        flags = [int(s % 2 != first_on) for s in range(S)]
        active = torch.tensor(flags, dtype=torch.int32, device="cuda")
        z = z0.clone()
        for s in range(S):
            if not flags[s]:
                z[s] = float("nan")
        for a_t, a_p in schedule_alphas():
            with bounds(ops, u, t, x, z, active) as g:
                prev, x0 = ops.cfg_ddim_step_masked(u, t, GS, x, a_t, a_p, active, True, kind, eta, z)
                prev2, none = ops.cfg_ddim_step_masked(u, t, GS, x, a_t, a_p, active, False, kind, eta, z)
                g.assert_written(prev, "prev")
                g.assert_written(x0, "x0")
                g.assert_written(prev2, "prev, no x0")
            assert none is None and torch.equal(prev, prev2)
            _, x0_r = table64(kind, f64(u), f64(t), f64(x), a_t, a_p)
            for s in range(S):
                if not flags[s]:
                    assert torch.equal(prev[s], x[s]), s
                    close(x0[s], x0_r[s], TOL[dt], f"{kind} x0 of the inactive image {s}")
                    continue
                p1, x01 = ops.cfg_ddim_step(u[s], t[s], GS, x[s], a_t, a_p, True, kind, eta, z[s])
                assert torch.equal(prev[s], p1) and torch.equal(x0[s], x01), (s, a_t)


# ===================================================================================== the pipeline against the patched oracle
def variance_list(zseed, count, shape=(1, 4, 32, 32)):
    g = torch.Generator().manual_seed(zseed)
    return [torch.randn(shape, generator=g) for _ in range(count)]


def eta_ddim_step(kind, eta, noises):
    """A stand-in for oracle.pipeline.ddim_step (same signature): the stochastic step for a `kind` prediction; each call pops the
    next tensor of (a copy of) `noises`."""
    src = list(noises)

    def ddim_step(m, t, x, acp, steps, num_train=1000):
        prev = t - num_train // steps
        a_t = float(acp[t])
        a_prev = float(acp[prev]) if prev >= 0 else float(acp[0])
        sa, s1 = a_t ** 0.5, (1 - a_t) ** 0.5
        if kind == "epsilon":
            x0, eps = (x - s1 * m) / sa, m
        elif kind == "v_prediction":
            x0, eps = sa * x - s1 * m, sa * m + s1 * x
        else:
            x0, eps = m, (x - sa * m) / s1
        sigma, c_dir = coefficients(a_t, a_prev, eta)
        return a_prev ** 0.5 * x0 + c_dir * eps + sigma * src.pop(0)
    return ddim_step


_ORACLE = {}


def eta_oracle_run(monkeypatch, kind, width, seed=0, zseed=1, eta=1.0, case="no_recurse_thr2"):
    """One CPU fp32 oracle run with the stochastic DDIM step: -> (setup, meta, image latents, image re-noise, variance noise,
    final latents, call counters, smallest relative margin of a threshold comparison).  Cached per case."""
    import oracle.pipeline as opipe
    from oracle import loss as oloss
    key = (kind, width, seed, zseed, eta, case)
    if key in _ORACLE:
        return _ORACLE[key]
    meta = meta4() if case == "no_recurse_thr2" else [m for m in G9 if m["name"] == case][0]
    setup = (wide_setup if width == "wide" else g9_setup)(meta)
    unet, embeds, lat0, noise, thr = setup
    (lat,), (nz,) = _per_image(meta, lat0, noise, (seed,))
    zs = variance_list(zseed, 4 * meta["steps"])
    margins = []
    orig = oloss.meets_threshold

    def recording(i, thresholds, sums):
        if not ((i not in thresholds and i != -1) or len(thresholds) == 0):
            thr_i = list(thresholds.values())[-1] if i == -1 else thresholds[i]
            margins.extend(abs(float(v) - thr_i) / thr_i for v in sums.values())
        return orig(i, thresholds, sums)
    with monkeypatch.context() as mp:
        mp.setattr(opipe, "ddim_step", eta_ddim_step(kind, eta, zs))
        mp.setattr(oloss, "meets_threshold", recording)
        smp = opipe.GuidedSampler(copy.deepcopy(unet), oloss.TokenPlan(BASE_ENTRIES, meta["hyper"]), thresholds=thr,
                                  only_update_on_threshold_steps=meta["only_update_on_threshold_steps"],
                                  max_iter_to_alter=meta["max_iter_to_alter"], steps=meta["steps"],
                                  scale_factor=meta["scale_factor"])
        ref = smp.sample(lat, embeds, nz)
    _ORACLE[key] = (setup, meta, lat, nz, zs, ref, dict(smp.calls), min(margins))
    return _ORACLE[key]


def call_eta(pipe, meta, embeds, thr, S=1, capture="loss-only", flags=None, **keywords):
    """test_pipeline_gpu.run_product / test_seeds_per_pass_gpu._call with the call's own keywords (latents / generator,
    renoise_noise, eta, variance_noise) passed through."""
    from guided_attention_amd import ops, run
    from guided_attention_amd.config import RunConfig
    from guided_attention_amd.utils import helpers, ptp_utils, shared_state as state
    cfg = RunConfig(meta_prompt=PROMPT, output_path="/tmp/ga_test_out")
    cfg.only_update_on_threshold_steps = meta["only_update_on_threshold_steps"]
    cfg.stable = pipe
    state.curHyperParams = dict(state.hyperParameterOverrides, **meta["hyper"], thresholds=thr)
    run.overrideConfig(cfg)
    run.parseMetaPrompt(cfg)
    assert sorted(cfg.token_dict) == [2, 5, 6]
    helpers.log_clear()
    controller = ptp_utils.AttentionStore(capture=capture)
    ptp_utils.register_attention_control(pipe, controller)
    for k, v in (flags or {}).items():
        setattr(pipe, k, v)
    ops.start_census()
    try:
        out = pipe(prompt=None, prompt_embeds=embeds[1:2].cuda(), negative_prompt_embeds=embeds[0:1].cuda(),
                   attention_store=controller, attention_res=16, guidance_scale=7.5, num_inference_steps=meta["steps"],
                   max_iter_to_alter=meta["max_iter_to_alter"], thresholds=cfg.thresholds, scale_factor=meta["scale_factor"],
                   output_type="latent", num_images_per_prompt=S, **keywords)
    finally:
        census = ops.stop_census()
    out.census = {}
    for key, n in census.items():      # launches per entry point
        out.census[key[0]] = out.census.get(key[0], 0) + n
    return out


def clones(tensors):
    return [t.clone() for t in tensors]


DDIM_KEYS = ("cfg_ddim_step", "cfg_ddim_step_pred", "cfg_ddim_step_masked", "cfg_ddim_step_pred_masked", "cfg_ddim_step_eta",
             "cfg_ddim_step_eta_masked")


def ddim_census(out):
    return {k: out.census[k] for k in DDIM_KEYS if k in out.census}


@pytest.mark.parametrize("kind", ["epsilon", "v_prediction"])
def test_fp32_pipeline_vs_oracle(monkeypatch, kind):
    """Solo, eager, fp32 on the g9 UNet, eta = 1.  5e-3 of the latent maximum: the fp32 bar of the existing tests on this UNet.  A
    product that ignored eta or the noise would be 0.31 .. 0.37 (epsilon) / 0.80 .. 0.83 (v) away.  Measured on the MI355X:
    3.9e-6 (epsilon), 1.8e-5 (v)."""
    (unet, embeds, lat0, noise, thr), meta, lat, nz, zs, ref, calls, margin = eta_oracle_run(monkeypatch, kind, "g9")
    assert margin >= 0.05, margin      # a condition on the inputs: no threshold comparison that rounding could flip
    pipe = product(unet, torch.float32, kind)
    out = call_eta(pipe, meta, embeds, thr, latents=lat.clone(), renoise_noise=clones(nz), eta=1.0, variance_noise=clones(zs))
    assert {k: out.unet_calls[k] for k in MAIN} == {k: calls[k] for k in MAIN}
    assert ddim_census(out) == {"cfg_ddim_step_eta": calls["fwd_b2"]}
    assert out.variance_draws == calls["fwd_b2"] == 4
    err = _rel(out.latents, ref)
    print(f"[measured] fp32 pipeline {kind} eta=1: latents max-rel {err:.3e}, oracle margin {margin:.3e}, calls {calls}")
    assert err < 5e-3, err


def test_fp32_recurse_rounds_vs_oracle(monkeypatch):
    """G9's default_like case (6 steps, 3 recurse rounds: 8 CFG steps, so more variance draws than timesteps), fp32, solo, epsilon,
    eta = 1.  The oracle's smallest threshold margin with this noise is 0.026 (asserted >= 0.02); the existing fp32 test holds the
    same case at eta = 0, where the margin is 0.004, to the same 5e-3: fp32 does not need the 0.05 of the 16-bit tests."""
    (unet, embeds, lat0, noise, thr), meta, lat, nz, zs, ref, calls, margin = eta_oracle_run(monkeypatch, "epsilon", "g9",
                                                                                           case="default_like")
    assert margin >= 0.02, margin
    pipe = product(unet, torch.float32, "epsilon")
    out = call_eta(pipe, meta, embeds, thr, latents=lat.clone(), renoise_noise=clones(nz), eta=1.0, variance_noise=clones(zs))
    assert {k: out.unet_calls[k] for k in MAIN} == {k: calls[k] for k in MAIN}
    assert out.variance_draws == calls["fwd_b2"] == 8 and meta["steps"] == 6
    assert ddim_census(out) == {"cfg_ddim_step_eta": 8}
    err = _rel(out.latents, ref)
    print(f"[measured] fp32 recurse pipeline eta=1: latents max-rel {err:.3e}, oracle margin {margin:.3e}, calls {calls}")
    assert err < 5e-3, err


def test_f16_graphs_joint_pass_vs_oracle(monkeypatch):
    """v-prediction at eta = 1 on the benched launch path: f16, hipGraph replay, the batch-3 joint pass, the package's own
    convolution and Linear kernels (wide_setup), at the project's f16 bar for this path (1.25e-2).  The eta = 0 run of the same
    product is measured next to it.  Measured on the MI355X (the [measured] line), two runs: 1.02e-2 and 9.3e-3 at eta = 1, 7.4e-3 and
    7.7e-3 at eta = 0 (the f16 run is not bit-reproducible from run to run: the library's stride-2 convolution backward in the
    guidance steps; the replays themselves repeat); the two oracle runs are 0.94 apart.  Later runs of the
    unchanged test: 1.31e-2 at eta = 1 (over the bar) and 8.7e-3 at eta = 0.  With torch.backends.cudnn.deterministic = True the
    run repeats and gives 1.650e-2 / 8.64e-3, twice: the figure is one draw of the rounding of ~60 f16 layers over 5 steps, and
    the bar lies inside the spread of those draws (9.3e-3 ... 1.65e-2), so this test passes or fails with the library's choice of
    kernel, not with the package's code."""
    (unet, embeds, lat0, noise, thr), meta, lat, nz, zs, ref, calls, margin = eta_oracle_run(monkeypatch, "v_prediction", "wide")
    assert margin >= 0.05, margin
    pipe = product(unet, torch.float16, "v_prediction")
    flags = dict(use_graphs=True, batch_loss_only_guidance=True)
    out = call_eta(pipe, meta, embeds, thr, flags=flags, latents=lat.clone(), renoise_noise=clones(nz), eta=1.0,
                   variance_noise=clones(zs))
    assert {k: out.unet_calls[k] for k in MAIN} == {k: calls[k] for k in MAIN}
    assert out.unet_calls["joint_b3"] > 0 and pipe._runner is not None and pipe._runner.joint
    assert ddim_census(out) == {"cfg_ddim_step_eta": calls["fwd_b2"]}
    assert out.variance_draws == calls["fwd_b2"]
    err = _rel(out.latents, ref)
    _, _, _, _, ref0, calls0, margin0 = oracle_run(monkeypatch, "v_prediction", "wide")
    out0 = call_eta(pipe, meta, embeds, thr, flags=flags, latents=lat.clone(), renoise_noise=clones(nz))
    assert ddim_census(out0) == {"cfg_ddim_step_pred": calls0["fwd_b2"]} and out0.variance_draws == 0
    err0 = _rel(out0.latents, ref0)
    print(f"[measured] f16 graphs pipeline v_prediction: eta=1 latents max-rel {err:.3e} (oracle margin {margin:.3e}), "
          f"eta=0 {err0:.3e} (margin {margin0:.3e}); the two oracle runs differ by {_rel(ref, ref0):.3e}")
    assert err < 1.25e-2, err


def test_three_images_fp32(monkeypatch):
    """num_images_per_prompt = 3 at eta = 1, epsilon: per image the oracle's counters and as many variance draws as CFG steps, and
    latents within 5e-3 of the oracle and of the image's solo call.  The image with seed 54 takes another branch than the other
    two, so the masked step runs with idle slots, whose noise slices are zeros and consume nothing."""
    runs = [eta_oracle_run(monkeypatch, "epsilon", "g9", seed, 100 + seed) for seed in FP32_SEEDS]
    assert min(r[7] for r in runs) >= 0.05, [r[7] for r in runs]
    (unet, embeds, _, _, thr), meta = runs[0][0], runs[0][1]
    lats, noises, zss = [r[2] for r in runs], [r[3] for r in runs], [r[4] for r in runs]
    pipe = product(unet, torch.float32, "epsilon")
    S = len(runs)
    solo = [call_eta(pipe, meta, embeds, thr, latents=lats[s].clone(), renoise_noise=clones(noises[s]), eta=1.0,
                     variance_noise=clones(zss[s])) for s in range(S)]
    out = call_eta(pipe, meta, embeds, thr, S, latents=torch.cat(lats).clone(), renoise_noise=[clones(n) for n in noises],
                   eta=1.0, variance_noise=[clones(z) for z in zss])
    assert set(ddim_census(out)) == {"cfg_ddim_step_eta_masked"} and out.census["cfg_ddim_step_eta_masked"] > 0
    per_image = out.unet_calls_per_image
    assert any(c != per_image[0] for c in per_image), per_image       # different branches: idle slots in the masked launches
    assert out.batched_passes["idle_slots"] > 0
    for s, r in enumerate(runs):
        ref, calls = r[5], r[6]
        assert {k: per_image[s][k] for k in calls} == calls, s
        assert out.variance_draws[s] == calls["fwd_b2"] == solo[s].variance_draws
        assert ddim_census(solo[s]) == {"cfg_ddim_step_eta": calls["fwd_b2"]}
        e_oracle, e_solo = _rel(out.latents[s], ref[0]), _rel(out.latents[s], solo[s].latents[0])
        print(f"[measured] batched eta=1 image {s}: vs oracle {e_oracle:.3e}, vs solo {e_solo:.3e}, margin {r[7]:.3e}")
        assert e_oracle < 5e-3 and e_solo < 5e-3, (s, e_oracle, e_solo)


def test_a_short_variance_list_names_the_image_and_the_step():
    meta = meta4()
    unet, embeds, lat0, noise, thr = g9_setup(meta)
    pipe = product(unet, torch.float32, "epsilon")
    with pytest.raises(ValueError, match="image 0, CFG step 2"):
        call_eta(pipe, meta, embeds, thr, latents=lat0.clone(), renoise_noise=clones(noise), eta=1.0,
                 variance_noise=variance_list(5, 2))


def test_noise_drawn_from_the_call_generator():
    """Without `variance_noise` every CFG step draws from the call's generator, the one the latents came from: a call that is
    handed the latents and the noise list pre-drawn from a twin generator agrees within the run-to-run band of
    test_an_epsilon_run_is_untouched (2e-4)."""
    meta = meta4()
    unet, embeds, lat0, noise, thr = g9_setup(meta)
    pipe = product(unet, torch.float32, "epsilon")
    drawn = call_eta(pipe, meta, embeds, thr, generator=torch.Generator().manual_seed(77), renoise_noise=clones(noise), eta=1.0)
    twin = torch.Generator().manual_seed(77)
    lat = torch.randn(lat0.shape, generator=twin)
    zs = [torch.randn(lat0.shape, generator=twin) for _ in range(drawn.variance_draws)]
    handed = call_eta(pipe, meta, embeds, thr, latents=lat, renoise_noise=clones(noise), eta=1.0, variance_noise=zs)
    assert drawn.variance_draws == handed.variance_draws == drawn.unet_calls["fwd_b2"] > 0
    assert drawn.unet_calls == handed.unet_calls
    assert ddim_census(drawn) == ddim_census(handed) == {"cfg_ddim_step_eta": drawn.unet_calls["fwd_b2"]}
    err = _rel(drawn.latents, handed.latents)
    print(f"[measured] generator-drawn against pre-drawn noise: {err:.3e}")
    assert err < 2e-4, err
    plain = call_eta(pipe, meta, embeds, thr, latents=lat, renoise_noise=clones(noise))      # and eta does something
    assert _rel(handed.latents, plain.latents) > 0.1
