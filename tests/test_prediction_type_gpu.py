"""v-prediction and sample-prediction checkpoints on the MI355X: ga_cfg_ddim_step_pred / _pred_masked against fp64 and against
each other, the epsilon path against the launch it has always been, and the pipeline (solo eager, hipGraphs with the joint
pass, batched) against the CPU oracle whose DDIM step is replaced, for the test's duration, by the table of include/ga_hip.h:

    m = u + g * (t - u);   sa = sqrt(alpha), s1 = sqrt(1 - alpha)
    epsilon       x0 = (x - s1_t m) / sa_t     eps = m
    v_prediction  x0 = sa_t x - s1_t m         eps = sa_t m + s1_t x
    sample        x0 = m                       eps = (x - sa_t m) / s1_t
    prev = sa_p x0 + s1_p eps

Kernel tolerances are the project's TOL table (f32 2e-5, f16 2e-3, bf16 1.6e-2 of max |ref|, what test_latent_ops holds the
epsilon step to); the alphas are those of the real 50-step schedule at t = 981, 501 and 1."""
import copy
import math

import numpy as np
import pytest
import torch

import hashrand
from test_kernels_gpu import DT, TOL, close, dev
from test_oracle_loop import BASE_ENTRIES, G9, g9_setup
from test_output_bounds_gpu import bounds
from test_pipeline_gpu import build_product, run_product, wide_setup
from test_seeds_per_pass_gpu import FP32_SEEDS, _call, _per_image, _rel

pytestmark = pytest.mark.gpu

ALL = ["f32", "f16", "bf16"]
TYPES = ["epsilon", "v_prediction", "sample"]
CODE = {"epsilon": 0, "v_prediction": 1, "sample": 2}
GS = 7.5
TWO_TRIPS = 2048 * 256 + 5     # grid_for caps the grid at 2048 blocks of 256: the smallest n whose grid-stride loop goes round twice


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from guided_attention_amd import ops as _ops
    _ops.load()
    _ops.prepare_device("cuda")
    return _ops


def schedule_alphas():
    from guided_attention_amd.scheduler import DDIMScheduler
    sch = DDIMScheduler()
    sch.set_timesteps(50)
    return [sch.alphas_for(t) for t in (981, 501, 1)]


def table64(kind, u, t, x, a_t, a_p, gs=GS):
    """(prev, x0) of the table above in fp64 numpy."""
    m = u + gs * (t - u)
    sa, s1 = math.sqrt(a_t), math.sqrt(1 - a_t)
    if kind == "epsilon":
        x0, eps = (x - s1 * m) / sa, m
    elif kind == "v_prediction":
        x0, eps = sa * x - s1 * m, sa * m + s1 * x
    else:
        x0, eps = m, (x - sa * m) / s1
    return math.sqrt(a_p) * x0 + math.sqrt(1 - a_p) * eps, x0


def f64(t):
    return t.detach().double().cpu().numpy()


def operands(shape, dt, seed):
    return tuple(dev(hashrand.normalish(shape, seed + k), DT[dt]) for k in range(3))


# ===================================================================================== the kernels against fp64
@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("n", [1, 7, 1000, 1027])
@pytest.mark.parametrize("kind", TYPES)
def test_step_vs_fp64(ops, kind, n, dt):
    """n = 1: one thread; 7: a partial wave; 1000: three whole blocks and a partial one; 1027: an odd count behind whole blocks."""
    u, t, x = operands((n,), dt, 31)
    for a_t, a_p in schedule_alphas():
        prev_r, x0_r = table64(kind, f64(u), f64(t), f64(x), a_t, a_p)
        with bounds(ops, u, t, x) as g:
            prev, x0 = ops.cfg_ddim_step(u, t, GS, x, a_t, a_p, True, kind)
            prev2, none = ops.cfg_ddim_step(u, t, GS, x, a_t, a_p, False, kind)
            for out, what in ((prev, "prev"), (x0, "x0"), (prev2, "prev, no x0")):
                g.assert_written(out, what)
        assert none is None and torch.equal(prev, prev2)
        close(prev, prev_r, TOL[dt], f"{kind} prev a_t={a_t:.4f}")
        close(x0, x0_r, TOL[dt], f"{kind} x0 a_t={a_t:.4f}")


@pytest.mark.parametrize("kind", TYPES)
def test_step_second_trip_of_the_grid_stride_loop(ops, kind):
    u, t, x = operands((TWO_TRIPS,), "f16", 41)
    a_t, a_p = schedule_alphas()[1]
    prev_r, x0_r = table64(kind, f64(u), f64(t), f64(x), a_t, a_p)
    with bounds(ops, u, t, x) as g:
        prev, x0 = ops.cfg_ddim_step(u, t, GS, x, a_t, a_p, True, kind)
        g.assert_written(prev, "prev")
        g.assert_written(x0, "x0")
    close(prev, prev_r, TOL["f16"], f"{kind} prev")
    close(x0, x0_r, TOL["f16"], f"{kind} x0")
    close(prev[-300:], prev_r[-300:], TOL["f16"], f"{kind} prev, the second trip")   # the 5 elements of the second trip and their block


# ===================================================================================== epsilon is the launch it has always been
def _direct(ops, u, t, x, a_t, a_p, want_x0, active=None):
    """ga_cfg_ddim_step_pred[_masked] with prediction = GA_PRED_EPSILON, called on the binding itself."""
    prev = torch.empty_like(x)
    x0 = torch.empty_like(x) if want_x0 else None
    lib, p = ops.load(), ops._ptr
    if active is None:
        ops.check(lib.ga_cfg_ddim_step_pred(p(u), p(t), GS, p(x), a_t, a_p, 0, p(prev), p(x0), x.numel(), ops.dtype_code(x),
                                            ops.stream_ptr()), "ga_cfg_ddim_step_pred")
    else:
        S = x.shape[0]
        ops.check(lib.ga_cfg_ddim_step_pred_masked(p(u), p(t), GS, p(x), a_t, a_p, 0, p(active), p(prev), p(x0), S,
                                                   x.numel() // S, ops.dtype_code(x), ops.stream_ptr()),
                  "ga_cfg_ddim_step_pred_masked")
    return prev, x0


@pytest.mark.parametrize("n,dt", [(n, dt) for n in (1, 7, 1000, 1027) for dt in ALL] + [(TWO_TRIPS, "f16")])
def test_epsilon_is_the_old_launch(ops, n, dt):
    u, t, x = operands((n,), dt, 51)
    S = 3
    um, tm, xm = operands((S, n), dt, 61) if n != TWO_TRIPS else (None,) * 3
    active = torch.tensor([1, 0, 1], dtype=torch.int32, device="cuda")
    for a_t, a_p in schedule_alphas():
        old_prev, old_x0 = ops.cfg_ddim_step(u, t, GS, x, a_t, a_p, True)
        ops.start_census()
        new_prev, new_x0 = ops.cfg_ddim_step(u, t, GS, x, a_t, a_p, True, prediction="epsilon")
        assert [k[0] for k in ops.stop_census()] == ["cfg_ddim_step"]
        d_prev, d_x0 = _direct(ops, u, t, x, a_t, a_p, True)
        assert torch.equal(new_prev, old_prev) and torch.equal(new_x0, old_x0)
        assert torch.equal(d_prev, old_prev) and torch.equal(d_x0, old_x0)
        if um is None:
            continue
        old_prev, old_x0 = ops.cfg_ddim_step_masked(um, tm, GS, xm, a_t, a_p, active, True)
        new_prev, new_x0 = ops.cfg_ddim_step_masked(um, tm, GS, xm, a_t, a_p, active, True, prediction="epsilon")
        d_prev, d_x0 = _direct(ops, um, tm, xm, a_t, a_p, True, active)
        assert torch.equal(new_prev, old_prev) and torch.equal(new_x0, old_x0)
        assert torch.equal(d_prev, old_prev) and torch.equal(d_x0, old_x0)
        assert torch.equal(old_prev[1], xm[1])


# ===================================================================================== the masked form
@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("n", [256, 1027])
@pytest.mark.parametrize("S", [1, 2, 3, 5])
@pytest.mark.parametrize("kind", ["v_prediction", "sample"])
def test_masked_step_matches_the_single_image_launch(ops, kind, S, n, dt):
    """n = 256: every image is one block; 1027: the image boundaries fall inside a block.  Alternating flags."""
    u, t, x = operands((S, n), dt, 71 + S)
    for first_on in (1, 0):
        flags = [int(s % 2 != first_on) for s in range(S)]
        active = torch.tensor(flags, dtype=torch.int32, device="cuda")
        for a_t, a_p in schedule_alphas():
            with bounds(ops, u, t, x, active) as g:
                prev, x0 = ops.cfg_ddim_step_masked(u, t, GS, x, a_t, a_p, active, True, kind)
                prev2, none = ops.cfg_ddim_step_masked(u, t, GS, x, a_t, a_p, active, False, kind)
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
                p1, x01 = ops.cfg_ddim_step(u[s], t[s], GS, x[s], a_t, a_p, True, kind)
                assert torch.equal(prev[s], p1) and torch.equal(x0[s], x01), (s, a_t)


# ===================================================================================== the pipeline against the patched oracle
def meta4():
    return dict([m for m in G9 if m["name"] == "no_recurse_thr2"][0], steps=4)


def table_ddim_step(kind):
    """A stand-in for oracle.pipeline.ddim_step (same signature) that reads its first argument as a `kind` prediction."""
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
        return a_prev ** 0.5 * x0 + (1 - a_prev) ** 0.5 * eps
    return ddim_step


_ORACLE = {}


def oracle_run(monkeypatch, kind, width, seed=0):
    """One CPU fp32 oracle run of the 4-step no_recurse_thr2 case with the DDIM step of `kind`: -> (setup, meta, image latents,
    image re-noise, final latents, call counters, smallest relative margin of a threshold comparison).  Cached per case."""
    import oracle.pipeline as opipe
    from oracle import loss as oloss
    key = (kind, width, seed)
    if key in _ORACLE:
        return _ORACLE[key]
    meta = meta4()
    setup = (wide_setup if width == "wide" else g9_setup)(meta)
    unet, embeds, lat0, noise, thr = setup
    (lat,), (nz,) = _per_image(meta, lat0, noise, (seed,))
    margins = []
    orig = oloss.meets_threshold

    def recording(i, thresholds, sums):
        if not ((i not in thresholds and i != -1) or len(thresholds) == 0):
            thr_i = list(thresholds.values())[-1] if i == -1 else thresholds[i]
            margins.extend(abs(float(v) - thr_i) / thr_i for v in sums.values())
        return orig(i, thresholds, sums)
    with monkeypatch.context() as mp:
        mp.setattr(opipe, "ddim_step", table_ddim_step(kind))
        mp.setattr(oloss, "meets_threshold", recording)
        smp = opipe.GuidedSampler(copy.deepcopy(unet), oloss.TokenPlan(BASE_ENTRIES, meta["hyper"]), thresholds=thr,
                                  only_update_on_threshold_steps=meta["only_update_on_threshold_steps"],
                                  max_iter_to_alter=meta["max_iter_to_alter"], steps=meta["steps"],
                                  scale_factor=meta["scale_factor"])
        ref = smp.sample(lat, embeds, nz)
    _ORACLE[key] = (setup, meta, lat, nz, ref, dict(smp.calls), min(margins))
    return _ORACLE[key]


def product(unet, dtype, kind):
    from guided_attention_amd.scheduler import DDIMScheduler
    pipe = build_product(copy.deepcopy(unet), dtype)
    pipe.scheduler = DDIMScheduler(prediction_type=kind)
    return pipe


MAIN = ("fwd_b1_grad", "bwd", "fwd_b2")


@pytest.mark.parametrize("kind", ["v_prediction", "sample"])
def test_fp32_pipeline_vs_oracle(monkeypatch, kind):
    """Solo, eager, fp32 on the g9 UNet.  5e-3 of the latent maximum: the bound of test_fp32_pipeline_matches_reference_call and
    of the batched fp32 tests on this UNet.  With the epsilon formula applied to these model outputs the error is near 0.8."""
    (unet, embeds, lat0, noise, thr), meta, _, _, ref, calls, margin = oracle_run(monkeypatch, kind, "g9")
    assert margin >= 0.05, margin      # a condition on the inputs: no threshold comparison that rounding could flip
    pipe = product(unet, torch.float32, kind)
    out, _ = run_product(pipe, meta, embeds, lat0, noise, thr)
    assert {k: out.unet_calls[k] for k in MAIN} == {k: calls[k] for k in MAIN}
    assert out.census.get("cfg_ddim_step_pred", 0) == calls["fwd_b2"] and "cfg_ddim_step" not in out.census
    err = _rel(out.latents, ref)
    print(f"[measured] fp32 pipeline {kind}: latents max-rel {err:.3e}, oracle margin {margin:.3e}, calls {calls}")
    assert err < 5e-3, err


def test_f16_graphs_joint_pass_vs_oracle(monkeypatch):
    """v-prediction on the benched launch path: f16, hipGraph replay, the batch-3 joint pass, the package's own convolution and
    Linear kernels (wide_setup), at the f16 bound of test_half_precision_pipeline_vs_oracle (1.25e-2; epsilon measured 4.6e-3
    there).  Measured on the MI355X (the [measured] line): 7.1e-3."""
    (unet, embeds, lat0, noise, thr), meta, _, _, ref, calls, margin = oracle_run(monkeypatch, "v_prediction", "wide")
    assert margin >= 0.05, margin
    pipe = product(unet, torch.float16, "v_prediction")
    out, _ = run_product(pipe, meta, embeds, lat0, noise, thr, use_graphs=True, batch_loss_only_guidance=True)
    assert {k: out.unet_calls[k] for k in MAIN} == {k: calls[k] for k in MAIN}
    assert out.unet_calls["joint_b3"] > 0 and pipe._runner is not None and pipe._runner.joint
    assert out.census.get("cfg_ddim_step_pred", 0) == calls["fwd_b2"] and "cfg_ddim_step" not in out.census
    err = _rel(out.latents, ref)
    print(f"[measured] f16 graphs pipeline v_prediction: latents max-rel {err:.3e}, oracle margin {margin:.3e}")
    assert err < 1.25e-2, err


def test_three_images_fp32_v_prediction(monkeypatch):
    """num_images_per_prompt = 3 under v-prediction: per image the oracle's counters, and latents within 5e-3 of the oracle and
    of the solo v-prediction call.  The images take different branches, so the masked step runs with idle slots."""
    runs = [oracle_run(monkeypatch, "v_prediction", "g9", seed) for seed in FP32_SEEDS]
    assert min(r[6] for r in runs) >= 0.05, [r[6] for r in runs]
    (unet, embeds, _, _, thr), meta = runs[0][0], runs[0][1]
    lats, noises = [r[2] for r in runs], [r[3] for r in runs]
    pipe = product(unet, torch.float32, "v_prediction")
    S = len(runs)
    solo = [_call(pipe, meta, embeds, [lats[s]], [noises[s]], thr, 1)[0] for s in range(S)]
    out, _ = _call(pipe, meta, embeds, lats, noises, thr, S)
    assert out.census.get("cfg_ddim_step_pred_masked", 0) > 0
    assert "cfg_ddim_step_masked" not in out.census and "cfg_ddim_step" not in out.census
    per_image = out.unet_calls_per_image
    assert any(c != per_image[0] for c in per_image), per_image       # different branches: idle slots in the masked launches
    assert out.batched_passes["idle_slots"] > 0
    for s, r in enumerate(runs):
        ref, calls = r[4], r[5]
        assert {k: per_image[s][k] for k in calls} == calls, s
        assert solo[s].census.get("cfg_ddim_step_pred", 0) == calls["fwd_b2"]
        e_oracle, e_solo = _rel(out.latents[s], ref[0]), _rel(out.latents[s], solo[s].latents[0])
        print(f"[measured] batched v_prediction image {s}: vs oracle {e_oracle:.3e}, vs solo {e_solo:.3e}, margin {r[6]:.3e}")
        assert e_oracle < 5e-3 and e_solo < 5e-3, (s, e_oracle, e_solo)


def test_an_epsilon_run_is_untouched():
    """The default scheduler: the old launch and only it, and the run-to-run band of test_variants_are_result_identical."""
    meta = meta4()
    unet, embeds, lat0, noise, thr = g9_setup(meta)
    pipe = build_product(unet, torch.float32)
    assert pipe.scheduler.config.prediction_type == "epsilon"
    base, _ = run_product(pipe, meta, embeds, lat0, noise, thr)
    again, _ = run_product(pipe, meta, embeds, lat0, noise, thr)
    for out in (base, again):
        assert out.census.get("cfg_ddim_step", 0) == out.unet_calls["fwd_b2"] > 0
        assert "cfg_ddim_step_pred" not in out.census
    err = _rel(again.latents, base.latents)
    assert err < 2e-4, err
