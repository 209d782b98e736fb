"""S images guided in one batched call (num_images_per_prompt > 1) on the MI355X: the batched / masked entry points against
the single-image ones on each image's slice, and the batched pipeline against solo calls on each image's inputs."""
import re

import pytest
import torch

from test_oracle_loop import G9, g9_setup
from test_pipeline_gpu import build_product

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
ENTRIES = [{"index": 2, "kind": "BOX", "geom": (.6, .3, .4, .55), "subprompt": "robot"},
           {"index": 5, "kind": "BOX", "geom": (.2, .3, .4, .55), "subprompt": "blue vase"},
           {"index": 6, "kind": "BOX", "geom": (.2, .3, .4, .55), "subprompt": "blue vase"}]
SHAPES = {"sd15_16": (16, (8, 8, 8, 8, 8)), "sd21_24": (24, (5, 10, 10, 20))}   # res, heads per image of each stored map


def _plan():
    from guided_attention_amd import ops
    from guided_attention_amd.utils import shared_state as state
    return ops.LossPlan(ENTRIES, dict(state.hyperParameterOverrides))


def _maps(S, res, heads, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.softmax(torch.randn(S * h, res * res, 77, generator=g) * 3, -1).to("cuda", dtype) for h in heads]


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("S", [1, 2, 3, 5])
def test_batched_loss_is_bit_identical_per_image(S, dt, shape):
    from guided_attention_amd import ops
    res, heads = SHAPES[shape]
    plan = _plan()
    maps = _maps(S, res, heads, DTYPES[dt], 10 * S + res)
    A, terms, loss = ops.aggregate_loss_fwd_batched(maps, S, res, 1, 76, plan)
    dloss = torch.tensor([0.0 if s % 2 else 1.5 + s for s in range(S)], device="cuda")
    dA, dPb = ops.smooth_loss_bwd_batched(A, res, 1, 76, plan, dloss, bcast_dtype=DTYPES[dt], bcast_scale=1 / sum(heads))
    for s in range(S):
        own = [m.reshape(S, -1, *m.shape[1:])[s] for m in maps]
        A1, t1, l1 = ops.aggregate_loss_fwd(own, res, 1, 76, plan)
        assert torch.equal(A[s], A1) and torch.equal(terms[s], t1) and torch.equal(loss[s:s + 1], l1)
        if dloss[s] == 0:
            assert not dA[s].any() and not dPb[s].any() and not torch.signbit(dA[s]).any()
            continue
        d1, p1 = ops.smooth_loss_bwd(A1, res, 1, 76, plan, dloss[s:s + 1], bcast_dtype=DTYPES[dt],
                                     bcast_scale=1 / sum(heads))
        assert torch.equal(dA[s], d1) and torch.equal(dPb[s], p1)
    assert ops.tickets_are_zero()


def test_batched_loss_and_gradient_vs_fp64():
    """The batched loss and dA at one shape against a float64 restatement (autograd through the oracle loss), at the bounds the
    solo kernels are held to (test_smooth_loss_other_resolutions): 5e-5 of the loss and of the gradient's maximum."""
    from guided_attention_amd import ops
    from oracle import loss as oloss
    from guided_attention_amd.utils import shared_state as state
    S, res, heads = 3, 16, (8, 8, 8, 8, 8)
    plan = _plan()
    maps = _maps(S, res, heads, torch.float32, 7)
    A, _, loss = ops.aggregate_loss_fwd_batched(maps, S, res, 1, 76, plan)
    dA, _ = ops.smooth_loss_bwd_batched(A, res, 1, 76, plan, torch.ones(S, device="cuda"))
    tp = oloss.TokenPlan(ENTRIES, dict(state.hyperParameterOverrides))
    for s in range(S):
        A64 = torch.cat([m.reshape(S, -1, *m.shape[1:])[s].double().cpu() for m in maps]).mean(0)
        A64 = A64.reshape(res, res, 77).requires_grad_(True)
        r = oloss.loss_torch(A64, tp)
        (g64,) = torch.autograd.grad(r["loss"], [A64])
        assert abs(loss[s].item() - r["loss"].item()) <= 5e-5 * abs(r["loss"].item())
        g64 = g64.reshape(res * res, 77)
        assert (dA[s].double().cpu() - g64).abs().max() <= 5e-5 * g64.abs().max()


CAPTURE = {"sd15_16": (8, 256, 40), "sd21_24_h5": (5, 576, 64), "sd21_24_h10": (10, 576, 64), "sd21_24_h20": (20, 576, 64)}


@pytest.mark.parametrize("shape", sorted(CAPTURE))
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("S", [1, 2, 3, 5])
def test_capture_backward_takes_one_map_per_image(S, dt, shape):
    from guided_attention_amd import ops
    torch.manual_seed(S)
    (H, N, D), Kt = CAPTURE[shape], 77
    dtype = DTYPES[dt]
    q = torch.randn(S, N, H * D, device="cuda", dtype=dtype)
    k = torch.randn(S, Kt, H * D, device="cuda", dtype=dtype)
    v = torch.randn(S, Kt, H * D, device="cuda", dtype=dtype)
    d_o = torch.randn_like(q)
    g = (torch.randn(S, N, Kt, device="cuda") * 1e-2).to(dtype)
    dense = g.unsqueeze(1).expand(S, H, N, Kt).reshape(S * H, N, Kt).contiguous()
    ref = ops.attn_capture_bwd(q, k, v, d_o, dense, H, D ** -0.5)
    ops._image_broadcasts.clear()
    ops._image_broadcasts[g.data_ptr()] = [S, N * Kt, g, 1]
    got = ops.attn_capture_bwd(q, k, v, d_o, g[0].unsqueeze(0).expand(S * H, N, Kt), H, D ** -0.5)
    ops.end_image_broadcasts()          # the one view was consumed through the table
    assert torch.equal(got, ref)


@pytest.mark.parametrize("side", [64, 96], ids=["sd15_512", "sd21_768"])
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("S", [1, 2, 3, 5])
def test_masked_latent_ops_match_the_single_image_launches(S, dt, side):
    from guided_attention_amd import ops
    torch.manual_seed(100 + S)
    dtype = DTYPES[dt]
    x, g, y, eu, et = (torch.randn(S, 4, side, side, device="cuda").to(dtype) for _ in range(5))
    active = [int(s % 2 == 0) for s in range(S)]
    steps = [20.0 * (s + 1) / 3 for s in range(S)]
    out, absmean = ops.latent_axpy_batched(x, g, steps, active, True)
    rn = ops.latent_axpby_masked(x, y, 0.9, 0.43, active)
    prev, x0 = ops.cfg_ddim_step_masked(eu, et, 7.5, x, 0.6, 0.7, active, True)
    for s in range(S):
        if not active[s]:
            assert torch.equal(out[s], x[s]) and torch.equal(rn[s], x[s]) and torch.equal(prev[s], x[s])
            continue
        o1, a1 = ops.latent_axpy(x[s:s + 1], g[s:s + 1], steps[s], True)
        assert torch.equal(out[s:s + 1], o1) and torch.equal(absmean[s:s + 1], a1)
        assert torch.equal(rn[s:s + 1], ops.latent_axpby(x[s:s + 1], y[s:s + 1], 0.9, 0.43))
        p1, x01 = ops.cfg_ddim_step(eu[s:s + 1], et[s:s + 1], 7.5, x[s:s + 1], 0.6, 0.7, True)
        assert torch.equal(prev[s:s + 1], p1) and torch.equal(x0[s:s + 1], x01)


# ------------------------------------------------------------------------------------------------ the batched pipeline
def _mask_numbers(lines):
    return [re.sub(r"-?\d+(\.\d+)?(e-?\d+)?", "#", ln) for ln in lines]


def _call(pipe, meta, embeds, lats, noises, thr, S):
    from guided_attention_amd import ops, run
    from guided_attention_amd.config import RunConfig
    from guided_attention_amd.utils import helpers, ptp_utils, shared_state as state
    cfg = RunConfig(meta_prompt="a [robot:.6,.3,.4,.55] and a [blue vase:.2,.3,.4,.55]", output_path="/tmp/ga_test_out")
    cfg.only_update_on_threshold_steps = meta["only_update_on_threshold_steps"]
    cfg.stable = pipe
    state.curHyperParams = dict(state.hyperParameterOverrides, **meta["hyper"], thresholds=thr)
    run.overrideConfig(cfg)
    run.parseMetaPrompt(cfg)
    helpers.log_clear()
    controller = ptp_utils.AttentionStore(capture="loss-only")
    ptp_utils.register_attention_control(pipe, controller)
    ops.start_census()
    out = pipe(prompt=None, prompt_embeds=embeds[1:2].cuda(), negative_prompt_embeds=embeds[0:1].cuda(),
               attention_store=controller, attention_res=16, guidance_scale=7.5, num_inference_steps=meta["steps"],
               max_iter_to_alter=meta["max_iter_to_alter"], thresholds=cfg.thresholds, scale_factor=meta["scale_factor"],
               latents=torch.cat(lats).clone(), renoise_noise=[[n.clone() for n in ns] for ns in noises] if S > 1 else
               [n.clone() for n in noises[0]], output_type="latent", num_images_per_prompt=S)
    out.census = {}
    for key, n in ops.stop_census().items():
        out.census[key[0]] = out.census.get(key[0], 0) + n
    return out, list(helpers.lines)


def _per_image(meta, lat0, noise, seeds):
    """Image inputs by seed: seed 0 is the fixture's own latents and re-noise, any other seed draws both from a generator."""
    lats, noises = [], []
    for seed in seeds:
        if seed == 0:
            lats.append(lat0)
            noises.append(noise)
        else:
            g = torch.Generator().manual_seed(seed)
            lats.append(torch.randn(lat0.shape, generator=g))
            noises.append([torch.randn(lat0.shape, generator=g) for _ in range(len(noise))])
    return lats, noises


# Per-image inputs (seeds of _per_image) on the no_recurse_thr2 fixture, 4 steps, picked so that the images take different
# branches — image 1 meets a threshold in fewer refinement iterations (23 guidance evaluations against 26) — while every
# threshold comparison of the oracle clears its threshold by >= 5 % (asserted below), so rounding cannot flip a branch.
FP32_SEEDS = (8, 54, 3)       # g9 widths
F16_SEEDS = (8, 40, 7)        # wide_setup widths: f16 runs the package's own convolution and Linear kernels
_ORACLE = {}


def _oracle(width, seeds):
    """CPU fp32 oracle per image: (setup, final latents, call counters, smallest relative threshold margin) per seed."""
    import copy
    import oracle.pipeline as opipe
    from oracle import loss as oloss
    from oracle.pipeline import GuidedSampler
    from test_oracle_loop import BASE_ENTRIES
    from test_pipeline_gpu import wide_setup
    key = (width, seeds)
    if key in _ORACLE:
        return _ORACLE[key]
    meta = dict([m for m in G9 if m["name"] == "no_recurse_thr2"][0], steps=4)
    unet, embeds, lat0, noise, thr = (wide_setup if width == "wide" else g9_setup)(meta)
    lats, noises = _per_image(meta, lat0, noise, seeds)
    margins = []
    orig = oloss.meets_threshold

    def recording(i, thresholds, sums):
        if not ((i not in thresholds and i != -1) or len(thresholds) == 0):
            t = list(thresholds.values())[-1] if i == -1 else thresholds[i]
            margins.extend(abs(float(v) - t) / t for v in sums.values())
        return orig(i, thresholds, sums)
    runs = []
    opipe.oloss.meets_threshold = recording
    try:
        for lat, nz in zip(lats, noises):
            margins.clear()
            smp = GuidedSampler(copy.deepcopy(unet), oloss.TokenPlan(BASE_ENTRIES, meta["hyper"]), thresholds=thr,
                                only_update_on_threshold_steps=meta["only_update_on_threshold_steps"],
                                max_iter_to_alter=meta["max_iter_to_alter"], steps=meta["steps"],
                                scale_factor=meta["scale_factor"])
            runs.append((smp.sample(lat, embeds, nz), dict(smp.calls), min(margins)))
    finally:
        opipe.oloss.meets_threshold = orig
    _ORACLE[key] = (meta, unet, embeds, lats, noises, thr, runs)
    return _ORACLE[key]


def _check_batched_against_solo(out, solo, S):
    assert out.latents.shape[0] == S and len(out.logs) == S and len(out.unet_calls_per_image) == S
    for s, (o1, lines1) in enumerate(solo):
        assert out.unet_calls_per_image[s] == o1.unet_calls, s
        assert _mask_numbers(out.logs[s]) == _mask_numbers(lines1), s
    assert out.unet_calls == {k: sum(c[k] for c in out.unet_calls_per_image) for k in out.unet_calls}
    calls = out.unet_calls_per_image
    assert any(c != calls[0] for c in calls), calls            # the images take different branches
    bp = out.batched_passes
    evals = sum(c["fwd_b1_grad"] + c["bwd"] + c["fwd_b2"] - c["joint_b3"] for c in calls)
    assert bp["idle_slots"] == S * (bp["eval"] + bp["bwd"] + bp["cfg"] + bp["joint"]) - evals
    assert bp["idle_slots"] > 0, bp


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graphs"])
def test_three_images_fp32_match_oracle_and_solo_calls(graphs):
    import copy
    meta, unet, embeds, lats, noises, thr, runs = _oracle("g9", FP32_SEEDS)
    assert min(r[2] for r in runs) >= 0.05, [r[2] for r in runs]
    pipe = build_product(copy.deepcopy(unet), torch.float32)
    pipe.use_graphs = graphs
    S = len(lats)
    solo = [_call(pipe, meta, embeds, [lats[s]], [noises[s]], thr, 1) for s in range(S)]
    out, _ = _call(pipe, meta, embeds, lats, noises, thr, S)
    _check_batched_against_solo(out, solo, S)
    for s, (ref, calls, _) in enumerate(runs):
        mine = out.unet_calls_per_image[s]
        assert {k: mine[k] for k in calls} == calls, s          # the oracle's counters for image s run alone
        assert _rel(out.latents[s], ref[0]) < 5e-3, s
        assert _rel(out.latents[s], solo[s][0].latents[0]) < 5e-3, s
    if graphs:
        assert out.batched_passes["joint"] > 0


def test_three_images_f16_graphs_joint_pass_own_kernels():
    import copy
    meta, unet, embeds, lats, noises, thr, runs = _oracle("wide", F16_SEEDS)
    assert min(r[2] for r in runs) >= 0.05, [r[2] for r in runs]
    pipe = build_product(copy.deepcopy(unet), torch.float16)
    pipe.use_graphs = True
    pipe.batch_loss_only_guidance = True
    S = len(lats)
    solo = [_call(pipe, meta, embeds, [lats[s]], [noises[s]], thr, 1) for s in range(S)]
    out, _ = _call(pipe, meta, embeds, lats, noises, thr, S)
    _check_batched_against_solo(out, solo, S)
    assert out.batched_passes["joint"] > 0 and pipe._runner.images == S and pipe._runner.joint
    assert out.census.get("linear", 0) > 0 and out.census.get("conv3x3", 0) > 0   # own kernels at batch S, 2S, 3S
    errs = []
    for s, (ref, calls, _) in enumerate(runs):
        mine = out.unet_calls_per_image[s]
        assert {k: mine[k] for k in calls} == calls, s
        e_oracle, e_solo = _rel(out.latents[s], ref[0]), _rel(out.latents[s], solo[s][0].latents[0])
        errs.append((e_oracle, e_solo))
        assert e_oracle < 1.25e-2, (s, e_oracle)
        assert e_solo < SOLO_F16_BOUND, (s, e_solo)
    print("[measured] f16 batched vs oracle / vs solo f16:", errs)


# batched f16 against the solo f16 call of the same image (different batch, different kernel plans): measured on the MI355X
# 5.0e-3 / 7.0e-3 / 6.7e-3 (vs the oracle 5.3e-3 / 5.5e-3 / 5.4e-3); the bound is 2.2x the largest
SOLO_F16_BOUND = 1.5e-2


def test_execute_two_seeds_per_pass_matches_one(tmp_path):
    """run.execute with seeds_per_pass = 2 on 3 seeds (random-init tiny model, f16, hipGraphs): chunks [2, 1], per-seed files
    written, latents within the f16 band of a seeds_per_pass = 1 run."""
    from guided_attention_amd import run
    from guided_attention_amd.config import RunConfig
    from guided_attention_amd.pipeline_guided_attention import GuidedAttention
    from guided_attention_amd.unet import UNetConfig
    from guided_attention_amd.utils import shared_state as state
    pipe = GuidedAttention.from_pretrained("random", random_init=True, unet_config=UNetConfig.tiny(32, 48), seed=5)
    pipe.to("cuda", torch.float16)
    pipe.use_graphs = True
    results = {}
    for per_pass in (1, 2):
        out_dir = tmp_path / f"spp{per_pass}"
        cfg = RunConfig(meta_prompt="a [robot:.6,.3,.4,.55] and a [blue vase:.2,.3,.4,.55]", seeds=[3, 4, 5],
                        n_inference_steps=3, output_path=out_dir, seeds_per_pass=per_pass)
        cfg.stable = pipe
        state.config = cfg
        state.hyperParameterIterations = [{}]
        run.execute(cfg)
        results[per_pass] = [t.float() for t in state.last_results["latents"]]
        folder = out_dir / "a _robot__6,_3,_4,_55_ and a _blue vase__2,_3,_4,_55_"
        assert len(list(folder.glob("*.png"))) == 3 and len(list(folder.glob("*.txt"))) == 3
    for a, b in zip(results[1], results[2]):
        assert a.shape == b.shape == (1, 4, 32, 32)
        assert _rel(b, a) < 1.25e-2
