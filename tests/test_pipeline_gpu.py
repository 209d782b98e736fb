"""End-to-end parity on the GPU: the product pipeline (HIP kernels, reference-style API) against
  * the reference's own `__call__` output (tests/golden/g9_loop.*), and
  * the CPU oracle loop on identical weights / latents / noise,
for a reduced-width UNet of the real topology.  Needs an MI355X (`pytest -m gpu`)."""
import numpy as np
import pytest
import torch

from types import SimpleNamespace

import hashrand
from conftest import load_json, load_npz
from oracle import loss as oloss
from oracle.pipeline import GuidedSampler
from test_oracle_loop import BASE_ENTRIES, G9, g9_setup

pytestmark = pytest.mark.gpu


def build_product(unet, dtype):
    from guided_attention_amd.pipeline_guided_attention import GuidedAttention
    from guided_attention_amd.text import SyntheticTextEncoder, WordTokenizer
    pipe = GuidedAttention(unet, None, None, SyntheticTextEncoder(48), WordTokenizer())
    return pipe.to("cuda", dtype)


def run_product(pipe, meta, embeds, lat0, noise, thr, capture="loss-only", **flags):
    from types import SimpleNamespace
    from guided_attention_amd.config import RunConfig
    from guided_attention_amd.utils import helpers, ptp_utils, shared_state as state
    cfg = RunConfig(meta_prompt="a [robot:.6,.3,.4,.55] and a [blue vase:.2,.3,.4,.55]", output_path="/tmp/ga_test_out")
    cfg.only_update_on_threshold_steps = meta["only_update_on_threshold_steps"]
    cfg.stable = pipe
    state.curHyperParams = dict(state.hyperParameterOverrides, **meta["hyper"], thresholds=thr)
    from guided_attention_amd import run
    run.overrideConfig(cfg)
    run.parseMetaPrompt(cfg)
    assert sorted(cfg.token_dict) == [2, 5, 6]
    helpers.log_clear()
    controller = ptp_utils.AttentionStore(capture=capture)
    ptp_utils.register_attention_control(pipe, controller)
    for k, v in flags.items():
        setattr(pipe, k, v)
    from guided_attention_amd import ops
    ops.start_census()
    out = pipe(prompt=None, prompt_embeds=embeds[1:2].cuda(), negative_prompt_embeds=embeds[0:1].cuda(),
               attention_store=controller, attention_res=16, guidance_scale=7.5, num_inference_steps=meta["steps"],
               max_iter_to_alter=meta["max_iter_to_alter"], thresholds=cfg.thresholds, scale_factor=meta["scale_factor"],
               latents=lat0.clone(), renoise_noise=[n.clone() for n in noise], output_type="latent")
    out.census = {}
    for key, n in ops.stop_census().items():      # launches per entry point of this image
        out.census[key[0]] = out.census.get(key[0], 0) + n
    out.lines = list(helpers.lines)
    return out, controller


def _mask_numbers(lines):
    from test_seeds_per_pass_gpu import _mask_numbers as mask
    return mask(lines)


@pytest.mark.parametrize("meta", G9, ids=lambda m: m["name"])
def test_fp32_pipeline_matches_reference_call(meta):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    g = load_npz("g9_loop.npz")
    unet, embeds, lat0, noise, thr = g9_setup(meta)
    pipe = build_product(unet, torch.float32)
    out, _ = run_product(pipe, meta, embeds, lat0, noise, thr)
    assert (out.unet_calls["fwd_b1_grad"], out.unet_calls["bwd"], out.unet_calls["fwd_b2"]) == \
        (meta["fwd_b1"], meta["bwd"], meta["fwd_b2"])
    ref = g[f"{meta['name']}.final_latents"]
    err = np.abs(out.latents.float().cpu().numpy() - ref).max() / np.abs(ref).max()
    assert err < 5e-3, err  # fp32 GPU vs fp32 CPU through up to 41 forward + 33 backward UNet passes


MAIN_CALLS = ("fwd_b1_grad", "bwd", "fwd_b2", "loss_evals")


@pytest.mark.parametrize("variant", ["rerun", "reference-capture", "truncated", "skip-unused", "graphs", "graphs-truncated",
                                     "graphs-two-pass", "two-launch-loss", "graphs-two-launch-loss", "graphs-no-run-ahead"])
def test_variants_are_result_identical(variant):
    """capture='reference', the truncated guidance forward and the skipped log-only guidance passes must
    not change the latents.  This fp32 model runs its convolutions and GEMMs on the library, whose backward kernels do not all
    repeat bit for bit (located for f16: the stride-2 backward-data kernel, DESIGN.md section 6 and test_reproducible_pass_gpu.py;
    the fp32 run was not traced), so the bar is the run-to-run band of an unchanged configuration ("rerun"), not bit equality."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    meta = G9[0]
    unet, embeds, lat0, noise, thr = g9_setup(meta)
    pipe = build_product(unet, torch.float32)
    base, _ = run_product(pipe, meta, embeds, lat0, noise, thr, guidance_forward="full", skip_unused_guidance=False)
    if variant == "rerun":
        out, _ = run_product(pipe, meta, embeds, lat0, noise, thr)
    elif variant == "reference-capture":
        out, ctrl = run_product(pipe, meta, embeds, lat0, noise, thr, capture="reference")
        # the last forward is the CFG pass: every map of this 32x32-latent UNet has <= 32^2 pixels and is kept
        assert {k: len(v) for k, v in ctrl.attention_store.items()} == \
            {"down_cross": 6, "mid_cross": 1, "up_cross": 9, "down_self": 6, "mid_self": 1, "up_self": 9}
        assert ctrl.attention_store["down_cross"][0].shape == (2 * 2, 1024, 77)
    elif variant == "truncated":
        out, _ = run_product(pipe, meta, embeds, lat0, noise, thr, guidance_forward="truncated")
    elif variant.endswith("two-launch-loss"):   # aggregate_attention and the loss as separate launches (base: fused)
        assert base.census.get("aggregate_loss_fwd", 0) > 0 and base.census.get("aggregate_maps", 0) == 0
        out, _ = run_product(pipe, meta, embeds, lat0, noise, thr, fused_aggregate_loss=False,
                             use_graphs=variant.startswith("graphs"))
        assert out.census.get("aggregate_loss_fwd", 0) == 0 and out.census.get("aggregate_maps", 0) > 0
        pipe.fused_aggregate_loss = True
    elif variant.startswith("graphs"):
        mode = "truncated" if variant.endswith("truncated") else "full"
        joint = not variant.endswith("two-pass")
        # default: the refinement loop enqueues backward / update / next evaluation before reading a loss table back;
        # "no-run-ahead": enqueue, read, decide, enqueue — same launches, same counters, same latents
        pipe.speculative_refinement = not variant.endswith("no-run-ahead")
        out, ctrl = run_product(pipe, meta, embeds, lat0, noise, thr, use_graphs=True, guidance_forward=mode,
                                batch_loss_only_guidance=joint)
        assert pipe.discarded_speculations == 0
        # every evaluation of the eager run is performed; with `joint`, the loss-only guidance forward and the CFG
        # pair of a step share one batch-3 pass
        assert {k: out.unet_calls[k] for k in MAIN_CALLS} == {k: base.unet_calls[k] for k in MAIN_CALLS}
        assert (out.unet_calls["joint_b3"] > 0) == joint and base.unet_calls["joint_b3"] == 0
        # after the run the store holds the maps of the last CFG evaluation (uncond + cond), however it was batched
        assert ctrl.attention_store["up_cross"][0].shape[0] == 2 * 2
        assert {k: len(v) for k, v in ctrl.attention_store.items() if v} == {"down_cross": 2, "up_cross": 3}
        out2, _ = run_product(pipe, meta, embeds, lat0, noise, thr, use_graphs=True, guidance_forward=mode,
                              batch_loss_only_guidance=joint)  # cached graphs
        err2 = (out.latents - out2.latents).abs().max().item() / out.latents.abs().max().item()
        assert err2 < 2e-4, err2  # a library backward kernel is not bit-reproducible run to run
        if variant in ("graphs", "graphs-no-run-ahead"):
            # the other way round the refinement loop — run-ahead against read-then-enqueue — on the same graphs: the same
            # log lines (numbers masked) and the same launches per entry point; no loss is exactly 0, nothing is discarded
            pipe.speculative_refinement = not pipe.speculative_refinement
            other, _ = run_product(pipe, meta, embeds, lat0, noise, thr, use_graphs=True, guidance_forward=mode,
                                   batch_loss_only_guidance=joint)
            assert pipe.discarded_speculations == 0
            assert _mask_numbers(other.lines) == _mask_numbers(out2.lines) and len(out2.lines) > 100
            assert other.census == out2.census      # both on cached graphs (`out` holds the warm-up launches of the capture)
    else:
        out, _ = run_product(pipe, meta, embeds, lat0, noise, thr, skip_unused_guidance=True)
        assert out.unet_calls["fwd_b1_grad"] < base.unet_calls["fwd_b1_grad"]
    pipe.guidance_forward, pipe.skip_unused_guidance, pipe.use_graphs, pipe.batch_loss_only_guidance = "full", False, False, True
    pipe.speculative_refinement = True
    assert out.unet_calls["bwd"] == base.unet_calls["bwd"] and out.unet_calls["fwd_b2"] == base.unet_calls["fwd_b2"]
    err = (out.latents - base.latents).abs().max().item() / base.latents.abs().max().item()
    assert err < 2e-4, err


def wide_setup(meta):
    """g9_setup with every level a multiple of 64 channels wide (64, 64, 128, 128): in the 16-bit dtypes every 3x3
    convolution and every transformer-block Linear then runs on the package's own kernels (ga_conv3x3_nhwc, ga_linear_fused) —
    with the g9 widths (32, ...) the first level falls back to the library and a fp16 run exercises less of the benched path."""
    from guided_attention_amd.unet import UNet2DConditionModel, UNetConfig
    from test_oracle_loop import hash_init_
    cfg = UNetConfig(sample_size=32, block_out_channels=(64, 64, 128, 128), attention_head_dim=2, cross_attention_dim=48)
    unet = hash_init_(UNet2DConditionModel(cfg), meta["unet_seed"]).float()
    for p in unet.parameters():
        p.requires_grad_(False)
    _, embeds, lat0, noise, thr = g9_setup(meta)
    return unet, embeds, lat0, noise, thr


# measured on the MI355X (the [measured] line): eager f16 5.7e-3 (rms 5.3e-3), bf16 4.8e-2 (rms 4.1e-2) in round 3; the graphs
# rows (round 4) are the path bench.py times — hipGraph replay, the batch-3 joint pass, own Linear / convolution kernels
_HALF_ORACLE = {}   # mode -> (setup, oracle latents, oracle call counters): one CPU oracle run (~28 s) serves both dtypes


@pytest.mark.parametrize("mode", ["eager", "graphs"])
@pytest.mark.parametrize("dt,tol", [("f16", 1.25e-2), ("bf16", 1.0e-1)])
def test_half_precision_pipeline_vs_oracle(dt, tol, mode):
    """The fast dtypes against the fp32 CPU oracle, case without threshold-driven branching near the limit
    (thresholds chosen so both sides take the same branches).  Stated tolerance: max |dlatent| / max |latent|.
    Measured (round 4, MI355X): f16 eager 5.0e-3 / graphs 4.6e-3, bf16 eager 4.6e-2 / graphs 3.6e-2 (rms within 10 % of max).
    "eager": the g9 UNet, two passes per step.  "graphs": `use_graphs=True` with the batch-3 joint pass of the loss-only steps
    on a UNet whose widths are multiples of 64, i.e. the benched launch path — hipGraph replay of g_eval / g_grad / g_cfg /
    g_joint on ga_linear_fused and ga_conv3x3_nhwc at every level (asserted from the launch census) — after 4 denoising steps
    with refinement at the first two.  Bounds 2 - 2.6x the measurement.
    Error budget: one UNet evaluation differs from fp32 by about 2^-11 (f16) / 2^-8 (bf16) per stored activation, ~3e-3 / 2e-2
    at the noise prediction after ~60 layers with f32 accumulation inside every kernel; the guidance update multiplies the latent
    gradient's error (a few %, in bf16) by scale_factor * sqrt(scale_range) and the DDIM recursion carries it on: the
    differences are common-mode (rms ~ max), not isolated spikes."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import copy
    meta = dict(G9[2], steps=4)
    if mode not in _HALF_ORACLE:
        setup = (wide_setup if mode == "graphs" else g9_setup)(meta)
        unet, embeds, lat0, noise, thr = setup
        product_unet = copy.deepcopy(unet)          # before the oracle installs its processors
        plan = oloss.TokenPlan(BASE_ENTRIES, meta["hyper"])
        smp = GuidedSampler(unet, plan, thresholds=thr, only_update_on_threshold_steps=meta["only_update_on_threshold_steps"],
                            max_iter_to_alter=meta["max_iter_to_alter"], steps=meta["steps"], scale_factor=meta["scale_factor"])
        _HALF_ORACLE[mode] = ((product_unet,) + setup[1:], smp.sample(lat0, embeds, noise).numpy(), dict(smp.calls))
    (unet, embeds, lat0, noise, thr), ref, calls = _HALF_ORACLE[mode]
    s = SimpleNamespace(calls=calls)
    pipe = build_product(copy.deepcopy(unet), {"f16": torch.float16, "bf16": torch.bfloat16}[dt])
    flags = dict(use_graphs=True, batch_loss_only_guidance=True) if mode == "graphs" else {}
    out, _ = run_product(pipe, meta, embeds, lat0, noise, thr, **flags)
    assert out.unet_calls["fwd_b1_grad"] == s.calls["fwd_b1_grad"] and out.unet_calls["bwd"] == s.calls["bwd"]
    assert out.unet_calls["fwd_b2"] == s.calls["fwd_b2"]
    if mode == "graphs":
        assert out.unet_calls["joint_b3"] > 0 and out.census.get("linear", 0) > 0 and out.census.get("conv3x3", 0) > 0
        assert pipe._runner is not None and pipe._runner.joint
    err = np.abs(out.latents.float().cpu().numpy() - ref).max() / np.abs(ref).max()
    rms = float(np.sqrt(np.mean((out.latents.float().cpu().numpy() - ref) ** 2)) / np.sqrt(np.mean(ref ** 2)))
    print(f"[measured] half-precision pipeline {dt} {mode}: latents max-rel {err:.3e} rms-rel {rms:.3e}")
    assert err < tol, err


def test_run_ahead_refinement_discards_an_update_enqueued_ahead_of_a_zero_loss(monkeypatch):
    """The refinement loop on the hipGraph runner enqueues backward_k, the update and eval_k+1 BEFORE it has read eval_k's loss
    table; the only fact it assumes is `loss != 0` (reference :551 — on a loss of exactly 0 the latents are not updated).  A
    zero loss is forced at the second refinement iteration of every refinement call: the run-ahead driver must drop the enqueued
    update and evaluation (they reach neither the latents nor the call counters nor the log) and evaluate the unchanged latents
    again, i.e. end with exactly the counters, log lines and latents of the driver that reads before it enqueues, and with its
    launches plus the dropped ones."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from guided_attention_amd.pipeline_guided_attention import GuidedAttention
    meta = G9[0]
    unet, embeds, lat0, noise, thr = g9_setup(meta)
    pipe = build_product(unet, torch.float32)
    seen = {"n": 0}

    def zero_at_second(losses_dict):
        from guided_attention_amd.utils import shared_state as state
        seen["n"] += 1
        return state.sub_iteration == 2
    monkeypatch.setattr(GuidedAttention, "_loss_is_zero", staticmethod(zero_at_second))
    pipe.speculative_refinement = False
    run_product(pipe, meta, embeds, lat0, noise, thr, use_graphs=True)   # captures the graphs; its census holds the warm-up launches
    base, _ = run_product(pipe, meta, embeds, lat0, noise, thr, use_graphs=True)
    pipe.speculative_refinement, pipe.discarded_speculations = True, 0
    out, _ = run_product(pipe, meta, embeds, lat0, noise, thr, use_graphs=True)
    assert pipe.discarded_speculations == 3 and seen["n"] > 40          # once per refinement call (3 recurse passes at step 0)
    assert base.unet_calls["bwd"] == meta["bwd"] - 3                     # the forced zero really skipped an update
    assert {k: out.unet_calls[k] for k in MAIN_CALLS} == {k: base.unet_calls[k] for k in MAIN_CALLS}
    err = (out.latents - base.latents).abs().max().item() / base.latents.abs().max().item()
    assert err < 2e-4, err
    # the same log lines, numbers masked: nothing of a discarded update is logged
    assert _mask_numbers(out.lines) == _mask_numbers(base.lines) and len(out.lines) > 100
    # the same launches per entry point — beyond what each of the 3 discarded speculations had enqueued when its loss was
    # read: one backward replay, one latent update, one evaluation replay
    expected = dict(base.census, latent_axpy=base.census["latent_axpy"] + 3)
    for replayed in (pipe._runner.launches["grad"], pipe._runner.launches["eval"]):
        for key, n in replayed.items():
            expected[key[0]] = expected.get(key[0], 0) + 3 * n
    assert out.census == expected


def test_attention_maps_match_oracle_fp16():
    """North-star wording: 'matching the reference CPU path's attention maps ... to a stated fp16 tolerance'.
    One guidance forward: the five stored 16x16 cross maps and their aggregate, HIP fp16 vs CPU fp32 oracle."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import copy
    from oracle import attention as oattn
    from oracle.pipeline import install_processors
    from guided_attention_amd.utils import ptp_utils, shared_state as state
    meta = G9[0]
    unet, embeds, lat0, _, _ = g9_setup(meta)
    gpu_unet = copy.deepcopy(unet)
    store = oattn.OracleStore()
    install_processors(unet, store)
    with torch.no_grad():
        unet(lat0, 981, encoder_hidden_states=embeds[1:2])
    A_ref = oattn.aggregate(store.attention_store, 16, ("up", "down", "mid"), True).numpy()
    pipe = build_product(gpu_unet, torch.float16)
    state.curHyperParams = dict(state.hyperParameterOverrides)
    ctrl = ptp_utils.AttentionStore()
    ptp_utils.register_attention_control(pipe, ctrl)
    with torch.no_grad():
        pipe.unet(lat0.cuda().half(), 981, encoder_hidden_states=embeds[1:2].cuda().half())
    assert {k: len(v) for k, v in ctrl.attention_store.items() if v} == {"down_cross": 2, "up_cross": 3}
    A = ptp_utils.aggregate_attention(ctrl, 16, ("up", "down", "mid"), True, 0).cpu().numpy()
    assert np.abs(A - A_ref).max() < 1e-2 * A_ref.max()  # whole UNet prefix in fp16 vs fp32
    for key in ("down_cross", "up_cross"):
        for got, ref in zip(ctrl.attention_store[key], [m for m in store.attention_store[key] if m.shape[1] == 256]):
            assert np.abs(got.float().cpu().numpy() - ref.numpy()).max() < 2e-2 * ref.numpy().max()


def test_cpu_pipeline_is_refused():
    from guided_attention_amd._lib import GaError
    from guided_attention_amd.pipeline_guided_attention import GuidedAttention
    from guided_attention_amd.unet import UNet2DConditionModel, UNetConfig
    from guided_attention_amd.utils import shared_state as state
    from guided_attention_amd.utils.ptp_utils import AttentionStore
    state.curHyperParams = dict(state.hyperParameterOverrides)
    pipe = GuidedAttention(UNet2DConditionModel(UNetConfig.tiny(32, 48)))
    with pytest.raises(GaError):
        pipe(prompt=None, prompt_embeds=torch.zeros(1, 77, 48), negative_prompt_embeds=torch.zeros(1, 77, 48),
             attention_store=AttentionStore(), latents=torch.zeros(1, 4, 32, 32), output_type="latent")


def test_graph_runner_follows_a_new_prompt_embedding():
    """The captured graphs read the cached text K/V projections: a new prompt embedding on a cached runner must
    refresh them (and an in-place edit of the embedding must invalidate the eager cache)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    meta = dict(G9[2], steps=3)
    unet, embeds, lat0, noise, thr = g9_setup(meta)
    pipe = build_product(unet, torch.float32)
    other = torch.from_numpy(hashrand.normalish((2, 77, 48), 4242))
    first, _ = run_product(pipe, meta, embeds, lat0, noise, thr, use_graphs=True)
    second, _ = run_product(pipe, meta, other, lat0, noise, thr, use_graphs=True)   # same runner, new prompt
    pipe.use_graphs = False
    eager_other, _ = run_product(pipe, meta, other, lat0, noise, thr)
    eager_first, _ = run_product(pipe, meta, embeds, lat0, noise, thr)

    def rel(a, b):
        return (a.latents - b.latents).abs().max().item() / b.latents.abs().max().item()

    assert rel(second, eager_other) < 2e-4 and rel(first, eager_first) < 2e-4
    assert rel(second, first) > 1e-2  # the prompt really changed the result


def test_custom_loss_plugin_against_reference_fixture():
    """`[CustomLoss:toLeftOf (cat, vase)]`: the plugin API (register_custom_loss / CustomLossBase / ToLeftOf) on the
    GPU against the reference's own ToLeftOf.calc_loss and its autograd gradient (tests/golden/g10)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from types import SimpleNamespace
    from guided_attention_amd import run
    from guided_attention_amd.config import RunConfig
    from guided_attention_amd.text import WordTokenizer
    from guided_attention_amd.utils import helpers, shared_state as state
    meta = load_json("g10_custom_loss.json")
    g = load_npz("g10_custom_loss.npz")
    cfg = RunConfig(meta_prompt=meta["meta_prompt"], output_path="/tmp/ga_test_out")
    cfg.stable = SimpleNamespace(tokenizer=WordTokenizer())
    state.config = cfg
    state.curHyperParams = dict(state.hyperParameterOverrides)
    run.register_custom_loss("toLeftOf", run.ToLeftOf())
    run.parseMetaPrompt(cfg)
    assert cfg.prompt == meta["prompt"] and list(cfg.custom_loss) == ["toLeftOf"] and cfg.custom_loss["toLeftOf"][1] == meta["args"]
    assert sorted(cfg.token_dict) == [2, 5]
    fn, args = cfg.custom_loss["toLeftOf"]
    for name in ("bos", "sharp"):
        A = torch.from_numpy(g[f"{name}.A"]).cuda().requires_grad_(True)
        text = torch.softmax(A[:, :, 1:-1] * 100, dim=-1)
        v = fn.calc_loss(text, args)
        np.testing.assert_allclose(v.detach().cpu().numpy(), g[f"{name}.loss"], rtol=2e-5, atol=1e-6)
        (gA,) = torch.autograd.grad(v.sum(), [A], allow_unused=True)
        ref = g[f"{name}.dA"]
        got = gA.cpu().numpy() if gA is not None else np.zeros_like(ref)
        assert np.abs(got - ref).max() <= 3e-5 * max(np.abs(ref).max(), 1e-12) + 1e-9


def test_pipeline_with_only_a_custom_loss():
    """A prompt whose annotated tokens are all KEYWORDs of a custom loss: the fused kernel has nothing to do, the
    plugin's loss alone drives the latent update (eager autograd path)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from guided_attention_amd import run
    from guided_attention_amd.config import RunConfig
    from guided_attention_amd.utils import helpers, ptp_utils, shared_state as state
    meta = dict(G9[2], steps=2)
    unet, embeds, lat0, noise, _ = g9_setup(meta)
    pipe = build_product(unet, torch.float32)
    cfg = RunConfig(meta_prompt="a [cat:.2,.5] and a [vase:.7,.5] [CustomLoss:toLeftOf (vase, cat)]", output_path="/tmp/ga_test_out")
    cfg.stable = pipe
    state.config = cfg
    state.curHyperParams = dict(state.hyperParameterOverrides, thresholds={0: 0.0}, recurse_steps=1)
    run.register_custom_loss("toLeftOf", run.ToLeftOf())
    run.overrideConfig(cfg)
    run.parseMetaPrompt(cfg)
    helpers.log_clear()
    ctrl = ptp_utils.AttentionStore()
    ptp_utils.register_attention_control(pipe, ctrl)
    out = pipe(prompt=None, prompt_embeds=embeds[1:2].cuda(), negative_prompt_embeds=embeds[0:1].cuda(),
               attention_store=ctrl, num_inference_steps=2, thresholds=cfg.thresholds, latents=lat0.clone(),
               renoise_noise=[n.clone() for n in noise], output_type="latent")
    assert out.unet_calls["bwd"] >= 1 and torch.isfinite(out.latents).all()
    plain, _ = run_product(pipe, dict(meta, hyper={"recurse_steps": 1}), embeds, lat0, noise, {0: 99.0})
    assert (out.latents - plain.latents).abs().max() > 1e-4  # the custom loss moved the latents


# measured on the MI355X (round 4, the [measured] line): f32 maps 1.6e-6, loss 7.9e-8, grad 2.0e-6, cosine 1.00000;
# f16 maps 1.6e-3, loss 5.7e-6, grad max-rel 5.7e-3, cosine 0.99993 — bounds <= 2.5x those, except the loss: its error is a
# cancellation residue (box masses of a 24x24 mean whose per-pixel errors average out), a random draw of that size: 4x
@pytest.mark.parametrize("dt,tol_maps,tol_loss,tol_grad", [("f32", 4e-6, 1e-6, 5e-6), ("f16", 4e-3, 2.5e-5, 1.4e-2)])
def test_sd21_768_shapes_one_guidance_step(dt, tol_maps, tol_loss, tol_grad):
    """BASELINE config 4 shapes (no reference oracle exists: the reference hard-codes 16): SD-2.1 layout
    (linear projections, per-level head counts with head_dim 64, EOT-normalised text slice), 768^2 -> latent 96^2,
    attention_res 24, three bounding boxes.  One guidance evaluation + latent gradient, HIP vs the CPU oracle — in fp32
    (library convolutions / GEMMs around the capture kernels) and in fp16, the configuration's own dtype: the 64 / 128-channel
    widths put every 3x3 convolution (96 / 48 / 24 / 12-wide maps: patch geometry 3) and every transformer Linear on the
    package's kernels (asserted from the census)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import copy
    from guided_attention_amd import ops
    from guided_attention_amd.pipeline_guided_attention import GuidedAttention
    from guided_attention_amd.unet import UNet2DConditionModel, UNetConfig
    from guided_attention_amd.utils import ptp_utils, shared_state as state
    from oracle import attention as oattn
    from oracle.pipeline import install_processors
    cfg = UNetConfig(sample_size=96, block_out_channels=(64, 64, 128, 128), attention_head_dim=(1, 1, 2, 2),
                     cross_attention_dim=64, use_linear_projection=True)
    unet = UNet2DConditionModel(cfg).init_weights_(seed=21).float()
    for p in unet.parameters():
        p.requires_grad_(False)
    embeds = torch.from_numpy(hashrand.normalish((1, 77, 64), 2101))
    lat = torch.from_numpy(hashrand.normalish((1, 4, 96, 96), 2102))
    entries = [{"index": 2, "kind": "BOX", "geom": (.6, .3, .4, .55), "subprompt": "robot"},
               {"index": 5, "kind": "BOX", "geom": (.2, .3, .4, .55), "subprompt": "blue vase"},
               {"index": 6, "kind": "BOX", "geom": (.2, .3, .4, .55), "subprompt": "blue vase"},
               {"index": 9, "kind": "BOX", "geom": (.35, .05, .35, .35), "subprompt": "moon"}]
    n_prompt_tokens = 11  # BOS + 9 words + first EOT -> text slice [1, 10)
    # oracle
    cpu_unet = copy.deepcopy(unet)
    store = oattn.OracleStore()
    install_processors(cpu_unet, store)
    lat_c = lat.clone().requires_grad_(True)
    cpu_unet(lat_c, 981, encoder_hidden_states=embeds)
    A_ref = oattn.aggregate(store.attention_store, 24, ("up", "down", "mid"), True)
    r = oloss.loss_torch(A_ref, oloss.TokenPlan(entries), normalize_eot=True, n_prompt_tokens=n_prompt_tokens)
    (g_ref,) = torch.autograd.grad(r["loss"], [lat_c])
    # product
    dtype = {"f32": torch.float32, "f16": torch.float16}[dt]
    pipe = GuidedAttention(unet).to("cuda", dtype)
    state.curHyperParams = dict(state.hyperParameterOverrides)
    ctrl = ptp_utils.AttentionStore(attention_res=24)
    ptp_utils.register_attention_control(pipe, ctrl)
    lat_g = lat.cuda().to(dtype).requires_grad_(True)
    with ops.census_scope() as cs:
        pipe.unet(lat_g, 981, encoder_hidden_states=embeds.cuda().to(dtype))
        assert {k: len(v) for k, v in ctrl.attention_store.items() if v} == {"down_cross": 2, "up_cross": 3}
        assert ctrl.attention_store["up_cross"][0].shape == (2, 576, 77)
        A = ptp_utils.aggregate_attention(ctrl, 24, ("up", "down", "mid"), True, 0)
        plan = ops.LossPlan(entries, state.curHyperParams)
        terms, loss = ops.SmoothLoss.apply(A.reshape(576, 77), 24, 1, n_prompt_tokens - 1, plan)
        (g_hip,) = torch.autograd.grad(loss, [lat_g])
    kinds = {k[0] for k in cs.launches}
    assert ("conv3x3" in kinds and "linear" in kinds) == (dt == "f16"), kinds     # fp16: own kernels; fp32: the library
    e_maps = np.abs(A.detach().cpu().numpy() - A_ref.detach().numpy()).max() / A_ref.max().item()
    e_loss = abs(loss.item() - float(r["loss"])) / abs(float(r["loss"]))
    err = (g_hip.float().cpu() - g_ref).abs().max().item() / g_ref.abs().max().item()
    cos = float((g_hip.float().cpu() * g_ref).sum() / (g_hip.float().cpu().norm() * g_ref.norm()))
    print(f"[measured] sd21 768 shapes {dt}: maps {e_maps:.3e} loss {e_loss:.3e} grad max-rel {err:.3e} cosine {cos:.5f}")
    assert e_maps < tol_maps and e_loss < tol_loss, (e_maps, e_loss)
    np.testing.assert_allclose(terms[:, 5].cpu().numpy(), [float(v) for v in r["token_loss"]], rtol=2e-4 if dt == "f32" else 2e-2,
                               atol=1e-6 if dt == "f32" else 1e-4)
    assert err < tol_grad and cos > (0.99999 if dt == "f32" else 0.9995), (err, cos)


def test_execute_reuses_graphs_across_seeds_and_survives_eager_images(tmp_path):
    """`run.execute` (the reference's entry point) builds a fresh token_dict per (seed, hyper-parameter state): the
    content-keyed loss plan must let both seeds replay ONE set of captured hipGraphs.  Eager images with other prompts
    in between must not disturb the text K/V tensors the graphs read (they are pinned in the per-layer cache)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from guided_attention_amd import run
    from guided_attention_amd.config import RunConfig
    from guided_attention_amd.graphs import GraphRunner
    from guided_attention_amd.pipeline_guided_attention import GuidedAttention
    from guided_attention_amd.utils import shared_state as state
    from guided_attention_amd.unet import UNetConfig
    pipe = GuidedAttention.from_pretrained("random", random_init=True, unet_config=UNetConfig.tiny(32, 48), seed=5)
    pipe.to("cuda", torch.float32)
    pipe.use_graphs = True
    cfg = RunConfig(meta_prompt="a [robot:.6,.3,.4,.55] and a [blue vase:.2,.3,.4,.55]", seeds=[3, 4],
                    n_inference_steps=3, output_path=tmp_path)
    cfg.stable = pipe
    state.config = cfg
    state.hyperParameterIterations = [{}]
    before = GraphRunner.captures
    run.execute(cfg)
    assert GraphRunner.captures == before + 1          # two seeds, one capture
    first = [t.clone() for t in state.last_results["latents"]]
    assert len(first) == 2 and (first[0] - first[1]).abs().max() > 1e-3
    runner = next(iter(pipe._graph_cache.values()))
    assert runner.pinned > 0
    # eager, unguided images with several other prompts (each adds contexts to every layer's K/V cache)
    for k in range(4):
        cfg2 = RunConfig(meta_prompt=f"plain prompt number {k} with no annotations at all", seeds=[9],
                         n_inference_steps=1, output_path=tmp_path, run_standard_sd=True)
        cfg2.stable = pipe
        state.config = cfg2
        run.execute(cfg2, save=False)
    state.config = cfg
    run.execute(cfg, save=False)
    assert GraphRunner.captures == before + 1          # still the same graphs
    for a, b in zip(first, state.last_results["latents"]):
        assert (a - b).abs().max().item() < 2e-4 * a.abs().max().item()
    assert (tmp_path / "a _robot__6,_3,_4,_55_ and a _blue vase__2,_3,_4,_55_" / "3_strict_False_inside_loss_scale_0.2"
            "_outside_loss_scale_0.2_shrink_factor_0.15_thresholds__0_1.0_use_optimizer_False_recurse_until_14"
            "_recurse_steps_3.png").exists()


def test_strict_mode_pipeline_vs_oracle():
    """curHyperParams['strict'] = True through the whole product path (fused kernel fwd + bwd, UNet backward, latent
    update), fp32, against the CPU oracle loop with the same hyper-parameters."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    meta = dict(G9[2], steps=2, hyper=dict(G9[2]["hyper"], strict=True))
    thr = {0: 0.05}   # strict losses are ~0.1-0.3: forces refinement at step 0
    unet, embeds, lat0, noise, _ = g9_setup(meta)
    plan = oloss.TokenPlan(BASE_ENTRIES, meta["hyper"])
    s = GuidedSampler(unet, plan, thresholds=thr, only_update_on_threshold_steps=meta["only_update_on_threshold_steps"],
                      max_iter_to_alter=meta["max_iter_to_alter"], steps=meta["steps"], scale_factor=meta["scale_factor"])
    ref = s.sample(lat0, embeds, noise).numpy()
    import copy
    pipe = build_product(copy.deepcopy(unet), torch.float32)
    out, _ = run_product(pipe, meta, embeds, lat0, noise, thr)
    assert s.calls["bwd"] >= 1
    assert (out.unet_calls["fwd_b1_grad"], out.unet_calls["bwd"]) == (s.calls["fwd_b1_grad"], s.calls["bwd"])
    err = np.abs(out.latents.float().cpu().numpy() - ref).max() / np.abs(ref).max()
    assert err < 5e-3, err


# measured on the MI355X (round 3, the [measured] line): f32 maps 6.8e-7, grad 4.4e-6, cosine 1.00000; bf16 maps 1.4e-2,
# loss 6.6e-5, grad max-rel 4.2e-2, cosine 0.99918 — the bf16 bounds are 2 - 2.4x that (round 2 carried 4e-2 / 3.5e-1 / 0.97)
@pytest.mark.parametrize("dt,tol_maps,tol_grad", [("f32", 1e-5, 5e-5), ("bf16", 3e-2, 1e-1)])
def test_sdxl_layout_one_guidance_step(dt, tol_maps, tol_grad):
    """BASELINE config 5 layout (no reference oracle exists: diffusers 0.12.1 predates SDXL): 3 levels, no attention on
    the top level, 2 / 3 transformer blocks per attention below (SDXL: 2 / 10), per-level head counts, linear
    projections, text_time added conditioning, attention_res = latent / 4, two guided tokens.  One guidance evaluation
    + latent gradient, HIP vs the CPU oracle on the same module."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import copy
    from guided_attention_amd import ops
    from guided_attention_amd.pipeline_guided_attention import GuidedAttention
    from guided_attention_amd.unet import UNet2DConditionModel, UNetConfig
    from guided_attention_amd.utils import ptp_utils, shared_state as state
    from oracle import attention as oattn
    from oracle.pipeline import install_processors
    cfg = UNetConfig.tiny_sdxl(sample_size=32, cross_attention_dim=64)
    unet = UNet2DConditionModel(cfg).init_weights_(seed=31).float()
    for p in unet.parameters():
        p.requires_grad_(False)
    pooled = torch.from_numpy(hashrand.normalish((2, 40), 3100))
    time_ids = torch.tensor([[256., 256., 0., 0., 256., 256.]] * 2)
    embeds = torch.from_numpy(hashrand.normalish((1, 77, 64), 3101))
    lat = torch.from_numpy(hashrand.normalish((1, 4, 32, 32), 3102))
    entries = [{"index": 2, "kind": "BOX", "geom": (.6, .3, .4, .55), "subprompt": "robot"},
               {"index": 6, "kind": "BOX", "geom": (.2, .3, .4, .55), "subprompt": "vase"}]
    res = 8
    cpu_unet = copy.deepcopy(unet)
    cpu_unet.set_added_cond(pooled, time_ids)
    store = oattn.OracleStore()
    install_processors(cpu_unet, store)
    assert store.num_att_layers == 2 * (2 * 2 + 2 * 3 + 3 + 3 * 3 + 3 * 2)   # self + cross per transformer block
    lat_c = lat.clone().requires_grad_(True)
    cpu_unet(lat_c, 981, encoder_hidden_states=embeds)
    A_ref = oattn.aggregate(store.attention_store, res, ("up", "down", "mid"), True)
    r = oloss.loss_torch(A_ref, oloss.TokenPlan(entries))
    (g_ref,) = torch.autograd.grad(r["loss"], [lat_c])
    dtype = {"f32": torch.float32, "bf16": torch.bfloat16}[dt]
    pipe = GuidedAttention(unet).to("cuda", dtype)
    pipe.unet.set_added_cond(pooled, time_ids)
    state.curHyperParams = dict(state.hyperParameterOverrides)
    ctrl = ptp_utils.AttentionStore(attention_res=res)
    ptp_utils.register_attention_control(pipe, ctrl)
    lat_g = lat.cuda().to(dtype).requires_grad_(True)
    pipe.unet(lat_g, 981, encoder_hidden_states=embeds.cuda().to(dtype))
    # the 8x8 level holds down_blocks.2 (2 x 3), the mid block (3) and up_blocks.0 (3 x 3) cross maps
    assert {k: len(v) for k, v in ctrl.attention_store.items() if v} == {"down_cross": 6, "mid_cross": 3, "up_cross": 9}
    A = ptp_utils.aggregate_attention(ctrl, res, ("up", "down", "mid"), True, 0)
    plan = ops.LossPlan(entries, state.curHyperParams)
    terms, loss = ops.SmoothLoss.apply(A.reshape(res * res, 77), res, 1, 76, plan)
    (g_hip,) = torch.autograd.grad(loss, [lat_g])
    assert np.abs(A.detach().cpu().numpy() - A_ref.detach().numpy()).max() < tol_maps * A_ref.max().item()
    np.testing.assert_allclose(loss.item(), float(r["loss"]), rtol=1e-5 if dt == "f32" else 2e-3)
    err = (g_hip.float().cpu() - g_ref).abs().max().item() / g_ref.abs().max().item()
    cos = float((g_hip.float().cpu() * g_ref).sum() / (g_hip.float().cpu().norm() * g_ref.norm()))
    print(f"[measured] sdxl layout {dt}: maps {np.abs(A.detach().cpu().numpy() - A_ref.detach().numpy()).max() / A_ref.max().item():.3e} "
          f"loss {abs(loss.item() - float(r['loss'])) / abs(float(r['loss'])):.3e} grad max-rel {err:.3e} cosine {cos:.5f}")
    assert err < tol_grad and cos > (0.99999 if dt == "f32" else 0.997), (err, cos)


def test_paint_with_words_pipeline_vs_oracle():
    """curHyperParams['paint_with_words_stop'] > 0 through the product path (score maximum, biased capture kernels, the
    gradient through the maximum) for the first step only, fp32, against the CPU oracle loop with the same setting."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    hyper = dict(G9[2]["hyper"], paint_with_words_stop=1, paint_with_words_weight=0.8)
    meta = dict(G9[2], steps=3, hyper=hyper)
    thr = {0: 0.5}
    unet, embeds, lat0, noise, _ = g9_setup(meta)
    plan = oloss.TokenPlan(BASE_ENTRIES, {k: v for k, v in hyper.items() if not k.startswith("paint")})
    s = GuidedSampler(unet, plan, thresholds=thr, only_update_on_threshold_steps=meta["only_update_on_threshold_steps"],
                      max_iter_to_alter=meta["max_iter_to_alter"], steps=meta["steps"], scale_factor=meta["scale_factor"],
                      paint_with_words={"stop": 1, "weight": 0.8})
    ref = s.sample(lat0, embeds, noise).numpy()
    s0 = GuidedSampler(unet, plan, thresholds=thr, only_update_on_threshold_steps=meta["only_update_on_threshold_steps"],
                       max_iter_to_alter=meta["max_iter_to_alter"], steps=meta["steps"], scale_factor=meta["scale_factor"])
    plain = s0.sample(lat0, embeds, noise).numpy()
    assert np.abs(ref - plain).max() > 1e-2 * np.abs(plain).max()       # the mask really changes the result
    import copy
    pipe = build_product(copy.deepcopy(unet), torch.float32)
    pipe.use_graphs = True    # must fall back to eager launches by itself while paint-with-words is on
    out, _ = run_product(pipe, meta, embeds, lat0, noise, thr)
    pipe.use_graphs = False
    assert s.calls["bwd"] >= 1
    assert (out.unet_calls["fwd_b1_grad"], out.unet_calls["bwd"]) == (s.calls["fwd_b1_grad"], s.calls["bwd"])
    err = np.abs(out.latents.float().cpu().numpy() - ref).max() / np.abs(ref).max()
    assert err < 5e-3, err


@pytest.fixture(scope="module")
def full_width():
    """The configuration bench.py times, built ONCE for the tests below: the full-width SD-1.x UNet (`UNetConfig.sd15()`, 860 M
    seeded weights) as the fp16 product pipeline on the GPU and as the fp32 CPU oracle (GuidedSampler), with the oracle's results
    for one guidance evaluation + latent update and one CFG evaluation + DDIM step on the same latents / prompt embedding
    (reference: pipeline_guided_attention.py:946-973, 456-470, 1010-1029).  The oracle passes cost ~7 s of host time in all."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import copy
    from types import SimpleNamespace
    from guided_attention_amd.pipeline_guided_attention import GuidedAttention
    from guided_attention_amd.text import SyntheticTextEncoder, WordTokenizer
    from guided_attention_amd.unet import UNet2DConditionModel, UNetConfig
    from oracle import attention as oattn
    from oracle.pipeline import ddim_step
    cfg_u = UNetConfig.sd15()
    unet = UNet2DConditionModel(cfg_u).init_weights_(seed=0).float()
    for p in unet.parameters():
        p.requires_grad_(False)
    fw = SimpleNamespace(t=981, step=20.0, guidance=7.5)
    fw.embeds = torch.randn(2, 77, cfg_u.cross_attention_dim, generator=torch.Generator("cpu").manual_seed(1234))
    fw.lat0 = torch.randn(1, 4, 64, 64, generator=torch.Generator("cpu").manual_seed(28))
    # product first (the deep copy goes to the GPU in fp16; the fp32 original stays for the oracle)
    fw.pipe = GuidedAttention(copy.deepcopy(unet).half(), None, None, SyntheticTextEncoder(cfg_u.cross_attention_dim),
                              WordTokenizer()).to("cuda", torch.float16)
    fw.emb_g, fw.lat_g = fw.embeds.cuda().half(), fw.lat0.cuda().half()
    # oracle (CPU fp32): guidance evaluation + update, then the CFG pair + DDIM step from the same latents
    s = GuidedSampler(unet, oloss.TokenPlan(BASE_ENTRIES), thresholds={0: 1.0})
    with torch.enable_grad():
        lat_c, r, _ = s._evaluate(fw.lat0, fw.t, fw.embeds[1:2])
        fw.new_ref = s._update(lat_c, r["loss"], fw.step).detach()
    fw.loss_ref = float(r["loss"])
    fw.g_ref = (fw.lat0 - fw.new_ref) / fw.step
    fw.A_ref = oattn.aggregate(s.store.attention_store, 16, ("up", "down", "mid"), True).detach()
    fw.maps_ref = {key: [m.detach().clone() for m in s.store.attention_store[key] if m.shape[1] == 256]
                   for key in ("down_cross", "up_cross")}
    with torch.no_grad():
        fw.eps_ref = unet(torch.cat([fw.lat0] * 2), fw.t, encoder_hidden_states=fw.embeds).sample.detach()
    eps = fw.eps_ref[0:1] + fw.guidance * (fw.eps_ref[1:2] - fw.eps_ref[0:1])
    fw.x_prev_ref = ddim_step(eps, fw.t, fw.lat0, s.acp, 50)
    del s, unet
    yield fw
    for runner in fw.pipe._graph_cache.values():
        runner.release()
    fw.pipe._graph_cache.clear()


def _activate_full_width(fw, graphs):
    """Module globals, controller and (optionally) the hipGraph runner for one test on the shared full-width pipeline."""
    from guided_attention_amd import run
    from guided_attention_amd.config import RunConfig
    from guided_attention_amd.graphs import GraphRunner
    from guided_attention_amd.utils import helpers, ptp_utils, shared_state as state
    pipe = fw.pipe
    rc = RunConfig(meta_prompt="a [robot:.6,.3,.4,.55] and a [blue vase:.2,.3,.4,.55]", output_path="/tmp/ga_test_out")
    rc.stable = pipe
    state.curHyperParams = dict(state.hyperParameterOverrides)
    run.overrideConfig(rc)
    run.parseMetaPrompt(rc)
    helpers.log_clear()
    ctrl = ptp_utils.AttentionStore()
    ptp_utils.register_attention_control(pipe, ctrl)
    pipe._attention_store = ctrl
    pipe.unet_calls = {k: 0 for k in ("fwd_b1_grad", "bwd", "fwd_b2", "loss_evals", "joint_b3")}
    pipe._deferred_log, pipe._deferred_losses = [], []
    pipe._truncate_at = None
    pipe.batch_loss_only_guidance = True
    pipe._runner = GraphRunner.for_run(pipe, ctrl, fw.emb_g, fw.lat_g, 16, True, 0.5, 3, False) if graphs else None
    return ctrl


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


# batches 2 and 3 (the CFG and joint passes) are held to the fp32 oracle at full width by
# test_full_width_joint_pass_and_ddim_step_vs_oracle_fp16 and their shapes to fp64 by the kernel tests; here every further batch
# size costs 45 s of MIOpen kernel look-ups for its library arm (round 4 measured batch 1 / 2 / 3: noise prediction 2.4e-3 / 2.6e-3 / 2.2e-3, latent gradient 2.8e-3 / 3.1e-3 / 3.6e-3)
@pytest.mark.parametrize("batch", [1])
def test_full_width_unet_own_kernels_match_the_library(full_width, batch):
    """The SD-1.x UNet at FULL width in fp16 (the shared full-width pipeline): one guidance-style forward + backward to the
    latents with the 3x3 convolutions on ga_conv3x3_nhwc (every real shape: measured plans, XCD-aware order, patch and per-tap
    variants, split-K, bias + residual epilogue, the flipped pack in the backward), the transformer blocks on ga_linear_fused and
    the UpBlock concatenations on ga_cat_channels, against the SAME UNet with all three back on the library (MIOpen, hipBLASLt +
    the separate LayerNorm / GEGLU / add kernels, torch.cat).  Both accumulate in f32 and round once per layer: the results
    agree to fp16 rounding noise."""
    from guided_attention_amd import fused_linear, ops
    pipe = full_width.pipe
    pipe._runner = None
    g = torch.Generator().manual_seed(5)
    lat = torch.randn(batch, 4, 64, 64, generator=g).cuda().half()
    ctx = torch.randn(batch, 77, 768, generator=g).cuda().half()
    wgt = torch.randn(batch, 4, 64, 64, generator=g).cuda().half()

    def run_once():
        x = lat.clone().requires_grad_(True)
        y = pipe.unet(x, 981, encoder_hidden_states=ctx).sample
        (gx,) = torch.autograd.grad((y.float() * wgt.float()).sum(), [x])
        return y.detach().float(), gx.float()

    with ops.census_scope() as cs:
        y_own, g_own = run_once()
    assert sum(n for k, n in cs.launches.items() if k[0] == "conv3x3") > 80      # the HIP convolution really ran
    assert sum(n for k, n in cs.launches.items() if k[0] == "linear") > 100      # and the fused Linear layers
    assert sum(n for k, n in cs.launches.items() if k[0].startswith("conv3x3_thin")) == 4   # conv_in, conv_out and the backward of each
    elementwise = (ops.geglu, ops.bias_residual_add, (ops.layer_norm, ops.add_layer_norm))
    pipe.unet.set_fused_impl(*elementwise, None)
    edge, pipe.unet.edge_conv_impl = pipe.unet.edge_conv_impl, None
    bench_mode, torch.backends.cudnn.benchmark = torch.backends.cudnn.benchmark, False   # no exhaustive library search here
    try:
        with ops.census_scope() as cs:
            y_lib, g_lib = run_once()
    finally:
        torch.backends.cudnn.benchmark = bench_mode
        pipe.unet.edge_conv_impl = edge
        pipe.unet.set_fused_impl(*elementwise, ops.conv3x3, fused_linear, ops.cat_channels)
    assert not any(k[0] in ("conv3x3", "linear") or k[0].startswith("conv3x3_thin") for k in cs.launches)
    assert torch.isfinite(y_own).all() and torch.isfinite(g_own).all()
    ey = float((y_own - y_lib).abs().max() / y_lib.abs().max())
    eg = float((g_own - g_lib).abs().max() / g_lib.abs().max())
    print(f"[measured] full width own kernels vs library, batch {batch}: noise prediction {ey:.3e} latent gradient {eg:.3e}")
    assert ey < 2e-2 and eg < 5e-2, (ey, eg)


# measured on the MI355X (round 4, the [measured] line, eager == graphs to every printed digit): maps 2.2e-3, aggregate 8.2e-4,
# loss 3.2e-6, latent gradient max-rel 1.03e-2 with cosine 0.99944, updated latents 5.2e-4.  The bounds below are <= 2.5x
# these (round 3 carried 3e-2 / 1e-2 / 2e-2 / 1.5e-1 / 2e-3 without a measurement), except the loss (6x): its error is a
# cancellation residue — O(1) box masses of a 40-map mean whose per-pixel errors average out — i.e. a random draw of order
# 1e-5 that moves with the last bit of any library kernel upstream, not a systematic deviation.
@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graphs"])
def test_full_width_guidance_evaluation_vs_oracle_fp16(full_width, graphs):
    """ONE guidance evaluation in fp16 through the product path at the REAL width — capture kernels, aggregate, smoothed box
    loss, the backward to the latents and one `_update_latent` — against the fp32 CPU oracle on the same weights, latents and
    prompt embedding (reference: pipeline_guided_attention.py:946-973, 456-470).

    Stated fp16 tolerances (max |difference| / max |oracle value| unless said otherwise), with the error budget behind
    each: a stored 16x16 cross map passes through up to ~60 fp16-rounded layers (rel. 2^-11 = 4.9e-4 each, random signs:
    ~sqrt(60) x 2^-12 = 1e-3 before its softmax): 5e-3; their 40-map mean: 2e-3; the loss is a sum of O(1) box masses of that
    mean: 2e-5 relative; the latent gradient additionally runs the whole backward in fp16 (loss gradients ~1e-5 carried under
    power-of-two scales): 2.5e-2 of its maximum, cosine > 0.998; the updated latents are x - 20 g with |20 g| << |x|: 1.3e-3."""
    from guided_attention_amd.utils import ptp_utils
    fw, pipe = full_width, full_width.pipe
    ctrl = _activate_full_width(fw, graphs)
    try:
        with torch.enable_grad():
            leaf, losses_dict = pipe._guidance_eval(fw.lat_g, fw.t, fw.emb_g[1:2], ctrl, 16, True, 0.5, 3, False)
            maps = {k: [m.detach().float().cpu() for m in v] for k, v in ctrl.attention_store.items() if v}
            A = ptp_utils.aggregate_attention(ctrl, 16, ("up", "down", "mid"), True, 0).detach().float().cpu()
            loss, _, unscaled = pipe._compute_loss(losses_dict, return_losses=True)
            if graphs:      # the captured backward pass leaves the latent gradient in the runner's static buffer
                new_lat = pipe._update_latent(leaf, loss, fw.step)
                grad = pipe._runner.grad.detach().float().cpu()
            else:
                grad = torch.autograd.grad(loss, [leaf], retain_graph=True)[0].detach().float().cpu()
                new_lat = pipe._update_latent(leaf, loss, fw.step)
        assert pipe.unet_calls["bwd"] == 1 and pipe.unet_calls["fwd_b1_grad"] == 1
        loss_v = float(losses_dict["_fused"]["host_total"])
        new_lat = new_lat.float().cpu()
    finally:
        pipe._runner = None
    assert {k: len(v) for k, v in maps.items()} == {"down_cross": 2, "up_cross": 3}
    e_map = max(_rel(got, ref) for key in ("down_cross", "up_cross") for got, ref in zip(maps[key], fw.maps_ref[key]))
    assert all(len(maps[key]) == len(fw.maps_ref[key]) for key in maps)
    e_A, e_loss = _rel(A, fw.A_ref), abs(loss_v - fw.loss_ref) / abs(fw.loss_ref)
    e_grad, e_lat = _rel(grad, fw.g_ref), _rel(new_lat, fw.new_ref)
    cos = float((grad * fw.g_ref).sum() / (grad.norm() * fw.g_ref.norm()))
    print(f"[measured] full width {'graphs' if graphs else 'eager'} fp16 vs fp32 oracle: maps {e_map:.3e} aggregate {e_A:.3e} "
          f"loss {e_loss:.3e} grad max-rel {e_grad:.3e} cosine {cos:.5f} updated latents {e_lat:.3e}")
    assert e_map < 5e-3 and e_A < 2e-3 and e_loss < 2e-5, (e_map, e_A, e_loss)
    assert e_grad < 2.5e-2 and cos > 0.998, (e_grad, cos)
    assert e_lat < 1.3e-3, e_lat


def test_full_width_joint_pass_and_ddim_step_vs_oracle_fp16(full_width):
    """ONE loss-only denoising step as bench.py runs 49 of every 50: the fp16 hipGraph batch-3 joint pass (`g_joint`: guidance
    forward on the cond embedding + the CFG pair, one replay on ga_linear_fused / ga_conv3x3_nhwc at M = 12 288 tokens) and
    `ga_cfg_ddim_step` on its noise prediction — eps_uncond, eps_cond, the logged loss and x_prev against the fp32 CPU oracle
    (reference: pipeline_guided_attention.py:1010-1029; the guidance evaluation :946-973 whose loss such a step only logs).
    Also: the separate B=2 CFG graph (`g_cfg`) gives the same noise prediction as samples 1-2 of the joint pass.
    Measured (round 4, MI355X): eps_uncond 1.7e-3, eps_cond 2.0e-3, loss 7.8e-6, x_prev 8.4e-4, B=2 graph vs joint samples
    1.4e-3; bounds <= 2.5x (the loss: see the test above).  Budget: the noise prediction is ~60 fp16-rounded layers deep
    (~sqrt(60) x 2^-12 per element, a few times that at the maximum): 5e-3 of its maximum; the CFG combine amplifies the
    cond - uncond difference by 7.5 and x_prev = c1 x + c2 eps with |c2| ~ 0.03 at t = 981: 2e-3 of max |x_prev|."""
    from guided_attention_amd import ops
    from guided_attention_amd.scheduler import DDIMScheduler
    fw, pipe = full_width, full_width.pipe
    ctrl = _activate_full_width(fw, True)
    try:
        runner = pipe._runner
        assert runner.joint
        with ops.census_scope() as cs:
            parts, noise = runner.joint_forward(fw.lat_g, fw.t, ctrl)
        losses_dict = pipe._loss_host(*parts)
        loss_v = float(losses_dict["_fused"]["host_total"])
        noise = noise.detach().clone()
        sch = DDIMScheduler()
        sch.set_timesteps(50)
        a_t, a_prev = sch.alphas_for(fw.t)
        x_prev, _ = ops.cfg_ddim_step(noise[0:1], noise[1:2], fw.guidance, fw.lat_g, a_t, a_prev, False)
        noise_cfg = runner.cfg_forward(fw.lat_g, fw.t, ctrl).detach().clone()
        # what the store publishes after a joint step: the CFG pair's maps (samples 1, 2), as after a two-pass step
        assert ctrl.attention_store["up_cross"][0].shape[0] == 2 * 8
    finally:
        pipe._runner = None
    lin = {k: n for k, n in cs.launches.items() if k[0] == "linear"}
    assert any(k[1] == 12288 and k[2] == 320 and k[5] == 2560 for k in lin), "the batch-3 GEGLU GEMM did not run on ga_linear_fused"
    assert any(k[0] == "conv3x3" and k[1] == 3 for k in cs.launches)
    e_u, e_c = _rel(noise[0:1].float().cpu(), fw.eps_ref[0:1]), _rel(noise[1:2].float().cpu(), fw.eps_ref[1:2])
    e_loss = abs(loss_v - fw.loss_ref) / abs(fw.loss_ref)
    e_x = _rel(x_prev.float().cpu(), fw.x_prev_ref)
    e_two = _rel(noise_cfg.float().cpu(), noise.float().cpu())
    print(f"[measured] full width joint step fp16 vs fp32 oracle: eps_uncond {e_u:.3e} eps_cond {e_c:.3e} loss {e_loss:.3e} "
          f"x_prev {e_x:.3e}; B=2 CFG graph vs joint samples 1-2 {e_two:.3e}")
    assert e_u < 5e-3 and e_c < 5e-3, (e_u, e_c)
    assert e_loss < 2e-5, e_loss
    assert e_x < 2e-3, e_x
    assert e_two < 3.5e-3, e_two          # different batch -> different tiles / split-K plans: fp16 rounding noise only
