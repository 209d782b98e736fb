"""SGD-momentum refinement (`use_optimizer`) in batched calls on the GPU: ga_latent_sgd_momentum_batched against the solo entry
(bit for bit, per image) and against fp64, where it writes, what it refuses; and the batched pipeline with
GuidedAttention.batched_momentum_refinement against the reference's own runs (tests/golden/g12_momentum.*, g9_loop.*) and
against solo calls on each image's inputs.  Needs an MI355X (`pytest -m gpu`)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import hashrand
from conftest import load_json, load_npz
from guarded_alloc import assert_intact, guarded, snapshot, unwritten_mask
from test_momentum_refinement_gpu import DTYPES, EPS, LR, MU, f64, half_ulp
from test_oracle_loop import G9, g9_setup
from test_pipeline_gpu import build_product, wide_setup
from test_prompts_per_pass_gpu import _install, _mask_numbers, _rel, _run

pytestmark = pytest.mark.gpu

G12 = {m["name"]: m for m in load_json("g12_momentum.json")}
BITS = {"f32": torch.int32, "f16": torch.int16, "bf16": torch.int16}
IMAGES = [1, 3, 64]
# one element; slices that lose 16-byte alignment (7, 255, 257: around one workgroup); 4 * 33 * 33 (4356 % 8 = 4: the 16-bit
# types go element by element, f32 in 16-byte vectors); the SD-1.x latents
SIZES = [1, 7, 255, 257, 4356, 16384]
NAN_PATTERNS = (0x7FC00000, 0x7F800001, -1, 0x7FFFFFFF)    # quiet, signalling, all ones, largest payload


@pytest.fixture(autouse=True)
def _keep_shared_state():
    from guided_attention_amd.utils import shared_state as state
    saved = state.curHyperParams, getattr(state, "config", None)
    yield
    state.curHyperParams, state.config = saved


# ------------------------------------------------------------------------------------------ the kernel
def inputs(S, n, dt, seed):
    """x (latents-like), g (gradient-like) (S, n) of the dtype, a hashed f32 velocity (S, n) and one lr per image."""
    x = torch.from_numpy(hashrand.normalish((S, n), seed) * np.float32(3.0)).to(DTYPES[dt]).cuda()
    g = torch.from_numpy(hashrand.normalish((S, n), seed + 1) * np.float32(0.4)).to(DTYPES[dt]).cuda()
    m = torch.from_numpy(hashrand.normalish((S, n), seed + 2)).cuda()
    lr = (torch.arange(S, dtype=torch.float32) * 0.37 + 1.0) * float(LR) / 3.0
    return x, g, m, lr.cuda()


def poison(m, rows):
    """NaN bit patterns (several kinds, varying along the slice) into the velocity slices `rows`."""
    pats = torch.tensor(NAN_PATTERNS, dtype=torch.int32, device=m.device)
    for s in rows:
        m[s].view(torch.int32).copy_(pats[(torch.arange(m.shape[1], device=m.device) + s) % len(NAN_PATTERNS)])
    return m


def flags(values):
    return torch.tensor([int(bool(v)) for v in values], dtype=torch.int32, device="cuda")


def launch(x, g, m, lr, first, active, out=None, images=None, n=None, mu=MU):
    """The C entry itself (ops.latent_sgd_momentum_batched always allocates its result): `out` may be x; -> (status, out)."""
    from guided_attention_amd import _lib
    out = torch.empty_like(x) if out is None else out
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    rc = _lib.load().ga_latent_sgd_momentum_batched(p(x), p(g), p(m), p(lr), float(mu), p(first), p(active), p(out),
                                                    x.shape[0] if images is None else images, x.shape[1] if n is None else n,
                                                    _lib.dtype_code(x), _lib.stream_ptr())
    return rc, out


def solo_expected(x, g, m, lr, first, active):
    """What the contract promises, built image by image: ga_latent_sgd_momentum on copies of an active image's slices, the
    latents and the prior velocity bytes of an inactive one."""
    from guided_attention_amd import ops
    out, vel = x.clone(), m.clone()
    lr_host, first_host, active_host = lr.cpu(), first.cpu().tolist(), active.cpu().tolist()
    for s in range(x.shape[0]):
        if active_host[s]:
            ms = m[s].clone()
            out[s] = ops.latent_sgd_momentum(x[s].clone(), g[s].clone(), ms, float(lr_host[s]), MU, bool(first_host[s]))
            vel[s] = ms
    return out, vel


PATTERNS = [("all-on", lambda s: True, 0), ("all-on", lambda s: True, 1), ("all-off", lambda s: False, 0),
            ("mixed", lambda s: s % 3 != 1, 1)]


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("S", IMAGES)
def test_every_image_is_bit_identical_to_the_solo_entry(S, n, dt):
    """Per image lr, `first` alternating over the images (both phases), `active` all on / all off / mixed.  The velocity is
    hashed values, with NaN patterns in the slices of first and of inactive images: an active image's out and velocity are the
    solo launch's bits, an inactive image's out is its latents and its velocity keeps its bytes."""
    from guided_attention_amd import ops
    x, g, m0, lr = inputs(S, n, dt, 1000 + 7 * S + n)
    for name, on, phase in PATTERNS:
        first_host, active_host = [(s + phase) % 2 == 0 for s in range(S)], [on(s) for s in range(S)]
        first, active = flags(first_host), flags(active_host)
        m = poison(m0.clone(), [s for s in range(S) if first_host[s] or not active_host[s]])
        want_out, want_vel = solo_expected(x, g, m, lr, first, active)
        snap = snapshot(x, g, lr, first, active)
        out = ops.latent_sgd_momentum_batched(x, g, m, lr, MU, first, active)
        assert out.shape == x.shape and out.dtype == x.dtype and out.data_ptr() != x.data_ptr()
        assert torch.equal(out.view(BITS[dt]), want_out.view(BITS[dt])), (name, phase)
        assert torch.equal(m.view(torch.int32), want_vel.view(torch.int32)), (name, phase)
        assert_intact(snap)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_lists_are_copied_to_the_device(dt):
    from guided_attention_amd import ops
    S, n = 3, 257
    x, g, m, lr = inputs(S, n, dt, 1500)
    m2 = m.clone()
    first, active = [1, 0, 1], [1, 1, 0]
    a = ops.latent_sgd_momentum_batched(x, g, m, lr.cpu().tolist(), MU, first, active)
    b = ops.latent_sgd_momentum_batched(x, g, m2, lr, MU, flags(first), flags(active))
    assert torch.equal(a.view(BITS[dt]), b.view(BITS[dt])) and torch.equal(m.view(torch.int32), m2.view(torch.int32))


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_first_image_with_an_all_nan_velocity_slice(dt):
    """`first` is a run-time flag here, so the old velocity is loaded — and dropped by a select: velocity == float32(g) bit for
    bit, out finite, on the 16-byte path (16384) and the element path (257)."""
    from guided_attention_amd import ops
    for n in (257, 16384):
        x, g, m, lr = inputs(3, n, dt, 2000 + n)
        poison(m, [0, 2])
        out = ops.latent_sgd_momentum_batched(x, g, m, lr, MU, [1, 0, 1], [1, 1, 1])
        for s in (0, 2):
            assert torch.equal(m[s].view(torch.int32), g[s].float().view(torch.int32)), s
        assert torch.isfinite(out.float()).all() and torch.isfinite(m).all()


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_out_may_alias_latents(dt):
    for S, n in ((3, 255), (3, 4356), (2, 16384)):
        x, g, m, lr = inputs(S, n, dt, 3000 + n)
        first, active = flags(s == 0 for s in range(S)), flags(s != 1 for s in range(S))
        m2, x2 = m.clone(), x.clone()
        rc, ref = launch(x, g, m, lr, first, active)
        assert rc == 0
        rc, same = launch(x2, g, m2, lr, first, active, out=x2)
        assert rc == 0 and same is x2
        assert torch.equal(x2.view(BITS[dt]), ref.view(BITS[dt])) and torch.equal(m.view(torch.int32), m2.view(torch.int32))


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_one_step_against_fp64(dt):
    """One step with first = 0 at S = 3, n = 4356 (per-image lr), at the bounds test_momentum_refinement_gpu.step_reference
    derives for the solo step: velocity 2^-23 (|mu b_old| + |g|), out 2^-23 (|x| + |lr b|) plus half an ulp of T."""
    from guided_attention_amd import ops
    S, n = 3, 4356
    x, g, m, lr = inputs(S, n, dt, 4000)
    b_old = f64(m)
    out = ops.latent_sgd_momentum_batched(x, g, m, lr, MU, [0] * S, [1] * S)
    x64, g64, lr64 = f64(x), f64(g), f64(lr)[:, None]
    mb = np.float64(MU) * b_old
    b64 = g64 + mb
    o64 = x64 - lr64 * b64
    bound_b, bound_o = EPS * (np.abs(mb) + np.abs(g64)), EPS * (np.abs(x64) + np.abs(lr64 * b64)) + half_ulp(o64, dt)
    err_b, err_o = np.abs(f64(m) - b64), np.abs(f64(out) - o64)
    print(f"[measured] sgd_momentum_batched {dt}: velocity {np.max(err_b / np.maximum(bound_b, 1e-300)):.3f} output "
          f"{np.max(err_o / bound_o):.3f} of the bound")
    assert (err_b <= bound_b).all(), err_b.max()
    assert (err_o <= bound_o).all(), err_o.max()


@pytest.mark.parametrize("dt,n", [("f16", 4356), ("f32", 16384)])
def test_the_launch_writes_its_outputs_and_nothing_else(dt, n):
    """Under guarded(ops), with the velocity in a guarded arena as well: red zones intact, every element of out written (the
    inactive image's too), every input bit-identical afterwards, the velocity changed in the active slices only."""
    from guided_attention_amd import ops
    S = 3
    x, g, m0, lr = inputs(S, n, dt, 5000 + n)
    first, active = flags([1, 0, 0]), flags([1, 0, 1])
    with guarded(ops) as guard:
        m = guard.carve((S, n), torch.float32, x.device, "the velocity buffer")
        m.copy_(m0)
        snap = snapshot(x, g, lr, first, active)
        out = ops.latent_sgd_momentum_batched(x, g, m, lr, MU, first, active)
        guard.assert_written(out, "out")
        assert_intact(snap)
    assert not bool(unwritten_mask(out).any())
    assert torch.equal(out[1].view(BITS[dt]), x[1].view(BITS[dt]))
    assert torch.equal(m[1].view(torch.int32), m0[1].view(torch.int32))
    for s in (0, 2):
        assert not torch.equal(m[s], m0[s])


def test_bad_arguments_are_refused_before_any_launch():
    from guided_attention_amd import ops
    from guided_attention_amd._lib import GA_MAX_IMAGES
    S, n = 3, 64
    x, g, m, lr = inputs(S, n, "f16", 6000)
    first, active = flags([1, 0, 1]), flags([1, 1, 1])
    out = torch.full_like(x, 7.0)
    snap = snapshot(out, m, x, g)
    for status, kw in ((-2, dict(images=0)), (-2, dict(images=GA_MAX_IMAGES + 1)), (-2, dict(n=0)), (-2, dict(mu=1.0)),
                       (-1, dict(active=None))):
        args = dict(first=first, active=active, out=out)
        args.update(kw)
        rc, _ = launch(x, g, m, lr, **args)
        assert rc == status, kw
    torch.cuda.synchronize()
    assert_intact(snap, "output or input")
    with pytest.raises(ops.GaError, match="velocity buffer"):
        ops.latent_sgd_momentum_batched(x, g, m.half(), lr, MU, first, active)
    with pytest.raises(ops.GaError, match="velocity buffer"):
        ops.latent_sgd_momentum_batched(x, g, m[:2], lr, MU, first, active)
    with pytest.raises(ops.GaError, match="first is a contiguous"):
        ops.latent_sgd_momentum_batched(x, g, m, lr, MU, first[:2], active)


# ------------------------------------------------------------------------------------------ the pipeline
META_PROMPT = "a [robot:.6,.3,.4,.55] and a [blue vase:.2,.3,.4,.55]"
ALWAYS_MET = {0: 100.0, 1: 100.0}     # the fixture's threshold steps; the losses of this case are of order 1


def _recording(pipe, margins):
    """pipe.meets_threshold with every comparison it makes recorded as |loss - threshold| / threshold."""
    inner = type(pipe).meets_threshold

    def meets(i, thresholds, losses):
        if not ((i not in thresholds and i != -1) or len(thresholds) == 0):
            thr = list(thresholds.values())[-1] if i == -1 else thresholds[i]
            _, per_sub = pipe.group_losses_by_sumprompt(losses)
            margins.extend(abs(float(v) - thr) / thr for v in per_sub.values())
        return inner(pipe, i, thresholds, losses)
    return meets


def _mixed_inputs(meta, setup):
    """(a) the fixture's `use_optimizer` case, (b) the same without it, (c) `use_optimizer` with thresholds that are always met —
    all three on the fixture's latents, embeddings and re-noise list."""
    _, embeds, lat0, noise, thr = setup
    plain = {k: v for k, v in meta["hyper"].items() if k != "use_optimizer"}
    base = dict(meta_prompt=META_PROMPT, embeds=embeds, lat=lat0, noise=noise)
    return [dict(base, thresholds=thr, hyper=dict(meta["hyper"])), dict(base, thresholds=thr, hyper=plain),
            dict(base, thresholds=dict(ALWAYS_MET), hyper=dict(meta["hyper"]))]


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graphs"])
def test_mixed_call_fp32_matches_the_reference_runs_and_solo_calls(graphs):
    """guidance_states with three images: (a) against the reference's own `use_optimizer` run (g12 `momentum_g9`), (b) against
    its plain run (g9 `no_recurse_thr2`), every image against its solo call on the same pipe, at 5e-3 of the latent maximum
    (the project's fp32 bar for GPU against reference and batched against solo; both fixtures hold every threshold comparison of
    (a) and (b) at least 5 % clear).  (c) meets its thresholds everywhere: its solo call takes no backward pass, so none of its
    branches hangs on a margin, and it idles through every refinement pass of the batched call."""
    meta = G12["momentum_g9"]
    g9 = [m for m in G9 if m["name"] == "no_recurse_thr2"][0]
    assert meta["thresholds"] == g9["thresholds"] and meta["steps"] == g9["steps"]
    setup = g9_setup(meta)
    imgs = _mixed_inputs(meta, setup)
    pipe = build_product(setup[0], torch.float32)
    pipe.use_graphs = graphs
    solo = [_run(pipe, meta, [im], False) for im in imgs]
    assert solo[2][0].unet_calls["bwd"] == 0
    assert solo[0][0].census.get("latent_sgd_momentum", 0) == meta["optimizer_steps"]
    pipe.batched_momentum_refinement = True
    out, _ = _run(pipe, meta, imgs, True)
    assert (graphs and pipe._runner is not None) or (not graphs and pipe._runner is None)
    refs = [load_npz("g12_momentum.npz")["momentum_g9.final_latents"], load_npz("g9_loop.npz")["no_recurse_thr2.final_latents"]]
    counters = [(meta["fwd_b1"], meta["bwd"] + meta["optimizer_steps"], meta["fwd_b2"]), (g9["fwd_b1"], g9["bwd"], g9["fwd_b2"])]
    errs = []
    for s in range(3):
        mine = out.unet_calls_per_image[s]
        assert mine == solo[s][0].unet_calls, s
        assert _mask_numbers(out.logs[s]) == _mask_numbers(solo[s][1]), s
        e_solo = _rel(out.latents[s], solo[s][0].latents[0])
        e_ref = _rel(out.latents[s], torch.from_numpy(refs[s][0])) if s < 2 else None
        errs.append((e_ref, e_solo))
        if s < 2:
            assert (mine["fwd_b1_grad"], mine["bwd"], mine["fwd_b2"]) == counters[s], s
    print(f"[measured] fp32 {'graphs' if graphs else 'eager'} mixed call vs reference / vs solo:", errs,
          "passes", out.batched_passes)
    for s, (e_ref, e_solo) in enumerate(errs):
        assert e_solo < 5e-3 and (e_ref is None or e_ref < 5e-3), (s, e_ref, e_solo)
    # (a) logs the two plain updates of the caller and nothing from inside a refinement; (b) one line per backward pass
    assert sum("gradient size average" in ln for ln in out.logs[0]) == meta["bwd"] == 2
    assert sum("gradient size average" in ln for ln in out.logs[1]) == g9["bwd"]
    assert out.census.get("latent_sgd_momentum_batched", 0) == meta["optimizer_steps"] == 20
    assert out.census.get("latent_sgd_momentum", 0) == 0 and out.census.get("latent_axpy", 0) == 0
    assert out.census.get("latent_axpy_batched", 0) > 0
    assert out.batched_passes["bwd"] < sum(c["bwd"] for c in out.unet_calls_per_image)   # plain and momentum shared passes
    assert out.batched_passes["idle_slots"] > 0


def _seeds_call(pipe, meta, embeds, lats, noises, thr):
    """One prompt, len(lats) images (num_images_per_prompt), the state in shared_state as run.execute leaves it."""
    from guided_attention_amd import ops, run
    from guided_attention_amd.config import RunConfig
    from guided_attention_amd.utils import helpers, ptp_utils, shared_state as state
    S = len(lats)
    cfg = RunConfig(meta_prompt=META_PROMPT, output_path="/tmp/ga_test_out")
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


def test_two_seeds_of_a_use_optimizer_state_fp32():
    """num_images_per_prompt = 2 with `use_optimizer` in curHyperParams.  Image 0 is the fixture's latents: against the
    reference's run at 5e-3.  Image 1 is the same latents negated, which has no reference run: against its own solo call at
    5e-3, counters exactly; every threshold comparison of that solo call (recorded where meets_threshold makes it) is at least
    5 % clear, so the branch it takes does not hang on a rounding."""
    meta = G12["momentum_g9"]
    unet, embeds, lat0, noise, thr = g9_setup(meta)
    pipe = build_product(unet, torch.float32)
    margins = []
    pipe.meets_threshold = _recording(pipe, margins)
    solo1, lines1 = _seeds_call(pipe, meta, embeds, [-lat0], [noise], thr)
    del pipe.meets_threshold
    print(f"[measured] image 1 (negated latents) solo: smallest threshold margin {min(margins):.3f} over {len(margins)} "
          f"comparisons, counters {solo1.unet_calls}")
    assert min(margins) >= 0.05, min(margins)
    pipe.batched_momentum_refinement = True
    out, _ = _seeds_call(pipe, meta, embeds, [lat0, -lat0], [noise, noise], thr)
    ref = torch.from_numpy(load_npz("g12_momentum.npz")["momentum_g9.final_latents"][0])
    e0, e1 = _rel(out.latents[0], ref), _rel(out.latents[1], solo1.latents[0])
    print(f"[measured] two seeds fp32: image 0 vs reference {e0:.3e}, image 1 vs solo {e1:.3e}, passes {out.batched_passes}")
    c0 = out.unet_calls_per_image[0]
    assert (c0["fwd_b1_grad"], c0["bwd"], c0["fwd_b2"]) == (meta["fwd_b1"], meta["bwd"] + meta["optimizer_steps"], meta["fwd_b2"])
    assert out.unet_calls_per_image[1] == solo1.unet_calls
    assert _mask_numbers(out.logs[1]) == _mask_numbers(lines1)
    assert e0 < 5e-3 and e1 < 5e-3, (e0, e1)
    assert out.census.get("latent_sgd_momentum_batched", 0) > 0 and out.census.get("latent_sgd_momentum", 0) == 0


def test_f16_graphs_momentum_and_plain_in_one_call():
    """f16, use_graphs, the 64/64/128/128 UNet (own Linear / convolution kernels at every level), 3 steps: the batched pair
    (momentum, plain) against the reference's fp32 latents of `momentum_wide` and of its plain run, at the bars the solo runs
    of the same fixture are held to (test_half_precision_momentum_pipeline_vs_reference: 2.5e-2; the plain refinement's
    1.25e-2 of test_half_precision_pipeline_vs_oracle).  The solo calls of the same pipe are measured next to it."""
    meta = G12["momentum_wide"]
    g = load_npz("g12_momentum.npz")
    unet, embeds, lat0, noise, thr = wide_setup(meta)
    plain = {k: v for k, v in meta["hyper"].items() if k != "use_optimizer"}
    base = dict(meta_prompt=META_PROMPT, embeds=embeds, lat=lat0, noise=noise, thresholds=thr)
    imgs = [dict(base, hyper=dict(meta["hyper"])), dict(base, hyper=plain)]
    pipe = build_product(copy.deepcopy(unet), torch.float16)
    pipe.use_graphs, pipe.batch_loss_only_guidance = True, True
    solo = [_run(pipe, meta, [im], False)[0] for im in imgs]
    pipe.batched_momentum_refinement = True
    out, _ = _run(pipe, meta, imgs, True)
    assert pipe._runner is not None and pipe._runner.images == 2
    refs = [torch.from_numpy(g["momentum_wide.final_latents"][0]), torch.from_numpy(g["momentum_wide.plain_final_latents"][0])]
    errs = [_rel(out.latents[s], refs[s]) for s in range(2)]
    errs_solo = [_rel(solo[s].latents[0], refs[s]) for s in range(2)]
    print(f"[measured] f16 graphs batched (momentum, plain) vs reference: {errs[0]:.3e}, {errs[1]:.3e}; solo calls, same pipe: "
          f"{errs_solo[0]:.3e}, {errs_solo[1]:.3e}")
    c = out.unet_calls_per_image
    assert (c[0]["fwd_b1_grad"], c[0]["bwd"], c[0]["fwd_b2"]) == (meta["fwd_b1"], meta["bwd"] + meta["optimizer_steps"],
                                                                  meta["fwd_b2"])
    assert (c[1]["fwd_b1_grad"], c[1]["bwd"], c[1]["fwd_b2"]) == (meta["plain"]["fwd_b1"], meta["plain"]["bwd"],
                                                                  meta["plain"]["fwd_b2"])
    assert out.census.get("latent_sgd_momentum_batched", 0) == meta["optimizer_steps"]
    assert out.census.get("latent_sgd_momentum", 0) == 0
    assert out.census.get("linear", 0) > 0 and out.census.get("conv3x3", 0) > 0
    assert errs[0] < 2.5e-2 and errs[1] < 1.25e-2, errs
