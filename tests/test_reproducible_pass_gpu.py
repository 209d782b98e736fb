"""The same pass on the same bits gives the same bits: the `wide_setup` UNet (every 3x3 convolution and transformer Linear on the
package's own kernels) in f16 and bf16, as an eager pass, as a hipGraph replay, and as a whole guided call.  Every comparison is
`repro_trace.same_bits`: dtype, shape and raw bytes.  Where a pass does not repeat, the failure message carries the first entry,
in execution order, at which two traced repeats differ (`repro_trace.record` / `first_difference`).  Needs an MI355X."""
import copy

import pytest
import torch

import repro_trace as rt
from test_oracle_loop import G9

pytestmark = pytest.mark.gpu

DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
T = 981
LOSS_ARGS = (16, True, 0.5, 3, False)   # attention_res, smooth, sigma, kernel_size, normalize_eot

# Framework operations found to break bit equality of a pass: call site, the recorded evidence (MI355X, torch 2.x on ROCm; the
# figures are in profiles/reproducibility.json) and the remedy the tests of this module apply, for the test only.  Everything else
# in a pass is then still held to bit equality.  No product default changes here.
FRAMEWORK_OPS = {
    "torch.nn.grad.conv2d_input, 3x3, stride 2, padding 1": {
        "call site": "guided_attention_amd/ops.py, Conv3x3.backward: the backward of the three down-sampling convolutions",
        "dtypes": ("f16",),
        "evidence": (
            "repro_trace.first_difference of two traced f16 evaluations: ('grad_input', 'down_blocks.2.downsamplers.0', 0, "
            "torch.float16, (1, 128, 8, 8)) — the first stride-2 backward the pass runs; every forward entry and every gradient "
            "before it is equal, 133 of 531 entries differ behind it, 3672 of 4096 elements of the latent gradient.  The call "
            "alone, 8 repeats on the same bits: (1, 128, 8, 8) f16 differs in 2216 ... 3581 of 8192 elements, (3, 128, 8, 8) f16 "
            "in 9299 ... 10608 of 24576, (3, 128, 8, 8) bf16 in 0 ... 4; (1, 64, 32, 32), (1, 64, 16, 16) and every batch-1 bf16 "
            "shape repeat.  With torch.backends.cudnn.deterministic = True all of them repeat, and so does the f16 evaluation."),
        "remedy": "cudnn.deterministic",
    },
}


@pytest.fixture(autouse=True)
def framework_remedies(request):
    """For this test only: where an operation of FRAMEWORK_OPS breaks the test's dtype, torch.backends.cudnn.deterministic is
    set for the test and restored behind it.  Graphs captured inside the test keep the kernels they captured."""
    params = getattr(getattr(request.node, "callspec", None), "params", {})
    dt = params.get("dt") or params.get("wide")
    saved = torch.backends.cudnn.deterministic
    if any(dt in entry["dtypes"] and entry["remedy"] == "cudnn.deterministic" for entry in FRAMEWORK_OPS.values()):
        torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = saved


_UNET = {}


def _wide(meta):
    """The fp32 CPU UNet and inputs of test_pipeline_gpu.wide_setup, built once per module run."""
    if "setup" not in _UNET:
        from test_pipeline_gpu import wide_setup
        _UNET["setup"] = wide_setup(meta)
    unet, embeds, lat0, noise, thr = _UNET["setup"]
    return copy.deepcopy(unet), embeds, lat0, noise, thr


def _activate(pipe, meta, thr):
    """Module globals and controller for passes driven by hand (what GuidedAttention.__call__ sets up for itself)."""
    from guided_attention_amd import run
    from guided_attention_amd.config import RunConfig
    from guided_attention_amd.utils import helpers, ptp_utils, shared_state as state
    rc = RunConfig(meta_prompt="a [robot:.6,.3,.4,.55] and a [blue vase:.2,.3,.4,.55]", output_path="/tmp/ga_test_out")
    rc.only_update_on_threshold_steps = meta["only_update_on_threshold_steps"]
    rc.stable = pipe
    state.curHyperParams = dict(state.hyperParameterOverrides, **meta["hyper"], thresholds=thr)
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
    pipe._runner = None
    return ctrl


@pytest.fixture(scope="module", params=list(DTYPES))
def wide(request):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from types import SimpleNamespace
    from test_pipeline_gpu import build_product
    meta = G9[2]
    unet, embeds, lat0, _, thr = _wide(meta)
    dtype = DTYPES[request.param]
    w = SimpleNamespace(dt=request.param, meta=meta, thr=thr, pipe=build_product(unet, dtype))
    w.emb, w.lat = embeds.cuda().to(dtype), lat0.cuda().to(dtype)
    w.ctrl = _activate(w.pipe, meta, thr)
    w.eager = {}      # results of the first eager pass of each kind: what the replays are compared with
    yield w
    for runner in w.pipe._graph_cache.values():
        runner.release()
    w.pipe._graph_cache.clear()


def _maps(store):
    return {f"map {key}[{i}]": m.detach().clone() for key in sorted(store) for i, m in enumerate(store[key])}


def _loss_parts(parts):
    terms, loss, _, _, packed = parts
    return {"terms": terms.detach().clone(), "loss": loss.detach().clone(), "packed": packed.cpu().clone()}


def eager_eval(w):
    """_guidance_forward -> _aggregate_loss_device -> autograd.grad to the latents, as GuidedAttention._guidance_parts and
    _latent_gradient run them."""
    from guided_attention_amd import ops
    pipe = w.pipe
    with torch.enable_grad():
        leaf = w.lat.detach().clone().requires_grad_(True)
        pipe._guidance_forward(leaf, T, w.emb[1:2])
        parts = pipe._aggregate_loss_device(w.ctrl, *LOSS_ARGS)
        out = dict(_loss_parts(parts), **_maps(w.ctrl.attention_store))
        grad = torch.autograd.grad(parts[1], [leaf])[0]
        ops.end_image_broadcasts()
    out["grad"] = grad.detach().clone()
    return out


def eager_cfg(w):
    with torch.no_grad():
        lat2 = w.lat[0:1].expand(2, -1, -1, -1).contiguous()
        noise = w.pipe.unet(lat2, T, encoder_hidden_states=w.emb).sample
    return dict(_maps(w.ctrl.attention_store), noise=noise.detach().clone())


def eager_joint(w):
    """The batch-3 pass of a loss-only step, as GraphRunner._joint_body runs it: rows [cond | uncond, cond] of the same latents,
    the loss on sample 0's maps."""
    pipe, ctrl = w.pipe, w.ctrl
    with torch.no_grad():
        lat3 = w.lat[0:1].expand(3, -1, -1, -1).contiguous()
        emb3 = torch.stack([w.emb[1], w.emb[0], w.emb[1]])
        noise = pipe.unet(lat3, T, encoder_hidden_states=emb3).sample
        full = ctrl.attention_store
        ctrl.attention_store = {k: [p[: p.shape[0] // 3] for p in v] for k, v in full.items()}
        parts = pipe._aggregate_loss_device(ctrl, *LOSS_ARGS)
        ctrl.attention_store = {k: [p[p.shape[0] // 3:] for p in v] for k, v in full.items()}
    return dict(_loss_parts(parts), **_maps(ctrl.attention_store), noise=noise[1:3].detach().clone())


def require_same(what, first, again, unet=None, rerun=None):
    """Every tensor of `again` same_bits with its namesake in `first`; the message lists each one that is not, with the number
    of elements that differ, and — where the pass can be traced — the first entry at which two traced repeats differ."""
    assert sorted(first) == sorted(again), (what, sorted(first), sorted(again))
    bad = [k for k in first if not rt.same_bits(first[k], again[k])]
    if not bad:
        return
    msg = f"{what}: not the same bits in " + ", ".join(
        f"{k} ({rt.differing_elements(first[k], again[k])} of {first[k].numel()} elements)"
        if first[k].shape == again[k].shape and first[k].dtype == again[k].dtype else f"{k} (shape or dtype)" for k in bad)
    if rerun is not None:
        a, b = rt.record(unet, rerun, every_module=True), rt.record(unet, rerun, every_module=True)
        others = [f"{x.phase} {x.name}[{x.index}]" for x, y in zip(a, b) if tuple(x) != tuple(y)]
        msg += (f"; first difference of two traced repeats: {rt.first_difference(a, b)}; {len(others)} of {len(a)} entries differ, "
                f"the first: {others[:8]}")
    pytest.fail(msg)


EAGER = {"eval": eager_eval, "cfg": eager_cfg, "joint": eager_joint}


@pytest.mark.parametrize("kind", list(EAGER))
def test_eager_pass_repeats(wide, kind):
    """Twice in one process on the same latents, timestep and embeddings: loss parts, latent gradient, noise prediction and
    every stored attention map."""
    w = wide
    w.pipe._runner = None
    first = EAGER[kind](w)
    w.eager[kind] = first
    assert all(torch.isfinite(v.float()).all() for v in first.values()) and len(first) > 3
    again = EAGER[kind](w)
    require_same(f"{w.dt} eager {kind}", first, again, w.pipe.unet, lambda: EAGER[kind](w))


def test_traced_passes_have_no_difference(wide):
    """The trace itself on the real model: two eager evaluations under repro_trace.record agree entry by entry, forward and
    backward, and the record reaches the modules of every level."""
    w = wide
    w.pipe._runner = None
    a = rt.record(w.pipe.unet, lambda: eager_eval(w), every_module=True)
    b = rt.record(w.pipe.unet, lambda: eager_eval(w), every_module=True)
    phases = {e.phase for e in a}
    assert phases == {"forward", "backward", "grad_input"} and len(a) > 300
    assert any(e.name.startswith("mid_block") for e in a) and any(e.name.startswith("up_blocks.3") for e in a)
    assert rt.first_difference(a, b) is None, rt.first_difference(a, b)


def _runner(w):
    from guided_attention_amd.graphs import GraphRunner
    w.pipe._runner = GraphRunner.for_run(w.pipe, w.ctrl, w.emb, w.lat, *LOSS_ARGS)
    assert w.pipe._runner.joint
    return w.pipe._runner


def graph_eval(w):
    runner = _runner(w)
    _, parts = runner.evaluate(w.lat, T, w.ctrl)
    out = dict(_loss_parts(parts), **_maps(w.ctrl.attention_store))
    out["grad"] = runner.backward().detach().clone()
    return out


def graph_cfg(w):
    noise = _runner(w).cfg_forward(w.lat, T, w.ctrl)
    return dict(_maps(w.ctrl.attention_store), noise=noise.detach().clone())


def graph_joint(w):
    parts, noise = _runner(w).joint_forward(w.lat, T, w.ctrl)
    return dict(_loss_parts(parts), **_maps(w.ctrl.attention_store), noise=noise.detach().clone())


GRAPH = {"eval": graph_eval, "cfg": graph_cfg, "joint": graph_joint}


@pytest.mark.parametrize("kind", list(GRAPH))
def test_graph_replay_repeats_and_equals_the_eager_pass(wide, kind):
    """GraphRunner.evaluate + backward / cfg_forward / joint_forward twice on the same inputs, with a replay on other latents in
    between (the pools, workspaces and static buffers then hold another pass's values); each replay against the eager pass too:
    the captured launches are exactly the eager ones."""
    w = wide
    try:
        if kind not in w.eager:
            w.pipe._runner = None
            w.eager[kind] = EAGER[kind](w)
        first = GRAPH[kind](w)
        lat = w.lat
        w.lat = (lat.float() * -3).to(lat.dtype)
        try:
            other = GRAPH[kind](w)
        finally:
            w.lat = lat
        assert not rt.same_bits(first["loss" if kind != "cfg" else "noise"], other["loss" if kind != "cfg" else "noise"])
        again = GRAPH[kind](w)
    finally:
        w.pipe._runner = None
    require_same(f"{w.dt} graph {kind}, replay against replay", first, again)
    require_same(f"{w.dt} graph {kind}, replay against the eager pass", w.eager[kind], first)


def test_a_flipped_input_bit_changes_the_pass(wide):
    """Control: the comparison can fail.  One latent element one ulp away gives another loss gradient and noise prediction."""
    w = wide
    w.pipe._runner = None
    first = w.eager.get("eval") or eager_eval(w)
    lat = w.lat
    w.lat = lat.clone()
    w.lat.view(-1).view(torch.int16)[777] ^= 1
    try:
        moved = eager_eval(w)
    finally:
        w.lat = lat
    assert not rt.same_bits(first["grad"], moved["grad"])
    assert not all(rt.same_bits(first[k], moved[k]) for k in first if k.startswith("map "))


@pytest.mark.parametrize("mode", ["eager", "graphs"])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_whole_call_repeats(dt, mode):
    """run_product on the wide UNet for the golden's step count (refinement at two thresholds, renoising, the CFG + DDIM steps),
    twice: the final latents bit for bit and the log lines character for character, numbers included."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from test_pipeline_gpu import build_product, run_product
    meta = G9[2]
    unet, embeds, lat0, noise, thr = _wide(meta)
    pipe = build_product(unet, DTYPES[dt])
    flags = dict(use_graphs=True, batch_loss_only_guidance=True) if mode == "graphs" else {}
    try:
        a, _ = run_product(pipe, meta, embeds, lat0, noise, thr, **flags)
        b, _ = run_product(pipe, meta, embeds, lat0, noise, thr, **flags)
    finally:
        for runner in pipe._graph_cache.values():
            runner.release()
        pipe._graph_cache.clear()
    assert a.unet_calls["bwd"] > 0 and a.unet_calls == b.unet_calls and len(a.lines) > 50
    assert (a.unet_calls["joint_b3"] > 0) == (mode == "graphs")
    assert torch.isfinite(a.latents.float()).all()
    differing = [(x, y) for x, y in zip(a.lines, b.lines) if x != y]
    same = rt.same_bits(a.latents, b.latents)
    assert same and not differing and len(a.lines) == len(b.lines), \
        (f"{dt} {mode}: {0 if same else rt.differing_elements(a.latents, b.latents)} of {a.latents.numel()} latent elements "
         f"differ, {len(differing)} of {len(a.lines)} log lines; first: {differing[:1]}")
