"""SGD-momentum refinement (`use_optimizer`) on the GPU: ga_latent_sgd_momentum against fp64, and the pipeline's momentum loop
against the reference's own `__call__` (tests/golden/g12_momentum.*, written by tests/golden/make_golden_momentum.py).
Needs an MI355X (`pytest -m gpu`)."""
import ctypes

import numpy as np
import pytest
import torch

import hashrand
from conftest import load_json, load_npz
from test_oracle_loop import g9_setup
from test_pipeline_gpu import MAIN_CALLS, build_product, run_product, wide_setup

pytestmark = pytest.mark.gpu

G12 = {m["name"]: m for m in load_json("g12_momentum.json")}
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
MANTISSA = {"f16": 10, "bf16": 7}           # stored fraction bits of the 16-bit types
SIZES = [1, 255, 257, 4356, 16384]          # one element; around one workgroup; 4 * 33 * 33 (odd map); the SD-1.x latents
MU = np.float32(0.8)
LR = np.float32(20 * np.sqrt(0.9) / 2.5)    # a step size of the pipeline's kind, not exactly representable
EPS = 2.0 ** -23


@pytest.fixture(autouse=True)
def _keep_shared_state():
    from guided_attention_amd.utils import shared_state as state
    saved = state.curHyperParams, getattr(state, "config", None)
    yield
    state.curHyperParams, state.config = saved


# ------------------------------------------------------------------------------------------ the kernel against fp64
def inputs(n, dt, seed, pad=0):
    """x (latents-like, sigma ~ 3), g (gradient-like) as tensors of the dtype on the GPU, `pad` spare elements in front."""
    x = torch.from_numpy(hashrand.normalish((n + pad,), seed) * np.float32(3.0)).to(DTYPES[dt]).cuda()
    g = torch.from_numpy(hashrand.normalish((n + pad,), seed + 1) * np.float32(0.4)).to(DTYPES[dt]).cuda()
    return x, g


def f64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def half_ulp(o64, dt):
    """Half a unit in the last place of the 16-bit type at o64 (0 for f32: its rounding is inside the f32 bound)."""
    if dt == "f32":
        return np.zeros_like(o64)
    _, e = np.frexp(np.abs(o64))                                   # |o| = m * 2^e, m in [0.5, 1)
    ulp = np.ldexp(1.0, e - 1 - MANTISSA[dt])
    if dt == "f16":
        ulp = np.maximum(ulp, 2.0 ** -24)                          # subnormal spacing
    return 0.5 * ulp


def step_reference(x, g, b_old, first):
    """fp64 step from the operands as the GPU holds them (mu, lr as their float32 values) -> (b64, o64, bound_b, bound_o):
    velocity |b - b64| <= 2^-23 (|mu b_old| + |g|), output |out - o64| <= 2^-23 (|x| + |lr b|) (+ half an ulp of a 16-bit
    type, added by the caller) — a fused or an unfused multiply-add stays inside both."""
    x64, g64 = f64(x), f64(g)
    mb = np.zeros_like(g64) if first else np.float64(MU) * f64(b_old)
    b64 = g64 + mb
    o64 = x64 - np.float64(LR) * b64
    return b64, o64, EPS * (np.abs(mb) + np.abs(g64)), EPS * (np.abs(x64) + np.abs(np.float64(LR) * b64))


def launch(x, g, m, first, out=None):
    """The C entry itself (ops.latent_sgd_momentum always allocates its result): `out` may be x."""
    from guided_attention_amd import _lib
    out = torch.empty_like(x) if out is None else out
    _lib.check(_lib.load().ga_latent_sgd_momentum(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(g.data_ptr()),
                                                  ctypes.c_void_p(m.data_ptr()), float(LR), float(MU), int(first),
                                                  ctypes.c_void_p(out.data_ptr()), x.numel(), _lib.dtype_code(x),
                                                  _lib.stream_ptr()), "ga_latent_sgd_momentum")
    return out


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("n", SIZES)
def test_kernel_steps_against_fp64(n, dt):
    """Three steps (first = 1, then two with the velocity read back); each step's fp64 reference starts from the GPU's own
    previous velocity buffer and previous output, so errors do not chain."""
    from guided_attention_amd import ops
    x, _ = inputs(n, dt, 100 + n)
    m = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
    for k in range(3):
        _, g = inputs(n, dt, 200 + 10 * k + n)
        b_old = m.clone()
        out = ops.latent_sgd_momentum(x, g, m, LR, MU, k == 0)
        assert out.dtype == x.dtype and out.shape == x.shape and out.data_ptr() != x.data_ptr()
        b64, o64, bound_b, bound_o = step_reference(x, g, b_old, k == 0)
        err_b, err_o = np.abs(f64(m) - b64), np.abs(f64(out) - o64)
        print(f"[measured] sgd_momentum {dt} n={n} step {k}: velocity {np.max(err_b / np.maximum(bound_b, 1e-300)):.3f} "
              f"output {np.max(err_o / (bound_o + half_ulp(o64, dt))):.3f} of the bound")
        assert (err_b <= bound_b).all(), (k, err_b.max())
        assert (err_o <= bound_o + half_ulp(o64, dt)).all(), (k, err_o.max())
        x = out


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_first_step_never_reads_the_velocity_buffer(dt):
    from guided_attention_amd import ops
    for n in (257, 16384):
        x, g = inputs(n, dt, 300 + n)
        m = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
        out = ops.latent_sgd_momentum(x, g, m, LR, MU, True)
        assert torch.equal(m.view(torch.int32), g.float().view(torch.int32))      # momentum == float32(g), bit for bit
        assert torch.isfinite(out.float()).all()


def test_three_chained_steps_against_torch_sgd():
    """f32 against torch.optim.SGD(lr, momentum=0.8) in fp32 on the CPU over three chained steps.  Allowed: three times the
    per-step bounds — the sum over the steps of 2^-23 (|mu b_old| + |g|) for the velocity and of 2^-23 (|x| + |lr b|) for the
    latents, taken from SGD's own values (a velocity difference is carried into the next step with weight mu < 1)."""
    from guided_attention_amd import ops
    n = 4356
    x0, _ = inputs(n, "f32", 400)
    grads = [inputs(n, "f32", 410 + k)[1] for k in range(3)]
    p = torch.nn.Parameter(x0.cpu().clone())
    opt = torch.optim.SGD([p], lr=float(LR), momentum=float(MU))
    x, m = x0, torch.empty(n, dtype=torch.float32, device="cuda")
    allowed_b, allowed_x = np.zeros(n), np.zeros(n)
    for k, g in enumerate(grads):
        b_prev = np.zeros(n) if k == 0 else opt.state[p]["momentum_buffer"].numpy().astype(np.float64)
        x_prev = p.detach().numpy().astype(np.float64)
        p.grad = g.cpu().clone()
        opt.step()
        b_now = opt.state[p]["momentum_buffer"].numpy().astype(np.float64)
        allowed_b += EPS * (np.abs(np.float64(MU) * b_prev) + np.abs(f64(g)))
        allowed_x += EPS * (np.abs(x_prev) + np.abs(np.float64(LR) * b_now))
        x = ops.latent_sgd_momentum(x, g, m, LR, MU, k == 0)
    err_b = np.abs(f64(m) - opt.state[p]["momentum_buffer"].numpy().astype(np.float64))
    err_x = np.abs(f64(x) - p.detach().numpy().astype(np.float64))
    print(f"[measured] three chained steps vs torch SGD: velocity {np.max(err_b / allowed_b):.3f} latents "
          f"{np.max(err_x / allowed_x):.3f} of three per-step bounds")
    assert (err_b <= allowed_b).all() and (err_x <= allowed_x).all()


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_out_may_alias_latents(dt):
    for n, first in ((255, True), (4356, False), (16384, False)):
        x, g = inputs(n, dt, 500 + n)
        m0 = torch.from_numpy(hashrand.normalish((n,), 503 + n)).cuda()
        m1, m2, x2 = m0.clone(), m0.clone(), x.clone()
        ref = launch(x, g, m1, first)
        assert launch(x2, g, m2, first, out=x2) is x2
        assert torch.equal(x2.view(torch.int16 if dt != "f32" else torch.int32), ref.view(torch.int16 if dt != "f32" else torch.int32))
        assert torch.equal(m1.view(torch.int32), m2.view(torch.int32))


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_pointers_offset_by_one_element_match_the_aligned_launch(dt):
    """latents, grad and the velocity buffer as `[1:]` slices (no pointer 16-byte aligned: the element-wise path) against the
    launch on aligned copies of the same values (the 16-byte path and its tail): the same bits."""
    bits = torch.int32 if dt == "f32" else torch.int16
    for n, first in ((255, False), (4356, False), (4356, True)):
        xp, gp = inputs(n, dt, 600 + n, pad=1)
        mp = torch.from_numpy(hashrand.normalish((n + 1,), 603 + n)).cuda()
        xs, gs, ms = xp[1:], gp[1:], mp[1:]
        assert all(t.data_ptr() % 16 != 0 and t.is_contiguous() for t in (xs, gs, ms))
        xa, ga, ma = xs.clone(), gs.clone(), ms.clone()
        assert all(t.data_ptr() % 16 == 0 for t in (xa, ga, ma))
        from guided_attention_amd import ops
        out_s = ops.latent_sgd_momentum(xs, gs, ms, LR, MU, first)
        out_a = ops.latent_sgd_momentum(xa, ga, ma, LR, MU, first)
        assert torch.equal(out_s.view(bits), out_a.view(bits)) and torch.equal(ms.view(torch.int32), ma.view(torch.int32))
        assert mp[0].item() == hashrand.normalish((n + 1,), 603 + n)[0]          # the element in front is untouched


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_two_launches_are_bit_identical(dt):
    from guided_attention_amd import ops
    bits = torch.int32 if dt == "f32" else torch.int16
    n = 16384
    x, g = inputs(n, dt, 700)
    m0 = torch.from_numpy(hashrand.normalish((n,), 703)).cuda()
    m1, m2 = m0.clone(), m0.clone()
    o1 = ops.latent_sgd_momentum(x, g, m1, LR, MU, False)
    o2 = ops.latent_sgd_momentum(x, g, m2, LR, MU, False)
    assert torch.equal(o1.view(bits), o2.view(bits)) and torch.equal(m1.view(torch.int32), m2.view(torch.int32))


def test_wrapper_refuses_a_wrong_velocity_buffer():
    from guided_attention_amd import ops
    x, g = inputs(64, "f16", 800)
    with pytest.raises(ops.GaError, match="velocity buffer"):
        ops.latent_sgd_momentum(x, g, torch.zeros(64, dtype=torch.float16, device="cuda"), LR, MU, True)
    with pytest.raises(ops.GaError, match="velocity buffer"):
        ops.latent_sgd_momentum(x, g, torch.zeros(32, dtype=torch.float32, device="cuda"), LR, MU, True)


# ------------------------------------------------------------------------------------------ the pipeline
@pytest.fixture(scope="module")
def g9_momentum():
    """The fp32 product on `momentum_g9`, eager: one run shared by the parity test and the variants."""
    meta = G12["momentum_g9"]
    setup = g9_setup(meta)
    pipe = build_product(setup[0], torch.float32)
    out, _ = run_product(pipe, meta, *setup[1:])
    return SimpleSetup(meta, setup, pipe, out)


class SimpleSetup:
    def __init__(self, meta, setup, pipe, out):
        self.meta, self.setup, self.pipe, self.out = meta, setup, pipe, out


def test_fp32_pipeline_matches_the_reference_momentum_call(g9_momentum):
    """The reference's `__call__` with use_optimizer on g9's `no_recurse_thr2`: 20 optimizer steps in two refinement calls (both
    run into the cap of 10) and two plain updates.  The product's backward count is the fixture's `bwd` (plain updates) plus its
    `optimizer_steps`.  Final latents within 5e-3 (max |d| / max |ref|), the project's bar for fp32 GPU against the fp32 CPU
    reference.  The case has two refinement calls, each of which the reference starts with a new optimizer: a velocity carried
    from the first call into the second ends 3.3e-2 from the reference (measured once on the MI355X with the re-arming taken
    out; re-armed per call: 4.0e-6) and fails this bar, as does the plain branch (2.0e-1 away: tests/golden/g9_loop.*)."""
    meta, out = g9_momentum.meta, g9_momentum.out
    assert meta["optimizer_steps"] == 20 and meta["bwd"] == 2
    assert (out.unet_calls["fwd_b1_grad"], out.unet_calls["fwd_b2"]) == (meta["fwd_b1"], meta["fwd_b2"])
    assert out.unet_calls["bwd"] == meta["bwd"] + meta["optimizer_steps"]
    ref = load_npz("g12_momentum.npz")["momentum_g9.final_latents"]
    err = np.abs(out.latents.float().cpu().numpy() - ref).max() / np.abs(ref).max()
    print(f"[measured] fp32 momentum pipeline vs reference: latents max-rel {err:.3e}")
    assert err < 5e-3, err
    assert out.census.get("latent_sgd_momentum", 0) == meta["optimizer_steps"] and out.census.get("latent_axpy", 0) == meta["bwd"]


@pytest.mark.parametrize("variant", ["graphs", "graphs-no-run-ahead"])
def test_momentum_variants_are_result_identical(g9_momentum, variant):
    """Eager, the hipGraph runner with the run-ahead loop, and the runner that reads each loss before it enqueues the next step:
    the same counters, the same launches (one momentum launch per optimizer step, one plain axpy per caller update), nothing
    speculated, latents within the run-to-run band of test_variants_are_result_identical."""
    meta, base, pipe = g9_momentum.meta, g9_momentum.out, g9_momentum.pipe
    try:
        pipe.speculative_refinement, pipe.discarded_speculations = variant == "graphs", 0
        out, _ = run_product(pipe, meta, *g9_momentum.setup[1:], use_graphs=True)
        assert pipe._runner is not None
        assert pipe.discarded_speculations == 0
    finally:
        pipe.use_graphs, pipe.speculative_refinement = False, True
    assert {k: out.unet_calls[k] for k in MAIN_CALLS} == {k: base.unet_calls[k] for k in MAIN_CALLS}
    for o in (base, out):
        assert o.census.get("latent_sgd_momentum", 0) == meta["optimizer_steps"]
        assert o.census.get("latent_axpy", 0) == meta["bwd"]
    err = (out.latents - base.latents).abs().max().item() / base.latents.abs().max().item()
    print(f"[measured] momentum {variant} vs eager: latents max-rel {err:.3e}")
    assert err < 2e-4, err


_WIDE = {}


@pytest.mark.parametrize("dt,tol", [("f16", 2.5e-2), ("bf16", 2.0e-1)])
def test_half_precision_momentum_pipeline_vs_reference(dt, tol):
    """f16 / bf16 with use_graphs=True on the 64/64/128/128 UNet (own Linear / convolution kernels at every level) against the
    reference's fp32 latents of `momentum_wide` (3 denoising steps, two refinement calls of 10 optimizer steps; every branch
    decision of the reference at least 21 % clear of its threshold).  Stated tolerance: max |dlatent| / max |latent|, twice the
    bound test_half_precision_pipeline_vs_oracle holds for the plain refinement (1.25e-2 f16, 1.0e-1 bf16): an error in a
    gradient enters the plain update once with weight step, the momentum update through the velocity with weights
    lr (1 + mu + mu^2 + ...) -> (step / 2.5) / (1 - 0.8) = 2 step.
    The same tree's plain refinement (the same case without use_optimizer, against the reference's plain run) is measured next
    to it.  Measured on the MI355X: momentum f16 5.0e-3 / bf16 3.3e-2, plain f16 4.1e-3 / bf16 4.3e-2."""
    import copy
    meta = G12["momentum_wide"]
    g = load_npz("g12_momentum.npz")
    if not _WIDE:
        _WIDE["setup"] = wide_setup(meta)
    unet, embeds, lat0, noise, thr = _WIDE["setup"]
    plain_meta = dict(meta, hyper={k: v for k, v in meta["hyper"].items() if k != "use_optimizer"})
    pipe = build_product(copy.deepcopy(unet), DTYPES[dt])
    flags = dict(use_graphs=True, batch_loss_only_guidance=True)
    out, _ = run_product(pipe, meta, embeds, lat0, noise, thr, **flags)
    assert pipe._runner is not None and pipe.discarded_speculations == 0
    plain, _ = run_product(pipe, plain_meta, embeds, lat0, noise, thr, **flags)

    def rel(o, ref):
        return np.abs(o.latents.float().cpu().numpy() - ref).max() / np.abs(ref).max()
    err, err_plain = rel(out, g["momentum_wide.final_latents"]), rel(plain, g["momentum_wide.plain_final_latents"])
    print(f"[measured] half-precision momentum pipeline {dt} graphs: latents max-rel {err:.3e}; plain refinement, same case: "
          f"{err_plain:.3e}")
    assert (out.unet_calls["fwd_b1_grad"], out.unet_calls["fwd_b2"]) == (meta["fwd_b1"], meta["fwd_b2"])
    assert out.unet_calls["bwd"] == meta["bwd"] + meta["optimizer_steps"]
    assert out.census.get("latent_sgd_momentum", 0) == meta["optimizer_steps"] and out.census.get("latent_axpy", 0) == meta["bwd"]
    assert out.census.get("linear", 0) > 0 and out.census.get("conv3x3", 0) > 0
    assert (plain.unet_calls["fwd_b1_grad"], plain.unet_calls["bwd"], plain.unet_calls["fwd_b2"]) == \
        (meta["plain"]["fwd_b1"], meta["plain"]["bwd"], meta["plain"]["fwd_b2"])
    assert plain.census.get("latent_sgd_momentum", 0) == 0
    assert err < tol, err
