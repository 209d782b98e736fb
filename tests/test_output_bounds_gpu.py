"""Where the HIP kernels put their results: every entry point that ops.py hands a freshly allocated output runs under
tests/guarded_alloc.py (outputs carved from 0xFF-filled arenas with 4 KiB red zones on both sides), at the small ragged shapes
where tiles, vectors and batches end.  Four assertions per case:
  1. no byte of any red zone changed (a partial tile written whole, a tail rounded up to the vector width, scratch indexed one
     block too far),
  2. every allocation is written in full (returned tensors, gradient buffers, statistics, side outputs: a plan that skips the
     stores of a partial last tile, of a tail, of one image — invisible to the value tests, whose output block the caching
     allocator refills with an earlier, correct result),
  3. the inputs are bit-identical afterwards,
  4. the result agrees with fp64 on the CPU at the tolerance of the op's own test in test_kernels_gpu.py (TOL, close, dev are
     imported from there).
No case may allocate 32 MiB or more inside the guard (that would pass through unguarded): asserted.

UNDEFINED ELEMENTS (the only masks; each rests on a sentence of include/ga_hip.h)
  allocation                                    mask built from                          header sentence
  GroupNormAct.forward / .backward `ws`         B, HW, C, G, dtype, direction of the     "workspace GA_GN_WORKSPACE_FLOATS(B, G) f32 scratch:
  (B * 257 * G * 2 floats, never returned)      launch: slots past B * NB * G * 2        [B][NB][G][2] partial sums for the NB pixel blocks
                                                (`gn_workspace_undefined`)               the launch uses, the slots behind them unspecified"
Nothing else is masked: terms rows past an image's T and rel_terms rows past its R are declared ZERO by the header and are
checked as written; partial sums (B, blocks, G, 2) and row partials (M, parts, 2) are written for every block the `_blocks`
query / `parts` names.

LAUNCH NAME -> CASES
  ga_attn_capture_fwd / _bwd / _bwd_strided          test_attn_capture, test_batched_loss_backward_reaches_the_capture_kernel
  ga_attn_scores_max, ga_attn_capture_{fwd,bwd}_biased          test_paint_with_words
  ga_attn_scores_max_grouped, ga_attn_capture_{fwd,bwd}_biased_grouped, ga_attn_pww_max_grad (in place)   test_paint_with_words_grouped
  ga_aggregate_maps, ga_smooth_loss_fwd / _bwd, ga_aggregate_loss_fwd          test_loss_single_image
  ga_aggregate_loss_fwd_batched, ga_smooth_loss_bwd_batched                    test_loss_batched
  ga_aggregate_loss_fwd_images, ga_smooth_loss_bwd_images                      test_loss_image_table
  ga_aggregate_loss_rel_fwd_images, ga_smooth_loss_rel_bwd_images              test_loss_relation_table
  ga_latent_axpy, ga_latent_axpby, ga_cfg_ddim_step                            test_latent_ops
  ga_latent_axpy_batched, ga_latent_axpby_masked, ga_cfg_ddim_step_masked      test_latent_ops_batched_and_masked
  ga_latent_sgd_momentum (momentum in place)                                   test_latent_sgd_momentum
  ga_self_attn_fwd / _bwd                                                      test_self_attention (separate and fused-QKV forms)
  ga_group_norm_fwd / _bwd                                                     test_group_norm
  ga_group_norm_apply, ga_conv3x3_nhwc_gn                                      test_conv3x3_gn_epilogue
  ga_geglu_fwd / _bwd                                                          test_geglu
  ga_bias_residual_add                                                         test_bias_residual_add
  ga_cat_channels, ga_cat_channels_gn, ga_cat_group_norm_fwd                   test_cat_channels
  ga_add_layer_norm_fwd / _bwd                                                 test_layer_norm
  ga_conv3x3_nhwc, ga_conv3x3_pack_weights                                     test_conv3x3
  ga_conv3x3_up2x_nhwc                                                         test_upsample_conv3x3
  ga_conv3x3_thin_in / _out / _pack                                            test_thin_convolutions
  ga_gemm_nt                                                                   test_gemm_nt
  ga_linear_fused                                                              test_linear_fused, test_linear_fused_gn_epilogue,
                                                                               test_linear_fused_strided_views, test_linear_stream_form
  allocate nothing on the device: ga_version, ga_strerror, ga_loss_lds_plan, ga_gaussian_weights, ga_conv3x3_plan,
  ga_splitk_workspace_floats, ga_linear_workspace, ga_conv3x3_packed_elems, ga_conv3x3_thin_packed_elems,
  ga_conv3x3_thin_supported, ga_conv3x3_gn_blocks, ga_linear_gn_blocks, ga_cat_channels_gn_blocks, ga_group_norm_one_launch,
  ga_group_norm_two_launch (host-side queries).
"""
import contextlib
import ctypes
import math

import numpy as np
import pytest
import torch

import hashrand
from guarded_alloc import RED, assert_copy_written, assert_intact, guarded, snapshot, unwritten_mask
from oracle import attention as oattn
from oracle import loss as oloss
from test_kernels_gpu import DT, STREAM_CASES, TOL, _fold, _gelu64, close, dev, from_bh, make_qkv, to_bh

pytestmark = pytest.mark.gpu

ALL = ["f32", "f16", "bf16"]
HALF = ["f16", "bf16"]
ids = lambda s: "x".join(map(str, s))  # noqa: E731


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from guided_attention_amd import ops as _ops
    _ops.load()
    _ops.prepare_device("cuda")     # the persistent 256 MB split-K slabs and the ticket words exist before any guard
    return _ops


def gn_blocks_in_use(HW, C, G, dtype, backward):
    """NB of the header's workspace sentence, from the launch's arguments (group_norm.hip: small_path / wide_ok / WideGeom /
    geometry): 0 where a group's slab stays in LDS (one launch, the workspace is not touched), else the pixel blocks of the
    statistics launch — the wide 16-bit path's or the generic one's."""
    cg, eb = C // G, 4 if dtype == torch.float32 else 2
    slab = 4 + (eb if backward else 0)
    if HW <= 1024 and cg % 2 == 0 and cg <= 2048 and HW * cg <= 20480 and 128 + slab * HW * cg <= 160 * 1024:
        return 0
    fill = -(-HW // 128)
    if eb == 2 and C % 8 == 0 and cg >= 8 and C <= 2048:
        per_block = max(fill, 8 * (256 // (C // 8)))
    else:
        per_block = max(fill, 8)
    return -(-HW // per_block)


def gn_workspace_undefined(B, HW, C, G, dtype):
    """The one mask (table above): of GroupNormAct's workspaces of B * 257 * G * 2 floats, the slots behind the
    [B][NB][G][2] partial sums in use.  The blocks in use must be written like any output."""
    def undefined(arena):
        if arena.asked_by not in ("GroupNormAct.forward", "GroupNormAct.backward") or arena.dtype != torch.float32 or \
                arena.shape != (B * 257 * G * 2,):
            return None
        nb = gn_blocks_in_use(HW, C, G, dtype, arena.asked_by.endswith("backward"))
        assert nb <= 257
        return torch.arange(arena.shape[0]) >= B * nb * G * 2
    return undefined


@contextlib.contextmanager
def bounds(ops, *inputs, undefined=lambda arena: None):
    """Run the body with ops' allocations guarded; afterwards: red zones, every allocation written, inputs intact, nothing
    large passed through."""
    snap = snapshot(*inputs)
    with guarded(ops) as g:
        yield g
        g.assert_all_written(undefined)
    assert g.arenas, "the case allocated nothing through ops: it checks nothing"
    assert_intact(snap)
    assert g.large_passthroughs == 0


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def f64(t):
    return t.detach().double().cpu()


# ===================================================================================== latent ops
# latent_ops.hip: axpy / axpby / cfg_ddim and the masked forms are grid-stride loops over single elements (`i < n`): n = 1 is one
# thread of one block, 7 a partial wave, 1000 three full blocks and a partial one, 4*16*16+3 = 1027 an odd count behind whole
# blocks.  axpy with absmean and axpy_batched are ONE 1024-thread block per image striding by 1024 (1027: three elements in the
# second trip).  sgd_momentum takes 16-byte vectors for n / N whole vectors and a scalar tail behind them (7 = 0 vectors of 8 + 7
# for 16 bits, 1 + 3 for f32; 1027 = 128 vectors + 3).
@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("n", [1, 7, 1000, 4 * 16 * 16 + 3])
def test_latent_ops(ops, dt, n):
    x, y, z = (dev(hashrand.normalish((n,), s), DT[dt]) for s in (1, 2, 3))
    xs, ys, zs = f64(x).numpy(), f64(y).numpy(), f64(z).numpy()
    a_t, a_p, gs = 0.35, 0.52, 7.5
    eps = xs + gs * (ys - xs)
    x0r = (zs - math.sqrt(1 - a_t) * eps) / math.sqrt(a_t)
    prevr = math.sqrt(a_p) * x0r + math.sqrt(1 - a_p) * eps
    with bounds(ops, x, y, z) as g:
        out, am = ops.latent_axpy(x, y, 17.3, True)
        out2, _ = ops.latent_axpy(x, y, 17.3, False)
        ab = ops.latent_axpby(x, y, 0.8, 0.6)
        prev, x0 = ops.cfg_ddim_step(x, y, gs, z, a_t, a_p, True)
        prev2, _ = ops.cfg_ddim_step(x, y, gs, z, a_t, a_p, False)
        for t, what in ((out, "axpy"), (am, "absmean"), (out2, "axpy, no absmean"), (ab, "axpby"), (prev, "prev"), (x0, "x0"),
                        (prev2, "prev, no x0")):
            g.assert_written(t, what)
    close(out, xs - 17.3 * ys, TOL[dt], "axpy")
    assert torch.equal(out, out2) and torch.equal(prev, prev2)
    np.testing.assert_allclose(am.item(), np.abs(ys).mean(), rtol=1e-4)
    close(ab, 0.8 * xs + 0.6 * ys, TOL[dt], "axpby")
    close(x0, x0r, TOL[dt], "x0")
    close(prev, prevr, TOL[dt], "prev")


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("n", [1, 7, 1000, 4 * 16 * 16 + 3])
def test_latent_ops_batched_and_masked(ops, dt, n):
    """S = 3 images, the middle one inactive (it must come out as a bit copy: its stores are a separate loop)."""
    S = 3
    x, y, z = (dev(hashrand.normalish((S, n), s), DT[dt]) for s in (4, 5, 6))
    xs, ys, zs = f64(x).numpy(), f64(y).numpy(), f64(z).numpy()
    active = torch.tensor([1, 0, 1], dtype=torch.int32, device="cuda")
    step = torch.tensor([17.3, 5.0, 0.25], dtype=torch.float32, device="cuda")
    on = np.array([1.0, 0.0, 1.0])[:, None]
    a_t, a_p, gs = 0.35, 0.52, 7.5
    eps = xs + gs * (ys - xs)
    x0r = (zs - math.sqrt(1 - a_t) * eps) / math.sqrt(a_t)
    prevr = math.sqrt(a_p) * x0r + math.sqrt(1 - a_p) * eps
    with bounds(ops, x, y, z, active, step) as g:
        out, am = ops.latent_axpy_batched(x, y, step, active, True)
        ab = ops.latent_axpby_masked(x, y, 0.8, 0.6, active)
        prev, x0 = ops.cfg_ddim_step_masked(x, y, gs, z, a_t, a_p, active, True)
        for t, what in ((out, "axpy_batched"), (ab, "axpby_masked"), (prev, "prev"), (x0, "x0")):
            g.assert_written(t, what)
    close(out, np.where(on > 0, xs - f64(step).numpy()[:, None] * ys, xs), TOL[dt], "axpy_batched")
    np.testing.assert_allclose(am.cpu().numpy()[[0, 2]], np.abs(ys).mean(1)[[0, 2]], rtol=1e-4)
    close(ab, np.where(on > 0, 0.8 * xs + 0.6 * ys, xs), TOL[dt], "axpby_masked")
    close(prev, np.where(on > 0, prevr, zs), TOL[dt], "prev masked")
    close(x0, x0r, TOL[dt], "x0 masked")       # every image's x0 estimate, the inactive one's included (include/ga_hip.h)
    assert torch.equal(out[1], x[1]) and torch.equal(ab[1], x[1]) and torch.equal(prev[1], z[1])


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("n", [1, 7, 1000, 4 * 16 * 16 + 3])
def test_latent_sgd_momentum(ops, dt, n):
    """The velocity buffer is the caller's and is updated in place (exempt from `inputs intact`): it is carved from a guarded
    arena here, so a vector store past its tail is seen; with first = 1 it is not read and must be written in full."""
    x, gr = (dev(hashrand.normalish((n,), s), DT[dt]) for s in (7, 8))
    xs, gs = f64(x).numpy(), f64(gr).numpy()
    lr, mu = 0.05, 0.9
    with bounds(ops, x, gr) as g:
        m = g.carve((n,), torch.float32, "cuda", "the velocity buffer")
        o1 = ops.latent_sgd_momentum(x, gr, m, lr, mu, True)
        g.assert_written(m, "velocity after the first step")
        m1 = f64(m).numpy()
        o2 = ops.latent_sgd_momentum(o1, gr, m, lr, mu, False)
        g.assert_written(o1, "latents, first step")
        g.assert_written(o2, "latents, second step")
    close(m1, gs, TOL["f32"], "velocity 1")
    close(o1, xs - lr * gs, TOL[dt], "latents 1")
    close(m, mu * m1 + gs, TOL["f32"], "velocity 2")
    close(o2, f64(o1).numpy() - lr * (mu * m1 + gs), TOL[dt], "latents 2")


# ===================================================================================== element-wise epilogues (ff_ops.hip)
# geglu / bias_residual_add: grid-stride loops over whole 16-byte vectors (F resp. C must be a multiple of the vector: there is no
# scalar tail in the kernel, the last vector IS the tail).  (1,1,16): two (f16) or four (f32) vectors, one partial wave;
# (3,7,64): 21 rows; bias (1,8,1,1): ONE vector in 16 bits; (1,64,3,5): 15 pixels x 8 vectors.
@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("shape", [(3, 7, 64), (1, 1, 16)], ids=ids)
def test_geglu(ops, shape, dt):
    B, N, F = shape
    x = dev(hashrand.normalish((B, N, 2 * F), 21 + F) * 1.5, DT[dt])
    gy = dev(hashrand.normalish((B, N, F), 22 + F), DT[dt])
    xr = f64(x).requires_grad_(True)
    h, gate = xr.chunk(2, dim=-1)
    yr = h * torch.nn.functional.gelu(gate)
    yr.backward(f64(gy))
    xa = x.clone().requires_grad_(True)
    with bounds(ops, x, gy) as g:
        y = ops.geglu(xa)
        (dx,) = torch.autograd.grad(y, [xa], gy)
        dx2 = ops.geglu_backward(x, gy)
        g.assert_written(y, "y")
        g.assert_written(dx2, "dx (geglu_backward)")
        assert_copy_written(dx, "dx")
    close(y, yr.detach().numpy(), TOL[dt], "geglu")
    close(dx, xr.grad.numpy(), TOL[dt] * 2, "geglu dx")
    assert torch.equal(dx, dx2)


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("shape", [(1, 64, 3, 5), (1, 8, 1, 1)], ids=ids)
def test_bias_residual_add(ops, shape, dt):
    B, C, H, W = shape
    y = cl(dev(hashrand.normalish(shape, 31 + C), DT[dt]))
    r = cl(dev(hashrand.normalish(shape, 32 + C), DT[dt]))
    bias = dev(hashrand.normalish((C,), 33), DT[dt])
    with bounds(ops, y, r, bias) as g:
        out = ops.bias_residual_add(y, bias, r)
        out0 = ops.bias_residual_add(y, None, r)
        g.assert_written(out, "out")
        g.assert_written(out0, "out, no bias")
    assert out.is_contiguous(memory_format=torch.channels_last)
    close(out, (f64(y) + f64(bias)[None, :, None, None] + f64(r)).numpy(), TOL[dt], "y + bias + residual")
    close(out0, (f64(y) + f64(r)).numpy(), TOL[dt], "no bias")


# cat_rows_kernel: four vectors per thread; threads whose four are all in range take the unconditional branch, the last few the
# `i < n` one; the two sources have their own counts (C1 != C2: the shorter source's threads run out first).
#   (1,8,16,3,5): 15 rows, 1 + 2 vectors (16 bits): everything in the conditional branch, one block
#   (2,64,32,50,64): the 50 x 64 map of the 768^2 configuration at 1/10 of its channels: 6400 rows, blocks of both branches,
#                    the GroupNorm behind it takes two launches -> ga_cat_channels_gn writes (B, blocks, G, 2) partial sums
#   (3,24,40,4,4): C1 != C2, 48 rows, the norm behind it is one launch -> ga_cat_group_norm_fwd writes cat, y and stats
@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("shape", [(1, 8, 16, 3, 5, 3), (2, 64, 32, 50, 64, 8), (3, 24, 40, 4, 4, 8)], ids=ids)
def test_cat_channels(ops, shape, dt):
    B, C1, C2, H, W, groups = shape       # groups: 8 channels per group at the first shape, 12 and 8 at the others
    T = DT[dt]
    a = cl(dev(hashrand.normalish((B, C1, H, W), 51 + C1), T))
    b = cl(dev(hashrand.normalish((B, C2, H, W), 52 + C2) * 1.7 + 0.4, T))
    ref = torch.cat([a, b], dim=1)
    assert ops.cat_channels_supported(a, b)
    with bounds(ops, a, b) as g:
        out = ops.cat_channels(a, b)
        g.assert_written(out, "cat")
    assert torch.equal(out, ref) and out.is_contiguous(memory_format=torch.channels_last)
    if dt == "f32":
        return
    gamma = dev(hashrand.normalish((C1 + C2,), 172) * 0.3 + 1.0, T)
    beta = dev(hashrand.normalish((C1 + C2,), 173) * 0.2, T)
    wide = ops.gn_two_launch(H * W, C1 + C2, groups, T)
    normed = torch.nn.functional.silu(torch.nn.functional.group_norm(f64(ref), groups, f64(gamma), f64(beta), 1e-5))
    with bounds(ops, a, b, gamma, beta, undefined=gn_workspace_undefined(B, H * W, C1 + C2, groups, T)) as g:
        y = ops.cat_channels(a, b, gn_for=groups, norm=(gamma, beta, 1e-5, True))
        made = dict(getattr(y, "_ga_gn", None) or {})
        assert made and ("partials" in made) == wide and ("done" in made) == (not wide), "neither fused form served the shape"
        g.assert_written(y, "cat")
        if wide:
            g.assert_written(made["partials"], "partial sums of ga_cat_channels_gn")
        else:
            g.assert_written(made["done"][0], "norm output of ga_cat_group_norm_fwd")
            g.assert_written(made["done"][1], "statistics of ga_cat_group_norm_fwd")
        z = ops.group_norm_act(y, gamma, beta, groups, 1e-5, True)
        g.assert_written(z, "norm on the concatenation's statistics")
    assert torch.equal(y, ref)
    close(z, normed.numpy(), TOL[dt] * 2, "norm behind the concatenation")
    if wide:
        yg = f64(ref).reshape(B, groups, -1)
        close(made["partials"][..., 0].sum(1), yg.sum(-1).numpy(), 2e-5, "sum")
        close(made["partials"][..., 1].sum(1), (yg * yg).sum(-1).numpy(), 2e-5, "sum of squares")


# ===================================================================================== LayerNorm
# layer_norm.hip: one wave per row, rows of C elements in 16-byte vectors; (1,1,8): ONE row of one (16 bit) / two (f32) vectors,
# 63 idle lanes and idle waves in the block; (3,5,64): 15 rows = not a multiple of the waves per block.
@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("shape", [(3, 5, 64), (1, 1, 8)], ids=ids)
def test_layer_norm(ops, shape, dt):
    B, N, C = shape
    a = dev(hashrand.normalish(shape, 41 + C) * 0.7, DT[dt])
    x = dev(hashrand.normalish(shape, 42 + C) * 1.3 + 0.2, DT[dt])
    w = dev(hashrand.normalish((C,), 43) * 0.4 + 1.0, DT[dt])
    b = dev(hashrand.normalish((C,), 44) * 0.2, DT[dt])
    gy, gx = (dev(hashrand.normalish(shape, s), DT[dt]) for s in (45, 46))
    sr = f64(a + x).requires_grad_(True)
    yr = torch.nn.functional.layer_norm(sr, (C,), f64(w), f64(b), 1e-5)
    torch.autograd.backward([sr * 1.0, yr], [f64(gx), f64(gy)])
    xr = f64(x).requires_grad_(True)
    ypr = torch.nn.functional.layer_norm(xr, (C,), f64(w), f64(b), 1e-5)
    ypr.backward(f64(gy))
    aa, xa, xp = (t.clone().requires_grad_(True) for t in (a, x, x))
    with bounds(ops, a, x, w, b, gy, gx) as g:
        xnew, y = ops.add_layer_norm(aa, xa, w, b, 1e-5)
        da, dxa = torch.autograd.grad([xnew, y], [aa, xa], [gx, gy])
        yp = ops.layer_norm(xp, w, b, 1e-5)
        (dxp,) = torch.autograd.grad(yp, [xp], gy)
        with torch.no_grad():
            yi = ops.layer_norm(x, w, b, 1e-5)      # inference: no statistics buffer
        for t, what in ((xnew, "a + x"), (y, "y"), (yp, "plain y"), (yi, "inference y")):
            g.assert_written(t, what)
        for t, what in ((da, "d a"), (dxa, "d x"), (dxp, "plain dx")):
            assert_copy_written(t, what)
    assert torch.equal(xnew.detach(), a + x) and torch.equal(da, dxa) and torch.equal(yi, yp.detach())
    close(y, yr.detach().numpy(), TOL[dt] * 2, "y")
    close(da, sr.grad.numpy(), TOL[dt] * 3, "d a")
    close(yp, ypr.detach().numpy(), TOL[dt] * 2, "plain y")
    close(dxp, xr.grad.numpy(), TOL[dt] * 3, "plain dx")


# ===================================================================================== GroupNorm
# group_norm.hip: small path (HW <= 1024, a group's slab in LDS: one launch) for (2,96,3,5) [3 channels per group is odd -> the
# generic path], (1,32,4,4) [ONE channel per group: generic], (2,512,17,19) [323 pixels, 16 channels per group: small path, odd
# pixel count]; (1,64,25,41) with 8 groups: 1025 pixels = the smallest pixel count past the small path's 1024 with >= 8 channels
# per group -> the two-launch wide path in 16 bits (partial blocks whose last one holds a single pixel row), the generic one in f32.
GN_SHAPES = [(2, 96, 3, 5, 32), (2, 512, 17, 19, 32), (1, 32, 4, 4, 32), (1, 64, 25, 41, 8)]


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("act", [True, False])
@pytest.mark.parametrize("shape", GN_SHAPES, ids=ids)
def test_group_norm(ops, shape, act, dt):
    B, C, H, W, G = shape
    T = DT[dt]
    if G == 8 and dt != "f32":
        assert ops.gn_two_launch(H * W, C, G, T) and not ops.gn_two_launch(H * W - 1, C, G, T)
    x = cl(dev(hashrand.normalish((B, C, H, W), 7 + C) * 1.7 + 0.3, T))
    w = dev(hashrand.normalish((C,), 8) * 0.5 + 1.0, T)
    b = dev(hashrand.normalish((C,), 9) * 0.2, T)
    cb = dev(hashrand.normalish((B, C), 11) * 0.7, T)
    gy, g2 = (cl(dev(hashrand.normalish((B, C, H, W), s), T)) for s in (10, 12))

    def ref(bias):
        xr = (f64(x) + (f64(bias)[:, :, None, None] if bias is not None else 0.0)).requires_grad_(True)
        yr = torch.nn.functional.group_norm(xr, G, f64(w), f64(b), 1e-5)
        yr = torch.nn.functional.silu(yr) if act else yr
        yr.backward(f64(gy))
        return yr.detach().numpy(), xr.grad.numpy()

    for bias in (None, cb):
        yr, dxr = ref(bias)
        xa, xc = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        with bounds(ops, x, w, b, cb, gy, g2, undefined=gn_workspace_undefined(B, H * W, C, G, T)) as g:
            y = ops.group_norm_act(xa, w, b, G, 1e-5, act, bias)
            (dx,) = torch.autograd.grad(y, [xa], gy)
            y4, alias = ops.group_norm_act(xc, w, b, G, 1e-5, act, bias, True)
            (dxs,) = torch.autograd.grad([y4, alias], [xc], [gy, g2])
            g.assert_written(y, "y")
            g.assert_written(y4, "y (with_alias)")
            assert_copy_written(dx, "dx")
            assert_copy_written(dxs, "dx + skip-connection gradient")
        tag = "with chan_bias" if bias is not None else "plain"
        assert y.is_contiguous(memory_format=torch.channels_last) and torch.equal(y4, y) and torch.equal(alias.detach(), x)
        close(y, yr, TOL[dt] * 2, f"y {tag}")
        close(dx, dxr, TOL[dt] * 3, f"dx {tag}")
        close(dxs, dxr + f64(g2).numpy(), TOL[dt] * 3, f"dx + skip-connection gradient {tag}")


# ===================================================================================== self-attention (flash kernels)
# self_attn.hip: query tiles x key tiles with the last of each ragged.  (1,1,2,8): two rows of one tile, the smallest head;
# (1,3,77,8): one ragged query tile, three heads interleaved in a row (a head's 8 columns are ONE 16-byte vector: a store of a
# neighbouring head's column would show in O); (1,2,130,16): two full 64-row tiles + 2 rows; (1,2,65,128): the 128-wide head
# (16 bit only), 64 + 1 rows; (2,2,200,48): two images, three full tiles + 8 rows, a head width that is no power of two.
# lse and delta (B*H, N) f32: rows N .. tile end must not be stored (the next head's rows follow directly).
SA_SHAPES = [(1, 1, 2, 8), (1, 3, 77, 8), (1, 2, 130, 16), (1, 2, 65, 128), (2, 2, 200, 48)]


@pytest.mark.parametrize("shape,dt", [(s, dt) for s in SA_SHAPES for dt in ALL if not (dt == "f32" and s[3] > 80)],
                         ids=lambda v: v if isinstance(v, str) else ids(v))     # the f32 build covers head_dim <= 80
def test_self_attention(ops, shape, dt):
    B, H, N, D = shape
    T = DT[dt]
    q, k, v, d_o = (dev(hashrand.normalish((B, N, H * D), s + N) * sp, T) for s, sp in ((11, 1.5), (12, 1.5), (13, 1.0), (14, 1.0)))
    scale = D ** -0.5
    Q, K, V = to_bh(q, H), to_bh(k, H), to_bh(v, H)
    _, Oref = oattn.capture_fwd_numpy(Q, K, V, scale)
    S = scale * np.einsum("bnd,bmd->bnm", Q, K)
    lse_ref = (np.log(np.exp(S - S.max(-1, keepdims=True)).sum(-1)) + S.max(-1)) / np.log(2.0)
    dQ, dK, dV = oattn.full_bwd_numpy(Q, K, V, scale, to_bh(d_o, H))
    with bounds(ops, q, k, v, d_o) as g:
        o, lse = ops.self_attn_fwd(q, k, v, H, scale)
        o_only, none = ops.self_attn_fwd(q, k, v, H, scale, want_lse=False)
        dq, dk, dv = ops.self_attn_bwd(q, k, v, o, d_o, lse, H, scale)
        for t, what in ((o, "O"), (lse, "lse"), (o_only, "O without lse"), (dq, "dQ"), (dk, "dK"), (dv, "dV")):
            g.assert_written(t, what)
        delta = [a for a in g.arenas if a.asked_by == "self_attn_bwd" and a.shape == (B * H, N)]
        assert len(delta) == 1 and delta[0].dtype == torch.float32        # covered by assert_all_written and its red zones
    assert none is None and torch.equal(o, o_only)
    close(o, from_bh(Oref, B, H), TOL[dt], "O")
    np.testing.assert_allclose(lse.cpu().numpy(), lse_ref, rtol=0, atol={"f32": 2e-4, "f16": 2e-2, "bf16": 1e-1}[dt])
    close(dq, from_bh(dQ, B, H), TOL[dt] * 3, "dQ")
    close(dk, from_bh(dK, B, H), TOL[dt] * 3, "dK")
    close(dv, from_bh(dV, B, H), TOL[dt] * 3, "dV")
    # the fused-QKV form: the same kernels on column slices of one (B, N, 3C) tensor, dq | dk | dv into ONE buffer whose three
    # column thirds are written by different stores: each third's neighbours are the other two
    qkv = torch.cat([q, k, v], dim=-1).contiguous().requires_grad_(True)
    with bounds(ops, qkv.detach(), d_o) as g:
        of = ops.SelfAttentionFusedQKV.apply(qkv, H, scale)
        (d_qkv,) = torch.autograd.grad(of, [qkv], d_o)
        g.assert_written(of, "O (fused QKV)")
        assert_copy_written(d_qkv, "d qkv")
    assert torch.equal(of, o) and torch.equal(d_qkv, torch.cat([dq, dk, dv], dim=-1))


# ===================================================================================== attention capture
# attn_capture.hip: P (B*H, N, Kt) in the activation type with Kt = 5 / 1 / 80 / 81 elements per row — rows that are no multiple
# of a 16-byte vector and (Kt = 1, 5, 81) not even 4-byte aligned from the second row on: a row store rounded up to a vector
# overwrites the next row (seen in the values) and, on the last row, the back red zone.  N = 17 / 100: a ragged last query tile;
# Kt = 81: the 8-key-tile path with one key in the last tile.
CAP_SHAPES = [(1, 3, 17, 5, 8), (1, 1, 16, 1, 8), (1, 2, 100, 80, 24), (1, 2, 64, 81, 32)]
# the biased (paint-with-words) entry points serve Kt <= 80 (the mask belongs to the text context): 81 keys are refused, see
# test_paint_with_words_refuses_more_than_80_keys; 77 keys (the text encoder's width, 154-byte rows of P) stand in for them
PWW_SHAPES = CAP_SHAPES[:3] + [(1, 2, 64, 77, 32)]


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("shape", CAP_SHAPES, ids=ids)
def test_attn_capture(ops, shape, dt):
    B, H, N, Kt, D = shape
    T = DT[dt]
    q, k, v = make_qkv(B, H, N, Kt, D, T, 100 + N + D)
    d_o = dev(hashrand.normalish((B, N, H * D), 300 + N), T)
    dp = dev(hashrand.normalish((B * H, N, Kt), 400 + N), T)
    m = dev(hashrand.normalish((N, Kt), 500 + N) * 3e-3, T)
    scale = D ** -0.5
    Q, K, V = to_bh(q, H), to_bh(k, H), to_bh(v, H)
    Pref, Oref = oattn.capture_fwd_numpy(Q, K, V, scale)
    with bounds(ops, q, k, v, d_o, dp, m) as g:
        o, p = ops.attn_capture_fwd(q, k, v, H, scale, True)
        o2, none = ops.attn_capture_fwd(q, k, v, H, scale, False)
        g.assert_written(o, "O")
        g.assert_written(p, "P")
        g.assert_written(o2, "O without capture")
        dqs = {}
        for mode, dprobs in (("none", None), ("dense", dp), ("bcast", m.unsqueeze(0).expand(B * H, N, Kt))):
            dqs[mode] = ops.attn_capture_bwd(q, k, v, d_o, dprobs, H, scale)
            g.assert_written(dqs[mode], f"dQ ({mode})")
    assert none is None and torch.equal(o, o2) and p.shape == (B * H, N, Kt)
    close(p, Pref, TOL[dt], "P")
    close(o, from_bh(Oref, B, H), TOL[dt], "O")
    for mode, dp_np in (("none", None), ("dense", f64(dp).numpy()), ("bcast", np.broadcast_to(f64(m).numpy(), (B * H, N, Kt)))):
        dQ, _, _ = oattn.capture_bwd_numpy(Q, K, V, scale, to_bh(d_o, H), dp_np)
        close(dqs[mode], from_bh(dQ, B, H), TOL[dt] * 2, f"dQ ({mode})")
    # the autograd form (P differentiable; the placeholder for an absent P is a zero-size tensor: passes through)
    qa = q.clone().requires_grad_(True)
    with bounds(ops, q, k, v, d_o, dp) as g:
        oa, pa = ops.AttnCapture.apply(qa, k, v, H, scale, True)
        (dqa,) = torch.autograd.grad([oa, pa], [qa], [d_o, dp])
        g.assert_written(pa, "P (autograd)")
        assert_copy_written(dqa, "dQ (autograd)")
    assert torch.equal(dqa, dqs["dense"])


def _check_packed_maximum(value, arg, q, k, H, scale, dt, head_maps):
    """One decoded packed word (value, flat index into the call's [B*H][N][Kt]) against the fp64 scores of `head_maps`: the
    value at the bar of the kernel's type; the index inside those head-maps, at a score that IS the maximum up to that bar (ties
    and near-ties of the rounded accumulation allowed), and equal to the fp64 argmax where the runner-up is further away."""
    scores = scale * np.einsum("bnd,bmd->bnm", to_bh(q, H), to_bh(k, H))
    own = np.zeros(scores.shape, bool)
    own[list(head_maps)] = True
    best = np.where(own, scores, -np.inf)
    smax, bar = best.max(), TOL[dt] * abs(best.max())
    assert abs(value - smax) <= bar, (value, smax)
    assert 0 <= arg < scores.size and own.reshape(-1)[arg], (arg, "outside the group's head-maps")
    assert scores.reshape(-1)[arg] >= smax - bar, (arg, scores.reshape(-1)[arg], smax)
    flat = np.sort(best.reshape(-1))
    if flat.size == 1 or flat[-1] - flat[-2] > 2 * bar:
        assert arg == int(best.reshape(-1).argmax()), (arg, int(best.reshape(-1).argmax()))


def _pww_reference(q, k, v, H, scale, mask, mult, d_o, dp):
    """oracle.attention.attention_probs in fp64 with the maximum inside the autograd graph -> P, O, dq."""
    q64 = f64(q).requires_grad_(True)
    pww = (f64(mask), mult / .4) if mult else None
    P = oattn.attention_probs(oattn.head_split(q64, H), oattn.head_split(f64(k), H), scale, pww)
    O = oattn.head_merge(torch.bmm(P, oattn.head_split(f64(v), H)), H)
    ((O * f64(d_o)).sum() + (P * f64(dp)).sum()).backward()
    return P.detach().numpy(), O.detach().numpy(), q64.grad.numpy()


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("shape", PWW_SHAPES, ids=ids)
def test_paint_with_words(ops, shape, dt):
    """The biased capture kernels: the packed maximum (int64 word, allocated by torch.zeros: not guarded, checked by value),
    P, O and dq through AttnCapturePaintWithWords against fp64 with the maximum inside the graph."""
    B, H, N, Kt, D = shape
    T = DT[dt]
    q, k, v = make_qkv(B, H, N, Kt, D, T, 600 + N + D, 0.6)
    d_o = dev(hashrand.normalish((B, N, H * D), 610 + N), T)
    dp = dev(hashrand.normalish((B * H, N, Kt), 611 + N) * 0.5, T)
    mask = dev((hashrand.uniform((N, Kt), 612 + N) > 0.6).astype(np.float32) * 0.8, T)
    scale, mult = D ** -0.5, 0.45
    Pref, Oref, dqref = _pww_reference(q, k, v, H, scale, mask, mult, d_o, dp)
    qa = q.clone().requires_grad_(True)
    with bounds(ops, q, k, v, d_o, dp, mask) as g:
        value, arg = ops.attn_scores_max(q, k, H, scale)
        o, p = ops.AttnCapturePaintWithWords.apply(qa, k, v, H, scale, True, mask, mult)
        (dq,) = torch.autograd.grad([o, p], [qa], [d_o, dp])
        g.assert_written(o, "O")
        g.assert_written(p, "P")
        assert_copy_written(dq, "dQ")
    _check_packed_maximum(float(value), int(arg), q, k, H, scale, dt, range(B * H))
    close(p, Pref, TOL[dt], "P")            # the bars of the plain capture kernels (test_attn_capture_fwd / _bwd)
    close(o, Oref, TOL[dt], "O")
    close(dq, dqref, TOL[dt] * 2, "dQ")


@pytest.mark.parametrize("dt", ALL)
def test_paint_with_words_refuses_more_than_80_keys(ops, dt):
    """(1,2,64,81,32): a refusal before any launch, not a partly written P — the outputs allocated for the call stay 0xFF."""
    B, H, N, Kt, D = CAP_SHAPES[3]
    q, k, v = make_qkv(B, H, N, Kt, D, DT[dt], 650, 0.6)
    mask = dev(np.zeros((N, Kt), np.float32), DT[dt])
    coef = torch.ones(1, device="cuda")
    packed, mult = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.ones(1, device="cuda")
    with guarded(ops) as g:
        for call in (lambda: ops.attn_scores_max(q, k, H, D ** -0.5),
                     lambda: ops.attn_capture_fwd_biased(q, k, v, H, D ** -0.5, True, mask, coef),
                     lambda: ops.attn_capture_bwd_biased(q, k, v, q, None, H, D ** -0.5, mask, coef),
                     lambda: ops.attn_scores_max_grouped(q, k, H, D ** -0.5, 1),
                     lambda: ops.attn_capture_fwd_biased_grouped(q, k, v, H, D ** -0.5, True, mask, packed, mult),
                     lambda: ops.attn_capture_bwd_biased_grouped(q, k, v, q, None, H, D ** -0.5, mask, packed, mult)):
            with pytest.raises(ops.GaError):
                call()
        torch.cuda.synchronize()
        assert g.arenas and all(bool(unwritten_mask(a.arena[RED:RED + a.nbytes].view(a.dtype)).all()) for a in g.arenas)


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("shape", [(3,) + s[1:] for s in PWW_SHAPES], ids=ids)
def test_paint_with_words_grouped(ops, shape, dt):
    """Three images in one call (batch row b is image b), one mask and multiplier each, image 1 does not paint: each image
    against its own fp64 reference.  ga_attn_pww_max_grad works in place on dq (exempt from `intact`; dq is guarded)."""
    B, H, N, Kt, D = shape
    T = DT[dt]
    q, k, v = make_qkv(B, H, N, Kt, D, T, 700 + N + D, 0.6)
    d_o = dev(hashrand.normalish((B, N, H * D), 710 + N), T)
    dp = dev(hashrand.normalish((B * H, N, Kt), 711 + N) * 0.5, T)
    mask = dev(np.stack([(hashrand.uniform((N, Kt), 712 + N + i) > 0.6).astype(np.float32) * (0.8 - 0.2 * i) for i in range(B)]), T)
    mults = (0.45, 0.0, 0.7)
    mult = torch.tensor(mults, dtype=torch.float32, device="cuda")
    scale = D ** -0.5
    qa = q.clone().requires_grad_(True)
    with bounds(ops, q, k, v, d_o, dp, mask, mult) as g:
        packed = ops.attn_scores_max_grouped(q, k, H, scale, B)
        o, p = ops.AttnCapturePaintWithWordsImages.apply(qa, k, v, H, scale, True, mask, mult)
        (dq,) = torch.autograd.grad([o, p], [qa], [d_o, dp])
        g.assert_written(o, "O")
        g.assert_written(p, "P")
        assert_copy_written(dq, "dQ")
    values, index = ops.unpack_scores_max(packed)           # one word per image: its own maximum, indexed in the whole call
    assert packed.shape == (B,) and packed.dtype == torch.int64
    for i in range(B):
        _check_packed_maximum(float(values[i]), int(index[i]), q, k, H, scale, dt, range(i * H, (i + 1) * H))
    for i in range(B):
        rows = slice(i * H, (i + 1) * H)
        Pref, Oref, dqref = _pww_reference(q[i:i + 1], k[i:i + 1], v[i:i + 1], H, scale, mask[i], mults[i], d_o[i:i + 1], dp[rows])
        close(p[rows], Pref, TOL[dt], f"P image {i}")
        close(o[i:i + 1], Oref, TOL[dt], f"O image {i}")
        close(dq[i:i + 1], dqref, TOL[dt] * 2, f"dQ image {i}")


# ===================================================================================== aggregate + loss
# aggregate.hip / smooth_loss.hip: A (npix, Kt = 77) f32 — 77 floats per row, rows 4-byte aligned only; res 5 (25 pixels: less
# than a wave), 15 (225: odd, no multiple of anything) and 16 (256).  terms (T, 8), loss (1,): T = 1 and 3.  dA / dP_bcast
# (npix, 77) with dP_bcast in a 16-bit type: 154-byte rows.
ENTRIES = [{"index": 2, "kind": "BOX", "geom": (.6, .3, .4, .55), "subprompt": "robot"},
           {"index": 5, "kind": "BOX", "geom": (.2, .3, .4, .55), "subprompt": "blue vase"},
           {"index": 6, "kind": "COOR", "geom": (.3, .7), "subprompt": "blue vase"}]
TERM_KEYS = ("max", "col", "row", "inside", "outside", "token_loss", "unscaled")
KT = 77


def _maps(res, layout, images, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.softmax(torch.randn(images * h, res * res, KT, generator=g) * 3, -1).to("cuda", dtype) for h in layout]


def _mean_map(maps, images, s):
    """fp64 mean of image s's head-maps (image-major) -> (npix, Kt)."""
    parts = [f64(m).reshape(images, -1, *m.shape[1:])[s] for m in maps]
    return torch.cat(parts, 0).mean(0)


def _check_loss(terms, loss, dA, A64, entries, res, what, first_last=(1, KT - 1), dscale=1.0):
    """One image's terms / loss / dA against oracle.loss.loss_and_grad_numpy of the fp64 mean map."""
    last = first_last[1]
    ref, dref = oloss.loss_and_grad_numpy(A64.reshape(res, res, KT).numpy(), oloss.TokenPlan(entries),
                                          normalize_eot=last != KT - 1, n_prompt_tokens=last + 1)
    np.testing.assert_allclose(loss, ref["loss"], rtol=5e-5, err_msg=what)
    t = terms.cpu().numpy()
    for col, key in enumerate(TERM_KEYS):
        np.testing.assert_allclose(t[:len(entries), col], ref[key], rtol=5e-5, atol=3e-6, err_msg=f"{what} {key}")
    if dA is not None:
        close(dA, dscale * dref.reshape(res * res, KT), 5e-5, f"{what} dA")


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("res", [5, 15, 16])
def test_loss_single_image(ops, res, T, dt):
    entries = ENTRIES[:T]
    plan = ops.LossPlan(entries, oloss.DEFAULT_HYPER)
    maps = _maps(res, (3, 2), 1, DT[dt], 40 + res)
    A64 = _mean_map(maps, 1, 0)
    with bounds(ops, *maps) as g:
        A = ops.aggregate_maps(maps)
        terms, loss = ops.smooth_loss_fwd(A, res, 1, KT - 1, plan)
        A2, terms2, loss2 = ops.aggregate_loss_fwd(maps, res, 1, KT - 1, plan)
        dA, dPb = ops.smooth_loss_bwd(A, res, 1, KT - 1, plan, None, DT[dt], 0.2)
        dA0, none = ops.smooth_loss_bwd(A, res, 1, KT - 1, plan)
        for t, what in ((A, "A"), (terms, "terms"), (loss, "loss"), (A2, "A (fused)"), (terms2, "terms (fused)"),
                        (loss2, "loss (fused)"), (dA, "dA"), (dPb, "dP_bcast"), (dA0, "dA without the broadcast map")):
            g.assert_written(t, what)
    assert none is None and torch.equal(A, A2) and torch.equal(terms, terms2) and torch.equal(loss, loss2) and torch.equal(dA, dA0)
    close(A, A64.numpy(), 2e-6, "A")
    _check_loss(terms, loss.item(), dA, f64(A), entries, res, f"res {res} T {T}")
    close(dPb, f64(dA).numpy() * 0.2, TOL[dt], "dP_bcast")
    assert ops.tickets_are_zero()


# S = 3 images per launch.  The batched form shares one plan; the table form has ragged per-image T (3, 0, 1 in a table of
# capacity 4: rows T .. T_max of terms are ZERO by the header, an unguided image's dA is exact zeros — all of it written).
@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("res", [5, 15, 16])
def test_loss_batched(ops, res, T, dt):
    S = 3
    entries = ENTRIES[:T]
    plan = ops.LossPlan(entries, oloss.DEFAULT_HYPER)
    maps = _maps(res, (3, 2), S, DT[dt], 50 + res)
    dloss = torch.tensor([1.0, 0.0, 2.5], device="cuda")
    with bounds(ops, *maps, dloss) as g:
        A, terms, loss = ops.aggregate_loss_fwd_batched(maps, S, res, 1, KT - 1, plan)
        dA, dPb = ops.smooth_loss_bwd_batched(A, res, 1, KT - 1, plan, dloss, DT[dt], 0.2)
        for t, what in ((A, "A"), (terms, "terms"), (loss, "loss"), (dA, "dA"), (dPb, "dP_bcast")):
            g.assert_written(t, what)
    for s in range(S):
        close(A[s], _mean_map(maps, S, s).numpy(), 2e-6, f"A image {s}")
        _check_loss(terms[s], loss[s].item(), dA[s] if s != 1 else None, f64(A[s]), entries, res, f"image {s}",
                    dscale=float(dloss[s]))
    assert not dA[1].any() and not dPb[1].any()
    close(dPb, f64(dA).numpy() * 0.2, TOL[dt], "dP_bcast")
    assert ops.tickets_are_zero()


RAGGED = [ENTRIES, [], ENTRIES[1:2]]        # T = 3, 0, 1


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("res", [5, 15, 16])
def test_loss_image_table(ops, res, dt):
    S = 3
    plans = [ops.LossPlan(e, oloss.DEFAULT_HYPER) for e in RAGGED]
    slices = [(1, KT - 1), (1, KT - 1), (1, 40)]
    table = ops.ImageTable(S, 4, res, True, .5, 3, torch.device("cuda")).set(plans, slices)
    maps = _maps(res, (3, 2), S, DT[dt], 60 + res)
    dloss = torch.tensor([1.0, 1.0, 2.5], device="cuda")
    with bounds(ops, *maps, dloss, table.device_rows) as g:
        A, terms, loss = ops.aggregate_loss_fwd_images(maps, table)
        dA, dPb = ops.smooth_loss_bwd_images(A, table, dloss, DT[dt], 0.2)
        for t, what in ((A, "A"), (terms, "terms"), (loss, "loss"), (dA, "dA"), (dPb, "dP_bcast")):
            g.assert_written(t, what)
    for s in (0, 2):
        _check_loss(terms[s], loss[s].item(), dA[s], f64(A[s]), RAGGED[s], res, f"image {s}", slices[s], float(dloss[s]))
        assert not terms[s, len(RAGGED[s]):].any()              # rows T .. T_max are zero (include/ga_hip.h)
    assert not terms[1].any() and float(loss[1]) == 0.0 and not dA[1].any() and not dPb[1].any()
    close(dPb, f64(dA).numpy() * 0.2, TOL[dt], "dP_bcast")
    assert ops.tickets_are_zero()


@pytest.mark.parametrize("dt", ALL)
@pytest.mark.parametrize("res", [5, 15, 16])
def test_loss_relation_table(ops, res, dt):
    """Ragged T (3, 0, 1) and ragged R (1, 2, 0): rel_terms rows past an image's R are zero by the header.  Values against
    the float64 plugin path of test_relation_loss_gpu.py (its bounds: 1e-4 of the loss, 2e-3 of the gradient's maximum)."""
    from test_relation_loss_gpu import _plan, _plugin_total
    S = 3
    rels = [[([1], [4])], [([0, 3], [5]), ([2], [6, 7])], None]
    plans = [_plan(e) for e in RAGGED]
    table = ops.ImageTable(S, 4, res, True, .5, 3, torch.device("cuda"), Q_max=8)
    table.set(plans, [(1, KT - 1)] * S, [ops.RelationPlan(r) if r else None for r in rels])
    maps = _maps(res, (3, 2), S, DT[dt], 70 + res)
    dloss = torch.ones(S, device="cuda")
    with bounds(ops, *maps, dloss, table.device_rows, table.device_rel_rows) as g:
        A, terms, box, rel_terms, rel = ops.aggregate_loss_rel_fwd_images(maps, table)
        dA, dPb = ops.smooth_loss_rel_bwd_images(A, table, dloss, DT[dt], 0.2)
        for t, what in ((A, "A"), (terms, "terms"), (box, "box loss"), (rel_terms, "rel_terms"), (rel, "relation loss"),
                        (dA, "dA"), (dPb, "dP_bcast")):
            g.assert_written(t, what)
    for s in range(S):
        l64, g64 = _plugin_total(f64(A[s]).reshape(res, res, KT), RAGGED[s], KT - 1, rels[s] or [], torch.float64, "cpu")
        got = float(box[s] + rel[s])
        assert abs(got - float(l64)) <= 1e-4 * max(abs(float(l64)), 1e-30), (s, got, float(l64))
        if float(g64.abs().max()) > 0:
            close(dA[s], g64.numpy(), 2e-3, f"dA image {s}")
        else:
            assert not dA[s].any()
        assert not rel_terms[s, len(rels[s] or []):].any() and not terms[s, len(RAGGED[s]):].any()
    close(dPb, f64(dA).numpy() * 0.2, TOL[dt], "dP_bcast")
    assert ops.tickets_are_zero()


@pytest.mark.parametrize("dt", HALF)
def test_batched_loss_backward_reaches_the_capture_kernel(ops, dt):
    """AggregateSmoothLossBatched -> AttnCapture: the per-image dP map goes to ga_attn_capture_bwd_strided through the
    image-broadcast table (its dq is allocated inside ops too); against the same graph with a dense copy of the map."""
    S, H, res, D = 2, 2, 5, 8
    N = res * res
    T = DT[dt]
    q, k, v = make_qkv(S, H, N, KT, D, T, 800, 0.5)
    plan = ops.LossPlan(ENTRIES, oloss.DEFAULT_HYPER)
    scale = D ** -0.5
    qa = q.clone().requires_grad_(True)
    with bounds(ops, q, k, v) as g:
        o, p = ops.AttnCapture.apply(qa, k, v, H, scale, True)
        A, terms, loss = ops.AggregateSmoothLossBatched.apply(S, res, 1, KT - 1, plan, p)
        (dq,) = torch.autograd.grad(loss.sum(), [qa])
        ops.end_image_broadcasts()
        assert_copy_written(dq, "dQ")
        g.assert_written(A, "A")
    dA, dPb = ops.smooth_loss_bwd_batched(A, res, 1, KT - 1, plan, torch.ones(S, device="cuda"), T, 1.0 / H)
    dense = dPb.unsqueeze(1).expand(S, H, N, KT).reshape(S * H, N, KT).contiguous()
    ref = ops.attn_capture_bwd(q, k, v, torch.zeros_like(q), dense, H, scale)
    dQ, _, _ = oattn.capture_bwd_numpy(to_bh(q, H), to_bh(k, H), to_bh(v, H), scale, np.zeros_like(to_bh(q, H)), f64(dense).numpy())
    close(dq, from_bh(dQ, S, H), TOL[dt] * 2, "dQ vs fp64")
    close(dq, f64(ref).numpy(), TOL[dt], "strided entry vs the dense one")


# ===================================================================================== 3x3 convolution
# conv3x3.hip epilogue: a workgroup stores its bm x bn tile row by row, rows past M = B*Ho*Wo and (n tile past Cout) masked; with
# split-K the last-arriving slice reduces the slabs and runs the same store.  Shapes (B, Cin, Cout, H, W, stride):
#   (2,192,192,9,7,1): 126 pixels: one partial 128-row tile / two 64-row tiles with 62 rows in the second; Cout = 192 = 1.5 tiles of 128
#   (2,192,64,9,7,2):  stride 2 -> 5 x 4 x 2 = 40 pixels: less than any tile
#   (1,64,64,10,10,1): 100 pixels, no tile divides: the per-tap kernel
#   (3,128,64,8,8,1):  tiles of whole 8x8 images: 192 pixels = 1.5 tiles of 128 (the patch-in-LDS variant, partial last tile)
#   (2,64,64,24,24,1): runs of pixels that wrap a row; 576 pixels per image = 4.5 tiles of 128: images must not share a tile
#   (2,128,64,3,128,1): one 128-pixel row per tile
#   (2,64,128,12,12,1): 144 pixels per image, the DMA patch kernel
CONV_SHAPES = [(2, 192, 192, 9, 7, 1), (2, 192, 64, 9, 7, 2), (1, 64, 64, 10, 10, 1), (3, 128, 64, 8, 8, 1), (2, 64, 64, 24, 24, 1),
               (2, 128, 64, 3, 128, 1), (2, 64, 128, 12, 12, 1)]


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=ids)
def test_conv3x3(ops, shape, dt):
    B, Cin, Cout, H, W, stride = shape
    T = DT[dt]
    x = cl(dev(hashrand.normalish((B, Cin, H, W), 61 + Cin), T))
    w = dev(hashrand.normalish((Cout, Cin, 3, 3), 62 + Cout) * (1.0 / math.sqrt(9 * Cin)), T)
    bias = dev(hashrand.normalish((Cout,), 63) * 0.3, T)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    res, gy = (cl(dev(hashrand.normalish((B, Cout, Ho, Wo), s), T)) for s in (64, 65))
    xr = f64(x).requires_grad_(True)
    y_plain = torch.nn.functional.conv2d(xr, f64(w), None, stride=stride, padding=1)
    yr = y_plain + f64(bias)[None, :, None, None] + f64(res)
    yr.backward(f64(gy))
    tol = TOL[dt] * 2
    with bounds(ops, w) as g:           # the weight pack is an ops allocation too (cached for the weight's lifetime)
        wp = ops.conv3x3_packed_weights(w, False)
        g.assert_written(wp, "packed weights")
    plans = [(bm, bn, sp, sp * B * Ho * Wo * Cout if sp > 1 else 0) for bm, bn in ((128, 128), (128, 64), (64, 64)) for sp in (1, 2, 3)]
    for plan in plans + [None]:
        with bounds(ops, x, wp, bias, res) as g:
            y = ops.conv3x3_nhwc(x, wp, Cout, stride, bias, res, plan=plan)
            y0 = ops.conv3x3_nhwc(x, wp, Cout, stride, None, None, plan=plan)
            g.assert_written(y, f"y {plan}")
            g.assert_written(y0, f"plain y {plan}")
        assert y.shape == (B, Cout, Ho, Wo) and y.is_contiguous(memory_format=torch.channels_last)
        close(y, yr.detach().numpy(), tol, f"y {plan}")
        close(y0, y_plain.detach().numpy(), tol, f"plain y {plan}")
    # backward to the input under every plan as well.  Conv3x3.backward takes no plan (it asks the planner), so the launch it
    # makes is made here directly: stride 1 = the same kernel on the flipped, transposed pack, gy (B, Cout, H, W) -> dx
    # (B, Cin, H, W).  The stride-2 backward is the library's transposed convolution: no kernel of this project, nothing to loop.
    if stride == 1:
        wpt = ops.conv3x3_packed_weights(w, True)
        for bm, bn, sp, _ in plans:
            plan = (bm, bn, sp, sp * B * H * W * Cin if sp > 1 else 0)
            with bounds(ops, gy, wpt) as g:
                dxp = ops.conv3x3_nhwc(gy, wpt, Cin, 1, plan=plan)
                g.assert_written(dxp, f"dx {plan}")
            close(dxp, xr.grad.numpy(), tol * 2, f"dx {plan}")
    assert ops.tickets_are_zero()
    # autograd wrapper, the planner's choice both ways
    xa, ra = x.clone().requires_grad_(True), res.clone().requires_grad_(True)
    with bounds(ops, x, w, bias, res, gy) as g:
        ya = ops.conv3x3(xa, w, bias, ra, stride)
        dx, dres = torch.autograd.grad(ya, [xa, ra], gy)
        g.assert_written(ya, "y (autograd)")
        assert_copy_written(dx, "dx")
    close(ya, yr.detach().numpy(), tol, "autograd forward")
    close(dx, xr.grad.numpy(), tol * 2, "dx")
    assert torch.equal(dres, gy)


# ga_conv3x3_nhwc_gn: the epilogue also writes (B, blocks = 2 * HW / bm, G, 2) partial sums — two slots per m tile (the n tile a
# group starts in and the one it continues into).  Served where whole m tiles make up an image and the consuming norm takes two
# launches: the smallest such map is 32 x 36 = 1152 pixels (> 1024, a multiple of 128) with 64 channels in 8 groups.
@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("with_cb", [False, True])
def test_conv3x3_gn_epilogue(ops, with_cb, dt):
    B, Cin, Cout, H, W, groups = 2, 64, 64, 32, 36, 8
    T = DT[dt]
    x = cl(dev(hashrand.normalish((B, Cin, H, W), 160 + Cin), T))
    w = dev(hashrand.normalish((Cout, Cin, 3, 3), 161) * (1.0 / math.sqrt(9 * Cin)), T)
    bias = dev(hashrand.normalish((Cout,), 162) * 0.3, T)
    res = cl(dev(hashrand.normalish((B, Cout, H, W), 163), T))
    cb = dev(hashrand.normalish((B, Cout), 164) * 0.7, T) if with_cb else None
    gamma = dev(hashrand.normalish((Cout,), 165) * 0.3 + 1.0, T)
    beta = dev(hashrand.normalish((Cout,), 166) * 0.2, T)
    assert ops.gn_two_launch(H * W, Cout, groups, T)
    yr = torch.nn.functional.conv2d(f64(x), f64(w), f64(bias), padding=1) + f64(res)
    wp = ops.conv3x3_packed_weights(w, False)
    for bm, bn in ((128, 128), (128, 64), (64, 64)):
        for splits in (1, 3):
            plan = (bm, bn, splits, splits * B * H * W * Cout if splits > 1 else 0)
            assert ops.load().ga_conv3x3_gn_blocks(H, W, Cout, groups, bm, bn) == 2 * (H * W // bm)
            with bounds(ops, x, wp, bias, res, cb, gamma, beta, undefined=gn_workspace_undefined(B, H * W, Cout, groups, T)) as g:
                y, made = ops.conv3x3_nhwc(x, wp, Cout, 1, bias, res, plan=plan, gn=(groups, cb))
                partials, blocks = made
                g.assert_written(y, f"y {plan}")
                g.assert_written(partials, f"partial sums {plan}")
                z = ops.GroupNormAct.apply(y, gamma, beta, groups, 1e-5, True, cb, False, made)
                g.assert_written(z, f"ga_group_norm_apply {plan}")
            assert tuple(partials.shape) == (B, 2 * (H * W // bm), groups, 2)
            close(y, yr.numpy(), TOL[dt] * 2, f"y {plan}")
            yd = f64(y) + (f64(cb)[:, :, None, None] if with_cb else 0.0)
            yg = yd.reshape(B, groups, -1)
            close(partials[..., 0].sum(1), yg.sum(-1).numpy(), 2e-5, f"sum {plan}")
            close(partials[..., 1].sum(1), (yg * yg).sum(-1).numpy(), 2e-5, f"sum of squares {plan}")
            ref = torch.nn.functional.silu(torch.nn.functional.group_norm(yd, groups, f64(gamma), f64(beta), 1e-5))
            close(z, ref.numpy(), TOL[dt] * 2, f"one-launch norm {plan}")
    assert ops.tickets_are_zero()


# ga_conv3x3_up2x_nhwc: (2,64,64,2,2) -> 4 x 4 maps: not served by the patch kernel, the wrapper up-samples and runs
# ga_conv3x3_nhwc (32 pixels: less than a tile); (3,64,64,4,4) -> 8 x 8: whole images per tile, 192 pixels = a partial last
# tile, the one shape here the fused kernel takes; (1,64,64,12,20) -> 24 x 40 = 960 pixels: 7.5 tiles of 128, runs of pixels:
# refused as well (the register-staged kernel gathers from a full-size input), the two-launch fallback runs.
@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("shape", [(2, 64, 64, 2, 2), (3, 64, 64, 4, 4), (1, 64, 64, 12, 20)], ids=ids)
def test_upsample_conv3x3(ops, shape, dt):
    B, Cin, Cout, H, W = shape
    T = DT[dt]
    ops._no_fused_upsample.clear()
    x = cl(dev(hashrand.normalish((B, Cin, H, W), 71 + Cin), T))
    w = dev(hashrand.normalish((Cout, Cin, 3, 3), 72 + Cout) * (1.0 / math.sqrt(9 * Cin)), T)
    bias = dev(hashrand.normalish((Cout,), 73) * 0.3, T)
    gy = cl(dev(hashrand.normalish((B, Cout, 2 * H, 2 * W), 74), T))
    xr = f64(x).requires_grad_(True)
    yr = torch.nn.functional.conv2d(torch.nn.functional.interpolate(xr, scale_factor=2.0, mode="nearest"), f64(w), f64(bias), padding=1)
    yr.backward(f64(gy))
    xa = x.clone().requires_grad_(True)
    # which form serves the shape is asked once, unguarded: a refused shape's output buffer is allocated and dropped unwritten
    # (ops remembers the refusal and allocates nothing for that shape afterwards)
    served = ops.conv3x3_up2x_nhwc(x, ops.conv3x3_packed_weights(w, False), Cout, bias) is not None
    assert served == (min(H, W) >= 4 and (B, H, W) != (1, 12, 20)), "which shapes the fused form serves changed: update this test"
    with bounds(ops, x, w, bias, gy) as g:
        y = ops.upsample_conv3x3(xa, w, bias)
        (dx,) = torch.autograd.grad(y, [xa], gy)
        g.assert_written(y, "y")
        wp = ops.conv3x3_packed_weights(w, False)
        for bm, bn in ((128, 128), (128, 64), (64, 64)):
            for sp in (1, 3):
                fused = ops.conv3x3_up2x_nhwc(x, wp, Cout, bias, plan=(bm, bn, sp, 0))
                assert (fused is not None) == served
                if fused is not None:
                    g.assert_written(fused, f"fused y {(bm, bn, sp)}")
                    assert torch.equal(fused, y) or bool(((fused.float() - y.float()).abs() <= TOL[dt] * 2 * y.float().abs().max()).all())
    close(y, yr.detach().numpy(), TOL[dt] * 2, "y")
    close(dx, xr.grad.numpy(), TOL[dt] * 3, "dx")
    assert ops.tickets_are_zero()


# thin_conv.hip: segments of 16 pixels of a row (W % 16 == 0): (2,64,5,16) one segment per row, 10 segments; (1,192,3,32) three
# 64-channel blocks, 6 segments; (3,128,7,48) 63 segments.  4 -> C writes channels-last (B, C, H, W), C -> 4 dense NCHW
# (B, 4, H, W): four planes of H*W elements each — a plane's neighbour is the next channel's plane.
@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("shape", [(2, 64, 5, 16), (1, 192, 3, 32), (3, 128, 7, 48)], ids=ids)
def test_thin_convolutions(ops, shape, dt):
    B, C, H, W = shape
    T = DT[dt]
    conv = torch.nn.functional.conv2d
    tol = TOL[dt] * 2
    for cin, cout in ((4, C), (C, 4)):
        x = dev(hashrand.normalish((B, cin, H, W), 81 + C + cin), T)
        x = x if cin == 4 else cl(x)
        w = dev(hashrand.normalish((cout, cin, 3, 3), 82) * (1.0 / math.sqrt(9 * cin)), T)
        bias = dev(hashrand.normalish((cout,), 83) * 0.3, T)
        gy = dev(hashrand.normalish((B, cout, H, W), 84), T)
        gy = cl(gy) if cout != 4 else gy
        assert ops.conv3x3_thin_supported(x, w)
        xr = f64(x).requires_grad_(True)
        yr = conv(xr, f64(w), f64(bias), padding=1)
        yr.backward(f64(gy))
        xa = x.clone().requires_grad_(True)
        with bounds(ops, x, w, bias, gy) as g:
            y = ops.conv3x3_thin_apply(xa, w, bias)
            (dx,) = torch.autograd.grad(y, [xa], gy)
            y0 = ops.conv3x3_thin_apply(x, w, None)
            g.assert_written(y, f"{cin} -> {cout} y")
            g.assert_written(y0, f"{cin} -> {cout} y without bias")
            assert_copy_written(dx, f"{cin} -> {cout} dx")
        close(y, yr.detach().numpy(), tol, f"{cin} -> {cout} forward")
        close(dx, xr.grad.numpy(), tol * 2, f"{cin} -> {cout} backward to the input")
        close(y0, conv(f64(x), f64(w), None, padding=1).numpy(), tol, f"{cin} -> {cout} no bias")


# ===================================================================================== GEMM / Linear
# ga_gemm_nt = the convolution kernel as a one-tap convolution, same epilogue: (200,64,72): M = 1.56 tiles of 128 / 3.1 of 64,
# N = 72 = one partial n tile (8 columns past 64: ONE 16-byte vector in the second 64-tile); (130,192,264): 2 rows in the
# last m tile, N = 2 tiles of 128 + 8.
@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("shape", [(200, 64, 72), (130, 192, 264)], ids=ids)
def test_gemm_nt(ops, shape, dt):
    from guided_attention_amd._lib import dtype_code, load, stream_ptr
    M, K, N = shape
    T = DT[dt]
    x = dev(hashrand.normalish((M, K), 71), T)
    w = dev(hashrand.normalish((N, K), 72) * (1.0 / math.sqrt(K)), T)
    bias = dev(hashrand.normalish((N,), 73) * 0.3, T)
    res = dev(hashrand.normalish((M, N), 74), T)
    ref = f64(x) @ f64(w).T + f64(bias) + f64(res)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    for bm, bn in ((128, 128), (128, 64), (64, 64)):
        for sp in (1, 3):
            if sp > K // ops.CONV_KC:
                continue
            with bounds(ops, x, w, bias, res) as g:
                y = g.carve((M, N), T, "cuda", "the test (y of ga_gemm_nt)")
                ws, tickets = ops.splitk_workspace(x.device, M, N, bm, bn, sp)
                rc = load().ga_gemm_nt(P(x), P(w), P(y), P(ws), P(tickets), P(bias), P(res), M, K, N, bm, bn, sp, dtype_code(x),
                                       stream_ptr())
                assert rc == 0
                g.assert_written(y, f"y tile {bm}x{bn} splits {sp}")
            close(y, ref.numpy(), TOL[dt] * 2, f"gemm tile {bm}x{bn} splits {sp}")
    assert ops.tickets_are_zero()


LIN_PLANS = [(128, 128, 1, 0), (128, 64, 1, 3), (64, 128, 1, 0), (64, 64, 2, 0), (64, 64, 3, 5)]


# linear.hip epilogue: y (M, n_out) row by row in 16-byte vectors, rows past M and vectors past n_out masked; GEGLU halves the
# stored width (n_out = N / 2 = 36 resp. 132: 4.5 resp. 16.5 vectors -> the last vector of a row is a HALF vector's worth of
# columns short of the tile) and writes preact (M, N) beside it; row_partials (M, parts, 2) f32 one slot per n tile; ln_stats
# (M, 2) f32.  Shapes as test_gemm_nt.
@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("plan", LIN_PLANS, ids=ids)
@pytest.mark.parametrize("shape", [(200, 64, 72), (130, 192, 264)], ids=ids)
def test_linear_fused(ops, shape, plan, dt):
    M, K, N = shape
    if K // 64 < plan[2]:
        plan = plan[:2] + (1,) + plan[3:]       # K = 64 is one k-step: the plan's tile and ring without the split
    T = DT[dt]
    x = dev(hashrand.normalish((M, K), 70 + M) * 1.5 + 0.3, T)
    w = dev(hashrand.normalish((N, K), 71 + N) * K ** -0.5, T)
    bias = dev(hashrand.normalish((N,), 72) * 0.3, T)
    res = dev(hashrand.normalish((M, N), 73), T)
    # GEGLU needs N % 16 == 0 (72 and 264 are not): N + 8 = 80 / 272 -> 40 / 136 stored columns = 1.25 / 4.25 half-tiles of 32
    wge = dev(hashrand.normalish((N + 8, K), 77 + N) * K ** -0.5, T)
    bge = dev(hashrand.normalish((N + 8,), 78) * 0.3, T)
    xd, wd, bd, rd = f64(x), f64(w), f64(bias), f64(res)
    ref_plain = xd @ wd.T + bd
    ref_ge = xd @ f64(wge).T + f64(bge)
    tol = TOL[dt] * 2
    with bounds(ops, x, w, bias, res, wge, bge) as g:
        y1 = ops.linear_fused(x, w, bias, plan=plan)["y"]
        y2 = ops.linear_fused(x, w, bias, residual=res, plan=plan)["y"]
        y3 = ops.linear_fused(x, w, None, plan=plan)["y"]
        out = ops.linear_fused(x, wge, bge, geglu=True, want_preact=True, plan=plan)
        yg = ops.linear_fused(x, wge, bge, geglu=True, plan=plan)["y"]
        for t, what in ((y1, "bias"), (y2, "bias + residual"), (y3, "no bias"), (out["y"], "geglu"), (out["preact"], "preact"),
                        (yg, "geglu without preact")):
            g.assert_written(t, f"{what} {plan}")
    close(y1, ref_plain.numpy(), tol, f"bias {plan}")
    close(y2, (ref_plain + rd).numpy(), tol, f"bias + residual {plan}")
    close(y3, (xd @ wd.T).numpy(), tol, f"no bias {plan}")
    close(out["preact"], ref_ge.numpy(), tol, f"geglu preact {plan}")
    pre = f64(out["preact"])
    F_ = (N + 8) // 2
    assert tuple(out["y"].shape) == (M, F_)
    close(out["y"], (pre[:, :F_] * _gelu64(pre[:, F_:])).numpy(), tol, f"geglu {plan}")
    assert torch.equal(yg, out["y"])
    # producer -> consumer: row partial sums, then the LayerNorm fold with its (mean, rstd) output
    gamma = dev(hashrand.normalish((K,), 74) * 0.2 + 1.0, T)
    beta = dev(hashrand.normalish((K,), 75) * 0.2, T)
    w0 = dev(hashrand.normalish((K, K), 76) * K ** -0.5, T)
    wg, colsum, shift = _fold(w, bias, gamma, beta, T)
    with bounds(ops, x, w0, wg, colsum, shift) as g:
        prod = ops.linear_fused(x, w0, None, residual=x, want_row_partials=True, plan=plan)
        g.assert_written(prod["y"], f"producer y {plan}")
        g.assert_written(prod["row_partials"], f"row partial sums {plan}")
        h = prod["y"]
        lnout = ops.linear_fused(h, wg, None, ln=(prod["row_partials"], colsum, shift, 1e-5), want_ln_stats=True, plan=plan)
        g.assert_written(lnout["y"], f"LayerNorm fold {plan}")
        g.assert_written(lnout["ln_stats"], f"ln_stats {plan}")
    hd = f64(h)
    assert tuple(prod["row_partials"].shape) == (M, -(-K // plan[1]), 2)
    close(prod["row_partials"][:, :, 0].sum(1), hd.sum(-1).numpy(), 1e-5, "row partial sums")
    close(prod["row_partials"][:, :, 1].sum(1), (hd * hd).sum(-1).numpy(), 1e-5, "row partial sums of squares")
    mean, var = hd.mean(-1, keepdim=True), hd.var(-1, unbiased=False, keepdim=True)
    ln = (hd - mean) / torch.sqrt(var + 1e-5) * f64(gamma) + f64(beta)
    close(lnout["y"], (ln @ wd.T + bd).numpy(), tol * 2, f"LayerNorm fold {plan}")
    close(lnout["ln_stats"][:, 0], mean[:, 0].numpy(), 1e-4, "mean")
    close(lnout["ln_stats"][:, 1], (1.0 / torch.sqrt(var + 1e-5))[:, 0].numpy(), 1e-3, "rstd")
    assert ops.tickets_are_zero()


# gn_partials (M / hw, blocks = 2 * hw / bm, G, 2): served where m tiles do not straddle images: hw = 128 is the smallest pixel
# count both tile heights divide (B = 2 images: the second image's blocks follow the first's directly).
@pytest.mark.parametrize("dt", HALF)
def test_linear_fused_gn_epilogue(ops, dt):
    B, HW, K, N, groups = 2, 128, 64, 64, 8
    T = DT[dt]
    M = B * HW
    x = dev(hashrand.normalish((M, K), 180 + K), T)
    w = dev(hashrand.normalish((N, K), 181) * (1.0 / math.sqrt(K)), T)
    bias = dev(hashrand.normalish((N,), 182) * 0.3, T)
    res = dev(hashrand.normalish((M, N), 183) * 1.5 + 0.3, T)
    ref = f64(x) @ f64(w).T + f64(bias) + f64(res)
    for bm, bn in ((128, 128), (128, 64), (64, 128), (64, 64)):
        plan = (bm, bn, 1, 4 if bm * bn <= 64 * 128 else 2)
        assert ops.load().ga_linear_gn_blocks(HW, N, groups, bm, bn) == 2 * (HW // bm)
        with bounds(ops, x, w, bias, res) as g:
            out = ops.linear_fused(x, w, bias, residual=res, plan=plan, gn=(groups, HW))
            partials, nb = out["gn"]
            g.assert_written(out["y"], f"y {plan}")
            g.assert_written(partials, f"gn partial sums {plan}")
        assert tuple(partials.shape) == (B, 2 * (HW // bm), groups, 2)
        close(out["y"], ref.numpy(), TOL[dt] * 2, f"y {plan}")
        yg = f64(out["y"]).reshape(B, HW, groups, N // groups).permute(0, 2, 1, 3).reshape(B, groups, -1)
        close(partials[..., 0].sum(1), yg.sum(-1).numpy(), 2e-5, f"sum {plan}")
        close(partials[..., 1].sum(1), (yg * yg).sum(-1).numpy(), 2e-5, f"sum of squares {plan}")


@pytest.mark.parametrize("dt", HALF)
def test_linear_fused_strided_views(ops, dt):
    """Column slices of a wider tensor as input, residual and OUTPUT (row stride > the row's width): the 64 columns on either
    side of the output slice belong to somebody else and must come back bit-identical (a full-tile store would take them)."""
    T = DT[dt]
    M, K, N = 300, 128, 64
    big = dev(hashrand.normalish((M, 3 * K), 80), T)
    w = dev(hashrand.normalish((N, K), 81) * 0.1, T)
    resbig = dev(hashrand.normalish((M, 3 * N), 82), T)
    for plan in ((64, 64, 1), (128, 128, 1), (128, 64, 2)):
        for j in range(3):
            xs, rs = big[:, K * j:K * (j + 1)], resbig[:, N * j:N * (j + 1)]
            ref = f64(xs) @ f64(w).T + f64(rs)
            with bounds(ops, big, w, resbig) as g:
                y = ops.linear_fused(xs, w, None, residual=rs, plan=plan)["y"]
                g.assert_written(y, f"slice {j}")
                wide = g.carve((M, 3 * N), T, "cuda", "the test (a wider output)")
                wide.copy_(resbig)
                before = wide.clone()
                view = wide[:, N * j:N * (j + 1)]
                got = ops.linear_fused(xs, w, None, residual=rs, plan=plan, out=view)["y"]
            assert got is view
            close(y, ref.numpy(), TOL[dt] * 2, f"slice {j} {plan}")
            assert torch.equal(view, y)
            keep = torch.ones(3 * N, dtype=torch.bool, device="cuda")
            keep[N * j:N * (j + 1)] = False
            assert torch.equal(wide[:, keep].view(torch.int16), before[:, keep].view(torch.int16)), f"columns beside slice {j} changed"


@pytest.mark.parametrize("dt", HALF)
def test_linear_stream_form(ops, dt):
    """linear_stream_kernel at the smallest of STREAM_CASES (fewest multiply-adds: 260 x 640 x 72 — three m tiles with 4 rows in
    the last, one n tile of which 72 columns exist; one tile per persistent workgroup, five partial sums per row)."""
    M, K, N, ptile, geglu = min(STREAM_CASES, key=lambda c: c[0] * c[1] * c[2])
    T = DT[dt]
    x0 = dev(hashrand.normalish((M, K), 150 + M) * 1.3 + 0.4, T)
    w0 = dev(hashrand.normalish((K, K), 151) * K ** -0.5, T)
    prod = ops.linear_fused(x0, w0, None, residual=x0, want_row_partials=True, plan=ptile + (1,))
    h, partials = prod["y"], prod["row_partials"]
    assert ops.linear_stream_serves(K, partials.shape[1], True, None, None, False, False, False)
    gamma = dev(hashrand.normalish((K,), 152) * 0.2 + 1.0, T)
    beta = dev(hashrand.normalish((K,), 153) * 0.2, T)
    w = dev(hashrand.normalish((N, K), 154) * K ** -0.5, T)
    bias = dev(hashrand.normalish((N,), 155) * 0.3, T)
    wg, colsum, shift = _fold(w, bias, gamma, beta, T)
    hd = f64(h)
    mean, var = hd.mean(-1, keepdim=True), hd.var(-1, unbiased=False, keepdim=True)
    ln = (hd - mean) / torch.sqrt(var + 1e-5) * f64(gamma) + f64(beta)
    pre = ln @ f64(w).T + f64(bias)
    ref = pre[:, :N // 2] * _gelu64(pre[:, N // 2:]) if geglu else pre
    with bounds(ops, h, wg, partials, colsum, shift) as g:
        y = ops.linear_fused(h, wg, None, geglu=geglu, ln=(partials, colsum, shift, 1e-5), plan=ops.LINEAR_STREAM_PLAN)["y"]
        g.assert_written(y, "stream form")
    close(y, ref.numpy(), TOL[dt] * 4, "stream form")
