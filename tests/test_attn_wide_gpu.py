"""ga_attn_wide_fwd (csrc/attn_wide.hip), the forward-only flash attention for head sizes 64 ... 512 that the VAE decoder's mid
block runs (one head of 512 channels), against the fp64 oracle on the 16-bit inputs.

Inputs and tolerance are those of test_kernels_gpu.test_self_attention_fwd_bwd: hashrand.normalish with q and k spread by 1.5
(1.0 above 1024 tokens), TOL = 2e-3 (f16) / 1.6e-2 (bf16) of max |ref| — the arithmetic is the same (f32 scores, maximum, sum and
accumulators, P rounded to T for the second product, one rounding at the store of O); only the contraction is longer.

Shapes: 512-wide heads at a whole number of 64-query / 32-key tiles (256), at a ragged one with a batch of two (200), at one
token; 256-, 64- and 192-wide heads (other instantiations) with ragged tiles and several heads; and the 4096-token mid block of a
512^2 image at full size.
"""
import pytest
import torch

import hashrand
from guarded_alloc import guarded, snapshot, assert_intact
from oracle import attention as oattn
from test_kernels_gpu import DT, TOL, close, dev, from_bh, to_bh

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 256, 512), (2, 1, 200, 512), (1, 1, 1, 512), (1, 1, 65, 256), (1, 2, 130, 64), (1, 3, 77, 192)]
FULL = (1, 1, 4096, 512)
HALF = ["f16", "bf16"]
ids = lambda s: "x".join(map(str, s))  # noqa: E731


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from guided_attention_amd import ops as _ops
    _ops.load()
    return _ops


def qkv(shape, dt):
    B, H, N, D = shape
    spread = 1.5 if N <= 1024 else 1.0
    q = dev(hashrand.normalish((B, N, H * D), 11 + N) * spread, DT[dt])
    k = dev(hashrand.normalish((B, N, H * D), 12 + N) * spread, DT[dt])
    v = dev(hashrand.normalish((B, N, H * D), 13 + N), DT[dt])
    return q, k, v


def reference(q, k, v, H, scale):
    B = q.shape[0]
    _, Oref = oattn.capture_fwd_numpy(to_bh(q, H), to_bh(k, H), to_bh(v, H), scale)
    return from_bh(Oref, B, H)


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("shape", SHAPES + [FULL], ids=ids)
def test_attn_wide_against_fp64(ops, shape, dt):
    B, H, N, D = shape
    q, k, v = qkv(shape, dt)
    scale = D ** -0.5
    assert ops.attn_wide_supported(q, H)
    o = ops.attn_wide_fwd(q, k, v, H, scale)
    assert o.shape == q.shape and o.dtype == q.dtype
    close(o, reference(q, k, v, H, scale), TOL[dt], "O")


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_fused_qkv_form_gives_the_same_bits(ops, shape, dt):
    """ld_qkv = 3*H*D: the column slices of one (B, N, 3C) tensor, read in place."""
    B, H, N, D = shape
    q, k, v = qkv(shape, dt)
    scale = D ** -0.5
    o = ops.attn_wide_fwd(q, k, v, H, scale)
    fused = torch.cat([q, k, v], dim=-1).contiguous()
    assert torch.equal(ops.attn_wide_fwd(fused, None, None, H, scale), o)


@pytest.mark.parametrize("dt", HALF)
def test_agrees_with_the_narrow_flash_kernel_at_64(ops, dt):
    """At a head size both kernels serve, the wide kernel is within TOL of ga_self_attn_fwd too."""
    shape = (1, 2, 130, 64)
    q, k, v = qkv(shape, dt)
    scale = 64 ** -0.5
    o = ops.attn_wide_fwd(q, k, v, 2, scale)
    narrow, _ = ops.self_attn_fwd(q, k, v, 2, scale, want_lse=False)
    close(o, narrow.double().cpu().numpy(), TOL[dt], "O against ga_self_attn_fwd")
    close(o, reference(q, k, v, 2, scale), TOL[dt], "O")


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("shape", [(2, 1, 200, 512), (1, 3, 77, 192)], ids=ids)
def test_output_is_written_in_full_and_nothing_else(ops, shape, dt):
    """O carved from a 0xFF arena with red zones: a ragged last query tile (200 = 3 * 64 + 8, 77 = 64 + 13) must store its
    live rows only, and all of them."""
    B, H, N, D = shape
    q, k, v = qkv(shape, dt)
    snap = snapshot(q, k, v)
    with guarded(ops) as g:
        o = ops.attn_wide_fwd(q, k, v, H, D ** -0.5)
        g.assert_written(o, "O")
        g.assert_all_written()
    assert len(g.arenas) == 1
    assert_intact(snap)
    close(o, reference(q, k, v, H, D ** -0.5), TOL[dt], "O")


def test_refusals_reach_python(ops):
    from guided_attention_amd._lib import GaError
    q = torch.zeros((1, 8, 96), dtype=torch.float16, device="cuda")       # head size 96: not a multiple of 64
    assert not ops.attn_wide_supported(q, 1)
    with pytest.raises(GaError, match="size out of the supported range"):
        ops.attn_wide_fwd(q, q, q, 1, 1.0)
    f = torch.zeros((1, 8, 64), dtype=torch.float32, device="cuda")
    assert not ops.attn_wide_supported(f, 1)
    with pytest.raises(GaError, match="not implemented"):
        ops.attn_wide_fwd(f, f, f, 1, 1.0)
