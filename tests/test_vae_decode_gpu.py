"""The VAE decoder on own kernels (GuidedAttention.own_vae_decode, vae.AutoencoderKLDecoder.decode_own) on the GPU.

Decoder: AutoencoderKLDecoder(ch=(64, 64, 128, 512)) — a 512-wide mid block (ga_attn_wide_fwd), every channel count a multiple
of 64, so every layer is inside the own kernels' envelope — with non-zero biases and GroupNorm weights / biases that differ from
group to group.  Latents (3, 4, 16, 16) in f16 and bf16; the decoder tests use the first two, the chunked pipeline test all three.

Measure: max |out - ref| / max |ref| on the decoder output before the clamp, ref = the same module's arithmetic in fp64 on the
CPU from the 16-bit parameters and inputs; err_parent = the framework 16-bit GPU decode (switch off), err_own = the own path.
Bound: err_own <= 2 * err_parent.  Both paths round to 16 bits once per layer boundary, only in different places, so neither
should be systematically worse; the factor 2 covers the reordered f32 sums (split-K, the norm's partial sums).

Layer counts come from the module tree: 14 resnets (2 mid + 4 x 3) with two 3x3 convolutions each and 3 up-samplers are 31
main-kernel convolutions (conv_in and conv_out are the thin kernels); 28 resnet norms + the attention's + conv_norm_out are
30 norms.
"""
import copy
from collections import Counter

import numpy as np
import pytest
import torch
import torch.nn as nn

import hashrand

pytestmark = pytest.mark.gpu

DT = {"f16": torch.float16, "bf16": torch.bfloat16}
CH = (64, 64, 128, 512)
UNIT = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8, "f32": 2.0 ** -24}     # one rounding of T: half an ulp, relative


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from guided_attention_amd import ops as _ops
    _ops.load()
    return _ops


def seed_parameters(vae, seed=7):
    """Non-zero biases; GroupNorm gains and offsets with a per-group part that differs from group to group."""
    g = torch.Generator().manual_seed(seed)
    norm_params = {id(p) for m in vae.modules() if isinstance(m, nn.GroupNorm) for p in (m.weight, m.bias)}
    with torch.no_grad():
        for m in vae.modules():
            if isinstance(m, nn.GroupNorm):
                cg = m.num_channels // m.num_groups
                m.weight.copy_((0.6 + 0.8 * torch.rand(m.num_groups, generator=g)).repeat_interleave(cg)
                               + 0.1 * torch.randn(m.num_channels, generator=g))
                m.bias.copy_((0.3 * torch.randn(m.num_groups, generator=g)).repeat_interleave(cg)
                             + 0.05 * torch.randn(m.num_channels, generator=g))
        for n, p in vae.named_parameters():
            if n.endswith("bias") and id(p) not in norm_params:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    return vae


def make_pipe(vae, dtype):
    from guided_attention_amd.pipeline_guided_attention import GuidedAttention
    from guided_attention_amd.unet import UNet2DConditionModel, UNetConfig
    return GuidedAttention(UNet2DConditionModel(UNetConfig.tiny(32, 48)), vae=vae).to("cuda", dtype)


def rel_err(out, ref):
    return float((out.double().cpu() - ref).abs().max() / ref.abs().max())


def fp64_decode(vae, latents):
    """The module's own arithmetic in fp64 on the CPU from the 16-bit parameters and the 16-bit latents."""
    ref = copy.deepcopy(vae).cpu().double()
    with torch.no_grad():
        return ref.decode(latents.double().cpu() / ref.scaling_factor)


def census_names(ops, fn):
    ops.start_census()
    try:
        out = fn()
    finally:
        rec = ops.stop_census()
    names = Counter()
    for key, n in rec.items():
        names[key[0]] += n
    return out, names


_CASES = {}


def case(dt):
    """Built once per dtype and left unchanged: the pipeline, the latents, the fp64 reference, both 16-bit decodes."""
    if dt not in _CASES:
        from guided_attention_amd.vae import AutoencoderKLDecoder
        vae = seed_parameters(AutoencoderKLDecoder(ch=CH).init_weights_())
        pipe = make_pipe(vae, DT[dt])
        lat = torch.from_numpy(np.ascontiguousarray(hashrand.normalish((3, 4, 16, 16), 41))).to("cuda", DT[dt])
        ref = fp64_decode(vae, lat)
        with torch.no_grad():
            parent = vae.decode(lat / vae.scaling_factor)
        own = vae.decode_own(lat, 1.0 / vae.scaling_factor)
        _CASES[dt] = dict(pipe=pipe, vae=vae, lat=lat, ref=ref, parent=parent, own=own,
                          err_parent=rel_err(parent[:2], ref[:2]), err_own=rel_err(own[:2], ref[:2]))
    return _CASES[dt]


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_own_decode_is_as_close_to_fp64_as_the_framework_decode(ops, dt):
    c = case(dt)
    print(f"\nvae decode {dt}: err_own {c['err_own']:.3e}  err_parent {c['err_parent']:.3e} (max abs / max |ref|, before the clamp)")
    assert c["own"].shape == c["parent"].shape == (3, 3, 128, 128) and c["own"].dtype == DT[dt]
    assert torch.isfinite(c["own"]).all()
    assert c["err_parent"] > 0
    assert c["err_own"] <= 2 * c["err_parent"], (c["err_own"], c["err_parent"])


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_census_of_one_own_decode(ops, dt):
    c = case(dt)
    vae, lat = c["vae"], c["lat"][:2]
    convs = [m for n, m in vae.decoder.named_modules()
             if isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3) and n not in ("conv_in", "conv_out")]
    norms = [m for m in vae.modules() if isinstance(m, nn.GroupNorm)]
    assert (len(convs), len(norms)) == (31, 30)
    out, names = census_names(ops, lambda: vae.decode_own(lat, 1.0 / vae.scaling_factor))
    assert out.shape == (2, 3, 128, 128)
    assert names["latent_affine4"] == 1
    assert names["conv3x3_thin_in"] == 1 and names["conv3x3_thin_out"] == 1
    assert names["attn_wide_fwd"] == 1 and names["self_attn_fwd"] == 0
    assert names["conv3x3"] == len(convs)
    assert names["group_norm_fwd"] + names["group_norm_apply"] == len(norms)
    assert names["linear"] == 4                                 # two 1x1 shortcuts (512 -> 128, 128 -> 64), q|k|v, proj_attn
    assert sum(names.values()) == 1 + 2 + 1 + 31 + 30 + 4


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("B,hw", [(1, 256), (3, 256), (1, 255), (3, 255)])
def test_latent_affine4_against_fp64(ops, B, hw, dt):
    """out = bias + W (pre_scale x) per pixel.  Tolerance: one rounding of T of the result, |ref| * unit(T), plus the f32
    evaluation itself — one product and four fmas, at most five f32 roundings of the sum of the absolute terms."""
    T = {"f32": torch.float32, **DT}[dt]
    W_side = 17 if hw == 255 else 16
    H_side = hw // W_side
    assert H_side * W_side == hw
    x = torch.from_numpy(np.ascontiguousarray(hashrand.normalish((B, 4, H_side, W_side), 3 + hw + B))).to("cuda", T)
    w = torch.from_numpy(np.ascontiguousarray(hashrand.normalish((4, 4, 1, 1), 5))).to("cuda", T)
    b = torch.from_numpy(np.ascontiguousarray(hashrand.normalish((4,), 6))).to("cuda", T)
    s = 1.0 / 0.18215
    out = ops.latent_affine4(x, w, b, s)
    assert out.shape == x.shape and out.dtype == T and out.is_contiguous()
    s32 = float(np.float32(s))
    xs = x.double().cpu() * s32
    w64, b64 = w.double().cpu().reshape(4, 4), b.double().cpu()
    ref = torch.einsum("oi,bihw->bohw", w64, xs) + b64[None, :, None, None]
    mag = torch.einsum("oi,bihw->bohw", w64.abs(), xs.abs()) + b64.abs()[None, :, None, None]
    tol = ref.abs() * UNIT[dt] + 5 * 2.0 ** -24 * mag
    err = (out.double().cpu() - ref).abs()
    assert bool((err <= tol).all()), float((err - tol).max())


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_pipeline_switch_and_chunks(ops, dt):
    """pipe.decode_latents with the switch on, S = 3 under a budget of two images per chunk (chunks of 2 + 1)."""
    from guided_attention_amd import vae as vae_mod
    c = case(dt)
    pipe, lat = c["pipe"], c["lat"]
    assert pipe.own_vae_decode is False
    off = pipe.decode_latents(lat)
    seen = []
    real = c["vae"].decode_own
    pipe.own_vae_decode = True
    pipe.vae_decode_budget = 2 * vae_mod.largest_activation(16, 16, CH)
    c["vae"].decode_own = lambda z, s: seen.append(z.shape[0]) or real(z, s)
    try:
        on = pipe.decode_latents(lat)
    finally:
        pipe.own_vae_decode, pipe.vae_decode_budget = False, None
        del c["vae"].decode_own
    assert seen == [2, 1]
    for img in (on, off):
        assert isinstance(img, np.ndarray) and img.dtype == np.float32 and img.shape == (3, 128, 128, 3)
        assert img.min() >= 0 and img.max() <= 1
    # |on - off| <= (|own - ref| + |parent - ref|) / 2 <= 3 err_parent max|ref| / 2 (triangle inequality after the / 2; the
    # clamp only shrinks differences)
    scale = float(c["ref"].abs().max())
    assert np.abs(on - off).max() <= 3 * c["err_parent"] / 2 * scale
    # every image against its own fp64 reference, whichever chunk it was in
    ref_img = (c["ref"] / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).numpy()
    for i in range(3):
        bound = 2 * rel_err(c["parent"][i:i + 1], c["ref"][i:i + 1]) * float(c["ref"][i].abs().max()) / 2
        unit = UNIT[dt]      # the image itself is rounded to T once more after the / 2 + 0.5 (values up to 1)
        assert np.abs(on[i] - ref_img[i]).max() <= bound + unit, i


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_tiny_decoder_falls_back_where_it_must(ops, dt):
    """AutoencoderKLDecoder.tiny(): 32-channel levels are outside the GEMM convolution (framework convolutions there), the
    64-wide attention runs on the narrow flash kernel.  Same bound, nothing raises."""
    from guided_attention_amd.vae import AutoencoderKLDecoder
    vae = seed_parameters(AutoencoderKLDecoder.tiny().init_weights_(), seed=9)
    make_pipe(vae, DT[dt])
    lat = torch.from_numpy(np.ascontiguousarray(hashrand.normalish((2, 4, 16, 16), 43))).to("cuda", DT[dt])
    ref = fp64_decode(vae, lat)
    with torch.no_grad():
        parent = vae.decode(lat / vae.scaling_factor)
    own, names = census_names(ops, lambda: vae.decode_own(lat, 1.0 / vae.scaling_factor))
    err_own, err_parent = rel_err(own, ref), rel_err(parent, ref)
    print(f"\ntiny vae decode {dt}: err_own {err_own:.3e}  err_parent {err_parent:.3e}")
    assert names["self_attn_fwd"] == 1 and names["attn_wide_fwd"] == 0
    assert 0 < names["conv3x3"] < 31                            # the 64-channel levels only
    assert err_own <= 2 * err_parent, (err_own, err_parent)


def test_full_sd_decoder_runs_every_layer_on_own_kernels(ops):
    """ch = (128, 256, 512, 512) at latent (1, 4, 64, 64), f16: a 512 x 512 image, 4096 tokens in the mid block.  No fp64
    reference at this size: finite, and within 3 x the small decoder's err_parent of the framework decode."""
    from guided_attention_amd.vae import AutoencoderKLDecoder
    err_parent = case("f16")["err_parent"]
    vae = seed_parameters(AutoencoderKLDecoder().init_weights_(), seed=11)
    make_pipe(vae, torch.float16)
    lat = torch.from_numpy(np.ascontiguousarray(hashrand.normalish((1, 4, 64, 64), 47))).to("cuda", torch.float16)
    with torch.no_grad():
        parent = vae.decode(lat / vae.scaling_factor)
    own, names = census_names(ops, lambda: vae.decode_own(lat, 1.0 / vae.scaling_factor))
    assert own.shape == parent.shape == (1, 3, 512, 512)
    assert torch.isfinite(own).all() and torch.isfinite(parent).all()
    diff = float((own.double() - parent.double()).abs().max() / parent.double().abs().max())
    print(f"\nfull SD decoder f16: own against framework {diff:.3e} (bound {3 * err_parent:.3e})")
    assert diff <= 3 * err_parent
    assert names["latent_affine4"] == 1 and names["conv3x3_thin_in"] == 1 and names["conv3x3_thin_out"] == 1
    assert names["attn_wide_fwd"] == 1 and names["conv3x3"] == 31
    assert names["group_norm_fwd"] + names["group_norm_apply"] == 30
    assert names["linear"] == 4                                 # shortcuts 512 -> 256 and 256 -> 128, q|k|v, proj_attn
