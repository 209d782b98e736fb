"""The VAE decode on own kernels (own_vae_decode) without a GPU: the two new entries are declared, bound, exported and validate
their arguments on the host; the switch exists, defaults to off, is a CLI flag and leaves an fp32 pipeline on the framework
path; the chunking arithmetic; the padded conv_out weight against conv2d."""
import ctypes
import re
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

HEADER = ROOT / "include" / "ga_hip.h"
SD_CHANNELS = (128, 256, 512, 512)
OK, NULL, SHAPE, DTYPE, ALIGN, UNSUPPORTED = 0, -1, -2, -3, -4, -6


@pytest.fixture(scope="module")
def lib():
    from guided_attention_amd import _lib
    if not _lib.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_entries_are_declared_bound_and_exported(lib):
    from guided_attention_amd import _lib, ops
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert re.search(r"\bint ga_attn_wide_fwd\s*\(", text)
    assert re.search(r"\bint ga_latent_affine4\s*\(", text)
    assert len(_lib.PROTOTYPES["ga_attn_wide_fwd"]) == 12
    assert len(_lib.PROTOTYPES["ga_latent_affine4"]) == 9
    assert hasattr(lib, "ga_attn_wide_fwd") and hasattr(lib, "ga_latent_affine4")
    assert int(re.search(r"#define GA_VERSION (\d+)", text).group(1)) == _lib.GA_VERSION == lib.ga_version() == 183
    for name in ("attn_wide_supported", "attn_wide_fwd", "latent_affine4"):
        assert hasattr(ops, name)


def test_attn_wide_validates_on_the_host(lib):
    p = ctypes.c_void_p(4096)   # never dereferenced: every call below returns before a launch
    f16, bf16, f32 = 0, 1, 2

    def call(Q=p, K=p, V=p, O=p, B=1, H=1, N=64, D=512, ld=0, dtype=f16):
        return lib.ga_attn_wide_fwd(Q, K, V, O, B, H, N, D, ld, 0.5, dtype, None)

    for name in ("Q", "K", "V", "O"):
        assert call(**{name: None}) == NULL
    for kw in (dict(B=0), dict(H=0), dict(N=0), dict(N=-3)):
        assert call(**kw) == SHAPE
    for D in (0, 32, 96, 160, 520, 576, 1024, -64):          # outside 64 .. 512, or not a multiple of 64
        assert call(D=D) == SHAPE
    assert call(H=2, D=256, ld=2 * 256) == SHAPE              # a row stride that is neither 0 nor 3*H*D
    assert call(H=2, D=256, ld=3 * 2 * 256 + 8) == SHAPE
    for name in ("Q", "K", "V", "O"):
        assert call(**{name: ctypes.c_void_p(4104)}) == ALIGN   # 8-byte aligned is not enough
    assert call(dtype=f32) == UNSUPPORTED
    assert call(dtype=f32, D=64) == UNSUPPORTED
    assert call(dtype=3) == DTYPE
    assert call(dtype=-1) == DTYPE
    assert call(dtype=bf16, D=100) == SHAPE


def test_latent_affine4_validates_on_the_host(lib):
    p = ctypes.c_void_p(4096)
    f = lib.ga_latent_affine4
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        x, W, b, out = args
        assert f(x, W, b, 1.0, out, 1, 256, 0, None) == NULL
    assert f(p, p, p, 1.0, p, 0, 256, 0, None) == SHAPE
    assert f(p, p, p, 1.0, p, -1, 256, 0, None) == SHAPE
    assert f(p, p, p, 1.0, p, 1, 0, 0, None) == SHAPE
    assert f(p, p, p, 1.0, p, 1, -7, 0, None) == SHAPE
    assert f(p, p, p, 1.0, p, 1, 256, 3, None) == DTYPE
    assert f(p, p, p, 1.0, p, 1, 256, -1, None) == DTYPE


def test_wrappers_refuse_cpu_tensors():
    from guided_attention_amd import ops
    q = torch.zeros((1, 8, 512), dtype=torch.float16)
    assert not ops.attn_wide_supported(q, 1)
    with pytest.raises(ops.GaError, match="GPU only"):
        ops.attn_wide_fwd(q, q, q, 1, 512 ** -0.5)
    with pytest.raises(ops.GaError, match="GPU only"):
        ops.latent_affine4(torch.zeros((1, 4, 8, 8)), torch.zeros((4, 4, 1, 1)), torch.zeros(4), 1.0)


def test_switch_defaults_to_off_and_is_a_cli_flag():
    from guided_attention_amd import run
    from guided_attention_amd.config import RunConfig
    from guided_attention_amd.pipeline_guided_attention import GuidedAttention
    pipe = GuidedAttention(SimpleNamespace(dtype=torch.float32, device=torch.device("cpu")))
    assert pipe.own_vae_decode is False
    assert RunConfig(meta_prompt="a").own_vae_decode is False
    base = ["--meta_prompt", "a [robot:.6,.3,.4,.55]", "--output_path", "/tmp/ga_own_vae"]
    assert run._parse_cli(base + ["--own_vae_decode", "true"]).own_vae_decode is True
    assert run._parse_cli(base).own_vae_decode is False


def test_fp32_pipeline_keeps_the_framework_path_with_the_switch_on():
    from guided_attention_amd.pipeline_guided_attention import GuidedAttention
    seen = []

    class StubVae:
        scaling_factor = 0.5
        ch = SD_CHANNELS

        def decode(self, z):
            seen.append(("decode", z.clone()))
            return z[:, :3].repeat_interleave(8, 2).repeat_interleave(8, 3)

        def decode_own(self, *a, **k):
            raise AssertionError("an fp32 pipeline must not take the own-kernel decode")

    pipe = GuidedAttention(SimpleNamespace(dtype=torch.float32, device=torch.device("cpu")), vae=StubVae())
    pipe.own_vae_decode = True
    lat = torch.arange(2 * 4 * 2 * 2, dtype=torch.float32).reshape(2, 4, 2, 2) / 64
    img = pipe.decode_latents(lat)
    assert [s[0] for s in seen] == ["decode"] and torch.equal(seen[0][1], lat / 0.5)      # one launch sequence, no chunking
    assert img.shape == (2, 16, 16, 3) and img.dtype.name == "float32" and img.min() >= 0 and img.max() <= 1
    pipe.own_vae_decode = False
    assert (pipe.decode_latents(lat) == img).all()


def test_decode_chunks():
    from guided_attention_amd import vae
    sizes = lambda chunks: [b - a for a, b in chunks]  # noqa: E731
    # the issue's arithmetic: 256 channels x 512 x 512 = 2^26 elements per image, 16 images in 2^30
    assert vae.largest_activation(64, 64, SD_CHANNELS) == 256 * 512 * 512
    assert sizes(vae.decode_chunks(64, 64, 64, SD_CHANNELS, budget=2 ** 30)) == [16, 16, 16, 16]
    # the bound the kernels set is one element lower (csrc/conv3x3.hip and csrc/linear.hip refuse an input of 2^31 bytes):
    # 15 images of 512^2 per chunk by default
    assert vae.MAX_CHUNK_ELEMS == 2 ** 30 - 1
    assert sizes(vae.decode_chunks(64, 64, 64, SD_CHANNELS)) == [15, 15, 15, 15, 4]
    assert vae.decode_chunks(3, 16, 16, SD_CHANNELS) == [(0, 3)]
    assert vae.decode_chunks(1, 96, 96, SD_CHANNELS) == [(0, 1)]
    assert vae.decode_chunks(3, 64, 64, SD_CHANNELS, budget=1000) == [(0, 1), (1, 2), (2, 3)]     # never below one image
    assert vae.decode_chunks(3, 16, 16, (64, 64, 128, 512), budget=2 * 64 * 128 * 128) == [(0, 2), (2, 3)]
    got = vae.decode_chunks(64, 64, 64, SD_CHANNELS)
    assert got[0][0] == 0 and got[-1][1] == 64 and all(a[1] == b[0] for a, b in zip(got, got[1:]))


def test_padded_conv_out_is_the_same_convolution():
    from guided_attention_amd.vae import AutoencoderKLDecoder, padded_conv_out
    g = torch.Generator().manual_seed(5)
    w = torch.randn((3, 64, 3, 3), generator=g) / 24
    b = torch.randn((3,), generator=g)
    x = torch.randn((2, 64, 9, 7), generator=g)
    w4, b4 = padded_conv_out(w, b)
    assert w4.shape == (4, 64, 3, 3) and b4.shape == (4,)
    y4 = F.conv2d(x, w4, b4, padding=1)
    assert torch.equal(y4[:, :3], F.conv2d(x, w, b, padding=1))
    assert torch.equal(y4[:, 3], torch.zeros_like(y4[:, 3]))
    # the decoder caches the pad per weight version
    dec = AutoencoderKLDecoder.tiny().init_weights_().decoder
    first = dec.padded_out()
    assert dec.padded_out()[0] is first[0]
    with torch.no_grad():
        dec.conv_out.weight.mul_(2.0)
    again = dec.padded_out()
    assert again[0] is not first[0] and torch.equal(again[0][:3], dec.conv_out.weight) and not again[0][3].any()


def test_installed_kernels_leave_decode_and_deepcopy_alone():
    import copy
    from guided_attention_amd import fused_linear, ops
    from guided_attention_amd.vae import AutoencoderKLDecoder, set_own_kernels
    vae = AutoencoderKLDecoder.tiny().init_weights_()
    z = torch.randn((1, 4, 4, 4), generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        before = vae.decode(z)
    keys = list(vae.state_dict())
    set_own_kernels(vae, ops, fused_linear)
    twin = copy.deepcopy(vae).double()
    assert twin.kernels is vae.kernels and twin.decoder.mid_block.attentions[0].kernels is vae.kernels
    with torch.no_grad():
        assert torch.equal(vae.decode(z), before)
    assert list(vae.state_dict()) == keys


def test_own_decode_without_installed_kernels_is_an_error():
    from guided_attention_amd import ops
    from guided_attention_amd.vae import AutoencoderKLDecoder
    with pytest.raises(ops.GaError, match="no kernels installed"):
        AutoencoderKLDecoder.tiny().decode_own(torch.zeros((1, 4, 8, 8)))
