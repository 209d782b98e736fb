"""AutoencoderKL decoder (SD-1.x / 2.x layout): latents -> image.  Caller of the hot path (`decode_latents`,
pipeline_guided_attention.py); reproduced so `.images[0]` exists, and outside the images/sec metric.
Parameter names follow the diffusers checkpoint layout (`post_quant_conv`, `decoder.*`).

Two forwards over the same parameters:

  * `decode` / `forward` — plain PyTorch (MIOpen convolutions, NCHW GroupNorm, `scaled_dot_product_attention`), not accelerated.
    The default, what the CPU runs and what every fp32 pipeline runs.
  * `decode_own` / `own` — the package's gfx950 kernels, channels-last between layers, under `no_grad`; taken by
    `GuidedAttention.decode_latents` when `own_vae_decode` is on (16-bit, GPU).  The kernels are handed in by
    `set_own_kernels` (GuidedAttention.to()), as the UNet's implementation attributes are:
        conv_in              ga_conv3x3_thin_in                      (W % 16 == 0, C % 64 == 0)
        3x3 convolutions     ga_conv3x3_nhwc, bias (+ skip) epilogue (channels % 64 == 0 both sides)
        up-samplers          ga_conv3x3_up2x_nhwc (no up-sampled tensor), else interpolate + ga_conv3x3_nhwc
        GroupNorm (+ SiLU)   ga_group_norm_fwd
        1x1 shortcuts, q/k/v (one GEMM), proj_attn (+ residual)      ga_linear_fused (in % 64 == 0, out % 16 == 0)
        mid-block attention  ga_self_attn_fwd (width <= 160), ga_attn_wide_fwd (width <= 512, % 64 == 0)
        conv_out             ga_conv3x3_thin_out on a weight padded to four output channels
        scale + post_quant   ga_latent_affine4
    A layer outside its kernel's envelope runs its framework code; nothing raises.  Measured against the framework path by
    tools/micro/vae_decode_bench.py (profiles/vae_decode.json; DESIGN section 7 states the figures).
"""
import types

import torch
import torch.nn as nn
import torch.nn.functional as F

# The convolution and Linear kernels address their input with 32-bit BYTE offsets and refuse one of 2^31 bytes or more
# (csrc/conv3x3.hip, csrc/linear.hip: `xb >= 1 << 31 -> GA_ERR_SHAPE`), i.e. 2^30 16-bit elements: the largest activation
# of one decode launch stays strictly below that.  GroupNorm, the thin convolutions and the attention index with 64 bits.
MAX_CHUNK_ELEMS = 2 ** 30 - 1


def _tokens(x):
    b, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(b, h * w, c)   # a view when x is channels-last


def _images(t, h, w):
    b, _, c = t.shape
    return t.reshape(b, h, w, c).permute(0, 3, 1, 2)    # channels-last strides, no copy


def _half(x):
    return x.is_cuda and x.dtype in (torch.float16, torch.bfloat16)


def _own_norm(k, norm, x, act):
    if _half(x) and norm.weight.dtype == x.dtype:
        return k.ops.group_norm_act(x, norm.weight, norm.bias, norm.num_groups, norm.eps, act)
    y = norm(x)
    return F.silu(y) if act else y


def _own_conv3x3(k, conv, x, residual=None):
    w = conv.weight
    if w.dtype == x.dtype and k.ops.conv3x3_supported(x, w, 1):
        return k.ops.conv3x3_nhwc(x, k.ops.conv3x3_packed_weights(w, False), w.shape[0], 1, conv.bias, residual)
    y = conv(x)
    return y if residual is None else y + residual


def _own_linear(k, x, weight, bias, residual=None):
    """x (B, N, K) tokens -> (B, N, out)."""
    if weight.dtype == x.dtype and x.is_contiguous() and k.lin.supported(x, weight.shape[1], weight.shape[0]) and \
            (residual is None or residual.is_contiguous()):
        return k.ops.linear_fused(x, weight, bias, residual=residual)["y"]
    y = F.linear(x, weight, bias)
    return y if residual is None else y + residual


def padded_conv_out(weight, bias):
    """(3, C, 3, 3), (3,) -> (4, C, 3, 3), (4,): a zero fourth output channel and a zero bias for it, what
    ga_conv3x3_thin_out (Cout = 4) takes.  Channels 0..2 of the padded convolution are the original's, channel 3 is 0."""
    cout = weight.shape[0]
    w = weight.new_zeros((4,) + tuple(weight.shape[1:]))
    w[:cout] = weight
    b = weight.new_zeros((4,))
    if bias is not None:
        b[:cout] = bias
    return w, b


class _Resnet(nn.Module):
    kernels = None   # set_own_kernels

    def __init__(self, cin, cout):
        super().__init__()
        self.norm1 = nn.GroupNorm(32, cin, eps=1e-6)
        self.conv1 = nn.Conv2d(cin, cout, 3, padding=1)
        self.norm2 = nn.GroupNorm(32, cout, eps=1e-6)
        self.conv2 = nn.Conv2d(cout, cout, 3, padding=1)
        self.conv_shortcut = nn.Conv2d(cin, cout, 1) if cin != cout else None

    def forward(self, x):
        h = self.conv1(F.silu(self.norm1(x)))
        h = self.conv2(F.silu(self.norm2(h)))
        return (x if self.conv_shortcut is None else self.conv_shortcut(x)) + h

    def own(self, x):
        k = self.kernels
        h = _own_conv3x3(k, self.conv1, _own_norm(k, self.norm1, x, True))
        h = _own_norm(k, self.norm2, h, True)
        if self.conv_shortcut is not None:
            sc = self.conv_shortcut
            _, _, hh, ww = x.shape
            x = _images(_own_linear(k, _tokens(x), sc.weight.reshape(sc.out_channels, sc.in_channels), sc.bias), hh, ww)
        return _own_conv3x3(k, self.conv2, h, residual=x)   # bias + skip connection in the epilogue


class _Attn(nn.Module):  # single-head spatial self-attention of the VAE mid block
    kernels = None

    def __init__(self, c):
        super().__init__()
        self.group_norm = nn.GroupNorm(32, c, eps=1e-6)
        self.query, self.key, self.value, self.proj_attn = (nn.Linear(c, c) for _ in range(4))

    def forward(self, x):
        b, c, h, w = x.shape
        t = self.group_norm(x).view(b, c, h * w).transpose(1, 2)
        q, k, v = self.query(t)[:, None], self.key(t)[:, None], self.value(t)[:, None]
        o = F.scaled_dot_product_attention(q, k, v)[:, 0]
        return x + self.proj_attn(o).transpose(1, 2).reshape(b, c, h, w)

    def fused_qkv(self):
        """[query | key | value] weights row-concatenated and their biases, built once and rebuilt when one of them changes
        (parameter names / state_dict are untouched)."""
        ps = (self.query.weight, self.key.weight, self.value.weight, self.query.bias, self.key.bias, self.value.bias)
        key = tuple((p.data_ptr(), p._version) for p in ps)
        cache = self.__dict__.get("_qkv_cache")
        if cache is None or cache[0] != key:
            with torch.no_grad():
                cache = (key, torch.cat(ps[:3], dim=0).contiguous(), torch.cat(ps[3:], dim=0).contiguous())
            self.__dict__["_qkv_cache"] = cache
        return cache[1], cache[2]

    def own(self, x):
        k = self.kernels
        b, c, h, w = x.shape
        x = x.contiguous(memory_format=torch.channels_last)
        xt = _tokens(x)                                             # the residual, as tokens
        t = _tokens(_own_norm(k, self.group_norm, x, False))
        wqkv, bqkv = self.fused_qkv()
        qkv = _own_linear(k, t, wqkv, bqkv)                         # one GEMM: (B, HW, 3C)
        scale = c ** -0.5                                           # what scaled_dot_product_attention uses: one head of C
        if k.ops.self_attention_supported(qkv, 1, c):
            o = k.ops.self_attn_fwd(qkv, None, None, 1, scale, want_lse=False)[0]
        elif k.ops.attn_wide_supported(qkv, 1, c):
            o = k.ops.attn_wide_fwd(qkv, None, None, 1, scale)
        else:
            q, kk, v = (s[:, None] for s in qkv.split(c, dim=-1))
            o = F.scaled_dot_product_attention(q, kk, v)[:, 0]
        return _images(_own_linear(k, o, self.proj_attn.weight, self.proj_attn.bias, residual=xt), h, w)


class _Up(nn.Module):
    kernels = None

    def __init__(self, cin, cout, upsample):
        super().__init__()
        self.resnets = nn.ModuleList([_Resnet(cin if i == 0 else cout, cout) for i in range(3)])
        self.upsamplers = nn.ModuleList([nn.Module()]) if upsample else None
        if upsample:
            self.upsamplers[0].conv = nn.Conv2d(cout, cout, 3, padding=1)

    def forward(self, x):
        for r in self.resnets:
            x = r(x)
        if self.upsamplers is not None:
            x = self.upsamplers[0].conv(F.interpolate(x, scale_factor=2.0, mode="nearest"))
        return x

    def own(self, x):
        k = self.kernels
        for r in self.resnets:
            x = r.own(x)
        if self.upsamplers is not None:
            conv = self.upsamplers[0].conv
            w = conv.weight
            if w.dtype == x.dtype and k.ops.conv3x3_supported(x, w, 1):
                wp = k.ops.conv3x3_packed_weights(w, False)
                y = k.ops.conv3x3_up2x_nhwc(x, wp, w.shape[0], conv.bias)     # the up-sampling happens in the patch gather
                if y is None:                                                 # a shape the patch kernel does not serve
                    y = k.ops.conv3x3_nhwc(F.interpolate(x, scale_factor=2.0, mode="nearest"), wp, w.shape[0], 1, conv.bias)
                return y
            x = conv(F.interpolate(x, scale_factor=2.0, mode="nearest"))
        return x


class _Mid(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.resnets = nn.ModuleList([_Resnet(c, c), _Resnet(c, c)])
        self.attentions = nn.ModuleList([_Attn(c)])

    def forward(self, x):
        return self.resnets[1](self.attentions[0](self.resnets[0](x)))

    def own(self, x):
        return self.resnets[1].own(self.attentions[0].own(self.resnets[0].own(x)))


class _Decoder(nn.Module):
    kernels = None

    def __init__(self, ch=(128, 256, 512, 512), latent=4):
        super().__init__()
        rev = list(reversed(ch))
        self.conv_in = nn.Conv2d(latent, rev[0], 3, padding=1)
        self.mid_block = _Mid(rev[0])
        ups, prev = [], rev[0]
        for i, c in enumerate(rev):
            ups.append(_Up(prev, c, i != len(rev) - 1))
            prev = c
        self.up_blocks = nn.ModuleList(ups)
        self.conv_norm_out = nn.GroupNorm(32, ch[0], eps=1e-6)
        self.conv_out = nn.Conv2d(ch[0], 3, 3, padding=1)

    def forward(self, z):
        x = self.mid_block(self.conv_in(z))
        for u in self.up_blocks:
            x = u(x)
        return self.conv_out(F.silu(self.conv_norm_out(x)))

    def padded_out(self):
        """padded_conv_out of conv_out, cached per (weight, bias) storage and version like the other packs (the thin kernel's
        own pack is cached on the padded tensor, which therefore has to stay the same object)."""
        w, b = self.conv_out.weight, self.conv_out.bias
        key = (w.data_ptr(), w._version, b.data_ptr(), b._version, w.dtype)
        cache = self.__dict__.get("_out_cache")
        if cache is None or cache[0] != key:
            with torch.no_grad():
                cache = (key,) + padded_conv_out(w, b)
            self.__dict__["_out_cache"] = cache
        return cache[1], cache[2]

    def own(self, z):
        """z (B, 4, h, w) dense NCHW -> (B, 3, 8h, 8w); activations stay channels-last between the layers."""
        k = self.kernels
        ci = self.conv_in
        if ci.weight.dtype == z.dtype and k.ops.conv3x3_thin_supported(z, ci.weight, forward_only=True):
            x = k.ops.conv3x3_thin(z, k.ops.conv3x3_thin_packed_weights(ci.weight, False), ci.out_channels, ci.bias)
        else:
            x = ci(z).contiguous(memory_format=torch.channels_last)
        x = self.mid_block.own(x)
        for u in self.up_blocks:
            x = u.own(x)
        x = _own_norm(k, self.conv_norm_out, x, True)
        co = self.conv_out
        if co.out_channels == 3 and co.weight.dtype == x.dtype:
            w4, b4 = self.padded_out()
            if k.ops.conv3x3_thin_supported(x, w4, forward_only=True):
                return k.ops.conv3x3_thin(x, k.ops.conv3x3_thin_packed_weights(w4, False), 4, b4)[:, :3]
        return co(x)


class AutoencoderKLDecoder(nn.Module):
    scaling_factor = 0.18215
    kernels = None

    def __init__(self, ch=(128, 256, 512, 512)):
        super().__init__()
        self.ch = tuple(ch)
        self.post_quant_conv = nn.Conv2d(4, 4, 1)
        self.decoder = _Decoder(ch)

    @classmethod
    def tiny(cls):
        return cls(ch=(32, 32, 64, 64))

    def decode(self, z):
        return self.decoder(self.post_quant_conv(z))

    def decode_own(self, latents, pre_scale=1.0):
        """decode(pre_scale * latents) on the package's kernels (see the module docstring): 16-bit latents on the GPU, no
        autograd.  One launch sequence for the whole batch: the caller keeps it within decode_chunks."""
        k = self.kernels
        if k is None:
            from ._lib import GaError
            raise GaError("the VAE has no kernels installed: move the pipeline to the GPU with GuidedAttention.to() "
                          "(vae.set_own_kernels) before decoding with own_vae_decode")
        with torch.no_grad():
            pq = self.post_quant_conv
            z = k.ops.latent_affine4(latents, pq.weight, pq.bias, pre_scale)
            return self.decoder.own(z)

    def init_weights_(self, seed=1):
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for n, p in self.named_parameters():
                if n.endswith("bias"):
                    p.zero_()
                elif p.dim() == 1:
                    p.fill_(1.0)
                else:
                    p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * (3.0 / p[0].numel()) ** 0.5)
        return self


class _Kernels(types.SimpleNamespace):
    """The kernel modules a layer's `own` forward calls.  Shared, never copied: a deep copy of the VAE keeps the same handles
    (Python modules cannot be copied)."""

    def __deepcopy__(self, memo):
        return self


def set_own_kernels(vae, ops, fused_linear):
    """Hand the kernel modules to every layer of the decoder that has an `own` forward (GuidedAttention.to() on the GPU).
    Nothing else changes: `decode` stays the framework path."""
    k = _Kernels(ops=ops, lin=fused_linear) if ops is not None else None
    for m in vae.modules():
        if isinstance(m, (_Resnet, _Attn, _Up, _Decoder, AutoencoderKLDecoder)):
            m.kernels = k


def largest_activation(h, w, channels):
    """Elements per image of the largest activation of a decode of (h, w) latents: ch[1] x 8h x 8w for the SD decoder (the
    input of the last up block); the maximum over the levels for any other channel list."""
    rev = list(reversed(channels))
    best, prev = 0, rev[0]
    for i, c in enumerate(rev):
        best = max(best, max(prev, c) * 4 ** i)
        if i != len(rev) - 1:
            best = max(best, c * 4 ** (i + 1))
        prev = c
    return best * h * w


def decode_chunks(images, h, w, channels, budget=MAX_CHUNK_ELEMS):
    """[(first, last)) image ranges of the decode launches for `images` latents of (h, w): the largest activation of a chunk
    stays at or below `budget` elements (MAX_CHUNK_ELEMS: what the kernels' 32-bit byte offsets allow), and a chunk is never
    smaller than one image."""
    per = max(1, int(budget) // largest_activation(h, w, channels))
    return [(a, min(a + per, images)) for a in range(0, images, per)]
