"""Block-level parity of the 16-bit product path: real UNet blocks (SD-1.x, SD-2.1, SDXL widths, real map sizes) with the
kernels the pipeline installs (pipeline_guided_attention.install_kernels), against the SAME blocks in fp64 on the CPU.

The per-kernel suite (test_kernels_gpu.py) holds every entry point to fp64; what it cannot see is the wiring between them:
which parameter each module hands to which kernel, the producer -> GroupNorm statistics handoffs (convolution epilogue,
concatenation partials and "done", proj_out), the gradient aliases (GroupNorm `g_alias`, LayerNorm `g_pass`), the LayerNorm
fold's shift, conv1's bias on the time projection.  The UNet-level tests build their weights with every bias 0 and every norm
gamma = 1 / beta = 0, where dropping or swapping any of those parameters changes nothing.  Here every bias is non-zero, every
norm has gamma = 1 + 0.3 N(0, 1) and beta = 0.2 N(0, 1), and the activations carry per-channel offsets of up to 4 standard
deviations (what trained activations look like, and what a one-pass variance has to survive).

The objective is a vector-Jacobian product: L = sum_i <output_i, cotangent_i> (+ <P, gP> over the captured 16 x 16 cross maps,
as the guidance loss reaches them), so the gradient to the block input and to every skip tensor is compared as well.  Two
metrics per tensor: max |got - ref| / max |ref|, and the worst relative L2 error over one (image, GroupNorm group) slab — an
error confined to one group, channel slice or image is diluted below the first and not below the second.
Needs an MI355X (`pytest -m gpu`)."""
import copy
import math
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

GROUPS = 32


@pytest.fixture(autouse=True)
def _gpu_state():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from guided_attention_amd import ops
    from guided_attention_amd.utils import shared_state as state
    ops.load()
    saved = state.curHyperParams
    state.curHyperParams = dict(state.hyperParameterOverrides, paint_with_words_stop=0)   # no paint-with-words bias
    yield
    state.curHyperParams = saved


# ------------------------------------------------------------------------------------------------ blocks from a real config
def _levels(cfg):
    ch = cfg.block_out_channels
    heads = cfg.attention_head_dim if isinstance(cfg.attention_head_dim, (tuple, list)) else (cfg.attention_head_dim,) * len(ch)
    tl = cfg.transformer_layers_per_block
    depth = tuple(tl) if isinstance(tl, (tuple, list)) else (tl,) * len(ch)
    return ch, heads, depth, ch[0] * 4


def down_block(cfg, i):
    """down_blocks[i] exactly as UNet2DConditionModel.__init__ builds it (DownBlock sets its own feeds_norm flags)."""
    from guided_attention_amd.unet import DownBlock
    ch, heads, depth, temb_c = _levels(cfg)
    in_c = ch[max(i - 1, 0)]
    return DownBlock(cfg, in_c, ch[i], temb_c, heads[i], i != len(ch) - 1, cfg.down_block_types[i] == "CrossAttnDownBlock2D",
                     depth[i])


def mid_block(cfg):
    from guided_attention_amd.unet import MidBlock
    ch, heads, depth, temb_c = _levels(cfg)
    return MidBlock(cfg, ch[-1], temb_c, heads[-1], depth[-1])


def up_block(cfg, i):
    """up_blocks[i] as the UNet builds it; the last one's last attention feeds conv_norm_out, as in the UNet."""
    from guided_attention_amd.unet import UpBlock
    ch, heads, depth, temb_c = _levels(cfg)
    rev, rev_heads, rev_depth = list(reversed(ch)), list(reversed(heads)), list(reversed(depth))
    prev_c = rev[max(i - 1, 0)]
    in_c = rev[min(i + 1, len(ch) - 1)]
    blk = UpBlock(cfg, in_c, rev[i], prev_c, temb_c, rev_heads[i], i != len(ch) - 1,
                  cfg.up_block_types[i] == "CrossAttnUpBlock2D", rev_depth[i])
    if i == len(ch) - 1 and blk.has_cross_attention:
        blk.attentions[-1].feeds_norm = True
    return blk


class UpWithNormOut(nn.Module):
    """The last SD-1.x UpBlock followed by a GroupNorm(+SiLU) standing in for conv_norm_out, so that the handoff of the block's
    last proj_out epilogue is consumed."""

    def __init__(self, blk, cfg):
        super().__init__()
        from guided_attention_amd.unet import GroupNormAct
        self.blk = blk
        self.norm_out = GroupNormAct(cfg.norm_num_groups, cfg.block_out_channels[0], eps=cfg.norm_eps, act=True)

    def forward(self, x, skips, temb_act, context):
        return self.norm_out(self.blk(x, skips, temb_act, context))


class DownPrefix(nn.Module):
    """resnets[0] -> attentions[0] -> resnets[1] of a DownBlock (the SDXL 10-deep level: one of its two transformers keeps the
    fp64 reference within host memory).  attentions[0].feeds_norm is set as in the full block: resnets[1].norm1 reads it."""

    def __init__(self, blk):
        super().__init__()
        self.blk = blk

    def forward(self, x, temb_act, context):
        b = self.blk
        h = b.attentions[0](b.resnets[0](x, temb_act), context)
        return b.resnets[1](h, temb_act), [h]


# ------------------------------------------------------------------------------------------------ parameters / inputs
def nontrivial_init_(module, seed, dtype):
    """Weights: uniform with unit gain.  Biases: magnitude 0.1 ... 0.3, random sign.  GroupNorm / LayerNorm: gamma =
    1 + 0.3 N(0, 1), beta = 0.2 N(0, 1).  Everything rounded to `dtype`, so a 16-bit copy and an fp64 copy hold identical values."""
    g = torch.Generator().manual_seed(seed)
    norm_params = set()
    for m in module.modules():
        if isinstance(m, (nn.GroupNorm, nn.LayerNorm)):
            norm_params.update({id(m.weight), id(m.bias)})
    with torch.no_grad():
        for name, p in module.named_parameters():
            if id(p) in norm_params:
                if name.endswith("weight"):
                    v = 1.0 + 0.3 * torch.randn(p.shape, generator=g)
                else:
                    v = 0.2 * torch.randn(p.shape, generator=g)
            elif name.endswith("bias"):
                sign = torch.randint(0, 2, p.shape, generator=g) * 2 - 1
                v = sign * (0.1 + 0.2 * torch.rand(p.shape, generator=g))
            else:
                v = (torch.rand(p.shape, generator=g) * 2 - 1) * math.sqrt(3.0 / p[0].numel())
            p.copy_(v.to(dtype).to(p.dtype))
    for p in module.parameters():
        p.requires_grad_(False)
    return module


def activation(g, B, C, H, W, dtype):
    """(B, C, H, W) with per-channel offsets of up to +-4 standard deviations, rounded to dtype, as fp64 on the CPU."""
    off = (torch.rand(1, C, 1, 1, generator=g, dtype=torch.float64) * 2 - 1) * 4.0
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64) + off
    return x.to(dtype).double()


def rounded(t, dtype):
    return t.to(dtype).double()


def to_gpu(t, dtype):
    t = t.to("cuda", dtype)
    return t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t


# ------------------------------------------------------------------------------------------------ the two runs
class Case(SimpleNamespace):
    pass


def build_case(kind, cfg, idx, dtype, batch, seed):
    """-> Case with .module (fp64 master, parameters rounded to dtype) and the fp64 CPU inputs x, skips, temb_act, context."""
    if kind == "down":
        mod = down_block(cfg, idx)
    elif kind == "down_prefix":
        mod = DownPrefix(down_block(cfg, idx))
    elif kind == "mid":
        mod = mid_block(cfg)
    else:
        blk = up_block(cfg, idx)
        mod = UpWithNormOut(blk, cfg) if idx == len(cfg.block_out_channels) - 1 else blk
    nontrivial_init_(mod.double(), seed, dtype)
    ch, _, _, temb_c = _levels(cfg)
    n = len(ch)
    g = torch.Generator().manual_seed(seed + 1)
    side = cfg.sample_size
    if kind in ("down", "down_prefix"):
        hw, cin = side >> idx, ch[max(idx - 1, 0)]
    elif kind == "mid":
        hw, cin = side >> (n - 1), ch[-1]
    else:
        hw, cin = side >> (n - 1 - idx), list(reversed(ch))[max(idx - 1, 0)]
    x = activation(g, batch, cin, hw, hw, dtype)
    skips = []
    if kind == "up":
        blk = mod.blk if isinstance(mod, UpWithNormOut) else mod
        nres = len(blk.resnets)
        # consumed from the end: resnets[j] pops the skip of width in_c for its last layer, out_c before that
        for j in reversed(range(nres)):
            c_res = blk.resnets[j].norm1.num_channels - (cin if j == 0 else blk.resnets[0].conv1.out_channels)
            skips.append(activation(g, batch, c_res, hw, hw, dtype))
    temb = torch.randn(batch, temb_c, generator=g, dtype=torch.float64)
    temb_act = rounded(torch.nn.functional.silu(temb), dtype)
    context = rounded(torch.randn(batch, 77, cfg.cross_attention_dim, generator=g, dtype=torch.float64), dtype)
    return Case(kind=kind, module=mod, x=x, skips=skips, temb_act=temb_act, context=context, dtype=dtype, hw=hw, seed=seed)


def _call(case, mod, x, skips, temb_act, context):
    if case.kind in ("down", "down_prefix"):
        y, outs = mod(x, temb_act, context)
        return [y] + list(outs)
    if case.kind == "mid":
        return [mod(x, temb_act, context)]
    return [mod(x, list(skips), temb_act, context)]


def _place(case):
    return {"down": "down", "down_prefix": "down", "mid": "mid", "up": "up"}[case.kind]


class _checkpointed:
    """Each BasicTransformerBlock of the fp64 reference recomputes its forward in the backward (the 64 x 64 self-attention holds
    8 x 4096^2 doubles = 1 GB per probability tensor; SDXL's level has 10 blocks in a row): host memory stays at about one
    block's worth."""

    def __init__(self, module):
        from guided_attention_amd.unet import BasicTransformerBlock
        self.blocks = [m for m in module.modules() if isinstance(m, BasicTransformerBlock)]

    def __enter__(self):
        from torch.utils.checkpoint import checkpoint
        for m in self.blocks:
            m.forward = (lambda f: lambda x, ctx: checkpoint(f, x, ctx, use_reentrant=False))(m.forward)

    def __exit__(self, *exc):
        for m in self.blocks:
            del m.forward


def cotangents(case, outs_shapes, scale=1.0):
    g = torch.Generator().manual_seed(case.seed + 7)
    cots = [rounded(torch.randn(s, generator=g, dtype=torch.float64), case.dtype) for s in outs_shapes]
    gp = rounded(1e-3 * torch.randn(case.hw * case.hw, 77, generator=g, dtype=torch.float64), case.dtype)
    return [c * scale for c in cots], gp * scale


_REF = {}


def reference(case, grad=True):
    """fp64 CPU run of a deep copy, no kernels installed, oracle attention processors.  -> (outputs, [grad x, grad skips...])."""
    from oracle import attention as oattn
    key = (case.key, grad)
    if key in _REF:
        return _REF[key]
    from guided_attention_amd.unet import Attention
    mod = case.module                       # fp64 already: the reference runs on the master copy
    store = oattn.OracleStore(max_pixels=256)
    for m in mod.modules():
        if isinstance(m, Attention):
            m.set_processor(oattn.OracleAttnProcessor(store, _place(case)))
    if not grad:
        with torch.no_grad():
            outs = _call(case, mod, case.x, case.skips, case.temb_act, case.context)
        res = ([o.detach() for o in outs], None, None)
        _REF[key] = res
        for m in mod.modules():
            if isinstance(m, Attention):
                m.set_processor(None)
        return res
    x = case.x.clone().requires_grad_(True)
    skips = [s.clone().requires_grad_(True) for s in case.skips]
    with _checkpointed(mod):
        outs = _call(case, mod, x, skips, case.temb_act, case.context)
        maps = [p for p in store.step_store["%s_cross" % _place(case)] if p.shape[1] == 256]
        cots, gp = cotangents(case, [o.shape for o in outs])
        L = sum((o * c).sum() for o, c in zip(outs, cots))
        for p in maps:
            L = L + (p * gp).sum()
        grads = torch.autograd.grad(L, [x] + skips)
    res = ([o.detach() for o in outs], list(grads), len(maps))
    _REF[key] = res
    for m in mod.modules():                 # the master leaves with the default processors again
        if isinstance(m, Attention):
            m.set_processor(None)
    return res


def product(case, grad=True, scale=1.0, capture="loss-only"):
    """The 16-bit product path on the GPU: the module with the kernels the pipeline installs, the product's attention
    processor with an AttentionStore.  -> (outputs, grads, number of 16 x 16 cross maps, launch census, concatenation forms)."""
    from guided_attention_amd import ops
    from guided_attention_amd.pipeline_guided_attention import install_kernels
    from guided_attention_amd.unet import Attention, UpBlock
    from guided_attention_amd.utils import ptp_utils
    # a copy whose parameters are the master's values in the test dtype on the GPU (no second host copy of the master)
    memo = {id(p): nn.Parameter(p.detach().to("cuda", case.dtype), requires_grad=False) for p in case.module.parameters()}
    mod = copy.deepcopy(case.module, memo)
    install_kernels(mod)
    store = ptp_utils.AttentionStore(capture=capture)
    store.num_att_layers = 1 << 30          # one open step: everything captured stays in step_store
    for m in mod.modules():
        if isinstance(m, Attention):
            m.set_processor(ptp_utils.AttendExciteCrossAttnProcessor(store, _place(case)))
    forms = []
    for m in mod.modules():                 # which concatenation form each UpBlock layer took
        if isinstance(m, UpBlock) and m.cat_impl is not None:
            def cat(a, b, _f=m.cat_impl, **kw):
                y = _f(a, b, **kw)
                pre = getattr(y, "_ga_gn", None)
                forms.append("none" if pre is None else ("done" if "done" in pre else "partials"))
                return y
            m.cat_impl = cat
    T = case.dtype
    with ops.census_scope() as cs, torch.set_grad_enabled(grad):
        x = to_gpu(case.x, T).requires_grad_(grad)
        skips = [to_gpu(s, T).requires_grad_(grad) for s in case.skips]
        outs = _call(case, mod, x, skips, to_gpu(case.temb_act, T), to_gpu(case.context, T))
        grads, n_maps = None, None
        if grad:
            maps = [p for p in store.step_store["%s_cross" % _place(case)]
                    if not isinstance(p, ptp_utils.ProbsNotCaptured) and p.shape[1] == 256]
            cots, gp = cotangents(case, [o.shape for o in outs], scale)
            L = sum((o.float() * to_gpu(c, T).float()).sum() for o, c in zip(outs, cots))
            gp = gp.to("cuda", T).float()
            for p in maps:
                L = L + (p.float() * gp).sum()
            grads = [g.detach().double().cpu() for g in torch.autograd.grad(L, [x] + skips)]
            n_maps = len(maps)
        torch.cuda.synchronize()
    kinds = {}
    for k, n in cs.launches.items():
        kinds[k[0]] = kinds.get(k[0], 0) + n
    return [o.detach().double().cpu() for o in outs], grads, n_maps, kinds, forms


# ------------------------------------------------------------------------------------------------ metrics
def max_rel(got, ref):
    return float((got - ref).abs().max() / ref.abs().max())


def group_rel(got, ref, groups=GROUPS):
    """Worst relative L2 error over one (image, GroupNorm group) slab of a (B, C, H, W) tensor."""
    B, C = ref.shape[:2]
    d = (got - ref).reshape(B, groups, -1).norm(dim=-1)
    r = ref.reshape(B, groups, -1).norm(dim=-1)
    return float((d / r).max())


def compare(name, got, ref, bars, report, groups=GROUPS):
    """bars = (max-rel bar, group-rel bar) for this tensor class; records the measurement in `report`."""
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{name}: non-finite values"
    m, gr = max_rel(got, ref), group_rel(got, ref, groups)
    report.append(f"{name} max-rel {m:.2e} group-rel {gr:.2e}")
    return (m, gr, bars)


def check_all(label, results):
    print(f"[measured] {label}: " + "; ".join(r for r in results["report"]))
    bad = [(n, m, gr, b) for n, (m, gr, b) in results["vals"].items() if not (m < b[0] and gr < b[1])]
    assert not bad, f"{label}: over the bar: {bad}"


def run_vjp(case, bars_out, bars_grad, scale=1.0, capture="loss-only"):
    outs_ref, grads_ref, n_ref = reference(case)
    outs, grads, n_maps, kinds, forms = product(case, True, scale, capture)
    assert n_maps == n_ref, ("captured 16 x 16 cross maps", n_maps, n_ref)
    rep, vals = [], {}
    for i, (o, r) in enumerate(zip(outs, outs_ref)):
        vals[f"out{i}"] = compare(f"out{i}", o, r, bars_out, rep)
    names = ["dx"] + [f"dskip{j}" for j in range(len(grads) - 1)]
    for nm, gt, gr in zip(names, grads, grads_ref):
        vals[nm] = compare(nm, gt / scale, gr, bars_grad, rep)
    return {"report": rep, "vals": vals}, kinds, forms


def assert_own_kernels(case, kinds, forms, grad=True):
    """The product's own kernels really ran where the shape is served."""
    from guided_attention_amd import ops
    from guided_attention_amd.unet import Transformer2DModel, UpBlock
    mod = case.module
    assert kinds.get("conv3x3", 0) > 0, kinds
    has_attn = any(isinstance(m, Transformer2DModel) for m in mod.modules())
    if has_attn:
        assert kinds.get("linear", 0) > 0, kinds
        assert kinds.get("self_attn_fwd", 0) + kinds.get("attn_capture_fwd", 0) > 0, kinds
        assert kinds.get("attn_capture_fwd", 0) > 0, kinds           # the 77-key cross-attention
    two = ops.gn_two_launch(case.hw * case.hw, mod_channels(case), GROUPS, case.dtype)
    if two:      # a producer's partial sums feed the large-map norms: the statistics launch is skipped
        assert kinds.get("group_norm_apply", 0) > 0, kinds
    if grad:
        assert kinds.get("group_norm_bwd", 0) > 0, kinds
    if any(isinstance(m, UpBlock) for m in mod.modules()):
        assert forms and "none" not in forms, forms                     # every concatenation handed the norm its data


def mod_channels(case):
    from guided_attention_amd.unet import ResnetBlock2D
    return [m for m in case.module.modules() if isinstance(m, ResnetBlock2D)][-1].conv2.out_channels


# ------------------------------------------------------------------------------------------------ the batch-1 VJP matrix
def _sd15():
    from guided_attention_amd.unet import UNetConfig
    return UNetConfig.sd15()


def _sd21():
    from guided_attention_amd.unet import UNetConfig
    return UNetConfig.sd21()


def _sdxl():
    from guided_attention_amd.unet import UNetConfig
    return UNetConfig.sdxl()


# (id, config, kind, index, dtype, seed).  SD-1.x at 512^2: maps 64 / 32 / 16 / 8; SD-2.1 at 768^2: 96 / 48 / 24 / 12;
# SDXL at 1024^2: 128 / 64 / 32.
VJP_CASES = [
    ("sd15-down0-f16", _sd15, "down", 0, torch.float16, 100),
    ("sd15-down1-f16", _sd15, "down", 1, torch.float16, 110),
    ("sd15-down2-f16", _sd15, "down", 2, torch.float16, 120),
    ("sd15-down3-f16", _sd15, "down", 3, torch.float16, 130),
    ("sd15-mid-f16", _sd15, "mid", 0, torch.float16, 140),
    ("sd15-up0-f16", _sd15, "up", 0, torch.float16, 150),
    ("sd15-up1-f16", _sd15, "up", 1, torch.float16, 160),
    ("sd15-up2-f16", _sd15, "up", 2, torch.float16, 170),
    ("sd15-up3-f16", _sd15, "up", 3, torch.float16, 180),
    ("sd15-down1-bf16", _sd15, "down", 1, torch.bfloat16, 210),
    ("sd15-up2-bf16", _sd15, "up", 2, torch.bfloat16, 220),
    ("sd21-down1-f16", _sd21, "down", 1, torch.float16, 310),
    ("sd21-down2-f16", _sd21, "down", 2, torch.float16, 320),
    ("sdxl-down2-bf16", _sdxl, "down_prefix", 2, torch.bfloat16, 410),
]

# Measured on the MI355X (the [measured] lines, worst tensor of each case): ((output max-rel, output group-rel), (gradient
# max-rel, gradient group-rel)).  The bars are BAR_FACTOR x these.  For scale: one fp16 rounding is 4.9e-4 relative, bf16 3.9e-3.
MEASURED_VJP = {
    "sd15-down0-f16": ((9.67e-04, 9.90e-04), (1.01e-03, 7.26e-04)),
    "sd15-down1-f16": ((1.17e-03, 9.96e-04), (8.63e-04, 7.19e-04)),
    "sd15-down2-f16": ((1.26e-03, 8.37e-04), (8.67e-04, 7.23e-04)),
    "sd15-down3-f16": ((5.06e-04, 3.43e-04), (8.83e-04, 4.27e-04)),
    "sd15-mid-f16": ((9.90e-04, 5.79e-04), (8.38e-04, 5.21e-04)),
    "sd15-up0-f16": ((7.92e-04, 5.47e-04), (7.06e-04, 6.25e-04)),
    "sd15-up1-f16": ((9.83e-04, 8.96e-04), (9.33e-04, 8.87e-04)),
    "sd15-up2-f16": ((9.59e-04, 9.50e-04), (1.01e-03, 8.95e-04)),
    "sd15-up3-f16": ((1.34e-03, 1.12e-03), (1.07e-03, 1.01e-03)),
    "sd15-down1-bf16": ((9.02e-03, 6.72e-03), (6.58e-03, 5.38e-03)),
    "sd15-up2-bf16": ((8.20e-03, 7.62e-03), (7.37e-03, 7.14e-03)),
    "sd21-down1-f16": ((1.28e-03, 8.52e-04), (8.48e-04, 7.22e-04)),
    "sd21-down2-f16": ((1.12e-03, 8.10e-04), (9.12e-04, 7.25e-04)),
    "sdxl-down2-bf16": ((1.27e-02, 1.16e-02), (1.21e-02, 1.00e-02)),
}
# batch-3 no-grad forward: (output max-rel, output group-rel)
MEASURED_B3 = {
    "sd15-down0-f16": (1.12e-03, 1.03e-03),
    "sd15-down1-f16": (1.07e-03, 1.01e-03),
    "sd15-down2-f16": (1.01e-03, 8.05e-04),
    "sd15-down3-f16": (5.95e-04, 3.43e-04),
    "sd15-mid-f16": (7.80e-04, 5.47e-04),
    "sd15-up0-f16": (7.40e-04, 5.50e-04),
    "sd15-up1-f16": (1.01e-03, 9.40e-04),
    "sd15-up2-f16": (9.82e-04, 1.02e-03),
    "sd15-up3-f16": (1.15e-03, 1.19e-03),
}
BAR_FACTOR = 2.5


def bars(measured):
    return tuple(v * BAR_FACTOR for v in measured)


def _case(cid, cfg_fn, kind, idx, dtype, seed):
    case = build_case(kind, cfg_fn(), idx, dtype, 1, seed)
    case.key = cid
    return case


_CASES = {}


@pytest.fixture(autouse=True, scope="module")
def _release_cases():
    """The cached master modules and fp64 references (up to ~10 GB of host memory) go with this module."""
    yield
    _CASES.clear()
    _REF.clear()


def get_case(spec):
    cid = spec[0]
    if cid not in _CASES:
        _CASES.clear()                      # one case's modules at a time
        _REF.clear()
        _CASES[cid] = _case(*spec)
    return _CASES[cid]


@pytest.mark.parametrize("spec", VJP_CASES, ids=[c[0] for c in VJP_CASES])
def test_block_vjp_matches_fp64(spec):
    """Forward and input / skip gradients of one block, 16-bit product path vs fp64 CPU, non-trivial parameters."""
    case = get_case(spec)
    out, grad = MEASURED_VJP[spec[0]]
    res, kinds, forms = run_vjp(case, bars(out), bars(grad))
    assert_own_kernels(case, kinds, forms)
    check_all(f"block vjp {spec[0]}", res)
    print(f"[census] {spec[0]}: {sorted(kinds.items())} cat forms {forms}")


# Gradients of the size the guidance backward carries: the cotangents scaled by 2^-8 (exact in both 16-bit types), the
# gradients compared after scaling back — the same bars as at unit scale.  Measured: every tensor within 8 % of its unit-scale
# value (worst: sd15-mid dx 1.04e-3 against 8.4e-4), so nothing the kernels carry leaves fp16's normal range at this size.
@pytest.mark.parametrize("spec", [c for c in VJP_CASES if c[0].startswith("sd15") and c[4] == torch.float16],
                         ids=[c[0] for c in VJP_CASES if c[0].startswith("sd15") and c[4] == torch.float16])
def test_block_vjp_small_cotangents(spec):
    case = get_case(spec)
    out, grad = MEASURED_VJP[spec[0]]
    res, kinds, forms = run_vjp(case, bars(out), bars(grad), scale=2.0 ** -8)
    check_all(f"block vjp 2^-8 {spec[0]}", res)


# AttentionStore(capture="reference"): the self maps of <= 32 x 32 layers are materialised, so the folded blocks take the
# ops.layer_norm path inside the processor.
@pytest.mark.parametrize("spec", [VJP_CASES[2], VJP_CASES[7]], ids=[VJP_CASES[2][0], VJP_CASES[7][0]])
def test_block_vjp_reference_capture(spec):
    case = get_case(spec)
    out, grad = MEASURED_VJP[spec[0]]        # measured within 4 % of the loss-only capture
    res, kinds, forms = run_vjp(case, bars(out), bars(grad), capture="reference")
    assert kinds.get("self_attn_fwd", 0) == 0 or case.hw > 32, kinds
    check_all(f"block vjp capture=reference {spec[0]}", res)


# ------------------------------------------------------------------------------------------------ batch-3 no-grad forward
FWD_CASES = [c for c in VJP_CASES if c[0].startswith("sd15") and c[4] == torch.float16]


@pytest.mark.parametrize("spec", FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_block_joint_forward_batch3(spec):
    """The joint pass (batch 3, no autograd: streamed GEGLU, no gradient aliases), forward only."""
    cid, cfg_fn, kind, idx, dtype, seed = spec
    case = build_case(kind, cfg_fn(), idx, dtype, 3, seed + 5)
    case.key = cid + "-b3"
    outs_ref, _, _ = reference(case, grad=False)
    outs, _, _, kinds, forms = product(case, grad=False)
    rep, vals = [], {}
    for i, (o, r) in enumerate(zip(outs, outs_ref)):
        vals[f"out{i}"] = compare(f"out{i}", o, r, bars(MEASURED_B3[cid]), rep)
    assert_own_kernels(case, kinds, forms, grad=False)
    check_all(f"block joint forward b3 {cid}", {"report": rep, "vals": vals})
    _REF.pop((case.key, False), None)


# ------------------------------------------------------------------------------------------------ the whole UNet, reduced width
def test_reduced_width_unet_wiring_fp16():
    """The full SD-1.x topology at every level a multiple of 64 wide (64, 64, 128, 128), 32 x 32 latents, the same non-trivial
    parameters, fp16, through UNet2DConditionModel.forward: the batched time projections (_time_projections, conv1's bias on
    them), conv_in / conv_out on the thin kernels and conv_norm_out's handoff.  Noise prediction, latent gradient and the
    aggregated 16 x 16 cross map vs the fp64 CPU UNet."""
    from guided_attention_amd import ops
    from guided_attention_amd.pipeline_guided_attention import install_kernels
    from guided_attention_amd.unet import UNet2DConditionModel, UNetConfig
    from guided_attention_amd.utils import ptp_utils
    from oracle import attention as oattn
    from oracle.pipeline import install_processors
    T = torch.float16
    cfg = UNetConfig(sample_size=32, block_out_channels=(64, 64, 128, 128), attention_head_dim=2, cross_attention_dim=64)
    unet = nontrivial_init_(UNet2DConditionModel(cfg), 500, T)
    g = torch.Generator().manual_seed(501)
    lat = rounded(torch.randn(1, 4, 32, 32, generator=g, dtype=torch.float64), T)
    ctx = rounded(torch.randn(1, 77, 64, generator=g, dtype=torch.float64), T)
    cot = rounded(torch.randn(1, 4, 32, 32, generator=g, dtype=torch.float64), T)
    gA = rounded(1e-2 * torch.randn(16, 16, 77, generator=g, dtype=torch.float64), T)
    # fp64 reference
    ref = copy.deepcopy(unet).double()
    store = oattn.OracleStore()
    install_processors(ref, store)
    x = lat.clone().requires_grad_(True)
    y_ref = ref(x, 981, encoder_hidden_states=ctx).sample
    A_ref = oattn.aggregate(store.attention_store, 16, ("up", "down", "mid"), True)
    (g_ref,) = torch.autograd.grad((y_ref * cot).sum() + (A_ref * gA).sum(), [x])
    # product
    gpu = unet.to("cuda", T)
    install_kernels(gpu)
    ctrl = ptp_utils.AttentionStore()
    ptp_utils.register_attention_control(SimpleNamespace(unet=gpu), ctrl)
    with ops.census_scope() as cs:
        xg = lat.to("cuda", T).requires_grad_(True)
        y = gpu(xg, 981, encoder_hidden_states=ctx.to("cuda", T)).sample
        A = ptp_utils.aggregate_attention(ctrl, 16, ("up", "down", "mid"), True, 0)
        (gg,) = torch.autograd.grad((y.float() * cot.to("cuda", T).float()).sum() + (A.float() * gA.cuda().float()).sum(), [xg])
        torch.cuda.synchronize()
    kinds = {}
    for k, n in cs.launches.items():
        kinds[k[0]] = kinds.get(k[0], 0) + n
    assert kinds.get("conv3x3", 0) > 0 and kinds.get("linear", 0) > 0, kinds
    assert sum(n for k, n in kinds.items() if k.startswith("conv3x3_thin")) == 4, kinds   # conv_in, conv_out, both backwards
    rep = []
    # measured on the MI355X: noise max-rel 1.59e-3 group-rel 1.84e-3, latent gradient 2.24e-3 / 2.31e-3, 16 x 16 map 2.05e-3
    vals = {"noise": compare("noise", y.detach().double().cpu(), y_ref.detach(), bars((1.59e-3, 1.84e-3)), rep, groups=4),
            "dlatent": compare("dlatent", gg.double().cpu(), g_ref, bars((2.24e-3, 2.31e-3)), rep, groups=4)}
    eA = max_rel(A.detach().double().cpu(), A_ref.detach())
    rep.append(f"map16 max-rel {eA:.2e}")
    vals["map16"] = (eA, 0.0, bars((2.05e-3, 1.0)))
    # noise and latent gradient have 4 channels: their slab metric runs over one channel at a time
    check_all("reduced-width unet fp16", {"report": rep, "vals": vals})


# ------------------------------------------------------------------------------------------------ stale producer statistics
def _ref_gn(x, cb, gamma, beta, eps, act=True):
    x = x.double().cpu()
    if cb is not None:
        x = x + cb.double().cpu()[:, :, None, None]
    y = torch.nn.functional.group_norm(x, GROUPS, gamma.double().cpu(), beta.double().cpu(), eps)
    return torch.nn.functional.silu(y) if act else y


def _produce(producer, g):
    """-> (tensor carrying producer statistics, channel bias or None, a callable that rebuilds the tensor's fp64 value)."""
    from guided_attention_amd import ops
    from guided_attention_amd.pipeline_guided_attention import install_kernels
    from guided_attention_amd.unet import Transformer2DModel
    T = torch.float16
    cl = torch.channels_last

    def rnd(*shape, s=1.0, o=0.0):
        return (torch.randn(*shape, generator=g) * s + o).to("cuda", T)

    if producer == "conv":      # conv1 of a 64 x 64 ResnetBlock2D: epilogue statistics of its result + the time term
        x = rnd(1, 320, 64, 64).contiguous(memory_format=cl)
        w = rnd(320, 320, 3, 3, s=(3.0 / 2880) ** 0.5)
        cb = rnd(1, 320, s=0.5)
        y = ops.conv3x3(x, w, None, None, 1, gn_for=(GROUPS, cb))
        return y, cb
    if producer in ("cat_partials", "cat_done"):
        hw, c1, c2 = (64, 640, 320) if producer == "cat_partials" else (16, 1280, 640)
        a = rnd(1, c1, hw, hw, o=0.5).contiguous(memory_format=cl)
        b = rnd(1, c2, hw, hw, s=1.5).contiguous(memory_format=cl)
        gamma, beta = rnd(c1 + c2, s=0.3, o=1.0), rnd(c1 + c2, s=0.2)
        y = ops.cat_channels(a, b, gn_for=GROUPS, norm=(gamma, beta, 1e-5, True))
        return y, None, (gamma, beta)
    # proj_out's epilogue, re-attached by Transformer2DModel.forward to the NCHW view (a DownBlock's first attention)
    tr = Transformer2DModel(8, 40, 320, 768, GROUPS, False)
    nontrivial_init_(tr, 77, T)
    tr.feeds_norm = True
    tr = tr.to("cuda", T)
    install_kernels(tr)
    with torch.no_grad():
        y = tr(rnd(1, 320, 64, 64).contiguous(memory_format=cl), rnd(1, 77, 768))
    return y, None


# measured on the MI355X: 2.3e-4 ... 4.2e-4 over the fourteen stale / fresh cases (one fp16 rounding of the norm's output);
# without the version check the stale partial sums gave errors of 8.5e-2 ... 5.0e-1, and the "done" cases handed out the stale
# output without a launch
STALE_BAR = 1.1e-3
STALE = [("conv", "mul"), ("conv", "add"), ("conv", "chan_bias"), ("cat_partials", "mul"), ("cat_partials", "add"),
         ("cat_done", "mul"), ("cat_done", "add"), ("cat_done", "gamma"), ("proj_out", "mul"), ("proj_out", "add")]


@pytest.mark.parametrize("producer,mutation", STALE, ids=[f"{p}-{m}" for p, m in STALE])
def test_group_norm_ignores_stale_producer_statistics(producer, mutation):
    """A tensor modified in place (or its channel bias, or the norm's gamma for the "done" form) between the producer that
    attached the GroupNorm's statistics / output and the norm: the norm must equal fp64 of what it is handed now, from its own
    statistics launch.  Without a mutation the handed data is used (the control: the producer did attach it)."""
    from guided_attention_amd import ops
    g = torch.Generator().manual_seed(600 + STALE.index((producer, mutation)))
    made = _produce(producer, g)
    y, cb = made[0], made[1]
    C = y.shape[1]
    gamma, beta = made[2] if len(made) > 2 else ((torch.randn(C, generator=g) * 0.3 + 1).to("cuda", y.dtype),
                                                  (torch.randn(C, generator=g) * 0.2).to("cuda", y.dtype))
    assert getattr(y, "_ga_gn", None) is not None, f"{producer}: no statistics attached (shape not served?)"
    done = "done" in y._ga_gn
    # per-channel factors / offsets: a uniform one would leave every group's normalised values unchanged
    ramp = torch.linspace(0.0, 1.0, C, device=y.device, dtype=y.dtype)[torch.randperm(C, generator=g)].view(1, C, 1, 1)
    with torch.no_grad():
        if mutation == "mul":
            y.mul_(0.5 + ramp)
        elif mutation == "add":
            y.add_(2.0 * ramp - 1.0)
        elif mutation == "chan_bias":
            cb.add_(0.5)
        else:
            gamma.mul_(0.5)
    with ops.census_scope() as cs:
        z = ops.group_norm_act(y, gamma, beta, GROUPS, 1e-5, True, cb)
        torch.cuda.synchronize()
    ref = _ref_gn(y, cb, gamma, beta, 1e-5)
    err = max_rel(z.double().cpu(), ref)
    print(f"[measured] stale statistics {producer} {mutation}: max-rel {err:.2e}")
    assert err < STALE_BAR, (producer, mutation, err)
    # the norm ran its own statistics: group_norm_fwd, no group_norm_apply on handed partials
    assert cs.launches and {k[0] for k in cs.launches} == {"group_norm_fwd"}, cs.launches


@pytest.mark.parametrize("producer", ["conv", "cat_partials", "cat_done", "proj_out"])
def test_group_norm_uses_fresh_producer_statistics(producer):
    """The control of the stale test: untouched, the producer's statistics (or norm output) are taken."""
    from guided_attention_amd import ops
    g = torch.Generator().manual_seed(3)
    made = _produce(producer, g)
    y, cb = made[0], made[1]
    C = y.shape[1]
    gamma, beta = made[2] if len(made) > 2 else ((torch.randn(C, generator=g) * 0.3 + 1).to("cuda", y.dtype),
                                                  (torch.randn(C, generator=g) * 0.2).to("cuda", y.dtype))
    done = "done" in y._ga_gn
    with ops.census_scope() as cs:
        z = ops.group_norm_act(y, gamma, beta, GROUPS, 1e-5, True, cb)
        torch.cuda.synchronize()
    err = max_rel(z.double().cpu(), _ref_gn(y, cb, gamma, beta, 1e-5))
    print(f"[measured] fresh statistics {producer}: max-rel {err:.2e}")
    assert err < STALE_BAR, (producer, err)
    kinds = {k[0] for k in cs.launches}
    assert kinds == (set() if done else {"group_norm_apply"}), cs.launches
