"""Python-side operators over the C ABI of libga_hip.so: thin argument marshalling plus the
`torch.autograd.Function` glue that puts the HIP forward/backward kernels into the autograd graph
the pipeline differentiates (reference: pipeline_guided_attention.py:466 autograd.grad(loss, latents)).
"""
import ctypes
import weakref
from collections import OrderedDict, namedtuple

import torch

from . import _lib
from ._lib import GaError, check, dtype_code, load, require_cuda, stream_ptr


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


# Optional launch census (bench.py): which shapes each capture kernel was launched with, and how often.
# Per-launch HIP events are useless while the host is the bottleneck (the event pair brackets host gaps),
# so bench.py replays each recorded shape back-to-back between two events instead (replay_launch_us).
_CENSUS = None


def start_census():
    global _CENSUS
    _CENSUS = {}


def stop_census():
    global _CENSUS
    rec, _CENSUS = _CENSUS, None
    return rec or {}


def _count(key):
    if _CENSUS is not None:
        _CENSUS[key] = _CENSUS.get(key, 0) + 1


class census_scope:
    """Collect the launches made inside the block into `.launches` (used while a hipGraph is captured, so that
    each replay can be accounted with `add_census`)."""

    def __enter__(self):
        global _CENSUS
        self._outer, _CENSUS = _CENSUS, {}
        return self

    def __exit__(self, *exc):
        global _CENSUS
        self.launches, _CENSUS = _CENSUS, self._outer


def add_census(launches):
    if _CENSUS is not None:
        for key, n in launches.items():
            _CENSUS[key] = _CENSUS.get(key, 0) + n


class no_gc:
    """No automatic garbage collection inside the block (collect once on entry): a cycle collection that runs while a stream is
    capturing may destroy an older hipGraph / stream / event, which aborts the process — every capture of this package sits
    inside one."""

    def __enter__(self):
        import gc
        self.was = gc.isenabled()
        gc.collect()
        gc.disable()

    def __exit__(self, *exc):
        if self.was:
            import gc
            gc.enable()


_KEEP = None   # while a hipGraph is being captured: every cached tensor a captured launch reads by raw pointer


class keepalive_scope:
    """Collect into `.tensors` every derived weight tensor (folded LayerNorm weights, transposes, convolution packs) handed
    out inside the block.  A GraphRunner captures inside one and keeps the list: its graphs read those tensors by raw pointer,
    so they must live exactly as long as the runner does, whatever the caches that made them evict later."""

    def __enter__(self):
        global _KEEP
        self._outer, _KEEP = _KEEP, []
        return self

    def __exit__(self, *exc):
        global _KEEP
        self.tensors, _KEEP = _KEEP, self._outer


def keep_alive(*tensors):
    if _KEEP is not None:
        _KEEP.extend(t for t in tensors if t is not None)
    return tensors[0] if len(tensors) == 1 else tensors


_side_streams = {}


def side_stream(device=None):
    """ONE side stream per device for warm-up runs, captures and micro-replays: the split-K scratch is kept per (device,
    stream) (linear_workspace), so every fresh torch.cuda.Stream() would cost another 256 MB of slabs."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    s = _side_streams.get(idx)
    if s is None:
        s = _side_streams[idx] = torch.cuda.Stream(device=idx)
    return s


def replay_launch_us(key, iters=100):
    """Average duration (us) of one launch of a recorded kernel shape, inputs resident in HBM: `iters` launches
    captured into one hipGraph (no host in the loop: a Python-driven loop is launch-bound at ~10 us per call and
    hides the kernel time), replayed between two HIP events on the launch stream.  For the self-attention and
    GroupNorm backward the figure covers the launches of one backward call (2 resp. up to 3 kernels)."""
    kind, B, H, N, Kt, D, flag, dt = key
    dtype = {"torch.float16": torch.float16, "torch.bfloat16": torch.bfloat16, "torch.float32": torch.float32}[dt]
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = load()
    fn = None
    if kind == "conv3x3":          # key = (kind, B, Cin, H*W, stride, Cout, epilogue?, dtype); the UNet's maps are square
        cin, hw, stride, cout = H, N, Kt, D
        side_len = int(round(hw ** 0.5))
        x = torch.randn(B, cin, side_len, hw // side_len, device=dev, dtype=dtype).contiguous(memory_format=torch.channels_last)
        # In the pipeline a convolution's weights are cold (1.7 GB of UNet weights cycle through a 256 MB Infinity Cache
        # between two uses) while its input was just written.  A back-to-back replay on ONE weight tensor would time an
        # L2-resident weight stream the product never sees: rotate over enough copies to exceed the Infinity Cache.
        n_copies = max(1, min(24, -(-320 * 2 ** 20 // (9 * cout * cin * 2))))
        wps = [torch.randn(9, cout, cin, device=dev, dtype=dtype) * (9 * cin) ** -0.5 for _ in range(n_copies)]
        turn = [0]
        ho, wo = (side_len - 1) // stride + 1, (hw // side_len - 1) // stride + 1
        bias = torch.randn(cout, device=dev, dtype=dtype) if flag else None
        res = (torch.randn(B, cout, ho, wo, device=dev, dtype=dtype).contiguous(memory_format=torch.channels_last)
               if flag else None)
        bm, bn, splits, _ = conv3x3_plan(B, side_len, hw // side_len, cin, cout, stride)
        y = torch.empty(B, cout, ho, wo, device=dev, dtype=dtype).contiguous(memory_format=torch.channels_last)
        code = dtype_code(x)

        def fn():
            wp = wps[turn[0] % n_copies]
            turn[0] += 1
            ws, tickets = splitk_workspace(dev, B * ho * wo, cout, bm, bn, splits)   # the scratch of the stream fn runs on
            check(lib.ga_conv3x3_nhwc(_ptr(x), _ptr(wp), _ptr(y), _ptr(ws), _ptr(tickets), _ptr(bias), _ptr(res), B, side_len,
                                      hw // side_len, cin, cout, stride, bm, bn, splits, code, stream_ptr()), "replay conv")
    elif kind in ("conv3x3_thin_in", "conv3x3_thin_out"):   # key = (kind, B, Cin, H*W, 1, Cout, bias?, dtype)
        cin, hw, cout = H, N, D
        side_len = int(round(hw ** 0.5))
        w = torch.randn(cout, cin, 3, 3, device=dev, dtype=dtype) * (9 * cin) ** -0.5
        wp = conv3x3_thin_packed_weights(w, False)
        bias = torch.randn(cout, device=dev, dtype=dtype) if flag else None
        x = torch.randn(B, cin, side_len, hw // side_len, device=dev, dtype=dtype)
        if cin != 4:
            x = x.contiguous(memory_format=torch.channels_last)

        def fn():
            conv3x3_thin(x, wp, cout, bias)
    elif kind in ("geglu_fwd", "geglu_bwd", "bias_residual_add", "add_layer_norm_fwd", "add_layer_norm_bwd"):
        rows, C = B, D
        code = dtype_code(torch.empty(0, dtype=dtype))
        t = lambda *shape: torch.randn(*shape, device=dev, dtype=dtype)  # noqa: E731
        if kind.startswith("geglu"):
            x, y, dy, dx = t(rows, 2 * C), t(rows, C), t(rows, C), t(rows, 2 * C)
            if kind == "geglu_fwd":
                def fn():
                    check(lib.ga_geglu_fwd(_ptr(x), _ptr(y), rows, C, code, stream_ptr()), "replay geglu fwd")
            else:
                def fn():
                    check(lib.ga_geglu_bwd(_ptr(x), _ptr(dy), _ptr(dx), rows, C, code, stream_ptr()), "replay geglu bwd")
        elif kind == "bias_residual_add":
            y, r, o, bias = t(rows, C), t(rows, C), t(rows, C), (t(C) if flag else None)

            def fn():
                check(lib.ga_bias_residual_add(_ptr(y), _ptr(bias), _ptr(r), _ptr(o), rows, C, code, stream_ptr()),
                      "replay bias residual")
        else:
            a, x, w, b_ = t(rows, C), t(rows, C), t(C), t(C)
            xn, y, dy, dx = t(rows, C), t(rows, C), t(rows, C), t(rows, C)
            stats = torch.empty(rows, 2, device=dev, dtype=torch.float32)
            check(lib.ga_add_layer_norm_fwd(_ptr(a), _ptr(x), _ptr(w), _ptr(b_), _ptr(xn), _ptr(y), _ptr(stats), rows, C,
                                            1e-5, code, stream_ptr()), "replay ln")
            if kind == "add_layer_norm_fwd":
                a_arg = a if flag else None

                def fn():
                    check(lib.ga_add_layer_norm_fwd(_ptr(a_arg), _ptr(x), _ptr(w), _ptr(b_), _ptr(xn), _ptr(y), _ptr(stats),
                                                    rows, C, 1e-5, code, stream_ptr()), "replay ln fwd")
            else:
                g_arg = a if flag else None

                def fn():
                    check(lib.ga_add_layer_norm_bwd(_ptr(xn), _ptr(stats), _ptr(w), _ptr(dy), _ptr(g_arg), _ptr(dx), rows,
                                                    C, code, stream_ptr()), "replay ln bwd")
    elif kind == "linear":        # key = (kind, M, K, 0, geglu | 2 ln | 4 residual, N, bias?, dtype)
        M, K, flags, N = B, H, Kt, D
        x = torch.randn(M, K, device=dev, dtype=dtype)
        n_copies = max(2, min(64, -(-320 * 2 ** 20 // (N * K * 2))))       # cold weights, as for the convolutions
        ws = [torch.randn(N, K, device=dev, dtype=dtype) * K ** -0.5 for _ in range(n_copies)]
        bias = torch.randn(N, device=dev, dtype=dtype) if flag else None
        geglu_, ln_, res_ = bool(flags & 1), bool(flags & 2), bool(flags & 4)
        n_out = N // 2 if geglu_ else N
        res = torch.randn(M, n_out, device=dev, dtype=dtype) if res_ else None
        ln = None
        if ln_:
            ln = (torch.rand(M, 5, 2, device=dev) * K, torch.randn(N, device=dev), torch.randn(N, device=dev), 1e-5)
        turn = [0]

        def fn():
            turn[0] += 1
            linear_fused(x, ws[turn[0] % n_copies], bias, residual=res, geglu=geglu_, ln=ln)
    elif kind in ("aggregate_maps", "aggregate_loss_fwd", "smooth_loss_fwd", "smooth_loss_bwd"):
        # B = guided tokens (aggregate_maps: tensors), H = head-maps in all, N = pixels, Kt = tokens of the context
        npix, res = N, int(round(N ** 0.5))
        nt = B if kind != "aggregate_maps" else 3
        entries = [{"index": 2 + i, "kind": "BOX", "geom": (.1 + .05 * i, .3, .4, .55), "subprompt": f"s{i}"}
                   for i in range(nt)]
        plan = LossPlan(entries, {"inside_loss_scale": .2, "outside_loss_scale": .2, "shrink_factor": .15})
        heads_all = max(H, 1)
        per = D if D and heads_all % D == 0 else (8 if heads_all % 8 == 0 else heads_all)   # heads per stored tensor, as counted
        maps = [torch.softmax(torch.randn(per, npix, Kt, device=dev), -1).to(dtype) for _ in range(heads_all // per)]
        A = torch.softmax(torch.randn(npix, Kt, device=dev), -1)
        if kind == "aggregate_maps":
            def fn():
                aggregate_maps(maps)
        elif kind == "aggregate_loss_fwd":
            def fn():
                aggregate_loss_fwd(maps, res, 1, Kt - 1, plan)
        elif kind == "smooth_loss_fwd":
            def fn():
                smooth_loss_fwd(A, res, 1, Kt - 1, plan)
        else:
            def fn():
                smooth_loss_bwd(A, res, 1, Kt - 1, plan, None, dtype if flag else None, 1.0 / 40)
    elif kind in ("latent_axpy", "latent_axpby", "cfg_ddim_step", "cfg_ddim_step_pred", "cfg_ddim_step_eta",
                  "latent_sgd_momentum"):
        x, y, z = (torch.randn(N, device=dev, dtype=dtype) for _ in range(3))
        if kind == "latent_axpy":
            def fn():
                latent_axpy(x, y, 20.0, bool(flag))
        elif kind == "latent_sgd_momentum":
            vel = torch.zeros(N, device=dev, dtype=torch.float32)

            def fn():
                latent_sgd_momentum(x, y, vel, 4.0, 0.8, bool(flag))
        elif kind == "latent_axpby":
            def fn():
                latent_axpby(x, y, 0.9, 0.1)
        elif kind == "cfg_ddim_step_pred":   # D = GA_PRED_V or GA_PRED_SAMPLE, as counted
            name = {_lib.GA_PRED_V: "v_prediction", _lib.GA_PRED_SAMPLE: "sample"}[D]

            def fn():
                cfg_ddim_step(x, y, 7.5, z, 0.5, 0.6, bool(flag), name)
        elif kind == "cfg_ddim_step_eta":    # D = GA_PRED_*, as counted; eta = 0.5
            name = {code: name for name, code in _lib.PREDICTION_CODE.items()}[D]
            w = torch.randn(N, device=dev, dtype=dtype)

            def fn():
                cfg_ddim_step(x, y, 7.5, z, 0.5, 0.6, bool(flag), name, 0.5, w)
        else:
            def fn():
                cfg_ddim_step(x, y, 7.5, z, 0.5, 0.6, bool(flag))
    elif kind.startswith("group_norm"):
        groups, HW, C = H, N, D
        side_len = int(round(HW ** 0.5))
        x = torch.randn(B, C, side_len, HW // side_len, device=dev, dtype=dtype).contiguous(memory_format=torch.channels_last)
        w, b_ = torch.ones(C, device=dev, dtype=dtype), torch.zeros(C, device=dev, dtype=dtype)
        y, dy = torch.empty_like(x), torch.randn_like(x)
        stats = torch.empty(B, groups, 2, device=dev, dtype=torch.float32)
        ws = torch.empty(B * 257 * groups * 2, device=dev, dtype=torch.float32)
        code = dtype_code(x)
        check(lib.ga_group_norm_fwd(_ptr(x), None, _ptr(w), _ptr(b_), _ptr(y), _ptr(stats), _ptr(ws), B, HW, C, groups,
                                    1e-5, int(flag), code, stream_ptr()), "replay gn")
        if kind == "group_norm_fwd":
            def fn():
                check(lib.ga_group_norm_fwd(_ptr(x), None, _ptr(w), _ptr(b_), _ptr(y), _ptr(stats), _ptr(ws), B, HW, C,
                                            groups, 1e-5, int(flag), code, stream_ptr()), "replay gn fwd")
        elif kind == "group_norm_apply":   # Kt = partial blocks per image (the producing convolution's epilogue left them)
            partials = torch.rand(B, Kt, groups, 2, device=dev) * (HW * C // groups) / Kt

            def fn():
                check(lib.ga_group_norm_apply(_ptr(x), None, _ptr(w), _ptr(b_), _ptr(y), _ptr(stats), _ptr(partials), Kt, B, HW,
                                              C, groups, 1e-5, int(flag), code, stream_ptr()), "replay gn apply")
        else:
            def fn():
                check(lib.ga_group_norm_bwd(_ptr(x), None, _ptr(dy), _ptr(w), _ptr(b_), _ptr(stats), None, _ptr(y), _ptr(ws), B,
                                            HW, C, groups, int(flag), code, stream_ptr()), "replay gn bwd")
    elif kind in ("attn_capture_fwd", "attn_capture_bwd", "self_attn_fwd", "self_attn_bwd", "self_attn_bwd_dp",
                  "self_attn_capture_fwd"):
        q = torch.randn(B, N, H * D, device=dev, dtype=dtype)
        k = torch.randn(B, Kt, H * D, device=dev, dtype=dtype)
        v = torch.randn(B, Kt, H * D, device=dev, dtype=dtype)
        out = torch.empty_like(q)
        code, scale = dtype_code(q), D ** -0.5
    if kind == "attn_capture_fwd":
        probs = torch.empty(B * H, N, Kt, device=dev, dtype=dtype) if flag else None

        def fn():
            check(lib.ga_attn_capture_fwd(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(probs), B, H, N, Kt, D, scale,
                                          code, stream_ptr()), "replay fwd")
    elif kind == "attn_capture_bwd":
        d_o = torch.randn_like(q)
        dp = torch.randn(N, Kt, device=dev, dtype=dtype) * 1e-3 if flag else None

        def fn():
            check(lib.ga_attn_capture_bwd(_ptr(q), _ptr(k), _ptr(v), _ptr(d_o), _ptr(dp), 0, Kt, _ptr(out), None, None,
                                          B, H, N, Kt, D, scale, code, stream_ptr()), "replay bwd")
    elif kind in ("self_attn_fwd", "self_attn_bwd", "self_attn_bwd_dp"):
        lse = torch.empty(B * H, N, device=dev, dtype=torch.float32)
        check(lib.ga_self_attn_fwd(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(lse), B, H, N, D, 0, scale, code,
                                   stream_ptr()), "replay sa")
        if kind == "self_attn_fwd":
            lse_arg = lse if flag else None

            def fn():
                check(lib.ga_self_attn_fwd(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(lse_arg), B, H, N, D, 0, scale,
                                           code, stream_ptr()), "replay sa fwd")
        elif kind == "self_attn_bwd_dp":    # one (N, N) cotangent shared by the head-maps, as AggregateMaps.backward sends it
            d_o, delta, rowdot = (torch.randn_like(q) if flag else None), torch.empty_like(lse), torch.empty_like(lse)
            d_p = torch.randn(N, N, device=dev, dtype=dtype) * 1e-3
            dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)

            def fn():
                check(lib.ga_self_attn_bwd_dp(_ptr(q), _ptr(k), _ptr(v), _ptr(out if flag else None), _ptr(d_o), _ptr(d_p), 0,
                                              _ptr(lse), _ptr(delta), _ptr(rowdot), _ptr(dq), _ptr(dk), _ptr(dv), B, H, N, D, 0,
                                              scale, code, stream_ptr()), "replay sa bwd dp")
        else:
            d_o, delta = torch.randn_like(q), torch.empty_like(lse)
            dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)

            def fn():
                check(lib.ga_self_attn_bwd(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(d_o), _ptr(lse), _ptr(delta),
                                           _ptr(dq), _ptr(dk), _ptr(dv), B, H, N, D, 0, scale, code, stream_ptr()),
                      "replay sa bwd")
    elif kind == "self_attn_capture_fwd":
        lse = torch.empty(B * H, N, device=dev, dtype=torch.float32)
        probs = torch.empty(B * H, N, N, device=dev, dtype=dtype)

        def fn():
            check(lib.ga_self_attn_capture_fwd(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(lse), _ptr(probs), B, H, N, D, 0,
                                               scale, code, stream_ptr()), "replay sa capture fwd")
    if fn is None:
        raise GaError(f"no replay recipe for kernel kind {kind!r}")
    side = side_stream(dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with no_gc(), torch.cuda.graph(graph, stream=side):
            for _ in range(iters):
                fn()
        graph.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        side.synchronize()
        e0.record(side)
        graph.replay()
        e1.record(side)
        side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    return e0.elapsed_time(e1) * 1e3 / iters


# --------------------------------------------------------------------------------------- K1
# The form of a capture call, as data.  kind "plain": softmax(scale q k^T) v.  "biased" (paint-with-words, solo): scores +
# bias[n][k] * coef[0], bias (N, Kt), coef f32 [1] on the device.  "grouped" (the same per image of a batched pass, batch row b
# belongs to image b % G): scores + bias[b % G][n][k] * (maximum of packed[b % G]) * coef[b % G]; bias (G, N, Kt) or one shared
# (N, Kt), packed int64 [G] from attn_scores_max_grouped, coef = the multipliers, f32 [G].
CaptureForm = namedtuple("CaptureForm", "kind bias coef packed")
_PLAIN = CaptureForm("plain", None, None, None)


def _group_bias(bias, groups, N, Kt, dtype):
    """-> (contiguous masks in `dtype`, group stride in elements): (N, Kt), (1, N, Kt) or a stride-0 expansion = one mask
    shared by every group (stride 0), (G, N, Kt) = one per group."""
    if bias.dim() == 2:
        bias = bias.unsqueeze(0)
    if bias.dim() != 3 or tuple(bias.shape[1:]) != (N, Kt) or bias.shape[0] not in (1, groups):
        raise GaError(f"bias must be (N, Kt) or (G, N, Kt) with G = {groups}, N = {N}, Kt = {Kt}; got {tuple(bias.shape)}")
    if bias.shape[0] == 1 or bias.stride(0) == 0:
        return bias[0].to(dtype).contiguous(), 0
    return bias.to(dtype).contiguous(), N * Kt


def _check_groups(B, packed, mult):
    G = mult.numel()
    if mult.dtype != torch.float32 or packed.dtype != torch.int64 or packed.numel() != G:
        raise GaError("packed must be int64 [G] and mult float32 [G], both on the device")
    if not 1 <= G <= _lib.GA_MAX_IMAGES or B % G:
        raise GaError(f"{G} groups for {B} batch rows: 1 ... {_lib.GA_MAX_IMAGES} groups, B a multiple of G")
    return G


def _form_bias(form, B, N, Kt, dtype):
    """The checks a form makes before any device work -> (its mask(s) as the kernels read them, group stride, G)."""
    if form.kind == "plain":
        return None, 0, 1
    if form.kind == "grouped":
        G = _check_groups(B, form.packed, form.coef)
        return _group_bias(form.bias, G, N, Kt, dtype) + (G,)
    if tuple(form.bias.shape) != (N, Kt) or form.coef.dtype != torch.float32:
        raise GaError(f"bias must be (N, Kt) = {(N, Kt)} and coef a float32 device scalar")
    return form.bias.to(dtype).contiguous(), 0, 1


def _d_probs_arg(d_probs, q, images=True):
    """d_probs as a capture backward passes it on, never materialising a broadcast -> (tensor or None, its _image_broadcasts
    entry or None, head-map stride, row stride).  A per-image view of a batched loss (`images`: the entry takes an image stride)
    is found in the _image_broadcasts table and counted as consumed here; anything else is cast to q's dtype and made contiguous
    unless it is one stride-0 map."""
    if d_probs is None:
        return None, None, 0, 0
    per_image = _image_broadcasts.get(d_probs.data_ptr()) if images and d_probs.stride(0) == 0 else None
    if per_image is not None and per_image[0] == q.shape[0] and d_probs.dtype == q.dtype and d_probs.stride(2) == 1:
        per_image[3] -= 1   # one [N][Kt] map per image over that image's head-maps (_FusedLoss.backward): no copy
        return d_probs, per_image, 0, d_probs.stride(1)
    if d_probs.dtype != q.dtype:
        d_probs = d_probs.to(q.dtype)
    if d_probs.stride(2) != 1 or (d_probs.stride(0) != 0 and not d_probs.is_contiguous()):
        d_probs = d_probs.contiguous()
    return d_probs, None, d_probs.stride(0), d_probs.stride(1)


def _capture_fwd(q, k, v, heads, scale, want_probs, form=_PLAIN):
    """The one forward launch: q (B,N,C), k/v (B,Kt,C) projections -> (o (B,N,C), probs (B*heads,N,Kt) or None).  Only the
    plain form is in the launch census (replay_launch_us has a recipe for it alone)."""
    require_cuda(q, k, v, *form[1:])
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    B, N, C = q.shape
    Kt, D = k.shape[1], C // heads
    bias, stride, G = _form_bias(form, B, N, Kt, q.dtype)
    o = torch.empty_like(q)
    probs = torch.empty((B * heads, N, Kt), dtype=q.dtype, device=q.device) if want_probs else None
    lib, io = load(), (_ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(probs))
    dims = (B, heads, N, Kt, D, float(scale), dtype_code(q))
    if form.kind == "plain":
        _count(("attn_capture_fwd", B, heads, N, Kt, D, bool(want_probs), str(q.dtype)))
        check(lib.ga_attn_capture_fwd(*io, *dims, stream_ptr()), "ga_attn_capture_fwd")
    elif form.kind == "biased":
        check(lib.ga_attn_capture_fwd_biased(*io, _ptr(bias), _ptr(form.coef), *dims, stream_ptr()), "ga_attn_capture_fwd_biased")
    else:
        check(lib.ga_attn_capture_fwd_biased_grouped(*io, _ptr(bias), stride, _ptr(form.packed), _ptr(form.coef), *dims, G,
                                                     stream_ptr()), "ga_attn_capture_fwd_biased_grouped")
    return o, probs


def _capture_bwd(q, k, v, d_o, d_probs, heads, scale, form=_PLAIN):
    """The one backward launch -> (dq (B,N,C) WITHOUT the gradient through a form's maximum, d loss / d coef (f32 [G]; None for
    the plain form)).  d_probs: None, a dense (B*heads,N,Kt) tensor, an expanded (stride-0 over the head-map axis) view of one
    (N,Kt) map, or — the plain and grouped forms, whose entries take an image stride — a per-image view of the batched loss
    (found in the _image_broadcasts table).  It goes to the kernel as strides, never materialised."""
    require_cuda(q, k, v, d_o, d_probs, *form[1:])
    B, N, C = q.shape
    Kt, D = k.shape[1], C // heads
    bias, stride, G = _form_bias(form, B, N, Kt, q.dtype)
    d_o = d_o.contiguous()
    d_probs, per_image, sh, sn = _d_probs_arg(d_probs, q, images=form.kind != "biased")
    si = per_image[1] if per_image is not None else sh * heads
    dq = torch.empty_like(q)
    gsum = torch.zeros(G, dtype=torch.float32, device=q.device) if form.kind != "plain" else None
    lib, io = load(), (_ptr(q), _ptr(k), _ptr(v), _ptr(d_o), _ptr(d_probs))
    dims = (B, heads, N, Kt, D, float(scale), dtype_code(q))
    if form.kind == "plain":
        _count(("attn_capture_bwd", B, heads, N, Kt, D, d_probs is not None, str(q.dtype)))
        check(lib.ga_attn_capture_bwd_strided(*io, si, sh, sn, _ptr(dq), None, None, *dims, stream_ptr()),
              "ga_attn_capture_bwd_strided")
    elif form.kind == "biased":
        check(lib.ga_attn_capture_bwd_biased(*io, sh, sn, _ptr(dq), _ptr(bias), _ptr(form.coef), _ptr(gsum), *dims,
                                             stream_ptr()), "ga_attn_capture_bwd_biased")
    else:
        check(lib.ga_attn_capture_bwd_biased_grouped(*io, si, sh, sn, _ptr(dq), _ptr(bias), stride, _ptr(form.packed),
                                                     _ptr(form.coef), _ptr(gsum), *dims, G, stream_ptr()),
              "ga_attn_capture_bwd_biased_grouped")
    return dq, gsum


def attn_capture_fwd(q, k, v, heads, scale, want_probs):
    """q (B,N,C), k/v (B,Kt,C) projections -> (o (B,N,C), probs (B*heads,N,Kt) or None)."""
    return _capture_fwd(q, k, v, heads, scale, want_probs)


def attn_capture_bwd(q, k, v, d_o, d_probs, heads, scale):
    """-> dq (B,N,C); d_probs as _capture_bwd takes it."""
    return _capture_bwd(q, k, v, d_o, d_probs, heads, scale)[0]


# --------------------------------------------------------------------------------------- K1 + paint-with-words
def attn_scores_max_grouped(q, k, heads, scale, groups):
    """-> packed int64 [groups] on the device: batch row b belongs to group b % groups, and word g holds the maximum over
    group g's scaled scores and its flat index into the WHOLE call's [B*heads][N][Kt] (see unpack_scores_max)."""
    require_cuda(q, k)
    q, k = q.contiguous(), k.contiguous()
    B, N, C = q.shape
    Kt = k.shape[1]
    if not 1 <= groups <= _lib.GA_MAX_IMAGES or B % groups:
        raise GaError(f"{groups} groups for {B} batch rows: 1 ... {_lib.GA_MAX_IMAGES} groups, B a multiple of G")
    packed = torch.zeros(groups, dtype=torch.int64, device=q.device)
    check(load().ga_attn_scores_max_grouped(_ptr(q), _ptr(k), B, heads, N, Kt, C // heads, float(scale), dtype_code(q),
                                            groups, _ptr(packed), stream_ptr()), "ga_attn_scores_max_grouped")
    return packed


def attn_scores_max(q, k, heads, scale):
    """-> (max over every scaled score of the call, f32 [1]; its flat index into [B*heads][N][Kt], int64 [1]), both
    on the device (no synchronisation): the `attention_scores.max()` of utils/ptp_utils.py:134."""
    require_cuda(q, k)
    q, k = q.contiguous(), k.contiguous()
    B, N, C = q.shape
    Kt = k.shape[1]
    packed = torch.zeros(1, dtype=torch.int64, device=q.device)
    check(load().ga_attn_scores_max(_ptr(q), _ptr(k), B, heads, N, Kt, C // heads, float(scale), dtype_code(q),
                                    _ptr(packed), stream_ptr()), "ga_attn_scores_max")
    return unpack_scores_max(packed)


def unpack_scores_max(packed):
    """packed words of ga_attn_scores_max(_grouped) (int64 [G]) -> (values f32 [G], flat indices int64 [G]), on the device."""
    hi = (packed >> 32) & 0xFFFFFFFF
    bits = torch.where((hi & 0x80000000) == 0, (~hi) & 0xFFFFFFFF, hi ^ 0x80000000)   # undo the order-preserving map
    value = (bits - ((bits >> 31) << 32)).to(torch.int32).view(torch.float32)
    return value, packed & 0xFFFFFFFF


def attn_capture_fwd_biased(q, k, v, heads, scale, want_probs, bias, coef):
    """attn_capture_fwd with scores + bias[n][k] * coef[0] (bias (N, Kt) in q's dtype, coef f32 [1] on the device)."""
    return _capture_fwd(q, k, v, heads, scale, want_probs, CaptureForm("biased", bias, coef, None))


def attn_capture_bwd_biased(q, k, v, d_o, d_probs, heads, scale, bias, coef):
    """-> (dq, d loss / d coef (f32 [1])) for the biased scores (see ga_hip.h)."""
    return _capture_bwd(q, k, v, d_o, d_probs, heads, scale, CaptureForm("biased", bias, coef, None))


def attn_capture_fwd_biased_grouped(q, k, v, heads, scale, want_probs, bias, packed, mult):
    """attn_capture_fwd with scores + bias[b % G][n][k] * (maximum of packed[b % G]) * mult[b % G]: bias (G, N, Kt) or one
    shared (N, Kt), packed int64 [G] from attn_scores_max_grouped, mult f32 [G], all on the device."""
    return _capture_fwd(q, k, v, heads, scale, want_probs, CaptureForm("grouped", bias, mult, packed))


def attn_capture_bwd_biased_grouped(q, k, v, d_o, d_probs, heads, scale, bias, packed, mult):
    """-> (dq WITHOUT the gradient through the maximum, d loss / d coef per group (f32 [G]))."""
    return _capture_bwd(q, k, v, d_o, d_probs, heads, scale, CaptureForm("grouped", bias, mult, packed))


def attn_pww_max_grad(dq, k, packed, bias_grad, mult, heads, scale):
    """IN PLACE on dq (B, N, C): the gradient through each group's maximum, added at the position packed[g] names."""
    require_cuda(dq, k, packed, bias_grad, mult)
    if not (dq.is_contiguous() and k.is_contiguous()):
        raise GaError("attn_pww_max_grad works in place on contiguous tensors")
    B, N, C = dq.shape
    G = _check_groups(B, packed, mult)
    if bias_grad.dtype != torch.float32 or bias_grad.numel() != G:
        raise GaError("bias_grad must be float32 [G]")
    check(load().ga_attn_pww_max_grad(_ptr(dq), _ptr(k), _ptr(packed), _ptr(bias_grad), _ptr(mult), B, heads, N, k.shape[1],
                                      C // heads, float(scale), dtype_code(dq), G, stream_ptr()), "ga_attn_pww_max_grad")
    return dq


def _solo_max_grad(dq, k, arg, gsum, mult, heads, scale):
    """IN PLACE on dq: the gradient that reaches the scores through the solo form's `.max()`, (mult * sum dS * mask) at the
    maximum's flat index `arg`, in torch (mult * scale is formed on the host, in double)."""
    B, N, C = dq.shape
    Kt, D = k.shape[1], C // heads
    bh, rem = arg // (N * Kt), arg % (N * Kt)
    n, kk = rem // Kt, rem % Kt
    b, h = bh // heads, bh % heads
    krow = k.view(B * Kt * heads, D).index_select(0, (b * Kt + kk) * heads + h)           # (1, D)
    add = (krow.float() * (gsum * (mult * scale))).to(dq.dtype)
    dq.view(B * N * heads, D).index_add_(0, (b * N + n) * heads + h, add)


class _AttnCapture(torch.autograd.Function):
    """(q, k, v, heads, scale, want_probs, kind, bias, mult) -> (o, probs): softmax(scale q k^T [+ the form's bias]) v with the
    probabilities as a second, differentiable output (an empty placeholder when they are not wanted).  The biased forms take
    their maximum in a launch of their own in front of the forward and send its gradient on behind the backward; only q is
    differentiated."""

    @staticmethod
    def forward(ctx, q, k, v, heads, scale, want_probs, kind, bias, mult):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        form, arg = _PLAIN, None
        if kind == "biased":
            smax, arg = attn_scores_max(q, k, heads, scale)
            form, mult = CaptureForm(kind, bias, smax * float(mult), None), float(mult)
        elif kind == "grouped":
            form, mult = CaptureForm(kind, bias, mult, attn_scores_max_grouped(q, k, heads, scale, mult.numel())), None
        o, probs = _capture_fwd(q, k, v, heads, scale, want_probs, form)
        ctx.save_for_backward(q, k, v, arg, *form[1:])
        ctx.meta = (kind, heads, scale, mult)
        if probs is None:
            probs = q.new_empty(0)
            ctx.mark_non_differentiable(probs)
        return o, probs

    @staticmethod
    def backward(ctx, d_o, d_probs):
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            raise GaError("gradients w.r.t. the attention context (K/V) are not part of the guided-attention "
                          "path (only the latents are differentiated); freeze the UNet parameters")
        q, k, v, arg, *operands = ctx.saved_tensors
        kind, heads, scale, mult = ctx.meta
        form = CaptureForm(kind, *operands)
        if d_probs is not None and d_probs.numel() == 0:
            d_probs = None
        if d_o is None:
            d_o = torch.zeros_like(q)
        dq, gsum = _capture_bwd(q, k, v, d_o, d_probs, heads, scale, form)
        if kind == "biased":
            _solo_max_grad(dq, k, arg, gsum, mult, heads, scale)
        elif kind == "grouped":
            attn_pww_max_grad(dq, k, form.packed, gsum, form.coef, heads, scale)
        return (dq,) + (None,) * 8


class AttnCapture:
    """(q, k, v, heads, scale, want_probs) -> (o, probs): softmax(scale q k^T) v with the probabilities as a second,
    differentiable output."""

    @staticmethod
    def apply(q, k, v, heads, scale, want_probs):
        return _AttnCapture.apply(q, k, v, heads, scale, want_probs, "plain", None, None)


class AttnCapturePaintWithWords:
    """softmax(scale q k^T + mask * mult * max(scale q k^T)) v with the probabilities as a second output — the
    paint-with-words branch of the reference's get_attention_scores (utils/ptp_utils.py:113-138; mult =
    0.4 * log(1 + sigma_t)).  The maximum is taken over the whole call and carries a gradient, as in the reference."""

    @staticmethod
    def apply(q, k, v, heads, scale, want_probs, mask, mult):
        return _AttnCapture.apply(q, k, v, heads, scale, want_probs, "biased", mask, mult)


class AttnCapturePaintWithWordsImages:
    """AttnCapturePaintWithWords for the G = mult.numel() images of a batched pass: batch row b is image b % G's, and each
    image gets what its solo call computes — the maximum over ITS rows, its mask (bias (G, N, Kt), or one shared (N, Kt)), its
    multiplier (mult f32 [G] on the device; 0 = that image does not paint) and the gradient through its own maximum.  Four
    launches (maximum, forward ... backward, gradient through the maximum), every per-image value stays on the device."""

    @staticmethod
    def apply(q, k, v, heads, scale, want_probs, bias, mult):
        return _AttnCapture.apply(q, k, v, heads, scale, want_probs, "grouped", bias, mult)


# --------------------------------------------------------------------------------------- K2
def aggregate_maps(maps):
    """maps: list of (heads_i, npix, Kt) tensors of one dtype -> A (npix, Kt) f32."""
    require_cuda(*maps)
    maps = [m.contiguous() for m in maps]
    npix, Kt = maps[0].shape[1], maps[0].shape[2]
    n = len(maps)
    ptrs = (ctypes.c_void_p * n)(*[m.data_ptr() for m in maps])
    heads = (ctypes.c_int * n)(*[m.shape[0] for m in maps])
    A = torch.empty((npix, Kt), dtype=torch.float32, device=maps[0].device)
    _count(("aggregate_maps", n, sum(m.shape[0] for m in maps), npix, Kt, maps[0].shape[0], False, str(maps[0].dtype)))
    check(load().ga_aggregate_maps(ptrs, heads, n, npix, Kt, _ptr(A), dtype_code(maps[0]), stream_ptr()),
          "ga_aggregate_maps")
    return A


class AggregateMaps(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *maps):
        ctx.shapes = [m.shape for m in maps]
        ctx.dtype = maps[0].dtype
        return aggregate_maps(list(maps))

    @staticmethod
    def backward(ctx, dA):
        total = sum(s[0] for s in ctx.shapes)
        g = (dA * (1.0 / total)).to(ctx.dtype)
        # one (npix, Kt) map broadcast over every head-map: handed on as a stride-0 view
        return tuple(g.unsqueeze(0).expand(s) for s in ctx.shapes)


# --------------------------------------------------------------------------------------- K3+K4
class LossPlan:
    """Host-side descriptor of the guided tokens and hyper-parameters (what config.token_dict and
    shared_state.curHyperParams hold in the reference), marshalled once into the C structs."""

    # the hyper-parameters a plan reads (what its cache key must cover)
    HYPER_KEYS = ("strict", "inside_loss_scale", "outside_loss_scale", "bb_center_weight", "shrink_factor")

    def __init__(self, entries, hyper, smooth=True, sigma=0.5, kernel_size=3, sub_prompt_avg_within=False,
                 check_geometry=True):
        """entries: list of dict(index, kind 'BOX'|'COOR', geom, subprompt)."""
        self.entries = list(entries)
        self.check_geometry = check_geometry
        self._checked_res = set()
        self.shrink = float(hyper["shrink_factor"]) if "shrink_factor" in hyper else 0.0
        T = len(self.entries)
        self.T = T
        if T == 0:  # only custom (Python) losses are active: nothing for the fused kernel to do
            self.tokens, self.params, self.weights = None, None, []
            return
        counts = OrderedDict()
        for e in self.entries:
            counts[e["subprompt"]] = counts.get(e["subprompt"], 0) + 1
        self.weights = [1.0 / counts[e["subprompt"]] if sub_prompt_avg_within else 1.0 for e in self.entries]
        self.tokens = (_lib.ga_token_t * T)()
        for i, (e, w) in enumerate(zip(self.entries, self.weights)):
            tk = self.tokens[i]
            tk.token = int(e["index"])
            tk.kind = _lib.GA_TOK_BOX if e["kind"] == "BOX" else _lib.GA_TOK_COOR
            geom = list(e["geom"]) + [0.0] * (4 - len(e["geom"]))
            for j in range(4):
                tk.geom[j] = float(geom[j])
            tk.weight = w
        self.params = _lib.ga_loss_params_t()
        self.params.strict = 1 if hyper.get("strict", False) else 0
        self.params.inside_scale = hyper["inside_loss_scale"]
        self.params.outside_scale = hyper["outside_loss_scale"]
        self.params.center_weight = hyper.get("bb_center_weight", .05)
        self.params.sigma = sigma
        self.params.shrink = hyper["shrink_factor"]
        self.params.ksize = kernel_size
        self.params.smooth = 1 if smooth else 0


def _check_boxes(plan, res):
    """The reference divides by the number of pixel centres inside the (shrunk) box (helpers.py:249,266:
    `at_most = 1.0 / num_inside`): a box that contains none raises ZeroDivisionError there, and so it does here
    (host-side, once per (plan, res))."""
    if not plan.check_geometry or res in plan._checked_res:
        return
    for e in plan.entries:
        if e["kind"] != "BOX":
            continue
        x, y, w, h = (float(v) * float(res) for v in e["geom"])
        ox, oy = plan.shrink * w, plan.shrink * h
        n_in = sum(1 for ii in range(res) for jj in range(res)
                   if x + ox <= jj + 0.5 <= x + w - ox and y + oy <= ii + 0.5 <= y + h - oy)
        if n_in == 0:
            raise ZeroDivisionError("float division by zero")
    plan._checked_res.add(res)


def smooth_loss_fwd(A, res, first, last, plan):
    require_cuda(A)
    if plan.T == 0:
        raise GaError("no guided tokens")
    _check_boxes(plan, res)
    if A.dtype != torch.float32:
        raise GaError("aggregated maps must be float32")
    A = A.contiguous()
    Kt = A.shape[-1]
    terms = torch.empty((plan.T, _lib.GA_TERMS), dtype=torch.float32, device=A.device)
    loss = torch.empty((1,), dtype=torch.float32, device=A.device)
    _count(("smooth_loss_fwd", plan.T, 0, res * res, Kt, 0, False, "torch.float32"))
    check(load().ga_smooth_loss_fwd(_ptr(A), res, Kt, first, last, plan.tokens, plan.T, ctypes.byref(plan.params),
                                    _ptr(terms), _ptr(loss), stream_ptr()), "ga_smooth_loss_fwd")
    return terms, loss


class SmoothLoss(torch.autograd.Function):
    """A (res*res, Kt) f32 -> (terms (T,8), loss (1,)).  Only `loss` is differentiable."""

    @staticmethod
    def forward(ctx, A, res, first, last, plan):
        terms, loss = smooth_loss_fwd(A, res, first, last, plan)
        ctx.save_for_backward(A)
        ctx.args = (res, first, last, plan)
        ctx.mark_non_differentiable(terms)
        return terms, loss

    @staticmethod
    def backward(ctx, _dterms, dloss):
        (A,) = ctx.saved_tensors
        res, first, last, plan = ctx.args
        dA, _ = smooth_loss_bwd(A, res, first, last, plan, dloss)
        return dA, None, None, None, None


# ------------------------------------------------------------------------- the fused aggregate + loss launches, every form
# Four forms — the solo call, S seeds of one prompt (batched), S images with a descriptor table (ImageTable), the table with
# relation rows — share one forward launch helper, one backward launch helper and one autograd Function, as every entry point
# of csrc/smooth_loss.hip fills one LossArgs.  What differs per form is data:
#   fwd, bwd   the C entry points (their names without "ga_" are the census keys)
#   images     S, or None for the solo form (A (npix, Kt), loss (1,), no image argument in the C calls)
#   res, rows  the map side and the rows of `terms` per image (plan.T, or the table's T_max)
#   desc       the descriptor arguments of both C calls: first, last, tokens, T, params, or device_rows, T_max[, device_rel_rows,
#              Q_max], params
#   rel        the forward also returns rel_terms and rel_loss
#   keep       the device buffers `desc` points into (a Function's context holds the form, not the table)
# An ImageTable builds its forms once; the argument forms cost one tuple per call.
LossForm = namedtuple("LossForm", "fwd bwd images res rows desc rel keep", defaults=(None,))


def _args_form(images, res, first, last, plan):
    desc = (first, last, plan.tokens, plan.T, ctypes.byref(plan.params))
    if images is None:
        return LossForm("ga_aggregate_loss_fwd", "ga_smooth_loss_bwd", None, res, plan.T, desc, False)
    return LossForm("ga_aggregate_loss_fwd_batched", "ga_smooth_loss_bwd_batched", images, res, plan.T, desc, False)


def _checked_args_form(maps, images, res, first, last, plan):
    """The argument form of a forward call, after the checks that come before any device work."""
    require_cuda(*maps)
    if plan.T == 0:
        raise GaError("no guided tokens")
    if images is not None and not 1 <= images <= _lib.GA_MAX_IMAGES:
        raise GaError(f"{images} images: a batched launch serves 1 ... {_lib.GA_MAX_IMAGES}")
    _check_boxes(plan, res)
    return _args_form(images, res, first, last, plan)


def _rel_form(table):
    if not table.Q_max:
        raise GaError("the table has no relation rows (Q_max = 0)")
    return table.rel_form


_tickets = {}   # (device index, stream) -> one zeroed 32-bit word (the arrival counter of the fused aggregate + loss launch)
_image_tickets = {}   # (device index, stream) -> GA_MAX_IMAGES zeroed words: image s of a batched aggregate + loss launch counts on word s


def _stream_key(device):
    """Scratch that kernels hand data through (split-K slabs, arrival tickets) is only safe under stream order: one set per
    (device, stream the launch goes to).  Launches captured into a hipGraph keep the set of their capture stream."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    return (idx, torch.cuda.current_stream(idx).cuda_stream)


def _ticket(device, per_image=False):
    """The ticket word of the solo loss launch, or (per_image) the words of a launch that serves S images."""
    words = _image_tickets if per_image else _tickets
    key = _stream_key(device)
    t = words.get(key)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            raise GaError("the batched loss launch's ticket words must exist before a hipGraph capture (ops.prepare_device)"
                          if per_image else
                          "the loss launch's ticket word must exist before a hipGraph capture (call ops.prepare_device first)")
        t = words[key] = torch.zeros(_lib.GA_MAX_IMAGES if per_image else 1, dtype=torch.int32, device=device)
    return t


# data_ptr of a batched dP_bcast -> [images, elements per image, the tensor, views not yet consumed]: the stride-0 head-map
# views that _FusedLoss.backward hands to autograd carry no image stride of their own; the capture backwards find it here
# (_d_probs_arg).  Read as a plain stride-0 map, such a view is image 0's gradient for every image, so every view must reach
# a capture backward through this table: end_image_broadcasts() (called right behind the autograd pass) raises when one did not,
# and drops the tensor.  The entry holds the tensor, so its memory cannot be reused while the entry exists.
_image_broadcasts = {}


def end_image_broadcasts():
    """After a batched backward: every per-image map view must have been consumed by the capture backward's strided entry."""
    left = sum(e[3] for e in _image_broadcasts.values())
    _image_broadcasts.clear()
    if left:
        raise GaError(f"{left} per-image dLoss/dA map(s) of the batched loss reached a consumer other than the capture backward: "
                      "read as a stride-0 map it would give every image image 0's gradient")


def _loss_fwd(form, maps):
    """K2 + K3 + K4 in one launch, any form: maps (list of ([S *] heads_i, res*res, Kt) tensors of one dtype, image-major) ->
    (A, terms, loss[, rel_terms, rel_loss]), each with a leading image axis unless the form is the solo one."""
    maps = [m.contiguous() for m in maps]
    npix, Kt = maps[0].shape[1], maps[0].shape[2]
    S, res = form.images, form.res
    if npix != res * res:
        raise GaError(f"maps have {npix} pixels, expected {res * res}")
    if S and any(m.shape[0] % S for m in maps):
        raise GaError(f"a stored map's head-map count is not a multiple of the {S} images")
    n = len(maps)
    ptrs = (ctypes.c_void_p * n)(*[m.data_ptr() for m in maps])
    heads = (ctypes.c_int * n)(*[m.shape[0] for m in maps])
    dev = maps[0].device
    lead = (S,) if S else ()
    out = (torch.empty(lead + (npix, Kt), dtype=torch.float32, device=dev),
           torch.empty(lead + (form.rows, _lib.GA_TERMS), dtype=torch.float32, device=dev),
           torch.empty(lead or (1,), dtype=torch.float32, device=dev))
    if form.rel:
        out += (torch.empty((S, _lib.GA_IMAGE_MAX_RELATIONS, 4), dtype=torch.float32, device=dev),
                torch.empty((S,), dtype=torch.float32, device=dev))
    _count((form.fwd[3:], form.rows, sum(m.shape[0] for m in maps), npix, Kt, S or maps[0].shape[0], False, str(maps[0].dtype)))
    tickets = _ticket(dev, per_image=bool(S))
    _check_ticketed(getattr(load(), form.fwd)(ptrs, heads, n, *lead, res, Kt, *form.desc, *map(_ptr, out), _ptr(tickets),
                                              dtype_code(maps[0]), stream_ptr()), form.fwd, tickets)
    return out


def _loss_bwd(form, A, dloss, bcast_dtype, bcast_scale):
    """The one backward launch, any form: A as the forward returned it, dloss (S,) on the device (the solo form: (1,), or None
    for 1) -> (dA, dP_bcast or None), both of A's shape; images with dloss == 0 or without guided tokens get exact zeros."""
    A = A.contiguous()
    S, Kt = form.images, A.shape[-1]
    if S and A.shape[0] != S:
        raise GaError(f"A holds {A.shape[0]} images, the table {S}")
    dA = torch.empty_like(A)
    dPb = torch.empty(A.shape, dtype=bcast_dtype, device=A.device) if bcast_dtype is not None else None
    code = _lib.DTYPE_CODE[bcast_dtype] if bcast_dtype is not None else _lib.GA_F32
    if S or dloss is not None:
        dloss = dloss.to(torch.float32).contiguous()
    if S and dloss.numel() != S:
        raise GaError(f"dloss has {dloss.numel()} values for {S} images")
    _count((form.bwd[3:], form.rows, S or 0, form.res * form.res, Kt, 0, bcast_dtype is not None, str(bcast_dtype or torch.float32)))
    check(getattr(load(), form.bwd)(_ptr(A), *((S,) if S else ()), form.res, Kt, *form.desc, _ptr(dloss), _ptr(dA), _ptr(dPb),
                                    float(bcast_scale), code, stream_ptr()), form.bwd)
    return dA, dPb


class _FusedLoss(torch.autograd.Function):
    """(form, *maps) -> what _loss_fwd returns, plus total = box + relation loss behind a relation form.  Only the last output
    (loss, or total) is differentiable.  Its backward is one launch too: the kernel emits the dtype-cast dLoss/dA / n_head_maps
    map that the capture kernels broadcast over the head-maps, so every stored map gets a stride-0 view of it and nothing is
    copied per map.  The forms with images take the per-image dloss vector (0 for an image that takes no update) and hand the
    views over through the image-broadcast table — here, and nowhere else."""

    @staticmethod
    def forward(ctx, form, *maps):
        out = _loss_fwd(form, list(maps))
        if form.rel:
            out += (out[2] + out[4],)
        ctx.save_for_backward(out[0])
        ctx.args = (form, [m.shape for m in maps], maps[0].dtype)
        ctx.mark_non_differentiable(*out[:-1])
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, *grads):
        (A,) = ctx.saved_tensors
        form, shapes, dtype = ctx.args
        if grads[-1] is None:
            return (None,) * (1 + len(shapes))
        per_image = sum(s[0] for s in shapes) // (form.images or 1)
        _, g = _loss_bwd(form, A, grads[-1], dtype, 1.0 / per_image)
        if form.images is None:
            return (None,) + tuple(g.unsqueeze(0).expand(s) for s in shapes)
        end_image_broadcasts()
        _image_broadcasts[g.data_ptr()] = [form.images, g[0].numel(), g, len(shapes)]
        return (None,) + tuple(g[0].unsqueeze(0).expand(s) for s in shapes)


def smooth_loss_bwd(A, res, first, last, plan, dloss=None, bcast_dtype=None, bcast_scale=1.0):
    require_cuda(A, dloss)
    return _loss_bwd(_args_form(None, res, first, last, plan), A, dloss, bcast_dtype, bcast_scale)


def aggregate_loss_fwd(maps, res, first, last, plan):
    """K2 + K3 + K4 in one launch: maps (list of (heads_i, res*res, Kt) tensors of one dtype) ->
    (A (res*res, Kt) f32, terms (T, 8), loss (1,))."""
    return _loss_fwd(_checked_args_form(maps, None, res, first, last, plan), maps)


class AggregateSmoothLoss:
    """(res, first, last, plan, *maps) -> (A (res*res, Kt) f32 [not differentiable here], terms (T, 8), loss (1,)): the
    aggregate and the smoothed box loss as ONE launch; the backward is one launch too (_FusedLoss)."""

    @staticmethod
    def apply(res, first, last, plan, *maps):
        return _FusedLoss.apply(_checked_args_form(maps, None, res, first, last, plan), *maps)


# ------------------------------------------------------------------------- S images per pass (num_images_per_prompt > 1)
def aggregate_loss_fwd_batched(maps, images, res, first, last, plan):
    """ga_aggregate_loss_fwd_batched: maps (list of (images * heads_i, res*res, Kt) tensors, image-major) ->
    (A (images, res*res, Kt) f32, terms (images, T, 8), loss (images,))."""
    return _loss_fwd(_checked_args_form(maps, images, res, first, last, plan), maps)


def smooth_loss_bwd_batched(A, res, first, last, plan, dloss, bcast_dtype=None, bcast_scale=1.0):
    """ga_smooth_loss_bwd_batched: A (S, res*res, Kt), dloss (S,) on the device -> (dA, dP_bcast or None), both (S, res*res, Kt);
    images with dloss == 0 get exact zeros."""
    require_cuda(A, dloss)
    return _loss_bwd(_args_form(A.shape[0], res, first, last, plan), A, dloss, bcast_dtype, bcast_scale)


class AggregateSmoothLossBatched:
    """(images, res, first, last, plan, *maps) -> (A (S, res*res, Kt), terms (S, T, 8), loss (S,)): AggregateSmoothLoss for S
    images in one launch each way."""

    @staticmethod
    def apply(images, res, first, last, plan, *maps):
        return _FusedLoss.apply(_checked_args_form(maps, images, res, first, last, plan), *maps)


# ------------------------------------------------------------------ S images of different prompts / layouts per pass
def _bucket(n):
    cap = 4
    while cap < n:
        cap *= 2
    return cap


def image_table_capacity(T):
    """The T_max bucket a table of images with at most T guided tokens is sized for (4, 8, 16 or 32): calls whose token counts
    fall in one bucket share a table shape, and with it the captured hipGraphs."""
    if not 0 <= T <= _lib.GA_IMAGE_MAX_TOKENS:
        raise GaError(f"{T} guided tokens: an image table row holds at most {_lib.GA_IMAGE_MAX_TOKENS}")
    return _bucket(T)


def relation_capacity(Q):
    """The Q_max bucket a relation table of images with at most Q distinct relation columns is sized for (0: no relation rows;
    else 4, 8, 16 or 32, as image_table_capacity)."""
    if not 0 <= Q <= _lib.GA_REL_MAX_COLUMNS:
        raise GaError(f"{Q} distinct relation columns: a launch serves at most {_lib.GA_REL_MAX_COLUMNS} per image")
    return _bucket(Q) if Q else 0


class RelationPlan:
    """Host-side descriptor of one image's relations (`[CustomLoss:toLeftOf (a, b)]` and the other directions): a list of
    (left_indices, right_indices) — toLeftOf — or (left_indices, right_indices, kind) with kind one of _lib.GA_REL_LEFT_OF,
    GA_REL_RIGHT_OF, GA_REL_ABOVE, GA_REL_BELOW; left holds a's indices and right b's for every kind.  Each index is 0-based in
    the image's text slice (what CustomLossBase.find_indices_for_sub_prompt returns), marshalled into a ga_image_relations_t.
    `width` (last - first of the slice), when given, is checked here; ImageTable.set checks it anyway.  `.relations` holds the
    (left, right) pairs, `.kinds` their kinds."""

    KINDS = (_lib.GA_REL_LEFT_OF, _lib.GA_REL_RIGHT_OF, _lib.GA_REL_ABOVE, _lib.GA_REL_BELOW)

    def __init__(self, relations=(), width=None):
        items = [tuple(item) for item in relations]
        for r, item in enumerate(items):
            if len(item) not in (2, 3):
                raise GaError(f"relation {r}: (left, right) or (left, right, kind) expected, got {len(item)} items")
        kinds = [item[2] if len(item) == 3 else _lib.GA_REL_LEFT_OF for item in items]
        for r, kind in enumerate(kinds):
            if isinstance(kind, bool) or not isinstance(kind, int) or kind not in self.KINDS:
                raise GaError(f"relation {r}: unknown kind {kind!r} (one of {self.KINDS})")
        relations = [(list(item[0]), list(item[1])) for item in items]
        if len(relations) > _lib.GA_IMAGE_MAX_RELATIONS:
            raise GaError(f"{len(relations)} relations: a relation row holds at most {_lib.GA_IMAGE_MAX_RELATIONS}")
        self.row = _lib.ga_image_relations_t()
        self.row.R = len(relations)
        for r, (left, right) in enumerate(relations):
            rel = self.row.rel[r]
            rel.kind = kinds[r]
            for name, side in (("left", left), ("right", right)):
                if not 1 <= len(side) <= _lib.GA_REL_MAX_TOKENS:
                    raise GaError(f"relation {r}: {len(side)} {name} tokens, a relation takes 1 ... {_lib.GA_REL_MAX_TOKENS} per side")
                for k, i in enumerate(side):
                    if int(i) != i or i < 0:
                        raise GaError(f"relation {r}: {name} index {i!r} is not a slice index")
                    getattr(rel, name)[k] = int(i)
            rel.n_left, rel.n_right = len(left), len(right)
        self.relations = relations
        self.kinds = kinds
        self.R = len(relations)
        self.columns = sorted({int(i) for left, right in relations for i in left + right})
        if width is not None:
            self.check_width(width)

    def check_width(self, width, what="relation"):
        for i in self.columns:
            if i >= width:
                raise GaError(f"{what}: index {i} lies outside the text slice of {width} tokens")


class ImageTable:
    """The per-image loss descriptors (ga_image_loss_t rows) of a call whose images differ in prompt, layout or loss settings,
    in ONE device buffer that this object owns for its lifetime: a captured hipGraph reads the rows by pointer, so a later
    call refills the same buffer instead of capturing again.  `set` validates every row on the host, then copies host to
    device once, on the current stream (ordered before every launch enqueued behind it), and only when the bytes change.
    Call-level: res, the smoothing (sigma, kernel size, on / off: one set of Gaussian weights) and the capacity T_max.
    Q_max > 0: the table also owns one relation row per image (ga_image_relations_t) in a second device buffer, filled by
    `set(..., relations=)` under the same rules; Q_max is the capacity of distinct relation columns per image."""

    def __init__(self, images, T_max, res, smooth, sigma, kernel_size, device, Q_max=0):
        if not 1 <= images <= _lib.GA_MAX_IMAGES:
            raise GaError(f"{images} images: a table launch serves 1 ... {_lib.GA_MAX_IMAGES}")
        if not 1 <= T_max <= _lib.GA_IMAGE_MAX_TOKENS or T_max * res * res > 24576:
            raise GaError(f"T_max = {T_max} at res {res}: the table launch serves T_max <= 32 and T_max * res^2 <= 24576")
        if not 0 <= Q_max <= _lib.GA_REL_MAX_COLUMNS or (T_max + Q_max) * res * res > 24576:
            raise GaError(f"T_max = {T_max}, Q_max = {Q_max} at res {res}: the relation launch serves Q_max <= "
                          f"{_lib.GA_REL_MAX_COLUMNS} and (T_max + Q_max) * res^2 <= 24576")
        self.images, self.T_max, self.res, self.Q_max = images, T_max, res, Q_max
        self.rel_rows = self.device_rel_rows = self._rel_uploaded = None
        self.relations = [None] * images
        if Q_max:
            self.rel_rows = (_lib.ga_image_relations_t * images)()
            self.device_rel_rows = torch.zeros(ctypes.sizeof(self.rel_rows), dtype=torch.uint8, device=device)
        self.params = _lib.ga_loss_params_t()   # only sigma, ksize and smooth are read
        self.params.sigma, self.params.ksize, self.params.smooth = sigma, kernel_size, 1 if smooth else 0
        self.rows = (_lib.ga_image_loss_t * images)()
        self.device_rows = torch.zeros(ctypes.sizeof(self.rows), dtype=torch.uint8, device=device)
        self._uploaded = None
        self.plans = [None] * images
        desc = (_ptr(self.device_rows), T_max)
        self.form = LossForm("ga_aggregate_loss_fwd_images", "ga_smooth_loss_bwd_images", images, res, T_max,
                             desc + (ctypes.byref(self.params),), False, self.device_rows)
        self.rel_form = LossForm("ga_aggregate_loss_rel_fwd_images", "ga_smooth_loss_rel_bwd_images", images, res, T_max,
                                 desc + (_ptr(self.device_rel_rows), Q_max, ctypes.byref(self.params)), True,
                                 (self.device_rows, self.device_rel_rows)) if Q_max else None

    def set(self, plans, slices, relations=None):
        """plans: S LossPlans (T = 0: the image is not guided); slices: S (first, last) text slices; relations (a table with
        Q_max > 0): S RelationPlans or None (None: the image has no relation)."""
        if len(plans) != self.images or len(slices) != self.images:
            raise GaError(f"{len(plans)} plans / {len(slices)} slices for a table of {self.images} images")
        if relations is not None and not self.Q_max:
            raise GaError("this table was built without relation rows (Q_max = 0)")
        rel_rows = None
        if self.Q_max:
            relations = list(relations) if relations is not None else [None] * self.images
            if len(relations) != self.images:
                raise GaError(f"{len(relations)} relation plans for a table of {self.images} images")
            rel_rows = (_lib.ga_image_relations_t * self.images)()
            for s, (rp, (first, last)) in enumerate(zip(relations, slices)):
                if rp is None or rp.R == 0:
                    continue
                rp.check_width(int(last) - int(first), f"image {s}")
                if len(rp.columns) > self.Q_max:
                    raise GaError(f"image {s}: {len(rp.columns)} distinct relation columns, the table holds {self.Q_max} per image")
                rel_rows[s] = rp.row
        rows = (_lib.ga_image_loss_t * self.images)()
        for s, (plan, (first, last)) in enumerate(zip(plans, slices)):
            if plan.T > self.T_max:
                raise GaError(f"image {s}: {plan.T} guided tokens, the table holds {self.T_max} per image")
            try:
                _check_boxes(plan, self.res)
            except ZeroDivisionError:
                raise ZeroDivisionError(f"float division by zero (image {s}: a box holds no pixel centre)") from None
            r = rows[s]
            r.first, r.last, r.T = int(first), int(last), plan.T
            if plan.T == 0:
                continue
            for t in range(plan.T):
                col = r.first + plan.tokens[t].token - 1
                if not r.first <= col < r.last:
                    raise GaError(f"image {s}: token {plan.tokens[t].token} lies outside its text slice [{first}, {last})")
                r.tok[t] = plan.tokens[t]
            p = plan.params
            r.strict, r.inside_scale, r.outside_scale, r.center_weight, r.shrink = (p.strict, p.inside_scale, p.outside_scale,
                                                                                    p.center_weight, p.shrink)
        data = bytes(rows)
        self.rows, self.plans = rows, list(plans)
        if data != self._uploaded:
            host = torch.frombuffer(bytearray(data), dtype=torch.uint8).pin_memory()
            self.device_rows.copy_(host, non_blocking=True)
            self._uploaded = data
            self.uploads += 1
        if rel_rows is not None:
            data = bytes(rel_rows)
            self.rel_rows, self.relations = rel_rows, relations
            if data != self._rel_uploaded:
                host = torch.frombuffer(bytearray(data), dtype=torch.uint8).pin_memory()
                self.device_rel_rows.copy_(host, non_blocking=True)
                self._rel_uploaded = data
                self.uploads += 1
        return self

    uploads = 0   # host -> device copies of the rows (a call whose rows equal the previous call's makes none)
    Q_max = 0     # capacity of distinct relation columns per image (0: the table has no relation rows)


def aggregate_loss_fwd_images(maps, table):
    """ga_aggregate_loss_fwd_images: maps (list of (S * heads_i, res*res, Kt) tensors, image-major) with one descriptor row per
    image -> (A (S, res*res, Kt) f32, terms (S, T_max, 8) [rows past an image's T are zero], loss (S,))."""
    require_cuda(*maps)
    return _loss_fwd(table.form, maps)


def smooth_loss_bwd_images(A, table, dloss, bcast_dtype=None, bcast_scale=1.0):
    """ga_smooth_loss_bwd_images: A (S, res*res, Kt), dloss (S,) on the device -> (dA, dP_bcast or None), both (S, res*res, Kt);
    images with dloss == 0 or without guided tokens get exact zeros."""
    require_cuda(A, dloss)
    return _loss_bwd(table.form, A, dloss, bcast_dtype, bcast_scale)


class AggregateSmoothLossImages:
    """(table, *maps) -> (A (S, res*res, Kt), terms (S, T_max, 8), loss (S,)): AggregateSmoothLossBatched with one descriptor
    row per image (ImageTable)."""

    @staticmethod
    def apply(table, *maps):
        require_cuda(*maps)
        return _FusedLoss.apply(table.form, *maps)


# ------------------------------------------------------------------ the toLeftOf relation inside the table launches
def aggregate_loss_rel_fwd_images(maps, table):
    """ga_aggregate_loss_rel_fwd_images: aggregate_loss_fwd_images on a table with relation rows -> (A, terms, loss [the box
    part], rel_terms (S, 4, 4) = (value, v, cL, cR) per relation, rel_loss (S,))."""
    require_cuda(*maps)
    return _loss_fwd(_rel_form(table), maps)


def smooth_loss_rel_bwd_images(A, table, dloss, bcast_dtype=None, bcast_scale=1.0):
    """ga_smooth_loss_rel_bwd_images: the gradient of dloss[s] * (box loss + relation loss) of image s -> (dA, dP_bcast or None)."""
    require_cuda(A, dloss)
    return _loss_bwd(_rel_form(table), A, dloss, bcast_dtype, bcast_scale)


class AggregateSmoothLossRelImages:
    """(table, *maps) -> (A (S, res*res, Kt), terms (S, T_max, 8), box (S,), rel_terms (S, 4, 4), rel (S,), total (S,) = box + rel):
    AggregateSmoothLossImages on a table with relation rows.  Only `total` is differentiable."""

    @staticmethod
    def apply(table, *maps):
        require_cuda(*maps)
        return _FusedLoss.apply(_rel_form(table), *maps)


LossLdsPlan = namedtuple("LossLdsPlan", "use_gcol stage_rows lds_bytes")
_LOSS_PLAN_KINDS = {"fwd": _lib.GA_LOSS_PLAN_FWD, "agg_fwd": _lib.GA_LOSS_PLAN_AGG_FWD, "bwd": _lib.GA_LOSS_PLAN_BWD}


def loss_lds_plan(kind, res, Kt, slots, images=1, table=False, Q_max=None, strict=False, A=None):
    """ga_loss_lds_plan (host only, no device): the LDS plan the loss launch of these sizes runs under, from the code the
    launches take it from -> LossLdsPlan(use_gcol, stage_rows, lds_bytes); GaError with the launch's own status otherwise.
    kind: 'fwd' (smooth_loss_fwd), 'agg_fwd' (aggregate_loss_fwd and its batched / table / relation forms) or 'bwd' (every
    backward).  slots: T of the argument form, T_max of an ImageTable (table=True); Q_max (not None): the relation launches.
    A: the map the launch gets — a tensor (its address), an address, or None for a 16-byte aligned map (what the aggregate
    forward allocates itself)."""
    addr = 4096 if A is None else (A.data_ptr() if torch.is_tensor(A) else int(A))
    gcol, rows, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
    check(load().ga_loss_lds_plan(_LOSS_PLAN_KINDS[kind], 1 if table else 0, 0 if Q_max is None else 1, images, res, Kt, slots,
                                  0 if Q_max is None else Q_max, 1 if strict else 0, ctypes.c_void_p(addr), ctypes.byref(gcol),
                                  ctypes.byref(rows), ctypes.byref(lds)), "ga_loss_lds_plan")
    return LossLdsPlan(gcol.value, rows.value, lds.value)


def _device_vector(values, dtype, device):
    """A small host list as a device tensor (pinned staging, asynchronous copy)."""
    return torch.tensor(values, dtype=dtype).pin_memory().to(device, non_blocking=True)


def latent_axpy_batched(latents, grad, step, active, want_absmean=False):
    """K5 for S images: latents / grad (S, ...); step (S,) f32 and active (S,) int32 on the device (lists are copied there).
    -> (out, absmean (S,) or None); inactive images come out unchanged, bit for bit."""
    require_cuda(latents, grad)
    latents, grad = latents.contiguous(), grad.contiguous().to(latents.dtype)
    S = latents.shape[0]
    if not torch.is_tensor(step):
        step = _device_vector([float(v) for v in step], torch.float32, latents.device)
    if not torch.is_tensor(active):
        active = _device_vector([int(bool(v)) for v in active], torch.int32, latents.device)
    out = torch.empty_like(latents)
    absmean = torch.zeros((S,), dtype=torch.float32, device=latents.device) if want_absmean else None
    n = latents.numel() // S
    _count(("latent_axpy_batched", S, 0, n, 0, 0, bool(want_absmean), str(latents.dtype)))
    check(load().ga_latent_axpy_batched(_ptr(latents), _ptr(grad), _ptr(step), _ptr(active), _ptr(out), _ptr(absmean), S, n,
                                        dtype_code(latents), stream_ptr()), "ga_latent_axpy_batched")
    return out, absmean


def latent_sgd_momentum_batched(latents, grad, momentum, lr, mu, first, active):
    """latent_sgd_momentum for S images in one launch: latents / grad (S, ...); momentum (f32, latents' size, updated in place in
    the slices of the active images); lr (S,) f32, first (S,) int32 and active (S,) int32 on the device (lists are copied
    there).  -> out: an inactive image comes out unchanged, bit for bit, an active one as latent_sgd_momentum leaves its slice.
    Where `first` is set the image's velocity slice is not used (it may hold anything)."""
    require_cuda(latents, grad, momentum)
    if momentum.dtype != torch.float32 or not momentum.is_contiguous() or momentum.numel() != latents.numel():
        raise GaError("latent_sgd_momentum_batched: the velocity buffer is a contiguous float32 tensor of the latents' size")
    latents, grad = latents.contiguous(), grad.contiguous().to(latents.dtype)
    S = latents.shape[0]
    if not torch.is_tensor(lr):
        lr = _device_vector([float(v) for v in lr], torch.float32, latents.device)
    if not torch.is_tensor(first):
        first = _device_vector([int(bool(v)) for v in first], torch.int32, latents.device)
    if not torch.is_tensor(active):
        active = _device_vector([int(bool(v)) for v in active], torch.int32, latents.device)
    for name, vec, dt in (("lr", lr, torch.float32), ("first", first, torch.int32), ("active", active, torch.int32)):
        if vec.dtype != dt or vec.numel() != S or not vec.is_contiguous() or vec.device != latents.device:
            raise GaError(f"latent_sgd_momentum_batched: {name} is a contiguous {dt} device tensor of {S} elements")
    out = torch.empty_like(latents)
    n = latents.numel() // S
    _count(("latent_sgd_momentum_batched", S, 0, n, 0, 0, False, str(latents.dtype)))
    check(load().ga_latent_sgd_momentum_batched(_ptr(latents), _ptr(grad), _ptr(momentum), _ptr(lr), float(mu), _ptr(first),
                                                _ptr(active), _ptr(out), S, n, dtype_code(latents), stream_ptr()),
          "ga_latent_sgd_momentum_batched")
    return out


def latent_axpby_masked(x, y, a, b, active):
    """K6 for S images: out = a*x + b*y where active (S,) int32 (device; a list is copied there), x elsewhere."""
    require_cuda(x, y)
    x, y = x.contiguous(), y.contiguous().to(x.dtype)
    S = x.shape[0]
    if not torch.is_tensor(active):
        active = _device_vector([int(bool(v)) for v in active], torch.int32, x.device)
    out = torch.empty_like(x)
    _count(("latent_axpby_masked", S, 0, x.numel() // S, 0, 0, False, str(x.dtype)))
    check(load().ga_latent_axpby_masked(_ptr(x), _ptr(y), float(a), float(b), _ptr(active), _ptr(out), S, x.numel() // S,
                                        dtype_code(x), stream_ptr()), "ga_latent_axpby_masked")
    return out


def cfg_ddim_step_masked(eps_uncond, eps_text, guidance, x, alpha_t, alpha_prev, active, want_x0=False, prediction="epsilon",
                         eta=0.0, noise=None):
    """CFG + DDIM step for S images; images with active = 0 keep x (bit for bit, whatever their noise slice holds).
    `prediction`, `eta` and `noise` (x's shape: one slice per image) as for cfg_ddim_step."""
    pred = prediction_code(prediction)
    noise = _variance_noise(eta, noise, x)
    require_cuda(eps_uncond, eps_text, x, noise)
    eps_uncond, eps_text, x = eps_uncond.contiguous(), eps_text.contiguous(), x.contiguous()
    S = x.shape[0]
    if not torch.is_tensor(active):
        active = _device_vector([int(bool(v)) for v in active], torch.int32, x.device)
    prev = torch.empty_like(x)
    x0 = torch.empty_like(x) if want_x0 else None
    if noise is not None:
        noise = noise.contiguous()
        _count(("cfg_ddim_step_eta_masked", S, 0, x.numel() // S, 0, pred, bool(want_x0), str(x.dtype)))
        check(load().ga_cfg_ddim_step_eta_masked(_ptr(eps_uncond), _ptr(eps_text), float(guidance), _ptr(x), _ptr(noise),
                                                 float(alpha_t), float(alpha_prev), float(eta), pred, _ptr(active), _ptr(prev),
                                                 _ptr(x0), S, x.numel() // S, dtype_code(x), stream_ptr()),
              "ga_cfg_ddim_step_eta_masked")
    elif pred == _lib.GA_PRED_EPSILON:
        _count(("cfg_ddim_step_masked", S, 0, x.numel() // S, 0, 0, bool(want_x0), str(x.dtype)))
        check(load().ga_cfg_ddim_step_masked(_ptr(eps_uncond), _ptr(eps_text), float(guidance), _ptr(x), float(alpha_t),
                                             float(alpha_prev), _ptr(active), _ptr(prev), _ptr(x0), S, x.numel() // S,
                                             dtype_code(x), stream_ptr()), "ga_cfg_ddim_step_masked")
    else:
        _count(("cfg_ddim_step_pred_masked", S, 0, x.numel() // S, 0, pred, bool(want_x0), str(x.dtype)))
        check(load().ga_cfg_ddim_step_pred_masked(_ptr(eps_uncond), _ptr(eps_text), float(guidance), _ptr(x), float(alpha_t),
                                                  float(alpha_prev), pred, _ptr(active), _ptr(prev), _ptr(x0), S,
                                                  x.numel() // S, dtype_code(x), stream_ptr()), "ga_cfg_ddim_step_pred_masked")
    return prev, x0


def gaussian_weights(kernel_size, sigma):
    w = (ctypes.c_float * (kernel_size * kernel_size))()
    check(load().ga_gaussian_weights(kernel_size, float(sigma), w), "ga_gaussian_weights")
    return torch.tensor(list(w), dtype=torch.float32).reshape(kernel_size, kernel_size)


# --------------------------------------------------------------------------------------- K5 / K6 / DDIM
def latent_axpy(latents, grad, step, want_absmean=False):
    require_cuda(latents, grad)
    latents, grad = latents.contiguous(), grad.contiguous().to(latents.dtype)
    out = torch.empty_like(latents)
    absmean = torch.empty((1,), dtype=torch.float32, device=latents.device) if want_absmean else None
    _count(("latent_axpy", 1, 0, latents.numel(), 0, 0, bool(want_absmean), str(latents.dtype)))
    check(load().ga_latent_axpy(_ptr(latents), _ptr(grad), float(step), _ptr(out), _ptr(absmean), latents.numel(),
                                dtype_code(latents), stream_ptr()), "ga_latent_axpy")
    return out, absmean


def latent_sgd_momentum(latents, grad, momentum, lr, mu, first):
    """One SGD-with-momentum step (the refinement loop under `use_optimizer`): momentum (f32, latents' shape, updated in
    place) <- grad if `first` else mu * momentum + grad; -> latents - lr * momentum as a new tensor.  With `first` the
    buffer's contents are not read."""
    require_cuda(latents, grad, momentum)
    if momentum.dtype != torch.float32 or not momentum.is_contiguous() or momentum.numel() != latents.numel():
        raise GaError("latent_sgd_momentum: the velocity buffer is a contiguous float32 tensor of the latents' size")
    latents, grad = latents.contiguous(), grad.contiguous().to(latents.dtype)
    out = torch.empty_like(latents)
    _count(("latent_sgd_momentum", 1, 0, latents.numel(), 0, 0, bool(first), str(latents.dtype)))
    check(load().ga_latent_sgd_momentum(_ptr(latents), _ptr(grad), _ptr(momentum), float(lr), float(mu), int(bool(first)),
                                        _ptr(out), latents.numel(), dtype_code(latents), stream_ptr()),
          "ga_latent_sgd_momentum")
    return out


def latent_axpby(x, y, a, b):
    require_cuda(x, y)
    x, y = x.contiguous(), y.contiguous().to(x.dtype)
    out = torch.empty_like(x)
    _count(("latent_axpby", 1, 0, x.numel(), 0, 0, False, str(x.dtype)))
    check(load().ga_latent_axpby(_ptr(x), _ptr(y), float(a), float(b), _ptr(out), x.numel(), dtype_code(x),
                                 stream_ptr()), "ga_latent_axpby")
    return out


def prediction_code(prediction):
    """The scheduler's prediction_type -> GA_PRED_*; anything the DDIM step does not serve is a ValueError (no device needed)."""
    try:
        return _lib.PREDICTION_CODE[prediction]
    except (KeyError, TypeError):
        raise ValueError(f"prediction type {prediction!r}: the DDIM step serves {sorted(_lib.PREDICTION_CODE)}") from None


def _variance_noise(eta, noise, x):
    """The checks of `eta` / `noise` the two DDIM wrappers share (ValueError, no device needed): -> the noise operand of an
    eta > 0 launch, None at eta == 0 (the noise, if any, is not looked at)."""
    eta = float(eta)
    if not 0.0 <= eta <= 1.0:   # a NaN fails the comparison
        raise ValueError(f"eta = {eta}: the DDIM step serves 0 <= eta <= 1")
    if eta == 0.0:
        return None
    if noise is None:
        raise ValueError("eta > 0 needs `noise`: the variance noise is the caller's (the step draws nothing)")
    if tuple(noise.shape) != tuple(x.shape) or noise.dtype != x.dtype:
        raise ValueError(f"noise is {tuple(noise.shape)} {noise.dtype}, x is {tuple(x.shape)} {x.dtype}: same shape and dtype")
    return noise


def cfg_ddim_step(eps_uncond, eps_text, guidance, x, alpha_t, alpha_prev, want_x0=False, prediction="epsilon", eta=0.0,
                  noise=None):
    """CFG combine + DDIM step.  `prediction`: what the two model outputs are (the scheduler's prediction_type): at eta = 0
    "epsilon" is the ga_cfg_ddim_step launch, "v_prediction" and "sample" are ga_cfg_ddim_step_pred.  0 < eta <= 1 (stochastic
    DDIM) is ga_cfg_ddim_step_eta for every type, with `noise` (standard normal, x's shape and dtype) as one more operand."""
    pred = prediction_code(prediction)
    noise = _variance_noise(eta, noise, x)
    require_cuda(eps_uncond, eps_text, x, noise)
    eps_uncond, eps_text, x = eps_uncond.contiguous(), eps_text.contiguous(), x.contiguous()
    prev = torch.empty_like(x)
    x0 = torch.empty_like(x) if want_x0 else None
    if noise is not None:
        noise = noise.contiguous()
        _count(("cfg_ddim_step_eta", 1, 0, x.numel(), 0, pred, bool(want_x0), str(x.dtype)))   # D slot: GA_PRED_*
        check(load().ga_cfg_ddim_step_eta(_ptr(eps_uncond), _ptr(eps_text), float(guidance), _ptr(x), _ptr(noise),
                                          float(alpha_t), float(alpha_prev), float(eta), pred, _ptr(prev), _ptr(x0), x.numel(),
                                          dtype_code(x), stream_ptr()), "ga_cfg_ddim_step_eta")
    elif pred == _lib.GA_PRED_EPSILON:
        _count(("cfg_ddim_step", 1, 0, x.numel(), 0, 0, bool(want_x0), str(x.dtype)))
        check(load().ga_cfg_ddim_step(_ptr(eps_uncond), _ptr(eps_text), float(guidance), _ptr(x), float(alpha_t),
                                      float(alpha_prev), _ptr(prev), _ptr(x0), x.numel(), dtype_code(x), stream_ptr()),
              "ga_cfg_ddim_step")
    else:
        _count(("cfg_ddim_step_pred", 1, 0, x.numel(), 0, pred, bool(want_x0), str(x.dtype)))   # D slot: GA_PRED_*
        check(load().ga_cfg_ddim_step_pred(_ptr(eps_uncond), _ptr(eps_text), float(guidance), _ptr(x), float(alpha_t),
                                           float(alpha_prev), pred, _ptr(prev), _ptr(x0), x.numel(), dtype_code(x),
                                           stream_ptr()), "ga_cfg_ddim_step_pred")
    return prev, x0


# --------------------------------------------------------------------------------------- GroupNorm (+SiLU), NHWC
def _nhwc(x):
    return x if x.is_contiguous(memory_format=torch.channels_last) else x.contiguous(memory_format=torch.channels_last)


class GroupNormAct(torch.autograd.Function):
    """y = [silu](group_norm(x [+ chan_bias[:, :, None, None]])) on channels-last (B, C, H, W) tensors;
    differentiable w.r.t. x only (chan_bias is the time-embedding term: it carries no gradient on this path).
    with_alias: returns (y, x) — the caller hands that second output to x's OTHER consumer (the block's skip connection),
    so that both gradients arrive in this node and ga_group_norm_bwd adds them in its own pass (`g_res`); autograd's
    accumulation would be one more launch per block (23 per guidance backward of the SD-1.x UNet)."""

    @staticmethod
    def forward(ctx, x, weight, bias, groups, eps, act, chan_bias, with_alias=False, produced=None):
        """produced = (partials (B, blocks, groups, 2) f32, blocks) from the epilogue of the convolution that made x
        (conv3x3_nhwc(..., gn=...)): the large-level forward is then ONE launch (ga_group_norm_apply) instead of two."""
        require_cuda(x, weight, bias, chan_bias)
        if x.dim() != 4:
            raise GaError("GroupNormAct expects a (B, C, H, W) tensor")
        x = _nhwc(x)
        B, C, H, W = x.shape
        if chan_bias is not None:
            if chan_bias.requires_grad:
                raise GaError("the channel bias of the fused GroupNorm carries no gradient on this path")
            chan_bias = chan_bias.to(x.dtype).contiguous()
            if tuple(chan_bias.shape) != (B, C):
                raise GaError(f"chan_bias must be (B, C) = {(B, C)}, got {tuple(chan_bias.shape)}")
        if produced is not None and produced[0] == "done":     # the producing concatenation's launch ran this norm too
            y, stats = produced[1], produced[2]
            ctx.save_for_backward(x, weight, bias, stats, chan_bias)
            ctx.meta = (groups, bool(act))
            if with_alias:
                ctx.set_materialize_grads(False)
                return y, x.view_as(x)
            return y
        y = torch.empty_like(x, memory_format=torch.channels_last)
        stats = torch.empty((B, groups, 2), dtype=torch.float32, device=x.device)
        if produced is not None:
            partials, blocks = produced
            _count(("group_norm_apply", B, groups, H * W, blocks, C, bool(act), str(x.dtype)))
            check(load().ga_group_norm_apply(_ptr(x), _ptr(chan_bias), _ptr(weight), _ptr(bias), _ptr(y), _ptr(stats),
                                             _ptr(partials), blocks, B, H * W, C, groups, float(eps), int(bool(act)),
                                             dtype_code(x), stream_ptr()), "ga_group_norm_apply")
        else:
            ws = torch.empty((B * 257 * groups * 2,), dtype=torch.float32, device=x.device)
            _count(("group_norm_fwd", B, groups, H * W, 0, C, bool(act), str(x.dtype)))
            check(load().ga_group_norm_fwd(_ptr(x), _ptr(chan_bias), _ptr(weight), _ptr(bias), _ptr(y), _ptr(stats), _ptr(ws),
                                           B, H * W, C, groups, float(eps), int(bool(act)), dtype_code(x), stream_ptr()),
                  "ga_group_norm_fwd")
        ctx.save_for_backward(x, weight, bias, stats, chan_bias)
        ctx.meta = (groups, bool(act))
        if with_alias:
            ctx.set_materialize_grads(False)
            return y, x.view_as(x)
        return y

    @staticmethod
    def backward(ctx, dy, g_alias=None):
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            raise GaError("GroupNorm weight gradients are not part of the guided-attention path (frozen UNet)")
        if dy is None:           # only the alias was differentiated
            return g_alias, None, None, None, None, None, None, None, None
        x, weight, bias, stats, chan_bias = ctx.saved_tensors
        groups, act = ctx.meta
        B, C, H, W = x.shape
        dy = _nhwc(dy)
        if g_alias is not None:
            g_alias = _nhwc(g_alias)
        dx = torch.empty_like(x, memory_format=torch.channels_last)
        ws = torch.empty((B * 257 * groups * 2,), dtype=torch.float32, device=x.device)
        _count(("group_norm_bwd", B, groups, H * W, 0, C, bool(act), str(x.dtype)))
        check(load().ga_group_norm_bwd(_ptr(x), _ptr(chan_bias), _ptr(dy), _ptr(weight), _ptr(bias), _ptr(stats),
                                       _ptr(g_alias), _ptr(dx), _ptr(ws), B, H * W, C, groups, int(act), dtype_code(x),
                                       stream_ptr()),
              "ga_group_norm_bwd")
        return dx, None, None, None, None, None, None, None, None


def _gn_versions(x, chan_bias):
    """What producer statistics attached to x (`_ga_gn`) were taken from: the version counters of x (a view shares its base's)
    and of the channel bias.  An in-place change of either after the producer ran moves a counter, and group_norm_act then takes
    its own statistics instead of stale ones."""
    return (x._version, None if chan_bias is None else chan_bias._version)


def group_norm_act(x, weight, bias, groups, eps, act, chan_bias=None, with_alias=False):
    """-> y, or (y, x) with with_alias (use that x for the skip connection: see GroupNormAct).
    When x came out of conv3x3(..., gn_for=(groups, chan_bias)) — the convolution's epilogue took the statistics this norm
    needs (same group count, the SAME channel-bias tensor) — the statistics launch is skipped."""
    pre = getattr(x, "_ga_gn", None)
    produced = None
    if pre is not None and pre["groups"] == groups and pre["chan_bias"] is chan_bias and pre["shape"] == tuple(x.shape) and \
            pre.get("versions") == _gn_versions(x, chan_bias):
        if "done" not in pre:
            produced = (pre["partials"], pre["blocks"])
        elif pre["weight"] is weight and pre["bias"] is bias and pre["eps"] == float(eps) and pre["act"] == bool(act) and \
                pre.get("norm_versions") == (weight._version, bias._version):
            produced = ("done",) + pre.pop("done")     # handed out once: a second norm of the same tensor launches its own
    return GroupNormAct.apply(x, weight, bias, groups, eps, act, chan_bias, with_alias, produced)


def gn_fused_with_cat(HW, C, groups, dtype):
    """True when ga_group_norm_fwd is ONE launch for the shape: a concatenation in front of it joins that launch."""
    code = _lib.DTYPE_CODE.get(dtype)
    return code is not None and (C // groups) % 2 == 0 and bool(load().ga_group_norm_one_launch(HW, C, groups, code))


def gn_two_launch(HW, C, groups, dtype):
    """True when ga_group_norm_fwd takes two launches for the shape (a producer's partial sums then save one)."""
    code = _lib.DTYPE_CODE.get(dtype)
    return code is not None and bool(load().ga_group_norm_two_launch(HW, C, groups, code))


# --------------------------------------------------------------------------------------- feed-forward / residual epilogues
class Geglu(torch.autograd.Function):
    """y = x[..., :F] * gelu(x[..., F:]) on the GEGLU projection's output (diffusers 0.12.1 GEGLU.forward)."""

    @staticmethod
    def forward(ctx, x):
        require_cuda(x)
        x = x.contiguous()
        F2 = x.shape[-1]
        rows = x.numel() // F2
        y = torch.empty(x.shape[:-1] + (F2 // 2,), dtype=x.dtype, device=x.device)
        _count(("geglu_fwd", rows, 0, 0, 0, F2 // 2, False, str(x.dtype)))
        check(load().ga_geglu_fwd(_ptr(x), _ptr(y), rows, F2 // 2, dtype_code(x), stream_ptr()), "ga_geglu_fwd")
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = dy.contiguous()
        F2 = x.shape[-1]
        dx = torch.empty_like(x)
        _count(("geglu_bwd", x.numel() // F2, 0, 0, 0, F2 // 2, False, str(x.dtype)))
        check(load().ga_geglu_bwd(_ptr(x), _ptr(dy), _ptr(dx), x.numel() // F2, F2 // 2, dtype_code(x), stream_ptr()),
              "ga_geglu_bwd")
        return dx


def geglu(x):
    return Geglu.apply(x)


def geglu_backward(x, dy):
    """d(h * gelu(gate)) w.r.t. the projection x = [h | gate] (..., 2F) given dy (..., F)."""
    require_cuda(x, dy)
    x, dy = x.contiguous(), dy.contiguous()
    F2 = x.shape[-1]
    dx = torch.empty_like(x)
    _count(("geglu_bwd", x.numel() // F2, 0, 0, 0, F2 // 2, False, str(x.dtype)))
    check(load().ga_geglu_bwd(_ptr(x), _ptr(dy), _ptr(dx), x.numel() // F2, F2 // 2, dtype_code(x), stream_ptr()),
          "ga_geglu_bwd")
    return dx


def cat_channels_supported(a, b):
    """Both channels-last-dense 4-D tensors of one 16- or 32-bit dtype on the GPU, same (B, H, W), channel counts that are
    whole 16-byte vectors, and a vector count the kernel's 32-bit row division serves."""
    if not (a.is_cuda and b.is_cuda and a.dim() == 4 and b.dim() == 4 and a.dtype == b.dtype):
        return False
    if a.dtype not in (torch.float16, torch.bfloat16, torch.float32):
        return False
    if a.shape[0] != b.shape[0] or a.shape[2:] != b.shape[2:]:
        return False
    per = 16 // a.element_size()
    if a.shape[1] % per or b.shape[1] % per:
        return False
    rows = a.shape[0] * a.shape[2] * a.shape[3]
    # Measured domain: maps of <= 64 x 64 pixels and results of <= 24 MB (every concatenation of the 512^2 SD-1.x passes:
    # -0.8 ... -0.9 % per forward pass, profiles/r3_ab_cat_channels.txt).  On the 768^2 configuration (96 x 96 maps, results up
    # to 53 MB) the library's copy was the faster one (0.917 against 0.887 images/s with every concatenation on this kernel).
    if a.shape[2] * a.shape[3] > 4096 or rows * (a.shape[1] + b.shape[1]) * a.element_size() > 24 * 1024 * 1024:
        return False
    return all(rows * (t.shape[1] // per) ** 2 < (1 << 32) for t in (a, b))   # the kernel's 32-bit multiply-high row division


class CatChannels(torch.autograd.Function):
    """torch.cat([a, b], dim=1) on channels-last activations as one ga_cat_channels launch (the UpBlock's concatenation of
    the running activation with the skip connection: diffusers 0.12.1 UpBlock2D / CrossAttnUpBlock2D, called from the
    reference's UNet forward pipeline_guided_attention.py:583-743).  Backward: the two channel slices of the gradient, as
    views — what torch.cat's own backward returns."""

    @staticmethod
    def forward(ctx, a, b):
        require_cuda(a, b)
        a, b = _nhwc(a), _nhwc(b)
        B, C1, H, W = a.shape
        C2 = b.shape[1]
        out = torch.empty((B, C1 + C2, H, W), dtype=a.dtype, device=a.device, memory_format=torch.channels_last)
        check(load().ga_cat_channels(_ptr(a), _ptr(b), _ptr(out), B * H * W, C1, C2, a.element_size(), stream_ptr()),
              "ga_cat_channels")
        ctx.c1 = C1
        return out

    @staticmethod
    def backward(ctx, g):
        return g[:, :ctx.c1], g[:, ctx.c1:]


class _CatChannelsGn(CatChannels):
    """CatChannels whose launch also takes the consuming GroupNorm's statistics (ga_cat_channels_gn); what it took leaves through
    `box` (forward-only side data without a gradient, as for _Conv3x3Gn)."""

    @staticmethod
    def forward(ctx, a, b, groups, box):
        require_cuda(a, b)
        a, b = _nhwc(a), _nhwc(b)
        B, C1, H, W = a.shape
        C2 = b.shape[1]
        blocks = int(load().ga_cat_channels_gn_blocks(H * W, C1 + C2, groups, dtype_code(a)))
        out = torch.empty((B, C1 + C2, H, W), dtype=a.dtype, device=a.device, memory_format=torch.channels_last)
        partials = torch.empty((B, blocks, groups, 2), dtype=torch.float32, device=a.device)
        check(load().ga_cat_channels_gn(_ptr(a), _ptr(b), _ptr(out), _ptr(partials), B, H * W, C1, C2, groups, dtype_code(a),
                                        stream_ptr()), "ga_cat_channels_gn")
        ctx.c1 = C1
        box.append((partials, blocks))
        return out

    @staticmethod
    def backward(ctx, g):
        return g[:, :ctx.c1], g[:, ctx.c1:], None, None


class _CatGroupNorm(CatChannels):
    """CatChannels and the GroupNorm(+SiLU) that consumes it as ONE launch (ga_cat_group_norm_fwd: the norms that are a single
    launch anyway).  The Function's output is the concatenation; the norm's output and statistics leave through `box` and
    GroupNormAct picks them up instead of launching (it stays the autograd node of the norm)."""

    @staticmethod
    def forward(ctx, a, b, weight, bias, groups, eps, act, box):
        require_cuda(a, b, weight, bias)
        a, b = _nhwc(a), _nhwc(b)
        B, C1, H, W = a.shape
        C2 = b.shape[1]
        out = torch.empty((B, C1 + C2, H, W), dtype=a.dtype, device=a.device, memory_format=torch.channels_last)
        y = torch.empty_like(out, memory_format=torch.channels_last)
        stats = torch.empty((B, groups, 2), dtype=torch.float32, device=a.device)
        _count(("group_norm_fwd", B, groups, H * W, 0, C1 + C2, bool(act), str(a.dtype)))
        check(load().ga_cat_group_norm_fwd(_ptr(a), _ptr(b), _ptr(out), _ptr(weight), _ptr(bias), _ptr(y), _ptr(stats), B, H * W,
                                           C1, C2, groups, float(eps), int(bool(act)), dtype_code(a), stream_ptr()),
              "ga_cat_group_norm_fwd")
        ctx.c1 = C1
        box.append((y, stats))
        return out

    @staticmethod
    def backward(ctx, g):
        return g[:, :ctx.c1], g[:, ctx.c1:], None, None, None, None, None, None


def cat_channels(a, b, gn_for=None, norm=None):
    """torch.cat([a, b], dim=1); the HIP launch where cat_channels_supported, the library otherwise (CPU oracle, odd widths).
    gn_for = the group count of the GroupNorm (no channel bias) that consumes the result: where that norm would take two launches
    this launch takes its statistics too, and the result carries them (`_ga_gn`, read by group_norm_act).
    norm = (weight, bias, eps, act) of that norm: where it is a single launch anyway, concatenation and norm are ONE launch, and
    the result carries the norm's output (`_ga_gn["done"]`) for group_norm_act to hand out."""
    if cat_channels_supported(a, b) and gn_for is not None and norm is not None and (a.shape[1] + b.shape[1]) % gn_for == 0 and \
            a.dtype in (torch.float16, torch.bfloat16) and norm[0].dtype == a.dtype and a.shape[1] % 2 == 0 and \
            gn_fused_with_cat(a.shape[2] * a.shape[3], a.shape[1] + b.shape[1], gn_for, a.dtype):
        weight, bias, eps, act = norm
        box = []
        y = _CatGroupNorm.apply(a, b, weight, bias, gn_for, eps, act, box)
        out, stats = box[0]
        y._ga_gn = {"done": (out, stats), "groups": gn_for, "chan_bias": None, "shape": tuple(y.shape), "weight": weight,
                    "bias": bias, "eps": float(eps), "act": bool(act), "versions": _gn_versions(y, None),
                    "norm_versions": (weight._version, bias._version)}
        return y
    if cat_channels_supported(a, b):
        if gn_for is not None and a.dtype in (torch.float16, torch.bfloat16) and (a.shape[1] + b.shape[1]) % gn_for == 0 and \
                gn_two_launch(a.shape[2] * a.shape[3], a.shape[1] + b.shape[1], gn_for, a.dtype) and \
                load().ga_cat_channels_gn_blocks(a.shape[2] * a.shape[3], a.shape[1] + b.shape[1], gn_for, dtype_code(a)):
            box = []
            y = _CatChannelsGn.apply(a, b, gn_for, box)
            partials, blocks = box[0]
            y._ga_gn = {"partials": partials, "blocks": blocks, "groups": gn_for, "chan_bias": None, "shape": tuple(y.shape),
                        "versions": _gn_versions(y, None)}
            return y
        return CatChannels.apply(a, b)
    return torch.cat([a, b], dim=1)


class BiasResidualAdd(torch.autograd.Function):
    """out = y + bias[c] + residual on channels-last activations (ResnetBlock2D: conv2's bias and the skip
    connection in one pass).  bias receives no gradient (frozen UNet)."""

    @staticmethod
    def forward(ctx, y, bias, residual):
        require_cuda(y, residual)
        if ctx.needs_input_grad[1]:
            raise GaError("bias gradients are not part of the guided-attention path (frozen UNet)")
        y, residual = _nhwc(y), _nhwc(residual)
        B, C, H, W = y.shape
        out = torch.empty_like(y, memory_format=torch.channels_last)
        _count(("bias_residual_add", B * H * W, 0, 0, 0, C, bias is not None, str(y.dtype)))
        check(load().ga_bias_residual_add(_ptr(y), _ptr(bias), _ptr(residual), _ptr(out), B * H * W, C, dtype_code(y),
                                          stream_ptr()), "ga_bias_residual_add")
        return out

    @staticmethod
    def backward(ctx, g):
        return g, None, g


def bias_residual_add(y, bias, residual):
    return BiasResidualAdd.apply(y, bias, residual)


def _ln_fwd(a, x, weight, bias, eps, need_stats):
    require_cuda(x, weight, bias)
    x = x.contiguous()
    C = x.shape[-1]
    rows = x.numel() // C
    y = torch.empty_like(x)
    stats = torch.empty((rows, 2), dtype=torch.float32, device=x.device) if need_stats else None
    xnew = None
    if a is not None:
        a = a.contiguous()
        xnew = torch.empty_like(x)
    _count(("add_layer_norm_fwd", rows, 0, 0, 0, C, a is not None, str(x.dtype)))
    check(load().ga_add_layer_norm_fwd(_ptr(a), _ptr(x), _ptr(weight), _ptr(bias), _ptr(xnew), _ptr(y), _ptr(stats), rows,
                                       C, float(eps), dtype_code(x), stream_ptr()), "ga_add_layer_norm_fwd")
    return (x if a is None else xnew), y, stats


def _ln_bwd(row, stats, weight, g_y, g_res):
    C = row.shape[-1]
    g_y = g_y.contiguous()
    g_res = g_res.contiguous() if g_res is not None else None
    d = torch.empty_like(row)
    _count(("add_layer_norm_bwd", row.numel() // C, 0, 0, 0, C, g_res is not None, str(row.dtype)))
    check(load().ga_add_layer_norm_bwd(_ptr(row), _ptr(stats), _ptr(weight), _ptr(g_y), _ptr(g_res), _ptr(d),
                                       row.numel() // C, C, dtype_code(row), stream_ptr()), "ga_add_layer_norm_bwd")
    return d


def _frozen(ctx, first):
    if ctx.needs_input_grad[first] or ctx.needs_input_grad[first + 1]:
        raise GaError("LayerNorm weight gradients are not part of the guided-attention path (frozen UNet)")


class LayerNorm(torch.autograd.Function):
    """y = LayerNorm(x) over the last dimension (one wave per row)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        _frozen(ctx, 1)
        row, y, stats = _ln_fwd(None, x, weight, bias, eps, ctx.needs_input_grad[0])
        if stats is not None:
            ctx.save_for_backward(row, stats, weight)
        return y

    @staticmethod
    def backward(ctx, g_y):
        row, stats, weight = ctx.saved_tensors
        return _ln_bwd(row, stats, weight, g_y, None), None, None, None


class AddLayerNorm(torch.autograd.Function):
    """(x_new, y) = (a + x, LayerNorm(a + x)).  The backward folds the gradient arriving at x_new from its other
    consumer (the next residual add) into the same launch."""

    @staticmethod
    def forward(ctx, a, x, weight, bias, eps):
        _frozen(ctx, 2)
        xnew, y, stats = _ln_fwd(a, x, weight, bias, eps, ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        if stats is not None:
            ctx.save_for_backward(xnew, stats, weight)
        return xnew, y

    @staticmethod
    def backward(ctx, g_xnew, g_y):
        xnew, stats, weight = ctx.saved_tensors
        d = g_xnew if g_y is None else _ln_bwd(xnew, stats, weight, g_y, g_xnew)
        return d, d, None, None, None


def layer_norm(x, weight, bias, eps):
    return LayerNorm.apply(x, weight, bias, eps)


def add_layer_norm(a, x, weight, bias, eps):
    """-> (a + x, LayerNorm(a + x))"""
    return AddLayerNorm.apply(a, x, weight, bias, eps)


# --------------------------------------------------------------------------------------- 3x3 convolution (implicit GEMM)
_conv_plan_cache = {}
_conv_pack_cache = {}   # (weight data_ptr, version, dtype, transpose) -> packed tensor (weights are frozen on this path)


_conv_plan_table = None


def _measured_conv_plans():
    """{(M, Cin, Cout, stride): (bm, bn, splits)} measured on an MI355X for the UNet's own shapes (tools/conv_tune.py);
    shapes not listed take the rule of ga_conv3x3_plan."""
    global _conv_plan_table
    if _conv_plan_table is None:
        import json
        from pathlib import Path
        path = Path(__file__).resolve().parent / "conv_plans.json"
        _conv_plan_table = {}
        if path.exists():
            for k, v in json.loads(path.read_text()).items():
                _conv_plan_table[tuple(int(x) for x in k.split(","))] = tuple(v)
    return _conv_plan_table


def conv3x3_plan(B, H, W, Cin, Cout, stride):
    key = (B, H, W, Cin, Cout, stride)
    plan = _conv_plan_cache.get(key)
    if plan is None:
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        hit = _measured_conv_plans().get((B * Ho * Wo, Cin, Cout, stride))
        if hit is not None:
            bm, bn, sp = hit
        else:
            c_bm, c_bn, c_sp, c_ws = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
            check(load().ga_conv3x3_plan(B, H, W, Cin, Cout, stride, ctypes.byref(c_bm), ctypes.byref(c_bn), ctypes.byref(c_sp),
                                         ctypes.byref(c_ws)), "ga_conv3x3_plan")
            bm, bn, sp = c_bm.value, c_bn.value, c_sp.value
        # the slices' f32 slabs live in the persistent per-device scratch: a plan never asks for more than it holds
        floats = lambda k: int(load().ga_splitk_workspace_floats(B * Ho * Wo, Cout, bm, bn, k))  # noqa: E731
        while sp > 1 and floats(sp) > LIN_SLAB_FLOATS:
            sp -= 1
        plan = _conv_plan_cache[key] = (bm, bn, sp, floats(sp))
    return plan


def conv3x3_packed_weights(weight, transpose_flip):
    """Blocked [9][N / 64][C / 64][64][64] pack (csrc/conv3x3.hip) of a (Cout, Cin, 3, 3) weight (any strides), cached per
    (storage, version)."""
    key = (weight.data_ptr(), weight._version, weight.dtype, bool(transpose_flip), tuple(weight.stride()), tuple(weight.shape))
    entry = _conv_pack_cache.get(key)
    # the entry is only good for the tensor object it was made from: a freed weight's address can be handed to another
    # tensor of the same shape with other contents (tests do that; the UNet's frozen parameters never move)
    hit = entry[1] if entry is not None and entry[0]() is weight else None
    if hit is None:
        require_cuda(weight)
        Cout, Cin = weight.shape[0], weight.shape[1]
        N, C = (Cin, Cout) if transpose_flip else (Cout, Cin)
        hit = torch.empty(int(load().ga_conv3x3_packed_elems(N, C)), dtype=weight.dtype, device=weight.device)
        so, si, sy, sx = weight.stride()
        check(load().ga_conv3x3_pack_weights(_ptr(weight), _ptr(hit), Cout, Cin, so, si, sy, sx, int(bool(transpose_flip)),
                                             dtype_code(weight), stream_ptr()), "ga_conv3x3_pack_weights")
        if len(_conv_pack_cache) > 512:
            # captured hipGraphs read the packs by raw pointer: only entries whose weight tensor is gone may be dropped
            # (a live weight's pack must stay where it is for as long as a graph may replay against it)
            for dead in [k for k, (ref, _) in _conv_pack_cache.items() if ref() is None]:
                del _conv_pack_cache[dead]
        _conv_pack_cache[key] = (weakref.ref(weight), hit)
    return keep_alive(hit)


CONV_KC = 64   # channels per k-step of ga_conv3x3_nhwc (kKC in csrc/conv3x3.hip): Cin must be a multiple


def conv3x3_supported(x, weight, stride=1):
    return (x.is_cuda and x.dtype in (torch.float16, torch.bfloat16) and weight.shape[2:] == (3, 3) and
            weight.shape[1] % CONV_KC == 0 and weight.shape[0] % CONV_KC == 0 and stride in (1, 2))   # both ways round: backward


def conv3x3_nhwc(x, wp, cout, stride=1, bias=None, residual=None, plan=None, gn=None):
    """x (B, Cin, H, W) channels-last, wp the [9][Cout][Cin] pack -> y (B, Cout, Ho, Wo) channels-last.
    gn = (groups, chan_bias (B, Cout) or None): the epilogue also leaves the GroupNorm statistics of y (+ chan_bias) for the
    norm layer that consumes it -> (y, (partials, blocks)) — or (y, None) where the shape is not one that saves a launch."""
    require_cuda(x, wp, bias, residual)
    x = _nhwc(x)
    B, Cin, H, W = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    bm, bn, splits = (plan or conv3x3_plan(B, H, W, Cin, cout, stride))[:3]
    y = torch.empty((B, cout, Ho, Wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    ws, tickets = splitk_workspace(x.device, B * Ho * Wo, cout, bm, bn, splits)
    if residual is not None:
        residual = _nhwc(residual)
    _count(("conv3x3", B, Cin, H * W, stride, cout, bias is not None or residual is not None, str(x.dtype)))
    if gn is not None:
        groups, cb = gn
        blocks = int(load().ga_conv3x3_gn_blocks(H, W, cout, groups, bm, bn)) if stride == 1 else 0
        if blocks and gn_two_launch(H * W, cout, groups, x.dtype):
            if cb is not None:
                require_cuda(cb)
                cb = cb.to(x.dtype).contiguous()
                if tuple(cb.shape) != (B, cout):
                    raise GaError(f"chan_bias must be (B, C) = {(B, cout)}, got {tuple(cb.shape)}")
            partials = torch.empty((B, blocks, groups, 2), dtype=torch.float32, device=x.device)
            _check_ticketed(load().ga_conv3x3_nhwc_gn(_ptr(x), _ptr(wp), _ptr(y), _ptr(ws), _ptr(tickets), _ptr(bias),
                                                      _ptr(residual), B, H, W, Cin, cout, bm, bn, splits, dtype_code(x),
                                                      stream_ptr(), _ptr(partials), _ptr(cb), groups),
                            "ga_conv3x3_nhwc_gn", tickets)
            return y, (partials, blocks)
    _check_ticketed(load().ga_conv3x3_nhwc(_ptr(x), _ptr(wp), _ptr(y), _ptr(ws), _ptr(tickets), _ptr(bias), _ptr(residual), B,
                                           H, W, Cin, cout, stride, bm, bn, splits, dtype_code(x), stream_ptr()),
                    "ga_conv3x3_nhwc", tickets)
    return (y, None) if gn is not None else y


GA_ERR_SHAPE = -2   # include/ga_hip.h
_no_fused_upsample = set()   # (B, H, W, Cin, Cout, dtype) the patch kernel does not serve: the caller up-samples itself


def conv3x3_up2x_nhwc(x, wp, cout, bias=None, plan=None):
    """conv3x3(nearest-neighbour 2x up-sampling of x) without the up-sampled tensor (ga_conv3x3_up2x_nhwc), or None when the
    shape is not served by the patch kernel."""
    require_cuda(x, wp, bias)
    x = _nhwc(x)
    B, Cin, H, W = x.shape
    key = (B, H, W, Cin, cout, x.dtype)
    if key in _no_fused_upsample:
        return None
    bm, bn, splits = (plan or conv3x3_plan(B, 2 * H, 2 * W, Cin, cout, 1))[:3]
    y = torch.empty((B, cout, 2 * H, 2 * W), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    ws, tickets = splitk_workspace(x.device, B * 4 * H * W, cout, bm, bn, splits)
    rc = load().ga_conv3x3_up2x_nhwc(_ptr(x), _ptr(wp), _ptr(y), _ptr(ws), _ptr(tickets), _ptr(bias), None, B, H, W, Cin,
                                     cout, bm, bn, splits, dtype_code(x), stream_ptr())
    if rc == GA_ERR_SHAPE:
        _no_fused_upsample.add(key)
        return None
    _check_ticketed(rc, "ga_conv3x3_up2x_nhwc", tickets)
    _count(("conv3x3", B, Cin, 4 * H * W, 1, cout, bias is not None, str(x.dtype)))
    return y


class UpsampleConv3x3(torch.autograd.Function):
    """y = conv2d(interpolate(x, scale_factor=2, mode="nearest"), weight, padding=1) + bias (diffusers 0.12.1 Upsample2D)
    in one launch; backward: the stride-1 backward-to-input kernel, then the 2x2 sums of the up-sampling's adjoint."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        if ctx.needs_input_grad[1] or (bias is not None and ctx.needs_input_grad[2]):
            raise GaError("convolution weight gradients are not part of the guided-attention path (frozen UNet)")
        y = conv3x3_up2x_nhwc(x, conv3x3_packed_weights(weight, False), weight.shape[0], bias)
        if y is None:
            up = torch.nn.functional.interpolate(x, scale_factor=2.0, mode="nearest")
            y = conv3x3_nhwc(up, conv3x3_packed_weights(weight, False), weight.shape[0], 1, bias)
        ctx.weight, ctx.in_shape = weight, tuple(x.shape)
        return y

    @staticmethod
    def backward(ctx, gy):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        g_up = conv3x3_nhwc(_nhwc(gy), conv3x3_packed_weights(ctx.weight, True), ctx.weight.shape[1], 1)
        B, C, H, W = ctx.in_shape
        gx = torch.ops.aten.upsample_nearest2d_backward(g_up, [2 * H, 2 * W], [B, C, H, W], 2.0, 2.0)
        return gx, None, None


def upsample_conv3x3(x, weight, bias=None):
    return UpsampleConv3x3.apply(x, weight, bias)


class Conv3x3(torch.autograd.Function):
    """y = conv2d(x, weight, bias=None, padding=1, stride) (+ bias + residual) on channels-last 16-bit activations.
    Differentiable w.r.t. x (stride 1: the same kernel on the flipped / transposed pack) and the residual; the weights
    are frozen on this path."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, stride, gn=None):
        """gn (see conv3x3_nhwc): the second output then holds (partials, blocks) for the consuming norm, as a Python attribute
        of the first (`_ga_gn_out`): forward-only side data, no gradient."""
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            raise GaError("convolution weight gradients are not part of the guided-attention path (frozen UNet)")
        wp = conv3x3_packed_weights(weight, False)
        ctx.weight, ctx.stride, ctx.in_shape = weight, stride, tuple(x.shape)
        ctx.has_res = residual is not None
        if gn is None:
            return conv3x3_nhwc(x, wp, weight.shape[0], stride, bias, residual)
        y, made = conv3x3_nhwc(x, wp, weight.shape[0], stride, bias, residual, gn=gn)
        ctx.gn_made = made
        return y

    @staticmethod
    def backward(ctx, gy):
        weight, stride = ctx.weight, ctx.stride
        gx = None
        # ONE dense copy when the gradient is a strided view (a channel slice of a concatenation's gradient): the kernel below
        # and the skip connection's consumer (ga_group_norm_bwd's g_res) both read it
        gy = _nhwc(gy)
        if ctx.needs_input_grad[0]:
            if stride == 1:
                gx = conv3x3_nhwc(gy, conv3x3_packed_weights(weight, True), weight.shape[1], 1)
            else:   # the three down-sampling convolutions: library transposed convolution
                gx = torch.nn.grad.conv2d_input(ctx.in_shape, weight, gy, stride=stride, padding=1)
        return gx, None, None, (gy if ctx.has_res else None), None


def conv3x3(x, weight, bias=None, residual=None, stride=1, gn_for=None):
    """gn_for = (groups, chan_bias or None) of the GroupNorm that consumes the result: where that norm would take two launches
    the convolution's epilogue takes its statistics, and the result carries them (`_ga_gn`, read by group_norm_act)."""
    if gn_for is None:
        return Conv3x3.apply(x, weight, bias, residual, stride)
    groups, cb = gn_for
    B, _, H, W = x.shape
    cout = weight.shape[0]
    if stride != 1 or not gn_two_launch(H * W, cout, groups, x.dtype):
        return Conv3x3.apply(x, weight, bias, residual, stride)
    box = []
    y = _Conv3x3Gn.apply(x, weight, bias, residual, (groups, cb), box)
    if box and box[0] is not None:
        partials, blocks = box[0]
        y._ga_gn = {"partials": partials, "blocks": blocks, "groups": groups, "chan_bias": cb, "shape": tuple(y.shape),
                    "versions": _gn_versions(y, cb)}
    return y


class _Conv3x3Gn(Conv3x3):
    """Conv3x3 (stride 1) whose epilogue also takes the consuming GroupNorm's statistics; what it took leaves through `box` (a
    Function's outputs are tensors; this is forward-only side data without a gradient)."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, gn, box):
        y = Conv3x3.forward(ctx, x, weight, bias, residual, 1, gn)
        box.append(ctx.gn_made)
        return y

    @staticmethod
    def backward(ctx, gy):
        return Conv3x3.backward(ctx, gy) + (None,)


conv3x3.supported = conv3x3_supported
conv3x3.upsample = upsample_conv3x3


# --------------------------------------------------------------------------------------- conv_in / conv_out (one side 4 channels)
_thin_pack_cache = {}


def conv3x3_thin_supported(x, weight, stride=1, forward_only=False):
    """The UNet's edge convolutions (csrc/thin_conv.hip): 3x3, stride 1, 4 channels in or 4 channels out, 16-bit, W % 16 == 0.
    forward_only: the caller never differentiates (the VAE decoder) — the adjoint kernel need not serve the shape (the C -> 4
    kernel stops at 320 channels, the 4 -> C kernel at 4096: the decoder's conv_in is 4 -> 512)."""
    if not (x.is_cuda and x.dim() == 4 and x.dtype in (torch.float16, torch.bfloat16) and weight.dtype == x.dtype
            and tuple(weight.shape[2:]) == (3, 3) and stride == 1 and x.shape[1] == weight.shape[1]):
        return False
    cout, cin = weight.shape[0], weight.shape[1]
    if min(cin, cout) != 4 or max(cin, cout) % 64 != 0:     # both ways round: the backward is the other kernel
        return False
    lib = load()
    return bool(lib.ga_conv3x3_thin_supported(x.shape[2], x.shape[3], cin, cout) and
                (forward_only or lib.ga_conv3x3_thin_supported(x.shape[2], x.shape[3], cout, cin)))


def conv3x3_thin_packed_weights(weight, transpose_flip):
    """ga_conv3x3_thin_pack of a (Cout, Cin, 3, 3) weight, cached per (storage, version) like conv3x3_packed_weights."""
    key = (weight.data_ptr(), weight._version, weight.dtype, bool(transpose_flip), tuple(weight.stride()), tuple(weight.shape))
    entry = _thin_pack_cache.get(key)
    hit = entry[1] if entry is not None and entry[0]() is weight else None
    if hit is None:
        require_cuda(weight)
        Cout, Cin = weight.shape[0], weight.shape[1]
        hit = torch.empty(int(load().ga_conv3x3_thin_packed_elems(Cout, Cin)), dtype=weight.dtype, device=weight.device)
        so, si, sy, sx = weight.stride()
        check(load().ga_conv3x3_thin_pack(_ptr(weight), _ptr(hit), Cout, Cin, so, si, sy, sx, int(bool(transpose_flip)),
                                          dtype_code(weight), stream_ptr()), "ga_conv3x3_thin_pack")
        if len(_thin_pack_cache) > 64:   # graphs read the packs by raw pointer: only a dead weight's entry may go
            for dead in [k for k, (ref, _) in _thin_pack_cache.items() if ref() is None]:
                del _thin_pack_cache[dead]
        _thin_pack_cache[key] = (weakref.ref(weight), hit)
    return keep_alive(hit)


def conv3x3_thin(x, wp, cout, bias=None):
    """x (B, 4, H, W) dense NCHW -> (B, cout, H, W) channels-last, or x (B, C, H, W) channels-last -> (B, 4, H, W) dense NCHW
    (cout == 4); wp from conv3x3_thin_packed_weights."""
    require_cuda(x, wp, bias)
    B, Cin, H, W = x.shape
    if bias is not None:
        bias = bias.to(x.dtype).contiguous()
    if Cin == 4:
        x = x.contiguous()
        y = torch.empty((B, cout, H, W), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
        _count(("conv3x3_thin_in", B, 4, H * W, 1, cout, bias is not None, str(x.dtype)))
        check(load().ga_conv3x3_thin_in(_ptr(x), _ptr(wp), _ptr(bias), _ptr(y), B, H, W, cout, dtype_code(x), stream_ptr()),
              "ga_conv3x3_thin_in")
        return y
    if cout != 4:
        raise GaError(f"conv3x3_thin serves 4 -> C and C -> 4 channels, got {Cin} -> {cout}")
    x = _nhwc(x)
    y = torch.empty((B, 4, H, W), dtype=x.dtype, device=x.device)
    _count(("conv3x3_thin_out", B, Cin, H * W, 1, 4, bias is not None, str(x.dtype)))
    check(load().ga_conv3x3_thin_out(_ptr(x), _ptr(wp), _ptr(bias), _ptr(y), B, H, W, Cin, dtype_code(x), stream_ptr()),
          "ga_conv3x3_thin_out")
    return y


class Conv3x3Thin(torch.autograd.Function):
    """y = conv2d(x, weight, bias, padding=1) for the UNet's conv_in / conv_out.  Differentiable w.r.t. x: the adjoint of the
    4 -> C kernel is the C -> 4 kernel on the transposed, mirrored pack and the other way round; the weights are frozen."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        if ctx.needs_input_grad[1] or (bias is not None and ctx.needs_input_grad[2]):
            raise GaError("convolution weight gradients are not part of the guided-attention path (frozen UNet)")
        ctx.weight = weight
        return conv3x3_thin(x, conv3x3_thin_packed_weights(weight, False), weight.shape[0], bias)

    @staticmethod
    def backward(ctx, gy):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        weight = ctx.weight
        return conv3x3_thin(gy, conv3x3_thin_packed_weights(weight, True), weight.shape[1]), None, None


def conv3x3_thin_apply(x, weight, bias=None):
    return Conv3x3Thin.apply(x, weight, bias)


conv3x3_thin_apply.supported = conv3x3_thin_supported


# --------------------------------------------------------------------------------------- tiled self-attention
def _sub_ptr(t, elem_offset):
    return ctypes.c_void_p(t.data_ptr() + elem_offset * t.element_size())


def _qkv_slices(q, k, v):
    """True when q, k, v are the three column slices, in this order, of ONE contiguous (B, N, 3C) tensor."""
    B, N, C = q.shape
    es = q.element_size()
    return all(tuple(t.shape) == (B, N, C) and tuple(t.stride()) == (N * 3 * C, 3 * C, 1) for t in (q, k, v)) and \
        k.data_ptr() == q.data_ptr() + C * es and v.data_ptr() == q.data_ptr() + 2 * C * es


def _self_attn_operands(q, k=None, v=None, in_place=False):
    """q, k, v as the flash kernels take them -> ((q, k, v pointers), row stride in elements (0 = dense rows of C), C, the
    tensors the pointers read).  Either three (B, N, C) tensors, made contiguous — `in_place`: unless they are the column
    slices of one (B, N, 3C) tensor, which are read where they lie — or, with k = v = None, ONE (B, N, 3C) tensor [q | k | v]
    (the output of a fused QKV projection), read in place with row stride 3C."""
    if k is None:
        qkv = q.contiguous()
        C = qkv.shape[2] // 3
        return (_sub_ptr(qkv, 0), _sub_ptr(qkv, C), _sub_ptr(qkv, 2 * C)), 3 * C, C, (qkv,)
    C = q.shape[2]
    if in_place and _qkv_slices(q, k, v):
        return (_ptr(q), _ptr(k), _ptr(v)), 3 * C, C, (q, k, v)
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    return (_ptr(q), _ptr(k), _ptr(v)), 0, C, (q, k, v)


def _probs_out(out, shape, like):
    if out is None:
        return torch.empty(shape, dtype=like.dtype, device=like.device)
    if tuple(out.shape) != tuple(shape) or out.dtype != like.dtype or out.device != like.device or not out.is_contiguous():
        raise GaError(f"out must be a contiguous {tuple(shape)} {like.dtype} tensor on {like.device}")
    return out


def _self_attn_fwd(q, k, v, heads, scale, want_lse, want_probs=False, out=None):
    """The one forward launch, operands as _self_attn_operands takes them -> (o (B,N,C), lse (B*heads,N) f32 log2-domain or
    None, probs (B*heads,N,N) or None, the operand tensors as read).  With `want_probs` (which needs the lse) it is the flash
    forward, then the probabilities from its row statistic (ga_self_attn_capture_fwd), written to `out` when given."""
    require_cuda(q, k, v)
    ptrs, ld, C, read = _self_attn_operands(q, k, v)
    B, N = q.shape[:2]
    o = torch.empty((B, N, C), dtype=q.dtype, device=q.device)
    lse = torch.empty((B * heads, N), dtype=torch.float32, device=q.device) if want_lse else None
    dims = (B, heads, N, C // heads, ld, float(scale), dtype_code(q), stream_ptr())
    if want_probs:
        probs = _probs_out(out, (B * heads, N, N), q)
        _count(("self_attn_capture_fwd", B, heads, N, N, C // heads, True, str(q.dtype)))
        check(load().ga_self_attn_capture_fwd(*ptrs, _ptr(o), _ptr(lse), _ptr(probs), *dims), "ga_self_attn_capture_fwd")
        return o, lse, probs, read
    _count(("self_attn_fwd", B, heads, N, N, C // heads, bool(want_lse), str(q.dtype)))
    check(load().ga_self_attn_fwd(*ptrs, _ptr(o), _ptr(lse), *dims), "ga_self_attn_fwd")
    return o, lse, None, read


def self_attn_fwd(q, k, v, heads, scale, want_lse=True):
    """q,k,v (B,N,C) projections -> (o (B,N,C), lse (B*heads,N) f32 log2-domain or None)."""
    return _self_attn_fwd(q, k, v, heads, scale, want_lse)[:2]


def self_attn_capture_fwd(q, k, v, heads, scale, out=None):
    """q,k,v (B,N,C) projections -> (o (B,N,C), lse (B*heads,N) f32 log2-domain, probs (B*heads,N,N) in q's dtype: the
    reference's layout, head-major batch).  `out`: where the probabilities go (contiguous, any element alignment)."""
    return _self_attn_fwd(q, k, v, heads, scale, True, True, out)[:3]


def self_attn_probs(q, k, lse, heads, scale, out=None):
    """The probabilities alone, from the lse a flash forward of the same q, k, scale left (ga_self_attn_probs)."""
    require_cuda(q, k, lse)
    q, k = q.contiguous(), k.contiguous()
    B, N, C = q.shape
    probs = _probs_out(out, (B * heads, N, N), q)
    _count(("self_attn_probs", B, heads, N, N, C // heads, True, str(q.dtype)))
    check(load().ga_self_attn_probs(_ptr(q), _ptr(k), _ptr(lse), _ptr(probs), B, heads, N, C // heads, 0, float(scale),
                                    dtype_code(q), stream_ptr()), "ga_self_attn_probs")
    return probs


def _probs_cotangent(d_probs, B, heads, N, like):
    """How a cotangent on the (B*heads, N, N) probabilities goes to ga_self_attn_bwd_dp: (tensor, map stride in elements).  No
    copy for a contiguous tensor of the kernels' dtype, nor for ONE (N, N) map expanded over the head-maps (strides (0, N, 1),
    what AggregateMaps.backward sends): that one goes with stride 0.  Anything else is made contiguous once."""
    if tuple(d_probs.shape) != (B * heads, N, N):
        raise GaError(f"d_probs must be {(B * heads, N, N)}, got {tuple(d_probs.shape)}")
    require_cuda(d_probs)
    if d_probs.dtype == like.dtype and d_probs.device == like.device:
        if d_probs.is_contiguous():
            return d_probs, N * N
        if tuple(d_probs.stride()) == (0, N, 1):
            return d_probs, 0
    return d_probs.to(device=like.device, dtype=like.dtype).contiguous(), N * N


def self_attn_bwd(q, k, v, o, d_o, lse, heads, scale, d_probs=None, out=None):
    """The one backward launch -> dq, dk, dv of the flash forward (ga_self_attn_bwd).  q, k, v may be the column slices of one
    fused (B, N, 3C) projection, read in place.
    d_probs: a cotangent on the probabilities (B*heads, N, N) the capture forward wrote -> ga_self_attn_bwd_dp; d_o may then be
    None (the loss read the maps only).
    `out`: (dq, dk, dv) to write, laid out as q, k, v are (the slices of one (B, N, 3C) tensor for the fused form).  Nothing is
    read on the host and nothing synchronises: the call can be captured."""
    require_cuda(q, k, v, o, d_o, lse)
    ptrs, ld, C, _read = _self_attn_operands(q, k, v, in_place=True)
    B, N = q.shape[:2]
    if d_o is not None:
        d_o = d_o.contiguous()
    if out is None:
        out = torch.empty((B, N, 3 * C), dtype=q.dtype, device=q.device).split(C, dim=-1) if ld else \
            tuple(torch.empty((B, N, C), dtype=q.dtype, device=q.device) for _ in range(3))
    elif bool(ld) != _qkv_slices(*out) or not (ld or all(t.is_contiguous() for t in out)):
        raise GaError("out must be laid out as q, k, v are")
    dq, dk, dv = out
    delta = torch.empty_like(lse)
    dims = (B, heads, N, C // heads, ld, float(scale), dtype_code(q), stream_ptr())
    if d_probs is None:
        _count(("self_attn_bwd", B, heads, N, N, C // heads, True, str(q.dtype)))
        check(load().ga_self_attn_bwd(*ptrs, _ptr(o), _ptr(d_o), _ptr(lse), _ptr(delta), _ptr(dq), _ptr(dk), _ptr(dv), *dims),
              "ga_self_attn_bwd")
        return dq, dk, dv
    dp, stride = _probs_cotangent(d_probs, B, heads, N, q)
    rowdot = torch.empty_like(lse)
    _count(("self_attn_bwd_dp", B, heads, N, N, C // heads, d_o is not None, str(q.dtype)))
    check(load().ga_self_attn_bwd_dp(*ptrs, _ptr(o if d_o is not None else None), _ptr(d_o), _ptr(dp), stride, _ptr(lse),
                                     _ptr(delta), _ptr(rowdot), _ptr(dq), _ptr(dk), _ptr(dv), *dims), "ga_self_attn_bwd_dp")
    return dq, dk, dv


class _SelfAttention(torch.autograd.Function):
    """(capture, heads, scale, *operands) -> (o, probs): softmax(scale q k^T) v for long key sequences, operands = q, k, v
    (B, N, C) or ONE fused (B, N, 3C) tensor, whose gradient is then one (B, N, 3C) tensor dq | dk | dv too.
    Without `capture` the probabilities are never materialised (probs is None), and a forward whose inputs need no gradient
    asks for no lse and saves nothing.  With it, probs (B*heads, N, N) comes from the forward's row statistic and is a
    differentiable output that is NOT kept for the backward: a cotangent on it goes to ga_self_attn_bwd_dp, which recomputes P
    as the flash backward does; either cotangent may be missing."""

    @staticmethod
    def forward(ctx, capture, heads, scale, *operands):
        if capture:
            ctx.set_materialize_grads(False)
        need = any(ctx.needs_input_grad[3:])
        o, lse, probs, read = _self_attn_fwd(*operands, *(None,) * (3 - len(operands)), heads, scale, capture or need, capture)
        if need:
            ctx.save_for_backward(*read, o, lse)
        ctx.meta = (heads, scale, len(operands))
        return o, probs

    @staticmethod
    def backward(ctx, d_o, d_probs):
        heads, scale, n = ctx.meta
        if d_o is None and d_probs is None:
            return (None,) * (3 + n)
        *read, o, lse = ctx.saved_tensors
        if n == 3:
            return (None, None, None) + tuple(self_attn_bwd(*read, o, d_o, lse, heads, scale, d_probs))
        C = o.shape[2]
        d_qkv = torch.empty_like(read[0])
        self_attn_bwd(*read[0].split(C, dim=-1), o, d_o, lse, heads, scale, d_probs, out=d_qkv.split(C, dim=-1))
        return None, None, None, d_qkv


class SelfAttention:
    """(q, k, v, heads, scale) -> o: softmax(scale q k^T) v for long key sequences; the probabilities are never materialised."""

    @staticmethod
    def apply(q, k, v, heads, scale):
        return _SelfAttention.apply(False, heads, scale, q, k, v)[0]


class SelfAttentionFusedQKV:
    """(qkv, heads, scale) -> o.  The same kernels on ONE (B, N, 3C) tensor [q | k | v] (the output of a fused QKV projection):
    they read the three column slices in place (row stride 3C) and the backward writes dq | dk | dv into one (B, N, 3C)
    tensor, so the projection's backward is a single GEMM too."""

    @staticmethod
    def apply(qkv, heads, scale):
        return _SelfAttention.apply(False, heads, scale, qkv)[0]


class SelfAttentionCapture:
    """SelfAttention that also returns the probabilities (B*heads, N, N): (q, k, v, heads, scale) -> (o, probs)."""

    @staticmethod
    def apply(q, k, v, heads, scale):
        return _SelfAttention.apply(True, heads, scale, q, k, v)


class SelfAttentionCaptureFusedQKV:
    """SelfAttentionFusedQKV that also returns the probabilities: (qkv (B, N, 3C), heads, scale) -> (o, probs)."""

    @staticmethod
    def apply(qkv, heads, scale):
        return _SelfAttention.apply(True, heads, scale, qkv)


def self_attention_supported(q, heads, channels=None):
    d = (channels or q.shape[-1]) // heads
    return q.is_cuda and d % 8 == 0 and d <= (80 if q.dtype == torch.float32 else 160) and q.dtype in _lib.DTYPE_CODE


# --------------------------------------------------------------------------------------- wide heads, forward only (VAE mid block)
def attn_wide_supported(q, heads, channels=None):
    """ga_attn_wide_fwd (csrc/attn_wide.hip): 16-bit, head sizes 64 ... 512 in steps of 64."""
    c = channels or q.shape[-1]
    d = c // heads
    return q.is_cuda and q.dtype in (torch.float16, torch.bfloat16) and c % heads == 0 and d % 64 == 0 and 64 <= d <= 512


def attn_wide_fwd(q, k=None, v=None, heads=1, scale=None):
    """q, k, v (B, N, C) projections, or ONE fused (B, N, 3C) tensor [q | k | v] with k = v = None (read in place, as
    _self_attn_operands does) -> o (B, N, C) = softmax(scale q k^T) v per head.  No lse, no autograd: the decoder's forward."""
    require_cuda(q, k, v)
    ptrs, ld, C, _read = _self_attn_operands(q, k, v)
    B, N = q.shape[:2]
    if scale is None:
        scale = (C // heads) ** -0.5
    o = torch.empty((B, N, C), dtype=q.dtype, device=q.device)
    _count(("attn_wide_fwd", B, heads, N, N, C // heads, False, str(q.dtype)))
    check(load().ga_attn_wide_fwd(*ptrs, _ptr(o), B, heads, N, C // heads, ld, float(scale), dtype_code(q), stream_ptr()),
          "ga_attn_wide_fwd")
    return o


def latent_affine4(x, weight, bias, pre_scale):
    """out = conv1x1(pre_scale * x) for a 4 -> 4 channel 1x1 convolution on dense NCHW latents (B, 4, H, W): the VAE decode's
    `latents / scaling_factor` and post_quant_conv in one launch (ga_latent_affine4).  weight (4, 4[, 1, 1]), bias (4,)."""
    require_cuda(x, weight, bias)
    if x.dim() != 4 or x.shape[1] != 4 or weight.numel() != 16 or bias.numel() != 4:
        raise GaError(f"latent_affine4 takes (B, 4, H, W) latents and a 4 -> 4 1x1 convolution, got {tuple(x.shape)}, "
                      f"{tuple(weight.shape)}")
    x = x.contiguous()
    w = weight.to(x.dtype).reshape(4, 4).contiguous()
    b = bias.to(x.dtype).contiguous()
    out = torch.empty_like(x)
    B, _, H, W = x.shape
    _count(("latent_affine4", B, 4, H * W, 0, 4, True, str(x.dtype)))
    check(load().ga_latent_affine4(_ptr(x), _ptr(w), _ptr(b), float(pre_scale), _ptr(out), B, H * W, dtype_code(x),
                                   stream_ptr()), "ga_latent_affine4")
    return out


# --------------------------------------------------------------------------------------- Linear layers with folded neighbours
_lin_ws = {}        # (device index, stream) -> {"slabs": f32 tensor, "tickets": int32 tensor}; never freed (captured graphs hold the pointers)
_lin_plan_cache = {}
_lin_plan_table = None
LIN_SLAB_FLOATS = 64 * 2 ** 20     # 256 MB of split-K slabs per device (of 288 GB), allocated once (outside any capture)
LIN_TICKETS = 1 << 16


def linear_workspace(device):
    """The split-K scratch of the CURRENT stream on `device`: slices of one launch hand their partial tiles to the last arriver
    through it, and two launches may only share it under stream order — so every stream that launches gets its own (the
    header's "stream-ordered use" made structural: the default stream, the one side stream of warm-ups / captures / micro-replays,
    a GUI thread's stream never meet in one slab or ticket array)."""
    key = _stream_key(device)
    ws = _lin_ws.get(key)
    if ws is None:
        if torch.cuda.is_current_stream_capturing():
            raise GaError("the Linear workspace must exist before a hipGraph capture (call ops.prepare_device first)")
        ws = _lin_ws[key] = {"slabs": torch.empty(LIN_SLAB_FLOATS, dtype=torch.float32, device=device),
                             "tickets": torch.zeros(LIN_TICKETS, dtype=torch.int32, device=device)}
    return ws


def _check_ticketed(rc, what, tickets):
    """check() for a launch that takes arrival tickets: a launch that failed after some slices had arrived would leave its
    ticket words non-zero, and every later launch on those tiles would never see a last arriver (Y silently unwritten) —
    return them to zero before raising."""
    if rc != 0 and tickets is not None and not torch.cuda.is_current_stream_capturing():
        tickets.zero_()
    check(rc, what)


def tickets_are_zero(device=None):
    """True when every arrival-ticket word of every stream's scratch on `device` is zero (what every completed launch leaves;
    synchronises).  GraphRunner.release asserts it."""
    torch.cuda.synchronize(device)
    idx = torch.device(device).index if device is not None else torch.cuda.current_device()
    words = ([ws["tickets"] for (d, _), ws in _lin_ws.items() if d == idx] + [t for (d, _), t in _tickets.items() if d == idx]
             + [t for (d, _), t in _image_tickets.items() if d == idx])
    return all(int(w.abs().sum().item()) == 0 for w in words)


def splitk_workspace(device, M, N, bm, bn, splits):
    """(f32 slabs, tickets) of an in-launch split-K reduction from the persistent per-device scratch, or (None, None)."""
    if splits <= 1:
        return None, None
    ws = linear_workspace(device)
    need = int(load().ga_splitk_workspace_floats(M, N, bm, bn, splits))
    if need > ws["slabs"].numel() or -(-M // bm) * -(-N // bn) > ws["tickets"].numel():
        raise GaError(f"split-K workspace too small: M={M} N={N} plan {(bm, bn, splits)} needs {need} floats")
    return ws["slabs"], ws["tickets"]


def prepare_device(device, stream=None):
    """Allocate the persistent scratch of the kernels (split-K slabs, arrival tickets) for the current stream (or `stream`) on
    `device` — before any hipGraph capture on that stream: captured launches keep these never-moving buffers."""
    device = torch.device(device)
    if device.type == "cuda":
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if stream is not None:
            with torch.cuda.stream(stream):
                linear_workspace(device)
                _ticket(device)
                _ticket(device, per_image=True)
        else:
            linear_workspace(device)
            _ticket(device)
            _ticket(device, per_image=True)


def _measured_linear_plans():
    global _lin_plan_table
    if _lin_plan_table is None:
        import json
        from pathlib import Path
        path = Path(__file__).resolve().parent / "linear_plans.json"
        _lin_plan_table = {}
        if path.exists():
            for k, v in json.loads(path.read_text()).items():
                _lin_plan_table[tuple(int(x) for x in k.split(","))] = tuple(v)
    return _lin_plan_table


def library_block(M, C):
    """True when tools/linear_tune.py measured the LIBRARY form of a whole transformer block (hipBLASLt GEMMs + the separate
    LayerNorm / GEGLU / residual kernels) faster than the folded ga_linear_fused form at M tokens x C channels — the long, wide
    GEMMs of SDXL's 1280-channel level at batch 3 (K = 1280 - 5120, N up to 10240); key "M,C,-1,-1" of linear_plans.json."""
    return bool(_measured_linear_plans().get((int(M), int(C), -1, -1), (0,))[0])


LINEAR_STREAM = _lib.GA_LINEAR_STREAM     # `stages` value of the persistent one-workgroup-per-CU form (csrc/linear.hip)
LINEAR_STREAM_PLAN = (128, 128, 1, LINEAR_STREAM)


def linear_stream_serves(K, parts, ln, bias, residual, want_preact, want_ln_stats, want_row_partials):
    """What linear_stream_kernel takes: the LayerNorm-folded no-grad forms (optionally GEGLU) at K >= 320."""
    return (ln is not None and bias is None and residual is None and not want_preact and not want_ln_stats
            and not want_row_partials and K // 64 >= 5 and 2 <= parts <= 20)


def linear_plan(M, K, N, geglu=False, stream_ok=False):
    """(bm, bn, splits[, stages]) for Y[M][N or N/2] = X[M][K] W[N][K]^T: the measured table (tools/linear_tune.py) or a rule:
    about one workgroup per CU and more; the depth is split when the tiles alone leave most of the chip idle.  stream_ok: the
    call is one linear_stream_kernel serves — the table's "M,K,N,geglu,8" entry says whether that form measured faster."""
    key = (int(M), int(K), int(N), int(bool(geglu)))
    if stream_ok and _measured_linear_plans().get(key + (LINEAR_STREAM,), (0,))[0]:
        return LINEAR_STREAM_PLAN
    plan = _lin_plan_cache.get(key)
    if plan is None:
        plan = _measured_linear_plans().get(key)
        if plan is None:
            n_out = N // 2 if geglu else N
            steps = K // 64
            best, best_cost = None, None
            for bm, bn in ((128, 128), (128, 64), (64, 128), (64, 64)):
                outc = bn // 2 if geglu else bn
                tiles = -(-M // bm) * -(-n_out // outc)
                waste = (-(-M // bm) * bm) * (-(-n_out // outc) * outc) / (M * n_out)
                for sp in (1, 2, 3, 4, 6, 8, 12, 16):
                    if sp > 1 and (steps // sp < 4 or sp * tiles * bm * bn > LIN_SLAB_FLOATS or tiles > LIN_TICKETS):
                        break     # too shallow a slice, or more slabs / tickets than the persistent scratch holds
                    wgs = tiles * sp
                    rounds = -(-wgs // 256)
                    per_wg = -(-steps // sp) * (0.09 if bm * bn == 128 * 128 else 0.055 if bm * bn == 128 * 64 else 0.04)
                    cost = rounds * (1.2 + per_wg) * waste ** 0.5 + (1.5 + sp * bm * bn * 4 / 100e3 if sp > 1 else 0.0)
                    if best_cost is None or cost < best_cost:
                        best, best_cost = (bm, bn, sp), cost
            plan = best
        _lin_plan_cache[key] = plan
    return plan


def linear_fused(x, weight, bias=None, residual=None, geglu=False, want_preact=False, ln=None, want_ln_stats=False,
                 want_row_partials=False, plan=None, out=None, gn=None):
    """Y = epilogue(X W^T) through ga_linear_fused (see include/ga_hip.h).
    x (..., K): rows `x.stride(-2)` elements apart, last dimension contiguous; weight (N, K) contiguous.
    ln = (partials (M, parts, 2) f32, colsum (N,) f32, shift (N,) f32, eps): LayerNorm folded in front (then `weight` is
    gamma o W and `bias` is ignored).  gn = (groups, hw): the rows are hw pixels per image and the epilogue also leaves the
    GroupNorm statistics of the stored result for the norm that consumes it ("gn": (partials, blocks), or None where the plan
    or shape does not serve).  -> dict(y, preact, ln_stats, row_partials, parts, gn)."""
    require_cuda(x, weight, bias, residual)
    if x.stride(-1) != 1 or not weight.is_contiguous():
        raise GaError("linear_fused needs unit-stride feature axes")
    K = x.shape[-1]
    lead = x.shape[:-1]
    M = 1
    for d in lead:
        M *= d
    ldx = x.stride(-2) if x.dim() > 1 else K
    if x.dim() > 2 and any(x.stride(i) != x.stride(i + 1) * x.shape[i + 1] for i in range(x.dim() - 2)):
        x = x.contiguous()
        ldx = K
    N = weight.shape[0]
    n_out = N // 2 if geglu else N
    if plan is None:
        stream_ok = ln is not None and linear_stream_serves(K, ln[0].shape[1], ln, bias, residual, want_preact, want_ln_stats,
                                                            want_row_partials)
        plan = linear_plan(M, K, N, geglu, stream_ok)
    plan = tuple(plan)
    bm, bn, splits = plan[:3]
    stages = plan[3] if len(plan) > 3 else 0
    y = out if out is not None else torch.empty(lead + (n_out,), dtype=x.dtype, device=x.device)
    ep = _lib.ga_linear_epilogue_t()
    ep.bias = bias.data_ptr() if bias is not None else None
    if residual is not None:
        if residual.stride(-1) != 1 or tuple(residual.shape) != tuple(y.shape):
            raise GaError("residual must have the result's shape and a unit-stride feature axis")
        if residual.dim() > 2 and any(residual.stride(i) != residual.stride(i + 1) * residual.shape[i + 1]
                                      for i in range(residual.dim() - 2)):
            residual = residual.contiguous()
        ep.residual, ep.ld_res = residual.data_ptr(), residual.stride(-2) if residual.dim() > 1 else n_out
    ep.geglu = int(bool(geglu))
    preact = None
    if geglu and want_preact:
        preact = torch.empty(lead + (N,), dtype=x.dtype, device=x.device)
        ep.preact, ep.ld_pre = preact.data_ptr(), N
    ln_stats = None
    if ln is not None:
        partials, colsum, shift, eps = ln
        if partials.dtype != torch.float32 or tuple(partials.shape) != (M, partials.shape[1], 2) or not partials.is_contiguous():
            raise GaError("LayerNorm partial sums must be a contiguous (M, parts, 2) float32 tensor")
        ep.ln_partials, ep.ln_parts, ep.ln_eps = partials.data_ptr(), partials.shape[1], float(eps)
        ep.ln_colsum, ep.ln_shift = colsum.data_ptr(), shift.data_ptr()
        if want_ln_stats:
            ln_stats = torch.empty((M, 2), dtype=torch.float32, device=x.device)
            ep.ln_stats_out = ln_stats.data_ptr()
    outc = bn // 2 if geglu else bn
    parts = -(-n_out // outc)
    row_partials = None
    if want_row_partials:
        row_partials = torch.empty((M, parts, 2), dtype=torch.float32, device=x.device)
        ep.row_partials_out = row_partials.data_ptr()
    gn_made = None
    if gn is not None and not geglu and stages != LINEAR_STREAM:
        groups, hw = gn
        blocks = int(load().ga_linear_gn_blocks(hw, N, groups, bm, bn)) if M % hw == 0 else 0
        if blocks:
            gn_partials = torch.empty((M // hw, blocks, groups, 2), dtype=torch.float32, device=x.device)
            ep.gn_partials, ep.gn_groups, ep.gn_hw = gn_partials.data_ptr(), groups, hw
            gn_made = (gn_partials, blocks)
    slabs = tickets = None
    if splits > 1:
        ws = linear_workspace(x.device)
        tiles = -(-M // bm) * parts
        if splits * tiles * bm * bn > ws["slabs"].numel() or tiles > ws["tickets"].numel():
            raise GaError(f"split-K workspace too small for M={M} N={N} plan {(bm, bn, splits)}")
        slabs, tickets = ws["slabs"], ws["tickets"]
    _count(("linear", M, K, 0, int(bool(geglu)) + 2 * int(ln is not None) + 4 * int(residual is not None), N, bias is not None,
            str(x.dtype)))
    _check_ticketed(load().ga_linear_fused(_ptr(x), ldx, _ptr(weight), _ptr(y), y.stride(-2) if y.dim() > 1 else n_out,
                                           ctypes.byref(ep), _ptr(slabs), _ptr(tickets), M, K, N, bm, bn, splits, stages,
                                           dtype_code(x), stream_ptr()), "ga_linear_fused", tickets)
    return {"y": y, "preact": preact, "ln_stats": ln_stats, "row_partials": row_partials, "parts": parts, "gn": gn_made}
