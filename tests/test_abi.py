"""CPU-side checks of the C ABI: the library loads, exports every symbol include/ga_hip.h declares,
and its host-only entry points behave.  No kernels are launched here."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from conftest import ROOT, load_npz

HEADER = ROOT / "include" / "ga_hip.h"


def declared_functions():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(ga_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    from guided_attention_amd import _lib
    if not _lib.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_header_and_binding_agree():
    from guided_attention_amd import _lib
    assert declared_functions() == sorted(_lib.PROTOTYPES)


def test_every_declared_symbol_is_exported(lib):
    names = declared_functions()
    assert len(names) >= 11
    for n in names:
        assert hasattr(lib, n), n


def test_no_kernel_uses_scratch_memory(lib):
    """Code-object metadata of every gfx950 kernel in the library: no private segment (a per-lane stack array the
    compiler failed to keep in registers is scratch-memory traffic in the inner loop — round 2 shipped eight bf16
    self-attention kernels with 64 bytes of it) and no spilled vector registers."""
    import sys
    sys.path.insert(0, str(ROOT / "tools"))
    import code_object_check
    from guided_attention_amd import _lib
    ks = code_object_check.kernels(_lib.LIB_PATH)
    assert len(ks) > 300, len(ks)
    assert any("self_attn_fwd_kernel" in k["name"] for k in ks) and any("conv3x3" in k["name"] for k in ks)
    bad = [(k["name"], k.get("private_segment_fixed_size"), k.get("vgpr_spill_count")) for k in code_object_check.offenders(ks)]
    assert not bad, bad


def test_hot_kernels_request_their_operands_in_batches(lib):
    """tools/load_chain_scan.py over the built library: the kernels a UNet pass spends its time in issue their loads in
    batches.  Round 3 found most of them waiting for one load at a time (conditional loads into register arrays, operands
    loaded where they are consumed): up to 37 serial round trips per launch in the capture backward, 44 in the loss
    launch, 26 - 31 in the small-slab GroupNorm and the dQ kernel.  A new chain in one of them shows up here."""
    import sys
    sys.path.insert(0, str(ROOT / "tools"))
    import load_chain_scan
    from guided_attention_amd import _lib
    res = load_chain_scan.chains(_lib.LIB_PATH)
    assert len(res) > 300, len(res)
    limits = {   # f16 instantiations the SD-1.x passes launch: longest run of serial load steps allowed
        "linear_kernelIDF16_Li64ELi64ELi4ELb0ELb0E": 3, "linear_kernelIDF16_Li128ELi128ELi2ELb1ELb1E": 3,
        "conv3x3_patch_dma_kernelIDF16_Li128ELi64ELb1ELb0ELb1E": 3, "conv3x3_patch_dma_kernelIDF16_Li64ELi64ELb1ELb0ELb1E": 3,
        "gn_small_fwd_kernelIDF16_Lb1ELi1024ELi12ELb0E": 1, "gn_small_bwd_kernelIDF16_Lb1ELi1024ELi12E": 1,
        # the norm that also concatenates its two sources: 19 dwords of arguments, 16 are preloaded — the other three come in one
        # batch of scalar loads behind the compatibility prologue's (two scalar steps in a row, no vector load waits alone)
        "gn_small_fwd_kernelIDF16_Lb1ELi1024ELi12ELb1E": 2,
        "gn_wide_apply_kernelIDF16_Lb1E": 3, "gn_wide_bwd_apply_kernelIDF16_Lb1E": 3,   # gamma / beta land last, on purpose
        "attn_capture_fwd_kernelIDF16_Li5ELi4ELi10ELb0E": 1, "attn_capture_bwd_kernelIDF16_Li5ELi4ELi10ELb0E": 1,
        "self_attn_fwd_kernelIDF16_Li10ELi1ELi1ELi64ELb0ELi4E": 3, "self_attn_bwd_dq_kernelIDF16_Li10ELi1ELi1ELi64E": 3,
        "aggregate_loss_fwd_kernelIDF16_": 8, "add_ln_bwd_kernelIDF16_Li3E": 3,
    }
    for pat, limit in limits.items():
        hits = {k: v for k, v in res.items() if pat in k}
        assert hits, pat
        for k, (run, serial, loads) in hits.items():
            assert run <= limit, (k, run, serial, loads)


def test_version_and_strerror(lib):
    m = re.search(r"#define GA_VERSION (\d+)", HEADER.read_text())
    assert lib.ga_version() == int(m.group(1))
    from guided_attention_amd import _lib
    assert _lib.GA_VERSION == int(m.group(1))        # the binding is written for the header's version (load() refuses otherwise)
    assert lib.ga_strerror(0) == b"ok"
    assert b"NULL" in lib.ga_strerror(-1)
    assert lib.ga_strerror(-999) == b"unknown status"


def test_loader_refuses_a_library_of_another_abi_version(monkeypatch):
    """Exported signatures changed between versions by pointers inserted in the middle of argument lists (round 3: `tickets`
    behind `workspace`): a binding and a library of different versions must not meet."""
    from guided_attention_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "GA_VERSION", _lib.GA_VERSION - 10)
    with pytest.raises(_lib.GaError, match="ABI version"):
        _lib.load()


def test_struct_layout_matches_header(tmp_path):
    """The ctypes mirrors against what a C compiler makes of include/ga_hip.h (sizes and every field offset)."""
    import subprocess
    from guided_attention_amd import _lib
    assert ctypes.sizeof(_lib.ga_token_t) == 48      # 2*int32 + 4*double + 2*float
    assert ctypes.sizeof(_lib.ga_loss_params_t) == 40
    fields = {"ga_token_t": ["token", "kind", "geom", "weight"],
              "ga_loss_params_t": ["inside_scale", "outside_scale", "center_weight", "sigma", "shrink", "ksize", "smooth",
                                   "strict"],
              "ga_linear_epilogue_t": ["bias", "residual", "ld_res", "geglu", "preact", "ld_pre", "ln_partials", "ln_parts", "ln_eps",
                                       "ln_colsum", "ln_shift", "ln_stats_out", "row_partials_out", "gn_partials", "gn_groups",
                                       "gn_hw"]}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "ga_hip.h"', "int main(void) {"]
    for st, fs in fields.items():
        src.append(f'  printf("{st} %zu\\n", sizeof({st}));')
        src += [f'  printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f in fs]
    src += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-I", str(HEADER.parent), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = dict(line.split() for line in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True,
                                                       check=True).stdout.splitlines())
    for st, fs in fields.items():
        cls = getattr(_lib, st)
        assert int(out[st]) == ctypes.sizeof(cls)
        for f in fs:
            assert int(out[f"{st}.{f}"]) == getattr(cls, f).offset, (st, f)


def test_gaussian_weights_host_entry(lib):
    g = load_npz("g1_gaussian.npz")
    for k, s in [(3, 0.5), (3, 1.0), (5, 1.0), (5, 0.75)]:
        w = (ctypes.c_float * (k * k))()
        assert lib.ga_gaussian_weights(k, s, w) == 0
        np.testing.assert_allclose(np.array(w).reshape(k, k), g[f"k{k}_s{s}"], rtol=0, atol=2e-7)
    assert lib.ga_gaussian_weights(9, 0.5, (ctypes.c_float * 81)()) == -2
    assert lib.ga_gaussian_weights(3, 0.5, None) == -1


def test_argument_validation_needs_no_gpu(lib):
    # every entry point validates before touching the device: errors come back as codes
    assert lib.ga_attn_capture_fwd(None, None, None, None, None, 1, 8, 256, 77, 160, 0.1, 0, None) == -1
    assert lib.ga_latent_axpy(None, None, 1.0, None, None, 16, 0, None) == -1
    assert lib.ga_geglu_fwd(None, None, 4, 16, 0, None) == -1
    assert lib.ga_geglu_bwd(None, None, None, 4, 16, 0, None) == -1
    assert lib.ga_bias_residual_add(None, None, None, None, 4, 16, 0, None) == -1
    assert lib.ga_add_layer_norm_fwd(None, None, None, None, None, None, None, 4, 16, 1e-5, 0, None) == -1
    assert lib.ga_add_layer_norm_bwd(None, None, None, None, None, None, 4, 16, 0, None) == -1
    assert lib.ga_self_attn_fwd(None, None, None, None, None, 1, 8, 64, 40, 0, 0.1, 0, None) == -1
    assert lib.ga_group_norm_fwd(None, None, None, None, None, None, None, 1, 64, 320, 32, 1e-5, 1, 0, None) == -1
    # shape / dtype / alignment errors are told apart (host-side checks on fake, never dereferenced pointers)
    p = ctypes.c_void_p(4096)
    assert lib.ga_geglu_fwd(p, p, 4, 12, 0, None) == -2          # F = 12 fp16 is not a whole 16-byte vector
    assert lib.ga_geglu_fwd(p, p, 4, 16, 7, None) == -3          # unknown dtype
    assert lib.ga_geglu_fwd(ctypes.c_void_p(4100), p, 4, 16, 0, None) == -4
    assert lib.ga_add_layer_norm_fwd(None, p, p, p, None, p, None, 4, 8192, 1e-5, 0, None) == -2   # C > 4096
    assert lib.ga_self_attn_fwd(p, p, p, p, None, 1, 8, 64, 200, 0, 0.1, 0, None) == -2           # D > 160
    assert lib.ga_self_attn_fwd(p, p, p, p, None, 1, 8, 64, 44, 0, 0.1, 0, None) == -4            # D % 8 != 0


_SA_ENTRIES = ("fwd", "bwd", "bwd_dp", "probs", "capture_fwd")
_SA_POINTERS = {   # ga_self_attn_<entry>: its pointer arguments in order (bwd_dp: dp_map_stride follows dP)
    "fwd": ("Q", "K", "V", "O", "LSE"),
    "bwd": ("Q", "K", "V", "O", "dO", "LSE", "delta", "dQ", "dK", "dV"),
    "bwd_dp": ("Q", "K", "V", "O", "dO", "dP", "LSE", "delta", "rowdot", "dQ", "dK", "dV"),
    "probs": ("Q", "K", "LSE", "P"),
    "capture_fwd": ("Q", "K", "V", "O", "LSE", "P"),
}
_SA_ALIGNED16 = {   # the ones that must sit on a 16-byte boundary
    "fwd": ("Q", "K", "V", "O"), "bwd": ("Q", "K", "V", "O", "dO", "dQ", "dK", "dV"),
    "bwd_dp": ("Q", "K", "V", "O", "dO", "dQ", "dK", "dV"), "probs": ("Q", "K"), "capture_fwd": ("Q", "K", "V", "O"),
}
# One bad call per row (changes against a good f16 call B 1, H 8, N 64, D 40, dense rows, every pointer 4096) and the status
# of each entry, in the order of _SA_ENTRIES.  fwd and bwd look at the dtype last and take any row stride >= H D that is a
# multiple of 8; the other three look at the dtype before the shape and take ld_qkv 0 or 3 H D only.  Every row returns
# before the first runtime call — where a row's own fault would pass an entry's checks, an unknown dtype stops that entry.
_SA_STATUS = [
    (dict(D=200), (-2, -2, -2, -2, -2)),
    (dict(D=44), (-4, -4, -4, -4, -4)),
    (dict(N=0), (-2, -2, -2, -2, -2)),
    (dict(dtype=7), (-3, -3, -3, -3, -3)),
    (dict(dtype=7, D=200), (-2, -2, -3, -3, -3)),
    (dict(dtype=7, Q=0), (-1, -1, -1, -1, -1)),
    (dict(dtype=7, Q=4104), (-4, -4, -3, -3, -3)),
    (dict(D=200, Q=4104), (-2, -2, -2, -2, -2)),
    (dict(ld=328, dtype=7), (-3, -3, None, None, None)),      # H D + 8: fine for fwd / bwd, which go on to the dtype
    (dict(ld=328), (None, None, -2, -2, -2)),
    (dict(ld=312), (-2, -2, -2, -2, -2)),                     # H D - 8
    (dict(ld=324, dtype=7), (-2, -2, -3, -3, -3)),            # not a multiple of 8
    (dict(dtype=2, D=96), (None, None, -6, -6, -6)),          # f32 above head size 80
    (dict(dtype=2, D=96, ld=8), (None, None, -6, -6, -6)),
    (dict(P=4097), (None, None, None, -4, -4)),               # P / dP off their element size
    (dict(P=4098, dtype=2), (None, None, None, -4, -4)),
    (dict(dP=4097), (None, None, -4, None, None)),
    (dict(dP=4098, dtype=2), (None, None, -4, None, None)),
    (dict(stride=-1), (None, None, -2, None, None)),          # dp_map_stride: 0 or >= N N
    (dict(stride=100), (None, None, -2, None, None)),
    (dict(stride=4095), (None, None, -2, None, None)),
    (dict(stride=4095, Q=4104), (None, None, -2, None, None)),
    (dict(O=0), (-1, -1, -1, None, -1)),                      # bwd_dp: O and dO come together or not at all
    (dict(dO=0), (None, -1, -1, None, None)),
    (dict(O=0, dO=0, dtype=7), (None, -1, -3, None, None)),
    (dict(O=4104, dO=4104), (None, -4, -4, None, None)),
]


def _self_attn_status(lib, entry, **change):
    a = dict(B=1, H=8, N=64, D=40, ld=0, scale=0.1, dtype=0, stride=0)
    p = {n: 4096 for n in _SA_POINTERS[entry]}
    for k, v in change.items():
        (p if k in p else a)[k] = v
    args = [ctypes.c_void_p(p[n]) if p[n] else None for n in _SA_POINTERS[entry]]
    if entry == "bwd_dp":
        args.insert(6, a["stride"])
    return getattr(lib, "ga_self_attn_" + entry)(*args, a["B"], a["H"], a["N"], a["D"], a["ld"], a["scale"], a["dtype"], None)


def test_self_attn_and_conv_status_codes(lib):
    """Which status the five ga_self_attn_* entries and the two convolution entries return for a bad argument, and which
    error wins when two are present: taken from the library as it stood before the entries' checks came to share their
    helpers.  Fake, never dereferenced pointers; no call here reaches the device."""
    for entry, expected in zip(_SA_ENTRIES, zip(*(codes for _, codes in _SA_STATUS))):
        for (change, _), code in zip(_SA_STATUS, expected):
            if code is not None:
                assert _self_attn_status(lib, entry, **change) == code, (entry, change)
        for n in _SA_POINTERS[entry]:
            if (entry, n) != ("fwd", "LSE"):      # optional there
                assert _self_attn_status(lib, entry, **{n: 0}) == -1, (entry, n)
        for n in _SA_ALIGNED16[entry]:
            assert _self_attn_status(lib, entry, **{n: 4104}) == -4, (entry, n)
    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(4104)

    def conv(X=p, Wp=p, Y=p, ws=None, tickets=None, bias=None, residual=None, B=1, H=16, W=16, Cin=64, Cout=64, stride=1, bm=64,
             bn=64, splits=1, dtype=0, up=False):
        if up:
            return lib.ga_conv3x3_up2x_nhwc(X, Wp, Y, ws, tickets, bias, residual, B, H, W, Cin, Cout, bm, bn, splits, dtype, None)
        return lib.ga_conv3x3_nhwc(X, Wp, Y, ws, tickets, bias, residual, B, H, W, Cin, Cout, stride, bm, bn, splits, dtype, None)
    for up in (False, True):
        assert conv(Y=None, up=up) == -1 and conv(Y=None, Cin=100, up=up) == -1
        assert conv(Cin=100, up=up) == -2 and conv(Cout=12, up=up) == -2 and conv(Cin=100, X=q, up=up) == -2
        assert conv(splits=65, up=up) == -2 and conv(splits=2, ws=p, up=up) == -2     # a split needs workspace and tickets
        assert conv(X=q, up=up) == -4 and conv(bias=q, up=up) == -4 and conv(residual=q, dtype=2, up=up) == -4
        assert conv(dtype=2, up=up) == -3 and conv(dtype=2, bm=96, up=up) == -3       # 16-bit types only; the tile comes after
        assert conv(B=2048, H=128, W=128, Cin=64, up=up) == -2                        # 32-bit byte offsets
    assert conv(stride=3) == -2
    assert conv(H=2, W=2, up=True) == -2      # a 4-wide output map: no patch kernel serves it, and only that one upsamples


def test_conv_plan_is_a_host_function(lib):
    """ga_conv3x3_plan needs no device: the split-K choice prices the f32 partial slabs (a large-M shape is never split,
    a small-M deep one is), the workspace it asks for matches the plan, and argument errors come back as codes."""
    def plan(B, H, W, ci, co, st):
        bm, bn, sp, ws = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
        rc = lib.ga_conv3x3_plan(B, H, W, ci, co, st, ctypes.byref(bm), ctypes.byref(bn), ctypes.byref(sp), ctypes.byref(ws))
        return rc, bm.value, bn.value, sp.value, ws.value
    rc, bm, bn, sp, ws = plan(3, 128, 128, 320, 320, 1)          # SDXL's top level, M = 49 152
    assert rc == 0 and sp == 1 and ws == 0 and (bm, bn) in ((128, 64), (64, 64), (128, 128))
    rc, bm, bn, sp, ws = plan(1, 16, 16, 1280, 1280, 1)          # M = 256, depth 11 520: split to fill the chip
    assert rc == 0 and sp > 1 and ws == sp * 256 * 1280
    rc, bm, bn, sp, ws = plan(1, 64, 64, 320, 320, 2)            # stride 2: output 32 x 32
    assert rc == 0 and ws == (sp * 1024 * 320 if sp > 1 else 0)
    assert plan(1, 16, 16, 100, 1280, 1)[0] == -2                # Cin not a multiple of 64
    assert plan(1, 16, 16, 1280, 1280, 3)[0] == -2               # stride 3
    assert lib.ga_conv3x3_nhwc(None, None, None, None, None, None, None, 1, 16, 16, 64, 64, 1, 64, 64, 1, 0, None) == -1
    assert lib.ga_gemm_nt(None, None, None, None, None, None, None, 16, 64, 64, 64, 64, 1, 0, None) == -1
    p = ctypes.c_void_p(4096)
    assert lib.ga_gemm_nt(p, p, p, None, None, None, None, 16, 72, 64, 64, 64, 1, 0, None) == -2   # K not a multiple of 64
    assert lib.ga_conv3x3_nhwc(p, p, p, None, None, None, None, 1, 16, 16, 64, 64, 1, 96, 64, 1, 0, None) == -2   # no 96-pixel tile


def test_round4_entry_points_validate_on_the_host(lib):
    """The edge convolutions, the concatenation that takes / runs the consuming GroupNorm and the statistics-from-the-producer
    pair: which shapes they serve is a host-side answer, and argument errors come back as codes without touching a device."""
    assert lib.ga_conv3x3_thin_supported(64, 64, 4, 320) == 1 and lib.ga_conv3x3_thin_supported(64, 64, 320, 4) == 1
    assert lib.ga_conv3x3_thin_supported(96, 96, 4, 320) == 1 and lib.ga_conv3x3_thin_supported(128, 128, 320, 4) == 1
    assert lib.ga_conv3x3_thin_supported(24, 24, 4, 320) == 0          # map width not a multiple of 16
    assert lib.ga_conv3x3_thin_supported(64, 64, 8, 320) == 0          # neither side four channels wide
    assert lib.ga_conv3x3_thin_supported(64, 64, 640, 4) == 0          # more channels than the slices' registers hold
    assert lib.ga_conv3x3_thin_packed_elems(320, 4) == 36 * 320 and lib.ga_conv3x3_thin_packed_elems(4, 320) == 36 * 320
    p = ctypes.c_void_p(4096)
    assert lib.ga_conv3x3_thin_in(None, p, None, p, 1, 64, 64, 320, 0, None) == -1
    assert lib.ga_conv3x3_thin_in(p, p, None, p, 1, 64, 60, 320, 0, None) == -2
    assert lib.ga_conv3x3_thin_out(p, p, None, p, 1, 64, 64, 320, 2, None) == -3       # fp32 stays on the library
    assert lib.ga_conv3x3_thin_out(ctypes.c_void_p(4100), p, None, p, 1, 64, 64, 320, 0, None) == -4
    assert lib.ga_conv3x3_thin_pack(p, p, 320, 8, 72, 9, 3, 1, 0, 0, None) == -2        # no four-channel side
    # GroupNorm: which shapes are one launch, which two, and what the concatenation's two forms serve
    assert lib.ga_group_norm_two_launch(4096, 320, 32, 0) == 1 and lib.ga_group_norm_one_launch(4096, 320, 32, 0) == 0
    assert lib.ga_group_norm_two_launch(256, 2560, 32, 0) == 0 and lib.ga_group_norm_one_launch(256, 2560, 32, 0) == 1
    assert lib.ga_cat_channels_gn_blocks(4096, 960, 32, 0) == 128 and lib.ga_cat_channels_gn_blocks(256, 2560, 32, 0) == 0
    assert lib.ga_cat_channels_gn_blocks(4096, 960, 32, 2) == 0                          # 16-bit types only
    assert lib.ga_cat_channels_gn(p, p, p, None, 1, 4096, 640, 320, 32, 0, None) == -1
    assert lib.ga_cat_channels_gn(p, p, p, p, 1, 4096, 644, 316, 32, 0, None) == -2      # not whole 16-byte vectors
    assert lib.ga_cat_channels_gn(p, p, p, p, 1, 256, 1280, 1280, 32, 0, None) == -6     # that norm is one launch: the other form
    assert lib.ga_cat_group_norm_fwd(p, p, p, p, p, p, p, 1, 4096, 640, 320, 32, 1e-5, 1, 0, None) == -6
    assert lib.ga_cat_group_norm_fwd(p, p, None, p, p, p, p, 1, 256, 1280, 1280, 32, 1e-5, 1, 0, None) == -1
    assert lib.ga_conv3x3_gn_blocks(64, 64, 320, 32, 128, 64) == 64 and lib.ga_conv3x3_gn_blocks(16, 16, 1280, 32, 128, 64) == 4   # 2 slots x 2 m tiles


def test_product_refuses_cpu_tensors():
    import torch
    from guided_attention_amd import ops
    with pytest.raises(ops.GaError):
        ops.latent_axpy(torch.zeros(4), torch.zeros(4), 1.0)
    with pytest.raises(ops.GaError):
        ops.aggregate_maps([torch.zeros(2, 4, 4)])


def test_no_write_through_store_has_its_data_overwritten_behind_it(lib):
    """The split-K slab stores (buffer_store_dwordx4 ... sc1) must not be followed within two instructions by a VALU write to
    the registers they store: on the MI355X that pair stored the new value from a few lanes now and then (round 3,
    linear_kernel<128, 64, 3>; csrc/ga_common.h keep_live is the fix).  Reads the built library's ISA — no GPU needed."""
    import sys
    sys.path.insert(0, str(ROOT / "tools"))
    from store_hazard_scan import write_through_offenders
    from guided_attention_amd import _lib
    bad = write_through_offenders(str(_lib.LIB_PATH), window=2)
    assert not bad, "\n".join(f"{f}: {s_} ; {w}" for f, s_, w in bad[:10])
