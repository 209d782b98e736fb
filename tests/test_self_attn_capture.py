"""ga_self_attn_probs / ga_self_attn_capture_fwd and their autograd Functions: what can be checked without a device — the header
and the binding agree, the entry points validate every argument on the host before any launch, the Functions refuse CPU tensors."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

HEADER = Path(__file__).resolve().parent.parent / "include" / "ga_hip.h"
ENTRIES = {"ga_self_attn_probs": 12, "ga_self_attn_capture_fwd": 14}


@pytest.fixture(scope="module")
def lib():
    from guided_attention_amd import _lib
    if not _lib.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_header_and_binding_agree_on_the_two_entries(lib):
    from guided_attention_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    ctype_of = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "const float*": ctypes.c_void_p,
                "float*": ctypes.c_void_p, "int": ctypes.c_int, "float": ctypes.c_float, "ga_stream_t": ctypes.c_void_p}
    for name, nargs in ENTRIES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in the header"
        params = [re.sub(r"\s+\w+$", "", p.strip()) for p in m.group(1).split(",")]
        assert len(params) == nargs
        assert [ctype_of[p] for p in params] == _lib.PROTOTYPES[name], name
        assert getattr(lib, name).restype is ctypes.c_int
    # the header promises that all of P is written
    assert re.search(r"EVERY element of P is written", HEADER.read_text())


def test_arguments_are_validated_without_a_device(lib):
    p, f16, f32 = ctypes.c_void_p(4096), 0, 2
    probs = lambda Q, K, L, P, B, H, N, D, ld, dt: lib.ga_self_attn_probs(Q, K, L, P, B, H, N, D, ld, 0.1, dt, None)  # noqa: E731
    cap = lambda Q, K, V, O, L, P, B, H, N, D, ld, dt: lib.ga_self_attn_capture_fwd(Q, K, V, O, L, P, B, H, N, D, ld, 0.1, dt, None)  # noqa: E731
    # missing pointers: P and LSE are required by both entries (the second launch of the capture entry reads LSE)
    assert probs(p, p, p, None, 1, 2, 64, 40, 0, f16) == -1
    assert probs(p, p, None, p, 1, 2, 64, 40, 0, f16) == -1
    assert probs(None, p, p, p, 1, 2, 64, 40, 0, f16) == -1
    assert cap(p, p, p, p, p, None, 1, 2, 64, 40, 0, f16) == -1
    assert cap(p, p, p, p, None, p, 1, 2, 64, 40, 0, f16) == -1
    assert cap(p, p, None, p, p, p, 1, 2, 64, 40, 0, f16) == -1
    assert cap(p, p, p, None, p, p, 1, 2, 64, 40, 0, f16) == -1
    for call in (lambda *a: probs(p, p, p, p, *a), lambda *a: cap(p, p, p, p, p, p, *a)):
        assert call(1, 2, 0, 40, 0, f16) == -2            # N = 0
        assert call(0, 2, 64, 40, 0, f16) == -2           # B = 0
        assert call(1, 0, 64, 40, 0, f16) == -2           # H = 0
        assert call(1, 2, 64, 12, 0, f16) == -4           # D = 12: not a multiple of 8
        assert call(1, 2, 64, 168, 0, f16) == -2          # D > 160
        assert call(1, 2, 64, 96, 0, f32) == -6           # f32 serves D <= 80
        assert call(1, 2, 64, 40, 80, f16) == -2          # ld_qkv is 0 or 3 * H * D = 240
        assert call(1, 2, 64, 40, 248, f16) == -2
        assert call(1, 2, 64, 40, 0, 7) == -3             # unknown dtype
    assert probs(ctypes.c_void_p(4100), p, p, p, 1, 2, 64, 40, 0, f16) == -4    # Q off a 16-byte boundary
    assert probs(p, p, p, ctypes.c_void_p(4097), 1, 2, 64, 40, 0, f16) == -4    # P off its element size


def test_the_functions_refuse_cpu_tensors():
    from guided_attention_amd import ops
    from guided_attention_amd._lib import GaError
    q, k, v = (torch.zeros(1, 64, 80, requires_grad=True) for _ in range(3))
    with pytest.raises(GaError):
        ops.SelfAttentionCapture.apply(q, k, v, 2, 0.1)
    with pytest.raises(GaError):
        ops.SelfAttentionCaptureFusedQKV.apply(torch.zeros(1, 64, 240, requires_grad=True), 2, 0.1)
    with pytest.raises(GaError):
        ops.self_attn_capture_fwd(q.detach(), k.detach(), v.detach(), 2, 0.1)
    with pytest.raises(GaError):
        ops.self_attn_probs(q.detach(), k.detach(), torch.zeros(2, 64), 2, 0.1)
