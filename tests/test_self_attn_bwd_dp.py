"""ga_self_attn_bwd_dp (the flash backward with a cotangent on the stored self-attention probabilities) and its host layer: what
can be checked without a device — the header and the binding agree, the entry validates every argument on the host before any
launch, the operator refuses CPU tensors, the framework restatement of the branch is gone."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

HEADER = Path(__file__).resolve().parent.parent / "include" / "ga_hip.h"
NAME = "ga_self_attn_bwd_dp"
# Q K V O dO | dP dp_map_stride | LSE delta rowdot | dQ dK dV | B H N D ld_qkv | scale dtype stream: ga_self_attn_bwd's 18
# parameters and the three new ones
NARGS = 21


@pytest.fixture(scope="module")
def lib():
    from guided_attention_amd import _lib
    if not _lib.LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_header_and_binding_agree_on_the_entry(lib):
    from guided_attention_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    ctype_of = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "const float*": ctypes.c_void_p,
                "float*": ctypes.c_void_p, "int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
                "ga_stream_t": ctypes.c_void_p}
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{NAME} is not declared in the header"
    params = [re.sub(r"\s+\w+$", "", p.strip()) for p in m.group(1).split(",")]
    assert len(params) == NARGS
    assert params[6] == "int64_t" and _lib.PROTOTYPES[NAME][6] is ctypes.c_int64      # dp_map_stride
    assert [ctype_of[p] for p in params] == _lib.PROTOTYPES[NAME]
    assert hasattr(lib, NAME) and getattr(lib, NAME).restype is ctypes.c_int
    # the header promises complete outputs
    assert re.search(r"EVERY element of dQ, dK, dV, delta and rowdot is written", HEADER.read_text())


def test_version_number_is_kept(lib):
    from guided_attention_amd import _lib
    m = re.search(r"#define GA_VERSION (\d+)", HEADER.read_text())
    assert int(m.group(1)) == 183 and _lib.GA_VERSION == 183 and lib.ga_version() == 183
    assert re.search(r"183\s+0\.1\.16 \(number kept", HEADER.read_text())


def test_arguments_are_validated_without_a_device(lib):
    p, f16, f32 = ctypes.c_void_p(4096), 0, 2

    def call(Q=p, K=p, V=p, O=p, dO=p, dP=p, stride=0, LSE=p, delta=p, rowdot=p, dQ=p, dK=p, dV=p, B=1, H=2, N=64, D=40, ld=0,
             dt=f16):
        return lib.ga_self_attn_bwd_dp(Q, K, V, O, dO, dP, stride, LSE, delta, rowdot, dQ, dK, dV, B, H, N, D, ld, 0.1, dt, None)

    # missing pointers
    assert call(dP=None) == -1
    assert call(rowdot=None) == -1
    assert call(dQ=None) == -1
    assert call(delta=None) == -1 and call(LSE=None) == -1 and call(V=None) == -1
    assert call(dO=None) == -1 and call(O=None) == -1            # one of the pair without the other
    # dO and O both missing is a form of the call: it gets past the NULL check and stops at the next wrong argument
    assert call(dO=None, O=None, N=0) == -2
    assert call(dO=None, O=None, stride=-1) == -2
    # the map stride: 0 (one shared map) or at least N * N
    assert call(stride=-1) == -2
    assert call(stride=64 * 64 - 1) == -2
    assert call(stride=1) == -2
    # as for ga_self_attn_bwd
    assert call(ld=80) == -2 and call(ld=248) == -2              # ld_qkv is 0 or 3 * H * D = 240
    assert call(D=44) == -4                                      # not a multiple of 8
    assert call(D=200) == -2                                     # D > 160
    assert call(D=96, dt=f32) == -6                              # f32 serves D <= 80
    assert call(B=0) == -2 and call(H=0) == -2 and call(N=0) == -2
    assert call(dt=7) == -3
    assert call(Q=ctypes.c_void_p(4100)) == -4                   # Q off a 16-byte boundary
    assert call(dO=ctypes.c_void_p(4100)) == -4
    assert call(dP=ctypes.c_void_p(4097)) == -4                  # dP off its element size
    assert call(dP=ctypes.c_void_p(4098), stride=-1) == -2       # ... which is all the alignment it needs


def test_the_operator_refuses_cpu_tensors():
    from guided_attention_amd import ops
    from guided_attention_amd._lib import GaError
    q, k, v, o = (torch.zeros(1, 64, 80) for _ in range(4))
    lse, d_probs = torch.zeros(2, 64), torch.zeros(2, 64, 64)
    with pytest.raises(GaError):
        ops.self_attn_bwd(q, k, v, o, torch.zeros_like(o), lse, 2, 0.1, d_probs=d_probs)
    with pytest.raises(GaError):
        ops.self_attn_bwd(q, k, v, o, None, lse, 2, 0.1, d_probs=d_probs)


def test_the_framework_restatement_is_gone():
    from guided_attention_amd import ops
    assert not hasattr(ops, "_probs_cotangent_terms")
