"""The guarded allocator of tests/guarded_alloc.py itself, on CPU tensors (the guard switched to guard the CPU device).
This is the proof that the red-zone check detects a store outside an output and that `assert_written` detects a missing one:
no GPU build that writes out of bounds is ever made or run."""
import types

import pytest
import torch

import guarded_alloc as ga
from guarded_alloc import GuardError, guarded

# a stand-in for guided_attention_amd.ops: a module that holds the name `torch` and allocates its outputs through it
_SOURCE = '''
import torch


def make_output(*args, **kwargs):
    return torch.empty(*args, **kwargs)


def make_like(src, **kwargs):
    return torch.empty_like(src, **kwargs)


class Scale(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y = torch.empty_like(x)
        y.copy_(x * 2)
        return y

    @staticmethod
    def backward(ctx, g):
        dx = torch.empty_like(g)
        dx.copy_(g * 2)
        return dx


def other_factories(n):
    return torch.zeros(n), torch.float16, torch.nn.functional.relu(torch.ones(n))
'''


@pytest.fixture()
def mod():
    m = types.ModuleType("fake_ops")
    exec(compile(_SOURCE, "fake_ops.py", "exec"), vars(m))
    return m


def _same_layout(got, real):
    assert got.shape == real.shape and got.stride() == real.stride() and got.dtype == real.dtype
    for fmt in (torch.contiguous_format, torch.channels_last):
        if real.dim() == 4:
            assert got.is_contiguous(memory_format=fmt) == real.is_contiguous(memory_format=fmt)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.int32])
def test_guarded_empty_has_the_layout_of_the_real_call(mod, dtype):
    wide = torch.zeros(6, 40, dtype=dtype)
    cl = torch.zeros(2, 8, 3, 5, dtype=dtype).contiguous(memory_format=torch.channels_last)
    with guarded(mod, devices=("cpu",)) as g:
        cases = [
            (mod.make_output(3, 5, dtype=dtype), torch.empty(3, 5, dtype=dtype)),
            (mod.make_output((2, 3, 7), dtype=dtype, device="cpu"), torch.empty((2, 3, 7), dtype=dtype)),
            (mod.make_output((2, 8, 3, 5), dtype=dtype, memory_format=torch.channels_last),
             torch.empty((2, 8, 3, 5), dtype=dtype, memory_format=torch.channels_last)),
            (mod.make_like(cl), torch.empty_like(cl)),                                       # preserve_format: channels_last
            (mod.make_like(cl.permute(0, 2, 3, 1)), torch.empty_like(cl.permute(0, 2, 3, 1))),
            (mod.make_like(torch.zeros(2, 8, 3, 5, dtype=dtype), memory_format=torch.channels_last),
             torch.empty_like(torch.zeros(2, 8, 3, 5, dtype=dtype), memory_format=torch.channels_last)),
            (mod.make_like(wide[:, 8:24]), torch.empty_like(wide[:, 8:24])),                 # a column slice: dense result
            (mod.make_like(wide[1:5]), torch.empty_like(wide[1:5])),
            (mod.make_like(wide, dtype=torch.float32), torch.empty_like(wide, dtype=torch.float32)),
        ]
        for got, real in cases:
            _same_layout(got, real)
            arena = g.owns(got)
            assert arena is not None and arena.asked_by in ("make_output", "make_like")
            assert got.data_ptr() % 16 == 0 and got.data_ptr() == arena.arena.data_ptr() + ga.RED
            assert bool(ga.unwritten_mask(got).all())
            if got.dtype == torch.int32:
                assert bool((got == -1).all())
            else:
                assert bool(torch.isnan(got).all())
        assert len(g.arenas) == len(cases)
        # zero-size requests (the q.new_empty(0) style placeholders) and other devices pass through
        z = mod.make_output(0, dtype=dtype)
        assert z.numel() == 0 and g.owns(z) is None
        assert mod.make_output((4,), dtype=dtype, device="meta").device.type == "meta"
        assert len(g.arenas) == len(cases) and g.large_passthroughs == 0
        # everything else is torch's own
        zeros, f16, relu = mod.other_factories(3)
        assert f16 is torch.float16 and bool((zeros == 0).all()) and bool((relu == 1).all())
    assert mod.torch is torch


def test_default_guard_leaves_the_cpu_alone(mod):
    with guarded(mod) as g:
        t = mod.make_output(5)
        assert g.owns(t) is None and not g.arenas


def test_large_requests_pass_through_and_are_counted(mod, monkeypatch):
    monkeypatch.setattr(ga, "LARGE", 1024)
    with guarded(mod, devices=("cpu",)) as g:
        small, big = mod.make_output(255, dtype=torch.float32), mod.make_output(256, dtype=torch.float32)
        assert g.owns(small) is not None and g.owns(big) is None
        assert g.large_passthroughs == 1


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("where", ["behind", "in front"])
def test_a_store_outside_the_body_fails_the_check_and_names_the_allocation(mod, where, dtype):
    """One element behind the last / in front of the first, written through as_strided the way a kernel that rounds its tail
    up to the vector width (or indexes one block too far back) would."""
    with pytest.raises(GuardError) as e:
        with guarded(mod, devices=("cpu",)) as g:
            mod.make_output(3, dtype=dtype).fill_(0)
            t = mod.make_output((5, 7), dtype=dtype)
            t.fill_(1.0)
            g.check()                                       # a full write of the body itself is clean
            body = g.owns(t).arena[ga.RED - 64:].view(dtype)            # 64 bytes in front of the body onwards
            first = 64 // dtype.itemsize
            body[first + 35 if where == "behind" else first - 1] = 2.0
    msg = str(e.value)
    assert "allocation #1" in msg and "(5, 7)" in msg and str(dtype) in msg and "make_output" in msg
    assert ("back red zone" in msg and f"offset {35 * dtype.itemsize} " in msg) if where == "behind" else \
        ("front red zone" in msg and f"offset {-dtype.itemsize} " in msg)
    assert mod.torch is torch


def test_explicit_check_and_scratch_that_the_module_dropped(mod):
    with guarded(mod, devices=("cpu",), check=False) as g:
        scratch = mod.make_output(10, dtype=torch.float32)
        scratch.as_strided((1,), (1,), 10).fill_(0.0)        # one float behind a scratch buffer ...
        del scratch                                          # ... that the module no longer holds
        with pytest.raises(GuardError, match=r"allocation #0 \(10,\) torch.float32 asked for by make_output"):
            g.check()


def test_unwritten_elements(mod):
    with guarded(mod, devices=("cpu",)) as g:
        t = mod.make_output((4, 6), dtype=torch.bfloat16)
        t[:, :5] = 0.5
        t[:3, 5] = float("nan")                              # a NaN the kernel computed is a written element (0x7fc0, not 0xffff)
        with pytest.raises(GuardError, match=r"terms: 1 of 24 elements never written, first at index \(3, 5\)"):
            g.assert_written(t, "terms")
        mask = torch.zeros(4, 6, dtype=torch.bool)
        mask[3, 5] = True
        g.assert_written(t, "terms", undefined=mask)         # declared unspecified: masked
        mask[3, 5], mask[0, 0] = False, True
        with pytest.raises(GuardError):
            g.assert_written(t, "terms", undefined=mask)     # a mask elsewhere does not hide it
        i = mod.make_output(8, dtype=torch.int32)
        i[:7] = 3
        with pytest.raises(GuardError, match="first at index \\(7,\\)"):
            g.assert_written(i, "packed")
        cl = mod.make_output((1, 8, 2, 2), dtype=torch.float16, memory_format=torch.channels_last)
        cl.fill_(0)
        cl[0, 5, 1, 0] = torch.tensor(-1, dtype=torch.int16).view(torch.float16)     # the raw 0xFFFF pattern back in place
        with pytest.raises(GuardError, match=r"first at index \(0, 5, 1, 0\)"):
            g.assert_written(cl, "y")
        with pytest.raises(GuardError, match="not a guarded allocation"):
            g.assert_written(torch.zeros(3), "a tensor from elsewhere")
        with pytest.raises(GuardError):
            ga.assert_copy_written(t.clone(), "copy")


def test_every_allocation_is_checked_unless_named_scratch(mod):
    with guarded(mod, devices=("cpu",)) as g:
        mod.make_output((2, 3), dtype=torch.float16).fill_(1)
        ws = mod.make_output(8, dtype=torch.float32)
        ws[:5] = 0
        del ws                                               # dropped by the module: still checked
        with pytest.raises(GuardError, match=r"3 of 8 elements never written, first at flat index 5: allocation #1 \(8,\)"):
            g.assert_all_written()
        tail = torch.arange(8) >= 5                          # slots 5 .. 7 declared unspecified
        g.assert_all_written(undefined=lambda a: tail if a.asked_by == "make_output" and a.shape == (8,) else None)
        with pytest.raises(GuardError, match="1 of 8 elements never written, first at flat index 5"):
            g.assert_all_written(undefined=lambda a: torch.arange(8) >= 6 if a.shape == (8,) else None)


def test_inputs_intact():
    a, b = torch.arange(12.).reshape(3, 4), torch.arange(5, dtype=torch.int32)
    nan = torch.tensor([float("nan"), 1.0])                  # compared as bits: a NaN input is not a change
    snap = ga.snapshot(a, None, b, nan)
    ga.assert_intact(snap)
    a[2, 1] = -0.0 + a[2, 1]
    ga.assert_intact(snap)
    a[2, 1] = 7.5
    with pytest.raises(GuardError, match=r"input #0 \(3, 4\) torch.float32 was modified by the call, first at index \(2, 1\)"):
        ga.assert_intact(snap)


def test_autograd_functions_of_the_module_keep_working(mod):
    x = torch.arange(6.).requires_grad_(True)
    with guarded(mod, devices=("cpu",)) as g:
        y = mod.Scale.apply(x)
        y.backward(torch.ones(6))
        assert [a.asked_by for a in g.arenas] == ["Scale.forward", "Scale.backward"]      # qualified: which Function asked
        g.assert_written(y, "y")
    assert torch.equal(y.detach(), x.detach() * 2) and torch.equal(x.grad, torch.full((6,), 2.0))


def test_the_proxy_is_gone_after_an_exception(mod):
    with pytest.raises(ZeroDivisionError):
        with guarded(mod, devices=("cpu",)):
            assert mod.torch is not torch
            1 / 0
    assert mod.torch is torch


def test_the_real_ops_module_is_patched_and_restored():
    from guided_attention_amd import ops
    real = ops.torch
    with guarded(ops, devices=("cpu",)) as g:
        assert ops.torch is g.proxy and ops.torch.float16 is torch.float16
        assert ops.torch.autograd.Function is torch.autograd.Function
    assert ops.torch is real is torch


def test_carve(mod):
    with guarded(mod, devices=("cpu",)) as g:
        y = g.carve((5, 3), torch.float16, "cpu")
        assert y.shape == (5, 3) and y.is_contiguous() and bool(torch.isnan(y).all()) and g.owns(y).asked_by == "the test"
