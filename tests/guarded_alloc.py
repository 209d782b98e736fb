"""Guarded output allocations: where a kernel puts its results, not which values it computes.

`guarded(ops)` replaces the name `torch` inside one module (guided_attention_amd.ops) by a proxy whose `empty` and
`empty_like` hand out tensors carved from a larger byte arena:

    [ RED bytes of 0xFF | body: the tensor's own bytes, 0xFF | padding to 16 bytes + RED bytes of 0xFF ]

0xFF in every byte is NaN as f16 / bf16 / f32 and -1 as int32, so
  * an element the kernel never stores still reads as all-0xFF afterwards (`assert_written`), whatever an earlier call
    left in the block the caching allocator would have handed out instead, and
  * a store in front of or behind the tensor lands in a red zone that `check()` reads back.
RED is a multiple of the allocator's own 512-byte granule, so the body keeps the alignment a plain allocation has and the
kernels choose the same vector paths as in production.  Every arena stays referenced until the guard is left: scratch that
the module drops right after its launch is checked as well.  Shape, strides and memory format of the returned tensor are
those of the real call, taken from the same call on the meta device.

Not guarded (handed to the real torch): other devices than the guarded ones, zero-size requests, requests of
LARGE bytes and more (counted in `large_passthroughs`), and every other factory (`zeros`, `full`, ...).
What this cannot see: out-of-bounds READS, and stores into memory the module did not allocate through empty / empty_like.
"""
import contextlib
import sys

import torch as _torch

RED = 4096                  # bytes in front of and behind every guarded body
LARGE = 32 * 1024 * 1024    # requests of this many bytes and more pass through (the persistent split-K slabs)
_SAME_SIZE_INT = {1: _torch.uint8, 2: _torch.int16, 4: _torch.int32, 8: _torch.int64}


class GuardError(AssertionError):
    pass


class _Arena:
    __slots__ = ("index", "arena", "nbytes", "shape", "dtype", "asked_by", "line")

    def __init__(self, index, arena, nbytes, shape, dtype, asked_by):
        self.index, self.arena, self.nbytes, self.shape, self.dtype = index, arena, nbytes, shape, dtype
        self.asked_by, self.line = asked_by if isinstance(asked_by, tuple) else (asked_by, None)

    def __str__(self):
        at = f" (line {self.line})" if self.line else ""
        return f"allocation #{self.index} {tuple(self.shape)} {self.dtype} asked for by {self.asked_by}{at}"

    def zones(self):
        return self.arena[:RED], self.arena[RED + self.nbytes:]


class _TorchProxy:
    """Stands in for the `torch` module inside the guarded module: `empty` / `empty_like` are guarded, the rest is torch's."""

    def __init__(self, guard):
        object.__setattr__(self, "_guard", guard)

    def __getattr__(self, name):
        return getattr(_torch, name)

    def empty(self, *args, **kwargs):
        device = _torch.device(kwargs.get("device") or "cpu")
        return self._guard._allocate(_torch.empty, args, kwargs, device)

    def empty_like(self, src, *args, **kwargs):
        device = _torch.device(kwargs.get("device") or src.device)
        return self._guard._allocate(_torch.empty_like, (src,) + args, kwargs, device)


class Guard:
    def __init__(self, module, devices=("cuda",)):
        self.module = module
        self.devices = tuple(devices)
        self.arenas = []
        self.large_passthroughs = 0
        self.proxy = _TorchProxy(self)

    # ------------------------------------------------------------------ allocation
    def _qualname(self, code):
        """`Class.method` for a method of a class of the guarded module (code objects carry it from Python 3.11 on)."""
        if hasattr(code, "co_qualname"):
            return code.co_qualname
        for name, cls in vars(self.module).items():
            if isinstance(cls, type):
                for attr in vars(cls).values():
                    if getattr(getattr(attr, "__func__", attr), "__code__", None) is code:
                        return f"{name}.{code.co_name}"
        return code.co_name

    def _asked_by(self):
        globs = vars(self.module)
        f = sys._getframe(3)
        while f is not None:
            if f.f_globals is globs:
                return self._qualname(f.f_code), f.f_lineno
            f = f.f_back
        return "<outside the guarded module>", None

    def _carve(self, shape, strides, dtype, device, asked_by):
        """The one place that lays an arena out: [RED | body, padded to 16 bytes | RED], all 0xFF."""
        nbytes = (1 + sum((n - 1) * s for n, s in zip(shape, strides))) * dtype.itemsize
        arena = _torch.full((RED + -(-nbytes // 16) * 16 + RED,), 0xFF, dtype=_torch.uint8, device=device)
        self.arenas.append(_Arena(len(self.arenas), arena, nbytes, shape, dtype, asked_by))
        return arena[RED:RED + nbytes].view(dtype).as_strided(shape, strides)

    def _allocate(self, real, args, kwargs, device):
        if device.type not in self.devices:
            return real(*args, **kwargs)
        meta = real(*args, **dict(kwargs, device="meta"))
        if meta.numel() == 0:
            return real(*args, **kwargs)
        shape, strides, dtype = tuple(meta.shape), tuple(meta.stride()), meta.dtype
        if (1 + sum((n - 1) * s for n, s in zip(shape, strides))) * dtype.itemsize >= LARGE:
            self.large_passthroughs += 1
            return real(*args, **kwargs)
        out = self._carve(shape, strides, dtype, device, self._asked_by())
        if kwargs.get("requires_grad"):
            out.requires_grad_(True)
        return out

    def carve(self, shape, dtype, device, asked_by="the test"):
        """A guarded tensor for a test that calls the C ABI itself (contiguous)."""
        meta = _torch.empty(shape, dtype=dtype, device="meta")
        return self._carve(tuple(meta.shape), tuple(meta.stride()), dtype, device, asked_by)

    # ------------------------------------------------------------------ checks
    def _sync(self):
        if any(a.arena.is_cuda for a in self.arenas):
            _torch.cuda.synchronize()

    def owns(self, t):
        """The arena whose body holds the first element of `t`, or None."""
        p = t.data_ptr()
        for a in self.arenas:
            base = a.arena.data_ptr() + RED
            if base <= p < base + a.nbytes:
                return a
        return None

    def check(self):
        """Every byte of every red zone is still 0xFF."""
        self._sync()
        if not self.arenas:
            return
        flags = _torch.stack([(z != 0xFF).any() for a in self.arenas for z in a.zones()]).cpu().tolist()
        for i, a in enumerate(self.arenas):
            for bad, zone, name in zip(flags[2 * i:2 * i + 2], a.zones(), ("front", "back")):
                if not bad:
                    continue
                off = int((zone != 0xFF).nonzero()[0, 0])
                where = off - RED if name == "front" else a.nbytes + off     # byte offset relative to the body's first byte
                raise GuardError(f"store outside the output: {a}: {name} red zone, first changed byte at offset {where} "
                                 f"from the start of the tensor ({a.nbytes} bytes), value {int(zone[off]):#04x}")

    def assert_written(self, t, what, undefined=None):
        """No element of `t` still has all its bytes 0xFF.  `undefined`: boolean mask (broadcastable to t) of elements the
        interface declares unspecified.  `t` must live in a guarded arena, or the check would prove nothing."""
        self._sync()
        arena = self.owns(t)
        if arena is None:
            raise GuardError(f"{what}: the tensor is not a guarded allocation (was it copied, or allocated outside the guard?)")
        unwritten = unwritten_mask(t)
        if undefined is not None:
            unwritten = unwritten & ~undefined.to(unwritten.device).expand(unwritten.shape)
        n = int(unwritten.sum())
        if n:
            first = tuple(int(i) for i in unwritten.nonzero()[0])
            raise GuardError(f"{what}: {n} of {t.numel()} elements never written, first at index {first} ({arena})")

    def assert_all_written(self, undefined=lambda arena: None):
        """Every guarded allocation, returned or not (gradient buffers, statistics, side outputs), is written in full.
        `undefined(arena)`: None, or a flat boolean mask over the allocation's elements of the slots that the interface
        leaves unspecified (a workspace's slots beyond the blocks in use)."""
        self._sync()
        for a in self.arenas:
            body = a.arena[RED:RED + a.nbytes].view(a.dtype)
            unwritten = unwritten_mask(body)
            mask = undefined(a)
            if mask is not None:
                unwritten = unwritten & ~mask.to(unwritten.device)
            n = int(unwritten.sum())
            if n:
                raise GuardError(f"{n} of {body.numel()} elements never written, first at flat index "
                                 f"{int(unwritten.nonzero()[0, 0])}: {a}")


def unwritten_mask(t):
    """Boolean tensor of t's shape: the elements whose bytes are all 0xFF."""
    flat = t.detach().contiguous().reshape(-1)
    bits = flat.view(_torch.uint8).reshape(-1, flat.dtype.itemsize)
    return (bits == 0xFF).all(1).reshape(t.shape)


def assert_copy_written(t, what):
    """For a tensor that autograd may have copied out of a guarded buffer (a leaf's .grad): a copy keeps the bits."""
    unwritten = unwritten_mask(t)
    n = int(unwritten.sum())
    if n:
        raise GuardError(f"{what}: {n} of {t.numel()} elements never written, first at index "
                         f"{tuple(int(i) for i in unwritten.nonzero()[0])}")


def snapshot(*tensors):
    """Bit copies of the inputs, to compare after the call (assert_intact)."""
    return [(t, t.detach().clone()) for t in tensors if t is not None]


def assert_intact(snap, what="input"):
    for i, (t, before) in enumerate(snap):
        now = t.detach()
        as_int = _SAME_SIZE_INT[now.dtype.itemsize]
        same = now.view(as_int) == before.view(as_int) if not now.dtype == _torch.bool else now == before
        if not bool(same.all()):
            first = tuple(int(j) for j in (~same).nonzero()[0])
            raise GuardError(f"{what} #{i} {tuple(t.shape)} {t.dtype} was modified by the call, first at index {first}")


@contextlib.contextmanager
def guarded(module, devices=("cuda",), check=True):
    """Replace `module.torch` by the guarding proxy for the duration; on a clean exit check every red zone."""
    guard = Guard(module, devices)
    real = module.torch
    module.torch = guard.proxy
    try:
        yield guard
    finally:
        module.torch = real
    if check:
        guard.check()
