"""Run-to-run bit equality: compare tensors by their raw bytes, and trace a module's forward and backward so that two runs
of the same work can be compared entry by entry, in execution order.  No GPU dependency: everything works on CPU tensors.

    record(module, fn)      -> [Entry(phase, name, index, dtype, shape, digest), ...] of one run of fn()
    first_difference(a, b)  -> the first place, in execution order, where two records differ, or None
    same_bits(x, y)         -> dtype, shape and bytes equal (raises if x and y are the same memory)

Phases of an Entry:
    "forward"     output `index` of the leaf module `name` (a module called k > 0 times before is named "name@k")
    "backward"    the gradient that arrived at that output: what the backward of everything downstream produced
    "grad_input"  the same gradient, under the name of each leaf module that took the tensor as input `index`; emitted BEFORE the
                  "backward" entry of the producer, so a layer whose own backward went wrong is the first name that differs
The digest is taken over the bytes (NaN payloads and the sign of zero count), on the host, at the moment the hook fires."""
import hashlib
from collections import namedtuple

import torch

Entry = namedtuple("Entry", "phase name index dtype shape digest")
Difference = namedtuple("Difference", "position a b")   # a / b: the Entry of each record there (None past the end of one)


def raw_bytes(t):
    """The tensor's elements as a flat uint8 tensor on its own device (a copy only where t is not contiguous)."""
    t = t.detach()
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    return t.contiguous().reshape(-1).view(torch.uint8)


def digest(t):
    return hashlib.blake2b(raw_bytes(t).cpu().numpy().tobytes(), digest_size=8).hexdigest()


def _storage_ptr(t):
    return t.untyped_storage().data_ptr() if t.numel() else None


def same_bits(x, y):
    """True when x and y have the same dtype, shape and bytes.  Comparing a tensor with itself (or with a view of its storage)
    cannot fail and is refused: ValueError."""
    if x is y:
        raise ValueError("same_bits: both arguments are the same tensor")
    px, py = _storage_ptr(x), _storage_ptr(y)
    if px is not None and px == py and x.device == y.device:
        raise ValueError("same_bits: the arguments share storage")
    if x.dtype != y.dtype or tuple(x.shape) != tuple(y.shape):
        return False
    bx, by = raw_bytes(x), raw_bytes(y)
    if bx.device != by.device:
        bx, by = bx.cpu(), by.cpu()
    return bool(torch.equal(bx, by))


def differing_elements(x, y):
    """How many elements differ in their bytes (for messages; same dtype and shape assumed)."""
    size = x.element_size()
    return int((raw_bytes(x).view(-1, size) != raw_bytes(y).view(-1, size).to(x.device)).any(dim=1).sum())


def _tensors(obj):
    """The tensors inside a module's arguments or result, in a fixed order."""
    if isinstance(obj, torch.Tensor):
        yield obj
    elif isinstance(obj, (list, tuple)):
        for o in obj:
            yield from _tensors(o)
    elif isinstance(obj, dict):
        for k in obj:
            yield from _tensors(obj[k])
    elif hasattr(obj, "__dict__") and not isinstance(obj, torch.nn.Module):   # result records such as `.sample`
        for k in vars(obj):
            yield from _tensors(vars(obj)[k])


def record(module, fn, every_module=False):
    """Run fn() with a forward hook on every leaf module of `module` and a gradient hook on every tensor those modules take or
    return -> the ordered list of entries.  The hooks are removed again before returning.
    every_module: hook the containers as well (a model whose blocks use their children's weights without calling them has few
    leaves that ever run); a container's entries follow those of the children it called, so the innermost name comes first."""
    entries, handles, calls, consumers, alive = [], [], {}, {}, []
    names = {m: n or type(m).__name__ for n, m in module.named_modules()
             if every_module or not any(True for _ in m.children())}

    def add(phase, name, index, t):
        if t is None:      # a Function that does not materialise missing gradients hands None on
            entries.append(Entry(phase, name, index, "None", (), ""))
        else:
            entries.append(Entry(phase, name, index, str(t.dtype), tuple(t.shape), digest(t)))

    def grad_hook(key):
        def hook(g):
            for cname, cindex in consumers[key]:
                add("grad_input", cname, cindex, g)
            for pname, pindex in producers[key]:
                add("backward", pname, pindex, g)
        return hook

    producers = {}

    def watch(t, producer):
        if id(t) not in consumers:       # one hook per tensor, however many modules return or take it
            consumers[id(t)], producers[id(t)] = [], []
            alive.append(t)              # ids stay unique for as long as the record runs
            handles.append(t.register_hook(grad_hook(id(t))))
        if producer is not None:
            producers[id(t)].append(producer)

    def forward_hook(mod, args, out):
        k = calls.get(mod, 0)
        calls[mod] = k + 1
        name = names[mod] + (f"@{k}" if k else "")
        for i, t in enumerate(_tensors(args)):
            if t.requires_grad and t.is_floating_point():
                watch(t, None)
                consumers[id(t)].append((name, i))
        for i, t in enumerate(_tensors(out)):
            add("forward", name, i, t)
            if t.requires_grad and t.is_floating_point():
                watch(t, (name, i))

    for m in names:
        handles.append(m.register_forward_hook(forward_hook))
    try:
        fn()
    finally:
        for h in handles:
            h.remove()
    return entries


def first_difference(a, b):
    """The first position at which two records differ -> Difference(position, entry of a, entry of b), or None.  A different
    order of execution, or one record ending early, is a difference like any other."""
    for i, (ea, eb) in enumerate(zip(a, b)):
        if tuple(ea) != tuple(eb):
            return Difference(i, ea, eb)
    if len(a) != len(b):
        n = min(len(a), len(b))
        return Difference(n, a[n] if len(a) > n else None, b[n] if len(b) > n else None)
    return None
