"""tests/repro_trace.py on the CPU: a four-layer toy whose second run is dishonest by one mantissa bit, in one layer's forward
and in another layer's backward.  `first_difference` must name exactly that layer and phase; honest runs must compare equal."""
import pytest
import torch

import repro_trace as rt


def flip_lowest_mantissa_bit(t, element=0):
    """A copy of t whose element `element` (flat index) has its lowest mantissa bit flipped."""
    ints = {2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    out = t.detach().clone().contiguous()
    out.view(-1).view(ints)[element] ^= 1
    return out


class _FlipGrad(torch.autograd.Function):
    """Identity whose backward flips one bit of the gradient when told to: a layer's backward that is off by one ulp."""

    @staticmethod
    def forward(ctx, x, dishonest):
        ctx.dishonest = dishonest
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return (flip_lowest_mantissa_bit(g, 3) if ctx.dishonest else g), None


class Layer(torch.nn.Module):
    def __init__(self, n, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.weight = torch.nn.Parameter(torch.randn(n, n, generator=g) / n ** 0.5)
        self.calls, self.bad_forward, self.bad_backward = 0, False, False

    def forward(self, x):
        self.calls += 1
        second = self.calls == 2
        x = _FlipGrad.apply(x, self.bad_backward and second)     # backward runs last for this layer: it corrupts d/d input
        y = torch.tanh(x @ self.weight)
        if self.bad_forward and second:
            y = y + (flip_lowest_mantissa_bit(y, 5) - y.detach())     # one ulp, exactly; the gradient still flows
        return y


class Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.body = torch.nn.Sequential(*[Layer(8, s) for s in range(4)])

    def forward(self, x):
        return self.body(x)


def _run(toy, x):
    def fn():
        leaf = x.clone().requires_grad_(True)
        toy(leaf).square().sum().backward()
    return rt.record(toy, fn)


@pytest.fixture
def x():
    return torch.randn(3, 8, generator=torch.Generator().manual_seed(7))


def test_honest_runs_have_no_difference(x):
    toy = Toy()
    a, b = _run(toy, x), _run(toy, x)
    assert rt.first_difference(a, b) is None
    # four forwards, then the gradients in reverse: at each layer's output, and at the input of each layer (the leaf included)
    assert [e.name for e in a if e.phase == "forward"] == [f"body.{i}" for i in range(4)]
    assert [e.name for e in a if e.phase == "backward"] == [f"body.{i}" for i in (3, 2, 1, 0)]
    assert [e.name for e in a if e.phase == "grad_input"] == [f"body.{i}" for i in (3, 2, 1, 0)]
    assert all(e.dtype == "torch.float32" and e.shape == (3, 8) and e.index == 0 for e in a)


def test_a_dishonest_forward_is_named(x):
    toy = Toy()
    toy.body[2].bad_forward = True
    d = rt.first_difference(_run(toy, x), _run(toy, x))
    assert d is not None and (d.a.phase, d.a.name) == ("forward", "body.2") == (d.b.phase, d.b.name)
    assert d.a.digest != d.b.digest and d.position == 2


def test_a_dishonest_backward_is_named(x):
    toy = Toy()
    toy.body[1].bad_backward = True
    a, b = _run(toy, x), _run(toy, x)
    d = rt.first_difference(a, b)
    assert d is not None and (d.a.phase, d.a.name) == ("grad_input", "body.1") == (d.b.phase, d.b.name)
    # every forward entry and every gradient upstream of that backward is the same
    assert a[:d.position] == b[:d.position] and d.position == 4 + 2 * 3 - 1
    # the producer of that tensor sees it next, under its own name
    assert (b[d.position + 1].phase, b[d.position + 1].name) == ("backward", "body.0")


def test_the_first_layers_backward_is_seen_at_the_leaf(x):
    toy = Toy()
    toy.body[0].bad_backward = True
    d = rt.first_difference(_run(toy, x), _run(toy, x))
    assert (d.a.phase, d.a.name) == ("grad_input", "body.0")


def test_order_and_length_are_part_of_the_record(x):
    toy = Toy()
    a = _run(toy, x)
    swapped = [a[1], a[0]] + a[2:]
    assert rt.first_difference(a, swapped).position == 0
    d = rt.first_difference(a, a[:-1])
    assert d.position == len(a) - 1 and d.a == a[-1] and d.b is None
    again = rt.record(toy, lambda: (toy(x), toy(x)))          # a module called again is a new name
    assert [e.name for e in again][4:] == [f"body.{i}@1" for i in range(4)]


def test_same_bits_is_a_comparison_of_bytes():
    a = torch.tensor([0.0, 1.0, float("nan")])
    assert rt.same_bits(a, a.clone())
    assert not rt.same_bits(a, torch.tensor([-0.0, 1.0, float("nan")]))             # the sign of zero counts
    other_nan = a.clone()
    other_nan.view(torch.int32)[2] ^= 1                                             # still a NaN, another payload
    assert torch.isnan(other_nan[2]) and not rt.same_bits(a, other_nan)
    assert not rt.same_bits(a, a.double()) and not rt.same_bits(a, a.clone().reshape(3, 1))
    assert not rt.same_bits(a, flip_lowest_mantissa_bit(a, 1))
    assert rt.differing_elements(a, flip_lowest_mantissa_bit(a, 1)) == 1
    for dt in (torch.float16, torch.bfloat16, torch.int64, torch.bool):
        t = torch.arange(6).reshape(2, 3).to(dt)
        assert rt.same_bits(t, t.clone()) and rt.same_bits(t.t(), t.t().clone())    # non-contiguous views compare by value
    assert rt.same_bits(torch.empty(0), torch.empty(0))
    assert rt.same_bits(torch.tensor(2.5), torch.tensor(2.5))                       # zero-dimensional


def test_same_bits_refuses_a_comparison_that_cannot_fail():
    a = torch.arange(4.0)
    with pytest.raises(ValueError):
        rt.same_bits(a, a)
    with pytest.raises(ValueError):
        rt.same_bits(a, a.view(2, 2))
    with pytest.raises(ValueError):
        rt.same_bits(a[:2], a[2:])


def test_digest_is_over_bytes():
    a = torch.tensor([0.0, 1.0])
    assert rt.digest(a) == rt.digest(a.clone()) != rt.digest(torch.tensor([-0.0, 1.0]))
    assert rt.digest(a) != rt.digest(a.half())
