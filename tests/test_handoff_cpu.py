"""CPU: side outputs carried on the tensor object (pose2room_amd.p2rnet.handoff) -- the range words of split16 operands, the
BatchNorm-backward sums and the residual mask ride on it.  The autograd tests pin the PyTorch behaviour this relies on: if
a future torch drops a tensor's attributes on the way from producer to consumer, they fail here instead of the train step
silently paying fallback passes."""
import torch
from torch.autograd import Function

from pose2room_amd.p2rnet import handoff


def test_put_take_round_trip():
    t = torch.zeros(4)
    handoff.put(t, 'k', 'v')
    handoff.put(t, 'other', 3)
    assert handoff.peek(t, 'k') == 'v'
    assert handoff.take(t, 'k') == 'v'
    assert handoff.take(t, 'k') is None                # consumed
    assert handoff.peek(t, 'k') is None
    assert handoff.take(t, 'other') == 3               # keys are independent
    assert handoff.take(torch.zeros(4), 'k') is None    # nothing was put


def test_in_place_change_voids_the_entry():
    t = torch.zeros(4)
    handoff.put(t, 'k', 'v')
    t.add_(1.0)
    assert handoff.peek(t, 'k') is None
    assert handoff.take(t, 'k') is None
    handoff.put(t, 'k', 'w')                           # a new entry for the new state
    assert handoff.take(t, 'k') == 'w'


def test_views_and_detached_tensors_get_nothing():
    t = torch.randn(2, 3)
    handoff.put(t, 'k', 'v')
    for other in (t.view_as(t), t.detach()):
        assert other.data_ptr() == t.data_ptr() and other._version == t._version
        assert handoff.peek(other, 'k') is None
        assert handoff.take(other, 'k') is None
    assert handoff.take(t, 'k') == 'v'                 # still there for the very tensor


def test_dropped_tensor_passes_nothing_on():
    t = torch.randn(64, 53)
    handoff.put(t, 'k', 'v')
    del t
    fresh = torch.randn(64, 53)                        # may well reuse the block: same address, version 0
    assert handoff.take(fresh, 'k') is None


class _Up(Function):
    seen = []

    @staticmethod
    def forward(ctx, x):
        return x * 2.0

    @staticmethod
    def backward(ctx, g):
        _Up.seen.append(handoff.take(g, 'k'))
        return g * 2.0


class _Down(Function):
    @staticmethod
    def forward(ctx, x):
        return x * 3.0

    @staticmethod
    def backward(ctx, g):
        gx = g * 3.0                                   # a fresh tensor: only autograd holds it once we return
        handoff.put(gx, 'k', 'from-down')
        return gx


def test_entry_on_a_returned_gradient_reaches_the_upstream_backward():
    _Up.seen.clear()
    x = torch.randn(5, requires_grad=True)
    _Down.apply(_Up.apply(x)).sum().backward()
    assert _Up.seen == ['from-down']
    assert torch.equal(x.grad, torch.full((5,), 6.0))


def test_accumulated_gradient_gets_nothing():
    """a second consumer: autograd sums the two contributions, out of place or into the first one in place"""
    _Up.seen.clear()
    x = torch.randn(5, requires_grad=True)
    y = _Up.apply(x)
    (_Down.apply(y).sum() + y.sum()).backward()
    assert _Up.seen == [None]
    assert torch.equal(x.grad, torch.full((5,), 8.0))


class _Producer(Function):
    @staticmethod
    def forward(ctx, x):
        y = x * 2.0
        handoff.put(y, 'k', 'from-producer')
        return y

    @staticmethod
    def backward(ctx, g):
        return g * 2.0


class _Consumer(Function):
    seen = []

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        _Consumer.seen.append(handoff.take(x, 'k'))
        return x * 3.0

    @staticmethod
    def backward(ctx, g):
        return g * 3.0


def test_entry_on_a_forward_output_reaches_the_consumer_forward():
    _Consumer.seen.clear()
    x = torch.randn(2, 3, requires_grad=True)
    _Consumer.apply(_Producer.apply(x)).sum().backward()
    assert _Consumer.seen == ['from-producer']
    assert torch.equal(x.grad, torch.full((2, 3), 6.0))
