"""The memory-contract harness (tests/memguard.py) can fail: small pure-torch fake ops on the CPU, each breaking one clause
of the contract, must be reported by the matching assertion; a correct op passes every halo fill."""
import pytest
import torch

from tests import memguard
from tests.memguard import ContractViolation, Input, guarded, poisoned_allocations, run_contract

N = 37


def _x(seed=0, n=N):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed))


def _past(t, before=0, after=0):
    """`t` (1-D, inside a guarded buffer) widened by elements of its halo -- what a kernel with a wrong bound touches"""
    return torch.as_strided(t, (t.numel() + before + after,), (1,), t.storage_offset() - before)


def _in_guard(t):
    return t.storage_offset() >= memguard.GUARD


# ---- the fake ops ---------------------------------------------------------------------------------------------------
def op_correct(x):
    out = torch.empty_like(x)
    out.copy_(x * 2)
    part = torch.empty((8, x.numel()), dtype=x.dtype, device=x.device)
    for i in range(8):
        part[i] = x * i
    return out, part.sum(0), x.max()


def op_writes_outside(x):
    out = torch.empty_like(x)
    out.copy_(x * 2)
    if _in_guard(out):                     # (a plain allocation has nothing around it that this test owns)
        w = _past(out, 1, 1)
        w[0] = 1.0
        w[-1] = 1.0
    return out


def op_writes_before_only(x):
    out = torch.empty_like(x)
    out.copy_(x * 2)
    if _in_guard(out):
        _past(out, 1, 0)[0] = 1.0
    return out


def op_writes_outside_its_input(x):
    _past(x.detach(), 0, 1)[-1] = 0.5
    return x * 2


def op_tail_unwritten(x):
    out = torch.empty_like(x)
    out[:-1] = x[:-1] * 2
    return out


def op_slot_unwritten(x):
    part = torch.empty((8, x.numel()), dtype=x.dtype, device=x.device)
    for i in range(7):                     # only 7 of the 8 workgroups had work ...
        part[i] = x * i
    return part.sum(0)                     # ... and all 8 slots are summed


def op_halo_into_sum(x):
    return _past(x.detach(), 0, 1).sum().reshape(1)


def op_halo_into_max(x):
    wide = _past(x.detach(), 0, 1)
    return wide[~wide.isnan()].max().reshape(1)      # a max that drops NaN, as v_max_f32 does


def op_modifies_input(x):
    x.detach()[3] = 0.0
    return x * 2


# ---- the harness reports each --------------------------------------------------------------------------------------
def test_correct_op_passes_every_fill():
    out = run_contract(op_correct, {'x': _x()}, 'cpu')
    assert set(out) == {'out.0', 'out.1', 'out.2'}
    assert torch.equal(out['out.0'], _x() * 2)


@pytest.mark.parametrize("op", [op_writes_outside, op_writes_before_only])
def test_write_outside_an_output_is_reported(op):
    with pytest.raises(ContractViolation, match=r"allocation #0 \(37,\).*written outside") as e:
        run_contract(op, {'x': _x()}, 'cpu')
    assert e.value.kind == 'halo'
    assert "before the start, nearest at offset -1" in str(e.value)
    if op is op_writes_outside:
        assert "past the end, nearest at offset +0" in str(e.value)


def test_write_outside_an_input_is_reported():
    with pytest.raises(ContractViolation, match=r"input x: written outside.*past the end, nearest at offset \+0") as e:
        run_contract(op_writes_outside_its_input, {'x': _x()}, 'cpu')
    assert e.value.kind == 'halo'


def test_unwritten_output_tail_is_reported():
    with pytest.raises(ContractViolation, match=r"out \(37,\): 1 element\(s\) never written.*flat index 36") as e:
        run_contract(op_tail_unwritten, {'x': _x()}, 'cpu')
    assert e.value.kind == 'poison'


def test_unwritten_partial_slot_is_reported():
    """one poisoned slot per column enters the sum: IEEE 754 addition of a quiet NaN and a number returns that NaN, payload
    included, so the result still carries the pattern and (b) -- which runs before (c) -- reports it"""
    with pytest.raises(ContractViolation, match=r"run 'zero': out \(37,\): 37 element\(s\) never written") as e:
        run_contract(op_slot_unwritten, {'x': _x()}, 'cpu')
    assert e.value.kind == 'poison'


def test_halo_in_a_sum_is_reported_and_zeros_alone_are_blind():
    """a poison halo arrives in the sum with its payload ((b), as above); a 3e38 halo is a finite number: (c)"""
    run_contract(op_halo_into_sum, {'x': _x()}, 'cpu', fills=('zero',))
    with pytest.raises(ContractViolation, match=r"run 'poison': out \(1,\): 1 element") as e:
        run_contract(op_halo_into_sum, {'x': _x()}, 'cpu', fills=('poison',))
    assert e.value.kind == 'poison'
    with pytest.raises(ContractViolation, match=r"out with 'big' halos differs from the plain run") as e:
        run_contract(op_halo_into_sum, {'x': _x()}, 'cpu', fills=('big',))
    assert e.value.kind == 'differs'


def test_halo_in_a_max_needs_the_big_fill():
    run_contract(op_halo_into_max, {'x': _x()}, 'cpu', fills=('zero', 'poison'))      # NaN is dropped: nothing to see
    with pytest.raises(ContractViolation, match=r"out with 'big' halos differs from the plain run") as e:
        run_contract(op_halo_into_max, {'x': _x()}, 'cpu')
    assert e.value.kind == 'differs'


def test_modified_input_is_reported():
    with pytest.raises(ContractViolation, match="input x was written to") as e:
        run_contract(op_modifies_input, {'x': _x()}, 'cpu')
    assert e.value.kind == 'input-modified'


def test_gradients_and_modules_are_returned_tensors():
    lin = torch.nn.Linear(N, 3)

    def fn(x, lin):
        y = lin(x)
        y.sum().backward()
        return y

    out = run_contract(fn, {'x': Input(_x(), grad=True), 'lin': lin}, 'cpu')
    assert {'out', 'grad:x', 'grad:lin.weight', 'grad:lin.bias'} <= set(out)
    assert lin.weight.grad is None          # the caller's module is copied, not used

    def bad(x, lin):
        y = lin(x)
        y.sum().backward()
        x.grad = torch.empty_like(x)        # a gradient buffer nobody fills
        return y

    with pytest.raises(ContractViolation, match="grad:x") as e:
        run_contract(bad, {'x': Input(_x(), grad=True), 'lin': lin}, 'cpu')
    assert e.value.kind == 'poison'


# ---- the pieces ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_type", ["cpu", "cuda"])
def test_device_filter(device_type):
    """only tensors of the chosen device type are replaced; everything else passes through untouched"""
    x = _x()
    with poisoned_allocations(device_type) as pa:
        a = torch.empty(5)
        b = torch.empty((2, 3), dtype=torch.int32)
        c = torch.empty_like(x)
        d = x.new_empty((4,))
        e = torch.empty(3, device='meta')
        z, f = torch.zeros(4), torch.full((4,), 2.0)
    cpu_made = [a, b, c, d]
    if device_type == 'cpu':
        assert len(pa.records) == 4
        assert all(t.storage_offset() == memguard.GUARD for t in cpu_made)
        assert all(int(memguard.poison_count(t)) == t.numel() for t in cpu_made)
        assert a.view(torch.int32)[0].item() == 0x7FC0BEEF and b[0, 0].item() == 0x7FC0BEEF
    else:
        assert not pa.records and all(t.storage_offset() == 0 for t in cpu_made)
    assert (a.shape, b.shape, b.dtype, c.shape, d.shape, e.device.type) == ((5,), (2, 3), torch.int32, x.shape, (4,), 'meta')
    assert z.storage_offset() == 0 and f.storage_offset() == 0 and bool((z == 0).all()) and bool((f == 2).all())
    # the replacements are gone afterwards
    assert torch.empty is memguard._ORIG_EMPTY and torch.empty_like is memguard._ORIG_EMPTY_LIKE
    assert 'new_empty' not in torch.Tensor.__dict__ or torch.Tensor.new_empty is memguard._ORIG_NEW_EMPTY
    assert torch.empty(3).storage_offset() == 0


def test_replacements_are_restored_after_an_error():
    with pytest.raises(KeyError):
        with poisoned_allocations('cpu'):
            raise KeyError('x')
    assert torch.empty is memguard._ORIG_EMPTY and torch.empty_like is memguard._ORIG_EMPTY_LIKE


@pytest.mark.parametrize("offset,mod32", [(0, 0), (16, 16), (4, 4)])
def test_guarded_alignment_and_layout(offset, mod32):
    buf, view = guarded((3, 5), torch.float32, 'cpu', fill='zero', halo='poison', offset_bytes=offset)
    assert view.is_contiguous() and view.shape == (3, 5) and view._base is None
    assert view.data_ptr() % 32 == mod32
    assert (view.data_ptr() % 16 == 0) == (offset != 4)
    assert buf.numel() == 15 + 2 * memguard.GUARD + offset // 4 and memguard.GUARD >= max(4096, 16 * 53)
    assert bool((view == 0).all()) and int(memguard.halo_damage(buf, view, 'poison')) == 0
    view.fill_(1.0)
    assert int(memguard.halo_damage(buf, view, 'poison')) == 0 and float(buf.nan_to_num(0.0).sum()) == 15.0


def test_empty_like_keeps_a_dense_permuted_layout():
    x = torch.randn(2, 3, 4).permute(2, 0, 1)
    with poisoned_allocations('cpu') as pa:
        y = torch.empty_like(x)
        y.copy_(x)
    assert y.stride() == torch.empty_like(x).stride() and torch.equal(y, x)
    pa.check()
    pa.assert_clean(y)


def test_poison_is_told_apart_from_a_computed_nan():
    with poisoned_allocations('cpu') as pa:
        out = torch.empty(4)
        out.copy_(torch.tensor([1.0, float('nan'), float('inf'), 0.0]) - torch.tensor([0.0, 0.0, float('inf'), 0.0]))
    assert bool(out.isnan().any())
    pa.assert_clean(out)
    for dtype, pattern in ((torch.float16, 0x7EEF), (torch.uint8, 0xA5), (torch.int64, 0x7FF8BEEF7FC0BEEF)):
        assert memguard.poison_value(dtype) == pattern
    _, h = guarded((4,), torch.float16, 'cpu')
    assert bool(h.isnan().all()) and int(memguard.poison_count(h)) == 4
    _, u = guarded((4,), torch.uint8, 'cpu')
    assert u.tolist() == [0xA5] * 4


def test_integer_input_halos_are_index_zero():
    idx = torch.arange(9, dtype=torch.int32)
    seen = []

    def fn(idx, x):
        seen.append((_past(idx, 2, 2).tolist(), _past(x.detach(), 0, 1)[-1].item()))
        return x.clone()

    run_contract(fn, {'idx': idx, 'x': _x()}, 'cpu')
    assert all(s[0] == [0, 0] + list(range(9)) + [0, 0] for s in seen)
    assert seen[0][1] == 0.0 and seen[1][1] == 0.0 and seen[2][1] != seen[2][1] and seen[3][1] == pytest.approx(3.0e38)


def test_handoff_entries_stay_with_a_guarded_tensor():
    from pose2room_amd.p2rnet import handoff
    with poisoned_allocations('cpu'):
        t = torch.empty(6)
        t.zero_()
        handoff.put(t, 'word', 42)
        assert handoff.peek(t, 'word') == 42 and handoff.peek(t.view(2, 3), 'word') is None
        t.add_(1)
        assert handoff.peek(t, 'word') is None
