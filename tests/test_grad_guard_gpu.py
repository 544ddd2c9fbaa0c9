"""GPU: the kernels of the gradient guard (csrc/grad_guard.hip) and `GradGuard` against the float64 mirror
`grad_guard.grad_guard_reference`, and the guarded optimizer step against a twin that steps on the gradients the guarded
step wrote back.  Every gradient lies in a `memguard.guarded` view: what a wrong kernel reads or writes next to a
gradient is a halo that the test owns (poison halos are NaN: a read past the end would be counted as non-finite)."""
import pytest
import torch
from torch import nn

from pose2room_amd.p2rnet import grad_guard as gg
from tests import grad_guard_cases as gc
from tests import memguard as mg

pytestmark = pytest.mark.gpu

CHUNK = 16384                                   # the chunk size of the kernels (P2R_GG_CHUNK)
assert CHUNK == gg.CHUNK and 70001 > 2 * CHUNK and 70001 in gc.NUMELS


def place(grads, dev, offsets=gc.OFFSETS, halo='poison', reverse=False):
    """CPU gradients / None -> (bufs, views): every gradient in a guarded view of its own that starts `offsets[i % len]`
    elements behind the allocator's alignment; reverse: allocated in the opposite order"""
    n = len(grads)
    bufs, views = [None] * n, [None] * n
    for i in (reversed(range(n)) if reverse else range(n)):
        g = grads[i]
        if g is not None:
            bufs[i], views[i] = mg.guarded(g.shape, g.dtype, dev, fill=g, halo=halo,
                                           offset_bytes=offsets[i % len(offsets)] * g.element_size())
    return bufs, views


def halos_intact(bufs, views, halo='poison'):
    bad = [int(mg.halo_damage(b, v, halo)) for b, v in zip(bufs, views) if b is not None]
    assert not any(bad), bad


def read(out):
    """Measured -> (sumsq list, nonfinite list, norm, scale, found) on the host"""
    return (out.sumsq.tolist(), out.nonfinite.tolist(), float(out.norm.item()), float(out.scale.item()),
            float(out.found.item()))


def check_against_reference(grads, dev, max_norm, offsets=gc.OFFSETS):
    bufs, views = place(grads, dev, offsets)
    out = gg.measure(views, max_norm, device=dev)
    sumsq, bad, norm, scale, found = read(out)
    ref = gg.grad_guard_reference(grads, max_norm)
    gc.assert_measured(sumsq, bad, norm, ref)
    assert found == ref['found']
    if max_norm > 0:
        assert abs(scale - ref['scale']) <= 2.0 ** -23 * ref['scale']      # the float32 of two norms within 1e-9
    else:
        assert scale == 1.0
    halos_intact(bufs, views)
    return out, ref


# ---- 1. the norm against float64 -------------------------------------------------------------------------------------------
def test_norm_against_float64(dev):
    """numels 0 .. 70001 (more than two chunks of 16384), float32 and float64 mixed, a None slot in the middle, views at
    element offsets 0, 1, 2, 3.  1e-9: the squares of float32 inputs are exact in float64, and a float64 sum of N <= 4M
    terms is off by at most N * 2^-53 < 4.5e-10."""
    grads = gc.mixed_list(0)
    assert grads[len(grads) // 2] is None and {g.dtype for g in grads if g is not None} == {torch.float32, torch.float64}
    out, ref = check_against_reference(grads, dev, 1.0)
    assert ref['norm'] > 100 and ref['scale'] > 100
    assert int(out.steps.item()) == 1 and int(out.skipped.item()) == 0
    for shift in (1, 2, 3):                     # every tensor at every misalignment
        check_against_reference(grads, dev, 0.0, offsets=gc.OFFSETS[shift:] + gc.OFFSETS[:shift])


# ---- 2. same values, other addresses ---------------------------------------------------------------------------------------
def test_same_values_other_addresses_same_bits(dev):
    grads = gc.mixed_list(0)
    ba, va = place(grads, dev)
    bb, vb = place(grads, dev, offsets=(3, 0, 2, 1, 1), reverse=True)
    assert any(x.data_ptr() % 16 != y.data_ptr() % 16 for x, y in zip(va, vb) if x is not None and x.numel())
    a1 = gg.measure(va, 3.0, device=dev)
    b = gg.measure(vb, 3.0, device=dev)
    a2 = gg.measure(va, 3.0, device=dev)
    for other in (b, a2):
        for f in ('sumsq', 'nonfinite', 'norm', 'scale', 'found'):
            assert mg.same_bits(getattr(a1, f), getattr(other, f)), f
    assert float(a1.scale.item()) > 1.0


# ---- 3. the memory contract ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("halo", mg.FILLS)
def test_memory_contract(dev, halo):
    """halos of the gradients and of every buffer the wrapper allocates intact, the gradients unmodified, every output
    and work-buffer element written, the same bits whatever lies in the halos"""
    grads = gc.mixed_list(4)
    plain_b, plain_v = place(grads, dev, halo='zero')
    base = gg.measure(plain_v, 2.0, count_skips=True, device=dev)
    bufs, views = place(grads, dev, halo=halo)
    with mg.poisoned_allocations('cuda') as pa:
        out = gg.measure(views, 2.0, count_skips=True, device=dev)
        torch.cuda.synchronize(dev)
    assert len(pa.records) == 8                 # the five results and the three work buffers; the counters are zeros
    tensors = out.tensors()
    pa.assert_clean(*tensors.values(), names=list(tensors))
    halos_intact(bufs, views, halo)
    for g, v in zip(grads, views):
        assert g is None or mg.same_bits(v.cpu(), g)
    for f in ('sumsq', 'nonfinite', 'norm', 'scale', 'found', 'steps', 'skipped'):
        assert mg.same_bits(getattr(out, f), getattr(base, f)), f
    assert out.first_chunk.tolist()[:3] == [0, 1, 2] and out.part_count.numel() == gg.n_chunks([0 if g is None else g.numel() for g in grads])


def test_scale_in_place_contract(dev):
    """p2r_grad_scale: g / scale in the gradient's own precision, nothing outside the gradients, nothing at all when
    scale == 1"""
    grads = gc.mixed_list(6)
    bufs, views = place(grads, dev)
    one = torch.ones(1, dtype=torch.float32, device=dev)
    gg.scale_grads(views, one)
    for g, v in zip(grads, views):
        assert g is None or mg.same_bits(v.cpu(), g)
    for s in (4.0, 13.37):
        bufs, views = place(grads, dev)
        scale = torch.tensor([s], dtype=torch.float32, device=dev)
        gg.scale_grads(views, scale)
        halos_intact(bufs, views)
        for g, v in zip(grads, views):
            if g is not None:
                assert mg.same_bits(v.cpu(), g / scale.cpu().to(g.dtype)), (s, g.numel(), g.dtype)


# ---- 4. non-finite positions -----------------------------------------------------------------------------------------------
def test_nonfinite_positions(dev):
    grads, spots = gc.nonfinite_list()
    assert {p for p, _ in spots[1]} >= {0, 70000, CHUNK - 1, CHUNK} and {p for p, _ in spots[3]} >= {0, 39999, CHUNK - 1, CHUNK}
    out, ref = check_against_reference(grads, dev, 1.0)
    assert out.nonfinite.tolist() == [0, 5, 0, 4, 0] and float(out.found.item()) == 1.0
    assert torch.isfinite(out.sumsq).all() and torch.isfinite(out.norm).all() and torch.isfinite(out.scale).all()
    again = gg.measure(place(grads, dev)[1], 1.0, count_skips=True, out=out)
    assert again is out and int(out.steps.item()) == 2 and int(out.skipped.item()) == 1


# ---- 5. large and tiny magnitudes ------------------------------------------------------------------------------------------
def test_large_magnitudes_and_denormals(dev):
    """4096 float32 entries of 1e30: a float32 norm is inf, the float64 norm is 64 times the float32 nearest to 1e30
    (1.0000000150474662e30: the entries are that number, so the norm is 6.4e31 * (1 + 1.5e-8))"""
    grads = gc.magnitude_list()
    big = gg.measure(place(grads[:1], dev)[1], 1.0)
    e30 = float(torch.tensor(1e30, dtype=torch.float32))
    assert gc.rel_close(float(big.norm.item()), 64.0 * e30, 1e-9) and gc.rel_close(float(big.norm.item()), 6.4e31, 2e-8)
    assert float((grads[0] * grads[0]).sum()) == float('inf')          # what a float32 sum of squares gives
    out, ref = check_against_reference(grads, dev, 1e10)              # (the divisor stays a finite float32)
    assert ref['sumsq'][1] > 0 and out.sumsq[1].item() > 0             # squares of float32 denormals are not flushed
    assert out.nonfinite.tolist() == [0, 0, 0, 0]


# ---- 6. many tensors -------------------------------------------------------------------------------------------------------
def test_many_tensors(dev):
    grads = gc.many_small()
    assert len(grads) == 700 > 4 * gg.GROUP and any(g is None for g in grads)
    out, ref = check_against_reference(grads, dev, 0.5)
    assert out.first_chunk.tolist() == list(range(700))


def test_nothing_to_measure(dev):
    """an empty table and a table of absent gradients: the finishing launch alone writes every result"""
    empty = gg.measure([], 1.0, count_skips=True, device=dev)
    assert read(empty) == ([], [], 0.0, 1.0, 0.0) and int(empty.steps.item()) == 1 and int(empty.skipped.item()) == 0
    with mg.poisoned_allocations('cuda') as pa:
        absent = gg.measure([None, None, None], 0.5, device=dev)
        torch.cuda.synchronize(dev)
    pa.assert_clean(*absent.tensors().values(), names=list(absent.tensors()))
    assert read(absent) == ([0.0] * 3, [0] * 3, 0.0, 1.0, 0.0) and absent.first_chunk.tolist() == [0, 1, 2]
    gg.scale_grads([None, None], torch.full((1,), 2.0, device=dev))


# ---- 7. two steps without a synchronise in between -------------------------------------------------------------------------
def _fused(params):
    return torch.optim.AdamW(params, lr=1e-2, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.01, fused=True)


def _state(opt, params):
    return [t.detach().clone() for p in params for t in (p, opt.state[p]['exp_avg'], opt.state[p]['exp_avg_sq'],
                                                          opt.state[p]['step'])]


def _same(a, b):
    return len(a) == len(b) and all(mg.same_bits(x, y) for x, y in zip(a, b))


def _named(params):
    return [(f"p{i}", p) for i, p in enumerate(params)]


def test_two_steps_back_to_back(dev):
    init, grads = gc.clip_problem(seed=7, steps=2)

    def run(sync):
        params = [nn.Parameter(t.to(dev)) for t in init]
        opt = _fused(params)
        guard = gg.GradGuard(_named(params), 1.0, 'skip', optimizer=opt)
        # both steps' gradients are on the device before the first launch; the second set lies at other addresses
        placed = [place(g, dev, offsets=(s, s + 1)) for s, g in enumerate(grads)]
        assert all(a.data_ptr() != b.data_ptr() for a, b in zip(placed[0][1], placed[1][1]))
        torch.cuda.synchronize(dev)
        for bufs, views in placed:
            for p, v in zip(params, views):
                p.grad = v
            guard.step(opt)
            if sync:
                torch.cuda.synchronize(dev)
            opt.zero_grad()
        torch.cuda.synchronize(dev)
        assert guard.report()['steps'] == 2 and guard.report()['skipped'] == 0
        return _state(opt, params)

    assert _same(run(False), run(True))


# ---- 8. the clip step ------------------------------------------------------------------------------------------------------
def test_clip_step(dev):
    """fused AdamW with weight decay, four steps, gradients about 13 times max_norm.  2^-22: one rounding of scale to
    float32, one of the quotient and one of the store, each <= 2^-24."""
    max_norm = 1.0
    init, grads = gc.clip_problem(seed=3, steps=4, max_norm=max_norm)
    assert [(t.numel(), t.dtype) for t in init] == list(gc.CLIP_NUMELS)
    pa = [nn.Parameter(t.to(dev)) for t in init]
    pb = [nn.Parameter(t.to(dev)) for t in init]
    oa, ob = _fused(pa), _fused(pb)
    guard = gg.GradGuard(_named(pa), max_norm, 'ignore', optimizer=oa)
    for step, g in enumerate(grads):
        ref = gg.grad_guard_reference(g, max_norm)
        assert 10 < ref['scale'] < 20
        bufs, views = place(g, dev)
        for p, v in zip(pa, views):
            p.grad = v
        guard.step(oa)
        assert 'grad_scale' not in oa.__dict__ and 'found_inf' not in oa.__dict__
        rep = guard.report()
        assert gc.rel_close(rep['norm'], ref['norm'], 1e-9) and abs(rep['scale'] - ref['scale']) <= 2.0 ** -23 * ref['scale']
        halos_intact(bufs, views)
        for p, gi in zip(pa, g):
            gc.assert_quotient(p.grad, gi, ref['scale'])
        for p, q in zip(pb, pa):
            p.grad = q.grad.detach().clone()
        ob.step()
        assert _same(_state(oa, pa), _state(ob, pb)), step
    assert guard.report()['steps'] == 4 and guard.report()['skipped'] == 0


def test_clip_step_of_an_optimizer_without_grad_scale(dev):
    """SGD cannot take the divisor: the gradients pass through p2r_grad_scale and equal the mirror's g / scale bit for bit
    wherever the device's float32 scale is the mirror's"""
    init, grads = gc.clip_problem(seed=5, steps=1)
    params = [nn.Parameter(t.to(dev)) for t in init]
    twin = [nn.Parameter(t.to(dev)) for t in init]
    opt, opt2 = torch.optim.SGD(params, lr=0.1, momentum=0.9), torch.optim.SGD(twin, lr=0.1, momentum=0.9)
    guard = gg.GradGuard(_named(params), 1.0, 'raise', optimizer=opt)
    bufs, views = place(grads[0], dev)
    for p, v in zip(params, views):
        p.grad = v
    guard.step(opt)
    scale = guard.report()['scale']
    halos_intact(bufs, views)
    for p, q, g in zip(params, twin, grads[0]):
        gc.assert_quotient(p.grad, g, scale, rel=2.0 ** -23)
        assert mg.same_bits(p.grad.cpu(), g / torch.tensor(scale, dtype=g.dtype))
        q.grad = p.grad.detach().clone()
    opt2.step()
    assert all(mg.same_bits(p.detach(), q.detach()) for p, q in zip(params, twin))
    with pytest.raises(ValueError, match="skip"):
        gg.GradGuard(_named(params), 1.0, 'skip', optimizer=opt)


# ---- 9. skip ---------------------------------------------------------------------------------------------------------------
def _three_steps(dev, nonfinite, poison_step=1, steps=(0, 1, 2)):
    init, grads = gc.clip_problem(seed=9, steps=3)
    grads[poison_step][2][4000] = float('inf')
    params = [nn.Parameter(t.to(dev)) for t in init]
    opt = _fused(params)
    guard = gg.GradGuard(_named(params), 1.0, nonfinite, optimizer=opt)
    states, reports = [_state_or_none(opt, params)], []
    for s in steps:
        bufs, views = place(grads[s], dev)
        for p, v in zip(params, views):
            p.grad = v
        try:
            guard.step(opt)
        except FloatingPointError as e:
            reports.append(e)
        else:
            reports.append(guard.report())
        states.append(_state_or_none(opt, params))
    return states, reports, guard


def _state_or_none(opt, params):
    return _state(opt, params) if opt.state else None


def test_skip(dev):
    states, reports, guard = _three_steps(dev, 'skip')
    assert _same(states[2], states[1])                                  # step 2 of 3 changed nothing, counters included
    assert [float(t) for t in states[2][3::4]] == [1.0] * 5
    assert reports[1]['skipped'] == 1 and reports[1]['steps'] == 2
    bad = {n: c for n, (_, c) in reports[1]['per_parameter'].items() if c}
    assert bad == {'p2': 1}
    assert all(v[0] > 0 and v[0] == v[0] for v in reports[1]['per_parameter'].values())     # the norms stay readable
    assert reports[2]['skipped'] == 1 and reports[2]['steps'] == 3 and not any(c for _, c in reports[2]['per_parameter'].values())
    twin_states, twin_reports, _ = _three_steps(dev, 'skip', steps=(0, 2))
    assert _same(states[3], twin_states[2]) and twin_reports[-1]['skipped'] == 0
    assert not _same(states[3], states[2])


def test_raise_names_the_parameter(dev):
    states, reports, guard = _three_steps(dev, 'raise')
    assert isinstance(reports[1], FloatingPointError) and "gradient of p2 has 1 non-finite entry" in str(reports[1])
    assert _same(states[2], states[1])                                  # and the step was left out
    assert isinstance(reports[0], dict) and isinstance(reports[2], dict)


def test_ignore_lets_it_through(dev):
    states, reports, guard = _three_steps(dev, 'ignore')
    assert reports[1]['skipped'] == 0 and reports[1]['per_parameter']['p2'][1] == 1
    assert not torch.isfinite(states[2][4 * 2]).all()                   # the inf reached the parameter, as it does today
    assert all(torch.isfinite(states[2][4 * i]).all() for i in (0, 1, 3, 4))


# ---- 10. the trainer, one tiny step ----------------------------------------------------------------------------------------
def _tiny_trainer(dev, **spec):
    from pose2room_amd.p2rnet import METHODS, P2RConfig, default_config
    from pose2room_amd.p2rnet.training import ModuleWrapper, Trainer, load_optimizer
    cfg = P2RConfig(default_config('train', data={'num_frames': 128}, optimizer=spec), device=dev)
    torch.manual_seed(42)
    net = ModuleWrapper(METHODS.get('P2RNet')(cfg)).to(dev)
    return Trainer(cfg, net, load_optimizer(cfg.config, net), dev)


def _tiny_step(trainer):
    from pose2room_amd.p2rnet.synthetic import make_batch
    torch.manual_seed(7)                # the mixture heads' noise
    return trainer.train_step(make_batch(2, 128, seed=1))


def _capture_grads(trainer):
    """the gradients as the guard finds them, cloned in front of every guarded step"""
    seen = []
    inner = trainer.grad_guard.step

    def step(optimizer):
        seen.append([None if p.grad is None else p.grad.detach().clone() for p in trainer.grad_guard.params])
        inner(optimizer)
    trainer.grad_guard.step = step
    return seen


def test_trainer_tiny_step(dev):
    plain = _tiny_trainer(dev)
    assert plain.grad_guard is None
    loss0 = _tiny_step(plain)

    wide = _tiny_trainer(dev, clip_norm=1e30, clip_impl='kernel')
    seen = _capture_grads(wide)
    _tiny_step(wide)
    rep = wide.grad_guard.report()
    n0 = rep['norm']
    ref = gg.grad_guard_reference(seen[0], 1e30)
    assert gc.rel_close(n0, ref['norm'], 1e-9) and n0 > 0 and rep['scale'] == 1.0 and rep['skipped'] == 0
    assert list(rep['per_parameter']) == [n for n, p in wide.net.named_parameters() if p.requires_grad]

    guarded = _tiny_trainer(dev, clip_norm=n0 / 2, clip_impl='kernel', nonfinite='skip')
    seen = _capture_grads(guarded)
    loss = _tiny_step(guarded)
    assert loss == loss0 and list(loss) == list(loss0)
    rep = guarded.grad_guard.report()
    ref = gg.grad_guard_reference(seen[0], n0 / 2)
    assert rep['scale'] == ref['scale'] and 1.5 < rep['scale'] < 2.5
    assert rep['skipped'] == 0 and rep['steps'] == 1 and gc.rel_close(rep['norm'], ref['norm'], 1e-9)
    for p, g in zip(guarded.grad_guard.params, seen[0]):
        if g is not None:
            gc.assert_quotient(p.grad, g, ref['scale'])

    name, weight = next((n, p) for n, p in guarded.net.named_parameters() if p.requires_grad and p.dim() >= 2)

    def poison(g):
        g = g.clone(memory_format=torch.contiguous_format)
        g.view(-1)[0] = float('nan')
        return g
    handle = weight.register_hook(poison)
    before = [p.detach().clone() for p in guarded.grad_guard.params]
    _tiny_step(guarded)
    handle.remove()
    rep = guarded.grad_guard.report()
    assert rep['skipped'] == 1 and rep['steps'] == 2 and rep['per_parameter'][name][1] >= 1
    assert all(mg.same_bits(p.detach(), b) for p, b in zip(guarded.grad_guard.params, before))
