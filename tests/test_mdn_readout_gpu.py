"""GPU: the sampler's read-outs over the individual draws (csrc/mdn_sample.hip, p2r_mdn_sample_ex): per-draw samples,
lower median, the unchanged mean, stream independence, memory contract, and `generate_hypotheses` with them.
Inputs, the mirror's results and the median-gap rule: tests/mdn_readout_cases.py."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

from tests import memguard
from tests import mdn_readout_cases as cases
from tests.test_mdn_sample_gpu import _assert_mirror, _heads, _net, _pis

pytestmark = pytest.mark.gpu

COUNTS = list(cases.COUNTS)


@functools.lru_cache(maxsize=None)
def _inputs(G, dev):
    c = cases.case(G)
    heads = [types.SimpleNamespace(mu=torch.from_numpy(mu).to(dev), log_sigma=torch.from_numpy(ls).to(dev))
             for mu, ls in c['heads']]
    allpi = torch.from_numpy(c['pi']).to(dev)
    return heads, allpi, [allpi[:, j * G:(j + 1) * G] for j in range(3)]


@functools.lru_cache(maxsize=None)
def _kernel(G, dev):
    """one launch: medians and draws of the three heads, six hypotheses"""
    from pose2room_amd.p2rnet import mdn_sample_op
    heads, _, pis = _inputs(G, dev)
    return mdn_sample_op.sample(heads, pis, COUNTS, cases.SEED, h_offset=cases.H_OFFSET, readout='median',
                                return_draws=True)


def _lower_median(draws, counts):
    """draws (H, ..., Nmax, D) -> (H, ..., D): torch.sort of each hypothesis' n draws at (n - 1) // 2"""
    return torch.stack([torch.sort(draws[h][..., :n, :], dim=-2).values[..., (n - 1) // 2, :] for h, n in enumerate(counts)])


@pytest.mark.parametrize("G", cases.GS)
def test_draws_match_mirror(dev, G):
    from pose2room_amd.p2rnet import mdn_sample_op
    _, draws = _kernel(G, dev)
    c = cases.case(G)
    for j, d in enumerate(draws):
        D = c['heads'][j][0].shape[1]
        assert d.shape == (len(COUNTS), cases.B, cases.L, max(COUNTS), D)
        # a flipped gate moves a draw by a whole component, far beyond this tolerance: the gate decisions are the mirror's
        _assert_mirror(d, c['draws'][j], c['heads'][j][0].dtype == np.float64)
        for h, n in enumerate(COUNTS):
            assert not bool(d[h, :, :, n:].any()), (j, h)
            assert bool((d[h, :, :, :n] != 0).any())
    # the same draws beside the mean read-out
    heads, _, pis = _inputs(G, dev)
    _, again = mdn_sample_op.sample(heads, pis, COUNTS, cases.SEED, h_offset=cases.H_OFFSET, return_draws=True)
    for a, b in zip(draws, again):
        assert torch.equal(a, b)


@pytest.mark.parametrize("G", cases.GS)
def test_median(dev, G):
    meds, draws = _kernel(G, dev)
    c = cases.case(G)
    flagged = total = 0
    for j, (m, d) in enumerate(zip(meds, draws)):
        f64 = c['heads'][j][0].dtype == np.float64
        assert m.shape == d.shape[:3] + d.shape[4:] and m.dtype == d.dtype
        for h, n in enumerate(COUNTS):
            # (a) one of the kernel's own draws, bit for bit
            assert bool((d[h, :, :, :n] == m[h].unsqueeze(2)).any(dim=2).all()), (j, h)
            # the library's lower median of them
            assert torch.equal(m[h], torch.median(d[h, :, :, :n], dim=2).values), (j, h)
        # (b) the order statistic of rank (n - 1) // 2
        assert torch.equal(m, _lower_median(d, COUNTS)), j
        assert torch.equal(m[0], d[0, :, :, 0]) and torch.equal(m[1], torch.minimum(d[1, :, :, 0], d[1, :, :, 1]))
        # (c) the mirror's median; where its neighbouring order statistics are within the tolerance, one of the three
        below, want, above = cases.order_stats(c['draws'][j], COUNTS)
        assert np.array_equal(want, c['median'][j])
        flags = c['flags'][j]
        got = m.cpu().numpy()
        want = want.copy()
        for alt in (below, above):
            closer = flags & ~np.isnan(alt) & (np.abs(got - alt) < np.abs(got - want))
            want[closer] = alt[closer]
        _assert_mirror(m, want, f64)
        flagged += int(flags.sum())
        total += flags.size
    assert flagged <= 0.01 * total, (flagged, total)


def _raw_heads(heads, pis, outs, draws, ex=True):
    from pose2room_amd import _lib
    from pose2room_amd.p2rnet.mdn_sample_op import _SampleHead, _SampleHeadEx
    hs = []
    for j, (h, p, o) in enumerate(zip(heads, pis, outs)):
        kw = dict(pi=_lib.ptr(p), log_sigma=_lib.ptr(h.log_sigma), mu=_lib.ptr(h.mu), out=_lib.ptr(o), D=h.mu.shape[1],
                  f64=int(h.mu.dtype == torch.float64), head_id=j)
        if ex:
            kw['draws'] = _lib.ptr(draws[j] if draws else None)
        hs.append((_SampleHeadEx if ex else _SampleHead)(**kw))
    return (type(hs[0]) * len(hs))(*hs)


def _call_ex(dev, arr, nheads, B, G, L, ctot, counts, seed, readout, n_max, h_off=0):
    from pose2room_amd import _lib
    c = (ctypes.c_int * len(counts))(*counts)
    st = _lib.lib().p2r_mdn_sample_ex(nheads, arr, B, G, L, ctot, len(counts), c, ctypes.c_ulonglong(seed), h_off, readout,
                                      n_max, _lib.current_stream(dev))
    torch.cuda.synchronize(dev)
    return st


@pytest.mark.parametrize("n", [1, 7, 99])
def test_mean_through_ex_is_byte_identical(dev, n):
    """p2r_mdn_sample_ex with the mean read-out against p2r_mdn_sample: without a draws pointer (the old kernel) and with
    one (the mean beside the per-draw sums in the new kernel)."""
    from pose2room_amd.p2rnet import mdn_sample_op
    B, G, L = 3, 100, 37
    heads = _heads(G, dev)
    _, pis = _pis(B, G, L, 3, dev)
    ns = [n, max(1, n // 2), n]
    seed = 0x0123456789abcdef
    want = mdn_sample_op.sample(heads, pis, ns, seed, h_offset=5)
    outs = [torch.full_like(w, float('nan')) for w in want]
    assert _call_ex(dev, _raw_heads(heads, pis, outs, None), 3, B, G, L, 3 * G, ns, seed, 0, 0, h_off=5) == 0
    for o, w in zip(outs, want):
        assert torch.equal(o, w)
    got, draws = mdn_sample_op.sample(heads, pis, ns, seed, h_offset=5, return_draws=True)
    for o, w, d in zip(got, want, draws):
        assert torch.equal(o, w)
        assert d.shape[3] == n and bool(torch.isfinite(d).all())


def test_stream_independence(dev):
    from pose2room_amd.p2rnet import mdn_sample_op
    B, G, L = 2, 24, 25
    heads = _heads(G, dev, seed=3)
    allpi, pis = _pis(B, G, L, 3, dev, seed=4)
    ns = [5, 17, 2, 33]
    kw = dict(readout='median', return_draws=True)
    m, d = mdn_sample_op.sample(heads, pis, ns, 77, **kw)
    m0, d0 = mdn_sample_op.sample(heads, pis, ns[:2], 77, **kw)
    m1, d1 = mdn_sample_op.sample(heads, pis, ns[2:], 77, h_offset=2, **kw)
    mc, dc = mdn_sample_op.sample(heads, [p.contiguous() for p in pis], ns, 77, **kw)
    assert pis[0].stride(0) == 3 * G * L and not pis[1].is_contiguous()
    for j in range(3):
        assert torch.equal(m[j], torch.cat([m0[j], m1[j]]))
        assert torch.equal(d[j][:2, :, :, :17], d0[j]) and torch.equal(d[j][2:], d1[j])
        assert torch.equal(m[j], mc[j]) and torch.equal(d[j], dc[j])
    # a head alone under its own stream index; medians without the draws output
    ma = mdn_sample_op.sample(heads[2:], pis[2:], ns, 77, head_ids=[2], readout='median')[0]
    assert torch.equal(ma, m[2])
    other = mdn_sample_op.sample(heads, pis, ns, 78, readout='median')
    assert not torch.equal(other[0], m[0])


def test_dimension_passes(dev):
    """D = 4 in f64 with more than 128 draws does not fit the 64 KiB of per-draw values: the kernel takes the dimensions
    in two passes and draws again -- the same values as the mirror's, the mean as the plain sampler's."""
    from pose2room_amd.p2rnet import mdn_sample_op
    B, G, L = 1, 4, 5
    heads = _heads(G, dev, seed=8, dims=((4, torch.float64), (4, torch.float32)))
    _, pis = _pis(B, G, L, 2, dev, seed=9)
    ns, seed = [200, 130, 3], 99
    med, draws = mdn_sample_op.sample(heads, pis, ns, seed, readout='median', return_draws=True)
    mean, draws2 = mdn_sample_op.sample(heads, pis, ns, seed, return_draws=True)
    plain = mdn_sample_op.sample(heads, pis, ns, seed)
    from pose2room_amd.p2rnet.mdn_sample_op import sample_reference
    for j, h in enumerate(heads):
        f64 = h.mu.dtype == torch.float64
        wm, wd = sample_reference(pis[j].cpu().numpy(), h.mu.cpu().numpy(), h.log_sigma.cpu().numpy(), ns, seed, 0, j,
                                  readout='median', return_draws=True)
        _assert_mirror(draws[j], wd, f64)
        _assert_mirror(med[j], wm, f64)
        assert torch.equal(med[j], _lower_median(draws[j], ns))
        assert torch.equal(draws[j], draws2[j]) and torch.equal(mean[j], plain[j])
        for i, n in enumerate(ns):
            assert not bool(draws[j][i, :, :, n:].any())


def test_memory_contract_and_rejections(dev):
    """out and draws in poisoned buffers between guard bands: every element written, no byte of a band changed; bad
    arguments come back as P2R_EINVAL before anything is launched."""
    B, G, L, H = 2, 50, 21, 3
    heads = _heads(G, dev, seed=21)
    _, pis = _pis(B, G, L, 3, dev, seed=22)
    ns, n_max, EINVAL = [4, 1, 9], 12, -22

    def buffers():
        outs = [memguard.guarded((H, B, L, h.mu.shape[1]), h.mu.dtype, dev) for h in heads]
        draws = [memguard.guarded((H, B, L, n_max, h.mu.shape[1]), h.mu.dtype, dev) for h in heads]
        return outs, draws

    def intact(pairs):
        return all(int(memguard.halo_damage(buf, view, 'poison')) == 0 for buf, view in pairs)

    results = {}
    for readout in (0, 1):
        outs, draws = buffers()
        arr = _raw_heads(heads, pis, [v for _, v in outs], [v for _, v in draws])
        assert _call_ex(dev, arr, 3, B, G, L, 3 * G, ns, 31, readout, n_max) == 0
        assert intact(outs + draws), "written outside"
        for _, v in outs + draws:
            assert int(memguard.poison_count(v)) == 0, "not filled completely"
        for _, v in draws:
            for h, n in enumerate(ns):
                assert not bool(v[h, :, :, n:].any())
        results[readout] = ([v for _, v in outs], [v for _, v in draws])
    from pose2room_amd.p2rnet import mdn_sample_op
    for o, w in zip(results[0][0], mdn_sample_op.sample(heads, pis, ns, 31)):
        assert torch.equal(o, w)
    for j in range(3):
        assert torch.equal(results[0][1][j], results[1][1][j])
        assert torch.equal(results[1][0][j], _lower_median(results[1][1][j], ns))
    # a draws pointer on one head only: the others' outputs all the same
    outs, draws = buffers()
    arr = _raw_heads(heads, pis, [v for _, v in outs], [None, draws[1][1], None])
    assert _call_ex(dev, arr, 3, B, G, L, 3 * G, ns, 31, 1, n_max) == 0
    assert intact(outs + draws)
    for j in range(3):
        assert torch.equal(outs[j][1], results[1][0][j])
        assert int(memguard.poison_count(draws[j][1])) == (0 if j == 1 else draws[j][1].numel())
    assert torch.equal(draws[1][1], results[1][1][1])
    # refused: nothing launched, nothing written
    outs, draws = buffers()
    arr = _raw_heads(heads, pis, [v for _, v in outs], [v for _, v in draws])
    nodraws = _raw_heads(heads, pis, [v for _, v in outs], None)
    assert _call_ex(dev, arr, 3, B, G, L, 3 * G, ns, 31, 7, n_max) == EINVAL
    assert _call_ex(dev, arr, 3, B, G, L, 3 * G, ns, 31, -1, n_max) == EINVAL
    assert _call_ex(dev, arr, 3, B, G, L, 3 * G, ns, 31, 1, 8) == EINVAL            # n_max below a count of 9
    assert _call_ex(dev, arr, 3, B, G, L, 3 * G, ns, 31, 0, 0) == EINVAL
    assert _call_ex(dev, arr, 3, B, G, L, 3 * G, ns, 31, 1, 257) == EINVAL
    assert _call_ex(dev, nodraws, 3, B, G, L, 3 * G, ns, 31, 1, 257) == EINVAL
    assert _call_ex(dev, arr, 3, B, G, L, 3 * G, [4, 0, 9], 31, 1, n_max) == EINVAL
    assert _call_ex(dev, arr, 3, B, 257, L, 3 * 257, ns, 31, 1, n_max) == EINVAL
    assert _call_ex(dev, arr, 4, B, G, L, 3 * G, ns, 31, 1, n_max) == EINVAL
    assert intact(outs + draws)
    for _, v in outs + draws:
        assert int(memguard.poison_count(v)) == v.numel()
    with pytest.raises(ValueError, match="'mean' or 'median'"):
        mdn_sample_op.sample(heads, pis, ns, 31, readout='mode')


# ----------------------------------------------------------------------------------------------------------------------
# the model surface
# ----------------------------------------------------------------------------------------------------------------------
KEYS = ('center', 'size', 'heading')


@functools.lru_cache(maxsize=None)
def _model(dev):
    from pose2room_amd.p2rnet.synthetic import make_batch
    net, cfg = _net(dev)
    return net, cfg, make_batch(2, 1024, seed=4242, device=dev)


def _check_hypotheses(hyps, ns, medians):
    """every head named in `medians` returns the lower median of its returned draws, bit for bit"""
    for h, (ep, _, _) in enumerate(hyps):
        assert set(ep['draws']) == set(KEYS)
        for k in KEYS:
            d = ep['draws'][k]
            assert d.shape == ep[k].shape[:2] + (ns[h],) + ep[k].shape[2:] and d.dtype == ep[k].dtype, k
            if k in medians:
                med = torch.sort(d, dim=2).values[:, :, (ns[h] - 1) // 2]
                assert torch.equal(ep[k], ep['aggregated_vote_xyz'] + med if k == 'center' else med), (h, k)


def test_generate_hypotheses_median_end_to_end(dev):
    from pose2room_amd.net_utils.ap_helper import parse_predictions
    net, cfg, data = _model(dev)
    ns = [1, 4, 9]
    with torch.no_grad():
        hyps = net.generate_hypotheses(data, 3, n_samples=ns, seed=11, central_tendency='median', return_draws=True)
        mean = net.generate_hypotheses(data, 3, n_samples=ns, seed=11)
        mean_d = net.generate_hypotheses(data, 3, n_samples=ns, seed=11, central_tendency='mean', return_draws=True)
    assert len(hyps) == 3 and all(len(t) == 3 for t in hyps)
    _check_hypotheses(hyps, ns, KEYS)
    for h, ((ep, eval_dict, parsed), (em, _, _), (ed, _, _)) in enumerate(zip(hyps, mean, mean_d)):
        assert 'draws' not in em
        for k in KEYS:
            assert torch.equal(ep['pi'][k], em['pi'][k]), k
            assert torch.equal(ed[k], em[k]) and torch.equal(ed['draws'][k], ep['draws'][k]), k
            if ns[h] > 2:
                assert not torch.equal(ep[k], em[k]), k
        for k in ('objectness_scores', 'sem_cls_scores', 'aggregated_vote_xyz', 'aggregated_vote_inds', 'vote_xyz'):
            assert torch.equal(ep[k], em[k]), k
        alone_eval, alone = parse_predictions(ep, data, cfg.eval_config)
        assert np.array_equal(eval_dict['pred_mask'], alone_eval['pred_mask'])
        assert np.array_equal(parsed['pred_corners_3d'], alone['pred_corners_3d'])
        assert len(eval_dict['batch_pred_map_cls']) == 2 and len(eval_dict['batch_gt_map_cls']) == 2
    # one draw: mean and median are that draw
    for k in KEYS:
        assert torch.equal(hyps[0][0][k], mean[0][0][k])
    with pytest.raises(ValueError, match="'mean' or 'median'"):
        net.generate_hypotheses(data, 2, n_samples=2, seed=1, central_tendency='mode')


@pytest.mark.parametrize("which", [KEYS, ('size',)])
def test_generate_hypotheses_reads_the_heads_setting(dev, which):
    """heads configured with 'median' (all of them, or the size head alone beside two 'mean' heads) are read out so when
    the call does not say otherwise; the modules are left as they were"""
    net, cfg, data = _model(dev)
    gm = dict(zip(KEYS, (net.detection.gmm_center.mdn, net.detection.gmm_size.mdn, net.detection.gmm_heading.mdn)))
    ns, seed = [1, 4, 9], 11
    try:
        for k in which:
            gm[k].hparams.central_tendency = 'median'
        with torch.no_grad():
            hyps = net.generate_hypotheses(data, 3, n_samples=ns, seed=seed, return_draws=True)
            over = net.generate_hypotheses(data, 3, n_samples=ns, seed=seed, central_tendency='mean')
        assert all(gm[k].hparams.central_tendency == 'median' for k in which)
    finally:
        for k in KEYS:
            gm[k].hparams.central_tendency = 'mean'
    _check_hypotheses(hyps, ns, which)
    from pose2room_amd.p2rnet.mdn_sample_op import sample_reference
    for j, k in enumerate(KEYS):
        pi = hyps[0][0]['pi'][k]
        m = gm[k]
        args = (pi.cpu().numpy(), m.mu.detach().cpu().numpy(), m.log_sigma.detach().cpu().numpy(), ns, seed, 0, j)
        want = sample_reference(*args, readout='median' if k in which else 'mean')
        want_mean = sample_reference(*args)
        for h in range(3):
            off = hyps[h][0]['aggregated_vote_xyz'] if k == 'center' else 0
            _assert_mirror(hyps[h][0][k] - off, want[h], k == 'heading')
            _assert_mirror(over[h][0][k] - off, want_mean[h], k == 'heading')


def test_multi_modal_metrics_median(dev):
    from pose2room_amd.p2rnet import testing
    from pose2room_amd.p2rnet.synthetic import make_batch
    net, cfg, _ = _model(dev)
    batches = [make_batch(4, 1024, seed=4300, device=dev)]
    logged = []
    old, cfg.log_string = cfg.log_string, logged.append
    try:
        out = testing.test_multi_modal(cfg, net, batches, 3, seed=123, ap_device=dev, central_tendency='median')
        ref = testing.test_multi_modal(cfg, net, batches, 3, seed=123, ap_device=dev)
    finally:
        cfg.log_string = old
    thr = cfg.config['test']['ap_iou_thresholds']
    assert out['central_tendency'] == 'median' and ref['central_tendency'] is None
    assert out['best_map'].shape == (len(thr),) and np.all(np.isfinite(out['best_map']))
    assert np.isfinite(out['tmd']) and out['tmd'] >= 1.0
    assert out['n_samples'] == ref['n_samples'] and out['seed'] == ref['seed']
    assert out['tmd'] != ref['tmd']
