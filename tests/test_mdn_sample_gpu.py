"""GPU: Bernoulli-gated mixture sampling (csrc/mdn_sample.hip) and multi-hypothesis generation
(`P2RNet.generate_hypotheses`, `testing.test_multi_modal`)."""
import ctypes
import types

import numpy as np
import pytest
import torch

from tests.test_model_cpu import build

pytestmark = pytest.mark.gpu


def _heads(G, dev, seed=0, dims=((3, torch.float32), (3, torch.float32), (2, torch.float64))):
    g = torch.Generator().manual_seed(seed)
    out = []
    for D, dt in dims:
        mu = torch.randn(G, D, generator=g, dtype=torch.float64).to(dt)
        ls = (torch.rand(G, D, generator=g) * 1.2 - 0.8).float()
        out.append(types.SimpleNamespace(mu=mu.to(dev), log_sigma=ls.to(dev)))
    return out


def _pis(B, G, L, nheads, dev, seed=1):
    """(B, nheads * G, L) mixture weights in one tensor: the heads' pi are channel-strided views of it"""
    g = torch.Generator().manual_seed(seed)
    allpi = torch.sigmoid(torch.randn(B, nheads * G, L, generator=g) * 2).to(dev)
    return allpi, [allpi[:, j * G:(j + 1) * G] for j in range(nheads)]


def _mirror(pi, head, ns, seed, h_offset=0, head_id=0):
    from pose2room_amd.p2rnet.mdn_sample_op import sample_reference
    return sample_reference(pi.detach().cpu().numpy(), head.mu.detach().cpu().numpy(),
                            head.log_sigma.detach().cpu().numpy(), ns, seed,
                            h_offset, head_id)


def _assert_mirror(got, want, f64):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape
    span = max(float(want.max() - want.min()), 1.0)
    err = float(np.abs(got - want).max())
    assert err <= (1e-12 if f64 else 2e-6) * span, (err, span)


@pytest.mark.parametrize("n", [1, 7, 99])
def test_kernel_matches_mirror(dev, n):
    from pose2room_amd.p2rnet import mdn_sample_op
    B, G, L = 3, 100, 37                       # B * L = 111 rows: not a multiple of the 16-row workgroup
    heads = _heads(G, dev)
    _, pis = _pis(B, G, L, 3, dev)
    ns = [n, max(1, n // 2), n]
    seed = 0x0123456789abcdef
    outs = mdn_sample_op.sample(heads, pis, ns, seed, h_offset=5)
    for j, (h, p, o) in enumerate(zip(heads, pis, outs)):
        _assert_mirror(o, _mirror(p, h, ns, seed, h_offset=5, head_id=j), h.mu.dtype == torch.float64)


def test_stream_properties(dev):
    from pose2room_amd.p2rnet import mdn_sample_op
    B, G, L = 2, 24, 40
    heads = _heads(G, dev, seed=3)
    _, pis = _pis(B, G, L, 3, dev, seed=4)
    ns = [3, 1, 8, 5, 2, 9]
    a = mdn_sample_op.sample(heads, pis, ns, 77)
    b = mdn_sample_op.sample(heads, pis, ns, 77)
    first = mdn_sample_op.sample(heads, pis, ns[:2], 77)
    rest = mdn_sample_op.sample(heads, pis, ns[2:], 77, h_offset=2)
    other = mdn_sample_op.sample(heads, pis, ns, 78)
    for j in range(3):
        assert torch.equal(a[j], b[j])                                    # same seed: bit-identical
        assert torch.equal(a[j], torch.cat([first[j], rest[j]]))          # 6 = 2 + 4 with the hypothesis offset
        assert not torch.equal(a[j], other[j])
        for h in range(1, 6):
            assert not torch.equal(a[j][0], a[j][h])                      # hypotheses differ
    # more hypotheses than one launch takes (64): the split over launches does not change a draw
    many = mdn_sample_op.sample(heads[:1], pis[:1], [2] * 70, 5)[0]
    tail = mdn_sample_op.sample(heads[:1], pis[:1], [2] * 3, 5, h_offset=66)[0]
    assert torch.equal(many[66:69], tail)
    # the heading head alone, under its own stream index, draws what it draws beside the others
    alone = mdn_sample_op.sample(heads[2:], pis[2:], ns, 77, head_ids=[2])[0]
    assert torch.equal(alone, a[2])


def _moments_check(samples, pi, mu, sigma, n):
    """samples (H, rows, D) f64; pi (rows, G); mu, sigma (G, D) f64 -> each row's mean and variance over the H
    hypotheses within 5 standard errors of the analytic ones"""
    H = samples.shape[0]
    mean_a = pi @ mu                                                              # (rows, D)
    var_a = (pi @ (mu ** 2 + sigma ** 2) - (pi ** 2) @ (mu ** 2)) / n
    mean_s = samples.mean(0)
    assert np.all(np.abs(mean_s - mean_a) <= 5 * np.sqrt(var_a / H))
    dev_s = samples - mean_s
    var_s = (dev_s ** 2).sum(0) / (H - 1)
    # variance on the log scale (standard error sqrt((kurtosis - 1) / H), kurtosis pooled over the rows): the sample
    # variance's own skew would otherwise put a 5-sigma bound on one side only
    kurt = ((dev_s ** 4).mean(0) / var_s ** 2).mean()
    assert np.all(np.abs(np.log(var_s / var_a)) <= 5 * np.sqrt((kurt - 1) / H))


def _rows(t):
    """(B, G, L) -> (B * L, G) f64"""
    return t.detach().double().cpu().numpy().transpose(0, 2, 1).reshape(-1, t.shape[1])


def test_moments_match_analytic(dev):
    from pose2room_amd.p2rnet import mdn_sample_op
    B, G, L, n, H = 4, 8, 1024, 3, 128
    heads = _heads(G, dev, seed=11)
    _, pis = _pis(B, G, L, 3, dev, seed=12)
    outs = mdn_sample_op.sample(heads, pis, [n] * H, 2024)
    for h, p, o in zip(heads, pis, outs):
        f64 = h.mu.dtype == torch.float64
        sigma = torch.exp(h.log_sigma.double()) if f64 else torch.exp(h.log_sigma).double()
        _moments_check(o.double().cpu().numpy().reshape(H, B * L, -1), _rows(p), h.mu.double().cpu().numpy(),
                       sigma.cpu().numpy(), n)


def test_module_path_moments_match_analytic(dev):
    """The torch-RNG module path (mdn.py generate_point_predictions, sample_pi=True) passes the same check: both
    sample one distribution."""
    from pose2room_amd.p2rnet.config import Struct
    from pose2room_amd.p2rnet.modules.mdn import MixtureDensityHead
    B, G, L, n, H = 1, 8, 64, 3, 256
    torch.manual_seed(5)
    for D, dt in ((3, torch.float32), (2, torch.float64)):
        cfg = Struct(input_dim=4, num_gaussian=G, out_dim=D, mu_bias_init=torch.randn(G, D, dtype=torch.float64).to(dt),
                     n_samples=1, central_tendency='mean')
        mdn = MixtureDensityHead(cfg).to(dev)
        with torch.no_grad():
            mdn.log_sigma.copy_(torch.rand(G, D) * 1.2 - 0.8)
            pi = torch.sigmoid(torch.randn(B, G, L, device=dev) * 2)
            samples = torch.stack([mdn.generate_point_predictions(pi, n, sample_pi=True) for _ in range(H)])  # (H,B,D,L)
        s = samples.double().cpu().numpy().transpose(0, 1, 3, 2).reshape(H, B * L, D)
        _moments_check(s, _rows(pi), mdn.mu.detach().double().cpu().numpy(),
                       torch.exp(mdn.log_sigma.detach()).double().cpu().numpy(), n)


def test_guard_bands_and_rejections(dev):
    from pose2room_amd import _lib
    from pose2room_amd.p2rnet import mdn_sample_op
    from pose2room_amd.p2rnet.mdn_sample_op import _SampleHead
    B, G, L, H = 2, 50, 21, 3
    heads = _heads(G, dev, seed=21)
    _, pis = _pis(B, G, L, 3, dev, seed=22)
    ns = [4, 1, 9]
    want = mdn_sample_op.sample(heads, pis, ns, 31)
    guard, SENT = 1024, -7.77e30
    bufs, hs = [], []
    for j, (h, p) in enumerate(zip(heads, pis)):
        D = h.mu.shape[1]
        buf = torch.full((guard + H * B * L * D + guard,), SENT, dtype=h.mu.dtype, device=dev)
        bufs.append(buf)
        hs.append(_SampleHead(pi=_lib.ptr(p), log_sigma=_lib.ptr(h.log_sigma), mu=_lib.ptr(h.mu),
                              out=ctypes.c_void_p(buf.data_ptr() + guard * buf.element_size()), D=D,
                              f64=int(h.mu.dtype == torch.float64), head_id=j))
    arr = (_SampleHead * 3)(*hs)

    def call(a=arr, nh=3, g=G, ctot=3 * G, counts=ns, h_off=0):
        c = (ctypes.c_int * len(counts))(*counts)
        st = _lib.lib().p2r_mdn_sample(nh, a, B, g, L, ctot, len(counts), c, ctypes.c_ulonglong(31), h_off,
                                       _lib.current_stream(dev))
        torch.cuda.synchronize(dev)
        return st

    assert call() == 0
    for buf, w in zip(bufs, want):
        assert bool((buf[:guard] == SENT).all()) and bool((buf[-guard:] == SENT).all()), "written outside"
        inner = buf[guard:-guard]
        assert not bool((inner == SENT).any()), "not filled completely"
        assert torch.equal(inner, w.reshape(-1))
    # bad arguments: status != 0, nothing launched
    assert call(counts=[0, 1, 2]) != 0 and call(counts=[1, 257, 2]) != 0
    assert call(g=257, ctot=3 * 257) != 0 and call(nh=4) != 0 and call(nh=0) != 0 and call(ctot=G - 1) != 0
    assert call(h_off=-1) != 0
    for field, value in (('D', 5), ('D', 0), ('pi', None), ('mu', None), ('out', None), ('log_sigma', None),
                         ('head_id', 256), ('f64', 2)):
        bad = (_SampleHead * 3)(*hs)
        setattr(bad[1], field, value)
        assert call(a=bad) != 0, field
    for buf in bufs:
        assert bool((buf[:guard] == SENT).all()) and bool((buf[-guard:] == SENT).all())
    # the wrapper turns them into RuntimeError; CPU tensors are refused
    with pytest.raises(RuntimeError):
        mdn_sample_op.sample(heads, pis, [0], 1)
    with pytest.raises(RuntimeError):
        mdn_sample_op.sample(heads, pis, [300], 1)
    with pytest.raises(RuntimeError):
        mdn_sample_op.sample(heads, [p.cpu() for p in pis], [2], 1)
    wide = _heads(257, dev, seed=3)
    _, wpis = _pis(1, 257, 4, 3, dev)
    with pytest.raises(RuntimeError):
        mdn_sample_op.sample(wide, wpis, [2], 1)
    five = [types.SimpleNamespace(mu=torch.zeros(G, 5, device=dev), log_sigma=torch.zeros(G, 5, device=dev))]
    with pytest.raises(RuntimeError):
        mdn_sample_op.sample(five, pis[:1], [2], 1)


def _net(dev, T=1024):
    net, cfg = build('test', T, device=dev)
    return net.to(dev).eval(), cfg


def test_generate_hypotheses_end_to_end(dev, mathmode):
    from pose2room_amd.net_utils.ap_helper import parse_predictions
    from pose2room_amd.p2rnet.synthetic import make_batch
    net, cfg = _net(dev)
    data = make_batch(4, 1024, seed=4242, device=dev)
    ns, seed = [2, 5, 3], 0xfeedface12345678
    with torch.no_grad():
        ref = net.generate_end_points(data)
        hyps = net.generate_hypotheses(data, 3, n_samples=ns, seed=seed)
    assert len(hyps) == 3
    ep0 = hyps[0][0]
    for k in ('center', 'size', 'heading'):
        assert torch.equal(ep0['pi'][k], ref['pi'][k]), k
    for k in ('objectness_scores', 'sem_cls_scores', 'aggregated_vote_xyz', 'aggregated_vote_inds'):
        assert torch.equal(ep0[k], ref[k]), k
    gm = [net.detection.gmm_center.mdn, net.detection.gmm_size.mdn, net.detection.gmm_heading.mdn]
    mir = [_mirror(ref['pi'][k], m, ns, seed, head_id=j) for j, (k, m) in enumerate(zip(('center', 'size', 'heading'), gm))]
    agg = ref['aggregated_vote_xyz'].cpu().numpy()
    for h, (ep, eval_dict, parsed) in enumerate(hyps):
        assert set(ep) >= set(ref)
        for k in ('center', 'size', 'heading'):
            assert ep[k].shape == ref[k].shape and ep[k].dtype == ref[k].dtype, k
        _assert_mirror(ep['center'] - ep['aggregated_vote_xyz'], mir[0][h], False)
        np.testing.assert_allclose(ep['center'].cpu().numpy(), agg + mir[0][h], rtol=0, atol=1e-4)
        _assert_mirror(ep['size'], mir[1][h], False)
        _assert_mirror(ep['heading'], mir[2][h], True)
        alone_eval, alone = parse_predictions(ep, data, cfg.eval_config)
        assert np.array_equal(eval_dict['pred_mask'], alone_eval['pred_mask'])
        for k in ('pred_corners_3d', 'obj_prob', 'pred_sem_cls', 'sem_cls_probs'):
            assert np.array_equal(parsed[k], alone[k]), k
        assert len(eval_dict['batch_pred_map_cls']) == 4 and len(eval_dict['batch_gt_map_cls']) == 4
    # reproducible from torch's seed; the trunk's end points shared, not recomputed
    torch.manual_seed(9)
    with torch.no_grad():
        a = net.generate_hypotheses(data, 2, eval=False)
    torch.manual_seed(9)
    with torch.no_grad():
        b = net.generate_hypotheses(data, 2, eval=False)
    for (ea, da, pa), (eb, db, pb) in zip(a, b):
        assert torch.equal(ea['center'], eb['center']) and np.array_equal(da['pred_mask'], db['pred_mask'])
        assert 'batch_gt_map_cls' not in da
    assert a[0][0]['vote_features'] is a[1][0]['vote_features']


def test_generate_hypotheses_module_heads(dev):
    """The trunk on the module chain (fused heads switched off) samples the same mixture weights' stream."""
    from pose2room_amd.p2rnet.modules import proposal_net
    from pose2room_amd.p2rnet.synthetic import make_batch
    net, cfg = _net(dev, 256)
    data = make_batch(2, 256, seed=77, device=dev)
    old = proposal_net.USE_FUSED_HEADS
    proposal_net.USE_FUSED_HEADS = False
    try:
        with torch.no_grad():
            ref = net.generate_end_points(data)
            hyps = net.generate_hypotheses(data, 2, n_samples=4, seed=3)
    finally:
        proposal_net.USE_FUSED_HEADS = old
    gm = [net.detection.gmm_center.mdn, net.detection.gmm_size.mdn, net.detection.gmm_heading.mdn]
    for j, k in enumerate(('center', 'size', 'heading')):
        pi = hyps[0][0]['pi'][k]
        assert torch.allclose(pi, ref['pi'][k], rtol=1e-5, atol=1e-6)
        mir = _mirror(pi, gm[j], [4, 4], 3, head_id=j)
        got = hyps[1][0][k] - (hyps[1][0]['aggregated_vote_xyz'] if k == 'center' else 0)
        _assert_mirror(got, mir[1], k == 'heading')


def test_multi_modal_metrics(dev, mathmode):
    from pose2room_amd.p2rnet import testing
    from pose2room_amd.p2rnet.synthetic import make_batch
    net, cfg = _net(dev)
    batches = [make_batch(4, 1024, seed=4300 + i, device=dev) for i in range(2)]
    logged = []
    cfg.log_string = logged.append
    out = testing.test_multi_modal(cfg, net, batches, 4, seed=123, ap_device=dev)
    thr = cfg.config['test']['ap_iou_thresholds']
    assert out['best_map'].shape == (len(thr),) and np.all(np.isfinite(out['best_map']))
    assert len(out['metrics']) == 4 and all(len(row) == len(thr) for row in out['metrics'])
    for row in out['metrics']:
        for t, m in enumerate(row):
            assert out['best_map'][t] >= m['mAP']
    assert np.isfinite(out['tmd']) and out['tmd'] >= 1.0
    assert len(out['n_samples']) == 4 and all(1 <= n <= 99 for n in out['n_samples'])
    assert any('TMD' in s for s in logged)
