"""CPU: the NumPy mirror of the sampler's read-outs (`mdn_sample_op.sample_reference`: median, per-draw samples) and the
median-gap condition the GPU tests of tests/test_mdn_readout_gpu.py rely on."""
import os

import numpy as np
import pytest
import torch

from tests import mdn_readout_cases as cases

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g12_mdn_readout.npz')


def _golden_head(z, tag):
    return dict(pi=z[f'{tag}_pi'], mu=z[f'{tag}_mu'], log_sigma=z[f'{tag}_log_sigma'], n_samples=z['n_samples'].tolist(),
                seed=int(z[f'{tag}_seed']), h_offset=int(z[f'{tag}_h_offset']), head_id=int(z[f'{tag}_head_id']))


@pytest.mark.parametrize("tag", ['f32', 'f64'])
def test_mirror_median_is_the_lower_median_of_its_draws(tag):
    """B = 2, L = 9, G = 5, a (3, f32) and a (2, f64) head, n = 1, 2, 7, 16 (golden/make_mdn_readout_golden.py)"""
    from pose2room_amd.p2rnet.mdn_sample_op import sample_reference
    z = np.load(GOLD)
    kw = _golden_head(z, tag)
    ns = kw['n_samples']
    assert ns == [1, 2, 7, 16] and kw['pi'].shape == (2, 5, 9)
    med, draws = sample_reference(**kw, readout='median', return_draws=True)
    mean, draws2 = sample_reference(**kw, return_draws=True)
    assert med.dtype == draws.dtype == kw['mu'].dtype and draws.shape == (4, 2, 9, 16, kw['mu'].shape[1])
    assert np.array_equal(draws, draws2)
    assert np.array_equal(med, sample_reference(**kw, readout='median'))
    for h, n in enumerate(ns):
        assert np.array_equal(med[h], np.sort(draws[h, :, :, :n], axis=2)[:, :, (n - 1) // 2])
        assert not np.any(draws[h, :, :, n:]) and np.any(draws[h, :, :, :n])
        # a draw is the double sum over g rounded once; the mean adds the unrounded sums: equal to a rounding of each draw
        approx = draws[h, :, :, :n].astype(np.float64).mean(axis=2)
        np.testing.assert_allclose(mean[h], approx, rtol=0, atol=16 * np.finfo(med.dtype).eps * np.abs(draws[h]).max())
    assert np.array_equal(med[0], draws[0, :, :, 0]) and np.array_equal(med[1], draws[1, :, :, :2].min(axis=2))
    # the 'mean' mirror is what it was before the read-outs existed, byte for byte
    assert mean.dtype == z[f'{tag}_mean'].dtype and mean.tobytes() == z[f'{tag}_mean'].tobytes()
    assert sample_reference(**kw).tobytes() == z[f'{tag}_mean'].tobytes()


def test_golden_inputs_come_from_their_seeds():
    z = np.load(GOLD)
    for tag, D, dt in (('f32', 3, np.float32), ('f64', 2, np.float64)):
        rng = np.random.default_rng(int(z[f'{tag}_input_seed']))
        assert np.array_equal(rng.random((2, 5, 9)).astype(np.float32), z[f'{tag}_pi'])
        assert np.array_equal(rng.standard_normal((5, D)).astype(dt), z[f'{tag}_mu'])


def test_unknown_readout_is_refused():
    from pose2room_amd.p2rnet.mdn_sample_op import sample_reference
    with pytest.raises(ValueError, match="'mean' or 'median'"):
        sample_reference(np.zeros((1, 2, 3), np.float32), np.zeros((2, 2), np.float32), np.zeros((2, 2), np.float32), [2], 1,
                         readout='mode')


def test_gap_tolerance_is_the_mirror_tolerance():
    """`cases.mirror_tolerance` restates the bound of `_assert_mirror` (the gap rule needs it per element): an error just
    inside it passes, one just outside fails."""
    from tests.test_mdn_sample_gpu import _assert_mirror
    for f64, dt in ((False, np.float32), (True, np.float64)):
        for span in (0.5, 37.0):
            want = np.linspace(0.0, span, 11).astype(dt)
            tol = cases.mirror_tolerance(want, f64)
            assert tol == cases.MIRROR_RTOL[f64] * max(span, 1.0)
            for scale, ok in ((0.9, True), (1.1, False)):
                got = want.copy()
                got[5] += dt(scale * tol)
                if ok:
                    _assert_mirror(torch.from_numpy(got), want, f64)
                else:
                    with pytest.raises(AssertionError):
                        _assert_mirror(torch.from_numpy(got), want, f64)


@pytest.mark.parametrize("G", cases.GS)
def test_median_gap_condition(G):
    """For the inputs and seed of the GPU tests: the share of outputs whose median order statistic has a neighbouring
    order statistic within the comparison tolerance is at most 1 %, so the exception the GPU test grants those elements
    cannot hide a wrong rank."""
    c = cases.case(G)
    flagged = total = 0
    for j, ((mu, _), med, draws, flags) in enumerate(zip(c['heads'], c['median'], c['draws'], c['flags'])):
        f64 = mu.dtype == np.float64
        assert flags.shape == med.shape == (len(cases.COUNTS), cases.B, cases.L, mu.shape[1])
        assert not flags[0].any()                                   # n = 1: no neighbour
        # the rule as stated, written out for one hypothesis: n = 7, ranks 2, 3, 4
        srt = np.sort(draws[2, :, :, :7], axis=2)
        tol = cases.mirror_tolerance(med, f64)
        want = (np.abs(srt[:, :, 3] - srt[:, :, 2]) <= tol) | (np.abs(srt[:, :, 4] - srt[:, :, 3]) <= tol)
        assert np.array_equal(flags[2], want) and np.array_equal(med[2], srt[:, :, 3])
        print(f"G={G} head {j}: {int(flags.sum())} of {flags.size} flagged")
        flagged += int(flags.sum())
        total += flags.size
    assert flagged <= 0.01 * total, (flagged, total)


def test_gap_rule_sees_a_close_neighbour():
    draws = np.zeros((2, 1, 1, 4, 1), dtype=np.float32)
    draws[0, 0, 0, :, 0] = [3.0, 1.0, 1.0 + 1e-6, 2.0]              # sorted 1, 1 + 1e-6, 2, 3: rank 1 next to rank 0
    draws[1, 0, 0, :3, 0] = [5.0, 1.0, 3.0]
    flags = cases.gap_flags(draws, [4, 3], False)
    assert flags[:, 0, 0, 0].tolist() == [True, False]
    below, med, above = cases.order_stats(draws, [4, 3])
    assert med[:, 0, 0, 0].tolist() == [np.float32(1.0 + 1e-6), 3.0] and above[1, 0, 0, 0] == 5.0 and below[1, 0, 0, 0] == 1.0


def test_central_tendency_config_and_errors():
    """`generation.central_tendency` reaches the heads' hparams; absent, they stay 'mean' (the model every existing
    config builds); `generate_hypotheses` refuses anything but the two read-outs before it computes."""
    from pose2room_amd.p2rnet import P2RConfig, default_config, METHODS
    nets = {}
    for ct in (None, 'median'):
        conf = default_config('test', data={'num_frames': 64})
        if ct is not None:
            conf['generation'] = {'central_tendency': ct}
        torch.manual_seed(0)
        np.random.seed(0)
        nets[ct] = METHODS.get('P2RNet')(P2RConfig(conf, device='cpu'))
    for ct, net in nets.items():
        for gm in (net.detection.gmm_center, net.detection.gmm_size, net.detection.gmm_heading):
            assert gm.mdn.hparams.central_tendency == (ct or 'mean')
    sd0, sd1 = nets[None].state_dict(), nets['median'].state_dict()
    assert list(sd0) == list(sd1) and all(torch.equal(sd0[k], sd1[k]) for k in sd0)
    with pytest.raises(ValueError, match="'mean' or 'median'"):
        nets[None].detection.generate_hypotheses(None, None, {}, 1, [1], 0, central_tendency='mode')
    nets[None].detection.gmm_size.mdn.hparams.central_tendency = 'mode'
    with pytest.raises(ValueError, match="'mean' or 'median'"):
        nets[None].detection.generate_hypotheses(None, None, {}, 1, [1], 0)
