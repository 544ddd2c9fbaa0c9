"""Multi-hypothesis generation, host side: the Philox stream's mirror against the Random123 known answers, and the
multi-modal evaluation (dump-record box parameters, TMD, best-of-N mAP) against the reference (g11)."""
import os

import numpy as np
import pytest

G11 = os.path.join(os.path.dirname(__file__), 'golden', 'g11_multimodal.npz')


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    from pose2room_amd.p2rnet.mdn_sample_op import philox4x32_10
    got = philox4x32_10([np.uint32(c) for c in ctr], [np.uint32(k) for k in key])
    assert tuple(int(v) for v in got) == want


def test_philox_vectorised_matches_scalar():
    from pose2room_amd.p2rnet.mdn_sample_op import philox4x32_10
    rng = np.random.default_rng(3)
    c = rng.integers(0, 2 ** 32, (4, 50), dtype=np.uint64).astype(np.uint32)
    k = rng.integers(0, 2 ** 32, 2, dtype=np.uint64).astype(np.uint32)
    vec = philox4x32_10(list(c), list(k))
    for i in (0, 17, 49):
        one = philox4x32_10([c[j, i] for j in range(4)], list(k))
        assert [int(v[i]) for v in vec] == [int(v) for v in one]


def test_mirror_stream_properties():
    """The mirror alone: gate decisions follow pi, hypotheses differ, h_offset only shifts the stream index."""
    from pose2room_amd.p2rnet.mdn_sample_op import sample_reference
    rng = np.random.default_rng(5)
    B, G, L = 2, 6, 5
    pi = rng.uniform(0, 1, (B, G, L)).astype(np.float32)
    mu = rng.normal(0, 1, (G, 3)).astype(np.float32)
    ls = rng.normal(0, 0.3, (G, 3)).astype(np.float32)
    a = sample_reference(pi, mu, ls, [3, 4, 5], seed=99)
    b = sample_reference(pi, mu, ls, [5], seed=99, h_offset=2)
    assert np.array_equal(a[2], b[0])
    assert not np.array_equal(a[0], a[1])
    zero = sample_reference(np.zeros_like(pi), mu, ls, [4], seed=99)
    assert np.array_equal(zero, np.zeros_like(zero))
    one = sample_reference(np.ones_like(pi), mu, np.full_like(ls, -30.0), [4], seed=99)   # every gate open, sigma ~ 0
    np.testing.assert_allclose(one[0], np.broadcast_to(mu.sum(0), (B, L, 3)), rtol=1e-5)


def test_resolve_draws_defaults():
    import torch
    from pose2room_amd.p2rnet.mdn_sample_op import resolve_draws
    torch.manual_seed(7)
    s1, n1 = resolve_draws(10)
    torch.manual_seed(7)
    s2, n2 = resolve_draws(10)
    assert (s1, n1) == (s2, n2) and 0 <= s1 < 2 ** 64 and len(n1) == 10 and all(1 <= n <= 99 for n in n1)
    assert resolve_draws(3, 7, seed=-1) == (2 ** 64 - 1, [7, 7, 7])
    assert resolve_draws(2, [1, 256], seed=5)[1] == [1, 256]
    for bad in ([0, 1], [1, 257], [1, 2, 3]):
        with pytest.raises(ValueError):
            resolve_draws(2, bad, seed=5)


def test_corners_to_params_matches_reference():
    from pose2room_amd.net_utils.multi_modal_eval import corners_to_params, params_to_corners
    z = np.load(G11)
    got = corners_to_params(z['a_corners'])
    np.testing.assert_allclose(got, z['a_params'], rtol=0, atol=1e-9)
    # the round trip the TMD relies on: params -> corners in the reference's order
    np.testing.assert_allclose(params_to_corners(got), z['a_corners'], rtol=0, atol=1e-9)


def _records(z):
    runs = sorted({int(k.split('_')[2]) for k in z.files if k.startswith('b_obbs_')})
    samples = sorted({int(k.split('_')[3]) for k in z.files if k.startswith('b_obbs_')})
    return [[{'obbs': z[f'b_obbs_{r}_{s}'], 'cls': z[f'b_cls_{r}_{s}'], 'inst_idx': z[f'b_inst_{r}_{s}']}
             for s in samples] for r in runs]


def test_tmd_and_best_of_n_match_reference_script():
    from pose2room_amd.net_utils.multi_modal_eval import tmd, best_of_n_map
    z = np.load(G11)
    assert tmd(_records(z)) == pytest.approx(float(z['b_tmd'][0]), rel=0, abs=1e-9)
    np.testing.assert_allclose(best_of_n_map(z['b_map']), z['b_best_map'], rtol=0, atol=1e-9)
    dicts = [[{'mAP': v} for v in row] for row in z['b_map']]
    np.testing.assert_allclose(best_of_n_map(dicts), z['b_best_map'], rtol=0, atol=1e-9)


def test_tmd_of_identical_runs_is_one():
    from pose2room_amd.net_utils.multi_modal_eval import tmd
    z = np.load(G11)
    recs = _records(z)
    assert tmd([recs[0]] * 4) == pytest.approx(1.0, abs=1e-12)


def test_confident_boxes_rule():
    from pose2room_amd.net_utils.multi_modal_eval import confident_boxes
    z = np.load(G11)
    corners = z['a_corners'][:40].reshape(2, 20, 8, 3)
    rng = np.random.default_rng(2)
    obj = rng.uniform(0, 1, (2, 20)).astype(np.float32)
    mask = (rng.random((2, 20)) < 0.6).astype(np.uint8)
    cls = rng.integers(0, 17, (2, 20))
    recs = confident_boxes({}, {'pred_mask': mask}, {'pred_corners_3d': corners, 'obj_prob': obj,
                                                     'pred_sem_cls': cls}, 0.5)
    params = z['a_params'][:40].reshape(2, 20, 7)
    for b, rec in enumerate(recs):
        keep = (obj[b] > 0.5) & (mask[b] == 1)
        assert rec['inst_idx'].dtype == bool and np.array_equal(rec['inst_idx'], keep)
        np.testing.assert_allclose(rec['obbs'], params[b][keep], rtol=0, atol=1e-9)
        assert np.array_equal(rec['cls'], cls[b][keep])
