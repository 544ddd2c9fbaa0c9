"""GPU: vote labels derived on the device (csrc/vote_labels.hip) equal, bit for bit, the reference's own get_votes
(G13) and the NumPy mirror; a store built from samples without votes equals one built from the mirror's votes; the lean
store (no votes, derived in the assemble launch) yields the batches of the full store and of the host loader.  Outputs
are allocated inside poisoned guard bands (tests/memguard.py): an element never written or a store outside shows."""
import random

import numpy as np
import pytest
import torch

from pose2room_amd.net_utils import vote_labels as vl
from pose2room_amd.p2rnet import dataloader as dl
from pose2room_amd.p2rnet import device_loader as dv
from tests import memguard, vote_cases
from tests.test_device_loader_gpu import KEYS, assert_same_batch

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64).cpu()


def _packed(joints_list, dev):
    t0 = np.asarray([j.shape[0] for j in joints_list], np.int32)
    off = np.zeros(len(t0), np.int64)
    off[1:] = np.cumsum(t0)[:-1]
    return (torch.from_numpy(np.concatenate(joints_list)).to(dev), torch.from_numpy(off).to(dev),
            torch.from_numpy(t0).to(dev))


def _kernel_votes(joints_list, tables, dev):
    """one p2r_vote_labels launch into a poisoned, guarded output"""
    joints, off, n = _packed(joints_list, dev)
    boxes = vl.ContactBoxes(tables, dev)
    with memguard.poisoned_allocations() as pa:
        votes = vl.vote_labels(joints, off, n, boxes)
        torch.cuda.synchronize()
    assert len(pa.records) == 1 and pa.records[0][1] is votes          # the output is the one guarded allocation
    pa.assert_clean(votes, names=['votes'])
    return votes


# ---- 1, 2: the kernel --------------------------------------------------------------------------------------------------
def test_kernel_equals_reference(dev):
    cases = vote_cases.g13()
    items = [c.joints.shape[0] * 53 for c in cases]
    assert {53, 265, 371, 1007, 1961} == set(items)     # below, just above and far from multiples of a workgroup's 256
    votes = _kernel_votes([c.joints for c in cases],
                          [vl.contact_tables(c.instances, 10, c.contact_dist, name=c.name) for c in cases], dev)
    want = torch.from_numpy(np.concatenate([c.votes for c in cases]))
    assert votes.shape == want.shape and votes.dtype == torch.float32
    assert torch.equal(_bits(votes), _bits(want))


def test_kernel_equals_mirror(dev):
    samples = vote_cases.second_set()
    assert [s[0].shape[0] for s in samples] == [1, 2, 5, 6, 64, 300]
    assert {len(s[2]) for s in samples} >= {0, 10}
    votes = _kernel_votes([s[0] for s in samples], [vl.contact_tables(s[2], 10, 1.0) for s in samples], dev)
    want = torch.from_numpy(np.concatenate([s[1] for s in samples]))
    assert (want[..., 0] == 1).any() and (want[..., 0] == 0).any()
    assert torch.equal(_bits(votes), _bits(want))


def test_second_threshold_through_generate_votes(dev):
    case = vote_cases.g13()[8]
    assert case.contact_dist == 0.5
    got = vl.generate_votes(case.joints, case.instances, contact_dist=0.5, device=dev)
    assert got.is_cuda and torch.equal(_bits(got), _bits(torch.from_numpy(case.votes)))
    wide = vl.generate_votes(case.joints, case.instances, device=dev)          # the default, 1.0, votes for more
    assert (wide[..., 0] == 1).sum() > (got[..., 0] == 1).sum()
    none = vl.generate_votes(case.joints, [], device=dev)                      # no boxes, K = 0
    assert not _bits(none).any()


# ---- 3: the store without given votes ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def samples():
    """the second set and G13's eight samples at contact distance 1.0, with the mirror's / the reference's votes"""
    return list(vote_cases.second_set()) + [vote_cases.mirrored(c) for c in vote_cases.g13()[:8]]


@pytest.fixture(scope="module")
def full(samples, dev):
    return dv.DeviceSampleStore.from_samples(samples, device=dev)


def _draws_for(ids):
    return [(b // 4 % 2, dv.ANGLES[b % 4], (-0.83, 0.41, -0.0625, 0.97)[b % 4]) for b in range(len(ids))]


def _host_batch(samples, ids, num_frames, use_height, augment, seed=3):
    """the host loader's batch: SampleListDataset items (which draw their own augmentation) + collate_fn"""
    from pose2room_amd.p2rnet import P2RConfig, default_config
    cfg = P2RConfig(default_config('train', data={'num_frames': num_frames, 'no_height': not use_height}))
    ds = dv.SampleListDataset(cfg, 'train' if augment else 'val', samples)
    random.seed(seed); np.random.seed(seed)
    draws = [dl.draw_augmentation() for _ in ids] if augment else None
    random.seed(seed); np.random.seed(seed)
    return dl.collate_fn([ds[i] for i in ids]), draws


def test_store_derives_missing_votes(dev, samples, full):
    bare = [(j, None, inst, name) for j, _, inst, name in samples]
    store = dv.DeviceSampleStore.from_samples(bare, device=dev)
    assert store.votes.shape == full.votes.shape and torch.equal(_bits(store.votes), _bits(full.votes))
    assert store.nbytes == full.nbytes and not store.lean and store.contact is None
    mixed = dv.DeviceSampleStore.from_samples([s if i % 3 else b for i, (s, b) in enumerate(zip(samples, bare))],
                                              device=dev)
    assert torch.equal(_bits(mixed.votes), _bits(full.votes))
    ids = [13, 0, 5, 4, 9, 2, 12]
    for augment in (True, False):
        want, draws = _host_batch(samples, ids, 16, True, augment)
        got = store.assemble(ids, 16, augment, draws, True)
        assert_same_batch(got, {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in want.items()})


# ---- 4: the lean store ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lean(samples, dev):
    return dv.DeviceSampleStore.from_samples([(j, None, inst, name) for j, _, inst, name in samples], device=dev,
                                             votes='derive')


def test_lean_store_holds_no_votes(samples, full, lean):
    N, F, J, K = len(samples), sum(s[0].shape[0] for s in samples), 53, 10
    assert lean.votes is None and lean._c.votes in (None, 0) and lean.lean and lean.contact.N == N
    per_sample = 8 + 4 + 16 + dv.N_VARIANTS * K * (24 + 8) + K * (12 + 4 + 8)
    assert full.nbytes == F * J * 13 * 4 + N * per_sample
    assert lean.nbytes == F * J * 3 * 4 + N * per_sample + N * (K * 15 * 8 + 4)
    assert lean.nbytes < 0.3 * full.nbytes
    given = dv.DeviceSampleStore.from_samples(samples, device=lean.device, votes='derive')      # given votes: ignored
    assert given.votes is None and given.nbytes == lean.nbytes


@pytest.mark.parametrize("augment", [False, True])
@pytest.mark.parametrize("use_height", [False, True])
@pytest.mark.parametrize("num_frames", [1, 16, 37, 64])
def test_lean_batch_equals_full_store(dev, samples, full, lean, num_frames, use_height, augment):
    ids = list(range(len(samples))) + [0, 7]             # 16 items: every sample, every (flip, angle) twice
    draws = _draws_for(ids) if augment else None
    if augment:
        assert {(d[0], d[1]) for d in draws} == {(f, a) for f in (0, 1) for a in dv.ANGLES}
    want = full.assemble(ids, num_frames, augment, draws, use_height)
    with memguard.poisoned_allocations() as pa:
        got = lean.assemble(ids, num_frames, augment, draws, use_height)
        torch.cuda.synchronize()
    assert len(pa.records) == len(KEYS)
    pa.assert_clean(*[got[k] for k in KEYS], names=KEYS)
    assert_same_batch(got, want)
    assert int((got['vote_label_mask'] == 1).sum()) > 0


# ---- 5: an epoch -----------------------------------------------------------------------------------------------------------
def test_lean_epoch_equals_host_loader(dev, samples):
    from pose2room_amd.p2rnet import P2RConfig, default_config
    from tests.test_device_loader_gpu import _epoch
    five = [samples[i] for i in (4, 0, 8, 13, 3)]
    cfg = P2RConfig(default_config('train', data={'num_frames': 24, 'no_height': False}, train={'batch_size': 2}))
    store = dv.DeviceSampleStore.from_samples(five, device=dev, votes='derive')
    host = dl.P2RNet_dataloader(cfg, 'train', dataset=dv.SampleListDataset(cfg, 'train', five))
    devl = dv.P2RNet_device_dataloader(cfg, 'train', store)
    assert len(devl.dataloader) == len(host.dataloader) == 3
    for seed in (0, 1):
        want, got = _epoch(host, seed, dev=dev), _epoch(devl, seed)
        assert len(got) == len(want) == 3
        for g, w in zip(got, want):
            assert_same_batch(g, w)
