"""CPU: the contract of the consensus clustering (csrc/consensus.hip, net_utils/consensus_device.py) before any kernel is
involved: the definition `consensus_reference` against links and clusters recorded from the reference's own box code
(G17), the ABI of include/p2r_consensus.h / libp2r_consensus.so, the argument checks of the entry points and of the
Python wrappers -- all of which return before any launch --, the cases the GPU test sweeps (the margin rule, every listed
situation present), and the teeth of the comparison function the GPU test shares: each of six wrong definitions must be
caught on at least one case."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from pose2room_amd import _lib
from pose2room_amd.net_utils import consensus_device as cd
from pose2room_amd.net_utils import scene_device as sd
from tests import consensus_cases as cc

EINVAL = -22
built = pytest.mark.skipif(not os.path.exists(cd.LIB_PATH), reason="libp2r_consensus.so is not built")


# ---- 1. the definition against the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,thr", [('025', 0.25), ('050', 0.5)])
def test_definition_reproduces_g17(tag, thr):
    z = cc.g17()
    H, K = int(z['H']), z['node_cls'].shape[1]
    assert (H, K) == (3, 6) and z['count'].shape == (3,)
    ref, extras = cd.consensus_reference(z['count'], z['node_obbs'], z['node_cls'], z['node_score'], H, thr, True,
                                         return_iou=True)
    iou, pool = extras[0]
    assert pool == [(h, s) for h in range(H) for s in range(int(z['count'][h]))]
    np.testing.assert_allclose(iou, z['iou'], rtol=0, atol=1e-9, equal_nan=True)          # the reference's box3d_iou
    v = z['iou'][~np.isnan(z['iou'])]
    assert np.abs(v - thr).min() >= cc.MARGIN
    with np.errstate(invalid='ignore'):
        assert np.array_equal(iou > thr, z['link_' + tag])
    leaders, cluster = z['leaders_' + tag], z['cluster_' + tag]
    assert ref.n_clusters[0] == len(leaders)
    assert np.array_equal(ref.leader_node[0, :len(leaders)], [pool[L][0] * K + pool[L][1] for L in leaders])
    assert np.array_equal([ref.cluster_of[h, s] for h, s in pool], cluster)
    assert np.array_equal(ref.members[0, :len(leaders)], np.bincount(cluster, minlength=len(leaders)))
    # the fixture is the design, bit for bit, and something merges at either threshold
    d = cc.g17_design()
    for k in ('count', 'node_obbs', 'node_cls', 'node_score'):
        assert np.array_equal(getattr(d, k), z[k]), k
    assert len(z['leaders_025']) < len(z['leaders_050']) < len(pool)


def test_definition_statistics_by_hand():
    """the identical case: two boxes in all four hypotheses -- support 4, zero spread, IoU 1, the scores' mean"""
    ref, _ = cc.reference('identical')
    c = cc.by_name('identical')
    assert ref.n_clusters.tolist() == [2] and ref.members[0, :3].tolist() == [4, 4, 0]
    assert ref.support[0, :2].tolist() == [4, 4] and ref.hyp_mask[0, :3].tolist() == [15, 15, 0]
    assert ref.leader_node[0, :3].tolist() == [0 * 3 + 1, 3 * 3 + 0, -1]                # scores 0.9 (h 0) and 0.875 (h 3)
    assert np.array_equal(ref.box[0, 0], c.node_obbs[0, 1]) and ref.cls[0, :2].tolist() == [6, 5]
    np.testing.assert_allclose(ref.iou_mean[0, :2], 1.0, rtol=0, atol=1e-12)
    assert not ref.center_rms[0].any() and np.array_equal(ref.center_mean[0, 0], c.node_obbs[0, 1, 0:3])
    high = sum(float(np.float32(0.9 - h / 8)) for h in range(4)) / 4                     # the scores are float32
    np.testing.assert_allclose(ref.score_mean[0, :2], [high, (0.5 + 0.625 + 0.75 + 0.875) / 4], rtol=0, atol=1e-12)
    assert ref.cluster_of.tolist() == [[1, 0, -1]] * 4
    # a spread by hand: the chain's first cluster holds A and B
    ref, _ = cc.reference('chain')
    c = cc.by_name('chain')
    a, b = c.node_obbs[0, 0, 0:3], c.node_obbs[1, 0, 0:3]
    np.testing.assert_allclose(ref.center_rms[0, 0], np.linalg.norm(a - b) / 2, rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref.center_mean[0, 0], (a + b) / 2, rtol=0, atol=1e-12)


def test_consensus_batch_host_side():
    """ConsensusBatch's host methods on CPU tensors: node dicts by support, the record layout of confident_boxes"""
    z = cc.g17()
    H, K = 3, 6
    N = H
    ref = cd.consensus_reference(z['count'], z['node_obbs'], z['node_cls'], z['node_score'], H, 0.25, True)
    t = torch.from_numpy
    inst = np.where(np.arange(K)[None] < z['count'][:, None], (5 * np.arange(K)[None] + 1) % K, -1).astype(np.int32)
    rmat = np.zeros((N, K, 3, 3))
    scenes = sd.SceneBatch(H, 1, K, t(z['count']), t(inst), t(z['node_obbs']), t(rmat), t(z['node_cls']), t(z['node_score']))
    batch = cd.ConsensusBatch(scenes, [t(a) for a in ref], 0.25, True)
    assert len(batch) == 1 and batch._host_arrays is None and scenes._host_arrays is None
    nodes = batch.nodes(0)
    assert batch._host_arrays is not None and scenes._host_arrays is not None               # one crossing fills both
    n = int(ref.n_clusters[0])
    assert len(nodes) == n and [x['support'] for x in nodes] == sorted(ref.support[0, :n].tolist(), reverse=True)
    for a, b in zip(nodes, nodes[1:]):
        assert (a['support'], -a['cluster']) > (b['support'], -b['cluster'])
    for x in nodes:
        c = x['cluster']
        h, s = divmod(int(ref.leader_node[0, c]), K)
        assert set(x) == {'centroid', 'R_mat', 'size', 'class_id', 'score', 'inst_idx', 'cluster', 'support', 'support_frac',
                          'members', 'hypotheses', 'score_mean', 'center_mean', 'center_rms', 'iou_mean'}
        assert np.array_equal(x['centroid'], z['node_obbs'][h, s, 0:3]) and x['inst_idx'] == (5 * s + 1) % K
        assert x['class_id'] == [z['node_cls'][h, s]] and x['members'] == ref.members[0, c]
        assert x['support_frac'] == x['support'] / 3 and len(x['hypotheses']) == x['support']
        assert x['hypotheses'] == sorted({hh for hh in range(H) for ss in range(K) if ref.cluster_of[hh, ss] == c})
    two = batch.nodes(0, min_support=2)
    assert [x['cluster'] for x in two] == [x['cluster'] for x in nodes if x['support'] >= 2] and 0 < len(two) < n
    recs = batch.records(min_support=2)
    assert len(recs) == 1 and list(recs[0]) == ['obbs', 'cls', 'inst_idx']
    assert recs[0]['obbs'].shape == (len(two), 7) and recs[0]['obbs'].dtype == np.float64
    assert recs[0]['cls'].dtype == np.int64 and recs[0]['inst_idx'].dtype == np.bool_ and recs[0]['inst_idx'].shape == (K,)
    assert np.array_equal(recs[0]['obbs'], np.array([ref.box[0, x['cluster']] for x in two]))
    assert sorted(np.nonzero(recs[0]['inst_idx'])[0].tolist()) == sorted({x['inst_idx'] for x in two})
    none = batch.records(min_support=4)[0]
    assert none['obbs'].shape == (0, 7) and none['cls'].shape == (0,) and not none['inst_idx'].any()
    with pytest.raises(IndexError):
        batch.nodes(1)


# ---- 2. the ABI ------------------------------------------------------------------------------------------------------------------
NAMES = ['p2r_consensus', 'p2r_consensus_workspace_bytes']


def test_header_parses():
    from pose2room_amd.net_utils import ap_device, mm_device, parse_device, vote_labels
    protos = _lib.prototypes(cd.HEADER_PATH)
    assert sorted(protos) == _lib.declared_symbols(cd.HEADER_PATH) == NAMES
    p = protos['p2r_consensus']
    assert p.kinds == 'iii' + 'pppp' + 'fi' + 'p' * 13 + 'pi' and p.has_stream and p.restype is ctypes.c_int
    assert p.argtypes[-2] is ctypes.c_ulonglong and p.argtypes[7] is ctypes.c_double
    w = protos['p2r_consensus_workspace_bytes']
    assert w.kinds == 'iii' and not w.has_stream and w.restype is ctypes.c_ulonglong
    for other in (None, ap_device.HEADER_PATH, mm_device.HEADER_PATH, vote_labels.HEADER_PATH, parse_device.HEADER_PATH,
                  sd.HEADER_PATH):
        assert not set(protos) & set(_lib.declared_symbols(*([other] if other else [])))
    with open(cd.HEADER_PATH) as f:
        text = f.read()
    for name, value in (('P2R_CONSENSUS_MAX_H', cd.MAX_H), ('P2R_CONSENSUS_MAX_K', cd.MAX_K),
                        ('P2R_CONSENSUS_MAX_POOL', cd.MAX_POOL)):
        assert f"#define {name} {value} " in text
    assert (cd.MAX_H, cd.MAX_K, cd.MAX_POOL) == (64, 1024, 2048)
    assert len(cd.Consensus._fields) == 13 and [n for n, _, _ in cd._output_specs(1, 1, 1)] == list(cd.Consensus._fields)


@built
def test_every_prototype_binds_and_library_exports_exactly_them():
    protos = _lib.prototypes(cd.HEADER_PATH)
    out = subprocess.run(["nm", "-D", "--defined-only", cd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("p2r_")}
    assert exported == set(protos)
    for name, p in protos.items():
        fn = getattr(cd.lib(), name)
        assert fn.argtypes == p.argtypes and fn.restype is p.restype
    assert os.path.basename(cd.LIB_PATH) == 'libp2r_consensus.so'
    for other in (_lib.LIB_PATH, sd.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", other], capture_output=True, text=True, check=True).stdout
        assert 'p2r_consensus' not in out


# ---- 3. argument checks: on the host, before any launch ---------------------------------------------------------------------
_BUF = ctypes.create_string_buffer(64)          # a non-NULL, 8-byte aligned address; never read, every call is refused first
_P = ctypes.addressof(_BUF) + (-ctypes.addressof(_BUF)) % 8
_POINTERS = ('count', 'node_obbs', 'node_cls', 'node_score', 'n_clusters', 'leader_node', 'members', 'support', 'hyp_mask',
             'box', 'cls', 'score', 'score_mean', 'center_mean', 'center_rms', 'iou_mean', 'cluster_of', 'workspace')


def _args(**over):
    H, B, K = over.get('H', 3), over.get('B', 2), over.get('K', 5)
    good = dict(H=H, B=B, K=K, count=_P, node_obbs=_P, node_cls=_P, node_score=_P, iou_thresh=0.25, class_aware=1,
                **{k: _P for k in _POINTERS[4:]})
    good['workspace_bytes'] = int(cd.lib().p2r_consensus_workspace_bytes(H, B, K)) if 'workspace_bytes' not in over else 0
    order = ['H', 'B', 'K', 'count', 'node_obbs', 'node_cls', 'node_score', 'iou_thresh', 'class_aware'] + \
        list(_POINTERS[4:]) + ['workspace_bytes']
    good.update(over)
    return [good[k] for k in order] + [None]


@built
def test_workspace_bytes():
    w = cd.lib().p2r_consensus_workspace_bytes
    assert w(3, 2, 5) == 2 * 15 * (12 + 1) * 8 and w(16, 1, 128) == 2048 * (12 + 32) * 8 and w(1, 1, 65) == 65 * 14 * 8
    assert w(3, 0, 5) == 0 and w(3, 2, 0) == 0
    for bad in ((0, 1, 5), (65, 1, 5), (3, -1, 5), (3, 2, -1), (3, 2, 1025), (3, 1, 683), (64, 1, 33), (1, 1 << 22, 1024)):
        assert w(*bad) == 0, bad
    assert w(2, 1, 1024) > 0 and w(64, 1, 32) > 0


@built
def test_entry_point_refuses_bad_arguments():
    fn = cd.lib().p2r_consensus
    need = int(cd.lib().p2r_consensus_workspace_bytes(3, 2, 5))
    assert need > 0
    bads = [dict(H=0), dict(H=65), dict(B=-1), dict(K=-1), dict(K=1025), dict(H=3, K=683), dict(H=64, K=33),
            dict(B=1 << 22, H=1, K=1024), dict(B=1 << 21, H=2, K=1000),          # B * H * K past int
            dict(iou_thresh=-0.01), dict(iou_thresh=float('nan')), dict(iou_thresh=float('-inf')),
            dict(workspace_bytes=need - 1), dict(workspace_bytes=0), dict(workspace=_P + 4)]
    bads += [{k: None} for k in _POINTERS]
    for bad in bads:
        assert fn(*_args(**bad)) == EINVAL, bad
    # problems without an output element: 0, and nothing launched (there is no device here to launch on)
    assert fn(3, 0, 5, *[None] * 4, 0.25, 1, *[None] * 14, 0, None) == 0
    assert fn(1, 0, 0, *[None] * 4, 0.0, 0, *[None] * 14, 0, None) == 0


def _cpu_inputs(N=6, K=5):
    return dict(count=torch.zeros(N, dtype=torch.int32), node_obbs=torch.zeros(N, K, 7, dtype=torch.float64),
                node_cls=torch.zeros(N, K, dtype=torch.int64), node_score=torch.zeros(N, K))


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    ok = _cpu_inputs()
    with pytest.raises(RuntimeError, match="GPU tensor"):
        cd.consensus_clusters(**ok, H=3)
    for name, bad in (('count', ok['count'].long()), ('count', ok['count'][:5]), ('node_obbs', ok['node_obbs'].float()),
                      ('node_cls', ok['node_cls'].int()), ('node_cls', ok['node_cls'][:, :4]),
                      ('node_score', ok['node_score'].double()), ('node_score', ok['node_score'][:3]),
                      ('node_obbs', ok['node_obbs'][..., :6]), ('node_obbs', 'x')):
        with pytest.raises(ValueError, match=name):
            cd.consensus_clusters(**{**ok, name: bad}, H=3)
    for H in (0, 4, 65, 7):
        with pytest.raises(ValueError, match="stack of"):
            cd.consensus_clusters(**ok, H=H)
    with pytest.raises(ValueError, match="2048 per pool"):
        cd.consensus_clusters(**_cpu_inputs(3, 683), H=3)
    with pytest.raises(ValueError, match="at most 1024"):
        cd.consensus_clusters(**_cpu_inputs(1, 1025), H=1)
    for thr in (-0.1, float('nan')):
        with pytest.raises(ValueError, match="iou_thresh"):
            cd.consensus_clusters(**ok, H=3, iou_thresh=thr)
    with pytest.raises(TypeError, match="SceneBatch"):
        cd.consensus_of(ok)
    scenes = sd.SceneBatch(3, 2, 5, ok['count'], torch.zeros(6, 5, dtype=torch.int32), ok['node_obbs'],
                           torch.zeros(6, 5, 3, 3, dtype=torch.float64), ok['node_cls'], ok['node_score'])
    with pytest.raises(RuntimeError, match="GPU tensor"):
        scenes.consensus()


def test_a_missing_library_is_an_error(monkeypatch):
    monkeypatch.setattr(cd._library, 'lib_path', os.path.join(os.path.dirname(cd.LIB_PATH), 'libp2r_consensus_absent.so'))
    monkeypatch.setattr(cd._library, '_handle', None)
    with pytest.raises(_lib.P2RLibraryError, match="libp2r_consensus_absent.so is missing"):
        cd.lib()


# ---- 4. the cases and the teeth of the comparison function ----------------------------------------------------------------------
def _pool_sizes(c):
    B = len(c.count) // c.H
    K = c.node_cls.shape[1]
    return [int(np.clip(c.count[b::B], 0, K).sum()) for b in range(B)]


def test_sweep_covers_what_it_claims():
    cases = cc.sweep()
    assert {c.situation for c in cases} == {'chain', 'equal scores', 'class', 'identical', 'disjoint', 'touching', 'empty',
                                            'H = 1', 'word edges', 'two leaders', 'bad count', 'NaN score', 'NaN box',
                                            'full pool', 'model shape'}
    for c in cases:
        ref, extras = cc.reference(c.name)
        assert cc.assert_margin(c, extras) >= cc.MARGIN                                # every case, no pair excused
        K = c.node_cls.shape[1]
        if c.situation not in ('word edges', 'full pool', 'model shape'):
            assert c.H <= 4 and K <= 8, c.name
        cc.check_consensus(ref, ref, c.skip)
    link = lambda name, i, j: cc.reference(name)[1][0][0][i, j] > cc.by_name(name).iou_thresh      # noqa: E731
    ref = lambda name: cc.reference(name)[0]                                                     # noqa: E731
    # chain: A~B, B~C, not A~C -> {A, B} and {C}
    assert link('chain', 0, 1) and link('chain', 1, 2) and not link('chain', 0, 2)
    assert ref('chain').cluster_of[:, 0].tolist() == [0, 0, 1]
    # equal scores inside one hypothesis and across two: linked, and the lower pool index leads
    c = cc.by_name('equal-scores')
    assert c.node_score[0, 0] == c.node_score[0, 1] and c.node_score[1, 0] == c.node_score[2, 0]
    assert link('equal-scores', 0, 1) and link('equal-scores', 2, 3)
    assert ref('equal-scores').leader_node[0, :2].tolist() == [0, 2] and ref('equal-scores').members[0, :2].tolist() == [2, 2]
    # class: the same geometry, another clustering
    a, b = cc.by_name('class-aware'), cc.by_name('class-blind')
    assert np.array_equal(a.node_obbs, b.node_obbs) and a.class_aware and not b.class_aware
    assert len(np.unique(a.node_cls[a.node_obbs[..., 3] > 0])) == 2
    assert ref('class-aware').n_clusters[0] == 3 and ref('class-blind').n_clusters[0] == 2
    assert ref('identical').support[0, :2].tolist() == [4, 4] and cc.by_name('identical').H == 4
    r = ref('disjoint')
    assert r.n_clusters[0] == 8 and (r.members[0, :8] == 1).all() and not r.iou_mean.any()
    # touching: IoU exactly 0 at threshold 0 does not link, an IoU above 0 does
    c = cc.by_name('touching')
    iou = cc.reference('touching')[1][0][0]
    assert c.iou_thresh == 0.0 and iou[0, 2] == 0.0 and iou[0, 4] == 0.0 and iou[1, 3] > 0.3
    assert ref('touching').cluster_of.tolist() == [[0, 1, -1], [2, 1, 3]]
    assert _pool_sizes(cc.by_name('empty-some')) == [3, 1] and 0 in cc.by_name('empty-some').count[0::2]
    assert _pool_sizes(cc.by_name('empty-all')) == [0, 0] and not ref('empty-all').n_clusters.any()
    assert cc.by_name('H1').H == 1
    assert sorted(_pool_sizes(c)[0] for c in cases if c.situation == 'word edges') == [63, 64, 65, 129]
    assert any(1 < _pool_sizes(c)[1] < _pool_sizes(c)[0] for c in cases if c.situation == 'word edges')
    # two leaders: the member's IoU with the later leader is the higher one
    iou = cc.reference('two-leaders')[1][0][0]
    assert 0.15 < iou[0, 2] < iou[1, 2] and iou[0, 1] == 0.0
    assert ref('two-leaders').cluster_of[:, 0].tolist() == [0, 1, 0]
    c = cc.by_name('bad-count')
    K = c.node_cls.shape[1]
    assert c.count.max() > K and c.count.min() < 0 and np.isnan(c.node_obbs).any()
    assert not np.isnan(ref('bad-count').box).any() and not np.isnan(ref('bad-count').score_mean).any()
    c = cc.by_name('nan-score')
    assert np.isnan(c.node_score).sum() == 3
    r = ref('nan-score')
    assert r.cluster_of.tolist() == [[0, 2, 1], [0, 2, -1]] and r.leader_node[0, :3].tolist() == [3, 2, 1]
    assert np.isnan(r.score[0, 2]) and np.isnan(r.score_mean[0, 0])
    c = cc.by_name('nan-box')
    assert c.skip == (1,) and np.isnan(c.node_obbs[1::2]).any() and not np.isnan(c.node_obbs[0::2]).any()
    c = cc.by_name('full-pool-H16-K128')
    assert (c.H, c.node_cls.shape[1]) == (16, 128) and _pool_sizes(c) == [cd.MAX_POOL]
    c = cc.by_name('model-shape-H10-K128')
    assert (c.H, c.node_cls.shape[1]) == (10, 128) and all(0.07 < m / 1280 < 0.13 for m in _pool_sizes(c))
    assert ref('model-shape-H10-K128').support.max() == 10


MUTATIONS = {
    'single-linkage': (dict(linkage='single'), None),
    'ge-for-gt': (dict(strict=False), None),
    'higher-index-first': (dict(tie='high'), None),
    'highest-iou-leader': (dict(assign='best'), None),
    'class-ignored': ({}, False),                            # class_aware = False where the case says True
    'support-as-members': (dict(support='members'), None),
}
SMALL_CASES = [c.name for c in cc.sweep() if c.situation not in ('full pool', 'model shape')]


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_wrong_definitions_are_caught(mutation):
    kw, aware = MUTATIONS[mutation]
    caught = []
    for name in SMALL_CASES:
        c = cc.by_name(name)
        if aware is not None and not c.class_aware:
            continue
        want = cc.reference(name)[0]
        wrong = cd.consensus_reference(*cc.inputs(c), c.iou_thresh, c.class_aware if aware is None else aware, **kw)
        try:
            cc.check_consensus(wrong, want, c.skip)
        except AssertionError:
            caught.append(name)
    designed = {'single-linkage': 'chain', 'ge-for-gt': 'touching', 'higher-index-first': 'equal-scores',
                'highest-iou-leader': 'two-leaders', 'class-ignored': 'class-aware', 'support-as-members': 'equal-scores'}
    assert designed[mutation] in caught, (mutation, caught)


def test_a_statistic_outside_the_bound_is_caught():
    want = cc.reference('chain')[0]
    for f in cc.CLOSE:
        a = getattr(want, f).copy()
        a[(0,) * a.ndim] += 1e-8
        with pytest.raises(AssertionError):
            cc.check_consensus(want._replace(**{f: a}), want)
        a = getattr(want, f).copy()
        a[(0,) * a.ndim] += 1e-10
        cc.check_consensus(want._replace(**{f: a}), want)
    box = want.box.copy()
    box[0, 0, 0] = np.nextafter(box[0, 0, 0], 1.0)              # the leader's row is a bit copy
    with pytest.raises(AssertionError):
        cc.check_consensus(want._replace(box=box), want)
    got = cc.reference('nan-box')[0]
    other = got._replace(n_clusters=got.n_clusters + np.array([0, 1], np.int32))
    cc.check_consensus(other, got, skip=(1,))                   # the skipped sample is not compared
    with pytest.raises(AssertionError):
        cc.check_consensus(other, got)
