"""GPU: the scene read-out on the device (csrc/scene.hip: p2r_scene_nodes, p2r_contact_frames, p2r_unique_frames;
net_utils/scene_device.py; P2RNet.predict_scenes) against the reference's own results (G15), against the float64
definitions of tests/scene_cases.py over an edge sweep, under the memory contract of tests/memguard.py, and end to end
on the synthetic model.

Indices are compared for equality: every contact case keeps its minimum at least 1e-6 m below every frame with a
different row (asserted without a GPU in tests/test_scene_cpu.py), and rows that are equal tie bit for bit.  node_obbs is
compared bit for bit with p2r_box_params' output, node_rmat with the tolerance tests/test_mm_device_gpu.py applies to the
device's heading (rtol 0, atol 1e-9: the same math library), dist with 12 * 2^-53 * (||x - c||_1 + max size / 2) at the
attaining joint against the definition evaluated on the very nodes the kernel read."""
import functools

import numpy as np
import pytest
import torch

from pose2room_amd.net_utils import mm_device
from pose2room_amd.net_utils import multi_modal_eval as mm
from pose2room_amd.net_utils import scene_device as sd
from tests import memguard
from tests import scene_cases as sc
from tests.memguard import run_contract

pytestmark = pytest.mark.gpu

EINVAL = -22
SWEEP = sc.sweep()


def _np(t):
    return t.cpu().numpy()


def _nodes(c, dev):
    t = lambda a: torch.from_numpy(a).to(dev)                                    # noqa: E731
    return sd.scene_nodes(t(c.obbs), t(c.obj_prob), t(c.pred_mask), t(c.pred_cls), c.threshold)


@functools.lru_cache(maxsize=None)
def _swept(i, dev):
    """-> (Nodes, frame, dist, Unique) of host arrays from the three launches on case i"""
    c = SWEEP[i]
    nodes = _nodes(c, dev)
    joints = torch.from_numpy(c.joints).to(dev)
    frame, dist = sd.contact_frames(joints, nodes[2], nodes[3], nodes[0])
    unique = sd.unique_frames(joints)
    return sc.Nodes(*map(_np, nodes)), _np(frame), _np(dist), sc.Unique(*map(_np, unique))


# ---- 1. G15: the reference's results -----------------------------------------------------------------------------------------
def _check_g15(z, obbs, nodes, frame, dist, unique):
    """nodes: sc.Nodes, unique: sc.Unique, all host arrays; obbs: p2r_box_params' output"""
    N, K = z['obj_prob'].shape
    np.testing.assert_allclose(obbs, z['box_params'], rtol=0, atol=1e-9)
    sc.check_unique(unique, sc.Unique(z['unique_count'], z['unique_index'], sc.unique_def(z['input_joints']).rank))
    want = sc.nodes_def(obbs, z['obj_prob'], z['pred_mask'], z['pred_sem_cls'], float(z['dump_threshold']))
    sc.check_nodes(nodes, want, sc.RMAT_TOL)                        # node_obbs: bit copies of p2r_box_params' rows
    for b in range(N):
        kept = np.nonzero(z['keep'][b])[0]
        m = len(kept)
        assert nodes.count[b] == m and np.array_equal(nodes.inst_idx[b, :m], kept)
        assert np.array_equal(nodes.node_cls[b, :m], z['pred_sem_cls'][b, kept])
        np.testing.assert_allclose(nodes.node_rmat[b, :m], z['rmat'][b, kept], **sc.RMAT_TOL)
        # the reference's dist_node2bbox indexes the de-duplicated frames
        assert np.array_equal(unique.rank[b][frame[b, :m]], z['contact_unique'][b, kept])
    ct = sc.contact_def(z['input_joints'], nodes.node_obbs, nodes.node_rmat, nodes.count)
    sc.check_contact(frame, dist, ct, z['input_joints'], nodes.node_obbs, nodes.count)


def test_g15_through_the_entry_points(dev):
    z = sc.g15()
    t = lambda k: torch.from_numpy(z[k]).to(dev)                                  # noqa: E731
    obbs = mm_device.box_params(t('pred_corners_3d'))
    nodes = sd.scene_nodes(obbs, t('obj_prob'), t('pred_mask'), t('pred_sem_cls'), float(z['dump_threshold']))
    frame, dist = sd.contact_frames(t('input_joints'), nodes[2], nodes[3], nodes[0])
    unique = sd.unique_frames(t('input_joints'))
    assert [x.dtype for x in nodes] == [torch.int32, torch.int32, torch.float64, torch.float64, torch.int64, torch.float32]
    assert frame.dtype == torch.int32 and dist.dtype == torch.float64 and all(u.dtype == torch.int32 for u in unique)
    _check_g15(z, _np(obbs), sc.Nodes(*map(_np, nodes)), _np(frame), _np(dist), sc.Unique(*map(_np, unique)))


def test_g15_through_the_tensor_path_without_a_synchronisation(dev):
    """`scenes_from_parsed`, what predict_scenes runs behind parse_predictions: the same results, and no call that waits
    for the device or copies to the host before the caller asks"""
    z = sc.g15()
    t = lambda k: torch.from_numpy(z[k]).to(dev)                                  # noqa: E731
    args = (t('pred_corners_3d'), t('obj_prob'), t('pred_mask'), t('pred_sem_cls'), t('input_joints'))
    sd.scenes_from_parsed(*args, float(z['dump_threshold']))                      # libraries loaded, allocator warm
    torch.cuda.synchronize(dev)
    torch.cuda.set_sync_debug_mode("error")
    try:
        batch = sd.scenes_from_parsed(*args, float(z['dump_threshold']))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert (batch.H, batch.B, batch.K) == (1, 3, 24) and batch._host_arrays is None
    h = batch.host()
    _check_g15(z, _np(mm_device.box_params(args[0])), sc.Nodes(*[h[k] for k in sc.Nodes._fields]), h['contact_frame'],
               h['contact_dist'], sc.Unique(h['unique_count'], h['unique_index'], h['unique_rank']))
    for b in range(3):
        kept = np.nonzero(z['keep'][b])[0]
        nodes = batch.nodes(b)
        assert [n['inst_idx'] for n in nodes] == kept.tolist()
        assert [n['contact_frame_unique'] for n in nodes] == z['contact_unique'][b, kept].tolist()
        assert np.array_equal(batch.unique(b), z['unique_index'][b, :z['unique_count'][b]])


# ---- 2. the edge sweep against the definitions ---------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(SWEEP)), ids=[c.name for c in SWEEP])
def test_sweep_nodes(dev, i):
    c = SWEEP[i]
    got = _swept(i, dev)[0]
    N, K = c.obj_prob.shape
    assert got.count.shape == (N,) and got.inst_idx.shape == (N, K) and got.node_obbs.shape == (N, K, 7)
    assert got.node_rmat.shape == (N, K, 3, 3) and got.node_cls.shape == (N, K) and got.node_score.shape == (N, K)
    sc.check_nodes(got, sc.nodes_def(c.obbs, c.obj_prob, c.pred_mask, c.pred_cls, c.threshold), sc.RMAT_TOL)


@pytest.mark.parametrize("i", range(len(SWEEP)), ids=[c.name for c in SWEEP])
def test_sweep_contact_frames(dev, i):
    c = SWEEP[i]
    nodes, frame, dist, _ = _swept(i, dev)
    want = sc.contact_def(c.joints, nodes.node_obbs, nodes.node_rmat, nodes.count)       # on the nodes the kernel read
    sc.check_contact(frame, dist, want, c.joints, nodes.node_obbs, nodes.count, c.skip_rows)
    if c.mirror is not None:                                          # the exact tie goes to the lower frame
        b, lo, hi = c.mirror
        for n in range(b, len(frame), c.joints.shape[0]):
            assert frame[n, 0] == lo and dist[n, 0] == want.d[(n, 0)][hi]


@pytest.mark.parametrize("i", range(len(SWEEP)), ids=[c.name for c in SWEEP])
def test_sweep_unique_frames(dev, i):
    sc.check_unique(_swept(i, dev)[3], sc.unique_def(SWEEP[i].joints))


def test_ground_truth_nodes_with_a_stored_matrix(dev):
    """the matrix is read, not rebuilt from the heading: nodes whose R_mat is a rotation about another axis"""
    c = next(c for c in SWEEP if c.name == "K24-T40-J53-C3-H2-all")
    nd = sc.nodes_def(c.obbs, c.obj_prob, c.pred_mask, c.pred_cls, c.threshold)
    a = nd.node_obbs[..., 6]
    rmat = np.zeros_like(nd.node_rmat)
    rmat[..., 0, 0], rmat[..., 1, 1], rmat[..., 1, 2] = 1.0, np.cos(a), -np.sin(a)
    rmat[..., 2, 1], rmat[..., 2, 2] = np.sin(a), np.cos(a)
    want = sc.contact_def(c.joints, nd.node_obbs, rmat, nd.count)
    t = lambda x: torch.from_numpy(x).to(dev)                                     # noqa: E731
    frame, dist = sd.contact_frames(t(c.joints), t(nd.node_obbs), t(rmat), t(nd.count))
    keep = [n for n in range(len(nd.count)) if n % 2 not in c.skip_rows]
    frame, dist = _np(frame), _np(dist)
    for n in keep:                    # no margin was designed for these matrices: the distance decides, not the index
        for s in range(nd.count[n]):
            d = want.d[(n, s)]
            bound = sc.dist_bound(c.joints[n % 2, want.frame[n, s], want.joint[n, s]], nd.node_obbs[n, s])
            assert abs(dist[n, s] - want.dist[n, s]) <= bound and abs(d[frame[n, s]] - want.dist[n, s]) <= bound
    assert not np.array_equal(want.frame, sc.contact_def(c.joints, nd.node_obbs, nd.node_rmat, nd.count).frame)


def test_empty_problems(dev):
    z = lambda *shape, dtype: torch.zeros(*shape, dtype=dtype, device=dev)        # noqa: E731
    joints = torch.from_numpy(SWEEP[1].joints).to(dev)
    B, T = joints.shape[:2]
    for N, K in ((0, 24), (2, 0), (0, 0)):
        nodes = sd.scene_nodes(z(N, K, 7, dtype=torch.float64), z(N, K, dtype=torch.float32), z(N, K, dtype=torch.uint8),
                               z(N, K, dtype=torch.int64), 0.5)
        assert nodes[0].shape == (N,) and not nodes[0].any() and nodes[2].shape == (N, K, 7)
        frame, dist = sd.contact_frames(joints, nodes[2], nodes[3], nodes[0])
        assert frame.shape == (N, K) and dist.shape == (N, K)
        batch = sd.scenes_from_parsed(z(N, K, 8, 3, dtype=torch.float64), z(N, K, dtype=torch.float32),
                                      z(N, K, dtype=torch.uint8), z(N, K, dtype=torch.int64), joints[:N], 0.5,
                                      num_hypotheses=1, contact=N > 0, unique=N > 0)
        assert len(batch) == N and all(batch.nodes(n) == [] for n in range(N))
    count, index, rank = sd.unique_frames(joints[:0])
    assert count.shape == (0,) and index.shape == (0, T) and rank.shape == (0, T)
    # all counts 0 at K > 0: every slot -1 / 0
    frame, dist = sd.contact_frames(joints, z(4, 24, 7, dtype=torch.float64), z(4, 24, 3, 3, dtype=torch.float64),
                                    z(4, dtype=torch.int32))
    assert bool((frame == -1).all()) and not bool(dist.any())


# ---- 3. the memory contract ------------------------------------------------------------------------------------------------
def _contract_case():
    return next(c for c in SWEEP if c.name == "K65-T40-J53-C4-H2-all"), next(c for c in SWEEP if c.name.startswith("K128-T257-J53-C3-H2"))


@pytest.mark.parametrize("which", [0, 1], ids=['all-kept-C4', 'mixed-C3'])
def test_memory_contract(dev, which):
    """outputs in poisoned, guard-banded buffers: every output element is overwritten, no halo is damaged, the inputs are
    bit-identical afterwards, and four runs over different surroundings give identical bits"""
    c = _contract_case()[which]
    nd = sc.nodes_def(c.obbs, c.obj_prob, c.pred_mask, c.pred_cls, c.threshold)
    t = torch.from_numpy
    got = run_contract(lambda **k: sd.scene_nodes(k['obbs'], k['obj_prob'], k['pred_mask'], k['pred_cls'], c.threshold),
                       dict(obbs=t(c.obbs), obj_prob=t(c.obj_prob), pred_mask=t(c.pred_mask), pred_cls=t(c.pred_cls)), dev)
    sc.check_nodes(sc.Nodes(*[_np(got[f'out.{i}']) for i in range(6)]), nd, sc.RMAT_TOL)
    got = run_contract(lambda **k: sd.contact_frames(k['joints'], k['node_obbs'], k['node_rmat'], k['count']),
                       dict(joints=t(c.joints), node_obbs=t(nd.node_obbs), node_rmat=t(nd.node_rmat), count=t(nd.count)), dev)
    sc.check_contact(_np(got['out.0']), _np(got['out.1']), sc.contact_def(c.joints, nd.node_obbs, nd.node_rmat, nd.count),
                     c.joints, nd.node_obbs, nd.count, c.skip_rows)
    got = run_contract(lambda **k: sd.unique_frames(k['joints']), dict(joints=t(c.joints)), dev)
    sc.check_unique(sc.Unique(*[_np(got[f'out.{i}']) for i in range(3)]), sc.unique_def(c.joints))


def test_refused_calls_leave_their_outputs_untouched(dev):
    c = SWEEP[4]
    nd = sc.nodes_def(c.obbs, c.obj_prob, c.pred_mask, c.pred_cls, c.threshold)
    N, K = c.obj_prob.shape
    B, T, J, C = c.joints.shape
    t = lambda a: torch.from_numpy(a).to(dev)                                    # noqa: E731
    ins = dict(obbs=t(c.obbs), obj_prob=t(c.obj_prob), pred_mask=t(c.pred_mask), pred_cls=t(c.pred_cls), joints=t(c.joints),
               node_obbs=t(nd.node_obbs), node_rmat=t(nd.node_rmat), count=t(nd.count))
    shapes = dict(count=((N,), torch.int32), inst_idx=((N, K), torch.int32), node_obbs=((N, K, 7), torch.float64),
                  node_rmat=((N, K, 3, 3), torch.float64), node_cls=((N, K), torch.int64), node_score=((N, K), torch.float32),
                  frame=((N, K), torch.int32), dist=((N, K), torch.float64), ucount=((B,), torch.int32),
                  index=((B, T), torch.int32), rank=((B, T), torch.int32))
    outs = {k: memguard.guarded(s, d, dev) for k, (s, d) in shapes.items()}
    p = lambda k: (outs[k][1] if k in outs else ins[k]).data_ptr()                # noqa: E731
    l = sd.lib()
    nodes_out = [p(k) for k in ('count', 'inst_idx', 'node_obbs', 'node_rmat', 'node_cls', 'node_score')]
    nodes_in = [p(k) for k in ('obbs', 'obj_prob', 'pred_mask', 'pred_cls')]
    contact_tail = [p(k) for k in ('node_obbs', 'node_rmat', 'count', 'frame', 'dist')]
    # the contact call's node_obbs / node_rmat / count are inputs there: pass the real ones, outputs stay the guarded ones
    contact_tail[:3] = [ins[k].data_ptr() for k in ('node_obbs', 'node_rmat', 'count')]
    stream = torch.cuda.current_stream(dev).cuda_stream
    refused = [l.p2r_scene_nodes(N, 1025, *nodes_in, 0.5, *nodes_out, stream),
               l.p2r_scene_nodes(-1, K, *nodes_in, 0.5, *nodes_out, stream),
               l.p2r_scene_nodes(N, K, None, *nodes_in[1:], 0.5, *nodes_out, stream),
               l.p2r_contact_frames(p('joints'), 3, T, J, C, N, K, *contact_tail, stream),
               l.p2r_contact_frames(p('joints'), B, 65536, J, C, N, K, *contact_tail, stream),
               l.p2r_contact_frames(p('joints'), B, T, 65, C, N, K, *contact_tail, stream),
               l.p2r_contact_frames(p('joints'), B, T, J, 5, N, K, *contact_tail, stream),
               l.p2r_unique_frames(p('joints'), B, 4097, J, C, p('ucount'), p('index'), p('rank'), stream),
               l.p2r_unique_frames(p('joints'), B, T, J, 2, p('ucount'), p('index'), p('rank'), stream),
               l.p2r_unique_frames(None, B, T, J, C, p('ucount'), p('index'), p('rank'), stream)]
    assert refused == [EINVAL] * len(refused)
    torch.cuda.synchronize(dev)
    for k, (buf, view) in outs.items():
        assert int(memguard.poison_count(view)) == view.numel(), k
        assert int(memguard.halo_damage(buf, view, 'poison')) == 0, k


# ---- 4. predict_scenes on the synthetic model ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(dev):
    from pose2room_amd.p2rnet.synthetic import make_batch
    from tests.test_model_cpu import build
    # the far-box filter is off, as wherever `generate` runs on these weights (tests/test_model_gpu.py): the boxes of an
    # untrained model lie far from the body, and parse_predictions asserts that every sample keeps a box
    net, cfg = build('test', 64, device=dev, remove_far_box=False)
    return net.to(dev).eval(), cfg, make_batch(2, 64, seed=77, device=dev)


def _clear_threshold(obj_prob, mask):
    """a threshold in the widest gap between the probabilities of the boxes the NMS kept: some kept, some not"""
    p = np.sort(np.unique(obj_prob[mask == 1].astype(np.float64)))
    assert len(p) >= 2
    i = int(np.argmax(np.diff(p)))
    return float((p[i] + p[i + 1]) / 2)


def _same_records(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert list(g) == list(w)
        assert g['inst_idx'].dtype == np.bool_ and np.array_equal(g['inst_idx'], w['inst_idx'])
        assert g['cls'].dtype == w['cls'].dtype and np.array_equal(g['cls'], w['cls'])
        assert g['obbs'].shape == w['obbs'].shape
        np.testing.assert_allclose(g['obbs'], w['obbs'], rtol=0, atol=1e-9)        # tests/test_mm_device_gpu.py's


def test_predict_scenes_records_are_confident_boxes_of_generate(model):
    net, cfg, data = model
    with torch.no_grad():
        ep, eval_dict, parsed = net.generate(data, eval=False)
    thr = _clear_threshold(parsed['obj_prob'], eval_dict['pred_mask'])
    want = mm.confident_boxes(ep, eval_dict, parsed, thr)
    batch = net.predict_scenes({'input_joints': data['input_joints']}, dump_threshold=thr)     # no ground truth needed
    K = parsed['obj_prob'].shape[1]
    assert (batch.H, batch.B, batch.K) == (1, 2, K) and batch.count.is_cuda and not batch.count.requires_grad
    _same_records(batch.records(), want)
    assert 0 < sum(int(r['inst_idx'].sum()) for r in want) < int((eval_dict['pred_mask'] == 1).sum())
    z = batch.host()
    joints = data['input_joints'].cpu().numpy()
    sc.check_unique(sc.Unique(z['unique_count'], z['unique_index'], z['unique_rank']), sc.unique_def(joints))
    ct = sc.contact_def(joints, z['node_obbs'], z['node_rmat'], z['count'])
    for n in range(2):                                  # the model's boxes carry no designed margin: the distance decides
        nodes = batch.nodes(n)
        assert len(nodes) == int(want[n]['inst_idx'].sum())
        for s, node in enumerate(nodes):
            assert 0 <= node['contact_frame'] < 64
            bound = sc.dist_bound(joints[n, ct.frame[n, s], ct.joint[n, s]], z['node_obbs'][n, s])
            assert abs(node['contact_dist'] - ct.dist[n, s]) <= bound
            assert abs(ct.d[(n, s)][node['contact_frame']] - ct.dist[n, s]) <= bound
    assert cfg.config.get('generation') is None or 'dump_threshold' not in cfg.config['generation']
    default = net.predict_scenes(data, contact=False, unique=False)                  # the default threshold is 0.5
    _same_records(default.records(), mm.confident_boxes(ep, eval_dict, parsed, 0.5))
    assert default.contact_frame is None and default.unique_index is None


def test_predict_scenes_hypotheses_are_the_triples_of_generate_hypotheses(model):
    net, cfg, data = model
    H, ns, seed = 2, [5, 40], 321
    with torch.no_grad():
        triples = net.generate_hypotheses(data, H, n_samples=ns, seed=seed, eval=False)
    thr = _clear_threshold(np.concatenate([t[2]['obj_prob'] for t in triples]),
                           np.concatenate([t[1]['pred_mask'] for t in triples]))
    batch = net.predict_scenes(data, num_hypotheses=H, n_samples=ns, seed=seed, dump_threshold=thr)
    assert (batch.H, batch.B) == (H, 2) and len(batch) == 4
    for h, (ep, eval_dict, parsed) in enumerate(triples):
        _same_records(batch.records(h), mm.confident_boxes(ep, eval_dict, parsed, thr))
    assert batch.unique_index.shape[0] == 2 and batch.contact_frame.shape[0] == 4      # the joints rows are not stacked
    assert sum(len(batch.nodes(n)) for n in range(4)) > 0


def test_predict_scenes_with_a_threshold_that_keeps_nothing(model, tmp_path):
    net, cfg, data = model
    batch = net.predict_scenes(data, dump_threshold=2.0)
    assert not bool(batch.count.any()) and bool((batch.contact_frame == -1).all()) and bool((batch.inst_idx == -1).all())
    assert all(batch.nodes(n) == [] for n in range(len(batch)))
    for rec in batch.records():
        assert rec['obbs'].shape == (0, 7) and not rec['inst_idx'].any()
    assert batch.save_npz(str(tmp_path / 'x.npz'), 0) is False and not (tmp_path / 'x.npz').exists()
