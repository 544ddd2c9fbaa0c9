"""CPU: the contract of the occupancy maps (csrc/occupancy.hip, net_utils/occupancy_device.py) before any kernel is
involved: the definition `occupancy_reference` against maps and a scene IoU recorded from the reference's own hull test
and metric (G18), the bit packing, the ABI of include/p2r_occupancy.h / libp2r_occupancy.so, the argument checks of the
entry points and of the Python wrappers -- all of which return before any launch --, the cases the GPU test sweeps (the
margin rule, every listed situation present), and the teeth of those cases: each of six wrong definitions must change a
designed case."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from pose2room_amd import _lib
from pose2room_amd.net_utils import occupancy_device as od
from pose2room_amd.net_utils import scene_device as sd
from tests import occupancy_cases as oc

EINVAL = -22
built = pytest.mark.skipif(not os.path.exists(od.LIB_PATH), reason="libp2r_occupancy.so is not built")


# ---- 1. the definition against the reference ---------------------------------------------------------------------------------
def test_definition_reproduces_g18():
    z = oc.g18()
    grid = od.Grid(z['origin'], float(z['voxel']), z['dims'])
    assert grid.dims == (32, 16, 32) and grid.voxel == 0.1 and z['occ'].shape == (2, 32, 16, 1) and z['margin'] >= 1e-7
    d = oc.g18_design()                                        # the fixture is the design, bit for bit
    assert d[0] == grid
    for k, a in zip(('count', 'node_obbs', 'node_rmat', 'node_score'), d[1:]):
        assert np.array_equal(a, z[k]), k
    ref = od.occupancy_reference(z['count'][:1], z['node_obbs'][:1], z['node_rmat'][:1], z['node_score'][:1], grid, 1, None,
                                 (z['count'][1:], z['node_obbs'][1:], z['node_rmat'][1:], z['node_score'][1:]))
    assert np.array_equal(ref.occ[0], z['occ'][0]) and np.array_equal(ref.gt_occ[0], z['occ'][1])      # the hull test
    iou = od.scene_iou(ref.counts)
    assert iou.dtype == np.float32 and iou[0] == z['iou'] and 0.0 < iou[0] < 1.0                        # calculate_scene_iou
    assert ref.counts[0].tolist() == [int(od.popcount(z['occ'][0])), int(od.popcount(z['occ'][1])),
                                      int(od.popcount(z['occ'][0] & z['occ'][1])), 0, 0]


@pytest.mark.parametrize("nx", [1, 63, 64, 65, 130])
def test_pack_unpack_round_trip(nx):
    rng = np.random.default_rng(nx)
    dense = rng.integers(0, 2, (2, 3, 4, nx)).astype(bool)
    dense[0, 0, 0], dense[0, 0, 1] = True, False
    words = od.pack_bits(dense)
    W = (nx + 63) // 64
    assert words.shape == (2, 3, 4, W) and words.dtype == np.int64
    assert np.array_equal(od.unpack_bits(words, nx), dense)
    u = words.view(np.uint64)
    for i in range(nx):
        assert np.array_equal((u[..., i // 64] >> np.uint64(i % 64)) & np.uint64(1), dense[..., i])
    if nx % 64:                                                # the padding bits are zero, also under a row of ones
        assert not (u[..., -1] >> np.uint64(nx % 64)).any()
    assert np.array_equal(od.popcount(words), dense.reshape(2, -1).sum(1))
    poisoned = (u | (~np.uint64(0) << np.uint64(nx % 64) if nx % 64 else np.uint64(0))).view(np.int64)
    poisoned = poisoned if nx % 64 == 0 else np.concatenate([words[..., :-1], poisoned[..., -1:]], -1)
    assert np.array_equal(od.unpack_bits(poisoned, nx), dense)


def test_definition_by_hand():
    """the dyadic case: faces on voxel centres are inside, equal scores go to the lower slot, a NaN score is -inf"""
    c, ref = oc.by_name('dyadic'), oc.reference('dyadic')
    dense = od.unpack_bits(ref.occ, 12)
    # box 0: x centres 0.625 .. 1.625 = voxels 2 .. 6, y 0.375 .. 0.875 = 1 .. 3, z 0.375 .. 0.875 = 1 .. 3
    assert dense[0, 1:4, 1:4, 2:7].all() and not dense[0, 1:3, 1:4, 1].any() and not dense[0, 0].any()
    own = ref.owner[0]
    assert (own[1:4, 1:4, 2:7] == 0).sum() == 44               # box 1 has the same score and a higher slot; one corner: below
    assert (own[1:4, 0, 4:9] == 1).all() and (own != 2).all()      # the NaN score inside box 1 owns nothing
    assert own[3, 4, 10] == 3 and dense[0, 3, 4, 10]           # the NaN score alone owns its voxel
    assert own[3, 3, 2] == 4 and (own == 4).sum() == 18        # the higher score in the higher slot takes the shared corner
    assert (ref.owner[1][1:4, 1:4, 4:7] == 1).all() and (ref.owner[1][1:4, 1:4, 2:4] == 0).all()
    assert np.array_equal(ref.owner >= 0, dense)
    body = od.unpack_bits(ref.body, 12)
    want = {(1, 1, 1), (3, 1, 2), (0, 0, 0), (4, 5, 11), (4, 5, 7)}                # (k, j, i) of the joints that count
    assert {tuple(x) for x in np.argwhere(body[0]).tolist()} == want and np.argwhere(body[1]).tolist() == [[1, 1, 1]]
    assert ref.counts[0].tolist() == [111, int(od.popcount(ref.gt_occ[0])), int(od.popcount(ref.occ[0] & ref.gt_occ[0])),
                                      5, int(dense[0][body[0]].sum())]
    assert np.array_equal(ref.fused, ref.occ) and np.array_equal(ref.votes, dense.astype(np.uint8))   # H = 1
    assert od.body_collision(ref.counts)[1] == 0.0 and od.scene_iou(np.zeros((1, 5), np.int64))[0] == 0.0
    assert c.dyadic and oc.assert_margin(c)[1] > 0


def test_occupancy_batch_host_side(tmp_path):
    """OccupancyBatch's host methods on CPU tensors"""
    c, ref = oc.by_name('hyp-3x2'), oc.reference('hyp-3x2')
    t = torch.from_numpy
    N, K = c.node_score.shape
    scenes = sd.SceneBatch(c.H, 2, K, t(c.count), torch.zeros(N, K, dtype=torch.int32), t(c.node_obbs), t(c.node_rmat),
                           torch.zeros(N, K, dtype=torch.int64), t(c.node_score))
    batch = od.OccupancyBatch(scenes, c.grid, [None if a is None else t(a) for a in ref], 2)
    assert len(batch) == 6 and (batch.H, batch.B) == (3, 2) and batch._host_arrays is None
    nx = c.grid.nx
    assert np.array_equal(batch.dense(4), od.unpack_bits(ref.occ[4], nx)) and batch.dense(4).shape == c.grid.dense_shape
    assert np.array_equal(batch.dense(1, fused=True), od.unpack_bits(ref.fused[1], nx))
    p = batch.probability(1)
    assert p.shape == c.grid.dense_shape and set(np.unique(p * 3).round(9)) <= {0.0, 1.0, 2.0, 3.0} and p.max() > 0.5
    assert np.array_equal(p >= 2 / 3 - 1e-12, batch.dense(1, fused=True))          # min_votes = 2 of 3
    iou, col = batch.iou(), batch.collision()
    assert iou.shape == (6,) and iou.dtype == np.float32 and ((0 <= iou) & (iou <= 1)).all() and iou.max() > 0
    assert col.shape == (6,) and ((0 <= col) & (col <= 1)).all() and batch.iou(fused=True).shape == (2,)
    inter, union = ref.counts[:, 2], ref.counts[:, 0] + ref.counts[:, 1] - ref.counts[:, 2]
    assert np.array_equal(iou, inter.astype(np.float32) / np.maximum(union.astype(np.float32), np.float32(1e-8)))
    path = str(tmp_path / 'occ.npz')
    batch.save_npz(path, 4)
    with np.load(path) as z:
        assert np.array_equal(z['occupancy'], batch.dense(4)) and np.array_equal(z['owner'], ref.owner[4])
        assert z['voxel'] == c.grid.voxel and np.array_equal(z['origin'], c.grid.origin)
        assert np.array_equal(z['body'], od.unpack_bits(ref.body[0], nx))
    with pytest.raises(IndexError):
        batch.dense(6)
    with pytest.raises(IndexError):
        batch.probability(2)
    bare = od.OccupancyBatch(scenes, c.grid, [t(ref.occ), None, None, None, t(ref.votes), t(ref.fused), t(ref.counts),
                                              t(ref.fused_counts)], 2)
    with pytest.raises(RuntimeError, match="ground-truth"):
        bare.iou()
    with pytest.raises(RuntimeError, match="joints"):
        bare.collision()


def test_grid():
    g = od.Grid((0.5, -1, 2), 0.05, (130, 64, 128))
    assert (g.nx, g.ny, g.nz, g.W, g.words) == (130, 64, 128, 3, 128 * 64 * 3)
    assert g.dense_shape == (128, 64, 130) and g.packed_shape == (128, 64, 3)
    assert g.centres(0)[3] == 0.5 + (3.0 + 0.5) * 0.05 and len(g.centres(2)) == 128
    for bad in (dict(origin=(0, 0)), dict(origin=(0, 0, float('nan'))), dict(origin=(0, float('inf'), 0)), dict(voxel=0.0),
                dict(voxel=-1.0), dict(voxel=float('nan')), dict(voxel=float('inf')), dict(dims=(0, 4, 4)),
                dict(dims=(4, 1025, 4)), dict(dims=(4, 4)), dict(dims=(4, 4, 2.5)), dict(origin='abc')):
        with pytest.raises(ValueError, match="Grid"):
            od.Grid(**{**dict(origin=(0, 0, 0), voxel=0.1, dims=(4, 4, 4)), **bad})
    joints = torch.tensor([[[[0.31, 1.0, -0.52, 9.0], [1.2, 1.4, 0.2, 9.0], [float('nan'), 50.0, 0.0, 9.0]]]])
    a = od.Grid.around(joints, 0.25, margin=0.5)
    assert a.voxel == 0.25 and a.origin == (-0.25, 0.5, -1.25) and a.dims == (8, 6, 8)
    lo, hi = np.array(a.origin), np.array(a.origin) + np.array(a.dims) * 0.25
    assert (lo <= np.array([0.31, 1.0, -0.52]) - 0.5).all() and (hi >= np.array([1.2, 1.4, 0.2]) + 0.5).all()
    with pytest.raises(ValueError, match="exceed"):
        od.Grid.around(joints, 0.001)
    with pytest.raises(ValueError, match="no finite"):
        od.Grid.around(joints[:, :, 2:], 0.25)


# ---- 2. the ABI ------------------------------------------------------------------------------------------------------------------
NAMES = ['p2r_occ_body', 'p2r_occ_boxes', 'p2r_occ_counts', 'p2r_occ_votes']


def test_header_parses():
    from pose2room_amd.net_utils import ap_device, consensus_device, mm_device, parse_device, vote_labels
    protos = _lib.prototypes(od.HEADER_PATH)
    assert sorted(protos) == _lib.declared_symbols(od.HEADER_PATH) == NAMES
    p = protos['p2r_occ_boxes']
    assert p.kinds == 'ii' + 'pppp' + 'ffff' + 'iii' + 'pp' and p.has_stream and p.restype is ctypes.c_int
    assert all(t is ctypes.c_double for t in p.argtypes[6:10])
    assert protos['p2r_occ_body'].kinds == 'p' + 'iiii' + 'ffff' + 'iii' + 'p' and protos['p2r_occ_body'].has_stream
    assert protos['p2r_occ_votes'].kinds == 'iiiii' + 'p' + 'i' + 'pp' and protos['p2r_occ_votes'].has_stream
    c = protos['p2r_occ_counts']
    assert c.kinds == 'iii' + 'pppp' and c.has_stream and c.argtypes[2] is ctypes.c_ulonglong
    for other in (None, ap_device.HEADER_PATH, mm_device.HEADER_PATH, vote_labels.HEADER_PATH, parse_device.HEADER_PATH,
                  sd.HEADER_PATH, consensus_device.HEADER_PATH):
        assert not set(protos) & set(_lib.declared_symbols(*([other] if other else [])))
    with open(od.HEADER_PATH) as f:
        text = f.read()
    for name, value in (('P2R_OCC_MAX_DIM', od.MAX_DIM), ('P2R_OCC_MAX_K', od.MAX_K), ('P2R_OCC_MAX_H', od.MAX_H),
                        ('P2R_OCC_NODE_CHUNK', od.NODE_CHUNK)):
        assert f"#define {name} {value} " in text
    assert (od.MAX_DIM, od.MAX_K, od.MAX_H) == (1024, sd.MAX_K, 64) and 'size_t' not in _lib._code(od.HEADER_PATH)
    assert len(od.Occupancy._fields) == 8 and len(od.COUNT_FIELDS) == 5


@built
def test_every_prototype_binds_and_library_exports_exactly_them():
    protos = _lib.prototypes(od.HEADER_PATH)
    out = subprocess.run(["nm", "-D", "--defined-only", od.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("p2r_")}
    assert exported == set(protos)
    for name, p in protos.items():
        fn = getattr(od.lib(), name)
        assert fn.argtypes == p.argtypes and fn.restype is p.restype
    assert os.path.basename(od.LIB_PATH) == 'libp2r_occupancy.so'
    for other in (_lib.LIB_PATH, sd.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", other], capture_output=True, text=True, check=True).stdout
        assert 'p2r_occ_' not in out


# ---- 3. argument checks: on the host, before any launch ---------------------------------------------------------------------
_BUF = ctypes.create_string_buffer(64)          # a non-NULL address; never read, every call is refused first
_P = ctypes.addressof(_BUF)
_GRID = dict(ox=0.0, oy=0.0, oz=0.0, voxel=0.1, nx=65, ny=3, nz=2)
BAD_GRIDS = [dict(nx=0), dict(nx=1025), dict(ny=0), dict(ny=1025), dict(nz=0), dict(nz=1025), dict(voxel=0.0),
             dict(voxel=-0.1), dict(voxel=float('nan')), dict(voxel=float('inf')), dict(ox=float('nan')),
             dict(oy=float('inf')), dict(oz=float('-inf'))]


def boxes_args(**over):
    a = dict(N=2, K=5, count=_P, node_obbs=_P, node_rmat=_P, node_score=_P, **_GRID, occ=_P, owner=_P)
    a.update(over)
    return list(a.values()) + [None]


def body_args(**over):
    a = dict(joints=_P, B=2, T=3, J=7, C=3, **_GRID, body=_P)
    a.update(over)
    return list(a.values()) + [None]


def votes_args(**over):
    a = dict(H=3, B=2, nx=65, ny=3, nz=2, occ=_P, min_votes=2, votes=_P, fused=_P)
    a.update(over)
    return list(a.values()) + [None]


def counts_args(**over):
    a = dict(N=6, B=2, words=12, a=_P, gt=_P, body=_P, counts=_P)
    a.update(over)
    return list(a.values()) + [None]


BAD_BOXES = [dict(N=-1), dict(K=-1), dict(K=1025), dict(N=1 << 21, nx=1024, ny=1024, nz=1024), dict(N=1 << 22, K=1024),
             dict(count=None), dict(node_obbs=None), dict(node_rmat=None), dict(node_score=None), dict(occ=None)] + BAD_GRIDS
BAD_BODY = [dict(B=-1), dict(T=-1), dict(J=-1), dict(C=2), dict(C=5), dict(B=1 << 12, T=1 << 12, J=1 << 12),
            dict(B=3, T=1 << 20, J=1 << 20), dict(B=1 << 21, nx=1024, ny=1024, nz=1024), dict(joints=None),
            dict(body=None)] + BAD_GRIDS
BAD_VOTES = [dict(H=0), dict(H=65), dict(B=-1), dict(min_votes=0), dict(min_votes=4), dict(nx=0), dict(nx=1025),
             dict(ny=0), dict(nz=1025), dict(H=64, B=1 << 20, nx=1024, ny=1024, nz=2), dict(occ=None), dict(fused=None)]
BAD_COUNTS = [dict(N=-1), dict(B=-1), dict(B=0), dict(B=4), dict(words=(1 << 24) + 1), dict(N=1 << 10, B=1, words=1 << 24),
              dict(a=None), dict(counts=None)]


@built
def test_entry_points_refuse_bad_arguments():
    l = od.lib()
    for fn, args, bads in ((l.p2r_occ_boxes, boxes_args, BAD_BOXES), (l.p2r_occ_body, body_args, BAD_BODY),
                           (l.p2r_occ_votes, votes_args, BAD_VOTES), (l.p2r_occ_counts, counts_args, BAD_COUNTS)):
        for bad in bads:
            assert fn(*args(**bad)) == EINVAL, (fn.__name__, bad)
    # problems without an output element: 0, and nothing launched (there is no device here to launch on)
    none = dict(count=None, node_obbs=None, node_rmat=None, node_score=None, occ=None, owner=None)
    assert l.p2r_occ_boxes(*boxes_args(N=0, **none)) == 0
    assert l.p2r_occ_body(*body_args(B=0, joints=None, body=None)) == 0
    assert l.p2r_occ_votes(*votes_args(B=0, occ=None, votes=None, fused=None)) == 0
    assert l.p2r_occ_counts(*counts_args(N=0, B=0, a=None, gt=None, body=None, counts=None)) == 0


def _cpu_inputs(N=6, K=5):
    return dict(count=torch.zeros(N, dtype=torch.int32), node_obbs=torch.zeros(N, K, 7, dtype=torch.float64),
                node_rmat=torch.zeros(N, K, 3, 3, dtype=torch.float64), node_score=torch.zeros(N, K))


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    ok, grid = _cpu_inputs(), od.Grid((0, 0, 0), 0.1, (65, 3, 2))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        od.occupancy_boxes(**ok, grid=grid)
    for name, bad in (('count', ok['count'].long()), ('count', ok['count'][:5]), ('node_obbs', ok['node_obbs'].float()),
                      ('node_rmat', ok['node_rmat'].float()), ('node_rmat', ok['node_rmat'][:, :, :2]),
                      ('node_score', ok['node_score'].double()), ('node_score', ok['node_score'][:3]),
                      ('node_obbs', ok['node_obbs'][..., :6]), ('node_obbs', 'x')):
        with pytest.raises(ValueError, match=name):
            od.occupancy_boxes(**{**ok, name: bad}, grid=grid)
    with pytest.raises(ValueError, match="Grid"):
        od.occupancy_boxes(**ok, grid=(0, 0, 0, 0.1))
    with pytest.raises(ValueError, match="at most 1024"):
        od.occupancy_boxes(**_cpu_inputs(1, 1025), grid=grid)
    joints = torch.zeros(2, 3, 7, 3)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        od.occupancy_body(joints, grid)
    for bad in (joints.double(), joints[..., :2], joints[0], 'x'):
        with pytest.raises(ValueError, match="joints"):
            od.occupancy_body(bad, grid)
    occ = torch.zeros(6, 2, 3, 2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        od.occupancy_votes(occ, 3, grid)
    for H in (0, 4, 65):
        with pytest.raises(ValueError, match="stack of"):
            od.occupancy_votes(occ, H, grid)
    for mv in (0, 4):
        with pytest.raises(ValueError, match="min_votes"):
            od.occupancy_votes(occ, 3, grid, min_votes=mv)
    for bad in (occ.int(), occ[..., :1], occ[:, :1]):
        with pytest.raises(ValueError, match="occ"):
            od.occupancy_votes(bad, 3, grid)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        od.occupancy_counts(occ, grid, gt=occ[:2], body=occ[:2])
    with pytest.raises(ValueError, match="multiple of"):
        od.occupancy_counts(occ, grid, B=4)
    with pytest.raises(ValueError, match="gt"):
        od.occupancy_counts(occ, grid, gt=occ[:3], B=2)
    with pytest.raises(ValueError, match="body"):
        od.occupancy_counts(occ, grid, body=occ[:2].int())
    with pytest.raises(TypeError, match="SceneBatch"):
        od.occupancy_of(ok, grid)
    scenes = sd.SceneBatch(3, 2, 5, ok['count'], torch.zeros(6, 5, dtype=torch.int32), ok['node_obbs'], ok['node_rmat'],
                           torch.zeros(6, 5, dtype=torch.int64), ok['node_score'])
    with pytest.raises(RuntimeError, match="GPU tensor"):
        scenes.occupancy(grid)
    with pytest.raises(ValueError, match="min_votes"):
        scenes.occupancy(grid, min_votes=4)
    with pytest.raises(ValueError, match="joints"):
        scenes.occupancy(grid, joints=torch.zeros(3, 3, 7, 3))
    with pytest.raises(ValueError, match="gt must be"):
        scenes.occupancy(grid, gt=scenes)


def test_a_missing_library_is_an_error(monkeypatch):
    monkeypatch.setattr(od._library, 'lib_path', os.path.join(os.path.dirname(od.LIB_PATH), 'libp2r_occupancy_absent.so'))
    monkeypatch.setattr(od._library, '_handle', None)
    with pytest.raises(_lib.P2RLibraryError, match="libp2r_occupancy_absent.so is missing"):
        od.lib()


# ---- 4. the cases and their teeth ----------------------------------------------------------------------------------------------
def test_sweep_covers_what_it_claims():
    cases = oc.sweep()
    assert {c.situation for c in cases} == {'nx', 'flat', 'K = 0', 'bad count', 'chunks', 'placement', 'headings',
                                            'nonfinite', 'dyadic', 'votes', 'model shape'}
    for c in cases:
        worst, zeros = oc.assert_margin(c)                    # every case, no triple excused
        assert worst >= oc.MARGIN and (zeros > 0) == c.dyadic
        ref = oc.reference(c.name)
        oc.check_occupancy(ref, ref)
        if c.situation not in ('chunks', 'model shape'):
            assert c.node_score.shape[1] <= 16 and np.prod(c.grid.dims) <= 4096, c.name
    assert sorted(c.grid.nx for c in cases if c.situation == 'nx') == [1, 63, 64, 65, 130]
    assert {c.grid.dims[1:] for c in cases if c.situation == 'flat'} == {(1, 3), (3, 1)}
    assert oc.by_name('K-0').node_score.shape == (2, 0) and not oc.reference('K-0').occ.any()
    c = oc.by_name('bad-count')
    K = c.node_score.shape[1]
    assert c.count.tolist() == [0, -3, K + 2, K] and c.H == 2
    assert oc.reference('bad-count').counts[:, 0].tolist()[:2] == [0, 0] and oc.reference('bad-count').counts[2:, 0].min() > 0
    assert sorted(c.node_score.shape[1] for c in cases if c.situation == 'chunks') == [od.NODE_CHUNK + 1, 2 * od.NODE_CHUNK + 1]
    for c in (c for c in cases if c.situation == 'chunks'):
        ref = oc.reference(c.name)
        K = c.node_score.shape[1]
        assert c.count[0] == K and ref.owner.max() == K - 1     # the last node, alone in its chunk, owns a voxel
        # voxels that nodes of two chunks cover, won by the earlier chunk here and by the later one there
        lower = od.reference_boxes(np.minimum(c.count, od.NODE_CHUNK), *oc.inputs(c)[1:], c.grid)[1]
        both = (lower >= 0) & (ref.owner >= 0)
        assert (both & (ref.owner >= od.NODE_CHUNK)).any() and (both & (ref.owner < od.NODE_CHUNK)).any()
    vol = oc.reference('placement').counts[:, 0].tolist()
    assert vol[0] == 0 and vol[1] == 65 * 4 * 3 and vol[2] == 0 and vol[3] > 0
    c = oc.by_name('headings')
    assert np.allclose(c.node_obbs[:3, 0, 6], [0, np.pi / 4, np.pi / 2]) and len({x.tobytes() for x in oc.reference('headings').occ}) >= 3
    c, ref = oc.by_name('nonfinite'), oc.reference('nonfinite')
    flat = np.concatenate([c.node_obbs[0].reshape(len(c.node_obbs[0]), -1), c.node_rmat[0].reshape(len(c.node_rmat[0]), -1)], 1)
    assert np.isnan(flat).any(1).sum() == 3 and np.isinf(flat).any(1).sum() == 6 and (np.abs(flat) == 1e300).any(1).sum() == 3
    assert set(np.unique(ref.owner[0])) == {-1, 0, len(flat) - 1} and ref.counts[1, 0] == 65 * 3 * 7
    c = oc.by_name('hyp-3x2')
    assert (c.H, len(c.count)) == (3, 6) and 0 < oc.reference('hyp-3x2').votes.max() <= 3
    assert (c.joints.shape[1] * c.joints.shape[2]) % 64 != 0 and c.joints.shape[3] == 4
    assert not np.array_equal(oc.reference('hyp-3x2').body[0], oc.reference('hyp-3x2').body[1])
    c = oc.by_name('model-shape-H10-K128')
    assert (c.H, c.node_score.shape, c.grid.dims) == (10, (20, 128), (64, 16, 64)) and oc.reference(c.name).votes.max() >= 5
    j = oc.by_name('dyadic').joints
    assert np.isnan(j).any() and np.isinf(j).any() and (np.abs(j) == np.float32(1e30)).any()


MUTATIONS = {
    'lt-for-le': (dict(strict=True), 'dyadic'),
    'no-half-offset': (dict(half_offset=False), 'headings'),
    'R-transposed': (dict(transpose=True), 'headings'),
    'size-for-half-size': (dict(full_size=True), 'placement'),
    'count-unclamped': (dict(clamp_count=False), 'bad-count'),
    'tie-to-higher-slot': (dict(tie='high'), 'dyadic'),
}
SMALL_CASES = [c.name for c in oc.sweep() if c.situation != 'model shape']


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_wrong_definitions_are_caught(mutation):
    kw, designed = MUTATIONS[mutation]
    caught = []
    for name in SMALL_CASES:
        c = oc.by_name(name)
        wrong = od.occupancy_reference(*oc.inputs(c), c.grid, c.H, c.joints, c.gt, **kw)
        try:
            oc.check_occupancy(wrong, oc.reference(name))
        except AssertionError:
            caught.append(name)
    assert designed in caught, (mutation, caught)
    if mutation == 'tie-to-higher-slot':                       # the maps agree: only the owner tells
        c = oc.by_name('dyadic')
        wrong = od.occupancy_reference(*oc.inputs(c), c.grid, c.H, c.joints, c.gt, **kw)
        assert np.array_equal(wrong.occ, oc.reference('dyadic').occ) and not np.array_equal(wrong.owner, oc.reference('dyadic').owner)


def test_a_single_bit_is_caught():
    want = oc.reference('nx-65')
    for f in ('occ', 'body', 'gt_occ', 'fused'):
        a = getattr(want, f).copy()
        a[0, 0, 0, 1] ^= np.int64(1) << np.int64(63)           # a padding bit
        with pytest.raises(AssertionError):
            oc.check_occupancy(want._replace(**{f: a}), want)
    for f in ('owner', 'votes', 'counts', 'fused_counts'):
        a = getattr(want, f).copy()
        a[(0,) * a.ndim] += 1
        with pytest.raises(AssertionError):
            oc.check_occupancy(want._replace(**{f: a}), want)
