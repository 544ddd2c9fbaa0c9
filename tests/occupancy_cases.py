"""Designed cases, the margin rule and the comparison function for the occupancy maps (csrc/occupancy.hip,
net_utils/occupancy_device.py; shared by tests/test_occupancy_cpu.py, tests/test_occupancy_gpu.py and
tests/golden/make_occupancy_golden.py).  The definition is `occupancy_device.occupancy_reference`.

Margin rule of every case (`assert_margin`, asserted by the generator for every case it hands out): for every (voxel
centre, counted node with finite parameters, axis) the definition's g = |R_a . d| - size_a / 2 is either at least
MARGIN = 1e-9 away from 0 or exactly 0.  1e-9 is about 1e6 times the rounding of the expression at the coordinates used
here (a few units, 2^-52 relative), so that any correct evaluation of the rule -- the reference's hull test included --
decides every voxel the same way.  Exactly 0 is allowed in the DYADIC cases alone: voxel = 0.25, axis-aligned boxes with
identity R whose centres and half sizes are multiples of 1/8, so that every d and every g is exact in binary floating
point and faces lie on voxel centres.  Those cases pin `<=` against `<`.

Comparison (`check_occupancy`): equality of every array -- the maps, the owners, the votes and the counts are integers.
"""
import collections
import functools
import os

import numpy as np

from pose2room_amd.net_utils import occupancy_device as od

MARGIN = 1e-9
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CHUNK = od.NODE_CHUNK

# gt: None or the (count, node_obbs, node_rmat, node_score) of the B ground-truth samples; joints: None or (B,T,J,3|4) f32
Case = collections.namedtuple('Case', 'name H grid count node_obbs node_rmat node_score joints gt situation dyadic')


def inputs(c):
    return c.count, c.node_obbs, c.node_rmat, c.node_score


@functools.lru_cache(maxsize=None)
def reference(name):
    """the definition's result for case `name`: computed once, shared, not modified"""
    c = by_name(name)
    return od.occupancy_reference(*inputs(c), c.grid, c.H, c.joints, c.gt)


def check_occupancy(got, want):
    """got, want: od.Occupancy of host arrays (None where a map is absent)"""
    for f in od.Occupancy._fields:
        g, w = getattr(got, f), getattr(want, f)
        assert (g is None) == (w is None), f
        if w is None:
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, (f, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(g, w), (f, int((g != w).sum()), np.argwhere(g != w)[:4].tolist())


def head2rot(h):
    return np.array([[np.cos(h), 0.0, -np.sin(h)], [0.0, 1.0, 0.0], [np.sin(h), 0.0, np.cos(h)]], np.float64)


def margins(count, node_obbs, node_rmat, grid):
    """-> (the smallest non-zero |g|, the number of exact zeros) over every voxel centre, counted finite node and axis"""
    N, K = node_obbs.shape[:2]
    px, py, pz = (grid.centres(a) for a in range(3))
    px, py, pz = px[None, None, :], py[None, :, None], pz[:, None, None]
    worst, zeros = np.inf, 0
    for n in range(N):
        for s in range(min(max(int(count[n]), 0), K)):
            obb, R = node_obbs[n, s], node_rmat[n, s]
            if not (np.isfinite(obb).all() and np.isfinite(R).all()):
                continue
            with np.errstate(over='ignore', invalid='ignore'):
                d0, d1, d2 = px - obb[0], py - obb[1], pz - obb[2]
                for a in range(3):
                    g = np.abs(np.abs((d0 * R[a, 0] + d1 * R[a, 1]) + d2 * R[a, 2]) - obb[3 + a] / 2.0)
                    g = g[np.isfinite(g)]
                    zeros += int((g == 0.0).sum())
                    g = g[g != 0.0]
                    if g.size:
                        worst = min(worst, float(g.min()))
    return worst, zeros


def assert_margin(c):
    worst, zeros = np.inf, 0
    for args in (inputs(c)[:3],) + ((c.gt[:3],) if c.gt is not None else ()):
        w, z = margins(*args, c.grid)
        worst, zeros = min(worst, w), zeros + z
    assert worst >= MARGIN, (c.name, worst)
    assert zeros == 0 or c.dyadic, (c.name, zeros)
    return worst, zeros


def _case(name, H, grid, count, obbs, rmat, score, joints=None, gt=None, situation='', dyadic=False):
    c = Case(name, H, grid, np.asarray(count, np.int32), np.asarray(obbs, np.float64), np.asarray(rmat, np.float64),
             np.asarray(score, np.float32), joints, gt, situation, dyadic)
    N, K = c.node_score.shape
    assert c.count.shape == (N,) and c.node_obbs.shape == (N, K, 7) and c.node_rmat.shape == (N, K, 3, 3) and N % H == 0
    assert joints is None or (joints.dtype == np.float32 and joints.shape[0] == N // H)
    assert gt is None or len(gt[0]) == N // H
    assert_margin(c)
    return c


# ---- building blocks -------------------------------------------------------------------------------------------------------
def random_nodes(rng, N, K, kept, grid, size=(0.15, 0.6)):
    """N samples of K slots, `kept` (an int or a list per sample) of them counted: rotated boxes with centres inside the
    grid's extent, sizes as a share of its largest extent, float32 scores with repeats; unused slots zero"""
    ext = np.array(grid.dims, np.float64) * grid.voxel
    lo = np.array(grid.origin)
    kept = [kept] * N if np.isscalar(kept) else list(kept)
    count = np.array(kept, np.int32)
    obbs, rmat, score = np.zeros((N, K, 7)), np.zeros((N, K, 3, 3)), np.zeros((N, K), np.float32)
    for n in range(N):
        for s in range(min(max(kept[n], 0), K)):
            h = rng.uniform(-np.pi, np.pi)
            sz = np.maximum(rng.uniform(size[0], size[1], 3) * np.minimum(ext.max(), 4 * ext), 0.6 * grid.voxel)
            obbs[n, s] = np.concatenate([lo + rng.uniform(0.0, 1.0, 3) * ext, sz, [h]])
            rmat[n, s] = head2rot(h)
            score[n, s] = np.float32(rng.integers(1, 17) / 16.0)            # sixteen values: plenty of ties
    return count, obbs, rmat, score


def random_joints(rng, B, T, J, C, grid):
    """joints scattered over the grid's extent and a little beyond it"""
    ext = np.array(grid.dims, np.float64) * grid.voxel
    x = np.array(grid.origin) + rng.uniform(-0.1, 1.1, (B, T, J, 3)) * ext
    out = np.zeros((B, T, J, C), np.float32)
    out[..., 0:3] = x
    if C == 4:
        out[..., 3] = rng.uniform(0, 1, (B, T, J))
    return out


def _random_case(name, seed, H, B, K, kept, dims, voxel=0.1, origin=(-0.35, 0.2, 1.15), T=3, J=7, C=3, with_gt=True,
                 situation='', size=(0.1, 0.4)):
    rng = np.random.default_rng(seed)
    grid = od.Grid(origin, voxel, dims)
    nodes = random_nodes(rng, H * B, K, kept, grid, size)
    gt = random_nodes(rng, B, 4, 3, grid, size) if with_gt else None
    return _case(name, H, grid, *nodes, random_joints(rng, B, T, J, C, grid), gt, situation)


def _dyadic_box(cx, cy, cz, sx, sy, sz):
    return np.array([cx, cy, cz, sx, sy, sz, 0.0])


def dyadic_case(shift=(0, 0, 0), name='dyadic'):
    """voxel 0.25, origin on a multiple of it, identity R: faces on voxel centres (g exactly 0 there), an overlap of two
    boxes with equal scores and one with a NaN score for the owner rule, joints exactly on voxel boundaries.  `shift`
    moves the origin, the boxes and the joints by whole voxels."""
    v = 0.25
    t = np.array(shift, np.float64) * v
    grid = od.Grid(tuple(t), v, (12, 6, 5))
    # centres of the voxels are at 0.125 + 0.25 i
    boxes = [_dyadic_box(1.125, 0.625, 0.625, 1.0, 0.5, 0.5),         # faces x = 0.625, 1.625: voxel centres 2 and 6
             _dyadic_box(1.625, 0.625, 0.625, 1.0, 1.0, 0.5),         # overlaps the first, the same score: slot 0 owns
             _dyadic_box(1.625, 0.875, 0.625, 0.5, 0.5, 0.5),         # a NaN score: owns nothing that another covers
             _dyadic_box(2.625, 1.125, 0.875, 0.25, 0.25, 0.25),      # a NaN score alone in its voxels: owns them
             _dyadic_box(0.375, 1.125, 1.0, 0.5, 0.5, 0.25)]          # the highest score in the highest slot: it shares
    #                                                                   one corner voxel with slot 0, and owns it
    K = 6
    obbs, rmat, score = np.zeros((2, K, 7)), np.zeros((2, K, 3, 3)), np.zeros((2, K), np.float32)
    for s, b in enumerate(boxes):
        obbs[0, s], rmat[0, s] = b + np.concatenate([t, np.zeros(4)]), np.eye(3)
    score[0, :5] = [0.5, 0.5, np.nan, np.nan, 0.75]
    # sample 1: the same two overlapping boxes, the higher score in the higher slot
    obbs[1, 0], obbs[1, 1] = obbs[0, 0], obbs[0, 1]
    rmat[1, 0] = rmat[1, 1] = np.eye(3)
    score[1, :2] = [0.25, 0.5]
    joints = np.zeros((2, 3, 7, 4), np.float32)
    joints[..., 0:3] = [0.3, 0.3, 0.3]
    special = [(0.5, 0.25, 0.75), (0.0, 0.0, 0.0), (3.0, 0.3, 0.3), (2.99, 1.49, 1.24), (-0.01, 0.3, 0.3),
               (np.nan, 0.3, 0.3), (0.3, np.inf, 0.3), (0.3, 0.3, -np.inf), (1e30, 0.3, 0.3), (0.3, -1e30, 0.3),
               (0.3, 0.3, 1.25), (1.75, 1.25, 1.0)]
    flat = joints[0].reshape(-1, 4)
    flat[:len(special), 0:3] = special
    joints[..., 0:3] += t.astype(np.float32)                                 # whole dyadic voxels: exact in float32
    gt = (np.array([1, 1], np.int32), obbs[:, 1:2].copy(), rmat[:, 1:2].copy(), np.ones((2, 1), np.float32))
    return _case(name, 1, grid, [5, 2], obbs, rmat, score, joints, gt, 'dyadic', dyadic=True)


def placement_case():
    """sample 0: a box wholly outside the grid; sample 1: a box that contains the whole grid; sample 2: a box thinner than
    a voxel that covers no centre; sample 3: the same thin box moved onto a plane of centres"""
    grid = od.Grid((0.0, 0.0, 0.0), 0.1, (65, 4, 3))
    K = 2
    obbs, rmat = np.zeros((4, K, 7)), np.zeros((4, K, 3, 3))
    h = 0.3
    rows = [[20.0, 0.2, 0.15, 1.0, 1.0, 1.0, h], [3.0, 0.2, 0.15, 40.0, 9.0, 9.0, h],
            [3.2, 0.2004, 0.15, 5.0, 0.02, 5.0, 0.0], [3.2, 0.25, 0.15, 5.0, 0.02, 5.0, 0.0]]
    for n, r in enumerate(rows):
        obbs[n, 0], rmat[n, 0] = r, head2rot(r[6])
    return _case('placement', 1, grid, [1, 1, 1, 1], obbs, rmat, np.full((4, K), 0.5, np.float32), None, None, 'placement')


def headings_case():
    grid = od.Grid((-1.0, 0.0, -1.0), 0.1, (33, 3, 31))
    rng = np.random.default_rng(5)
    hs = [0.0, np.pi / 4, np.pi / 2, rng.uniform(-np.pi, np.pi)]
    obbs, rmat = np.zeros((4, 1, 7)), np.zeros((4, 1, 3, 3))
    for n, h in enumerate(hs):
        obbs[n, 0] = [0.6171, 0.1503, 0.4907, 1.803, 0.2507, 0.6011, h]
        rmat[n, 0] = head2rot(h)
    return _case('headings', 1, grid, [1] * 4, obbs, rmat, np.full((4, 1), 0.5, np.float32), None, None, 'headings')


def nonfinite_case():
    """one good node in slot 0 and nodes with NaN, +inf and 1e300 in the centre, the size, the heading and R behind it; the
    nodes with a non-finite value cover nothing, those with 1e300 are evaluated like any other (a centre or a matrix
    entry of 1e300 and a size of -1e300 leave the node without a voxel; sample 1 holds a node with a size of 1e300, which
    covers the whole grid)"""
    grid = od.Grid((0.0, 0.0, 0.0), 0.1, (65, 3, 7))
    good = np.array([3.017, 0.1503, 0.3507, 2.003, 0.2507, 0.4011, 0.4])
    bads = [(0, np.nan), (1, np.inf), (2, 1e300), (3, np.nan), (4, np.inf), (5, -np.inf), (3, -1e300), (6, np.inf),
            ('R', np.nan), ('R', np.inf), ('R', 1e300), ('R', -np.inf)]
    K = len(bads) + 2
    obbs, rmat = np.zeros((2, K, 7)), np.zeros((2, K, 3, 3))
    obbs[0, 0], rmat[0, 0] = good, head2rot(good[6])
    obbs[1, 0], rmat[1, 0] = [3.0, 0.2, 0.3, 50.0, 1e300, 50.0, 0.4], head2rot(0.4)
    for s, (where, v) in enumerate(bads, 1):
        # a big box that would cover everything: a node that is wrongly kept shows in every voxel
        obbs[0, s], rmat[0, s] = [3.0, 0.2, 0.3, 50.0, 50.0, 50.0, 0.4], head2rot(0.4)
        if where == 'R':
            rmat[0, s, s % 3, (s + 1) % 3] = v
        else:
            obbs[0, s, where] = v
    obbs[0, K - 1], rmat[0, K - 1] = [5.513, 0.1503, 0.3507, 0.503, 0.2507, 0.4011, 0.0], np.eye(3)     # a good node at the end
    score = np.stack([np.linspace(0.9, 0.1, K).astype(np.float32)] * 2)
    return _case('nonfinite', 1, grid, [K, 1], obbs, rmat, score, None, None, 'nonfinite')


def bad_count_case():
    """H = 2, B = 2: counts 0, negative, above K and K.  Sample 2 (count K + 2) is followed by a sample whose nodes cover
    other voxels: a count that is not clamped runs on into them."""
    rng = np.random.default_rng(11)
    grid = od.Grid((0.0, 0.0, 0.0), 0.1, (40, 3, 4))
    K = 3
    count, obbs, rmat, score = random_nodes(rng, 4, K, K, grid, size=(0.1, 0.3))
    obbs[2, :, 0] = rng.uniform(0.3, 1.5, K)                  # sample 2 in the low x, sample 3 in the high x
    obbs[3, :, 0] = rng.uniform(2.5, 3.7, K)
    count = np.array([0, -3, K + 2, K], np.int32)
    return _case('bad-count', 2, grid, count, obbs, rmat, score, random_joints(rng, 2, 3, 7, 3, grid), None, 'bad count')


def model_shape_case():
    """K = 128, H = 10, B = 2, a 64 x 16 x 64 grid; about 10 % of the proposals kept"""
    rng = np.random.default_rng(21)
    grid = od.Grid((-3.2, 0.0, -3.2), 0.1, (64, 16, 64))
    kept = rng.integers(9, 17, 20).tolist()
    nodes = random_nodes(rng, 20, 128, kept, grid, size=(0.05, 0.3))
    gt = random_nodes(rng, 2, 8, 6, grid, size=(0.05, 0.3))
    return _case('model-shape-H10-K128', 10, grid, *nodes, random_joints(rng, 2, 64, 53, 4, grid), gt, 'model shape')


def copies(c, H):
    """H hypotheses that all hold the scenes of case c (H = 1)"""
    assert c.H == 1
    rep = lambda a: np.concatenate([a] * H, 0)                                  # noqa: E731
    return c._replace(name=f'{c.name}-x{H}', H=H, count=rep(c.count), node_obbs=rep(c.node_obbs),
                      node_rmat=rep(c.node_rmat), node_score=rep(c.node_score))


@functools.lru_cache(maxsize=None)
def sweep():
    cases = []
    for nx in (1, 63, 64, 65, 130):                          # the word boundary and the padding bits
        cases.append(_random_case(f'nx-{nx}', 100 + nx, 1, 1, 5, 4, (nx, 3, 2), situation='nx'))
    cases.append(_random_case('ny-1', 3, 1, 1, 5, 4, (65, 1, 3), situation='flat'))
    cases.append(_random_case('nz-1', 4, 1, 1, 5, 4, (65, 3, 1), situation='flat'))
    cases.append(_random_case('K-0', 5, 1, 2, 0, 0, (65, 3, 2), situation='K = 0'))
    cases.append(bad_count_case())
    # one node above the LDS chunk of the kernel, and two chunks plus one: all counted, overlapping across the chunks
    cases.append(_random_case(f'K-{CHUNK + 1}', 6, 1, 1, CHUNK + 1, CHUNK + 1, (70, 4, 5), with_gt=False,
                              situation='chunks', size=(0.03, 0.12)))
    cases.append(_random_case(f'K-{2 * CHUNK + 1}', 7, 1, 2, 2 * CHUNK + 1, [2 * CHUNK + 1, CHUNK + 3], (70, 4, 5),
                              with_gt=False, situation='chunks', size=(0.03, 0.12)))
    cases.append(placement_case())
    cases.append(headings_case())
    cases.append(nonfinite_case())
    cases.append(dyadic_case())
    cases.append(_random_case('hyp-3x2', 8, 3, 2, 6, [4, 3, 0, 6, 2, 5], (66, 5, 9), T=5, J=13, C=4, situation='votes'))
    cases.append(model_shape_case())
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


def by_name(name):
    for c in sweep():
        if c.name == name:
            return c
    raise KeyError(name)


def g18():
    with np.load(os.path.join(GOLDEN, 'g18_occupancy.npz')) as z:
        return {k: z[k] for k in z.files}


def g18_design():
    """two scenes of three rotated boxes each on a 32 x 16 x 32 grid of 0.1 m -> (grid, count, obbs, rmat, score); the
    grid's origin is chosen so that every voxel centre keeps 1e-7 from every face (asserted by the golden script)"""
    rng = np.random.default_rng(18)
    grid = od.Grid((-1.6013, 0.0021, -1.5987), 0.1, (32, 16, 32))
    obbs, rmat = np.zeros((2, 3, 7)), np.zeros((2, 3, 3, 3))
    for n in range(2):
        for s in range(3):
            h = rng.uniform(-np.pi, np.pi)
            obbs[n, s] = np.concatenate([rng.uniform([-1.0, 0.3, -1.0], [1.0, 1.0, 1.0]), rng.uniform(0.4, 1.6, 3), [h]])
            rmat[n, s] = head2rot(h)
    return grid, np.array([3, 3], np.int32), obbs, rmat, np.full((2, 3), 0.5, np.float32)
