"""Float64 NumPy definitions, comparison functions and designed cases for the scene read-out on the device
(csrc/scene.hip, net_utils/scene_device.py; shared by tests/test_scene_cpu.py, tests/test_scene_gpu.py and
tests/golden/make_scene_golden.py).

The three definitions are written from include/p2r_scene.h, not from the kernels:
  * `nodes_def`   the keep rule (double)obj_prob > threshold && pred_mask == 1, compaction in ascending proposal index,
                  head2rot of the heading;
  * `contact_def` d(t) = max over joints and axes of |(v0 R[a,0] + v1 R[a,1]) + v2 R[a,2]| - size_a / 2 with v = x - c in
                  float64, the FIRST frame that attains the minimum, and where the minimum is attained;
  * `unique_def`  first[t] = the first frame whose row equals frame t's element by element (==), by comparing all pairs.
Each takes switches that turn it into a wrong definition (last minimum, adjacent-only de-duplication, no mask term, >=);
the CPU test feeds those through the comparison functions below and expects each to be caught.

Margin rule of every contact case (`assert_contact_margins`): for every node, the minimum of d over frames is at least
CONTACT_MARGIN = 1e-6 m below d of every frame WITH A DIFFERENT ROW -- about 1e9 times the rounding bound `dist_bound`
at room scale, so no implementation's rounding can move an argmin; rows that are equal give the same d bit for bit and
the first wins.  The one exception is declared by the case (`mirror`): a frame and its mirror image about a plane
through the centre of an axis-aligned box whose coordinates are multiples of 2^-10.  There v' = -v in one coordinate
exactly, every product and sum of the definition changes sign without changing its rounding, and d is equal bit for bit
in any implementation that follows the operation order of the header: the tie is exact, and the lower index must win.
"""
import collections
import functools
import os

import numpy as np

from tests import parse_cases as pc

CONTACT_MARGIN = 1e-6
RMAT_TOL = dict(rtol=0, atol=1e-9)     # what tests/test_mm_device_gpu.py applies to the device's heading: the same libm
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

Nodes = collections.namedtuple('Nodes', 'count inst_idx node_obbs node_rmat node_cls node_score')
Contact = collections.namedtuple('Contact', 'frame dist d joint')          # d: {(n, s): (T,) f64}; joint: (N,K) attaining
Unique = collections.namedtuple('Unique', 'count index rank')
Case = collections.namedtuple('Case', 'name obbs obj_prob pred_mask pred_cls threshold joints mirror skip_rows')


# ---- the definitions ---------------------------------------------------------------------------------------------------
def head2rot(h):
    """(...,) -> (...,3,3): rows (cos h, 0, -sin h), (0, 1, 0), (sin h, 0, cos h)"""
    h = np.asarray(h, np.float64)
    R = np.zeros(h.shape + (3, 3))
    R[..., 0, 0], R[..., 0, 2], R[..., 1, 1], R[..., 2, 0], R[..., 2, 2] = np.cos(h), -np.sin(h), 1.0, np.sin(h), np.cos(h)
    return R


def nodes_def(obbs, obj_prob, pred_mask, pred_cls, threshold, use_mask=True, strict=True):
    assert obbs.dtype == np.float64 and obj_prob.dtype == np.float32 and pred_mask.dtype == np.uint8
    N, K = obj_prob.shape
    p = obj_prob.astype(np.float64)
    keep = (p > threshold) if strict else (p >= threshold)
    if use_mask:
        keep = keep & (pred_mask == 1)
    out = Nodes(np.zeros(N, np.int32), np.full((N, K), -1, np.int32), np.zeros((N, K, 7)), np.zeros((N, K, 3, 3)),
                np.zeros((N, K), np.int64), np.zeros((N, K), np.float32))
    for n in range(N):
        idx = np.nonzero(keep[n])[0]
        m = len(idx)
        out.count[n] = m
        out.inst_idx[n, :m] = idx
        out.node_obbs[n, :m] = obbs[n, idx]
        out.node_rmat[n, :m] = head2rot(obbs[n, idx, 6])
        out.node_cls[n, :m] = pred_cls[n, idx]
        out.node_score[n, :m] = obj_prob[n, idx]
    return out


def box_distance(x, obb, R):
    """x (..., 3) f32 / f64 coordinates -> (..., 3) f64: g_a of the header, in its operation order"""
    v = np.asarray(x, np.float64)[..., 0:3] - obb[0:3]
    g = [np.abs((v[..., 0] * R[a, 0] + v[..., 1] * R[a, 1]) + v[..., 2] * R[a, 2]) - obb[3 + a] / 2.0 for a in range(3)]
    return np.stack(g, -1)


def contact_def(joints, node_obbs, node_rmat, count, pick='first'):
    """joints (B,T,J,C) f32; sample n reads row n % B"""
    assert joints.dtype == np.float32 and node_obbs.dtype == np.float64 and node_rmat.dtype == np.float64
    N, K = node_obbs.shape[:2]
    B = joints.shape[0]
    frame, dist = np.full((N, K), -1, np.int32), np.zeros((N, K))
    joint, d_all = np.zeros((N, K), np.int64), {}
    for n in range(N):
        for s in range(min(int(count[n]), K)):
            g = box_distance(joints[n % B], node_obbs[n, s], node_rmat[n, s])             # (T,J,3)
            per_joint = g.max(-1)
            d = per_joint.max(-1)
            t = int(np.argmin(d)) if pick == 'first' else len(d) - 1 - int(np.argmin(d[::-1]))
            frame[n, s], dist[n, s], joint[n, s], d_all[(n, s)] = t, d[t], int(np.argmax(per_joint[t])), d
    return Contact(frame, dist, d_all, joint)


def rows_equal_matrix(rows):
    """(T, ...) -> (T,T) bool: NumPy's row equality, element by element with == (so -0 == +0 and NaN != NaN)"""
    flat = rows.reshape(len(rows), -1)
    return np.stack([(flat == r).all(-1) for r in flat])


def unique_def(joints, adjacent_only=False):
    B, T = joints.shape[:2]
    count, index, rank = np.zeros(B, np.int32), np.full((B, T), -1, np.int32), np.zeros((B, T), np.int32)
    for b in range(B):
        eq = rows_equal_matrix(joints[b])
        if adjacent_only:
            first = np.arange(T)
            for t in range(1, T):
                if eq[t, t - 1]:
                    first[t] = first[t - 1]
        else:
            first = np.array([int(np.argmax(eq[t, :t + 1])) if eq[t, t] else t for t in range(T)])
        firsts = np.nonzero(first == np.arange(T))[0]
        count[b] = len(firsts)
        index[b, :len(firsts)] = firsts
        rank[b] = np.searchsorted(firsts, first)
    return Unique(count, index, rank)


def dist_bound(x, obb):
    """12 * 2^-53 * (||x - c||_1 + max size / 2): at most six roundings per implementation on the way to g"""
    return 12 * 2.0 ** -53 * (np.abs(np.asarray(x, np.float64)[0:3] - obb[0:3]).sum() + obb[3:6].max() / 2.0)


# ---- comparison functions, shared by the CPU and the GPU test -----------------------------------------------------------
def check_nodes(got, want, rmat_tol=None):
    """got, want: Nodes of host arrays.  Everything equal; node_obbs bit for bit; node_rmat within rmat_tol (None: equal)"""
    assert np.array_equal(got.count, want.count), (got.count, want.count)
    assert np.array_equal(got.inst_idx, want.inst_idx)
    assert np.array_equal(got.node_cls, want.node_cls)
    assert np.array_equal(got.node_obbs.view(np.int64), want.node_obbs.view(np.int64))
    assert np.array_equal(got.node_score.view(np.int32), want.node_score.view(np.int32))
    if rmat_tol is None:
        assert np.array_equal(got.node_rmat, want.node_rmat)
    else:
        np.testing.assert_allclose(got.node_rmat, want.node_rmat, **rmat_tol)
        structural = np.ones((3, 3), bool)
        structural[[0, 0, 2, 2], [0, 2, 0, 2]] = False                 # the zeros and the one are exact
        assert np.array_equal(got.node_rmat[..., structural], want.node_rmat[..., structural])


def check_contact(frame, dist, want, joints, node_obbs, count, skip_rows=()):
    """frame (N,K) / dist (N,K) against `want` = contact_def of the same nodes: frames equal, dist within dist_bound at
    the attaining joint, -1 / 0 beyond count.  Samples whose joints row is in skip_rows (a NaN row: unspecified) must
    only name a frame of the recording."""
    N, K = frame.shape
    B, T = joints.shape[:2]
    for n in range(N):
        m = min(int(count[n]), K)
        assert np.array_equal(frame[n, m:], np.full(K - m, -1)) and not dist[n, m:].any(), n
        if n % B in skip_rows:
            assert ((frame[n, :m] >= 0) & (frame[n, :m] < T)).all(), n
            continue
        assert np.array_equal(frame[n, :m], want.frame[n, :m]), (n, frame[n, :m], want.frame[n, :m])
        for s in range(m):
            t = want.frame[n, s]
            bound = dist_bound(joints[n % B, t, want.joint[n, s]], node_obbs[n, s])
            assert abs(dist[n, s] - want.dist[n, s]) <= bound, (n, s, dist[n, s], want.dist[n, s], bound)


def check_unique(got, want):
    assert np.array_equal(got.count, want.count), (got.count, want.count)
    assert np.array_equal(got.index, want.index)
    assert np.array_equal(got.rank, want.rank)


def assert_contact_margins(joints, contact, count, mirror=None, skip_rows=()):
    """the margin rule of the module docstring; mirror = (row b, t_low, t_high) declares the one exact tie"""
    B = joints.shape[0]
    eqs = [rows_equal_matrix(joints[b]) for b in range(B)]
    worst = np.inf
    for (n, s), d in contact.d.items():
        b = n % B
        if b in skip_rows:
            continue
        t = contact.frame[n, s]
        assert t == int(np.argmin(d))
        other = ~eqs[b][t]
        if mirror is not None and b == mirror[0] and t in mirror[1:] and d[mirror[1]] == d[mirror[2]]:
            assert t == mirror[1], "an exact tie of the mirror pair goes to the lower frame"
            other[mirror[2]] = False
        assert (d[~other] == d[t]).all()                               # equal rows: equal bits
        if other.any():
            worst = min(worst, (d[other] - d[t]).min())
    assert worst >= CONTACT_MARGIN, worst
    return worst


# ---- designed cases ----------------------------------------------------------------------------------------------------
def skeletons(rng, hips, J, C):
    """hips (B,T,3) -> (B,T,J,C) f32: joint 0 is the hip, the others keep a fixed offset from it plus a small motion; a
    fourth channel holds a height-like value of its own"""
    B, T = hips.shape[:2]
    limb = rng.normal(0, 0.25, (B, 1, J, 3))
    limb[:, :, 0] = 0.0
    x = hips[:, :, None, :] + limb + rng.normal(0, 0.02, (B, T, J, 3))
    if C == 4:
        x = np.concatenate([x, rng.uniform(0, 2, (B, T, J, 1))], -1)
    return x.astype(np.float32)


def add_frame_content(joints, nan_row=None):
    """adjacent duplicates, distant duplicates, a +-0.0 pair, in every row; a NaN frame in row nan_row.  Needs T >= 32."""
    B, T, J, C = joints.shape
    assert T >= 32
    joints[:, 7] = joints[:, 6]                              # adjacent
    joints[:, 8] = joints[:, 6]
    joints[:, T - 2] = joints[:, 3]                          # distant
    joints[:, T // 2] = joints[:, 3]
    joints[:, 11, J // 2, 1] = 0.0
    joints[:, 12] = joints[:, 11]                            # equal under ==, different bits
    joints[:, 12, J // 2, 1] = -0.0
    joints[:, 25] = joints[:, 11]
    if nan_row is not None:
        joints[nan_row, 17] = joints[nan_row, 16]            # two identical rows with a NaN: both stay
        joints[nan_row, 16:18, J - 1, C - 1] = np.nan
    return joints


def _walk(rng, B, T):
    t = np.linspace(0.0, 1.0, T) if T > 1 else np.zeros(1)
    ph = rng.uniform(0, 6, (B, 2, 1))
    return np.stack([3.0 * np.cos(2.3 * np.pi * t + ph[:, 0]), 0.9 + 0.05 * np.sin(9 * t) + 0 * ph[:, 0],
                     2.5 * np.sin(1.7 * np.pi * t + ph[:, 1])], -1) + rng.normal(0, 0.02, (B, T, 3))


def make_case(name, K, T, J, C, H, kept, seed):
    """B = 2 joints rows, N = 2 H samples.  kept: 'none' | 'all' | 'mixed'.  For T >= 32: the frame content of
    `add_frame_content` with a NaN frame in row 1 (in the last channel: with C = 3 the contact result of that row's
    samples is unspecified and they are in skip_rows; with C = 4 the NaN is in the channel the contact search does not
    read), and in row 0 a mirror pair for proposal 0 (kept unless 'none')."""
    B, N, thr = 2, 2 * H, 0.5
    for s in range(seed, seed + 200):
        rng = np.random.default_rng(s)
        joints = skeletons(rng, _walk(rng, B, T), J, C)
        obbs = np.concatenate([rng.uniform(-4, 4, (N, K, 1)), rng.uniform(0, 2, (N, K, 1)), rng.uniform(-4, 4, (N, K, 1)),
                               np.exp(rng.normal(-0.2, 0.5, (N, K, 3))), rng.uniform(-np.pi, np.pi, (N, K, 1))], -1)
        prob = rng.uniform(0.05, 0.95, (N, K)).astype(np.float32)
        mask = (rng.uniform(size=(N, K)) < 0.6).astype(np.uint8)
        if kept == 'all':
            prob, mask = np.maximum(prob, np.float32(0.55)), np.ones_like(mask)
        elif kept == 'none':
            prob = np.where(mask == 1, np.minimum(prob, np.float32(0.45)), prob)
        else:                                                # the decisions a wrong keep rule gets wrong
            if K >= 4:
                prob[:, 1], mask[:, 1] = 0.5, 1              # exactly the threshold: not kept
                prob[:, 2], mask[:, 2] = 0.9, 0              # suppressed by the NMS
                prob[:, 3], mask[:, 3] = 0.9, 2              # a mask value that is not 1
        mirror, skip_rows = None, ()
        if T >= 32:
            joints = add_frame_content(joints, nan_row=1)
            skip_rows = (1,) if C == 3 else ()
            if kept != 'none':
                # proposal 0 of the samples on row 0: an axis-aligned box on a 2^-10 grid, a frame inside it and its mirror
                # image about the plane x = centre.x; the mirror comes first
                grid = lambda a: np.round(np.asarray(a) * 1024) / 1024                       # noqa: E731
                c = grid(rng.uniform(-1, 1, 3))
                obbs[0::B, 0] = np.concatenate([c, [1.0, 1.5, 0.75], [0.0]])
                prob[0::B, 0], mask[0::B, 0] = 0.9, 1
                lo, hi = 5, 20
                inside = c + grid(rng.uniform(-0.2, 0.2, (J, 3)))
                joints[0, hi, :, 0:3] = inside
                inside[:, 0] = 2 * c[0] - inside[:, 0]
                joints[0, lo, :, 0:3] = inside
                if C == 4:
                    joints[0, lo, :, 3] = joints[0, hi, :, 3]
                assert not np.array_equal(joints[0, lo], joints[0, hi])
                mirror = (0, lo, hi)
        case = Case(name, obbs, prob, mask, rng.integers(0, 22, (N, K)).astype(np.int64), thr, joints, mirror, skip_rows)
        nd = nodes_def(obbs, prob, mask, case.pred_cls, thr)
        ct = contact_def(joints, nd.node_obbs, nd.node_rmat, nd.count)
        try:
            assert_contact_margins(joints, ct, nd.count, mirror, skip_rows)
            if mirror is not None:                           # the tie is there, and it is the minimum
                d = ct.d[(0, 0)]
                assert nd.inst_idx[0, 0] == 0 and ct.frame[0, 0] == mirror[1] and d[mirror[1]] == d[mirror[2]]
        except AssertionError:
            continue
        return case
    raise AssertionError(f"{name}: no seed in {seed}..{seed + 199} with clear contact decisions")


SWEEP_K = (1, 24, 65, 128)
SWEEP_T = (1, 40, 257)
_KEPT = ('mixed', 'all', 'none')


@functools.lru_cache(maxsize=None)
def sweep():
    """-> tuple of Case: every K with every T; J, C, H and the kept share cycle with periods 2, 2, 2 and 3 against the
    index i, i // 2 and i // 4, so every value of each meets every T and both parities of the others."""
    out, i = [], 0
    for K in SWEEP_K:
        for T in SWEEP_T:
            J, C, H, kept = (53, 1)[i % 2], (3, 4)[(i // 2) % 2], (1, 2)[(i // 4 + i) % 2], _KEPT[i % 3]
            out.append(make_case(f"K{K}-T{T}-J{J}-C{C}-H{H}-{kept}", K, T, J, C, H, kept, 7000 + 200 * i))
            i += 1
    # the combinations the cycling leaves out: all kept at the wave-crossing K with full skeletons and both C, H = 2
    out.append(make_case("K65-T40-J53-C4-H2-all", 65, 40, 53, 4, 2, 'all', 9900))
    out.append(make_case("K128-T257-J53-C3-H2-mixed", 128, 257, 53, 3, 2, 'mixed', 10100))
    out.append(make_case("K24-T40-J1-C3-H1-none", 24, 40, 1, 3, 1, 'none', 10300))
    return tuple(out)


def g15_design():
    """The designed inputs of G15: the recorded parse results of G14 (N = 3, K = 24: corners, objectness probability,
    keep mask, classes) and full skeletons of 53 joints around G14's hip track, T = 40, with duplicated frames; the
    first seed whose contact decisions are clear (deterministic: the seeds are tried in order)."""
    from pose2room_amd.net_utils.multi_modal_eval import corners_to_params
    case, z = pc.g14()
    corners, prob, mask = z['pred_corners_3d'], z['obj_prob'], z['pred_mask']
    cls = z['pred_sem_cls'].astype(np.int64)
    obbs = corners_to_params(corners).reshape(corners.shape[0], corners.shape[1], 7)
    nd = nodes_def(obbs, prob, mask, cls, 0.5)
    assert nd.count.min() >= 1
    for s in range(1500, 1700):
        rng = np.random.default_rng(s)
        joints = add_frame_content(skeletons(rng, case.joints[:, :, 0, :].astype(np.float64), 53, 3))
        try:
            assert_contact_margins(joints, contact_def(joints, nd.node_obbs, nd.node_rmat, nd.count), nd.count)
        except AssertionError:
            continue
        return dict(pred_corners_3d=corners, obj_prob=prob, pred_mask=mask, pred_sem_cls=cls, input_joints=joints,
                    dump_threshold=np.float64(0.5))
    raise AssertionError("g15: no seed with clear contact decisions")


def g15():
    return np.load(os.path.join(GOLDEN, 'g15_scene.npz'))
