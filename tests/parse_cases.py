"""Cases and a float64 NumPy restatement for prediction parsing on the device (csrc/parse_boxes.hip,
net_utils/parse_device.py; shared by tests/test_parse_device_cpu.py, tests/test_parse_device_gpu.py and
tests/golden/make_parse_golden.py).

`restate` is the arithmetic of include/p2r_parse.h written once more, in NumPy: float32 where the header says float32,
float64 elsewhere, in the header's order.  Besides the five outputs it returns how far every far-box and size-bound
decision is from flipping; `nms_margins` does the same for the score-order and overlap decisions of the NMS that follows.
A case whose margins are all >= MARGIN cannot change a mask through the one-ulp differences between the device's
exp / atan2 / cos / sin and NumPy's, which is what lets the GPU tests demand bit-equal masks with no case left out; the
generator below redraws boxes until its cases have GEN_MARGIN, and the CPU test asserts MARGIN on every one of them.
"""
import collections
import functools
import os

import numpy as np

MARGIN = 1e-4            # the project's decision margin (tests/test_eval_gpu.py)
GEN_MARGIN = 2e-4        # what the generator asks of its own cases
CHUNK = 256              # frames the kernel stages per pass (parse_device.CHUNK_FRAMES; asserted equal in the CPU test)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

CORNER_SIGNS = np.array([(-1, -1, -1), (+1, -1, -1), (+1, +1, -1), (-1, +1, -1),
                         (-1, -1, +1), (+1, -1, +1), (+1, +1, +1), (-1, +1, +1)], np.float64)

Case = collections.namedtuple(
    'Case', 'name center size_log heading_sc objectness sem_scores cls_in joints origin_joint contact_dist '
            'remove_far_box nms_mode')
Restated = collections.namedtuple('Restated', 'corners boxes obj_prob pred_cls nonempty far_margin size_margin n_inside first_inside')


def restate(center, size_log, heading_sc, objectness, sem_scores, cls_in=None, joints=None, origin_joint=0,
            contact_dist=1.0, remove_far_box=True, nms_mode=0):
    """-> Restated: corners (N,K,8,3) f64, boxes (N,K,7|8) f64, obj_prob (N,K) f32, pred_cls (N,K) i64, nonempty (N,K) u8,
    far_margin (N,K) f64: | min over frames of max over axes of (|l_i| - hf_i) | (inf without the filter or for a box
    whose size already decides), size_margin (N,K) f64: distance of the nearest size component to 0.01 or 10, n_inside
    (N,K): the number of frames inside the enlarged box, first_inside (N,K): the first of them (0 without the filter)."""
    assert center.dtype == size_log.dtype == objectness.dtype == np.float32 and heading_sc.dtype == np.float64
    N, K = center.shape[:2]
    size = np.exp(size_log)                                                     # f32
    assert size.dtype == np.float32
    theta = np.arctan2(heading_sc[..., 0], heading_sc[..., 1])
    c, s = np.cos(theta), np.sin(theta)
    zero, one = np.zeros_like(c), np.ones_like(c)
    R = np.stack([np.stack([c, zero, -s], -1), np.stack([zero, one, zero], -1), np.stack([s, zero, c], -1)], -2)  # (N,K,3,3)
    halff = size / np.float32(2.0)                                              # f32
    vectors = halff.astype(np.float64)[..., None] * R                           # row i = half_i * R_i
    ctr = center.astype(np.float64)
    corners = ctr[:, :, None, :] + CORNER_SIGNS[:, 0, None] * vectors[:, :, None, 0, :]
    corners = corners + CORNER_SIGNS[:, 1, None] * vectors[:, :, None, 1, :]
    corners = corners + CORNER_SIGNS[:, 2, None] * vectors[:, :, None, 2, :]
    mins, maxs = corners.min(2), corners.max(2)

    m = objectness.max(-1, keepdims=True)
    e = np.exp(objectness - m)                                                  # f32
    obj_prob = e[..., 1] / (e[..., 0] + e[..., 1])
    assert obj_prob.dtype == np.float32
    pred_cls = np.argmax(sem_scores, -1).astype(np.int64) if cls_in is None else cls_in.astype(np.int64)

    score = obj_prob.astype(np.float64)[..., None]
    if nms_mode == 2:
        z, o = np.zeros_like(score), np.ones_like(score)
        boxes = np.concatenate([mins[..., 0:1], z, mins[..., 2:3], maxs[..., 0:1], o, maxs[..., 2:3], score], -1)
    elif nms_mode == 1:
        boxes = np.concatenate([mins, maxs, score, pred_cls.astype(np.float64)[..., None]], -1)
    else:
        boxes = np.concatenate([mins, maxs, score], -1)

    size64 = size.astype(np.float64)
    size_margin = np.minimum(np.abs(size64 - np.float64(np.float32(0.01))), np.abs(size64 - 10.0)).min(-1)
    far_margin = np.full((N, K), np.inf)
    n_inside = first_inside = np.zeros((N, K), np.int64)
    if not remove_far_box:
        nonempty = np.ones((N, K), np.uint8)
    else:
        ok = ~((size < np.float32(0.01)).any(-1) | (size > np.float32(10)).any(-1))
        hf = (halff + np.float32(contact_dist)).astype(np.float64)              # both operations in f32
        assert (halff + np.float32(contact_dist)).dtype == np.float32
        Bj = joints.shape[0]
        hips = joints[np.arange(N) % Bj][:, :, origin_joint, 0:3].astype(np.float64)           # (N,T,3)
        r = hips[:, None, :, :] - ctr[:, :, None, :]                            # (N,K,T,3)
        cc, ss = c[..., None], s[..., None]
        l0 = r[..., 0] * cc + r[..., 2] * (-ss)
        l1 = r[..., 1]
        l2 = r[..., 0] * ss + r[..., 2] * cc
        out = np.stack([np.abs(l0) - hf[:, :, None, 0], np.abs(l1) - hf[:, :, None, 1], np.abs(l2) - hf[:, :, None, 2]], -1)
        inside = (np.abs(l0) <= hf[:, :, None, 0]) & (np.abs(l1) <= hf[:, :, None, 1]) & (np.abs(l2) <= hf[:, :, None, 2])
        nonempty = (ok & inside.any(-1)).astype(np.uint8)
        far_margin = np.where(ok, np.abs(out.max(-1).min(-1)), np.inf)
        n_inside, first_inside = inside.sum(-1), inside.argmax(-1)
    return Restated(corners, boxes, obj_prob, pred_cls, nonempty, far_margin, size_margin, n_inside, first_inside)


def restate_case(case):
    return restate(*case[1:])


def nms_margins(boxes, nonempty, thr, same_cls=False):
    """boxes (N,K,7|8) rows of p2r_nms3d, nonempty (N,K) -> (min |score_i - score_j|, min |IoU_ij - thr|) over the pairs of
    boxes that reach the NMS (same class only with same_cls): the decisions a keep mask is made of."""
    gap, over = np.inf, np.inf
    for b, ne in zip(boxes, nonempty):
        b = b[ne != 0]
        if len(b) < 2:
            continue
        iu = np.triu_indices(len(b), 1)
        lo = np.maximum(b[:, None, 0:3], b[None, :, 0:3])
        hi = np.minimum(b[:, None, 3:6], b[None, :, 3:6])
        inter = np.prod(np.maximum(0.0, hi - lo), -1)
        vol = np.prod(b[:, 3:6] - b[:, 0:3], -1)
        iou = inter / (vol[:, None] + vol[None, :] - inter)
        pair = np.ones_like(iou, bool) if not same_cls else b[:, None, 7] == b[None, :, 7]
        sel = pair[iu]
        if sel.any():
            gap = min(gap, np.abs(b[:, None, 6] - b[None, :, 6])[iu][sel].min())
            over = min(over, np.abs(iou - thr)[iu][sel].min())
    return gap, over


# ---- the generator --------------------------------------------------------------------------------------------------------
_AXIS_HEADINGS = [(0.0, 1.0), (1.0, 0.0), (-1.0, 0.0), (0.0, -1.0), (-0.0, -1.0)]          # 0, pi/2, -pi/2, pi, -pi
# sizes just inside and just outside the bounds of the far-box filter (the bounds are f32: 0.01f and 10f)
_EDGE_SIZES = [0.0103, 0.0097, 9.9996, 10.0004]


def _track(rng, T, J, origin_joint, far):
    """joints (T,J,3) f32: the origin joint walks through the room (or `far` away from it); the other joints hold
    positions that would put a hip inside every box, so a kernel that reads the wrong joint is seen"""
    t = np.linspace(0.0, 1.0, T) if T > 1 else np.zeros(1)
    walk = np.stack([3.0 * np.cos(2.3 * np.pi * t + rng.uniform(0, 6)), 0.9 + 0.05 * np.sin(9 * t),
                     2.5 * np.sin(1.7 * np.pi * t + rng.uniform(0, 6))], -1) + rng.normal(0, 0.02, (T, 3))
    joints = rng.uniform(-2.0, 2.0, (T, J, 3))
    joints[:, origin_joint] = walk + (np.array([150.0, 40.0, -120.0]) if far else 0.0)
    return joints.astype(np.float32)


def make_case(name, N, K, T, joints_repeat=1, nms_mode=0, lone=None, J=7, origin_joint=2, C=6, with_cls=False,
              contact_dist=1.0, remove_far_box=True, seed=0, spaced_scores=False, edges=True):
    """lone: None = the hip track walks among the boxes; 'none' = it stays far from all of them; an int f = it stays far
    except for frame f, which visits a spot that the first boxes of every sample (a third of them) are built around.
    spaced_scores: objectness probabilities at least 4e-3 apart within a sample (for tests that go on to the NMS).
    edges: boxes 1..4 get a size component just inside / outside a bound (K >= 5)."""
    rng = np.random.default_rng(seed)
    assert N % joints_repeat == 0
    Bj = N // joints_repeat
    far = lone is not None
    joints = np.stack([_track(rng, T, J, origin_joint, far) for _ in range(Bj)])
    spot = np.array([0.5, 1.0, -0.25])
    if isinstance(lone, (int, np.integer)):
        assert 0 <= lone < T
        joints[:, lone, origin_joint] = (spot + rng.normal(0, 0.05, (Bj, 3))).astype(np.float32)
    n_spot = (K + 2) // 3 if isinstance(lone, (int, np.integer)) else 0

    def draw(n):
        centre = np.stack([rng.uniform(-6, 6, n), rng.uniform(-0.5, 2.5, n), rng.uniform(-6, 6, n)], -1)
        size_log = rng.normal(-0.2, 0.6, (n, 3))
        hd = rng.normal(0, 1, (n, 2))
        return centre, size_log, hd

    center = np.zeros((N, K, 3), np.float32)
    size_log = np.zeros((N, K, 3), np.float32)
    heading = np.zeros((N, K, 2), np.float64)
    redraw = np.ones((N, K), bool)
    for _ in range(64):
        n = int(redraw.sum())
        centre, sl, hd = draw(n)
        ii, kk = np.nonzero(redraw)
        near = kk < n_spot                                      # boxes built around the visited spot
        centre[near] = spot + rng.uniform(-0.6, 0.6, (int(near.sum()), 3))
        axis = (kk % 7 == 3)                                    # every seventh box has a heading on an axis
        hd[axis] = np.array(_AXIS_HEADINGS)[(kk[axis] // 7 + ii[axis]) % len(_AXIS_HEADINGS)]
        if edges and K >= 5:
            for e, v in enumerate(_EDGE_SIZES):
                sel = kk == 1 + e
                sl[sel, (e + ii[sel]) % 3] = np.log(v)
        center[redraw], size_log[redraw], heading[redraw] = centre, sl, hd
        r = restate(center, size_log, heading, np.zeros((N, K, 2), np.float32), np.zeros((N, K, 1), np.float32),
                    None, joints, origin_joint, contact_dist, True, 0)
        redraw = (r.far_margin < GEN_MARGIN) | (r.size_margin < GEN_MARGIN)
        if not redraw.any():
            break
    else:
        raise AssertionError(f"{name}: no draw with all margins >= {GEN_MARGIN}")

    if spaced_scores:
        steps = np.stack([rng.permutation(K) for _ in range(N)])
        p1 = 0.06 + 0.88 * (steps + rng.uniform(0.1, 0.9, (N, K))) / K           # distinct by >= 0.88 * 0.2 / K
        logit = np.log(p1 / (1 - p1))
        objectness = np.stack([rng.normal(0, 1, (N, K)), np.zeros((N, K))], -1)
        objectness[..., 1] = objectness[..., 0] + logit
    else:
        objectness = rng.normal(0, 2, (N, K, 2))
    sem = rng.normal(0, 1, (N, K, C)).astype(np.float32)
    if K >= 3:
        sem[:, 2, :] = sem[:, 2, :1]                            # an all-equal row: the first maximum is class 0
    if C >= 3 and K >= 1:
        sem[:, 0, C - 1] = sem[:, 0, 1] = sem[:, 0].max(-1) + 1.0               # a tie between classes 1 and C-1: class 1
    cls_in = rng.integers(0, C, (N, K)).astype(np.int64) if with_cls else None
    return Case(name, center, size_log, heading, objectness.astype(np.float32), sem, cls_in, joints, origin_joint,
                contact_dist, remove_far_box, nms_mode)


def _lone_frame(kind, T):
    if kind == 'first':
        return 0
    if kind == 'last':
        return T - 1
    if kind == 'chunk2':                                        # the first frame of the second chunk, where there is one
        return CHUNK if T > CHUNK else T // 2
    return None if kind == 'walk' else 'none'


SWEEP_T = (1, 63, 64, 65, CHUNK, CHUNK + 1, 2 * CHUNK + 1)
SWEEP_K = (1, 5, 128, 130)
_N_REP = ((1, 1), (3, 1), (3, 3))
_LONE = ('walk', 'first', 'last', 'chunk2', 'none')


@functools.lru_cache(maxsize=None)
def sweep():
    """-> tuple of Case: every T with every K; N / joints_repeat, nms_mode, where the only inside hip is, class input,
    the joint count and the filter switch cycle through their values with coprime periods.  Then the chunk seams."""
    out, i = [], 0
    for T in SWEEP_T:
        for K in SWEEP_K:
            (N, rep), mode, kind = _N_REP[(i // 3) % 3], i % 3, _LONE[i % 5]
            J, origin = ((53, 0), (7, 2), (1, 0))[i % 3 if i % 2 else 1]
            out.append((f"T{T}-K{K}-N{N}x{rep}-m{mode}-{kind}",
                        dict(N=N, K=K, T=T, joints_repeat=rep, nms_mode=mode, lone=_lone_frame(kind, T), J=J,
                             origin_joint=origin, with_cls=i % 4 == 0, remove_far_box=i % 11 != 10, seed=1000 + i)))
            i += 1
    seams = [(CHUNK, CHUNK - 1), (CHUNK + 1, CHUNK), (CHUNK + 1, CHUNK - 1), (2 * CHUNK + 1, CHUNK),
             (2 * CHUNK + 1, 2 * CHUNK), (2 * CHUNK + 1, 2 * CHUNK - 1), (2 * CHUNK + 1, 0), (65, 64), (64, 63)]
    for j, (T, f) in enumerate(seams):
        K = (5, 130, 128)[j % 3]
        out.append((f"seam-T{T}-f{f}-K{K}", dict(N=3, K=K, T=T, joints_repeat=(1, 3)[j % 2], nms_mode=j % 3, lone=f,
                                               seed=2000 + j)))
    return tuple(make_case(name, **kw) for name, kw in out)


def nms_decisions_clear(case, thr=0.1, margin=GEN_MARGIN):
    """every sample keeps at least two boxes after the far-box filter, and in all three NMS modes every score-order and
    overlap decision among them is at least `margin` from flipping"""
    for mode in (0, 1, 2):
        r = restate_case(case._replace(nms_mode=mode))
        if r.nonempty.sum(1).min() < 2 or min(nms_margins(r.boxes, r.nonempty, thr, mode == 1)) < margin:
            return False
    return True


def searched(name, seed, **kw):
    """the first case from `seed` on whose NMS decisions are clear as well (deterministic: the seeds are tried in order)"""
    for s in range(seed, seed + 400):
        case = make_case(name, seed=s, **kw)
        if nms_decisions_clear(case):
            return case
    raise AssertionError(f"{name}: no seed in {seed}..{seed + 399} gives clear NMS decisions")


@functools.lru_cache(maxsize=None)
def nms_cases():
    """Cases that go on to the NMS (kernel against torch path, both return forms): small K, spaced scores, and boxes
    that overlap (those around a visited spot do).  nms_iou = 0.1 is the configured threshold."""
    out = []
    for i, (N, K, T, mode, lone) in enumerate([(2, 24, 40, 0, 3), (3, 17, CHUNK + 1, 1, CHUNK), (2, 33, 65, 2, 7)]):
        out.append(searched(f"nms-N{N}-K{K}-T{T}-m{mode}", 3000 + 400 * i, N=N, K=K, T=T, nms_mode=mode, lone=lone, J=53,
                            origin_joint=0, C=4, spaced_scores=True))
    return tuple(out)


def g14():
    """G14 (tests/golden/g14_parse_far.npz, written by tests/golden/make_parse_golden.py) -> (Case, the npz)."""
    z = np.load(os.path.join(GOLDEN, 'g14_parse_far.npz'))
    case = Case('g14', z['center'], z['size'], z['heading'], z['objectness_scores'], z['sem_cls_scores'], None,
                z['input_joints'], 0, float(z['contact_dist']), True, 0)
    return case, z


def g14_design():
    """The designed end points of G14: N = 3, K = 24, T = 40, rotated boxes, a hip track that enters some enlarged boxes
    and misses others, at least two near boxes per sample, every decision clear."""
    return searched('g14', 1400, N=3, K=24, T=40, J=4, origin_joint=0, C=22, spaced_scores=True)
