"""Designed cases, the margin rule and the comparison function for the interaction timeline (csrc/interaction.hip,
net_utils/interaction_device.py; shared by tests/test_interaction_cpu.py, tests/test_interaction_gpu.py and
tests/golden/make_interaction_golden.py).  The definition is `interaction_device.interaction_reference`.

Margin rule of every case (`assert_margin`, asserted when a case is built): for every (counted node, frame, joint, axis)
with finite values, | |local_a| - half_a | of the definition is either at least MARGIN = 1e-9 or exactly 0.  1e-9 is
about 1e6 times the rounding of the expression at the coordinates used here, so that any correct evaluation of the rule
-- the reference's hull test included -- decides every joint the same way.  Exactly 0 is allowed in the DYADIC cases
alone: boxes whose rotation has entries 0 and +-1, with centres, half sizes, threshold and joints that are multiples of
2^-10, so that every operation of the expression is exact and both sides agree on `<=`.

Pattern cases put the bits where they want them: node s is a unit cube far from every other node, joint s sits at its
centre in the frames of pattern s and ten units away in the others.

Comparison (`check_interaction`): equality of every array -- all results are integers.
"""
import collections
import functools
import os

import numpy as np

from pose2room_amd.net_utils import interaction_device as idv

MARGIN = 1e-9
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

Case = collections.namedtuple(
    'Case', 'name H joints count node_obbs node_rmat thresh merge_gap min_len M situation dyadic')


def inputs(c):
    return c.joints, c.count, c.node_obbs, c.node_rmat, c.thresh


def run_args(c):
    return c.merge_gap, c.min_len, c.M


@functools.lru_cache(maxsize=None)
def reference(name):
    """the definition's result for case `name`: computed once, shared, not modified"""
    c = by_name(name)
    return idv.interaction_reference(*inputs(c), *run_args(c))


def check_interaction(got, want):
    """got, want: idv.Interaction of host arrays (None where a tensor is absent)"""
    for f in idv.Interaction._fields:
        g, w = getattr(got, f), getattr(want, f)
        assert (g is None) == (w is None), f
        if w is None:
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, (f, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(g, w), (f, int((g != w).sum()), np.argwhere(g != w)[:4].tolist())


def head2rot(h):
    return np.array([[np.cos(h), 0.0, -np.sin(h)], [0.0, 1.0, 0.0], [np.sin(h), 0.0, np.cos(h)]], np.float64)


def margins(joints, count, node_obbs, node_rmat, thresh):
    """-> (the smallest non-zero | |local| - half |, the number of exact zeros) over every counted node, frame, joint, axis"""
    N, K = node_obbs.shape[:2]
    B = joints.shape[0]
    worst, zeros = np.inf, 0
    for n in range(N):
        p = joints[n % B, :, :, 0:3].astype(np.float64)
        for s in range(min(max(int(count[n]), 0), K)):
            c, size, R = node_obbs[n, s, 0:3], node_obbs[n, s, 3:6], node_rmat[n, s]
            with np.errstate(over='ignore', invalid='ignore'):
                d0, d1, d2 = p[..., 0] - c[0], p[..., 1] - c[1], p[..., 2] - c[2]
                for a in range(3):
                    local = ((0.0 + d0 * R[a, 0]) + d1 * R[a, 1]) + d2 * R[a, 2]
                    g = np.abs(np.abs(local) - (size[a] / 2.0 + thresh))
                    g = g[np.isfinite(g)]
                    zeros += int((g == 0.0).sum())
                    g = g[g != 0.0]
                    if g.size:
                        worst = min(worst, float(g.min()))
    return worst, zeros


def assert_margin(c):
    worst, zeros = margins(*inputs(c))
    assert worst >= MARGIN, (c.name, worst)
    assert zeros == 0 or c.dyadic, (c.name, zeros)
    return worst, zeros


def _case(name, H, joints, count, obbs, rmat, thresh, merge_gap=0, min_len=1, M=16, situation='', dyadic=False):
    c = Case(name, H, np.ascontiguousarray(joints, np.float32), np.asarray(count, np.int32), np.asarray(obbs, np.float64),
             np.asarray(rmat, np.float64), float(thresh), int(merge_gap), int(min_len), int(M), situation, dyadic)
    N, K = c.node_obbs.shape[:2]
    assert c.count.shape == (N,) and c.node_obbs.shape == (N, K, 7) and c.node_rmat.shape == (N, K, 3, 3) and N % H == 0
    assert c.joints.ndim == 4 and c.joints.shape[0] == N // H and c.joints.shape[3] in (3, 4)
    T = c.joints.shape[1]
    assert 0 <= c.merge_gap <= T and 1 <= c.min_len <= T and 1 <= c.M <= idv.MAX_M
    assert_margin(c)
    return c


# ---- building blocks -------------------------------------------------------------------------------------------------------
def walking_joints(rng, B, T, J, C, quantum=None):
    """a body that wanders through a 4 x 4 room: a smooth path of its centre, fixed joint offsets within half a metre and a
    jitter per frame and joint, so that contacts come, flicker and go; quantum: round to multiples of it (exact in f32)"""
    t = np.arange(T)[None, :, None] / max(T, 16)
    f, ph = rng.uniform(1.0, 6.0, (B, 1, 3)), rng.uniform(0, 2 * np.pi, (B, 1, 3))
    centre = np.array([1.6, 0.0, 1.6]) * np.sin(2 * np.pi * f * t + ph) + np.array([0.0, 0.9, 0.0])
    x = centre[:, :, None, :] + rng.uniform(-0.5, 0.5, (B, 1, J, 3)) + rng.normal(0, 0.05, (B, T, J, 3))
    if quantum:
        x = np.round(x / quantum) * quantum
    out = np.zeros((B, T, J, C), np.float32)
    out[..., 0:3] = x
    if C == 4:
        out[..., 3] = rng.uniform(0, 1, (B, T, J))
    return out


def random_nodes(rng, N, K, kept):
    """N samples of K slots, `kept` (an int or a list per sample) of them counted: rotated boxes in the room of
    `walking_joints`; unused slots zero"""
    kept = [kept] * N if np.isscalar(kept) else list(kept)
    obbs, rmat = np.zeros((N, K, 7)), np.zeros((N, K, 3, 3))
    for n in range(N):
        for s in range(min(max(kept[n], 0), K)):
            h = rng.uniform(-np.pi, np.pi)
            obbs[n, s] = np.concatenate([rng.uniform([-1.8, 0.2, -1.8], [1.8, 1.4, 1.8]), rng.uniform(0.3, 1.5, 3), [h]])
            rmat[n, s] = head2rot(h)
    return np.array(kept, np.int32), obbs, rmat


def _random_case(name, seed, H, B, K, kept, T, J, C, thresh=0.1, merge_gap=0, min_len=1, M=16, situation=''):
    rng = np.random.default_rng(seed)
    joints = walking_joints(rng, B, T, J, C)
    return _case(name, H, joints, *random_nodes(rng, H * B, K, kept), thresh, merge_gap, min_len, M, situation)


def spans(T, *runs):
    row = np.zeros(T, bool)
    for a, b in runs:
        assert 0 <= a < b <= T
        row[a:b] = True
    return row


def pattern_case(name, patterns, merge_gap, min_len, M, C=3, extra_slots=0, situation='patterns'):
    """one sample; node s is in contact exactly in the frames of patterns[s] (bool (T,)); extra_slots uncounted slots"""
    S, T = len(patterns), len(patterns[0])
    K, J = S + extra_slots, S
    obbs, rmat = np.zeros((1, K, 7)), np.zeros((1, K, 3, 3))
    joints = np.zeros((1, T, J, C), np.float32)
    for s, row in enumerate(patterns):
        obbs[0, s] = [100.0 * s, 1.0, -3.0, 1.0, 1.0, 1.0, 0.3 * s]
        rmat[0, s] = head2rot(0.3 * s)
        joints[0, :, s, 0:3] = [100.0 * s, 1.0, -3.0]
        joints[0, ~np.asarray(row), s, 0] += 10.0
    return _case(name, 1, joints, [S], obbs, rmat, 0.25, merge_gap, min_len, M, situation)


MERGE_GAP, MIN_LEN, PATTERN_M = 3, 4, 3
PATTERNS_130 = collections.OrderedDict([
    ('ends at bit 63', [(60, 64)]),
    ('starts at bit 0 of the next word', [(64, 70)]),
    ('over three words', [(30, 129)]),
    ('ends at T-1', [(120, 130)]),
    ('all frames', [(0, 130)]),
    ('none', []),
    ('gap of merge_gap across a word boundary', [(55, 62), (65, 70)]),
    ('gap of merge_gap + 1 across a word boundary', [(55, 62), (66, 70)]),
    ('runs of min_len and min_len - 1', [(10, 14), (20, 23)]),
    ('more than M intervals', [(0, 4), (10, 14), (20, 24), (30, 34), (40, 44), (126, 130)]),
    ('merged, then long enough', [(10, 12), (15, 17)]),
    ('single frames at the word edges', [(0, 1), (63, 64), (64, 65), (127, 128), (128, 129)]),
])


def patterns_case():
    return pattern_case('patterns-130', [spans(130, *r) for r in PATTERNS_130.values()], MERGE_GAP, MIN_LEN, PATTERN_M,
                        C=4, extra_slots=1)


def long_patterns_case():
    """T = 4097: 65 words, two chunks of 64.  Runs and gaps across the chunk boundary (frame 4096 is word 64)"""
    T = 4097
    rows = [spans(T, (4000, 4097)),                           # over the chunk boundary, ends at T-1
            spans(T, (5, 9), (4090, 4094), (4096, 4097)),     # a gap of 2 over the chunk boundary: merged; first run kept
            spans(T, (0, 4096)),                              # all of the first chunk, not the last frame
            spans(T, (4096, 4097)),                           # the last frame alone: shorter than min_len
            spans(T, (100, 2000), (2003, 4000)),              # a gap of 3 = merge_gap + 1 far from its ends' words
            spans(T, *[(70 * i, 70 * i + 6) for i in range(58)])]     # 58 runs over every word
    return pattern_case('patterns-4097', rows, 2, 3, 64, situation='patterns')


def dyadic_case():
    """joints exactly on enlarged faces (in), one float32 step outside (out), NaN and infinite coordinates, and two equal
    boxes for the tie of the labels.  R is the identity or a quarter turn; all values are multiples of 2^-10."""
    T, J = 6, 5
    obbs, rmat = np.zeros((2, 4, 7)), np.zeros((2, 4, 3, 3))
    quarter = np.array([[0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])
    obbs[0, 0], rmat[0, 0] = [1.0, 0.5, -2.0, 1.0, 0.5, 2.0, 0.0], np.eye(3)           # half + thresh: 0.75, 0.5, 1.25
    obbs[0, 1], rmat[0, 1] = obbs[0, 0], np.eye(3)                                      # the same box again: the tie
    obbs[0, 2], rmat[0, 2] = [1.0, 0.5, -2.0, 2.0, 0.5, 1.0, np.pi / 2], quarter        # the same box, a quarter turn
    obbs[0, 3], rmat[0, 3] = [1.0, 0.5, -2.0, 4.0, 4.0, 4.0, 0.0], np.eye(3)            # a larger box in the last slot
    obbs[1, 0], rmat[1, 0] = obbs[0, 0], np.eye(3)
    far = [50.0, 50.0, 50.0]
    joints = np.zeros((2, T, J, 3), np.float32)
    joints[:] = far
    step = np.nextafter(np.float32(1.75), np.float32(2.0))
    joints[0, 0, 0] = [1.75, 0.5, -2.0]                       # on the +x face of boxes 0, 1, 2: in
    joints[0, 1, 0] = [step, 0.5, -2.0]                       # one float32 step beyond: out of 0, 1, 2; in 3
    joints[0, 2, 0] = [1.0, 1.0, -3.25]                       # on an edge: +y and -z faces at once
    joints[0, 2, 1] = [0.25, 0.0, -0.75]                      # on a corner
    joints[0, 3, 0] = [np.nan, 0.5, -2.0]                     # a NaN coordinate: inside nothing
    joints[0, 3, 1] = [1.0, 0.5, -2.0]                        # ... the frame is in contact through the next joint
    joints[0, 3, 2] = [1.0, np.inf, -2.0]
    joints[0, 4, 0] = [1.0, 0.5, np.nan]                      # a frame whose only near joint has a NaN: no contact
    joints[0, 5, :3] = [1.0, 0.5, -2.0]                       # three joints in every box: a tie of 3 : 3 : 3 : 3
    joints[1, 0, 4] = [0.25, 0.5, -2.0]                       # sample 1: on the -x face
    joints[1, 5, 4] = [1.0, 0.5, float(np.nextafter(np.float32(-3.25), np.float32(-4.0)))]
    return _case('dyadic', 1, joints, [4, 1], obbs, rmat, 0.25, 0, 1, 4, 'dyadic', dyadic=True)


def ties_case():
    """slots 0 and 1 hold the same box, slot 2 a box around them: equal joint counts wherever 0 is in contact"""
    rng = np.random.default_rng(31)
    joints = walking_joints(rng, 1, 70, 9, 3)
    count, obbs, rmat = random_nodes(rng, 1, 3, 3)
    obbs[0, 0, 3:6] = [2.5, 1.8, 2.5]
    obbs[0, 1], rmat[0, 1] = obbs[0, 0], rmat[0, 0]
    obbs[0, 2, 0:3], obbs[0, 2, 3:6] = obbs[0, 0, 0:3], [0.8, 0.8, 0.8]
    return _case('ties', 1, joints, count, obbs, rmat, 0.1, 1, 2, 8, 'ties')


def bad_count_case():
    """H = 2, B = 1: a negative count and one above K"""
    rng = np.random.default_rng(41)
    joints = walking_joints(rng, 1, 65, 7, 4)
    _, obbs, rmat = random_nodes(rng, 2, 3, 3)
    return _case('bad-count', 2, joints, [-2, 6], obbs, rmat, 0.2, 1, 2, 4, 'bad count')


def saturate_case():
    """260 nodes that all hold the one joint: n_active saturates at 255"""
    K, T = 260, 3
    obbs, rmat = np.zeros((1, K, 7)), np.zeros((1, K, 3, 3))
    obbs[0, :] = [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0]
    rmat[0, :] = np.eye(3)
    joints = np.zeros((1, T, 1, 3), np.float32)
    joints[0, 1] = 9.0
    return _case('saturate-K260', 1, joints, [K], obbs, rmat, 0.125, 0, 1, 2, 'saturate')


def copies(c, H):
    """H hypotheses that all hold the scenes of case c (H = 1)"""
    assert c.H == 1
    rep = lambda a: np.concatenate([a] * H, 0)                                  # noqa: E731
    return c._replace(name=f'{c.name}-x{H}', H=H, count=rep(c.count), node_obbs=rep(c.node_obbs),
                      node_rmat=rep(c.node_rmat))


@functools.lru_cache(maxsize=None)
def sweep():
    cases = [
        _random_case('T-1', 101, 1, 1, 1, 1, 1, 1, 3, thresh=1.0, situation='T'),
        _random_case('T-63', 163, 1, 1, 4, 4, 63, 53, 4, merge_gap=1, min_len=2, situation='T'),
        _random_case('T-64', 164, 1, 2, 5, [5, 1], 64, 64, 3, merge_gap=2, min_len=1, M=2, situation='T'),
        _random_case('T-65', 165, 1, 2, 5, [0, 5], 65, 64, 4, merge_gap=0, min_len=3, situation='T'),
        _random_case('T-130-2x2', 230, 2, 2, 5, [5, 1, 0, 3], 130, 53, 3, merge_gap=2, min_len=3, M=5, situation='T'),
        _random_case('T-4097-3x1', 4097, 3, 1, 4, [4, 1, 2], 4097, 3, 3, thresh=0.05, merge_gap=3, min_len=5, M=64,
                     situation='T'),
        _random_case('K-0', 5, 1, 2, 0, 0, 10, 3, 3, situation='K = 0'),
        _random_case('none-kept', 6, 1, 2, 4, 0, 70, 5, 3, situation='count = 0'),
        patterns_case(), long_patterns_case(), dyadic_case(), ties_case(), bad_count_case(), saturate_case(),
    ]
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


def by_name(name):
    for c in sweep():
        if c.name == name:
            return c
    raise KeyError(name)


def g20():
    with np.load(os.path.join(GOLDEN, 'g20_interaction.npz')) as z:
        return {k: z[k] for k in z.files}


G20_THRESH = 0.1


def g20_design(seed=20):
    """one scene: T = 130 frames of 53 joints on a 2^-10 lattice (float32), six rotated boxes
    -> (joints (1,130,53,3) f32, count, node_obbs (1,6,7), node_rmat (1,6,3,3))"""
    rng = np.random.default_rng(seed)
    joints = walking_joints(rng, 1, 130, 53, 3, quantum=2.0 ** -10)
    count, obbs, rmat = random_nodes(rng, 1, 6, 6)
    return joints, count, obbs, rmat
