"""Seeded recordings with holes for the recording repair (net_utils/recording_repair.py, csrc/recording_repair.hip) and
G19 (tests/golden/g19_recording_repair.npz, made by tests/golden/make_recording_repair_golden.py with np.interp); shared
by tests/test_recording_repair_cpu.py and tests/test_recording_repair_gpu.py.  Built once, never changed.

Finite coordinates are drawn with |x| <= 1e3: p_b - p_a cannot overflow, the one place where the NaN bits of host and
device could differ.  The sweep crosses frame counts around the 64-frame word, R in {1, 3} with unequal lengths (so
recording boundaries fall inside the packed frame axis), J around the 16 joints a wave ballots and the 64 lanes, max_gap
around the word and hold_ends, thinned to 36 cases; every joint of every recording gets one of the PATTERNS, rotated so
that a case with one joint still meets each of them somewhere in the sweep."""
import collections
import functools
import os

import numpy as np

from pose2room_amd.net_utils import recording_repair as rr

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g19_recording_repair.npz')

FRAMES = (1, 2, 63, 64, 65, 127, 128, 129, 193)
JOINTS = (1, 3, 53, 64, 65)
GAPS = (0, 1, 5, 63, 64, 65, 130)

# joints: one (F, J, 3) f64 array per recording; spec: the RepairSpec (smooth = 0: the smoothing has tests of its own)
Case = collections.namedtuple("Case", "name joints spec")


def _gap(x, j, lo, hi):
    x[max(lo, 0):max(hi, 0), j] = np.nan


def _none(x, j, mg, rng):
    pass


def _single(x, j, mg, rng):
    x[rng.integers(x.shape[0]), j] = np.nan


def _straddle(x, j, mg, rng):
    """a gap over a word boundary where there is one, else in the middle"""
    F = x.shape[0]
    edge = 64 * int(rng.integers(1, (F - 1) // 64 + 1)) if F > 64 else F // 2
    _gap(x, j, edge - 2, min(edge + 3, F))


def _exact(x, j, mg, rng):
    """a gap of exactly max_gap and one of max_gap + 1, as far as they fit between measured frames"""
    F = x.shape[0]
    _gap(x, j, 1, min(1 + mg, F - 1))
    _gap(x, j, 2 + mg, min(3 + 2 * mg, F - 1))


def _ends(x, j, mg, rng):
    """a leading gap of max_gap and a trailing gap of max_gap + 1, as far as they fit"""
    F = x.shape[0]
    lead = min(mg, (F - 1) // 2)
    _gap(x, j, 0, lead)
    _gap(x, j, max(F - (mg + 1), lead + 1), F)


def _never(x, j, mg, rng):
    x[:, j] = np.nan


def _inf(x, j, mg, rng):
    f = rng.integers(x.shape[0], size=3)
    x[f, j, rng.integers(3, size=3)] = [np.inf, -np.inf, np.inf]


def _one_coordinate(x, j, mg, rng):
    f = int(rng.integers(x.shape[0]))
    x[f:f + 2, j, rng.integers(3)] = np.nan


def _random(x, j, mg, rng):
    x[rng.random(x.shape[0]) < 0.3, j] = np.nan


def _long_ends(x, j, mg, rng):
    """ends longer than max_gap when the recording is long enough"""
    F = x.shape[0]
    _gap(x, j, 0, min(mg + 1, F - 1))
    _gap(x, j, max(F - (mg + 2), mg + 2), F)


PATTERNS = (_none, _single, _straddle, _exact, _ends, _never, _inf, _one_coordinate, _random, _long_ends)


def recording(F, J, rng, mg, shift=0, dead=False):
    """(F, J, 3) f64 with |x| <= 1e3; joint j gets PATTERNS[(j + shift) % 10]; dead: no valid frame at all"""
    x = rng.uniform(-1e3, 1e3, (F, J, 3))
    for j in range(J):
        PATTERNS[(j + shift) % len(PATTERNS)](x, j, mg, rng)
    if dead:
        x[:, :, int(rng.integers(3))] = np.nan
    return x


@functools.lru_cache(maxsize=None)
def sweep():
    cases = []
    for i, F in enumerate(FRAMES):
        for t in range(4):
            n = 4 * i + t
            J, mg, hold = JOINTS[(i + t) % 5], GAPS[(2 * i + 3 * t) % 7], (i + t) % 2
            lengths = (F,) if t % 2 == 0 else (FRAMES[(i + 3) % 9], F, FRAMES[(i + 5) % 9])
            rng = np.random.default_rng(1900 + n)
            joints = [recording(f, J, rng, mg, shift=n + 3 * k, dead=(len(lengths) == 3 and k == 2 and i % 3 == 0))
                      for k, f in enumerate(lengths)]
            cases.append(Case(f"F{'-'.join(map(str, lengths))}_J{J}_gap{mg}_hold{hold}", joints,
                              rr.RepairSpec(mg, bool(hold), 0)))
    return cases


def by_name(name):
    return {c.name: c for c in sweep()}[name]


@functools.lru_cache(maxsize=None)
def reference(name):
    """repair_reference of a sweep case, computed once"""
    c = by_name(name)
    return rr.repair_reference(c.joints, c.spec)


def contract_case(lengths, J, mg=5, seed=7):
    rng = np.random.default_rng(seed)
    return [recording(f, J, rng, mg, shift=k) for k, f in enumerate(lengths)]


def scene_recordings(holes, seed=0):
    """Recordings that `build_samples` keeps (tests/sample_build_cases.seeded_recording), punched: holes = per recording
    None, 'short' (gaps up to 4 frames, not on the origin joint's first frames) or 'long' (one gap of 12 frames too)"""
    from tests import sample_build_cases as sbc
    recs = []
    for i, kind in enumerate(holes):
        r = sbc.seeded_recording(70 + 9 * i, 3 + i, seed=seed + i, name=f'holes_{i}_{kind}')
        x, rng = r['joints'], np.random.default_rng(seed + 100 + i)
        if kind is not None:
            for j in range(0, 53, 4):
                f = int(rng.integers(1, x.shape[0] - 6))
                x[f:f + 1 + (j // 4) % 4, j, rng.integers(3)] = np.nan
            x[0:2, 7] = np.nan                                  # a leading gap
            x[-3:, 9] = np.inf                                  # a trailing gap
        if kind == 'long':
            x[20:32, 11] = np.nan
        recs.append(r)
    return recs


@functools.lru_cache(maxsize=None)
def g19():
    return dict(np.load(PATH))
