"""CPU: the contract of the recording repair (csrc/recording_repair.hip, net_utils/recording_repair.py) before any
kernel is involved: the NumPy mirror against np.interp's own outputs (G19), its internal consistency over the sweep of
tests/recording_repair_cases.py against a frame-by-frame walk written independently, the smoothing against np.convolve,
the spec's validation, and the ABI of include/p2r_recording_repair.h / libp2r_recording_repair.so with the argument
checks of its three entry points, which return on the host before any launch."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from pose2room_amd import _lib
from pose2room_amd.net_utils import recording_repair as rr
from pose2room_amd.net_utils import sample_build as sb
from pose2room_amd.net_utils import vote_labels as vl
from tests import recording_repair_cases as rc

EINVAL = -22
SWEEP = rc.sweep()
EVERYTHING = rr.RepairSpec(rr.MAX_GAP, True, 0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _split(packed, joints):
    """a packed result -> one array per recording"""
    return np.split(packed, np.cumsum([len(x) for x in joints])[:-1])


# ---- 1. the mirror against np.interp -------------------------------------------------------------------------------------
def test_mirror_equals_np_interp_on_g19():
    z = rc.g19()
    n = partly = 0
    for r in range(int(z['n_recordings'])):
        x, want = z[f'r{r}_joints'], z[f'r{r}_filled']
        out, how, stats, bits = rr.repair_reference([x], EVERYTHING)
        valid = np.isfinite(x).all(-1)
        assert np.array_equal(_bits(out), _bits(want))                      # every item, filled or measured
        assert np.array_equal(how == 0, valid) and set(np.unique(how)) == {0, 1, 2} and stats[0, 2] == 0
        assert np.array_equal(_bits(out[valid]), _bits(x[valid]))
        # an invalid item has all three coordinates replaced, the finite ones too
        partly += int((~valid & np.isfinite(x).any(-1)).sum())
        assert np.isfinite(out).all()
        n += int((~valid).sum())
    assert n == 163 and partly > 0 and os.path.getsize(rc.PATH) < 32768


def test_sweep_covers_what_it_claims():
    assert len(SWEEP) == 36 and len({c.name for c in SWEEP}) == 36
    assert {len(x) for c in SWEEP for x in c.joints} == set(rc.FRAMES)
    assert {c.joints[0].shape[1] for c in SWEEP} == set(rc.JOINTS) and {c.spec.max_gap for c in SWEEP} == set(rc.GAPS)
    assert {(len(c.joints), c.spec.hold_ends) for c in SWEEP} == {(1, False), (1, True), (3, False), (3, True)}
    assert all(len({len(x) for x in c.joints}) == 3 for c in SWEEP if len(c.joints) == 3)       # unequal lengths
    seen, exact, longer, dead, inf, one = set(), 0, 0, 0, 0, 0
    for c in SWEEP:
        out, how, stats, bits = rc.reference(c.name)
        seen |= set(np.unique(how).tolist())
        exact += int((stats[:, 3] == c.spec.max_gap).any() and c.spec.max_gap > 0)
        longer += int((stats[:, 3] == c.spec.max_gap + 1).any())
        for x in c.joints:
            assert np.abs(x[np.isfinite(x)]).max() <= 1e3
            dead += int(not np.isfinite(x).all(-1).any())
            inf += int(np.isinf(x).any())
            one += int((np.isnan(x).any(-1) & np.isfinite(x).any(-1)).any())
    assert seen == {0, 1, 2, 3} and min(exact, longer, dead, inf, one) >= 2


# ---- 2. the mirror against a walk over the frames ----------------------------------------------------------------------------
def _walk(valid, max_gap, hold_ends):
    """how and the four statistics of one recording by walking every joint's frames once: the runs of invalid frames"""
    F, J = valid.shape
    how, longest = np.zeros((F, J), np.uint8), 0
    for j in range(J):
        f = 0
        while f < F:
            if valid[f, j]:
                f += 1
                continue
            e = f
            while e < F and not valid[e, j]:
                e += 1
            g, at_end = e - f, f == 0 or e == F
            if g == F or g > max_gap or (at_end and not hold_ends):
                how[f:e, j] = 3
            else:
                how[f:e, j] = 2 if at_end else 1
            longest = max(longest, min(g, max_gap + 1))
            f = e
    return how, [int((how > 0).sum()), int(((how == 1) | (how == 2)).sum()), int((how == 3).sum()), longest]


@pytest.mark.parametrize("i", range(len(SWEEP)), ids=[c.name for c in SWEEP])
def test_mirror_is_consistent(i):
    c = SWEEP[i]
    out, how, stats, bits = rc.reference(c.name)
    word_offset, n_words = rr.word_offsets([len(x) for x in c.joints])
    assert bits.shape == (n_words, c.joints[0].shape[1]) and bits.dtype == np.uint64
    for r, (x, o, h) in enumerate(zip(c.joints, _split(out, c.joints), _split(how, c.joints))):
        valid = np.isfinite(x).all(-1)
        F = len(x)
        own = bits[word_offset[r]:word_offset[r] + (F + 63) // 64]
        assert np.array_equal(rr.unpack_bits(own, F), valid) and np.array_equal(rr.pack_bits(valid), own)
        if F % 64:
            assert not (own[-1] >> np.uint64(F % 64)).any()                # bits past the last frame
        want_how, want_stats = _walk(valid, c.spec.max_gap, c.spec.hold_ends)
        assert np.array_equal(h, want_how) and stats[r].tolist() == want_stats
        assert np.array_equal(_bits(o[valid]), _bits(x[valid]))             # measured items are untouched
        assert np.array_equal(_bits(o[h == 3]), np.full((int((h == 3).sum()), 3), 0x7ff8000000000000, np.uint64))
        assert np.isfinite(o[h != 3]).all()
    # repairing what is fully repaired changes nothing
    done = [o for r, o in enumerate(_split(out, c.joints)) if stats[r, 2] == 0]
    if done:
        again, how2, stats2, _ = rr.repair_reference(done, c.spec)
        assert np.array_equal(_bits(again), _bits(np.concatenate(done))) and not how2.any() and not stats2.any()


def test_integer_linear_track_is_reproduced_exactly():
    F = 200
    f = np.arange(F, dtype=np.float64)
    x = np.stack([np.stack([3 * f - 7, -5 * f + 1000, 0 * f + 12], -1), np.stack([f, 2 * f, -f], -1)], 1)
    holes = x.copy()
    for lo, hi in ((1, 2), (10, 75), (100, 199)):
        holes[lo:hi, 0] = np.nan
        holes[lo + 3:hi - 1, 1, 2] = np.inf
    out, how, stats, _ = rr.repair_reference([holes], rr.RepairSpec(100, False, 0))
    assert np.array_equal(out, x) and stats.tolist() == [[1 + 65 + 99 + 61 + 95, 321, 0, 99]]
    assert set(np.unique(how)) == {0, 1}


def test_held_ends_and_long_gaps():
    x = np.arange(30, dtype=np.float64).reshape(10, 1, 3)
    x[[0, 1, 4, 5, 6, 9], 0, 1] = np.nan
    out, how, stats, _ = rr.repair_reference([x], rr.RepairSpec(2, True, 0))
    assert how[:, 0].tolist() == [2, 2, 0, 0, 3, 3, 3, 0, 0, 2] and stats.tolist() == [[6, 3, 3, 3]]
    assert np.array_equal(out[[0, 1, 9]], x[[2, 2, 8]]) and np.isnan(out[4:7]).all()
    out, how, stats, _ = rr.repair_reference([x], rr.RepairSpec(3, False, 0))
    assert how[:, 0].tolist() == [3, 3, 0, 0, 1, 1, 1, 0, 0, 3] and stats.tolist() == [[6, 3, 3, 3]]
    assert np.array_equal(out[4:7, 0], (x[3, 0] + (x[7, 0] - x[3, 0]) / 4 * np.arange(1, 4)[:, None]))
    out, how, stats, _ = rr.repair_reference([x], rr.RepairSpec(0, True, 0))
    assert how[:, 0].tolist() == [3, 3, 0, 0, 3, 3, 3, 0, 0, 3] and stats.tolist() == [[6, 0, 6, 1]]


# ---- 3. the smoothing -------------------------------------------------------------------------------------------------------
def test_binomial_weights_are_exact():
    from math import comb
    for h in range(1, rr.MAX_HALF + 1):
        w = rr.binomial_weights(h)
        assert w.tolist() == [comb(2 * h, k) / 4 ** h for k in range(2 * h + 1)] and w.sum() == 1.0
        assert all(float(v * 4 ** h).is_integer() for v in w)


@pytest.mark.parametrize("h", [1, 3, 8])
def test_constant_track_stays_constant(h):
    """ends included.  The constants are float32 values: 24 bits times the 14 bits of a weight's numerator is exact in
    float64, so acc is the constant times ws without a rounding, whatever the window."""
    rng = np.random.default_rng(h)
    const = rng.uniform(-1e3, 1e3, (1, 5, 3)).astype(np.float32).astype(np.float64)
    for F in (1, 2, h, h + 1, 2 * h + 1, 40):
        x = np.repeat(const, F, 0)
        assert np.array_equal(rr.smooth_reference(x, h), x), F


@pytest.mark.parametrize("h", [1, 2, 5, 8])
def test_interior_equals_np_convolve(h):
    """|mirror - np.convolve| <= 2h eps sum |w_k x_k|: the standard bound of a sum of 2h + 1 terms (2h additions),
    each side within half of it"""
    rng = np.random.default_rng(40 + h)
    F, w = 150, rr.binomial_weights(h)
    x = rng.uniform(-1e3, 1e3, (F, 4, 3))
    got = rr.smooth_reference(x, h)
    eps = np.finfo(np.float64).eps
    for j in range(4):
        for c in range(3):
            want = np.convolve(x[:, j, c], w, mode='valid')                # frames h .. F - h - 1
            bound = 2 * h * eps * np.convolve(np.abs(x[:, j, c]), w, mode='valid')
            assert (np.abs(got[h:F - h, j, c] - want) <= bound).all()
    assert not np.array_equal(got, x)
    # the ends: the window truncated and renormalised
    w0 = w[h:] / w[h:].sum()
    assert np.allclose(got[0], np.tensordot(w0, x[:h + 1], 1), rtol=1e-13, atol=0)
    # non-finite values are ordinary data
    x[70, 2, 1] = np.nan
    bad = np.isnan(rr.smooth_reference(x, h))
    assert bad[70 - h:71 + h, 2, 1].all() and bad.sum() == 2 * h + 1


def test_repair_reference_smooths_after_the_fill():
    c = rc.by_name(SWEEP[21].name)
    spec = c.spec._replace(smooth=2)
    out, how, stats, bits = rr.repair_reference(c.joints, spec)
    plain = rc.reference(c.name)
    assert np.array_equal(how, plain[1]) and np.array_equal(stats, plain[2]) and np.array_equal(bits, plain[3])
    want = np.concatenate([rr.smooth_reference(o, 2) for o in _split(plain[0], c.joints)])
    assert np.array_equal(_bits(want), _bits(out))


# ---- 4. the spec ----------------------------------------------------------------------------------------------------------
def test_spec_validation():
    assert rr.RepairSpec() == (30, True, 0) and rr.RepairSpec(0, 0, 8) == (0, False, 8)
    assert rr.RepairSpec(np.int64(4096), np.bool_(True), np.int32(1)) == (4096, True, 1)
    for kw, name in ((dict(max_gap=-1), 'max_gap'), (dict(max_gap=4097), 'max_gap'), (dict(max_gap=2.0), 'max_gap'),
                     (dict(max_gap=True), 'max_gap'), (dict(smooth=9), 'smooth'), (dict(smooth=-1), 'smooth'),
                     (dict(smooth=None), 'smooth'), (dict(hold_ends=2), 'hold_ends'), (dict(hold_ends='yes'), 'hold_ends')):
        with pytest.raises(ValueError, match=name):
            rr.RepairSpec(**kw)
    with pytest.raises(TypeError, match="RepairSpec"):
        rr.repair_reference([np.zeros((2, 1, 3))], (30, True, 0))
    with pytest.raises(ValueError, match="float64"):
        rr.repair_reference([np.zeros((2, 1, 3), np.float32)], rr.RepairSpec())
    rec = dict(name='r', joints=np.zeros((4, 53, 3)), room_bbox=None, object_nodes=[])
    with pytest.raises(ValueError, match="on_unrepairable"):
        sb.build_samples([rec], repair=rr.RepairSpec(), on_unrepairable='drop')
    with pytest.raises(TypeError, match="repair"):
        sb.build_samples([rec], repair=(30, True, 0))
    with pytest.raises(TypeError, match="Recordings"):
        rr.repair_packed(None, rr.RepairSpec())
    assert issubclass(rr.RepairedSamples, sb.BuiltSamples) and rr.RepairedSamples._fields == sb.BuiltSamples._fields
    built = rr.RepairedSamples(sb.BuiltSamples(*range(11)), 'stats')
    assert tuple(built) == tuple(range(11)) and len(built) == 11 and built.repair == 'stats' and built.kept == 7


# ---- 5. the ABI ----------------------------------------------------------------------------------------------------------
NAMES = ['p2r_gap_fill', 'p2r_joint_valid_bits', 'p2r_smooth_frames']


def test_header_binds_and_library_exports_exactly_it():
    protos = _lib.prototypes(rr.HEADER_PATH)
    assert sorted(protos) == _lib.declared_symbols(rr.HEADER_PATH) == NAMES
    assert protos['p2r_joint_valid_bits'].kinds == 'ppip' and protos['p2r_joint_valid_bits'].has_stream
    assert protos['p2r_gap_fill'].kinds == 'ppipiippp' and protos['p2r_gap_fill'].has_stream
    assert protos['p2r_smooth_frames'].kinds == 'pip' and protos['p2r_smooth_frames'].has_stream
    assert protos['p2r_gap_fill'].argtypes[2] is ctypes.c_longlong and protos['p2r_gap_fill'].argtypes[4] is ctypes.c_int
    assert os.path.basename(rr.LIB_PATH) == 'libp2r_recording_repair.so'
    out = subprocess.run(["nm", "-D", "--defined-only", rr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("p2r_")}
    assert exported == set(protos)
    for other in (None, vl.HEADER_PATH, sb.HEADER_PATH):
        assert not set(protos) & set(_lib.declared_symbols(*([other] if other else [])))
    with open(rr.HEADER_PATH) as f:
        text = f.read()
    assert '#include "p2r_sample_build.h"' in text and 'typedef' not in text       # p2r_recordings is reused
    assert f'#define P2R_RR_MAX_GAP {rr.MAX_GAP} ' in text and f'#define P2R_RR_MAX_HALF {rr.MAX_HALF} ' in text
    l = rr.lib()
    for name in NAMES:
        assert getattr(l, name).argtypes == protos[name].argtypes and getattr(l, name).restype is ctypes.c_int


def test_header_compiles_as_c(tmp_path):
    from tests.test_binding_cpu import _c_compiler
    src = tmp_path / "use.c"
    src.write_text('#include "p2r_recording_repair.h"\nint main(void) { p2r_recordings r; (void)r; '
                   'return P2R_RR_MAX_GAP == 4096 && P2R_RR_MAX_HALF == 8 ? 0 : 1; }\n')
    subprocess.run([_c_compiler(), "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(rr.HEADER_PATH), str(src), "-o",
                    str(tmp_path / "use")], check=True, capture_output=True, text=True)
    assert subprocess.run([str(tmp_path / "use")]).returncode == 0


# ---- 6. argument checks: on the host, before any launch ------------------------------------------------------------------
_BUF = ctypes.create_string_buffer(64)          # a non-NULL address; never read, every call below is refused first
_P = ctypes.addressof(_BUF)
_Q = _P + 8


def _rec(**over):
    return sb._Recordings(**{**dict(joints=_P, frame_offset=_P, n_frames=_P, n_frames_total=100, R=2, J=53,
                                    max_frames=60), **over})


BAD_RECS = [dict(joints=None), dict(frame_offset=None), dict(n_frames=None), dict(n_frames_total=0), dict(R=0),
            dict(J=0), dict(J=257), dict(max_frames=0), dict(max_frames=65536)]
GOOD = {
    'p2r_joint_valid_bits': dict(word_offset=_P, n_words_total=2, bits=_P),
    'p2r_gap_fill': dict(word_offset=_P, n_words_total=2, bits=_P, max_gap=30, hold_ends=1, out=_Q, how=_P, stats=_P),
    'p2r_smooth_frames': dict(half_width=2, out=_Q),
}
BAD = {
    'p2r_joint_valid_bits': [dict(word_offset=None), dict(bits=None), dict(n_words_total=0),
                             dict(n_words_total=2 ** 31)],
    'p2r_gap_fill': [dict(word_offset=None), dict(bits=None), dict(out=None), dict(how=None), dict(stats=None),
                     dict(out=_P), dict(n_words_total=0), dict(max_gap=-1), dict(max_gap=4097)],
    'p2r_smooth_frames': [dict(out=None), dict(out=_P), dict(half_width=0), dict(half_width=9), dict(half_width=-1)],
}


def test_entry_points_refuse_bad_arguments():
    l = rr.lib()
    n = 0
    for name in NAMES:
        fn = getattr(l, name)
        assert fn(None, *GOOD[name].values(), None) == EINVAL
        for over in BAD_RECS:
            rec = _rec(**over)
            assert fn(ctypes.byref(rec), *GOOD[name].values(), None) == EINVAL, (name, over)
        for over in BAD[name]:
            rec = _rec()
            assert fn(ctypes.byref(rec), *{**GOOD[name], **over}.values(), None) == EINVAL, (name, over)
            n += 1
    assert n == 18
