"""Raw recordings with missing joints, conditioned on the device (csrc/recording_repair.hip,
include/p2r_recording_repair.h).

The reference's poses come out of a simulator and are always finite; recordings from motion capture or a pose estimator
drop single joints for a few frames.  A (frame, joint) item is VALID iff its three coordinates are finite.  The stage
marks the items that are not, fills the short gaps of every joint by linear interpolation in time (the ends by holding
the nearest measurement), leaves the others as NaN -- so that `p2r_recording_scan` still flags the recording -- and
optionally low-passes every track with a binomial filter.  The arithmetic contract is the header's comment.

  * `RepairSpec`         max_gap, hold_ends, smooth
  * `repair_reference`   the NumPy mirror of the three entry points, in their operation order: the definition
  * `valid_bits`, `gap_fill`, `smooth_frames`   the entry points on a `Recordings`
  * `repair_packed`      a `Recordings` -> (repaired `Recordings`, how, stats), two or three library calls, no read-back
  * `repair_batch`       a batch (B, T, J, 3) of any float dtype, for the inference side
  * `build_samples(..., repair=spec)` and `DeviceSampleStore.from_recordings(..., repair=spec)` run it in front of the scan

how (frames, J) u8: 0 measured, 1 interpolated, 2 held from the nearest end, 3 left as NaN.  stats (R, 4) i32: invalid
items, filled items, items left, the longest run of invalid frames of any joint capped at max_gap + 1.
No CPU fallback: the mirror is what the tests compare against, not a second implementation behind the op.
"""
import collections
import ctypes

import numpy as np
import torch

from .. import _lib
from . import sample_build as sb

MAX_GAP, MAX_HALF = 4096, 8             # P2R_RR_MAX_GAP / P2R_RR_MAX_HALF of include/p2r_recording_repair.h
MEASURED, INTERPOLATED, HELD, LEFT = 0, 1, 2, 3
UNREPAIRABLE = sb.UNREPAIRABLE
QUIET_NAN = np.array([0x7ff8000000000000], np.uint64).view(np.float64)[0]

_library = _lib.extension("recording_repair")
HEADER_PATH, LIB_PATH = _library.header_path, _library.lib_path
lib, _launch = _library.lib, _library.launch


class RepairSpec(collections.namedtuple("RepairSpec", "max_gap hold_ends smooth")):
    """max_gap: the longest gap, in frames, that is filled (0 .. 4096; 0 fills nothing); hold_ends: fill a gap at the
    beginning or the end of a recording with the nearest measurement; smooth: the half width of the binomial low-pass
    run over the repaired tracks (0: none, up to 8)."""
    __slots__ = ()

    def __new__(cls, max_gap=30, hold_ends=True, smooth=0):
        for name, v, hi in (('max_gap', max_gap, MAX_GAP), ('smooth', smooth, MAX_HALF)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= hi:
                raise ValueError(f"RepairSpec: {name} must be an integer in 0..{hi}, got {v!r}")
        if not isinstance(hold_ends, (bool, np.bool_, int, np.integer)) or hold_ends not in (0, 1):
            raise ValueError(f"RepairSpec: hold_ends must be a bool, got {hold_ends!r}")
        return super().__new__(cls, int(max_gap), bool(hold_ends), int(smooth))


def _spec(spec, who):
    if not isinstance(spec, RepairSpec):
        raise TypeError(f"{who}: spec must be a RepairSpec, got {type(spec).__name__}")
    return spec


# ---- the contract in NumPy ------------------------------------------------------------------------------------------
def word_offsets(frames):
    """frame counts (R,) -> (word_offset (R,) i64, n_words_total): a word is 64 consecutive frames of one recording"""
    words = (np.asarray(frames, np.int64) + 63) // 64
    off = np.zeros(len(words), np.int64)
    off[1:] = np.cumsum(words)[:-1]
    return off, int(words.sum())


def pack_bits(valid):
    """valid (F, J) bool of one recording -> (ceil(F / 64), J) u64, bit i of word w = frame 64 * w + i"""
    F, J = valid.shape
    nw = (F + 63) // 64
    padded = np.zeros((nw * 64, J), np.uint64)
    padded[:F] = valid
    return (padded.reshape(nw, 64, J) << np.arange(64, dtype=np.uint64)[None, :, None]).sum(1, dtype=np.uint64)


def unpack_bits(bits, F):
    """pack_bits' inverse for a recording of F frames"""
    nw, J = bits.shape
    dense = (bits[:, None, :] >> np.arange(64, dtype=np.uint64)[None, :, None]) & np.uint64(1)
    return dense.reshape(nw * 64, J)[:F].astype(bool)


def binomial_weights(h):
    """w_k = C(2h, k + h) / 4^h for k = -h .. h, exact in float64"""
    w = np.ones(1)
    for _ in range(2 * h):
        w = np.convolve(w, [1.0, 1.0])
    return w / 4.0 ** h


def fill_reference(x, max_gap, hold_ends):
    """p2r_gap_fill for one recording x (F, J, 3) f64 -> (out, how (F, J) u8, stats (4,) i32, valid (F, J) bool)"""
    F, J = x.shape[:2]
    valid = np.isfinite(x).all(-1)
    out, how = x.copy(), np.zeros((F, J), np.uint8)
    n_invalid = n_filled = n_left = longest = 0
    for j in np.flatnonzero(~valid.all(0)):
        good, f = np.flatnonzero(valid[:, j]), np.flatnonzero(~valid[:, j])
        pos = np.searchsorted(good, f)                                      # the valid frames in front of f
        if good.size:
            a = np.where(pos > 0, good[np.maximum(pos - 1, 0)], -1)         # the nearest valid frame before f
            b = np.where(pos < good.size, good[np.minimum(pos, good.size - 1)], F)
        else:
            a, b = np.full(f.size, -1), np.full(f.size, F)
        run = b - a - 1                     # the gap's length in all of its places: a = -1 in front, b = F at the end
        short = run <= max_gap
        interior = short & (a >= 0) & (b < F)
        end = short & bool(hold_ends) & ((a >= 0) != (b < F))
        out[f, j], how[f, j] = QUIET_NAN, LEFT
        fi, ai, bi = f[interior], a[interior], b[interior]
        pa, pb = x[ai, j], x[bi, j]
        slope = (pb - pa) / (bi.astype(np.float64) - ai.astype(np.float64))[:, None]
        out[fi, j] = slope * (fi.astype(np.float64) - ai.astype(np.float64))[:, None] + pa
        how[fi, j] = INTERPOLATED
        fe = f[end]
        out[fe, j] = x[np.where(a[end] >= 0, a[end], b[end]), j]
        how[fe, j] = HELD
        n_invalid += f.size
        n_filled += int(interior.sum() + end.sum())
        n_left += int(f.size - interior.sum() - end.sum())
        longest = max(longest, int(np.minimum(run, max_gap + 1).max()))
    return out, how, np.array([n_invalid, n_filled, n_left, longest], np.int32), valid


def smooth_reference(x, h):
    """p2r_smooth_frames for one recording x (F, J, 3) f64"""
    F, w = x.shape[0], binomial_weights(h)
    acc, ws = np.zeros_like(x), np.zeros(F)
    with np.errstate(invalid='ignore', over='ignore'):
        for k in range(-h, h + 1):                          # ascending, over the frames f + k inside the recording
            lo, hi = max(0, -k), min(F, F - k)
            if lo < hi:
                acc[lo:hi] = acc[lo:hi] + w[k + h] * x[lo + k:hi + k]
                ws[lo:hi] = ws[lo:hi] + w[k + h]
        return acc / ws[:, None, None]


def repair_reference(joints_list, spec):
    """The NumPy mirror of p2r_joint_valid_bits, p2r_gap_fill and p2r_smooth_frames: one (F, J, 3) float64 array per
    recording -> (joints (F_total, J, 3) f64, how (F_total, J) u8, stats (R, 4) i32, bits (n_words_total, J) u64),
    packed as the kernels pack them."""
    spec = _spec(spec, "repair_reference")
    outs, hows, stats, bits = [], [], [], []
    for x in joints_list:
        x = np.asarray(x)
        if x.dtype != np.float64 or x.ndim != 3 or x.shape[2] != 3 or x.shape[0] < 1:
            raise ValueError(f"repair_reference: float64 joints (F, J, 3) expected, got {x.dtype} {x.shape}")
        out, how, st, valid = fill_reference(x, spec.max_gap, spec.hold_ends)
        outs.append(smooth_reference(out, spec.smooth) if spec.smooth else out)
        hows.append(how)
        stats.append(st)
        bits.append(pack_bits(valid))
    return np.concatenate(outs), np.concatenate(hows), np.stack(stats), np.concatenate(bits)


# ---- the device ops -------------------------------------------------------------------------------------------------
def _words(rec):
    """-> (word_offset (R,) i64 on the device, n_words_total) of a Recordings; made once per Recordings, uploaded from
    pinned memory without a synchronisation"""
    if getattr(rec, '_words', None) is None:
        off, total = word_offsets(rec.frames)
        rec._words = (torch.from_numpy(off).pin_memory().to(rec.device, non_blocking=True), total)
    return rec._words


def _recordings(rec, who):
    if not isinstance(rec, sb.Recordings):
        raise TypeError(f"{who}: rec must be a Recordings, got {type(rec).__name__}")
    return rec


def valid_bits(rec):
    """p2r_joint_valid_bits: a Recordings -> bits (n_words_total, J) i64 on the device (the u64 words; view them as
    uint64 on the host)"""
    rec = _recordings(rec, "valid_bits")
    word_offset, n_words = _words(rec)
    bits = torch.empty((n_words, rec.J), dtype=torch.int64, device=rec.device)
    _launch("p2r_joint_valid_bits", rec.device, ctypes.byref(rec.c), word_offset, n_words, bits)
    return bits


def gap_fill(rec, bits, max_gap, hold_ends):
    """p2r_gap_fill: a Recordings and its valid_bits -> (joints (F_total, J, 3) f64, how (F_total, J) u8, stats (R, 4)
    i32) on the device"""
    rec = _recordings(rec, "gap_fill")
    word_offset, n_words = _words(rec)
    if not (torch.is_tensor(bits) and bits.dtype == torch.int64 and tuple(bits.shape) == (n_words, rec.J)
            and bits.device == rec.device and bits.is_contiguous()):
        raise RuntimeError(f"gap_fill: bits must be a contiguous int64 ({n_words}, {rec.J}) tensor on {rec.device} "
                           "(no CPU fallback)")
    if isinstance(max_gap, bool) or not isinstance(max_gap, (int, np.integer)) or not 0 <= max_gap <= MAX_GAP:
        raise ValueError(f"gap_fill: max_gap must be an integer in 0..{MAX_GAP}, got {max_gap!r}")
    out = torch.empty_like(rec.joints)
    how = torch.empty(rec.joints.shape[:2], dtype=torch.uint8, device=rec.device)
    stats = torch.empty((rec.R, 4), dtype=torch.int32, device=rec.device)
    _launch("p2r_gap_fill", rec.device, ctypes.byref(rec.c), word_offset, n_words, bits, int(max_gap),
            int(bool(hold_ends)), out, how, stats)
    return out, how, stats


def smooth_frames(rec, half_width):
    """p2r_smooth_frames: a Recordings -> joints (F_total, J, 3) f64 on the device"""
    rec = _recordings(rec, "smooth_frames")
    if isinstance(half_width, bool) or not isinstance(half_width, (int, np.integer)) or not 1 <= half_width <= MAX_HALF:
        raise ValueError(f"smooth_frames: half_width must be an integer in 1..{MAX_HALF}, got {half_width!r}")
    out = torch.empty_like(rec.joints)
    _launch("p2r_smooth_frames", rec.device, ctypes.byref(rec.c), int(half_width), out)
    return out


def repair_packed(rec, spec):
    """A Recordings -> (the repaired Recordings, how (F_total, J) u8, stats (R, 4) i32), all on the device: two library
    calls, three with spec.smooth, and no read-back.  The result shares frame_offset and n_frames with `rec`."""
    rec, spec = _recordings(rec, "repair_packed"), _spec(spec, "repair_packed")
    out, how, stats = gap_fill(rec, valid_bits(rec), spec.max_gap, spec.hold_ends)
    fixed = sb.Recordings.from_packed(out, rec.frame_offset, rec.n_frames, rec.frames)
    fixed._words = _words(rec)
    if spec.smooth:
        fixed = sb.Recordings.from_packed(smooth_frames(fixed, spec.smooth), rec.frame_offset, rec.n_frames, rec.frames)
        fixed._words = _words(rec)
    return fixed, how, stats


def repair_batch(input_joints, spec):
    """A batch input_joints (B, T, J, 3) of any float dtype on a GPU, taken as B recordings of T frames -> (joints in the
    input's dtype, how (B, T, J) u8, stats (B, 4) i32) on its device.  The arithmetic is float64."""
    spec = _spec(spec, "repair_batch")
    x = input_joints
    if not (torch.is_tensor(x) and x.is_floating_point() and x.dim() == 4 and x.shape[3] == 3):
        raise ValueError("repair_batch: input_joints must be a float tensor (B, T, J, 3), got "
                         f"{tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
    if not x.is_cuda:
        raise RuntimeError("repair_batch: input_joints must be on a GPU (no CPU fallback)")
    B, T, J = (int(s) for s in x.shape[:3])
    if not (B >= 1 and 1 <= T <= sb.MAX_FRAMES and 1 <= J <= sb.MAX_J):
        raise ValueError(f"repair_batch: B >= 1, T in 1..{sb.MAX_FRAMES} and J in 1..{sb.MAX_J} expected, got "
                         f"{tuple(x.shape)}")
    packed = x.detach().to(torch.float64).reshape(B * T, J, 3).contiguous()
    if packed.data_ptr() == x.data_ptr():
        packed = packed.clone()
    frame_offset = torch.arange(B, dtype=torch.int64, device=x.device) * T
    n_frames = torch.full((B,), T, dtype=torch.int32, device=x.device)
    rec = sb.Recordings.from_packed(packed, frame_offset, n_frames, np.full(B, T, np.int32))
    fixed, how, stats = repair_packed(rec, spec)
    return fixed.joints.reshape(B, T, J, 3).to(x.dtype), how.reshape(B, T, J), stats


class RepairedSamples(sb.BuiltSamples):
    """build_samples' result with `repair=`: the BuiltSamples tuple, fields, order and length unchanged, and the
    attribute `repair`: stats (R, 4) int32 on the host, one row per recording given (kept or not)."""

    def __new__(cls, built, repair):
        self = super().__new__(cls, *built)
        self.repair = repair
        return self
