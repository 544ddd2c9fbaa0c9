"""Writes tests/golden/g19_recording_repair.npz: recordings with holes and what np.interp makes of them.

Per recording r: `r{r}_joints` (F, J, 3) float64 with NaN / inf coordinates where a joint is missing, and `r{r}_filled`,
np.interp over the measured frames of every (joint, coordinate) track, evaluated at every frame: linear inside a gap, the
nearest measurement in front of the first and behind the last measured frame.  The repair with max_gap above every gap
and hold_ends must reproduce it bit for bit (tests/test_recording_repair_cpu.py, tests/test_recording_repair_gpu.py).

    python tests/golden/make_recording_repair_golden.py
"""
import os

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'g19_recording_repair.npz')
SHAPES = ((37, 3), (130, 2), (64, 1), (9, 4))


def main():
    rng = np.random.default_rng(19)
    z = dict(n_recordings=np.int64(len(SHAPES)), numpy_version=np.array(np.__version__))
    for r, (F, J) in enumerate(SHAPES):
        x = rng.uniform(-1e3, 1e3, (F, J, 3))
        for j in range(J):
            missing = rng.random(F) < 0.35
            missing[rng.integers(F)] = False                    # every joint is measured somewhere
            lo = int(rng.integers(F))
            missing[lo:lo + int(rng.integers(1, 12))] &= j % 2 == 0     # and has a stretch without a hole, or a long one
            x[missing, j] = np.nan
            x[missing & (rng.random(F) < 0.3), j, rng.integers(3)] = rng.choice([np.inf, -np.inf, 12.5])
        if r == 1:
            x[60:70, 0] = np.nan                                # over the word boundary
            x[:3, 1], x[-5:, 1] = np.nan, np.nan                # both ends
        valid = np.isfinite(x).all(-1)
        assert valid.any(0).all() and not valid.all()
        frames = np.arange(F, dtype=np.float64)
        filled = np.empty_like(x)
        for j in range(J):
            for c in range(3):
                filled[:, j, c] = np.interp(frames, frames[valid[:, j]], x[valid[:, j], j, c])
        assert np.array_equal(filled[valid], x[valid])
        z[f'r{r}_joints'], z[f'r{r}_filled'] = x, filled
    np.savez_compressed(OUT, **z)
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
