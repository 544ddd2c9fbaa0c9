"""Inputs, mirror results and the median-gap rule shared by tests/test_mdn_readout_cpu.py and tests/test_mdn_readout_gpu.py.

The case: B = 2, L = 9 (18 rows: one full 16-row group of the sampler and a partial one), heads (3, f32), (3, f32),
(2, f64) under stream indices 0, 1, 2, six hypotheses with 1, 2, 7, 16, 17 and 256 draws (below, at and above one round
of the kernel's 16 sample slices; Nmax = 256), G = 3 or 100 components.  Everything is NumPy on the host and computed once
per G (`case`); nobody may write to what it returns.

Median-gap rule.  A kernel draw may differ from the mirror's by rounding; where two of the mirror's order statistics
around the median are closer than the comparison tolerance, the kernel may rightly rank them the other way round and
return the neighbour.  `gap_flags` marks the output elements whose median order statistic has a neighbouring order
statistic (rank - 1 or rank + 1) within the tolerance -- equal neighbours included.  The inputs below are chosen so that
the mirror alone keeps that share at or below 1 % (test_mdn_readout_cpu.py asserts it): mixture weights drawn towards 1
(sigmoid(2 z + 4)), so that a draw with no open gate -- the exact value 0, which ties with every other such draw -- is
rare, and sigma in exp(-0.8 .. 0.4) against a tolerance of 2e-6 (f32) / 1e-12 (f64) of the value range.
"""
import functools

import numpy as np

B, L = 2, 9
COUNTS = (1, 2, 7, 16, 17, 256)
DIMS = ((3, np.float32), (3, np.float32), (2, np.float64))
SEED = 0x5eed0fd2a7500d17
H_OFFSET = 3
GS = (3, 100)
# the factors of tests/test_mdn_sample_gpu._assert_mirror, by f64; test_mdn_readout_cpu.py checks that they are
MIRROR_RTOL = {False: 2e-6, True: 1e-12}


def mirror_tolerance(want, f64):
    """absolute tolerance `_assert_mirror` applies to a comparison against `want`"""
    return MIRROR_RTOL[bool(f64)] * max(float(want.max() - want.min()), 1.0)


def heads_np(G, seed=40):
    rng = np.random.default_rng(seed + G)
    return [(rng.standard_normal((G, D)).astype(dt), (rng.random((G, D)) * 1.2 - 0.8).astype(np.float32))
            for D, dt in DIMS]


def pis_np(G, seed=41):
    """(B, 3 * G, L) f32: the three heads' mixture weights as channel blocks of one tensor"""
    rng = np.random.default_rng(seed + G)
    z = rng.standard_normal((B, len(DIMS) * G, L))
    return (1.0 / (1.0 + np.exp(-(2.0 * z + 4.0)))).astype(np.float32)


def order_stats(draws, counts):
    """draws (H, B, L, Nmax, D) -> (below, median, above), each (H, B, L, D): the order statistics of rank
    (n - 1) // 2 - 1, (n - 1) // 2 and (n - 1) // 2 + 1 of every hypothesis' first n draws (NaN where there is none)"""
    H, b, l, _, D = draws.shape
    out = [np.full((H, b, l, D), np.nan, dtype=draws.dtype) for _ in range(3)]
    for h, n in enumerate(counts):
        srt = np.sort(draws[h, :, :, :n], axis=2)
        k = (n - 1) // 2
        for o, kk in zip(out, (k - 1, k, k + 1)):
            if 0 <= kk < n:
                o[h] = srt[:, :, kk]
    return out


def gap_flags(draws, counts, f64):
    """-> bool (H, B, L, D): the median order statistic has a neighbour within the comparison tolerance"""
    below, med, above = order_stats(draws, counts)
    tol = mirror_tolerance(med, f64)
    with np.errstate(invalid='ignore'):
        return (np.abs(med - below) <= tol) | (np.abs(above - med) <= tol)


@functools.lru_cache(maxsize=None)
def case(G):
    """-> dict(heads=[(mu, log_sigma)], pi=(B, 3G, L), median=[(H, B, L, D)], draws=[(H, B, L, 256, D)], flags=[bool])"""
    from pose2room_amd.p2rnet.mdn_sample_op import sample_reference
    heads, pi = heads_np(G), pis_np(G)
    median, draws, flags = [], [], []
    for j, (mu, ls) in enumerate(heads):
        m, d = sample_reference(pi[:, j * G:(j + 1) * G], mu, ls, COUNTS, SEED, H_OFFSET, j, readout='median',
                                return_draws=True)
        median.append(m)
        draws.append(d)
        flags.append(gap_flags(d, COUNTS, mu.dtype == np.float64))
    return dict(heads=heads, pi=pi, median=median, draws=draws, flags=flags)
