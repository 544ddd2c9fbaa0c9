"""Writes g12_mdn_readout.npz: the 'mean' output of `mdn_sample_op.sample_reference` for two small heads, recorded with the
mirror as it was before it learnt the median / per-draw read-outs, with the inputs and the seeds they come from.
tests/test_mdn_readout_cpu.py holds the mirror to these bytes.  Run from the repository root; the mirror is pure NumPy."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from pose2room_amd.p2rnet.mdn_sample_op import sample_reference   # noqa: E402

B, L, G = 2, 9, 5
ns = [1, 2, 7, 16]
out = {'n_samples': np.array(ns), 'shape_BLG': np.array([B, L, G])}
for tag, D, dt, in_seed, seed, hid in (('f32', 3, np.float32, 1201, 0x1234abcd5678ef01, 0),
                                       ('f64', 2, np.float64, 1202, 0x0fedcba987654321, 2)):
    rng = np.random.default_rng(in_seed)
    pi = rng.random((B, G, L)).astype(np.float32)
    mu = rng.standard_normal((G, D)).astype(dt)
    ls = (rng.random((G, D)) * 1.2 - 0.8).astype(np.float32)
    mean = sample_reference(pi, mu, ls, ns, seed, h_offset=3, head_id=hid)
    out.update({f'{tag}_pi': pi, f'{tag}_mu': mu, f'{tag}_log_sigma': ls, f'{tag}_mean': mean,
                f'{tag}_input_seed': np.array(in_seed), f'{tag}_seed': np.array(seed, dtype=np.uint64),
                f'{tag}_h_offset': np.array(3), f'{tag}_head_id': np.array(hid)})
np.savez(os.path.join(HERE, 'g12_mdn_readout.npz'), **out)
