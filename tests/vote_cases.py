"""Shared inputs of tests/test_vote_labels_cpu.py and tests/test_vote_labels_gpu.py: the samples of G13
(tests/golden/g13_vote_labels.npz, the reference's own get_votes; maker: tests/golden/make_vote_labels_golden.py) and a
second ragged set the fixture does not hold.  Loaded and computed once per process."""
import collections
import functools
import os

import numpy as np

G13_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g13_vote_labels.npz')

Case = collections.namedtuple('Case', 'name joints instances contact_dist votes hist face_dist')


@functools.lru_cache(maxsize=None)
def g13():
    """-> tuple of Case, votes = the reference's, cast to f32"""
    g = np.load(G13_PATH)
    out = []
    for i in range(int(g['n_samples'])):
        inst = [{'class_id': int(g[f's{i}_class_id'][k]), 'centroid': g[f's{i}_centroid'][k],
                 'R_mat': g[f's{i}_R_mat'][k], 'size': g[f's{i}_size'][k]} for k in range(len(g[f's{i}_class_id']))]
        out.append(Case(str(g['names'][i]), g[f's{i}_joints'], inst, float(g[f's{i}_contact_dist']), g[f's{i}_votes'],
                        g[f's{i}_hist'], float(g[f's{i}_face_dist'])))
    return tuple(out)


# (T0, n_boxes) of the second set, seeds 400..: one frame, frame counts around a workgroup's 256 items (5 frames = 265
# items), a sample far longer than one workgroup, all ten box slots full and none
SECOND = [(1, 3), (2, 10), (5, 0), (6, 7), (64, 4), (300, 10)]


@functools.lru_cache(maxsize=None)
def second_set():
    """-> tuple of (joints, mirror votes, instances, name) raw samples, contact distance 1.0"""
    from pose2room_amd.net_utils.vote_labels import vote_labels_reference
    from pose2room_amd.p2rnet.synthetic import make_raw_sample
    out = []
    for i, (T0, nb) in enumerate(SECOND):
        joints, _, inst, name = make_raw_sample(T0, n_boxes=nb, seed=400 + i)
        out.append((joints, vote_labels_reference(joints, inst, 1.0), inst, name))
    return tuple(out)


def mirrored(case):
    """a G13 case as a raw sample (joints, votes, instances, name) with the reference's votes"""
    return case.joints, case.votes, case.instances, case.name
