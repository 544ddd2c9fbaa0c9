"""G16 (tests/golden/g16_sample_build.npz, made by tests/golden/make_sample_build_golden.py from the reference's own
check_in_box / augment_sample / get_votes) as recordings and expected samples, and seeded recordings for the scan's
edge cases; shared by tests/test_sample_build_cpu.py and tests/test_sample_build_gpu.py.  Loaded once, never changed."""
import collections
import functools
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g16_sample_build.npz')
REASONS = {0: None, 1: "never in the room", 2: "near no object"}

# recording: the dict build_samples takes; first / reason: the reference's; variants: per a = 0..7 (joints f32, votes
# f32, nodes) of the reference, [] for a rejected recording
Case = collections.namedtuple("Case", "recording first reason variants hist face_dist")


@functools.lru_cache(maxsize=None)
def g16():
    z = np.load(PATH)
    cases = []
    for i in range(int(z['n_recordings'])):
        k = lambda s: z[f'r{i}_{s}']                                            # noqa: E731
        nodes = [dict(class_id=int(c), centroid=k('centroid')[j].copy(), R_mat=k('R_mat')[j].copy(),
                      size=k('size')[j].copy()) for j, c in enumerate(k('class_id'))]
        rec = dict(name=str(z['names'][i]), joints=k('joints'), object_nodes=nodes,
                   room_bbox=dict(centroid=k('room_centroid'), size=k('room_size'), R_mat=k('room_R_mat')))
        status = int(k('status'))
        variants = []
        if status == 0:
            for a in range(8):
                vn = [dict(class_id=n['class_id'], centroid=k(f'a{a}_centroid')[j], R_mat=k(f'a{a}_R_mat')[j],
                           size=n['size']) for j, n in enumerate(nodes)]
                variants.append((k(f'a{a}_joints'), k(f'a{a}_votes'), vn))
        cases.append(Case(rec, int(k('first')), REASONS[status], variants, k('hist'), float(k('face_dist'))))
    return cases, float(z['contact_dist']), int(z['origin_joint'])


def seeded_recording(F, first, J=53, origin=0, seed=0, near=True, name=None):
    """A recording of F frames whose origin joint enters a 10 x 3 x 10 room around (100, 1.5, -50) at frame `first`
    (None: never) and, with `near`, stands inside the one object box from then on; near='before': the box stands where the
    body is BEFORE it enters the room, so only trimmed frames are near it.  Margins to every face >= 0.1 m."""
    rng = np.random.default_rng(seed)
    centre = np.array([100.0, 0.0, -50.0])
    hip = centre + np.stack([rng.uniform(-2, 2, F), np.full(F, 0.9), rng.uniform(-2, 2, F)], -1)
    joints = hip[:, None, :] + rng.uniform(-0.5, 0.5, (F, J, 3))
    joints[:, origin] = hip
    joints[:F if first is None else first] += np.array([0.0, 0.0, 30.0])
    room = dict(centroid=centre + np.array([0.0, 1.5, 0.0]), size=np.array([10.0, 3.0, 10.0]), R_mat=np.eye(3))
    where = {True: [0.0, 1.0, 0.0], False: [8.0, 1.0, 0.0], 'before': [0.0, 1.0, 30.0]}[near]
    box = dict(class_id=3, centroid=centre + np.array(where), R_mat=np.eye(3), size=np.array([2.2, 1.0, 2.2]))
    return dict(name=name or f'seeded_{F}_{first}_{seed}', joints=joints, room_bbox=room, object_nodes=[box])
