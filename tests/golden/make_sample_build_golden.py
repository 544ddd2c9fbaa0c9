"""Writes tests/golden/g16_sample_build.npz: what stage 3 of the reference's data preparation
(utils/virtualhome/3_generate_samples.py, `run()` lines 96-187) makes of seeded raw recordings -- the fixture
csrc/sample_build.hip and its NumPy mirror (net_utils/sample_build.py) are pinned against.

    python tests/golden/make_sample_build_golden.py --reference PATH_TO_THE_REFERENCE_CHECKOUT

The reference script is loaded by file path with the stubs of make_vote_labels_golden.import_reference, and its
`check_in_box`, `augment_sample` and `get_votes` make every decision and every array: the room test of the origin joint
and the trim (its lines 96-103), the object test against the boxes enlarged by twice the contact distance (110-124),
the move to the room's floor centre (126-134), then per variant 0..7 augment_sample and, through
make_vote_labels_golden.reference_votes, get_votes over the variant's nodes (161-187).
Reading the simulator's files and the class mapping are not part of it: recordings come with mapped class ids.

A recording is a `synthetic.make_raw_sample` sequence widened to float64 with a seeded sub-float32 jitter, moved to a
world offset inside a room box, its leading frames pushed out of the room.  Cases: first = 0; first > 0; first = F - 1
(one frame kept); never in the room; in the room but near no object; no objects; a room turned about y.

Stored, data only: per recording r{i}_joints (F, 53, 3) f64, r{i}_room_centroid / _room_size / _room_R_mat,
r{i}_class_id / _centroid / _R_mat / _size (the object nodes), r{i}_first (-1: never in the room), r{i}_status (0 kept,
1 never in the room, 2 near no object); per kept recording and variant a: r{i}_a{a}_joints (n, 53, 3) f32 and
r{i}_a{a}_votes (n, 53, 10) f32 = the reference's float64 results cast as its file writer's consumers read them,
r{i}_a{a}_centroid / _R_mat (the augmented nodes), r{i}_hist (how many joints of variant 0 lie in 0, 1, 2, ... contact
boxes, by the reference's hull test), r{i}_face_dist (the smallest distance of a hip to a face of the room or of an
enlarged object box, and of a joint of any variant to a face of a contact box).  `names` are the base names.

The maker refuses to write a fixture in which that distance is below 1e-6 m (G13's bound), a hit count of 0, 1, 2 or >= 3
never occurs, or a rejection kind is missing.  With that margin every decision is the same with or without fused
multiply-adds in NumPy's BLAS.  Fixed zip timestamps: a re-run reproduces the file byte for byte.
"""
import argparse
import os
import sys
from copy import deepcopy

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_vote_labels_golden import import_reference, reference_votes, save_npz      # noqa: E402

PATH = os.path.join(HERE, 'g16_sample_build.npz')
MIN_FACE_DIST = 1e-6
CONTACT = 1.0
# name, frames, first (None: never in the room), boxes, seed, room angle about y, kind
CASES = [('first_0', 37, 0, 4, 21, 0.0, 'kept'),
         ('first_7', 12, 7, 6, 22, 0.0, 'kept'),
         ('last_frame_only', 20, 19, 1, 23, 0.0, 'kept'),
         ('never_in_room', 9, None, 4, 24, 0.0, 'no_room'),
         ('near_no_object', 11, 2, 3, 25, 0.0, 'no_object'),
         ('no_objects', 6, 0, 0, 26, 0.0, 'no_object'),
         ('turned_room', 8, 3, 5, 27, 0.6, 'kept')]
STATUS = {'kept': 0, 'no_room': 1, 'no_object': 2}


def rot_y(th):
    return np.array([[np.cos(th), 0., -np.sin(th)], [0., 1., 0.], [np.sin(th), 0., np.cos(th)]])


def make_recording(name, F, first, n_boxes, seed, angle, kind):
    from pose2room_amd.p2rnet.synthetic import make_raw_sample
    joints32, _, inst, _ = make_raw_sample(F, n_boxes=n_boxes, seed=seed)
    rng = np.random.default_rng(1000 + seed)
    world = np.array([rng.uniform(-40, 40), rng.uniform(-2, 2), rng.uniform(-40, 40)])
    joints = joints32.astype(np.float64) + rng.normal(0.0, 1e-5, joints32.shape) + world
    out = F if first is None else first
    joints[:out] += np.array([25.0, 0.0, 0.0])                   # the leading frames stand outside the room
    room = {'centroid': world + np.array([0.0, 1.5, 0.0]), 'size': np.array([9.0, 3.0, 9.5]), 'R_mat': rot_y(angle)}
    nodes = [{'class_id': int(n['class_id']), 'centroid': np.array(n['centroid']) + world, 'R_mat': np.array(n['R_mat']),
              'size': np.array(n['size'])} for n in inst]
    if kind == 'no_object':
        for n in nodes:
            n['centroid'] = n['centroid'] + np.array([60.0, 0.0, 60.0])
    elif nodes and first is not None:
        # the last frame's hip stands in box 0, so that a recording cut to one frame still passes the object test
        nodes[0]['centroid'][[0, 2]] = joints[-1, 0, [0, 2]] + np.array([0.21, -0.17])
        if name == 'last_frame_only':       # one small box off to the side: some joints of the frame lie in no box
            nodes = nodes[:1]
            nodes[0]['size'] = np.array([0.3, 0.4, 0.3])
            nodes[0]['centroid'][0] += 0.8
    return {'name': name, 'joints': joints, 'room_bbox': room, 'object_nodes': nodes}


def face_distance(points, box, half):
    """smallest | half_a - |local_a| | of (..., 3) points over the three axes of a box"""
    local = (points - np.asarray(box['centroid'])).dot(np.asarray(box['R_mat']).T)
    return float(np.abs(half - np.abs(local)).min())


def run_reference(ref, rec):
    """Stage 3 on one recording, every decision and every array made by the reference's check_in_box, augment_sample and
    get_votes -> (first, status, [(joints f64, votes f64, nodes, hits per joint)] per variant)"""
    from pose2room_amd.net_utils import sample_build as sb
    hip = rec['joints'][:, ref.dataset_config.origin_joint_id]
    in_room = np.flatnonzero(ref.check_in_box(hip, rec['room_bbox']))
    if in_room.size == 0:
        return -1, STATUS['no_room'], []
    first = int(in_room[0])
    kept = rec['joints'][first:]
    if not any(ref.check_in_box(hip[first:], box).any() for box in sb.enlarged_nodes(rec['object_nodes'], CONTACT)):
        return first, STATUS['no_object'], []
    # the origin moves to the room's floor centre; the room box itself is not stored, augment_sample only wants one
    shift = sb.floor_shift(rec['room_bbox'])
    room = dict(rec['room_bbox'], centroid=np.array(rec['room_bbox']['centroid']) - shift)
    moved = [dict(box, centroid=np.array(box['centroid']) - shift) for box in rec['object_nodes']]
    flip_per_frame = np.tile(sb.FLIP, (kept.shape[0], 1, 1))         # augment_sample multiplies frame by frame
    variants = []
    for a in range(8):
        _, nodes, joints = ref.augment_sample(deepcopy(room), deepcopy(moved), kept - shift, flip_per_frame, sb.ROT90, a)
        votes, hits = reference_votes(ref, joints, nodes, CONTACT)
        variants.append((joints, votes, nodes, hits.ravel()))
    return first, STATUS['kept'], variants


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    a = ap.parse_args()
    recs = [make_recording(*c) for c in CASES]
    ref = import_reference(os.path.abspath(a.reference))
    ref.dataset_config.contact_dist_thresh = CONTACT
    origin = ref.dataset_config.origin_joint_id
    out = {'n_recordings': np.array(len(recs)), 'names': np.array([r['name'] for r in recs]),
           'contact_dist': np.array(CONTACT), 'origin_joint': np.array(origin)}
    total, seen = np.zeros(4, np.int64), set()
    for i, (rec, case) in enumerate(zip(recs, CASES)):
        first, status, variants = run_reference(ref, rec)
        assert status == STATUS[case[6]] and first == (-1 if case[2] is None else case[2]), (case, first, status)
        seen.add(status)
        nodes, room = rec['object_nodes'], rec['room_bbox']
        n = len(nodes)
        hip = rec['joints'][:, origin]
        dist = face_distance(hip, room, np.array(room['size']) / 2.)
        for node in nodes:
            dist = min(dist, face_distance(hip, node, (np.array(node['size']) + 2 * CONTACT) / 2.))
        out.update({f'r{i}_joints': rec['joints'], f'r{i}_room_centroid': room['centroid'], f'r{i}_room_size': room['size'],
                    f'r{i}_room_R_mat': room['R_mat'], f'r{i}_first': np.array(first), f'r{i}_status': np.array(status),
                    f'r{i}_class_id': np.array([x['class_id'] for x in nodes], np.int64),
                    f'r{i}_centroid': np.array([x['centroid'] for x in nodes], np.float64).reshape(n, 3),
                    f'r{i}_R_mat': np.array([x['R_mat'] for x in nodes], np.float64).reshape(n, 3, 3),
                    f'r{i}_size': np.array([x['size'] for x in nodes], np.float64).reshape(n, 3)})
        hist = np.zeros(11, np.int64)
        for v, (joints, votes, vnodes, hits) in enumerate(variants):
            assert joints.dtype == np.float64 and votes.dtype == np.float64
            assert np.array_equal(votes[..., 0].ravel() != 0, hits > 0) and votes.shape == joints.shape[:2] + (10,)
            for node in vnodes:
                dist = min(dist, face_distance(joints, node, np.array(node['size']) / 2. + CONTACT))
            if v == 0:
                hist = np.bincount(np.minimum(hits, 10), minlength=11)
            out.update({f'r{i}_a{v}_joints': joints.astype(np.float32), f'r{i}_a{v}_votes': votes.astype(np.float32),
                        f'r{i}_a{v}_centroid': np.array([x['centroid'] for x in vnodes], np.float64).reshape(n, 3),
                        f'r{i}_a{v}_R_mat': np.array([x['R_mat'] for x in vnodes], np.float64).reshape(n, 3, 3)})
        assert dist >= MIN_FACE_DIST, f"recording {i} ({rec['name']}): {dist:.3g} m from a face: choose another seed"
        total += np.array([hist[0], hist[1], hist[2], hist[3:].sum()])
        out.update({f'r{i}_hist': hist, f'r{i}_face_dist': np.array(dist)})
        print(f"{i} {rec['name']}: F={rec['joints'].shape[0]} first={first} status={status} boxes={n} "
              f"hist={hist.tolist()} face={dist:.3g}")
    assert all(total > 0), f"a hit count of 0, 1, 2 or >= 3 never occurs: {total.tolist()}"
    assert seen == {0, 1, 2}, f"a rejection kind is missing: {sorted(seen)}"
    save_npz(PATH, out)
    print(f"wrote {PATH}: {os.path.getsize(PATH)} bytes, hits over all kept recordings {total.tolist()}")
    assert os.path.getsize(PATH) < 1000000


if __name__ == '__main__':
    main()
