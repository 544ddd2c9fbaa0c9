"""Writes tests/golden/g13_vote_labels.npz: vote labels made by the reference's own `get_votes`
(utils/virtualhome/3_generate_samples.py:56-79, driven as its lines 176-187 drive it) for seeded samples of this
project, the fixture csrc/vote_labels.hip and its NumPy mirror are pinned against.

    python tests/golden/make_vote_labels_golden.py [--reference /root/reference]

The reference script is loaded by file path (its name is no module name); the modules its imports need and this image
lacks (h5py, quaternion, plyfile, trimesh, seaborn, the Unity simulator's utils_viz) are stubbed as
make_model_golden.import_reference stubs them -- none of them is on get_votes' path, which needs NumPy and SciPy's
Delaunay only.  Joints are f32 widened to f64, as a sample file's are.

Per sample i: s{i}_joints (T0, 53, 3) f32, s{i}_class_id / _centroid / _R_mat / _size (the instance list),
s{i}_contact_dist, s{i}_votes (T0, 53, 10) = the reference's f64 votes cast to f32, s{i}_hist = how many joints lie in
0, 1, 2, ... contact boxes (counted with the reference's hull test), s{i}_face_dist = the smallest distance of any
joint to any face of any contact box.  The maker refuses to write a fixture in which a hit count of 0, 1, 2, 3 or >= 4
never occurs, or in which a joint is closer than 1e-6 m to a face (a label must not hang on a rounding of the hull test).
The file is written with fixed zip timestamps, so a re-run reproduces it byte for byte.
"""
import argparse
import importlib.util
import io
import os
import sys
import tempfile
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

PATH = os.path.join(HERE, 'g13_vote_labels.npz')
# (T0, n_boxes, seed) of synthetic.make_raw_sample, contact distance 1.0
SYNTHETIC = [(1, 10, 1), (5, 10, 2), (37, 10, 3), (37, 2, 4), (19, 1, 5), (7, 0, 6), (37, 4, 7)]
DEMO_FRAMES, DEMO_BOXES, DEMO_SEED = 37, 6, 13          # the reference's demo pose sequence (g8: demo_sequence)
SECOND = (19, 6, 8, 0.5)                                # (T0, n_boxes, seed, contact distance)
MIN_FACE_DIST = 1e-6


def import_reference(reference):
    """-> the module of utils/virtualhome/3_generate_samples.py"""
    sys.path.insert(0, reference)
    stubs = ['h5py', 'quaternion', 'plyfile', 'trimesh', 'seaborn', 'external', 'external.virtualhome',
             'external.virtualhome.simulation', 'external.virtualhome.simulation.unity_simulator',
             'external.virtualhome.simulation.unity_simulator.utils_viz']
    for n in stubs:
        sys.modules[n] = types.ModuleType(n)
        sys.modules[n].__path__ = []
    sys.modules['plyfile'].PlyData = sys.modules['plyfile'].PlyElement = object
    sys.modules['external.virtualhome.simulation.unity_simulator.utils_viz'].get_skeleton = None
    scratch = tempfile.mkdtemp()            # Dataset_Config makes its data directories under the working directory
    os.makedirs(os.path.join(scratch, 'datasets'), exist_ok=True)
    os.chdir(scratch)
    spec = importlib.util.spec_from_file_location(
        'p2r_reference_generate_samples', os.path.join(reference, 'utils', 'virtualhome', '3_generate_samples.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_votes(ref, joints, instances, contact_dist):
    """The reference's votes of one sample (lines 176-187 of its script around its get_votes) -> (votes (T0, J, 10) f64,
    hits (T0, J): the number of contact boxes each joint lies in by the reference's own hull test)."""
    from utils.pc_utils import extract_pc_in_box3d
    from utils.tools import get_box_corners
    ref.dataset_config.contact_dist_thresh = contact_dist
    n_frames, n_joints = joints.shape[:2]
    all_joints = joints.astype(np.float64).reshape(n_frames * n_joints, 3)
    N = n_frames * n_joints
    joint_votes = np.zeros((N, 10))
    joint_vote_idx = np.zeros((N)).astype(np.int32)
    indices = np.arange(N)
    hits = np.zeros(N, np.int64)
    for node in instances:
        joint_votes, joint_vote_idx = ref.get_votes(node, all_joints, joint_votes, indices, joint_vote_idx)
        vectors = np.diag(np.array(node['size']) / 2. + contact_dist).dot(node['R_mat'])
        hits += extract_pc_in_box3d(all_joints, np.array(get_box_corners(node['centroid'], vectors)))[1]
    return joint_votes.reshape(n_frames, n_joints, 10), hits.reshape(n_frames, n_joints)


def face_distance(joints, instances, contact_dist):
    """smallest | h_a - |local_a| | over all joints, boxes and axes (inf without boxes)"""
    p = joints.astype(np.float64)
    best = np.inf
    for node in instances:
        local = (p - np.asarray(node['centroid'])).dot(np.asarray(node['R_mat']).T)
        best = min(best, float(np.abs(np.array(node['size']) / 2. + contact_dist - np.abs(local)).min()))
    return best


def demo_sample():
    """the first frames of the reference's demo pose sequence with seeded boxes around it"""
    g8 = np.load(os.path.join(HERE, 'g8_loader_demo.npz'))
    joints = np.ascontiguousarray(g8['demo_sequence'][:DEMO_FRAMES]).astype(np.float32)
    rng = np.random.default_rng(DEMO_SEED)
    mid = joints.reshape(-1, 3).astype(np.float64).mean(0)
    instances = []
    for _ in range(DEMO_BOXES):
        th = rng.uniform(-np.pi, np.pi)
        R = np.array([[np.cos(th), 0., -np.sin(th)], [0., 1., 0.], [np.sin(th), 0., np.cos(th)]])
        c = np.array([mid[0] + rng.uniform(-1.5, 1.5), rng.uniform(0.2, 1.5), mid[2] + rng.uniform(-1.5, 1.5)])
        instances.append({'class_id': int(rng.integers(0, 22)), 'centroid': c, 'R_mat': R,
                          'size': rng.uniform(0.3, 2.0, 3)})
    return joints, instances


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps (NumPy stamps the members with the time of writing)"""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for key, value in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(value), allow_pickle=False)
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default='/root/reference')
    a = ap.parse_args()
    from pose2room_amd.p2rnet.synthetic import make_raw_sample
    cases = []
    for T0, nb, seed in SYNTHETIC:
        joints, _, inst, name = make_raw_sample(T0, n_boxes=nb, seed=seed)
        cases.append((name, joints, inst, 1.0))
    cases.append(('demo_sequence',) + demo_sample() + (1.0,))
    T0, nb, seed, thr = SECOND
    joints, _, inst, name = make_raw_sample(T0, n_boxes=nb, seed=seed)
    cases.append((name + '_contact_0.5', joints, inst, thr))

    ref = import_reference(os.path.abspath(a.reference))
    out = {'n_samples': np.array(len(cases)), 'names': np.array([c[0] for c in cases])}
    total = np.zeros(11, np.int64)
    for i, (name, joints, inst, thr) in enumerate(cases):
        votes, hits = reference_votes(ref, joints, inst, thr)
        hist = np.bincount(hits.ravel(), minlength=11)
        dist = face_distance(joints, inst, thr)
        assert dist >= MIN_FACE_DIST, f"sample {i} ({name}): a joint {dist:.3g} m from a face: choose another seed"
        assert np.array_equal(votes[..., 0] != 0, hits > 0)
        total += hist
        n = len(inst)
        out.update({f's{i}_joints': joints, f's{i}_class_id': np.array([x['class_id'] for x in inst], np.int64),
                    f's{i}_centroid': np.array([x['centroid'] for x in inst], np.float64).reshape(n, 3),
                    f's{i}_R_mat': np.array([x['R_mat'] for x in inst], np.float64).reshape(n, 3, 3),
                    f's{i}_size': np.array([x['size'] for x in inst], np.float64).reshape(n, 3),
                    f's{i}_contact_dist': np.array(thr), f's{i}_votes': votes.astype(np.float32),
                    f's{i}_hist': hist, f's{i}_face_dist': np.array(dist)})
        print(f"{i} {name}: T0={joints.shape[0]} boxes={n} contact={thr} hist={hist.tolist()} face={dist:.3g}")
    assert all(total[:4] > 0) and total[4:].sum() > 0, f"a hit count of 0, 1, 2, 3 or >= 4 never occurs: {total.tolist()}"
    save_npz(PATH, out)
    print(f"wrote {PATH}: {os.path.getsize(PATH)} bytes, hits over all samples {total.tolist()}")


if __name__ == '__main__':
    main()
