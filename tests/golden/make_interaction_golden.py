"""G20: which joints of a walking body lie inside the enlarged boxes of one designed scene, from the reference's own code
(tests/interaction_cases.py: g20_design -- 130 frames of 53 float32 joints, six rotated boxes, contact distance 0.1).
Recorded: the inputs; per (node, frame, joint) the mask the reference's `extract_pc_in_box3d` (utils/pc_utils.py: a
Delaunay hull test) returns for the corners its `get_box_corners` (utils/tools.py) makes of the enlarged vectors
`diag(size / 2 + contact distance) . R_mat` -- the steps of `get_votes`, utils/virtualhome/3_generate_samples.py:59-64 --
bit-packed along the joints; and from that mask alone the frame bits, the joints per frame and the joint mask per node.
The hull test has a tolerance and the closed form has none: the script asserts with the float64 definition that no joint
lies within 1e-9 of an enlarged face, and takes the next seed if one does; it asserts that `interaction_reference`
reproduces the recorded arrays before it writes.  BUILD container only.

    python tests/golden/make_interaction_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True
import make_model_golden as mm  # noqa: E402
from make_scene_golden import stand_in_vtk  # noqa: E402
from make_vote_labels_golden import save_npz  # noqa: E402
from tests import interaction_cases as ic  # noqa: E402
from pose2room_amd.net_utils import interaction_device as idv  # noqa: E402


def main():
    from utils.pc_utils import extract_pc_in_box3d
    from utils.tools import get_box_corners
    thresh = ic.G20_THRESH
    for seed in range(20, 40):
        joints, count, obbs, rmat = ic.g20_design(seed)
        worst, zeros = ic.margins(joints, count, obbs, rmat, thresh)
        if worst >= ic.MARGIN and zeros == 0:
            break
    else:
        raise SystemExit("no seed keeps every joint 1e-9 from every enlarged face")
    _, T, J, _ = joints.shape
    K = obbs.shape[1]
    all_joints = joints[0].astype(np.float64).reshape(T * J, 3)
    inside = np.zeros((1, K, T, J), bool)
    for s in range(int(count[0])):
        enlarged = np.diag(obbs[0, s, 3:6] / 2.0 + thresh).dot(rmat[0, s])          # half sizes plus the distance, as rows
        corners = np.array(get_box_corners(obbs[0, s, 0:3], enlarged))
        inside[0, s] = extract_pc_in_box3d(all_joints, corners)[1].reshape(T, J)
    njoint = inside.sum(3).astype(np.uint8)
    bits = idv.pack_bits(njoint > 0)
    joint_mask = idv.pack_bits(inside.any(2))[..., 0]

    assert np.array_equal(idv.reference_inside(joints, count, obbs, rmat, thresh), inside)
    ref = idv.interaction_reference(joints, count, obbs, rmat, thresh)
    assert np.array_equal(ref.bits, bits) and np.array_equal(ref.njoint, njoint) and np.array_equal(ref.joint_mask, joint_mask)
    per_node = (njoint > 0).sum(2)[0]
    assert (per_node > 0).sum() >= 4 and (per_node < T).all() and njoint.max() > 1, per_node

    path = os.path.join(HERE, 'g20_interaction.npz')
    save_npz(path, dict(seed=np.int64(seed), joints=joints, count=count, node_obbs=obbs, node_rmat=rmat,
                        contact_thresh=np.float64(thresh), inside=np.packbits(inside, axis=3, bitorder='little'),
                        bits=bits, njoint=njoint, joint_mask=joint_mask, margin=np.float64(worst)))
    print('seed', seed, 'frames in contact per node', per_node.tolist(), 'most joints', int(njoint.max()),
          'margin %.3g' % worst, 'bytes', os.path.getsize(path))


if __name__ == '__main__':
    mm.import_reference()
    stand_in_vtk()
    main()
