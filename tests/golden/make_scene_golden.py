"""G15: the reference's scene read-out (demo.py:204-256 `visualize_step` and `Vis_Demo`'s `dist_node2bbox`,
utils/virtualhome/vis_gt_vh.py:14-22) on designed inputs fed in directly, without a network or a renderer
(tests/scene_cases.py: g15_design -- the recorded parse results of G14, N = 3, K = 24, and full skeletons of 53 joints
over T = 40 frames with adjacent duplicates, distant duplicates and a +-0.0 pair).  Recorded, all from the imported
reference: `corners2params` + `rot2head` of every box, `head2rot` of every kept box, the keep masks, the demo's
unique-frame indices, and `dist_node2bbox` of every kept box on the de-duplicated frames.  The script asserts the margin
rule of the contact decisions and that the NumPy definitions of tests/scene_cases.py reproduce every recorded index
before it writes.  BUILD container only.

    python tests/golden/make_scene_golden.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True
import make_model_golden as mm  # noqa: E402
from tests import scene_cases as sc  # noqa: E402


def stand_in_vtk():
    """utils/vis_base.py does `from vtk.util.numpy_support import numpy_to_vtk` at module level and vtk is not installed:
    stand-in modules of this script's own, registered before the import; nothing recorded here renders anything"""
    util, support = types.ModuleType('vtk.util'), types.ModuleType('vtk.util.numpy_support')
    support.numpy_to_vtk = None
    util.numpy_support = support
    sys.modules['vtk.util'], sys.modules['vtk.util.numpy_support'] = util, support
    sys.modules['vtk'].util = util


def main():
    from net_utils.box_util import corners2params
    from utils.pc_utils import head2rot, rot2head
    from utils.virtualhome.vis_gt_vh import dist_node2bbox
    d = sc.g15_design()
    corners, prob, mask, cls = d['pred_corners_3d'], d['obj_prob'], d['pred_mask'], d['pred_sem_cls']
    joints, thr = d['input_joints'], float(d['dump_threshold'])
    N, K = prob.shape
    T, J = joints.shape[1:3]
    out = dict(d, box_params=np.zeros((N, K, 7)), keep=np.zeros((N, K), bool), rmat=np.zeros((N, K, 3, 3)),
               unique_count=np.zeros(N, np.int32), unique_index=np.full((N, T), -1, np.int32),
               contact_unique=np.full((N, K), -1, np.int32))
    for b in range(N):                                        # demo.py:217-256 with batch_id = b
        box_size, R_mat, center = corners2params(corners[b])
        heading = rot2head(R_mat)
        out['box_params'][b] = np.hstack([center, box_size, heading[:, np.newaxis]])
        keep_idx = np.logical_and(prob[b] > thr, mask[b, :] == 1)
        out['keep'][b] = keep_idx
        _, idx = np.unique(joints[b], axis=0, return_index=True)
        idx = np.sort(idx)
        out['unique_count'][b], out['unique_index'][b, :len(idx)] = len(idx), idx
        input_joint_pnts = joints[b][idx]
        for k in np.nonzero(keep_idx)[0]:
            bbox = out['box_params'][b, k]
            node = {'centroid': bbox[:3], 'R_mat': head2rot(float(bbox[6])), 'size': bbox[3:6], 'class_id': [cls[b, k]]}
            out['rmat'][b, k] = node['R_mat']
            out['contact_unique'][b, k] = dist_node2bbox([node], input_joint_pnts.reshape(-1, 3), J)[0]

    # the definitions reproduce every recorded index, with clear margins
    nd = sc.nodes_def(out['box_params'], prob, mask, cls, thr)
    ct = sc.contact_def(joints, nd.node_obbs, nd.node_rmat, nd.count)
    un = sc.unique_def(joints)
    worst = sc.assert_contact_margins(joints, ct, nd.count)
    assert np.array_equal(un.count, out['unique_count']) and np.array_equal(un.index, out['unique_index'])
    assert (un.count < T).all() and (un.rank != np.arange(T)).any()
    for b in range(N):
        kept = np.nonzero(out['keep'][b])[0]
        assert np.array_equal(nd.inst_idx[b, :nd.count[b]], kept) and nd.count[b] == len(kept) >= 1
        assert np.array_equal(nd.node_rmat[b, :len(kept)], out['rmat'][b, kept])
        assert np.array_equal(un.rank[b][ct.frame[b, :len(kept)]], out['contact_unique'][b, kept])
    path = os.path.join(HERE, 'g15_scene.npz')
    np.savez_compressed(path, **out)
    print('kept', out['keep'].sum(1), 'unique', out['unique_count'], 'of', T, 'contact margin %.3g' % worst,
          'bytes', os.path.getsize(path))


if __name__ == '__main__':
    mm.import_reference()
    stand_in_vtk()
    main()
