"""G17: the links and greedy clusters of a designed pool of oriented boxes, from the reference's own box code
(tests/consensus_cases.py: g17_design -- H = 3 hypotheses of one sample, K = 6, rotated boxes around shared objects, two
classes).  Recorded: the inputs; for every pair of the pool that passes the class test the reference's
`box3d_iou(get_box_corners(...), get_box_corners(...))` with the item that precedes as the first argument (NaN for the
other pairs); the link matrices at thresholds 0.25 and 0.5; and the clusters of a plain greedy loop over each: walking
the items by score descending, pool index ascending, an item joins the earliest leader it is linked to, or leads.  The
script asserts the 1e-6 margin of every IoU from both thresholds and that `consensus_reference` reproduces the links and
the clusters before it writes.  BUILD container only.

    python tests/golden/make_consensus_golden.py
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
from tests import consensus_cases as cc  # noqa: E402
from pose2room_amd.net_utils import consensus_device as cd  # noqa: E402


def main():
    from net_utils.box_util import box3d_iou
    from utils.pc_utils import head2rot
    from utils.tools import get_box_corners
    c = cc.g17_design()
    H, K = c.H, c.node_cls.shape[1]
    pool = [(h, s) for h in range(H) for s in range(int(c.count[h]))]
    m = len(pool)
    obb = np.array([c.node_obbs[h, s] for h, s in pool])
    cls = np.array([c.node_cls[h, s] for h, s in pool])
    score = np.array([c.node_score[h, s] for h, s in pool], np.float32)
    corners = [np.array(get_box_corners(o[0:3], np.diag(o[3:6] / 2.) @ head2rot(float(o[6])))) for o in obb]
    order = sorted(range(m), key=lambda p: (-float(score[p]), p))
    rank = {p: r for r, p in enumerate(order)}
    iou = np.full((m, m), np.nan)
    for i in range(m):
        for j in range(i + 1, m):
            if cls[i] == cls[j]:
                a, b = (i, j) if rank[i] < rank[j] else (j, i)
                iou[i, j] = iou[j, i] = box3d_iou(corners[a], corners[b])[0]
    out = dict(count=c.count, node_obbs=c.node_obbs, node_cls=c.node_cls, node_score=c.node_score, H=np.int64(H), iou=iou,
               order=np.array(order, np.int64))
    for tag, thr in (('025', 0.25), ('050', 0.5)):
        v = iou[~np.isnan(iou)]
        assert np.abs(v - thr).min() >= cc.MARGIN
        with np.errstate(invalid='ignore'):
            link = iou > thr
        leaders, cluster = [], np.full(m, -1, np.int64)
        for p in order:                                       # the plain greedy loop
            for ci, L in enumerate(leaders):
                if link[L, p]:
                    cluster[p] = ci
                    break
            else:
                leaders.append(p)
                cluster[p] = len(leaders) - 1
        out['link_' + tag], out['cluster_' + tag], out['leaders_' + tag] = link, cluster, np.array(leaders, np.int64)
        ref, extras = cd.consensus_reference(*cc.inputs(c), thr, True, return_iou=True)
        np.testing.assert_allclose(extras[0][0], iou, rtol=0, atol=1e-9, equal_nan=True)
        assert extras[0][1] == pool and ref.n_clusters[0] == len(leaders)
        assert np.array_equal(ref.leader_node[0, :len(leaders)], [pool[L][0] * K + pool[L][1] for L in leaders])
        assert np.array_equal([ref.cluster_of[h, s] for h, s in pool], cluster)
    assert len(out['leaders_025']) < len(out['leaders_050']) < m           # the thresholds differ, and something merges
    path = os.path.join(HERE, 'g17_consensus.npz')
    np.savez_compressed(path, **out)
    print('pool', m, 'clusters', len(out['leaders_025']), len(out['leaders_050']), 'bytes', os.path.getsize(path))


if __name__ == '__main__':
    mm.import_reference()
    stand_in_vtk()
    main()
