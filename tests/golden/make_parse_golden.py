"""G14: the reference's `parse_predictions` with `remove_far_box: True` (ap_helper.py:183-196, the Delaunay hull test of
every hip position against every enlarged box) on designed end points fed in directly, without a network
(tests/parse_cases.py: g14_design -- N = 3, K = 24, T = 40, rotated boxes, a hip track that enters some enlarged boxes
and misses others, at least two near boxes per sample).  Every far-box, size-bound, score-order and overlap decision of
the inputs is at least MARGIN from its threshold in the float64 replay, in all three NMS modes; the script checks that,
and that the replay reproduces the reference's masks, before it writes.  BUILD container only.

    python tests/golden/make_parse_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True
import make_model_golden as mm  # noqa: E402
from tests import parse_cases as pc  # noqa: E402

NMS_IOU = 0.1
# name of the recorded mask -> (use_3d_nms, use_cls_nms, nms_mode of the replay)
MODES = {'pred_mask': (True, False, 0), 'pred_mask_cls': (True, True, 1), 'pred_mask_2d': (False, False, 2)}


def main():
    from net_utils.ap_helper import parse_predictions
    case = pc.g14_design()
    ep = {'center': torch.from_numpy(case.center), 'size': torch.from_numpy(case.size_log),
          'heading': torch.from_numpy(case.heading_sc), 'objectness_scores': torch.from_numpy(case.objectness),
          'sem_cls_scores': torch.from_numpy(case.sem_scores)}
    data = {'input_joints': torch.from_numpy(case.joints)}
    out = {'center': case.center, 'size': case.size_log, 'heading': case.heading_sc,
           'objectness_scores': case.objectness, 'sem_cls_scores': case.sem_scores, 'input_joints': case.joints,
           'nms_iou': np.float64(NMS_IOU)}
    for key, (use_3d, use_cls, mode) in MODES.items():
        cfg = mm.RefCfg({'mode': 'test', 'test': {
            'remove_far_box': True, 'use_3d_nms': use_3d, 'nms_iou': NMS_IOU, 'use_old_type_nms': False,
            'use_cls_nms': use_cls, 'per_class_proposal': True, 'conf_thresh': 0.05, 'multi_mode': False,
            'sample_cls': False}})
        assert cfg.dataset_config.origin_joint_id == case.origin_joint
        assert cfg.dataset_config.contact_dist_thresh == case.contact_dist
        out['contact_dist'] = np.float64(cfg.dataset_config.contact_dist_thresh)
        eval_dict, parsed = parse_predictions(ep, data, cfg.eval_config)
        # the float64 replay: margins of every decision, and the reference's far-box decisions themselves -- a kept box
        # passed the filter, and the boxes the replay calls near are exactly those among which the NMS picked
        r = pc.restate_case(case._replace(nms_mode=mode))
        gap, over = pc.nms_margins(r.boxes, r.nonempty, NMS_IOU, mode == 1)
        margins = dict(far=r.far_margin.min(), size=r.size_margin.min(), order=gap, overlap=over)
        assert min(margins.values()) >= pc.MARGIN, (key, margins)
        assert r.nonempty.sum(1).min() >= 1
        assert not (eval_dict['pred_mask'].astype(bool) & ~r.nonempty.astype(bool)).any(), key
        np.testing.assert_allclose(r.corners, parsed['pred_corners_3d'], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(r.obj_prob, parsed['obj_prob'], rtol=1e-6, atol=1e-7)
        assert np.array_equal(r.pred_cls, parsed['pred_sem_cls'])
        out[key] = eval_dict['pred_mask']
        print(key, 'kept', eval_dict['pred_mask'].sum(1), 'of near', r.nonempty.sum(1), 'of', r.nonempty.shape[1],
              {k: float('%.3g' % v) for k, v in margins.items()})
    out['pred_corners_3d'] = parsed['pred_corners_3d']
    out['obj_prob'] = parsed['obj_prob']
    out['pred_sem_cls'] = parsed['pred_sem_cls'].astype(np.int64)
    # the reference's far-box mask is local to parse_predictions: at nms_iou = 1 no box suppresses another (an IoU never
    # exceeds 1), so the keep mask of that run IS the mask of the boxes that passed the Delaunay test
    cfg.eval_config['nms_iou'] = 1.0
    out['nonempty'] = parse_predictions(ep, data, cfg.eval_config)[0]['pred_mask']
    assert np.array_equal(out['nonempty'], r.nonempty), 'closed-form far-box test vs the Delaunay hull test'
    np.savez_compressed(os.path.join(HERE, 'g14_parse_far.npz'), **out)
    print('nonempty', out['nonempty'].sum(1), 'bytes', os.path.getsize(os.path.join(HERE, 'g14_parse_far.npz')))


if __name__ == '__main__':
    mm.import_reference()
    main()
