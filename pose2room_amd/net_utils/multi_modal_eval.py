"""Multi-modal evaluation: confident-box records, best-of-N mAP and TMD (host side, NumPy).

Restates what the reference does around its multi-mode test runs:
  * `confident_boxes`: the per-sample dump record of models/p2rnet/testing.py:77-134 -- box parameters by
    corners2params + rot2head (net_utils/box_util.py:174-204, utils/pc_utils.py:34-47) of every proposal's corners,
    kept where objectness > dump_threshold and the NMS mask is 1: {obbs (M,7), cls (M,), inst_idx (K,) bool}.
  * `tmd`: utils/eval/multi_modal_eval.py's diversity over runs -- per proposal index kept in any run, corners
    rebuilt from the record (head2rot, diag(size / 2) . R, utils/tools.py:33-51 corner order),
    TMD = (class entropy, base 2, + 1) x (mean over runs of the summed mean-corner distances to every run + 1),
    averaged over every (sample, proposal).
  * `best_of_n_map`: the same script's max over runs of each IoU threshold's mAP.
"""
import numpy as np

# get_box_corners (utils/tools.py:33-51): signs of (v0, v1, v2) for corners 0..7
_CORNER_SIGNS = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1],
                          [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], dtype=np.float64)


def corners_to_params(corners):
    """corners (M, 8, 3) -> (M, 7) = centre, size, heading: box axes from the edges 0-1, 1-2, 0-4, made right-handed
    with the second axis pointing up, heading = atan2(-R[0, 2], R[0, 0])."""
    c = np.asarray(corners, dtype=np.float64).reshape(-1, 8, 3)
    center = (c.max(axis=1) + c.min(axis=1)) / 2.
    vectors = np.stack([(c[:, 1] - c[:, 0]) / 2., (c[:, 2] - c[:, 1]) / 2., (c[:, 4] - c[:, 0]) / 2.], axis=1)
    size = np.linalg.norm(vectors, axis=2) * 2
    R = (1 / (size / 2))[:, :, None] * vectors
    R[R[:, 1, 1] < 0, 1] *= -1
    flip = np.einsum('ij,ij->i', np.cross(R[:, 0], R[:, 1]), R[:, 2]) < 0
    R[flip, 2] *= -1
    heading = np.arctan2(-R[:, 0, 2], R[:, 0, 0])
    return np.hstack([center, size, heading[:, None]])


def params_to_corners(obbs):
    """(M, 7) centre, size, heading -> corners (M, 8, 3) in the get_box_corners order (R rows: (cos, 0, -sin),
    (0, 1, 0), (sin, 0, cos))."""
    obbs = np.asarray(obbs, dtype=np.float64).reshape(-1, 7)
    h = obbs[:, 6]
    R = np.zeros((len(obbs), 3, 3))
    R[:, 0, 0], R[:, 0, 2], R[:, 1, 1], R[:, 2, 0], R[:, 2, 2] = np.cos(h), -np.sin(h), 1, np.sin(h), np.cos(h)
    vectors = (obbs[:, 3:6] / 2.)[:, :, None] * R
    out = obbs[:, None, 0:3].repeat(8, axis=1)
    for k in range(3):
        out = out + _CORNER_SIGNS[None, :, k, None] * vectors[:, None, k, :]
    return out


def confident_boxes(end_points, eval_dict, parsed, dump_threshold):
    """One generation's (`generate` / one hypothesis of `generate_hypotheses`) dump records, one per sample:
    {'obbs' (M, 7) f64, 'cls' (M,) int64, 'inst_idx' (K,) bool}.  A sample without a box over the threshold gets a
    record without instances (the reference writes no file for it)."""
    corners = parsed['pred_corners_3d']
    obj = parsed['obj_prob']
    cls = parsed['pred_sem_cls']
    mask = eval_dict['pred_mask']
    out = []
    for b in range(corners.shape[0]):
        params = corners_to_params(corners[b])
        keep = np.logical_and(obj[b] > dump_threshold, mask[b] == 1)
        out.append({'obbs': params[keep, :], 'cls': np.asarray(cls[b])[keep], 'inst_idx': keep})
    return out


def _entropy2(labels):
    _, freq = np.unique(np.asarray(labels), return_counts=True)
    p = freq / freq.sum()
    return float(-(p * np.log(p)).sum() / np.log(2))


def tmd(records_per_hypothesis):
    """records_per_hypothesis[h][sample] = dump record of hypothesis (run) h -> mean TMD over every (sample, proposal
    index) kept in at least one hypothesis."""
    stats = {}
    for records in records_per_hypothesis:
        for si, rec in enumerate(records):
            inst = np.nonzero(np.asarray(rec['inst_idx']))[0]
            corners = params_to_corners(rec['obbs'])
            for j, k in enumerate(inst):
                st = stats.setdefault((si, int(k)), {'box3d': [], 'cls': []})
                st['box3d'].append(corners[j])
                st['cls'].append(rec['cls'][j])
    vals = []
    for st in stats.values():
        boxes = np.array(st['box3d'])                                           # (N, 8, 3)
        pair = np.mean(np.linalg.norm(boxes[:, None] - boxes[None], axis=-1), axis=-1)    # (N, N)
        vals.append((_entropy2(st['cls']) + 1) * (np.mean(pair.sum(axis=-1)) + 1))
    return float(np.mean(vals))


def best_of_n_map(ap_results):
    """ap_results[h] = the mAP of each IoU threshold of hypothesis h (numbers, or metric dicts with 'mAP')
    -> (T,) max over hypotheses."""
    rows = [[m['mAP'] if isinstance(m, dict) else m for m in r] for r in ap_results]
    return np.max(np.array(rows, dtype=np.float64), axis=0)
