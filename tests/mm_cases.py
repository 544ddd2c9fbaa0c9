"""Shared inputs of the device multi-modal evaluation tests (test_mm_device_cpu.py, test_mm_device_gpu.py): G11's dump
records scattered into the dense (hypothesis, sample, proposal) form the kernels take, a dense NumPy restatement of
`multi_modal_eval.tmd` written from the host functions, and the edge-shape cases.  NumPy only, computed once."""
import functools
import os

import numpy as np

G11 = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'g11_multimodal.npz'))


def g11_records():
    """-> [run][sample] dump records {'obbs', 'cls', 'inst_idx'} as the reference wrote them"""
    runs = sorted({int(k.split('_')[2]) for k in G11.files if k.startswith('b_obbs_')})
    samples = sorted({int(k.split('_')[3]) for k in G11.files if k.startswith('b_obbs_')})
    return [[{'obbs': G11[f'b_obbs_{r}_{s}'], 'cls': G11[f'b_cls_{r}_{s}'], 'inst_idx': G11[f'b_inst_{r}_{s}']}
             for s in samples] for r in runs]


def records_dense(records):
    """[h][sample] records -> obbs (H,S,K,7) f64, keep (H,S,K) u8, cls (H,S,K) i64; slots outside a record are zero"""
    H, S, K = len(records), len(records[0]), len(records[0][0]['inst_idx'])
    obbs, keep, cls = np.zeros((H, S, K, 7)), np.zeros((H, S, K), np.uint8), np.zeros((H, S, K), np.int64)
    for h, recs in enumerate(records):
        for s, rec in enumerate(recs):
            inst = np.asarray(rec['inst_idx'], dtype=bool)
            obbs[h, s, inst] = rec['obbs']
            cls[h, s, inst] = rec['cls']
            keep[h, s] = inst
    return obbs, keep, cls


@functools.lru_cache(maxsize=None)
def g11_dense():
    """G11's records as dense (H=10, S=5, K=24) arrays"""
    out = records_dense(g11_records())
    assert out[1].shape == (10, 5, 24)
    return out


def tmd_dense(obbs, keep, cls):
    """obbs (H,B,K,7), keep (H,B,K), cls (H,B,K) -> (value (B,K) f64, count (B,K) i32): per (sample, proposal) the
    number of hypotheses that kept it and the value `multi_modal_eval.tmd` averages, over them in ascending h; 0 where
    none did.  tmd(records) == value.sum() / (count > 0).sum()."""
    from pose2room_amd.net_utils.multi_modal_eval import _entropy2, params_to_corners
    H, B, K = keep.shape
    value, count = np.zeros((B, K)), np.zeros((B, K), np.int32)
    for b in range(B):
        for k in range(K):
            hs = np.nonzero(keep[:, b, k])[0]
            count[b, k] = len(hs)
            if len(hs):
                boxes = params_to_corners(obbs[hs, b, k])                                           # (n,8,3)
                pair = np.mean(np.linalg.norm(boxes[:, None] - boxes[None], axis=-1), axis=-1)      # (n,n)
                value[b, k] = (_entropy2(cls[hs, b, k]) + 1) * (np.mean(pair.sum(axis=-1)) + 1)
    return value, count


def random_obbs(rng, shape):
    """box parameters like the network's: centre in +-3, size 0.4..2, heading in +-pi"""
    return np.concatenate([rng.uniform(-3, 3, shape + (3,)), rng.uniform(0.4, 2.0, shape + (3,)),
                           rng.uniform(-np.pi, np.pi, shape + (1,))], -1)


EDGE_SHAPES = [(1, 1, 1), (2, 1, 1), (64, 1, 2), (3, 2, 65), (10, 3, 40)]


@functools.lru_cache(maxsize=None)
def edge_case(H, B, K):
    """Random keeps at about 0.6 density and classes from 5, plus constructed cells where the shape has room.
    -> (obbs, keep, cls, value, count, cells): value / count by `tmd_dense`; cells = {name: ((b, k), value that cell
    must have, whether exactly)}."""
    rng = np.random.default_rng(1000 * H + 10 * B + K)
    obbs = random_obbs(rng, (H, B, K))
    keep = (rng.uniform(size=(H, B, K)) < 0.6).astype(np.uint8)
    cls = rng.integers(0, 5, (H, B, K))
    cells = {}
    if (H, B, K) == (1, 1, 1):
        keep[:] = 1
        cells['kept once'] = ((0, 0), 1.0, True)
    if (H, B, K) == (2, 1, 1):
        keep[:] = 0
        cells['kept nowhere'] = ((0, 0), 0.0, True)
    if (H, B, K) == (64, 1, 2):
        keep[:, 0, 0] = 1                                   # 64 distinct classes: entropy 6
        cls[:, 0, 0] = rng.permutation(64) + 100
        obbs[:, 0, 0] = obbs[0, 0, 0]
        cells['64 classes'] = ((0, 0), 7.0, False)
        keep[:, 0, 1] = 1                                   # 64 identical boxes of one class
        cls[:, 0, 1] = 3
        obbs[:, 0, 1] = obbs[5, 0, 1]
        cells['identical boxes'] = ((0, 1), 1.0, True)
    if H >= 3 and K >= 40:
        keep[:, 0, 0] = 0
        cells['kept nowhere'] = ((0, 0), 0.0, True)
        keep[:, 0, 1] = 0
        keep[H - 1, 0, 1] = 1
        cells['kept once'] = ((0, 1), 1.0, True)
        keep[:, 0, 2] = 1
        cls[:, 0, 2] = 2
        obbs[:, 0, 2] = obbs[0, 0, 2]
        cells['identical boxes'] = ((0, 2), 1.0, True)
    if H >= 10 and B >= 2:
        keep[:, 1, 3] = 0                                   # classes [0,0,1,2] on identical boxes: entropy 1.5
        keep[[1, 4, 6, 9], 1, 3] = 1
        cls[[1, 4, 6, 9], 1, 3] = [0, 0, 1, 2]
        obbs[:, 1, 3] = obbs[1, 1, 3]
        cells['classes 0 0 1 2'] = ((1, 3), 2.5, False)
    value, count = tmd_dense(obbs, keep, cls)
    for name, ((b, k), want, exact) in cells.items():      # the restatement itself on the constructed cells
        assert (value[b, k] == want) if exact else abs(value[b, k] - want) < 1e-12, (name, value[b, k])
    return obbs, keep, cls, value, count, cells
