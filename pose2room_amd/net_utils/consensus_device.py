"""The consensus scene of H hypotheses: greedy-leader clustering of oriented boxes, on the device.

`P2RNet.predict_scenes(num_hypotheses=H)` returns H scenes per sample in one `SceneBatch`.  This module merges them into
one: which objects the hypotheses agree on, in how many of them each appears (`support`), and how far apart they put it
(`center_rms`, `iou_mean`).  The reference has no counterpart -- its `multi_modal_eval.tmd` groups boxes by proposal
index, which measures diversity and gives no scene; after a per-hypothesis NMS the same object is carried by different
proposal indices in different hypotheses, so the grouping here is geometric.

`consensus_reference` is the DEFINITION (NumPy, float64, written from the rules below, not from the kernels);
`consensus_clusters` is the device path (csrc/consensus.hip, include/p2r_consensus.h: two launches for the whole batch,
no copy to the host); `ConsensusBatch` is what `SceneBatch.consensus` and `P2RNet.predict_consensus` return.  No CPU
fallback: a missing library is an error.

The rules, for the node tensors of N = H * B samples, hypothesis-major (n = h * B + b):
  pool   of sample b: every item (h, s) with s < count[h * B + b] (a count outside 0..K is clamped); the pool index p
         ascends by (h, s).
  order  item i precedes item j iff score_i > score_j (float32), or the scores are equal and p_i < p_j; a NaN score
         counts as -inf.  (Not nms3d's "higher index first on ties".)
  link   L(i, j) iff (not class_aware or cls_i == cls_j) and box3d_iou(params_to_corners(obb_i),
         params_to_corners(obb_j)) > iou_thresh, the item that precedes as the first argument.  A NaN IoU never links.
  greedy walking the items in order, an item is a leader iff no earlier leader links to it, otherwise a member of the
         EARLIEST leader that links to it.  Links are not transitive: A~B, B~C, not A~C, A first -> {A, B} and {C}.
         Cluster c of a sample is its c-th leader in order.
Mean size and mean heading are deliberately absent: boxes at theta and theta + pi, or at theta + pi / 2 with swapped
sizes, are the same solid, so an average of those parameters is not defined.  The leader's box is the representative.
"""
import collections

import numpy as np
import torch

from .. import _lib
from . import scene_device
from .scene_device import _on_gpu, _want

MAX_H, MAX_K, MAX_POOL = 64, 1024, 2048        # P2R_CONSENSUS_MAX_H / _K / _POOL of include/p2r_consensus.h

_library = _lib.extension("consensus")
HEADER_PATH, LIB_PATH = _library.header_path, _library.lib_path
lib = _library.lib

# capacity Mc = H * K per sample; unused slots are zero, -1 for leader_node; cluster_of is (N,K), -1 from count on
Consensus = collections.namedtuple(
    'Consensus', 'n_clusters leader_node members support hyp_mask box cls score score_mean center_mean center_rms '
                 'iou_mean cluster_of')


def _output_specs(H, B, K):
    Mc = H * K
    return (('n_clusters', (B,), torch.int32), ('leader_node', (B, Mc), torch.int32), ('members', (B, Mc), torch.int32),
            ('support', (B, Mc), torch.int32), ('hyp_mask', (B, Mc), torch.int64), ('box', (B, Mc, 7), torch.float64),
            ('cls', (B, Mc), torch.int64), ('score', (B, Mc), torch.float32), ('score_mean', (B, Mc), torch.float64),
            ('center_mean', (B, Mc, 3), torch.float64), ('center_rms', (B, Mc), torch.float64),
            ('iou_mean', (B, Mc), torch.float64), ('cluster_of', (H * B, K), torch.int32))


def consensus_clusters(count, node_obbs, node_cls, node_score, H, iou_thresh=0.25, class_aware=True):
    """count (N) i32, node_obbs (N,K,7) f64, node_cls (N,K) i64, node_score (N,K) f32 as `scene_nodes` returns them, on
    one GPU, N = H * B hypothesis-major -> Consensus of device tensors (the rules of the module docstring).  Two
    launches, no synchronisation."""
    what = "consensus_clusters"
    if not torch.is_tensor(node_obbs) or node_obbs.dim() != 3 or node_obbs.shape[-1] != 7:
        raise ValueError(f"{what}: node_obbs must be (N,K,7)")
    N, K = node_obbs.shape[:2]
    H = int(H)
    if not 1 <= H <= MAX_H or N % H != 0:
        raise ValueError(f"{what}: {N} samples are no stack of {H} hypotheses (1..{MAX_H})")
    if K > MAX_K or H * K > MAX_POOL or N * K > 0x7fffffff:
        raise ValueError(f"{what}: at most {MAX_K} nodes per sample, {MAX_POOL} per pool and 2^31-1 in all, got N={N}, "
                         f"K={K}, H={H}")
    iou_thresh = float(iou_thresh)
    if not iou_thresh >= 0.0:
        raise ValueError(f"{what}: iou_thresh must be >= 0, got {iou_thresh}")
    _want(what, "count", count, torch.int32, (N,))
    _want(what, "node_obbs", node_obbs, torch.float64, (N, K, 7))
    _want(what, "node_cls", node_cls, torch.int64, (N, K))
    _want(what, "node_score", node_score, torch.float32, (N, K))
    count, node_obbs, node_cls, node_score = _on_gpu(what, count=count, node_obbs=node_obbs, node_cls=node_cls,
                                                     node_score=node_score)
    dev, B = count.device, N // H
    need = int(lib().p2r_consensus_workspace_bytes(H, B, K))
    out = [torch.empty(shape, dtype=dtype, device=dev) for _, shape, dtype in _output_specs(H, B, K)]
    workspace = torch.empty((need // 8,), dtype=torch.int64, device=dev)
    _library.launch("p2r_consensus", dev, H, B, K, count, node_obbs, node_cls, node_score, iou_thresh,
                    int(bool(class_aware)), *out, workspace, need)
    # the workspace goes back to the caching allocator here; the allocator hands it out again only to work enqueued on
    # this stream, behind the two launches
    return Consensus(*out)


# ---- the definition ----------------------------------------------------------------------------------------------------
def _pair_iou(corners, first, second, chunk=1 << 16):
    """box3d_iou(corners[first[k]], corners[second[k]])[0] for every k, in chunks (the same per-pair function)"""
    from .box_util import box3d_iou_pairs
    out = np.zeros(len(first))
    for a in range(0, len(first), chunk):
        c1, c2 = torch.from_numpy(corners[first[a:a + chunk]]), torch.from_numpy(corners[second[a:a + chunk]])
        out[a:a + chunk] = box3d_iou_pairs(c1, c2)[0].numpy()
    return out


def consensus_reference(count, node_obbs, node_cls, node_score, H, iou_thresh=0.25, class_aware=True, *,
                        linkage='leader', strict=True, tie='low', assign='earliest', support='hypotheses',
                        return_iou=False):
    """The definition, on host arrays: count (N) i32, node_obbs (N,K,7) f64, node_cls (N,K) i64, node_score (N,K) f32
    -> Consensus of ndarrays (with return_iou: and per sample the pool's (m,m) IoU matrix, NaN where the class test
    fails, and the pool's (h, s) list).
    The keyword-only switches turn it into a WRONG definition, for the tests of the comparison functions:
    linkage='single' (transitive closure), strict=False (>= for >), tie='high' (the higher index first on equal scores),
    assign='best' (a member goes to the leader with the highest IoU), support='members'."""
    from .multi_modal_eval import params_to_corners
    count, node_obbs = np.asarray(count), np.asarray(node_obbs)
    node_cls, node_score = np.asarray(node_cls), np.asarray(node_score)
    assert node_obbs.dtype == np.float64 and node_score.dtype == np.float32 and node_cls.dtype == np.int64
    N, K = node_cls.shape
    H = int(H)
    assert H >= 1 and N % H == 0 and float(iou_thresh) >= 0.0
    B, Mc = N // H, H * K
    out = Consensus(np.zeros(B, np.int32), np.full((B, Mc), -1, np.int32), np.zeros((B, Mc), np.int32),
                    np.zeros((B, Mc), np.int32), np.zeros((B, Mc), np.int64), np.zeros((B, Mc, 7)),
                    np.zeros((B, Mc), np.int64), np.zeros((B, Mc), np.float32), np.zeros((B, Mc)), np.zeros((B, Mc, 3)),
                    np.zeros((B, Mc)), np.zeros((B, Mc)), np.full((N, K), -1, np.int32))
    extras = []
    for b in range(B):
        pool = [(h, s) for h in range(H) for s in range(min(max(int(count[h * B + b]), 0), K))]
        m = len(pool)
        hs = np.array(pool, np.int64).reshape(m, 2)
        n_of = hs[:, 0] * B + b
        obb, cl, raw = node_obbs[n_of, hs[:, 1]], node_cls[n_of, hs[:, 1]], node_score[n_of, hs[:, 1]]
        sc = np.where(np.isnan(raw), np.float32(-np.inf), raw).astype(np.float32)
        p = np.arange(m)
        order = np.lexsort((p if tie == 'low' else -p, -sc.astype(np.float64)))      # float32 -> float64 keeps the order
        rank = np.empty(m, np.int64)
        rank[order] = p
        # the IoU of every pair that passes the class test, the item that precedes as the first argument
        i, j = np.triu_indices(m, 1)
        if class_aware:
            same = cl[i] == cl[j]
            i, j = i[same], j[same]
        first, second = np.where(rank[i] < rank[j], i, j), np.where(rank[i] < rank[j], j, i)
        iou = np.full((m, m), np.nan)
        if len(i):
            v = _pair_iou(params_to_corners(obb), first, second)
            iou[i, j] = iou[j, i] = v
        with np.errstate(invalid='ignore'):
            link = (iou > iou_thresh) if strict else (iou >= iou_thresh)                  # NaN: False
        extras.append((iou, pool))
        # the walk
        cluster = np.full(m, -1, np.int64)
        leaders = []
        if linkage == 'single':
            for a in order:                                  # the first item of a connected component leads all of it
                if cluster[a] >= 0:
                    continue
                leaders.append(a)
                stack = [a]
                while stack:
                    u = stack.pop()
                    if cluster[u] >= 0:
                        continue
                    cluster[u] = len(leaders) - 1
                    stack.extend(np.nonzero(link[u] & (cluster < 0))[0].tolist())
        else:
            for a in order:
                hit = np.nonzero(link[np.array(leaders, np.int64), a])[0] if leaders else []
                if len(hit) == 0:
                    leaders.append(a)
                    cluster[a] = len(leaders) - 1
                elif assign == 'earliest':
                    cluster[a] = hit[0]
                else:
                    cluster[a] = hit[int(np.argmax(iou[np.array(leaders)[hit], a]))]
        # the statistics, every sum over the members in ascending pool index
        out.n_clusters[b] = len(leaders)
        hyp = np.zeros(Mc, np.uint64)
        for c, L in enumerate(leaders):
            mem = np.nonzero(cluster == c)[0]
            n = len(mem)
            out.leader_node[b, c] = hs[L, 0] * K + hs[L, 1]
            out.members[b, c] = n
            hset = sorted(set(hs[mem, 0].tolist()))
            out.support[b, c] = len(hset) if support == 'hypotheses' else n
            for h in hset:
                hyp[c] |= np.uint64(1) << np.uint64(h)
            out.box[b, c], out.cls[b, c], out.score[b, c] = obb[L], cl[L], raw[L]
            ssum, csum, isum = 0.0, np.zeros(3), 0.0
            for q in mem:
                ssum = ssum + float(raw[q])
                csum = csum + obb[q, 0:3]
                if q != L:
                    isum = isum + iou[L, q]
            mean = csum / n
            dsum = 0.0
            for q in mem:
                d = obb[q, 0:3] - mean
                dsum = dsum + ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            out.score_mean[b, c], out.center_mean[b, c] = ssum / n, mean
            out.center_rms[b, c] = np.sqrt(dsum / n)
            out.iou_mean[b, c] = isum / (n - 1) if n > 1 else 0.0
        out.hyp_mask[b] = hyp.view(np.int64)
        out.cluster_of[n_of, hs[:, 1]] = cluster
    return (out, extras) if return_iou else out


# ---- the batch ---------------------------------------------------------------------------------------------------------
class ConsensusBatch(object):
    """The consensus scenes of the B samples of a `SceneBatch` of H hypotheses (`.scenes`), on the device: the tensors of
    `Consensus` as attributes.  Nothing is copied to the host before `host`, `nodes` or `records` is called; `host`
    copies everything once (the SceneBatch's tensors in the same crossing) and caches."""

    _FIELDS = Consensus._fields

    def __init__(self, scenes, clusters, iou_thresh=0.25, class_aware=True):
        self.scenes = scenes
        self.H, self.B, self.K = scenes.H, scenes.B, scenes.K
        self.iou_thresh, self.class_aware = float(iou_thresh), bool(class_aware)
        for name, t in zip(self._FIELDS, clusters):
            setattr(self, name, t)
        if tuple(self.n_clusters.shape) != (self.B,) or tuple(self.leader_node.shape) != (self.B, self.H * self.K):
            raise ValueError(f"ConsensusBatch: n_clusters ({self.B},) and leader_node ({self.B},{self.H * self.K}) "
                             f"expected, got {tuple(self.n_clusters.shape)} and {tuple(self.leader_node.shape)}")
        self._host_arrays = None

    def __len__(self):
        return self.B

    def clusters(self):
        """-> Consensus of the device tensors"""
        return Consensus(*[getattr(self, f) for f in self._FIELDS])

    def host(self):
        """-> {field: ndarray} of the consensus tensors (one synchronisation, cached; the SceneBatch's host arrays are
        filled by the same crossing)"""
        if self._host_arrays is None:
            from .ap_helper import _to_host
            sb = self.scenes
            mine = [getattr(self, f) for f in self._FIELDS]
            theirs = [] if sb._host_arrays is not None else [f for f in sb._FIELDS if getattr(sb, f) is not None]
            arrays = _to_host(mine + [getattr(sb, f) for f in theirs])
            if sb._host_arrays is None:
                sb._host_arrays = dict(zip(theirs, arrays[len(mine):]))
            self._host_arrays = dict(zip(self._FIELDS, arrays[:len(mine)]))
        return self._host_arrays

    def _selected(self, z, b, min_support):
        """the clusters of sample b with support >= min_support: by support descending, then cluster index"""
        if not 0 <= b < self.B:
            raise IndexError(f"ConsensusBatch: sample {b} outside {self.B}")
        n = int(z['n_clusters'][b])
        sup = z['support'][b, :n]
        keep = np.nonzero(sup >= min_support)[0]
        return keep[np.argsort(-sup[keep].astype(np.int64), kind='stable')]

    def nodes(self, b, min_support=1):
        """-> the `object_node` dicts of the consensus scene of sample b, as `SceneBatch.nodes` builds them for the
        leaders (with the leader's contact fields where the SceneBatch computed them), each also with 'cluster',
        'support', 'support_frac' = support / H, 'members', 'hypotheses' (a list of h), 'score_mean', 'center_mean' (3,),
        'center_rms' and 'iou_mean'; the clusters with support >= min_support, by support descending, then cluster
        index."""
        z = self.host()
        per_h = {}
        out = []
        for c in self._selected(z, b, min_support):
            h, s = divmod(int(z['leader_node'][b, c]), self.K)
            if h not in per_h:
                per_h[h] = self.scenes.nodes(self.scenes.sample(b, h))
            node = dict(per_h[h][s])
            mask = int(z['hyp_mask'][b, c]) & 0xFFFFFFFFFFFFFFFF
            node.update(cluster=int(c), support=int(z['support'][b, c]), support_frac=int(z['support'][b, c]) / self.H,
                        members=int(z['members'][b, c]), hypotheses=[k for k in range(self.H) if (mask >> k) & 1],
                        score_mean=float(z['score_mean'][b, c]), center_mean=z['center_mean'][b, c].copy(),
                        center_rms=float(z['center_rms'][b, c]), iou_mean=float(z['iou_mean'][b, c]))
            out.append(node)
        return out

    def records(self, min_support=1):
        """-> the layout of `multi_modal_eval.confident_boxes`, one record per sample of the batch: {'obbs' (M,7) f64,
        'cls' (M,) i64, 'inst_idx' (K,) bool} of the leaders with support >= min_support in the order of `nodes`;
        inst_idx marks the proposal indices of those leaders."""
        z = self.host()
        sz = self.scenes.host()
        out = []
        for b in range(self.B):
            sel = self._selected(z, b, min_support)
            keep = np.zeros(self.K, dtype=bool)
            for c in sel:
                h, s = divmod(int(z['leader_node'][b, c]), self.K)
                keep[sz['inst_idx'][h * self.B + b, s]] = True
            out.append({'obbs': np.array(z['box'][b, sel], dtype=np.float64).reshape(len(sel), 7),
                        'cls': np.array(z['cls'][b, sel]), 'inst_idx': keep})
        return out


def consensus_of(scenes, iou_thresh=0.25, class_aware=True):
    """SceneBatch -> ConsensusBatch (what `SceneBatch.consensus` calls)"""
    if not isinstance(scenes, scene_device.SceneBatch):
        raise TypeError(f"consensus_of: a SceneBatch expected, got {type(scenes).__name__}")
    clusters = consensus_clusters(scenes.count, scenes.node_obbs, scenes.node_cls, scenes.node_score, scenes.H,
                                  iou_thresh, class_aware)
    return ConsensusBatch(scenes, clusters, iou_thresh, class_aware)
