"""Occupancy maps of predicted scenes, on the device: the scene as a voxel grid, a scene-level IoU, hypothesis votes.

`predict_scenes`, `generate_hypotheses` and `SceneBatch.consensus` all end in lists of boxes.  This module turns the
nodes of a `SceneBatch` into what a planner consumes and what the reference's scene metric scores:

  * the voxels the nodes of every sample cover, bit-packed, optionally with the node that owns each voxel
    (`occupancy_boxes`; on the host this is the reference's `extract_pc_in_box3d`, utils/pc_utils.py:16-31, a Delaunay
    hull test per box over every voxel centre);
  * the voxels the body passed through (`occupancy_body`) -- the only evidence the network sees, and free space;
  * per voxel the number of hypotheses that put something there, and the map of those with `min_votes` or more
    (`occupancy_votes`): an uncertainty map that needs no IoU threshold and no clustering decision;
  * volumes and overlaps (`occupancy_counts`), from which `OccupancyBatch.iou` is the arithmetic of the reference's
    `calculate_scene_iou(..., normalization='none')` (models/eval_metrics.py) and `OccupancyBatch.collision` the share of
    the body's voxels that a scene fills.

`occupancy_reference` is the DEFINITION (NumPy, float64, explicit element-wise operations in the order the kernels use,
no `np.dot` / `@`); the kernels are csrc/occupancy.hip behind include/p2r_occupancy.h.  No CPU fallback: a missing library
is an error.

The rules.  A grid is `origin` (3 doubles), `voxel` (> 0) and `dims` = (nx, ny, nz); the centre of voxel (i, j, k) is
origin[a] + ((double)index_a + 0.5) * voxel per axis.  Dense arrays are (.., nz, ny, nx); bit-packed arrays are
(.., nz, ny, W) int64 words, W = ceil(nx / 64), bit i % 64 of word i // 64 is voxel i, padding bits zero.
  boxes   slot s of sample n counts iff s < min(max(count[n], 0), K).  Node s covers a point p iff, with d = p - centre,
          fabs((d0 * R[a][0] + d1 * R[a][1]) + d2 * R[a][2]) - size[a] / 2.0 <= 0 for a = 0, 1, 2 (the expression of
          `contact_frames`; inclusive).  A node with a non-finite value among its 7 box parameters or 9 matrix entries
          covers nothing.  A voxel is occupied iff a counted node covers its centre; its owner is the covering node that
          precedes the others by `consensus`'s order: higher float32 score first, NaN as -inf, ties to the lower slot.
  body    a joint marks voxel index_a = floor(((double)x_a - origin[a]) / voxel) when all three are inside the grid;
          joints with a non-finite coordinate or an index outside mark nothing.
  votes   for N = H * B samples, hypothesis-major, votes[b, voxel] = the number of hypotheses whose bit is set; the fused
          map has the bit iff votes >= min_votes.
  counts  per sample n with rows n % B of the ground-truth and body maps: vol, vol_gt, inter_gt, vol_body, inter_body.
"""
import collections
import math

import numpy as np
import torch

from .. import _lib
from .scene_device import _on_gpu, _want, _want_joints

MAX_DIM, MAX_K, MAX_H, NODE_CHUNK = 1024, 1024, 64, 128    # P2R_OCC_MAX_DIM / _K / _H / _NODE_CHUNK of the header
MAX_ELEMS = 0x7fffffff
MAX_T = 65535                                              # scene_device.MAX_T: the recordings `contact_frames` takes

_library = _lib.extension("occupancy")
HEADER_PATH, LIB_PATH = _library.header_path, _library.lib_path
lib, _launch = _library.lib, _library.launch

COUNT_FIELDS = ('vol', 'vol_gt', 'inter_gt', 'vol_body', 'inter_body')


# ---- the grid ----------------------------------------------------------------------------------------------------------
class Grid(object):
    """origin (3 finite floats), voxel (finite, > 0), dims = (nx, ny, nz), each 1..1024."""

    def __init__(self, origin, voxel, dims):
        try:
            self.origin = tuple(float(v) for v in origin)
            self.voxel = float(voxel)
            self.dims = tuple(int(v) for v in dims)
            whole = all(int(v) == v for v in dims)
        except (TypeError, ValueError) as e:
            raise ValueError(f"Grid: origin (3 floats), voxel (a float) and dims (3 ints) expected: {e}") from None
        if len(self.origin) != 3 or not all(math.isfinite(v) for v in self.origin):
            raise ValueError(f"Grid: origin must be three finite numbers, got {origin!r}")
        if not (math.isfinite(self.voxel) and self.voxel > 0.0):
            raise ValueError(f"Grid: voxel must be finite and > 0, got {voxel!r}")
        if len(self.dims) != 3 or not whole or not all(1 <= v <= MAX_DIM for v in self.dims):
            raise ValueError(f"Grid: dims must be three integers in 1..{MAX_DIM}, got {dims!r}")

    nx, ny, nz = (property(lambda self, a=a: self.dims[a]) for a in range(3))

    @property
    def W(self):
        return (self.dims[0] + 63) // 64

    @property
    def words(self):
        return self.dims[2] * self.dims[1] * self.W

    @property
    def dense_shape(self):
        return (self.dims[2], self.dims[1], self.dims[0])

    @property
    def packed_shape(self):
        return (self.dims[2], self.dims[1], self.W)

    def centres(self, axis):
        """the float64 centres of the voxels along one axis"""
        return self.origin[axis] + (np.arange(self.dims[axis]).astype(np.float64) + 0.5) * self.voxel

    def __repr__(self):
        return f"Grid(origin={self.origin}, voxel={self.voxel}, dims={self.dims})"

    def __eq__(self, other):
        return isinstance(other, Grid) and (self.origin, self.voxel, self.dims) == (other.origin, other.voxel, other.dims)

    def __hash__(self):
        return hash((self.origin, self.voxel, self.dims))

    @classmethod
    def around(cls, joints, voxel, margin=1.0):
        """The grid of `voxel`-sized cells that holds every finite joint of a batch and `margin` around them, its origin on
        a multiple of `voxel`.  joints (B,T,J,3|4), a tensor on any device or an array.  This reads the joints back to
        the host (one synchronisation): call it once, outside the loop that must not wait."""
        voxel, margin = float(voxel), float(margin)
        if not (math.isfinite(voxel) and voxel > 0.0 and math.isfinite(margin) and margin >= 0.0):
            raise ValueError(f"Grid.around: voxel > 0 and margin >= 0 expected, got {voxel}, {margin}")
        x = joints.detach().cpu().numpy() if torch.is_tensor(joints) else np.asarray(joints)
        if x.ndim < 2 or x.shape[-1] not in (3, 4):
            raise ValueError(f"Grid.around: joints (..., 3|4) expected, got {x.shape}")
        x = x[..., 0:3].reshape(-1, 3).astype(np.float64)
        x = x[np.isfinite(x).all(1)]
        if len(x) == 0:
            raise ValueError("Grid.around: no finite joint")
        lo = np.floor((x.min(0) - margin) / voxel)
        hi = np.ceil((x.max(0) + margin) / voxel)
        dims = np.maximum(hi - lo, 1.0)
        if (dims > MAX_DIM).any():
            raise ValueError(f"Grid.around: {dims.astype(np.int64).tolist()} voxels of {voxel} exceed {MAX_DIM} per axis")
        return cls((lo * voxel).tolist(), voxel, dims.astype(np.int64).tolist())


def _want_grid(what, grid):
    if not isinstance(grid, Grid):
        raise ValueError(f"{what}: grid must be an occupancy_device.Grid, got {type(grid).__name__}")
    return grid


def _want_maps(what, name, t, rows, grid):
    return _want(what, name, t, torch.int64, (rows,) + grid.packed_shape)


# ---- the device path ---------------------------------------------------------------------------------------------------
def occupancy_boxes(count, node_obbs, node_rmat, node_score, grid, owner=False):
    """count (N) i32, node_obbs (N,K,7) f64, node_rmat (N,K,3,3) f64, node_score (N,K) f32 as `scene_nodes` returns
    them, on one GPU -> (occ (N,nz,ny,W) i64 bit-packed, owner (N,nz,ny,nx) i16 or None): the voxels whose centre a
    counted node covers and, with owner=True, the slot of the node that owns each (-1: free).  One launch."""
    what = "occupancy_boxes"
    _want_grid(what, grid)
    if not torch.is_tensor(node_obbs) or node_obbs.dim() != 3 or node_obbs.shape[-1] != 7:
        raise ValueError(f"{what}: node_obbs must be (N,K,7)")
    N, K = node_obbs.shape[:2]
    if K > MAX_K or N * K > MAX_ELEMS or N * grid.words > MAX_ELEMS:
        raise ValueError(f"{what}: at most {MAX_K} nodes per sample, 2^31-1 nodes and 2^31-1 words in all, got N={N}, "
                         f"K={K}, {grid.words} words per map")
    _want(what, "count", count, torch.int32, (N,))
    _want(what, "node_obbs", node_obbs, torch.float64, (N, K, 7))
    _want(what, "node_rmat", node_rmat, torch.float64, (N, K, 3, 3))
    _want(what, "node_score", node_score, torch.float32, (N, K))
    count, node_obbs, node_rmat, node_score = _on_gpu(what, count=count, node_obbs=node_obbs, node_rmat=node_rmat,
                                                      node_score=node_score)
    dev = count.device
    occ = torch.empty((N,) + grid.packed_shape, dtype=torch.int64, device=dev)
    own = torch.empty((N,) + grid.dense_shape, dtype=torch.int16, device=dev) if owner else None
    _launch("p2r_occ_boxes", dev, N, K, count, node_obbs, node_rmat, node_score, *grid.origin, grid.voxel, *grid.dims,
            occ, own)
    return occ, own


def occupancy_body(joints, grid):
    """joints (B,T,J,3|4) f32 on a GPU -> body (B,nz,ny,W) i64 bit-packed: the voxels a joint falls into.  Two launches."""
    what = "occupancy_body"
    _want_grid(what, grid)
    joints = _want_joints(what, joints, MAX_T)
    B, T, J, C = joints.shape
    if B * grid.words > MAX_ELEMS or B * T * J > MAX_ELEMS:
        raise ValueError(f"{what}: 2^31-1 words and joints in all, got B={B}, T={T}, J={J}, {grid.words} words per map")
    joints, = _on_gpu(what, joints=joints)
    body = torch.empty((B,) + grid.packed_shape, dtype=torch.int64, device=joints.device)
    _launch("p2r_occ_body", joints.device, joints, B, T, J, C, *grid.origin, grid.voxel, *grid.dims, body)
    return body


def occupancy_votes(occ, H, grid, min_votes=None, votes=True):
    """occ (H * B,nz,ny,W) i64 on a GPU, hypothesis-major -> (votes (B,nz,ny,nx) u8 or None, fused (B,nz,ny,W) i64): per
    voxel the number of hypotheses with the bit, and the map of the voxels with min_votes (default H // 2 + 1) or more.
    One launch."""
    what = "occupancy_votes"
    _want_grid(what, grid)
    if not torch.is_tensor(occ) or occ.dim() != 4:
        raise ValueError(f"{what}: occ must be (N,nz,ny,W)")
    N, H = occ.shape[0], int(H)
    if not 1 <= H <= MAX_H or N % H != 0:
        raise ValueError(f"{what}: {N} samples are no stack of {H} hypotheses (1..{MAX_H})")
    min_votes = H // 2 + 1 if min_votes is None else int(min_votes)
    if not 1 <= min_votes <= H:
        raise ValueError(f"{what}: min_votes must be in 1..{H}, got {min_votes}")
    if N * grid.words > MAX_ELEMS:
        raise ValueError(f"{what}: 2^31-1 words in all, got {N} maps of {grid.words}")
    _want_maps(what, "occ", occ, N, grid)
    occ, = _on_gpu(what, occ=occ)
    B, dev = N // H, occ.device
    v = torch.empty((B,) + grid.dense_shape, dtype=torch.uint8, device=dev) if votes else None
    fused = torch.empty((B,) + grid.packed_shape, dtype=torch.int64, device=dev)
    _launch("p2r_occ_votes", dev, H, B, *grid.dims, occ, min_votes, v, fused)
    return v, fused


def occupancy_counts(a, grid, gt=None, body=None, B=None):
    """a (N,nz,ny,W) i64; gt, body (B,nz,ny,W) i64 or None, on one GPU; sample n reads row n % B (B defaults to the rows of
    gt or body, else N) -> counts (N,5) i64: vol, vol_gt, inter_gt, vol_body, inter_body (COUNT_FIELDS); the columns of
    a map that is None are 0.  One launch."""
    what = "occupancy_counts"
    _want_grid(what, grid)
    if not torch.is_tensor(a) or a.dim() != 4:
        raise ValueError(f"{what}: a must be (N,nz,ny,W)")
    N = a.shape[0]
    if B is None:
        rows = [t.shape[0] for t in (gt, body) if torch.is_tensor(t) and t.dim()]
        B = rows[0] if rows else N
    B = int(B)
    if B < 0 or (N > 0 and (B < 1 or N % B != 0)):
        raise ValueError(f"{what}: {N} samples over {B} rows: N must be a multiple of B")
    if N * grid.words > MAX_ELEMS:
        raise ValueError(f"{what}: 2^31-1 words in all, got {N} maps of {grid.words}")
    _want_maps(what, "a", a, N, grid)
    maps = dict(a=a)
    if gt is not None:
        maps['gt'] = _want_maps(what, "gt", gt, B, grid)
    if body is not None:
        maps['body'] = _want_maps(what, "body", body, B, grid)
    maps = dict(zip(maps, _on_gpu(what, **maps)))
    dev = maps['a'].device
    counts = torch.empty((N, 5), dtype=torch.int64, device=dev)
    _launch("p2r_occ_counts", dev, N, B, grid.words, maps['a'], maps.get('gt'), maps.get('body'), counts)
    return counts


# ---- bits ----------------------------------------------------------------------------------------------------------------
def pack_bits(dense):
    """bool (..., nx) -> int64 (..., ceil(nx / 64)): bit i % 64 of word i // 64 is element i, padding bits zero"""
    dense = np.asarray(dense).astype(bool)
    nx = dense.shape[-1]
    W = (nx + 63) // 64
    padded = np.zeros(dense.shape[:-1] + (W * 64,), dtype=bool)
    padded[..., :nx] = dense
    bits = padded.reshape(dense.shape[:-1] + (W, 64)).astype(np.uint64)
    words = np.zeros(dense.shape[:-1] + (W,), dtype=np.uint64)
    for k in range(64):
        words |= bits[..., k] << np.uint64(k)
    return words.view(np.int64)


def unpack_bits(words, nx):
    """int64 (..., W) -> bool (..., nx), the inverse of `pack_bits` (the padding bits are dropped unseen)"""
    words = np.ascontiguousarray(words).view(np.uint64)
    W = words.shape[-1]
    assert W == (nx + 63) // 64, (W, nx)
    out = np.zeros(words.shape[:-1] + (W, 64), dtype=bool)
    for k in range(64):
        out[..., k] = (words >> np.uint64(k)) & np.uint64(1)
    return out.reshape(words.shape[:-1] + (W * 64,))[..., :nx]


def popcount(words):
    """the number of set bits of every int64 map (..., nz, ny, W) -> int64 (...)"""
    w = np.ascontiguousarray(words).view(np.uint64)
    n = np.zeros(w.shape, dtype=np.int64)
    for k in range(64):
        n += ((w >> np.uint64(k)) & np.uint64(1)).astype(np.int64)
    return n.reshape(w.shape[:-3] + (-1,)).sum(-1)


def scene_iou(counts):
    """counts (..., 5) -> float32 (...): inter_gt / max(vol + vol_gt - inter_gt, 1e-8) in the reference's float32
    arithmetic (`calculate_scene_iou`: torch.sum(a & b).float() / torch.clamp(torch.sum(a | b).float(), min=1e-8))"""
    c = np.asarray(counts)
    inter = c[..., 2].astype(np.float32)
    union = (c[..., 0] + c[..., 1] - c[..., 2]).astype(np.float32)
    return inter / np.maximum(union, np.float32(1e-8))


def body_collision(counts):
    """counts (..., 5) -> float64 (...): inter_body / max(vol_body, 1), the share of the body's voxels the scene fills"""
    c = np.asarray(counts)
    return c[..., 4].astype(np.float64) / np.maximum(c[..., 3], 1).astype(np.float64)


# ---- the definition ----------------------------------------------------------------------------------------------------
Occupancy = collections.namedtuple('Occupancy', 'occ owner body gt_occ votes fused counts fused_counts')


def reference_boxes(count, node_obbs, node_rmat, node_score, grid, *, strict=False, half_offset=True, transpose=False,
                    full_size=False, clamp_count=True, tie='low'):
    """The box rule on host arrays -> (dense bool (N,nz,ny,nx), owner int16 (N,nz,ny,nx)).
    The keyword-only switches turn it into a WRONG definition, for the tests of the designed cases: strict=True (< for
    <=), half_offset=False (centres without the 0.5), transpose=True (R transposed), full_size=True (size for size / 2),
    clamp_count=False (a count above K runs on into the next sample's slots), tie='high' (equal scores: the higher slot
    owns)."""
    count, node_obbs, node_rmat = np.asarray(count), np.asarray(node_obbs), np.asarray(node_rmat)
    node_score = np.asarray(node_score)
    assert node_obbs.dtype == np.float64 and node_rmat.dtype == np.float64 and node_score.dtype == np.float32
    N, K = node_score.shape
    nx, ny, nz = grid.dims
    off = 0.5 if half_offset else 0.0
    px = (grid.origin[0] + (np.arange(nx).astype(np.float64) + off) * grid.voxel)[None, None, :]
    py = (grid.origin[1] + (np.arange(ny).astype(np.float64) + off) * grid.voxel)[None, :, None]
    pz = (grid.origin[2] + (np.arange(nz).astype(np.float64) + off) * grid.voxel)[:, None, None]
    dense = np.zeros((N, nz, ny, nx), dtype=bool)
    owner = np.full((N, nz, ny, nx), -1, dtype=np.int16)
    flat_obbs, flat_rmat, flat_score = node_obbs.reshape(-1, 7), node_rmat.reshape(-1, 3, 3), node_score.reshape(-1)
    for n in range(N):
        m = max(int(count[n]), 0)
        m = min(m, K) if clamp_count else min(m, (N - n) * K)
        best = np.full((nz, ny, nx), -np.inf, dtype=np.float32)
        for s in range(m):
            obb, R, sc = flat_obbs[n * K + s], flat_rmat[n * K + s], flat_score[n * K + s]
            if not (np.isfinite(obb).all() and np.isfinite(R).all()):
                continue
            if transpose:
                R = R.T
            sc = np.float32(-np.inf) if np.isnan(sc) else np.float32(sc)
            with np.errstate(over='ignore', invalid='ignore'):
                d0, d1, d2 = px - obb[0], py - obb[1], pz - obb[2]
                inside = np.ones((nz, ny, nx), dtype=bool)
                for a in range(3):
                    g = np.abs((d0 * R[a, 0] + d1 * R[a, 1]) + d2 * R[a, 2]) - (obb[3 + a] if full_size else obb[3 + a] / 2.0)
                    inside &= (g < 0.0) if strict else (g <= 0.0)
            first = inside & ~dense[n]
            take = first | (inside & ((sc >= best) if tie == 'high' else (sc > best)))
            owner[n][take] = s
            best[take] = sc
            dense[n] |= inside
    return dense, owner


def reference_body(joints, grid):
    """The body rule: joints (B,T,J,3|4) float32 -> dense bool (B,nz,ny,nx)"""
    joints = np.asarray(joints)
    assert joints.dtype == np.float32 and joints.ndim == 4
    B = joints.shape[0]
    nx, ny, nz = grid.dims
    dense = np.zeros((B, nz, ny, nx), dtype=bool)
    x = joints[..., 0:3].reshape(B, -1, 3).astype(np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        v = np.floor((x - np.array(grid.origin, np.float64)) / grid.voxel)
        ok = (np.isfinite(x) & (v >= 0.0) & (v < np.array(grid.dims, np.float64))).all(-1)
    for b in range(B):
        idx = v[b][ok[b]].astype(np.int64)
        dense[b, idx[:, 2], idx[:, 1], idx[:, 0]] = True
    return dense


def reference_votes(dense, H, min_votes):
    """dense bool (H * B, nz, ny, nx) -> (votes uint8 (B,nz,ny,nx), fused bool (B,nz,ny,nx))"""
    N = dense.shape[0]
    assert N % H == 0 and 1 <= min_votes <= H
    votes = dense.reshape((H, N // H) + dense.shape[1:]).astype(np.int64).sum(0)
    return votes.astype(np.uint8), votes >= min_votes


def reference_counts(dense, gt=None, body=None, B=None):
    """dense bool (N,...); gt, body bool (B,...) or None -> int64 (N,5) (COUNT_FIELDS)"""
    N = dense.shape[0]
    B = (len(gt) if gt is not None else len(body) if body is not None else N) if B is None else B
    out = np.zeros((N, 5), dtype=np.int64)
    for n in range(N):
        out[n, 0] = dense[n].sum()
        if gt is not None:
            out[n, 1], out[n, 2] = gt[n % B].sum(), (dense[n] & gt[n % B]).sum()
        if body is not None:
            out[n, 3], out[n, 4] = body[n % B].sum(), (dense[n] & body[n % B]).sum()
    return out


def occupancy_reference(count, node_obbs, node_rmat, node_score, grid, H=1, joints=None, gt=None, min_votes=None,
                        **switches):
    """The definition of everything `SceneBatch.occupancy` returns, on host arrays: the node arrays of N = H * B samples,
    joints (B,T,J,3|4) float32 or None, gt = the (count, node_obbs, node_rmat, node_score) arrays of B ground-truth samples
    or None -> Occupancy: occ (N,nz,ny,W) int64, owner (N,nz,ny,nx) int16, body / gt_occ (B,nz,ny,W) int64 or None, votes
    (B,nz,ny,nx) uint8, fused (B,nz,ny,W) int64, counts (N,5) and fused_counts (B,5) int64.  `switches`: the wrong
    definitions of `reference_boxes`."""
    dense, owner = reference_boxes(count, node_obbs, node_rmat, node_score, grid, **switches)
    N, H = dense.shape[0], int(H)
    assert H >= 1 and N % H == 0
    B = N // H
    min_votes = H // 2 + 1 if min_votes is None else int(min_votes)
    body = reference_body(joints, grid) if joints is not None else None
    gt_dense = reference_boxes(*gt, grid, **switches)[0] if gt is not None else None
    assert body is None or len(body) == B
    assert gt_dense is None or len(gt_dense) == B
    votes, fused = reference_votes(dense, H, min_votes)
    return Occupancy(pack_bits(dense), owner, None if body is None else pack_bits(body),
                     None if gt_dense is None else pack_bits(gt_dense), votes, pack_bits(fused),
                     reference_counts(dense, gt_dense, body, B), reference_counts(fused, gt_dense, body, B))


# ---- the batch ---------------------------------------------------------------------------------------------------------
class OccupancyBatch(object):
    """The occupancy maps of the N = H * B samples of a `SceneBatch` (`.scenes`) on `.grid`, on the device: the tensors of
    `Occupancy` as attributes (owner, body, gt_occ: None when not asked for; `.gt_scenes` is the ground-truth SceneBatch
    or None).  Nothing is copied to the host before
    `host` or one of the methods below is called; `host` copies everything once and caches."""

    _FIELDS = Occupancy._fields

    def __init__(self, scenes, grid, maps, min_votes, gt_scenes=None):
        self.scenes, self.grid, self.gt_scenes = scenes, _want_grid("OccupancyBatch", grid), gt_scenes
        self.H, self.B, self.min_votes = scenes.H, scenes.B, int(min_votes)
        for name, t in zip(self._FIELDS, maps):
            setattr(self, name, t)
        if tuple(self.occ.shape) != (self.H * self.B,) + grid.packed_shape:
            raise ValueError(f"OccupancyBatch: occ {(self.H * self.B,) + grid.packed_shape} expected, got "
                             f"{tuple(self.occ.shape)}")
        self._host_arrays = None

    def __len__(self):
        return self.H * self.B

    def maps(self):
        """-> Occupancy of the device tensors"""
        return Occupancy(*[getattr(self, f) for f in self._FIELDS])

    def host(self):
        """-> {field: ndarray} of the tensors that are present (one synchronisation, cached)"""
        if self._host_arrays is None:
            from .ap_helper import _to_host
            names = [f for f in self._FIELDS if getattr(self, f) is not None]
            self._host_arrays = dict(zip(names, _to_host([getattr(self, f) for f in names])))
        return self._host_arrays

    def dense(self, n, fused=False):
        """-> the bool volume (nz, ny, nx) of sample n of the stack, or with fused=True of the fused map of sample n of
        the batch"""
        z = self.host()
        rows = z['fused'] if fused else z['occ']
        if not 0 <= n < len(rows):
            raise IndexError(f"OccupancyBatch: sample {n} outside {len(rows)}")
        return unpack_bits(rows[n], self.grid.nx)

    def probability(self, b):
        """-> float64 (nz, ny, nx): per voxel the share of the H hypotheses that occupy it in sample b of the batch"""
        z = self.host()
        if not 0 <= b < self.B:
            raise IndexError(f"OccupancyBatch: sample {b} outside {self.B}")
        return z['votes'][b].astype(np.float64) / self.H

    def iou(self, fused=False):
        """-> float32 (N,), or (B,) for the fused maps: the scene IoU with the ground-truth map of the sample, in the
        arithmetic of the reference's `calculate_scene_iou(..., normalization='none')`"""
        if self.gt_occ is None:
            raise RuntimeError("OccupancyBatch: no ground-truth scenes were given (gt=None)")
        return scene_iou(self.host()['fused_counts' if fused else 'counts'])

    def collision(self, fused=False):
        """-> float64 (N,), or (B,) for the fused maps: the share of the voxels the body passed through that the scene
        fills (compare with the same figure of the ground truth: people sit in sofas)"""
        if self.body is None:
            raise RuntimeError("OccupancyBatch: no joints were given (joints=None)")
        return body_collision(self.host()['fused_counts' if fused else 'counts'])

    def save_npz(self, path, n):
        """Sample n of the stack: occupancy (nz,ny,nx) bool, origin, voxel, and where present owner (nz,ny,nx) int16, the
        body map and the hypothesis share of its sample of the batch."""
        z = self.host()
        out = dict(occupancy=self.dense(n), origin=np.array(self.grid.origin), voxel=np.float64(self.grid.voxel),
                   probability=self.probability(n % self.B))
        if 'owner' in z:
            out['owner'] = z['owner'][n]
        if 'body' in z:
            out['body'] = unpack_bits(z['body'][n % self.B], self.grid.nx)
        np.savez_compressed(path, **out)


def occupancy_of(scenes, grid, joints=None, gt=None, min_votes=None, owner=False):
    """SceneBatch -> OccupancyBatch (what `SceneBatch.occupancy` calls).  joints (B,T,J,3|4) f32 adds the body map, gt (a
    SceneBatch of the B ground-truth scenes, `scenes_from_labels`) the ground-truth map; both enter the counts.  At most
    7 launches -- boxes, ground-truth boxes, body (2), votes, counts of the N maps and of the B fused maps -- and no
    synchronisation."""
    from . import scene_device
    what = "SceneBatch.occupancy"
    if not isinstance(scenes, scene_device.SceneBatch):
        raise TypeError(f"{what}: a SceneBatch expected, got {type(scenes).__name__}")
    _want_grid(what, grid)
    if gt is not None and (not isinstance(gt, scene_device.SceneBatch) or gt.H != 1 or gt.B != scenes.B):
        raise ValueError(f"{what}: gt must be a SceneBatch of the {scenes.B} samples of the batch (one hypothesis)")
    if joints is not None and (not torch.is_tensor(joints) or joints.dim() != 4 or joints.shape[0] != scenes.B):
        raise ValueError(f"{what}: joints must be ({scenes.B},T,J,3|4), one row per sample of the batch")
    H = scenes.H
    min_votes = H // 2 + 1 if min_votes is None else int(min_votes)
    if not 1 <= min_votes <= H:
        raise ValueError(f"{what}: min_votes must be in 1..{H}, got {min_votes}")
    occ, own = occupancy_boxes(scenes.count, scenes.node_obbs, scenes.node_rmat, scenes.node_score, grid, owner=owner)
    gt_occ = occupancy_boxes(gt.count, gt.node_obbs, gt.node_rmat, gt.node_score, grid)[0] if gt is not None else None
    body = occupancy_body(joints, grid) if joints is not None else None
    votes, fused = occupancy_votes(occ, H, grid, min_votes)
    counts = occupancy_counts(occ, grid, gt_occ, body, B=scenes.B)
    fused_counts = occupancy_counts(fused, grid, gt_occ, body, B=scenes.B)
    return OccupancyBatch(scenes, grid, Occupancy(occ, own, body, gt_occ, votes, fused, counts, fused_counts), min_votes,
                          gt_scenes=gt)


def scenes_from_labels(data, cfg=None):
    """The ground-truth scenes of a batch as a SceneBatch of B samples (one hypothesis), by the chain the predictions
    take: the corners `parse_groundtruths` builds from data['center_label'], data['size'], data['heading'] (kept on the
    device here), `mm_device.box_params`, `scene_nodes` with pred_mask = data['box_label_mask'] and an objectness of 1.
    cfg is accepted for symmetry with the prediction path and not read.  Three launches of the project's own and the
    tensor arithmetic of `boxes_to_corners`; nothing crosses to the host."""
    from . import mm_device, scene_device
    from .ap_helper import boxes_to_corners
    center = data['center_label'][:, :, 0:3].detach()
    size = torch.exp(data['size']).detach()
    heading = torch.atan2(data['heading'][..., 0], data['heading'][..., 1]).detach()
    mask = data['box_label_mask'].detach()
    corners = boxes_to_corners(size, heading.to(torch.float64), center)
    corners = (corners * (mask != 0).to(torch.float64)[:, :, None, None]).to(torch.float64)
    B, K = mask.shape
    obbs = mm_device.box_params(corners)
    nodes = scene_device.scene_nodes(obbs, torch.ones((B, K), dtype=torch.float32, device=obbs.device),
                                     (mask != 0).to(torch.uint8), data['sem_cls_label'].detach().to(torch.int64), 0.5)
    return scene_device.SceneBatch(1, B, K, *nodes)
