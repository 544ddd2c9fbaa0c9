/* p2r_consensus.h -- C ABI of libp2r_consensus.so: the consensus scene of H hypotheses on the device (MI355X / gfx950).
 *
 * An extension library next to libp2r_hip.so and its sisters, built from pose2room_amd/csrc/consensus.hip with the same
 * flags (floating-point contraction off).  The other libraries and their headers are unchanged by it.  Conventions are
 * those of p2r_scene.h: all pointers are DEVICE pointers, tensors are contiguous row-major, `stream` is a hipStream_t
 * (NULL = default stream), every function returns P2R_OK (0), a hipError_t code, or P2R_EINVAL for arguments outside its
 * limits -- before it touches the device.  A problem without an output element returns 0 and launches nothing.  No
 * floating-point atomics: two runs give identical bits.  No call synchronises, and no workgroup waits for another.
 * Every loop is bounded by H, K or H * K.  The C side never allocates: the caller passes a workspace.
 *
 * Byte counts are `unsigned long long` where C would say size_t: the binding is derived from this header by a parser that
 * maps no size_t, and on the LP64 hosts this library is built for the two are the same 64-bit type.
 */
#ifndef P2R_CONSENSUS_H
#define P2R_CONSENSUS_H

#include "p2r_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define P2R_CONSENSUS_MAX_H 64        /* hypotheses: one bit each in hyp_mask */
#define P2R_CONSENSUS_MAX_K 1024      /* node slots per sample of a hypothesis (P2R_SCENE_MAX_K) */
#define P2R_CONSENSUS_MAX_POOL 2048   /* H * K: the pooled items of one sample of the batch */

/* Greedy-leader clustering of the oriented boxes that H hypotheses predict for each of B samples.
 *
 * Inputs, the node tensors p2r_scene_nodes writes for N = H * B samples, hypothesis-major (n = h * B + b): count (N)
 * i32, node_obbs (N,K,7) f64 centre, size, heading, node_cls (N,K) i64, node_score (N,K) f32.
 * Pool of sample b: every (h, s) with s < min(max(count[h * B + b], 0), K); the pool index p ascends by (h, s); Mc = H * K
 * is the capacity.  Item i PRECEDES item j iff score_i > score_j in f32, or the scores are equal and p_i < p_j; a NaN
 * score counts as -inf.  Items i, j are LINKED iff (class_aware == 0 or cls_i == cls_j) and IoU > iou_thresh, where IoU
 * is the oriented-box IoU of p2r_obb_iou (the same per-pair code) of the corners rebuilt from the parameters -- R rows
 * (cos h, 0, -sin h), (0, 1, 0), (sin h, 0, cos h), v_k = (size_k / 2) R[k], corner = ((centre + s0 v_0) + s1 v_1) + s2 v_2
 * with the signs of get_box_corners -- with the item that precedes as the subject of the clip.  A NaN IoU never links.
 * Walking the items in order, an item is a LEADER iff no earlier leader is linked to it, otherwise a MEMBER of the
 * earliest leader linked to it (links are not transitive).  Cluster c of a sample is its c-th leader in order.
 *
 * Outputs, every element written by every call, unused slots zero and -1 for indices: n_clusters (B) i32;
 * leader_node (B,Mc) i32 = h * K + s of the leader; members (B,Mc) i32 counted with the leader; support (B,Mc) i32 the
 * number of distinct hypotheses with a member; hyp_mask (B,Mc) i64 with bit h set for each of them; box (B,Mc,7) f64 the
 * leader's row as a bit copy; cls (B,Mc) i64 and score (B,Mc) f32 the leader's values; score_mean (B,Mc) f64;
 * center_mean (B,Mc,3) f64; center_rms (B,Mc) f64 = sqrt(mean over the members of ((dx dx + dy dy) + dz dz)) with d the
 * member's centre minus center_mean (two passes); iou_mean (B,Mc) f64 the mean IoU of the members other than the leader
 * with the leader, 0 for a singleton; cluster_of (N,K) i32 the cluster of every node slot in its sample, -1 for slots
 * from count on.  All sums run over the members in ascending pool index.
 *
 * Two launches for the whole batch.  (1) One wave per 64 x 64 tile of pairs of a sample's pool (upper triangle): the
 * corners of the tile's items, an exact prefilter (another class, or strictly disjoint axis-aligned bounds: IoU 0, never
 * above a threshold >= 0), the surviving pairs compacted by ballots and evaluated one lane per pair; the link bits go to a
 * bit matrix of ceil(Mc / 64) 64-bit words per row in the workspace, each word written by exactly one workgroup.
 * (2) One workgroup per sample: the items ranked by counting, one wave walks the ranks against a `taken` bitset (leader r
 * claims row[r] & ~taken), then all waves evaluate the member-leader IoUs and the per-cluster statistics.
 *
 * workspace: p2r_consensus_workspace_bytes(H, B, K) bytes, 8-byte aligned; its contents before and after are unspecified.
 * Limits: 1 <= H <= P2R_CONSENSUS_MAX_H, B >= 0, 0 <= K <= P2R_CONSENSUS_MAX_K, H * K <= P2R_CONSENSUS_MAX_POOL, B * H * K
 * fits int (the grid of the first launch, B * ceil(H * K / 64)^2 workgroups, is no larger), iou_thresh >= 0 and not NaN,
 * workspace_bytes at least the size above -- P2R_EINVAL otherwise, and for a NULL or misaligned workspace that has bytes
 * and a NULL pointer to a tensor that has elements.
 * B = 0 launches nothing; K = 0 writes n_clusters = 0. */
int p2r_consensus(int H, int B, int K, const int *count, const double *node_obbs, const long long *node_cls,
                  const float *node_score, double iou_thresh, int class_aware, int *n_clusters, int *leader_node,
                  int *members, int *support, long long *hyp_mask, double *box, long long *cls, float *score,
                  double *score_mean, double *center_mean, double *center_rms, double *iou_mean, int *cluster_of,
                  void *workspace, unsigned long long workspace_bytes, void *stream);

/* Host only: the bytes of workspace p2r_consensus needs for these sizes; 0 for sizes outside the limits above and for an
 * empty problem. */
unsigned long long p2r_consensus_workspace_bytes(int H, int B, int K);

#ifdef __cplusplus
}
#endif
#endif /* P2R_CONSENSUS_H */
