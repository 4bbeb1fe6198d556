/*
 * simpleicp_hip_orient.h -- companion C ABI of libsimpleicp_hip.so: normals oriented consistently -- neighbouring normals made
 * to agree along a minimum spanning forest of the k-NN graph, weighted by how parallel they are (Hoppe et al. 1992; Open3D's
 * orient_normals_consistent_tangent_plane, PCL, CloudCompare).  sicp_estimate_normals returns an eigenvector whose sign is
 * arbitrary and the FPFH descriptor depends on the signs (contract (F)); this entry gives every component of the graph one sign.
 *
 * This header includes simpleicp_hip.h and does not change it: SICP_ABI_VERSION stays what it is, these entries have
 * SICP_ORIENT_VERSION of their own.  The conventions of simpleicp_hip.h and simpleicp_hip_fpfh.h hold.  The entry runs on the
 * ctx's stream and is complete on return; `normals`, `normals_out` and `flipped_out` are host memory or memory of the ctx's device
 * (told apart as sicp_select_in_range tells its output); `reference` and *out are host memory.
 *
 * ---- contract (H), sicp_orient ----
 * The slot's cloud of n points, 1 <= n < 2^31; normals (n, 3) float32, upcast exactly; 2 <= k <= SICP_FPFH_MAX_K, k <= n;
 * reference: NULL or three finite doubles; away: 0 (towards the reference) or non-zero (away from it).  Everything is float64,
 * every operation rounded on its own, no fused multiply-add, no libm call.
 *  1. Void points.  Point i is VOID iff a component of its normal is not finite or all three are zero.  A void point has no
 *     edges, is a component of its own and is never flipped.
 *  2. Edges.  {i, j}, i != j, is an EDGE iff j is among ranks 0 .. k-1 of sicp_knn(slot, k) for point i (contracts (D) and (K)),
 *     or i among those of j, and neither is void.  Exact duplicates are ordinary neighbours.  The graph is undirected: an edge
 *     listed from both ends is one edge.
 *  3. Weight.  s_ij = (nx_i * nx_j + ny_i * ny_j) + nz_i * nz_j, c_ij = fabs(s_ij): the dot product of contracts (P) and (N),
 *     symmetric bit for bit.  (float32 components: no product overflows, s_ij is finite.)
 *  4. Order.  Edge e comes before edge f iff c_e > c_f, or c_e == c_f and min(i, j) of e is smaller, or those are equal too and
 *     max(i, j) of e is smaller.  The order is total.
 *  5. Forest.  The minimum spanning forest of the graph under that order: an edge belongs to it iff no path of edges that all
 *     come before it joins its ends.  The order is total, so the forest is unique; no seed and no order of arrival has a say.
 *     A COMPONENT is a tree of the forest, or a void point.
 *  6. Signs.  Along a forest edge, i and j DISAGREE iff s_ij < 0 (-0.0 and +0.0 agree).  The lowest-index point of a component
 *     is its ANCHOR and keeps its sign; every other point is flipped iff the number of disagreeing edges on its forest path to
 *     the anchor is odd.
 *  7. Vote, only with a reference r.  With the normal as step 6 leaves it, t_i = ((r_x - x_i) * nx + (r_y - y_i) * ny) +
 *     (r_z - z_i) * nz (k_fpfh_orient's expression) for every point that is not void.  Per component pos = #{t_i > 0},
 *     neg = #{t_i < 0}.  away == 0: every point of the component is flipped once more iff neg > pos; away != 0: iff pos > neg.
 *     A tie leaves the component as it is.  One bit per component, not per point: a grazing angle is one vote among many.
 *  8. Outputs.  normals_out[i] = the input normal, negated (exactly) iff point i is flipped; it may be the very array `normals`.
 *     flipped_out[i] = 1 iff flipped, else 0.
 *  9. The record, all int64.  n_points = n; n_void; n_components (void points included); n_forest_edges = n - n_components;
 *     n_flipped; n_components_voted = the components step 7 flipped; rounds = the rounds of Boruvka's algorithm on the graph that
 *     join anything -- in a round every component takes the first edge (order of step 4) that leaves it, and all components so
 *     linked become one; rounds <= ceil(log2 n).  Like the forest it depends on the graph and the order alone.
 * Every byte of the outputs depends on the inputs alone: integer atomics only, no floating-point atomic takes part.
 *
 * Refused with SICP_ERR_INVALID before any device work, the message naming the argument, the outputs untouched: a NULL ctx,
 * normals, normals_out or out (reference and flipped_out are nullable); a slot that is no slot, is empty or holds a shard; k < 2,
 * k > SICP_FPFH_MAX_K or k > n; a reference that is not finite; a ctx with an exchange or an active communicator; 2^31 points or
 * more.
 *
 * Working memory, 4 k + 37 bytes per point -- the lists as an (k, n) int32 table, the normals, two words of union state and two
 * 8-byte words of a component's offers, later its votes and anchor, the flipped bytes -- and 12 more where normals_out is host
 * memory; with the k-NN search's own chunk buffers it stays with the ctx, is reused from call to call and goes with
 * sicp_ctx_destroy.  Switch, read at sicp_ctx_create: SICP_ORIENT_CHUNK (points per k-NN search; 0 or unset: chosen per call as
 * sicp_fpfh chooses its own).
 */
#ifndef SIMPLEICP_HIP_ORIENT_H
#define SIMPLEICP_HIP_ORIENT_H

#include "simpleicp_hip.h"
#include "simpleicp_hip_fpfh.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: sicp_orient. */
#define SICP_ORIENT_VERSION 1

int sicp_orient_version(void);

typedef struct sicp_orient_stats {
    int64_t n_points, n_void, n_components, n_forest_edges, n_flipped, n_components_voted, rounds;
} sicp_orient_stats;

/* normals, normals_out: (n, 3) float32; reference (nullable): 3 doubles (host); flipped_out (nullable): (n) uint8; *out: host. */
int sicp_orient(sicp_ctx *ctx, int slot, const float *normals, int k, const double *reference, int away, float *normals_out,
                uint8_t *flipped_out, sicp_orient_stats *out);

#ifdef __cplusplus
}
#endif

#endif
