/*
 * simpleicp_hip_global.h -- companion C ABI of libsimpleicp_hip.so: the two steps of a global registration that follow the
 * descriptors (simpleicp_hip_fpfh.h): the nearest descriptor of every query row, and poses from triples of matches scored by
 * their inliers.
 *
 * This header includes simpleicp_hip.h and does not change it: SICP_ABI_VERSION stays what it is, these entries have
 * SICP_GLOBAL_VERSION of their own.  The conventions of simpleicp_hip.h hold.  Neither entry touches a cloud slot: the ctx gives
 * its stream and its scratch.  Both run on the ctx's stream and are complete on return; every array pointer is host or device
 * memory (told apart as sicp_fpfh tells its pointers apart).  No floating-point atomic takes part; the results do not depend on
 * grid shape or launch order.
 *
 * ---- contract (M), sicp_feature_match ----
 * query (nq, dim), target (nt, dim): row-major float32; 1 <= dim <= SICP_MATCH_MAX_DIM; nq, nt >= 1; nt < 2^31.
 * Everything is float32, every operation rounded on its own (no FMA):
 *   t_b = q[b] - g[b],  p_b = t_b * t_b,  d2 = ((p_0 + p_1) + p_2) + ... + p_{dim-1}     (from p_0, in column order)
 * idx_out[i] is the target row j with the smallest (d2, j) among the rows whose d2 < +inf: ties go to the lowest index, a NaN or
 * infinite d2 never wins.  No such row: idx_out[i] = -1, d2_out[i] = +inf (n_unmatched counts these queries).
 *
 * ---- contract (R), sicp_ransac_triplets ----
 * src, dst (m, 3) float64: row c of src is matched to row c of dst.  triples (h, 3) int32, drawn by the caller (the library holds
 * no random generator).  3 <= m < 2^31, h >= 1, max_distance finite and > 0, 0 <= edge_ratio <= 1.
 * Everything is float64, every operation rounded on its own; dot products are (a*b + c*d) + e*f; cross products as in contract (F)
 * (component x of a x b: a.y*b.z - a.z*b.y, and cyclic); no libm call takes part except sqrt and division.
 * A hypothesis (i0, i1, i2) with source points p0, p1, p2 and destination points q0, q1, q2, in this order:
 *  1. an index outside 0 .. m-1, or two equal indices: VOID (inliers = -1); nothing is dereferenced.
 *  2. the edge check (Open3D's edge-length checker), settled before the pose: r2 = edge_ratio * edge_ratio; for the pairs
 *     (0,1), (0,2), (1,2): ls2 = |pa - pb|^2, lt2 = |qa - qb|^2, each (dx*dx + dy*dy) + dz*dz.  The hypothesis passes iff
 *     ls2 >= r2 * lt2 and lt2 >= r2 * ls2 for all three pairs; it is PRUNED (inliers = -2) as soon as one pair has
 *     ls2 < r2 * lt2 or lt2 < r2 * ls2.  A NaN compares false in the pruning test: a pair with a NaN length prunes nothing, and
 *     step 4 declares the hypothesis void.
 *  3. the frame of a triangle (a0, a1, a2): u = a1 - a0, e1 = u / sqrt(u.u); v = a2 - a0, s = e1.v, v' = v - s*e1 (one
 *     multiplication and one subtraction per component); e2 = v' / sqrt(v'.v'); e3 = e1 x e2; c = ((a0 + a1) + a2) / 3.0 per
 *     component.
 *  4. the pose, Ep / Eq the frames of the source / destination triangle, cp / cq their centroids:
 *       R[r][k] = (Eq1[r]*Ep1[k] + Eq2[r]*Ep2[k]) + Eq3[r]*Ep3[k],   t[r] = cq[r] - ((R[r][0]*cp.x + R[r][1]*cp.y) + R[r][2]*cp.z)
 *     Any of the twelve numbers not finite: VOID (-1) -- coincident points, collinear points (v' == 0), non-finite coordinates.
 *     This is a minimal solver, exact for congruent triangles, not a least-squares fit.
 *  5. inliers = the number of rows c in 0 .. m-1 with d2 < max_distance * max_distance (one rounded multiplication, strict, a NaN
 *     fails), y = R p_c + t by contract (T) (fma(R02,z, fma(R01,y, R00*x)) + t0, ...), d2 between y and dst[c] by contract (D)
 *     (fma(dz,dz, fma(dy,dy, dx*dx))).  An exact integer.
 * poses_out row: R row-major, then t; all +0.0 for a void or pruned hypothesis.
 * best: the lowest index among the hypotheses with the largest inliers >= 0; best = -1, best_inliers = -1 if there is none.
 *
 * Refused with SICP_ERR_INVALID before any device work, the message naming the argument: a NULL ctx, a NULL required pointer, a
 * size, dim, max_distance or edge_ratio out of range, a ctx with an exchange or an active communicator.
 *
 * Scratch (8 bytes per query; the staged copy of whatever array is host memory) stays with the ctx and goes with
 * sicp_ctx_destroy.  SICP_MATCH_CHUNK (read at sicp_ctx_create): target rows per chunk of the grid's second dimension (tests).
 */
#ifndef SIMPLEICP_HIP_GLOBAL_H
#define SIMPLEICP_HIP_GLOBAL_H

#include "simpleicp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: sicp_feature_match, sicp_ransac_triplets. */
#define SICP_GLOBAL_VERSION 1

/* Widest descriptor sicp_feature_match takes (FPFH: 33). */
#define SICP_MATCH_MAX_DIM 64

int sicp_global_version(void);

/* n_unmatched: queries without a target row of finite distance */
typedef struct sicp_match_stats { int64_t n_query, n_target, n_unmatched; } sicp_match_stats;

/* idx_out: (nq) int32; d2_out (nullable): (nq) float32; *out: the record (host). */
int sicp_feature_match(sicp_ctx *ctx, const float *query, int64_t nq, const float *target, int64_t nt, int dim,
                       int32_t *idx_out, float *d2_out, sicp_match_stats *out);

typedef struct sicp_ransac_stats { int64_t n_hypotheses, n_void, n_pruned, best, best_inliers; } sicp_ransac_stats;

/* poses_out (nullable): (h, 12) float64; inliers_out: (h) int32; *out: the record (host). */
int sicp_ransac_triplets(sicp_ctx *ctx, const double *src, const double *dst, int64_t m, const int32_t *triples, int64_t h,
                         double max_distance, double edge_ratio, double *poses_out, int32_t *inliers_out, sicp_ransac_stats *out);

#ifdef __cplusplus
}
#endif

#endif
