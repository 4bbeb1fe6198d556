/*
 * simpleicp_hip_keypoints.h -- companion C ABI of libsimpleicp_hip.so: ISS keypoints (Intrinsic Shape Signatures, Zhong 2009),
 * the points a global registration describes and matches instead of the whole cloud.
 *
 * This header includes simpleicp_hip.h and does not change it: SICP_ABI_VERSION stays what it is, this entry has
 * SICP_KEYPOINTS_VERSION of its own.  The conventions of simpleicp_hip.h hold.
 *
 * The rules, arithmetic contract (I) of DESIGN.md section 22.  Everything is float64; every operation named below is rounded
 * on its own (no FMA outside contract (D)'s distances); no libm call takes part except sqrt and division, both correctly
 * rounded; no floating-point atomics; every sum has a fixed order.
 *
 * Inputs: the slot's n points; k_s and k_n (2 <= k <= SICP_KEYPOINT_MAX_K, k <= n); salient_radius and nms_radius (+inf: none;
 * otherwise finite and > 0); gamma21 and gamma32 (finite and > 0); min_neighbors >= 1.
 *
 * Support of point i: the ranks 0 .. k_s-1 of sicp_knn(slot, k_s) for the point itself (contracts (D) and (K)), the point
 * itself included.  A rank counts iff d2 < salient_radius * salient_radius (one rounded multiplication, strict; +inf: every
 * rank counts).  m_i is the number of ranks that count.
 *
 * Sums: tree(t) is contract (E)'s balanced adjacent-pair tree over the positions 0 .. K-1 -- position r is rank r --, K the
 * next power of two >= k_s; a rank that does not count and every pad position contribute +0.0.
 *
 * Covariance, with m = (double)m_i:
 *   c_a  = tree(x_a) / m                                   for the three axes
 *   C_ab = tree((x_a - c_a) * (x_b - c_b)) / m             for the six entries 00 01 02 11 12 22: two subtractions, one
 *                                                          multiplication per rank, one division per entry
 * Eigenvalues: the cyclic Jacobi iteration of the normals (jacobi3, the one text of oracle/sicp_oracle.c:orc_normals) on C; the
 * three diagonal entries w that it leaves are sorted as the normals sort them: lo the first smallest, hi the first largest,
 * all equal: lo = 2, hi = 0; mid the third.  e1 = w[hi], e2 = w[mid], e3 = w[lo].  m_i == 0: e1 = e2 = e3 = +0.0.
 *
 * Salient: point i is salient iff m_i >= min_neighbors and e2 < gamma21 * e1 and e3 < gamma32 * e2 and e3 > 0 (one rounded
 * multiplication each, no division; a NaN fails).  A support whose e3 is exactly 0 -- flat or collinear in exact arithmetic, as
 * lattices are -- is never salient; what rounding leaves of a degenerate support is judged like any other number.
 * Saliency: s_i = e3 when salient, else +0.0.
 *
 * Non-maximum suppression, for a salient i: the neighbourhood is the ranks of sicp_knn(slot, k_n) for the point itself with
 * d2 < nms_radius * nms_radius; c_i their number (the point itself, or the duplicates that outrank it, included).  i is a
 * keypoint iff c_i >= min_neighbors and, for every such rank j != i, s_i > s_j or (s_i == s_j and i < j): ties go to the lowest
 * index.
 *
 * Clipping: a ball that holds more than k points is seen through its k nearest only.  n_clipped_salient counts the points whose
 * rank k_s-1 still counted, n_clipped_nms the salient points whose rank k_n-1 still lay in the neighbourhood (both always 0 with
 * a radius of +inf): k was too small for that radius there.
 *
 * keep_out (n bytes: 1 keypoint, 0 not), saliency_out (n doubles, nullable) and eig_out ((n, 3) doubles: e1 e2 e3, nullable)
 * are host or device memory (told apart as sicp_select_in_range tells its in_range_out).  The call runs on the ctx's stream
 * and is complete on return.  Refused with SICP_ERR_INVALID before any device work, the message naming the argument: a NULL
 * ctx / keep_out / out; k_s or k_n < 2, > SICP_KEYPOINT_MAX_K, > n; a radius NaN or <= 0; a gamma not finite or <= 0;
 * min_neighbors < 1; an empty slot or a shard; a ctx with an exchange or an active communicator; a cloud of 2^31 points or more.
 *
 * Scratch (8 bytes of saliency and 8 bytes of row list per point, 16 k bytes per point of one chunk, the staging of outputs that
 * are host memory) stays with the ctx and goes with sicp_ctx_destroy.
 */
#ifndef SIMPLEICP_HIP_KEYPOINTS_H
#define SIMPLEICP_HIP_KEYPOINTS_H

#include "simpleicp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: sicp_keypoints. */
#define SICP_KEYPOINTS_VERSION 1

/* Largest k_s and k_n (the one-sweep k-NN's, SICP_OUTLIER_MAX_K). */
#define SICP_KEYPOINT_MAX_K 128

int sicp_keypoints_version(void);

/* n_small: points with m_i < min_neighbors */
typedef struct sicp_keypoint_stats {
    int64_t n_points, n_salient, n_keypoints, n_small, n_clipped_salient, n_clipped_nms;
} sicp_keypoint_stats;

int sicp_keypoints(sicp_ctx *ctx, int slot, int k_s, double salient_radius, int k_n, double nms_radius, double gamma21,
                   double gamma32, int64_t min_neighbors, uint8_t *keep_out, double *saliency_out, double *eig_out,
                   sicp_keypoint_stats *out);

#ifdef __cplusplus
}
#endif

#endif
