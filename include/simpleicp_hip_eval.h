/*
 * simpleicp_hip_eval.h -- companion C ABI of libsimpleicp_hip.so: how good a registration is.  Fitness, inlier RMSE and
 * the sums of the information matrix of one resident cloud against the other under a transform, reduced on the device.
 *
 * This header includes simpleicp_hip.h and does not change it: SICP_ABI_VERSION stays what it is, these entries
 * have SICP_EVAL_VERSION of their own.  The conventions of simpleicp_hip.h hold.
 *
 * The rule, arithmetic contract (E) of DESIGN.md section 14.
 *   Queries i = 0 ... Q-1 are the rows sel_idx of the query slot in the order given (sel_idx NULL: the slot's points
 *   in their order, Q = its size).  (idx_i, d2_i) of query i is what sicp_knn(search_slot, k = 1, H, max_distance)
 *   defines for it -- contracts (T), (D), (K), the bound strict: d2 < max_distance * max_distance.  Query i is an
 *   inlier iff idx_i >= 0.
 *   Ten float64 terms per query, p = (x, y, z) the query point as stored (the query cloud's own frame):
 *     t0 = d2_i | t1..t3 = x, y, z | t4..t9 = x*x, y*y, z*z, x*y, x*z, y*z (one rounded multiplication each)
 *   for an inlier, +0.0 each for every other query.
 *   n_inliers is an exact count.  S_j is the balanced adjacent-pair tree over t_j: the Q terms padded with +0.0 to the
 *   next power of two P >= max(Q, 1), then a <- a[0::2] + a[1::2] (separately rounded float64 additions) until one
 *   value is left.  The record depends on the input alone: not on launch geometry, not on repetition; no
 *   floating-point atomics take part.
 *
 * Refused with SICP_ERR_INVALID, before any device work, with a message that names the argument: out NULL, equal or
 * empty slots, a max_distance that is NaN or negative (+inf is allowed), a row of sel_idx out of range, a query cloud
 * that is a shard, a ctx with an exchange (sicp_set_exchange, an active communicator).
 *
 * The entry runs on the ctx's stream and is complete on return.  Its scratch (about 80 bytes per 1024 queries) stays
 * with the ctx and goes with sicp_ctx_destroy.
 */
#ifndef SIMPLEICP_HIP_EVAL_H
#define SIMPLEICP_HIP_EVAL_H

#include "simpleicp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: sicp_evaluate. */
#define SICP_EVAL_VERSION 1

typedef struct sicp_eval {
    int64_t n_queries, n_inliers;
    double  sum_d2;        /* S_0 */
    double  sum_p[3];      /* S_1..3 */
    double  sum_pp[6];     /* S_4..9: xx yy zz xy xz yz */
} sicp_eval;

int sicp_eval_version(void);

/* Every query (see above) of query_slot searches its nearest point among H * search_slot (H: 16 doubles, row major, NULL =
 * identity) within max_distance.  sel_idx: host or device memory (told apart as sicp_select_in_range tells its own), NULL =
 * every point of the slot, Q is ignored then.  *out: host memory. */
int sicp_evaluate(sicp_ctx *ctx, int query_slot, int search_slot, const int64_t *sel_idx, int64_t Q,
                  const double *H, double max_distance, sicp_eval *out);

#ifdef __cplusplus
}
#endif

#endif
