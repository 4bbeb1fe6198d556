/*
 * simpleicp_hip_consistency.h -- companion C ABI of libsimpleicp_hip.so: matched points pruned by pairwise length consistency.
 * A rigid motion keeps lengths, so two matches i and j can both be right only if the distance between their points in the one
 * cloud agrees with the distance between their partners in the other.  These pairwise tests form a graph on the matches (the
 * compatibility graph of TEASER++ and SC2-PCR); the right matches form a clique in it, wrong ones are tied to it by chance.  The
 * entry builds that graph and gives every match its degree and its core number; the rows of the largest core number (the maximal
 * k-core, TEASER++'s KCORE_HEU) are the pruned set.  It is a filter in front of the pose estimators of
 * simpleicp_hip_global.h, simpleicp_hip_posefit.h and simpleicp_hip_robust.h, which take the rows they are given.
 *
 * This header includes simpleicp_hip.h and does not change it: SICP_ABI_VERSION stays what it is, this entry has
 * SICP_CONSISTENCY_VERSION of its own.  The conventions of simpleicp_hip.h hold.  The entry touches no cloud slot: the ctx gives
 * its stream and its scratch.  It runs on the ctx's stream and is complete on return; src, dst, degree_out and core_out are each
 * host or device memory (told apart as sicp_pose_robust tells its pointers apart), the record is host memory.
 *
 * ---- contract (C), sicp_match_consistency ----
 * src, dst (m, 3) float64: row c of src (p_c) is matched to row c of dst (q_c).  3 <= m <= SICP_CONSISTENCY_MAX_ROWS,
 * tolerance finite and > 0, min_length finite and >= 0.
 * A row is VALID iff its six coordinates are finite.
 * For rows i != j:  a = sqrt(d2(p_i, p_j)),  b = sqrt(d2(q_i, q_j)),  d2 contract (D)'s squared distance
 *     d2(u, v) = fma(dz, dz, fma(dy, dy, dx * dx)),  dx = u.x - v.x, dy = u.y - v.y, dz = u.z - v.z
 * in float64, every operation rounded on its own, sqrt the correctly rounded one.  The expression is the same bits for (i, j)
 * and for (j, i): a floating-point subtraction with its operands swapped gives the exact negative, so dx, dy and dz only change
 * their sign; they enter (D) only as the products dx * dx, dy * dy, dz * dz, which do not see the sign, and nothing else of (D)
 * depends on the order.  The graph is therefore symmetric bit for bit, whichever row an implementation takes first.
 * Rows i and j are COMPATIBLE iff both are valid, a and b are finite (a length whose square overflows is not), and
 *     fabs(a - b) <= tolerance  and  a >= min_length  and  b >= min_length
 * (a NaN fails every comparison).  No row is compatible with itself.  With min_length == 0 two rows with the same points -- exact
 * duplicates, a = b = 0 -- are compatible; any min_length > 0 keeps them apart.
 * degree_out[i] = the number of rows compatible with row i.
 * core_out[i] = the core number of row i in that graph: the largest k such that i lies in a set of rows each of which is
 * compatible with at least k others of the set.  (A property of the graph, not of an algorithm: the set of rows with core number
 * >= k is the one largest such set, for every k.)  An invalid row has degree 0 and core 0.
 * The record, all int64: n_rows = m; n_valid = the valid rows; n_edges = the compatible pairs {i, j} (half the sum of the
 * degrees); max_degree, max_core = the largest of degree_out and of core_out; n_max_core = the rows whose core number is max_core,
 * 0 when max_core == 0; n_subrounds = the passes the library's peeling took to find the core numbers -- informative, and the one
 * field that may differ between the library's two paths and between versions.
 * Everything that leaves the entry is an integer.  The degrees are integer sums, the core numbers do not depend on any order; no
 * floating-point sum exists.  The results do not depend on grid shape, launch order or path.
 *
 * Refused with SICP_ERR_INVALID before any device work, the message naming the argument, the outputs untouched: a NULL ctx, a NULL
 * required pointer (all five are required), m, tolerance or min_length out of range, a ctx with an exchange or an active
 * communicator.
 *
 * Scratch -- the compatibility matrix as bits, m rows of ceil(m / 64) 64-bit words (128 MB at SICP_CONSISTENCY_MAX_ROWS), the
 * peeling's state (four bytes a row and ceil(m / 64) words), the staged copy of whatever array is host memory -- stays with the
 * ctx and goes with sicp_ctx_destroy.
 */
#ifndef SIMPLEICP_HIP_CONSISTENCY_H
#define SIMPLEICP_HIP_CONSISTENCY_H

#include "simpleicp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: sicp_match_consistency. */
#define SICP_CONSISTENCY_VERSION 1

/* Most rows a call takes: thin the matches first if there are more. */
#define SICP_CONSISTENCY_MAX_ROWS 32768

int sicp_consistency_version(void);

typedef struct sicp_consistency_stats {
    int64_t n_rows, n_valid, n_edges, max_degree, max_core, n_max_core, n_subrounds;
} sicp_consistency_stats;

/* src, dst (m, 3) float64: row c of src is matched to row c of dst.  tolerance finite > 0: how far the two lengths of a pair may
 * differ; min_length finite >= 0: pairs closer than this in either cloud are not compatible.  degree_out, core_out (m) int32,
 * *out: the record (host). */
int sicp_match_consistency(sicp_ctx *ctx, const double *src, const double *dst, int64_t m, double tolerance, double min_length,
                           int32_t *degree_out, int32_t *core_out, sicp_consistency_stats *out);

#ifdef __cplusplus
}
#endif

#endif
