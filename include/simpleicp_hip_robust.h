/*
 * simpleicp_hip_robust.h -- companion C ABI of libsimpleicp_hip.so: the rigid pose of matched points by a robust fit over all
 * matches at once -- every match weighted by the Geman-McClure weight of its residual, the weighted least-squares pose refitted,
 * the weight's scale tightened round by round (graduated non-convexity, as Fast Global Registration runs it).  The deterministic
 * partner of the random triples of simpleicp_hip_global.h (contract (R)): no seed, no hypothesis count, no edge ratio.
 *
 * This header includes simpleicp_hip.h and does not change it: SICP_ABI_VERSION stays what it is, this entry has
 * SICP_ROBUST_VERSION of its own.  The conventions of simpleicp_hip.h hold.  The entry touches no cloud slot: the ctx gives its
 * stream and its scratch.  It runs on the ctx's stream and is complete on return; every array pointer is host or device memory
 * (told apart as sicp_fpfh tells its pointers apart).  No floating-point atomic takes part; the results do not depend on grid
 * shape, launch order or on which of the library's two paths ran.
 *
 * ---- contract (G), sicp_pose_robust ----
 * src, dst (m, 3) float64: row c of src (p_c) is matched to row c of dst (q_c).  3 <= m < 2^31, 1 <= b < 2^31,
 * 1 <= rounds <= SICP_ROBUST_MAX_ROUNDS, max_distance finite and > 0, divisor finite and > 1, start_scale finite and > 0 or
 * exactly 0 (automatic).  md2 = max_distance * max_distance (one rounded multiplication).
 * Everything is float64, every operation rounded on its own, a fused multiply-add only where contracts (T) and (D) have one; no
 * libm call takes part except sqrt and division.  Every sum over rows is the adjacent-pair tree of contract (E) over the rows
 * 0 .. m-1 (pad with +0.0 to the next power of two, a = a[0::2] + a[1::2] until one value is left).
 * Under a pose (R, t): y = R p_c + t by contract (T), d2_c between y and q_c by contract (D).  A row is VALID iff its six
 * coordinates are finite; it COUNTS under a pose iff it is valid and its d2_c is finite.
 * For every pose k, independently:
 *  0. the start.  Any of the twelve numbers of poses_in[k] not finite: VOID -- inliers_out[k] = -1, poses_out[k] twelve +0.0,
 *     scales_out[k] = +0.0, no round.  poses_in == NULL (b must be 1): the start is R = I, t = 0.
 *     The scale s: start_scale if it is not 0.  Otherwise s = 2.0 * max(d2_c) over the rows that count under the start (the
 *     library takes the maximum as an integer maximum of the bit patterns, which order like the values for d2_c >= +0: exact,
 *     whatever the order); no row counts: the pose is VOID as above.  (A maximum so large that s is +inf gives weights that are
 *     not finite: the first round yields nothing.)  Then  if (s < md2) s = md2.
 *  1. a round, with the current pose (R, t) and the scale s:
 *     the weight  u = s / (s + d2_c),  w_c = u * u;  a row that does not count under (R, t) has w_c = +0.0 and contributes +0.0
 *     to every tree of the round (none of the products below is formed for it).
 *     Sweep A, seven trees: W = tree(w_c), Sp[i] = tree(w_c * p_c[i]), Sq[i] = tree(w_c * q_c[i]).
 *     W not finite or not > 0: the round yields nothing.  cp[i] = Sp[i] / W, cq[i] = Sq[i] / W.
 *     Sweep B, nine trees: K[i][j] = tree((w_c * (p_c[i] - cp[i])) * (q_c[j] - cq[j])) -- one subtraction per factor, the weight
 *     multiplied onto the first factor, then the product.
 *     Horn's symmetric 4 x 4 matrix of K, the SICP_POSEFIT_SWEEPS cyclic Jacobi sweeps, the quaternion of the largest diagonal
 *     entry, its normalisation, R and t[r] = cq[r] - ((R[r][0]*cp.x + R[r][1]*cp.y) + R[r][2]*cp.z): expression by expression
 *     those of contract (L) step 1 (simpleicp_hip_posefit.h) from "Horn's symmetric 4 x 4 matrix" on.
 *     Any of the twelve numbers not finite: the round yields nothing.
 *     A round that yields nothing ends the rounds of this pose; the pose and the scale before it stay.  Otherwise its pose is
 *     the current one, and  s = s / divisor;  if (s < md2) s = md2.
 *  2. the output.  poses_out[k] is the current pose after the last round -- the latest, there is no "keep the best": the
 *     estimator's answer is where the graduation ends.  inliers_out[k] is the number of rows with d2_c < md2 (strict, a NaN
 *     fails) under it; scales_out[k] is the final s.
 *  3. the record: n_poses = b; n_void = void poses (of either kind); best = the lowest k with the largest inliers_out >= 0,
 *     best_inliers its count; best = -1, best_inliers = -1 if there is none.
 * poses_in, poses_out rows: R row-major, then t -- the layout of contract (R)'s poses_out.
 *
 * Refused with SICP_ERR_INVALID before any device work, the message naming the argument: a NULL ctx, a NULL required pointer
 * (poses_in is required unless b == 1), m, b, rounds, max_distance, divisor or start_scale out of range, a ctx with an exchange
 * or an active communicator.
 *
 * Scratch (per pose: nine doubles for every 1 024 rows and 22 words of state; the staged copy of whatever array is host memory)
 * stays with the ctx and goes with sicp_ctx_destroy.
 */
#ifndef SIMPLEICP_HIP_ROBUST_H
#define SIMPLEICP_HIP_ROBUST_H

#include "simpleicp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: sicp_pose_robust. */
#define SICP_ROBUST_VERSION 1

/* Most rounds a call takes. */
#define SICP_ROBUST_MAX_ROUNDS 256

int sicp_robust_version(void);

typedef struct sicp_robust_stats { int64_t n_poses, n_void, best, best_inliers; } sicp_robust_stats;

/* src, dst (m, 3) float64: row c of src is matched to row c of dst.  poses_in (b, 12) float64: R row-major then t; NULL: b must
 * be 1 and the start is the identity.  max_distance finite > 0; rounds >= 1; divisor finite > 1; start_scale finite > 0, or 0:
 * twice the largest squared residual under the start.  poses_out (b, 12) float64, inliers_out (b) int32, scales_out (b) float64,
 * *out: the record (host). */
int sicp_pose_robust(sicp_ctx *ctx, const double *src, const double *dst, int64_t m, const double *poses_in, int64_t b,
                     double max_distance, int rounds, double divisor, double start_scale, double *poses_out, int32_t *inliers_out,
                     double *scales_out, sicp_robust_stats *out);

#ifdef __cplusplus
}
#endif

#endif
