/*
 * simpleicp_hip_posefit.h -- companion C ABI of libsimpleicp_hip.so: the rigid pose that best maps matched points onto each other
 * in the least-squares sense (Kabsch / Horn), and poses refitted on their own inliers -- what follows a hypothesis' pose of
 * simpleicp_hip_global.h (its contract (R)) in a global registration.
 *
 * This header includes simpleicp_hip.h and does not change it: SICP_ABI_VERSION stays what it is, this entry has
 * SICP_POSEFIT_VERSION of its own.  The conventions of simpleicp_hip.h hold.  The entry touches no cloud slot: the ctx gives its
 * stream and its scratch.  It runs on the ctx's stream and is complete on return; every array pointer is host or device memory
 * (told apart as sicp_fpfh tells its pointers apart).  No floating-point atomic takes part; the results do not depend on grid
 * shape or launch order.
 *
 * ---- contract (L), sicp_pose_refit ----
 * src, dst (m, 3) float64: row c of src (p_c) is matched to row c of dst (q_c).  3 <= m < 2^31, b >= 1,
 * 1 <= rounds <= SICP_POSEFIT_MAX_ROUNDS, max_distance > 0 (finite or +inf).  md2 = max_distance * max_distance (one rounded
 * multiplication; +inf stays +inf).
 * Everything is float64, every operation rounded on its own, a fused multiply-add only where contracts (T) and (D) have one; no
 * libm call takes part except sqrt and division.  Every sum over rows is the adjacent-pair tree of contract (E) over the rows
 * 0 .. m-1 (pad with +0.0 to the next power of two, a = a[0::2] + a[1::2] until one value is left).
 * For every pose k, independently:
 *  0. the start.  Any of the twelve numbers of poses_in[k] not finite: VOID -- inliers_out[k] = -1, poses_out[k] twelve +0.0,
 *     no round.  Otherwise the pose is scored as in contract (R) step 5: its mask is the rows c with d2 < md2 (strict, a NaN
 *     fails), y = R p_c + t by contract (T), d2 between y and q_c by contract (D); its count is the number of those rows.  With
 *     md2 = +inf these are the rows whose d2 is finite.  poses_in == NULL (b must be 1): there is no input pose -- its count is
 *     taken as -1 -- and the first round's mask is the rows whose six coordinates are finite.
 *  1. a round, under the mask of the current pose (the input pose, then the latest round's), n its count:
 *     n < 3: the round yields nothing.
 *     Sweep A: Sp = tree(p_c), Sq = tree(q_c) per component, a row outside the mask contributing +0.0; cp = Sp / n, cq = Sq / n
 *     (n converted exactly).
 *     Sweep B: K[i][j] = tree((p_c[i] - cp[i]) * (q_c[j] - cq[j])), one subtraction per factor and one multiplication, +0.0 for
 *     a row outside the mask (centred first: coordinates of 1e6 with an extent of 100 lose nothing to cancellation).
 *     Horn's symmetric 4 x 4 matrix, with Sxy = K[0][1] and so on:
 *       N00 = (Sxx + Syy) + Szz    N01 = Syz - Szy            N02 = Szx - Sxz            N03 = Sxy - Syx
 *                                  N11 = (Sxx - Syy) - Szz    N12 = Sxy + Syx            N13 = Szx + Sxz
 *                                                             N22 = (Syy - Sxx) - Szz    N23 = Syz + Szy
 *                                                                                        N33 = (Szz - Sxx) - Syy
 *     Cyclic Jacobi on A = N, V = I: SICP_POSEFIT_SWEEPS sweeps, each over the pairs (p, q) = (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
 *     in this order.  A pair with A[p][q] == 0 is skipped.  Otherwise
 *       theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]),   t = (theta < 0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0)),
 *       c = 1.0 / sqrt(t * t + 1.0),   s = t * c,
 *       A'[p][p] = A[p][p] - t * A[p][q],   A'[q][q] = A[q][q] + t * A[p][q],   A'[p][q] = A'[q][p] = 0,
 *       for the two r outside the pair: A'[r][p] = A'[p][r] = c * A[r][p] - s * A[r][q],  A'[r][q] = A'[q][r] = s * A[r][p] + c * A[r][q],
 *       for r = 0 .. 3:                 V'[r][p] = c * V[r][p] - s * V[r][q],             V'[r][q] = s * V[r][p] + c * V[r][q]
 *     (all from the values before the rotation).  The quaternion (w, x, y, z) is the column j of V with the largest A[j][j], the
 *     lowest j on a tie (strict comparisons from j = 0), divided by sqrt(((w*w + x*x) + y*y) + z*z).
 *       R00 = ((w*w + x*x) - y*y) - z*z    R01 = (x*y - w*z) * 2.0            R02 = (x*z + w*y) * 2.0
 *       R10 = (x*y + w*z) * 2.0            R11 = ((w*w - x*x) + y*y) - z*z    R12 = (y*z - w*x) * 2.0
 *       R20 = (x*z - w*y) * 2.0            R21 = (y*z + w*x) * 2.0            R22 = ((w*w - x*x) - y*y) + z*z
 *       t[r] = cq[r] - ((R[r][0]*cp.x + R[r][1]*cp.y) + R[r][2]*cp.z)                        (contract (R), step 4)
 *     Any of the twelve numbers not finite: the round yields nothing.
 *  2. keep the best.  A round's pose is scored as in step 0.  The output is the pose with the largest count among the input pose
 *     and the pose of every round; the earliest wins a tie, so the input pose stays unless a round is strictly better and
 *     inliers_out[k] >= the input pose's count.  The next round starts from the latest round's pose, not from the best.  A
 *     round that yields nothing, or whose pose equals its predecessor's bit for bit, ends the rounds of this pose (they would
 *     repeat themselves).  No pose at all (NULL start, no round's pose): inliers_out = -1, twelve +0.0.
 *  3. the record: n_void = void input poses; n_improved = poses whose output count is above their input count; best = the lowest
 *     k with the largest inliers_out >= 0, best_inliers its count; best = -1, best_inliers = -1 if there is none.
 * poses_in, poses_out rows: R row-major, then t -- the layout of contract (R)'s poses_out.
 *
 * Refused with SICP_ERR_INVALID before any device work, the message naming the argument: a NULL ctx, a NULL required pointer
 * (poses_in is required unless b == 1), m, b, rounds or max_distance out of range, a ctx with an exchange or an active
 * communicator.
 *
 * Scratch (per pose: nine doubles and a count for every 1 024 rows, and 35 words of state; the staged copy of whatever array is
 * host memory) stays with the ctx and goes with sicp_ctx_destroy.
 */
#ifndef SIMPLEICP_HIP_POSEFIT_H
#define SIMPLEICP_HIP_POSEFIT_H

#include "simpleicp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: sicp_pose_refit. */
#define SICP_POSEFIT_VERSION 1

/* Most rounds a call takes. */
#define SICP_POSEFIT_MAX_ROUNDS 64

/* Jacobi sweeps of every fit (DESIGN.md section 19 says how the number was found). */
#define SICP_POSEFIT_SWEEPS 6

int sicp_posefit_version(void);

typedef struct sicp_posefit_stats { int64_t n_poses, n_void, n_improved, best, best_inliers; } sicp_posefit_stats;

/* src, dst (m, 3) float64: row c of src is matched to row c of dst.  poses_in (b, 12) float64: R row-major then t, the layout of
 * contract (R)'s poses_out; NULL: b must be 1 and the start is "every row counts" (a plain fit).  max_distance finite > 0
 * or +inf.  rounds >= 1.  poses_out (b, 12) float64, inliers_out (b) int32, *out: the record (host). */
int sicp_pose_refit(sicp_ctx *ctx, const double *src, const double *dst, int64_t m, const double *poses_in, int64_t b,
                    double max_distance, int rounds, double *poses_out, int32_t *inliers_out, sicp_posefit_stats *out);

#ifdef __cplusplus
}
#endif

#endif
