/*
 * simpleicp_hip_plane.h -- companion C ABI of libsimpleicp_hip.so: the dominant plane of a cloud (ground, floor, table, wall) --
 * planes through triples of its points scored by their inliers, and planes refitted on their own inliers.  What comes before the
 * clustering of simpleicp_hip_cluster.h in a segmentation: with the ground gone, the objects on it fall apart into clusters.
 *
 * This header includes simpleicp_hip.h and does not change it: SICP_ABI_VERSION stays what it is, these entries have
 * SICP_PLANE_VERSION of their own.  The conventions of simpleicp_hip.h and simpleicp_hip_global.h hold.  Neither entry touches a
 * cloud slot: the ctx gives its stream and its scratch.  Both run on the ctx's stream and are complete on return; every array
 * pointer is host or device memory (told apart as sicp_fpfh tells its pointers apart).  No floating-point atomic takes part; the
 * results do not depend on grid shape or launch order.
 *
 * X (n, 3) float64 rows; mask (n) uint8, nullable: NULL means every row is a candidate.  A row with mask 0 never counts and never
 * defines a plane.  A plane is four float64 numbers (a, b, c, d): the unit normal, then d; the residual of a row (x, y, z) is
 *     r = fma(c, z, fma(b, y, a * x)) + d
 * (one multiplication, two fused multiply-adds, one addition), and the row is an INLIER of the plane iff it is a candidate and
 * fabs(r) < max_distance (strict, a NaN fails).
 *
 * ---- contract (P), sicp_plane_triplets ----
 * triples (h, 3) int32, drawn by the caller (the library holds no random generator).  3 <= n < 2^31, h >= 1, max_distance finite
 * and > 0.  Everything is float64, every operation rounded on its own, a fused multiply-add only in the residual above; no libm
 * call takes part except sqrt and division.
 * A hypothesis (i0, i1, i2) with the points p0, p1, p2, in this order:
 *  1. an index outside 0 .. n-1, or two equal indices: VOID (inliers = -1; the plane is four +0.0); nothing is dereferenced.
 *     After the index checks: one of the three rows masked out: VOID.
 *  2. the plane: u = p1 - p0, v = p2 - p0, w = u x v (component x: u.y*v.z - u.z*v.y, and cyclic: contract (F)'s cross product),
 *     len = sqrt((w.x*w.x + w.y*w.y) + w.z*w.z), nrm = w / len per component, d = -((nrm.x*p0.x + nrm.y*p0.y) + nrm.z*p0.z).
 *     Any of the four numbers not finite: VOID -- collinear or coincident points, non-finite coordinates.  The normal's
 *     orientation is the triple's: there is no sign rule.
 *  3. inliers = the number of inliers of the plane among the rows 0 .. n-1.  An exact integer.
 * The record: n_points = n, n_candidates = rows with mask != 0 (n for a NULL mask), n_hypotheses = h, n_void; best: the lowest
 * index among the hypotheses with the largest inliers >= 0, best_inliers its count; best = -1, best_inliers = -1 if there is none.
 *
 * ---- contract (Q), sicp_plane_refit ----
 * Contract (L) of simpleicp_hip_posefit.h, for planes.  b >= 1, 1 <= rounds <= SICP_PLANE_MAX_ROUNDS; keep_out requires b == 1.
 * Every sum over rows is the adjacent-pair tree of contract (E) over the rows 0 .. n-1 (pad with +0.0 to the next power of two,
 * a = a[0::2] + a[1::2] until one value is left).  For every plane k, independently:
 *  0. the start.  Any of the four numbers of planes_in[k] not finite: VOID -- inliers_out[k] = -1, planes_out[k] four +0.0, no
 *     round.  Otherwise the plane is scored as in (P): its mask is its inliers, its count their number.
 *  1. a round, under the mask of the current plane (the input plane, then the latest round's), k its count:
 *     k < 3: the round yields nothing.
 *     Sweep A: S = tree(rows) per component, a row outside the mask contributing +0.0; c = S / k (k converted exactly).
 *     Sweep B: the six centred products (x-cx)(x-cx), (x-cx)(y-cy), (x-cx)(z-cz), (y-cy)(y-cy), (y-cy)(z-cz), (z-cz)(z-cz), one
 *     subtraction per factor and one multiplication, +0.0 for a row outside the mask, summed by the same tree; not divided.
 *     The cyclic Jacobi iteration of the normals (jacobi3: simpleicp_hip.h's normals, oracle/sicp_oracle.c:orc_normals) on that
 *     symmetric matrix, exactly as it stands.  The normal is the column of V with the smallest diagonal entry, the lowest column
 *     on a tie (strict comparisons from column 0), divided by sqrt((x*x + y*y) + z*z), and negated if its dot product with the
 *     current plane's normal, (a*b + c*d) + e*f, is < 0.  d = -((n.x*c.x + n.y*c.y) + n.z*c.z).
 *     Any of the four numbers not finite: the round yields nothing.
 *  2. keep the best.  A round's plane is scored as in step 0.  The output is the plane with the largest count among the input
 *     plane and the plane of every round; the earliest wins a tie.  The next round starts from the latest round's plane, not from
 *     the best.  A round that yields nothing, or whose plane equals its predecessor's bit for bit, ends the rounds of this plane.
 *  3. keep_out (nullable; b == 1): 1 where the row is an inlier of planes_out[0], 0 elsewhere -- all 0 for a void output; the same
 *     residual expression as the count, so its popcount is inliers_out[0].
 *  4. the record: n_planes = b; n_void = void input planes; n_improved = planes whose output count is above their input count;
 *     best = the lowest k with the largest inliers_out >= 0, best_inliers its count; -1 and -1 if there is none.
 *
 * Refused with SICP_ERR_INVALID before any device work, the message naming the argument: a NULL ctx, a NULL required pointer
 * (planes_out of sicp_plane_triplets, mask and keep_out are nullable), n, h, b, rounds or max_distance out of range, keep_out
 * with b != 1, a ctx with an exchange or an active communicator.
 *
 * Scratch (four doubles per hypothesis; per refitted plane six doubles and a count for every 1 024 rows and 21 words of state;
 * the staged copy of whatever array is host memory) stays with the ctx and goes with sicp_ctx_destroy.  SICP_PLANE_SPAN (read at
 * sicp_ctx_create): rows a workgroup of the scoring kernel takes (tests; 0 or unset: chosen per call).
 */
#ifndef SIMPLEICP_HIP_PLANE_H
#define SIMPLEICP_HIP_PLANE_H

#include "simpleicp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: sicp_plane_triplets, sicp_plane_refit. */
#define SICP_PLANE_VERSION 1

/* Most rounds a call of sicp_plane_refit takes. */
#define SICP_PLANE_MAX_ROUNDS 16

int sicp_plane_version(void);

typedef struct sicp_plane_stats { int64_t n_points, n_candidates, n_hypotheses, n_void, best, best_inliers; } sicp_plane_stats;

/* planes_out (nullable): (h, 4) float64; inliers_out: (h) int32; *out: the record (host). */
int sicp_plane_triplets(sicp_ctx *ctx, const double *X, int64_t n, const uint8_t *mask, const int32_t *triples, int64_t h,
                        double max_distance, double *planes_out, int32_t *inliers_out, sicp_plane_stats *out);

typedef struct sicp_plane_refit_stats { int64_t n_planes, n_void, n_improved, best, best_inliers; } sicp_plane_refit_stats;

/* planes_in, planes_out: (b, 4) float64; inliers_out: (b) int32; keep_out (nullable, b == 1): (n) uint8; *out: the record (host). */
int sicp_plane_refit(sicp_ctx *ctx, const double *X, int64_t n, const uint8_t *mask, const double *planes_in, int64_t b,
                     double max_distance, int rounds, double *planes_out, int32_t *inliers_out, uint8_t *keep_out,
                     sicp_plane_refit_stats *out);

#ifdef __cplusplus
}
#endif

#endif
