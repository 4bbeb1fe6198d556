/*
 * simpleicp_hip_fpfh.h -- companion C ABI of libsimpleicp_hip.so: FPFH descriptors (33 floats per point), the expensive
 * step of a global registration.
 *
 * This header includes simpleicp_hip.h and does not change it: SICP_ABI_VERSION stays what it is, this entry has
 * SICP_FPFH_VERSION of its own.  The conventions of simpleicp_hip.h hold.
 *
 * The rules, arithmetic contract (F) of DESIGN.md section 17.  Everything is float64; every operation named below is rounded
 * on its own (no FMA); dot products are (a*b + c*d) + e*f as in contracts (P) and (N); no libm call takes part except sqrt
 * and division, both correctly rounded; no floating-point atomics; every sum has a fixed order.
 *
 * Inputs: the slot's n points; one float32 normal per point, upcast exactly; k (2 <= k <= SICP_FPFH_MAX_K, k <= n); radius
 * (+inf: none; otherwise finite and > 0).  With a viewpoint (vx, vy, vz) the normal of the point (x, y, z) is negated before
 * use iff ((vx-x)*nx + (vy-y)*ny) + (vz-z)*nz < 0 (a NaN compares false: such a normal stays as it is).
 *
 * Neighbourhood of point i: ranks 1 .. k-1 of sicp_knn(slot, k) for the point itself (contracts (D) and (K)); rank 0 is left
 * out whichever point it is.  Rank 0 always has d2 == 0: it is the point itself or, for a point with exact duplicates, the
 * lowest-index duplicate -- the point itself is then one of the later ranks with d2 == 0, and every pair with d2 == 0 is void
 * (below).  Either way the pairs that count are the ranks with d2 > 0.  A rank counts only if d2 < radius * radius (one rounded
 * multiplication, strict; radius = +inf: every rank counts).
 *
 * Pair feature of the point (p, n_p) with a neighbour (q, n_q), d2 from the k-NN list:
 *   dp = q - p,  f4 = sqrt(d2),  a1 = (n_p . dp) / f4,  a2 = (n_q . dp) / f4
 *   fabs(a1) < fabs(a2):  n1 = n_q, n2 = n_p, dp = -dp, f3 = -a2       otherwise:  n1 = n_p, n2 = n_q, f3 = a1
 *   v = dp x n1 (component x: dp.y*n1.z - dp.z*n1.y, and cyclic),  vn = sqrt(v . v),  v = v / vn,  w = n1 x v
 *   f2 = v . n2,  a = w . n2,  b = n1 . n2                               (f1 = atan2(a, b) is never formed)
 * The pair is VOID, counted nowhere, if d2 == 0, if vn == 0, or if any of the six normal components is not finite.
 *
 * Bins, eleven per feature: f1 in 0..10, f2 in 11..21, f3 in 22..32.
 *   bin(f) = min(10, max(0, floor(11 * ((f + 1) * 0.5))))   taken in float64 before the conversion; a NaN gives 0
 *   f2 -> 11 + bin(f2),  f3 -> 22 + bin(f3)
 *   f1: the number of borders phi_j = -pi + 2 pi j / 11, j = 1 .. 10, the direction (b, a) has reached, decided with the table
 *   SICP_FPFH_BORDERS of (c_j, s_j) and the cross products x_j = c_j*a - s_j*b (two rounded multiplications, one subtraction):
 *     a > 0:  5 + #{ j in 6..10 : x_j >= 0 }      (borders 1..5 lie below 0 and are passed; 6..10 share the upper half plane)
 *     a < 0:      #{ j in 1..5  : x_j >= 0 }      (borders 6..10 lie above 0; 1..5 share the lower half plane)
 *     a == +-0 and b < 0: 0                       (the direction -pi, first sector of [-pi, pi); +pi is the same direction)
 *     anything else (a == +-0 or NaN, b >= 0, b == +-0 or NaN): 5      (atan2(0, b >= 0) = 0; a = b = 0 included)
 *   The table's twenty literals ARE the contract; that they are cos / sin of phi_j to within an ulp is documentation.
 *
 * SPFH: c_i[0..32] exact counts, m_i the number of non-void pairs of point i; S_i[b] = (100.0 * c_i[b]) / m_i, all +0.0 when
 * m_i == 0.
 *
 * FPFH, for every bin b: W_i[b] = sum of S_j[b] / d2_ij over the neighbours j that count, in rank order, from +0.0, every
 * division and addition rounded on its own; a neighbour with d2 == 0 or a non-finite normal is skipped.  For each group of
 * eleven bins T = ((W_i[g] + W_i[g+1]) + ...) + W_i[g+10] in bin order.
 *   F_i[b] = S_i[b] + (T > 0 ? (W_i[b] * 100.0) / T : 0.0),  rounded once to float32.
 *
 * normals, fpfh_out and spfh_counts_out are host or device memory (told apart as sicp_select_in_range tells its
 * in_range_out).  The call runs on the ctx's stream and is complete on return.  Refused with SICP_ERR_INVALID before any
 * device work, the message naming the argument: a NULL normals / fpfh_out / out; k < 2, k > SICP_FPFH_MAX_K, k > n; radius
 * NaN or <= 0; a non-finite viewpoint; an empty slot or a shard; a ctx with an exchange or an active communicator; a cloud of
 * 2^31 points or more.
 *
 * Scratch (12 + 68 bytes per point, 16 k bytes per point of one chunk, 132 bytes per point when fpfh_out is host memory)
 * stays with the ctx and goes with sicp_ctx_destroy.
 */
#ifndef SIMPLEICP_HIP_FPFH_H
#define SIMPLEICP_HIP_FPFH_H

#include "simpleicp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: sicp_fpfh. */
#define SICP_FPFH_VERSION 1

/* Largest k (the one-sweep k-NN's, SICP_OUTLIER_MAX_K) and the descriptor's length. */
#define SICP_FPFH_MAX_K 128
#define SICP_FPFH_BINS 33

/* (c_j, s_j), j = 1 .. 10: the borders of the eleven sectors of f1. */
#define SICP_FPFH_BORDERS { \
    {-0x1.aeb8c8764f0bap-1, -0x1.14cedf8bb580bp-1}, \
    {-0x1.a9628d9c712b6p-2, -0x1.d1bb48eee2c13p-1}, \
    {0x1.2375f640f44dbp-3, -0x1.fac9e043842efp-1}, \
    {0x1.4f49e7f775887p-1, -0x1.82f19bb3a28a1p-1}, \
    {0x1.eb42a9bcd5057p-1, -0x1.207e7fd768dbfp-2}, \
    {0x1.eb42a9bcd5057p-1, 0x1.207e7fd768dbfp-2}, \
    {0x1.4f49e7f775887p-1, 0x1.82f19bb3a28a1p-1}, \
    {0x1.2375f640f44dbp-3, 0x1.fac9e043842efp-1}, \
    {-0x1.a9628d9c712b6p-2, 0x1.d1bb48eee2c13p-1}, \
    {-0x1.aeb8c8764f0bap-1, 0x1.14cedf8bb580bp-1} }

int sicp_fpfh_version(void);

/* n_pairs: the sum of the m_i; n_void_pairs: ranks 1 .. k-1 within the radius whose pair was void; n_empty: points with m_i == 0 */
typedef struct sicp_fpfh_stats { int64_t n_points, n_pairs, n_void_pairs, n_empty; } sicp_fpfh_stats;

/* normals: (n, 3) float32; viewpoint: 3 doubles (host) or NULL; fpfh_out: (n, 33) float32; spfh_counts_out (nullable):
 * (n, 34) uint16, the 33 counts and m_i; *out: the record (host). */
int sicp_fpfh(sicp_ctx *ctx, int slot, const float *normals, int k, double radius, const double *viewpoint, float *fpfh_out,
              uint16_t *spfh_counts_out, sicp_fpfh_stats *out);

#ifdef __cplusplus
}
#endif

#endif
