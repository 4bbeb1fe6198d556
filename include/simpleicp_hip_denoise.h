/*
 * simpleicp_hip_denoise.h -- companion C ABI of libsimpleicp_hip.so: moving-least-squares smoothing of a cloud at polynomial
 * order 0/1 -- every point is projected onto the plane fitted to its neighbourhood (PCL's MovingLeastSquares without a
 * polynomial, CloudCompare's "MLS smooth").  The step in front of everything that stands on a neighbourhood's covariance:
 * normals, smooth regions, orientation, descriptors.
 *
 * This header includes simpleicp_hip.h and does not change it: SICP_ABI_VERSION stays what it is, this entry has
 * SICP_DENOISE_VERSION of its own.  The conventions of simpleicp_hip.h hold.
 *
 * The rules, arithmetic contract (W) of DESIGN.md section 28.  Everything is float64; every operation named below is rounded
 * on its own (no FMA outside contract (D)'s distances); no libm call takes part except sqrt and division, both correctly
 * rounded; no floating-point atomics; every sum has a fixed order.  The contract covers finite coordinates whose sums do not
 * overflow.
 *
 * Inputs: the slot's n points; k (2 <= k <= SICP_KEYPOINT_MAX_K, k <= n); radius and bandwidth (+inf: none; otherwise > 0);
 * strength (finite, 0 <= strength <= 1); min_neighbors >= 1.
 *
 * 1. Support of point i: the ranks 0 .. k-1 of sicp_knn(slot, k) for the point itself (contracts (D) and (K)), the point itself
 *    included.  A rank counts iff d2 < radius * radius (one rounded multiplication, strict; +inf: every rank that holds a point
 *    counts).  m_i is the number of ranks that count.
 * 2. Weights: bandwidth = +inf: w = 1.0 for every rank that counts.  Otherwise t = 1.0 - d2 / (bandwidth * bandwidth) (one
 *    multiplication, one division, one subtraction) and w = t > 0 ? t * t : +0.0.  A rank that does not count and every pad
 *    position contribute +0.0 to every sum below, whatever their products would be.
 * 3. Sums: tree(t) is contract (E)'s balanced adjacent-pair tree over the positions 0 .. K-1 -- position r is rank r --, K the
 *    next power of two >= k, as contract (I) uses it.
 *      W    = tree(w)
 *      c_a  = tree(w * x_a) / W                               for the three axes
 *      C_ab = tree(w * ((x_a - c_a) * (x_b - c_b))) / W       for the six entries 00 01 02 11 12 22: the inner product is
 *                                                             rounded first, then the weight is applied
 * 4. Plane: the cyclic Jacobi iteration of the normals (jacobi3 of sicp_normals.h, the one text of
 *    oracle/sicp_oracle.c:orc_normals) on C with its eigenvectors; the normal n is the column normal_from_cov's rule takes --
 *    the first smallest diagonal entry, column 2 when all three are equal -- under that rule's sign: negated iff its component
 *    of largest magnitude (the first of equals) is negative.  n stays float64 for the projection; normals_out gets its three
 *    components rounded to float32.
 * 5. Projection:
 *      h     = ((x_i - c_x) * n_x + (y_i - c_y) * n_y) + (z_i - c_z) * n_z
 *      g     = strength * h
 *      out_a = x_a - g * n_a                                  for the three axes
 *      displacement_out[i] = g
 * 6. Small supports: m_i < min_neighbors: out = x_i bit for bit, the normal is three +0.0, g = +0.0.
 * 7. Record: n_points; n_small: the points of 6; n_moved: the points with g != 0.0; n_clipped: the points whose rank k-1 still
 *    counted under a finite radius (always 0 with +inf: k was too small for that radius there); max_displacement: the largest
 *    fabs(g), +0.0 if none -- an integer maximum over the bit patterns, which order as the non-negative doubles do.
 * 8. Jacobi rule: every point is projected from the input positions; no point sees another's output.  Every byte of the outputs
 *    depends on the inputs alone.
 *
 * points_out ((n, 3) doubles), normals_out ((n, 3) floats, nullable) and displacement_out (n doubles, nullable) are host or
 * device memory (told apart as sicp_keypoints tells its outputs apart); *out is host memory.  The call runs on the ctx's stream
 * and is complete on return.  Refused with SICP_ERR_INVALID before any device work, the message naming the argument, the
 * outputs untouched: a NULL ctx / points_out / out; k < 2, > SICP_KEYPOINT_MAX_K, > n; a radius or bandwidth NaN or <= 0; a
 * strength not finite, < 0 or > 1; min_neighbors < 1; an empty slot or a shard; a ctx with an exchange or an active
 * communicator; a cloud of 2^31 points or more.
 *
 * Scratch (16 k bytes per point of one chunk, the staging of outputs that are host memory) stays with the ctx and goes with
 * sicp_ctx_destroy.  Switch, read at sicp_ctx_create: SICP_DENOISE_CHUNK (points per k-NN search; 0 or unset: chosen per call).
 */
#ifndef SIMPLEICP_HIP_DENOISE_H
#define SIMPLEICP_HIP_DENOISE_H

#include "simpleicp_hip.h"
#include "simpleicp_hip_keypoints.h" /* SICP_KEYPOINT_MAX_K */

#ifdef __cplusplus
extern "C" {
#endif

/* 1: sicp_denoise. */
#define SICP_DENOISE_VERSION 1

int sicp_denoise_version(void);

typedef struct sicp_denoise_stats {
    int64_t n_points, n_small, n_moved, n_clipped;
    double max_displacement;
} sicp_denoise_stats;

int sicp_denoise(sicp_ctx *ctx, int slot, int k, double radius, double bandwidth, double strength, int64_t min_neighbors,
                 double *points_out, float *normals_out, double *displacement_out, sicp_denoise_stats *out);

#ifdef __cplusplus
}
#endif

#endif
