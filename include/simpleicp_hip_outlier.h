/*
 * simpleicp_hip_outlier.h -- companion C ABI of libsimpleicp_hip.so: outlier removal, the statistical and the radius
 * filter.
 *
 * This header includes simpleicp_hip.h and does not change it: SICP_ABI_VERSION stays what it is, these entries
 * have SICP_OUTLIER_VERSION of their own.  The conventions of simpleicp_hip.h hold.
 *
 * The rules, arithmetic contract (O) of DESIGN.md section 15.
 *
 * Candidates: every point of the slot (rows and mask NULL), the m entries of the host list `rows` in the order given
 * (a repeated row is an entry of its own), or the points whose byte of the device mask is non-zero.  Neighbours are
 * always searched among ALL points of the slot, the candidate itself included.
 *
 * Statistical filter (k, std_ratio).  d2_(0) <= ... <= d2_(k-1): the candidate's k nearest points as sicp_knn(slot, k)
 * defines them (contracts (D) and (K); d2_(0) = 0, the point itself).
 *   d_i       = (sqrt(d2_(0)) + sqrt(d2_(1)) + ... + sqrt(d2_(k-1))) / k     float64, every sqrt (correctly rounded),
 *               every addition (in rank order) and the one division rounded on its own
 *   t_i       = d_i for a candidate, +0.0 for every other position (positions: the m list entries of a `rows` call,
 *               all n points otherwise); m = the exact number of candidates
 *   mean      = tree(t) / m             tree: contract (E)'s adjacent-pair tree, padded with +0.0 to a power of two
 *   u_i       = (d_i - mean) * (d_i - mean) for a candidate, +0.0 otherwise
 *   std       = sqrt(tree(u) / (m - 1));  m == 1: 0.0
 *   threshold = mean + std_ratio * std  (one multiplication, one addition)
 *   keep_i    = d_i <= threshold
 * m == 0 (an all-zero mask): nothing is kept; mean, std and threshold are 0.0.  No floating-point atomics take part:
 * the record and every verdict byte depend on the input alone.
 *
 * Radius filter (radius, min_points).  count_i = the points j of the slot, i itself included, with
 * d2(i, j) < radius * radius (contract (D); one rounded multiplication; strict).  keep_i = count_i > min_points.
 * The walk stops at min_points + 1: the count that leaves is min(count_i, min_points + 1).
 *
 * Outputs hold one value per list entry (`rows`) or per point of the slot (otherwise); in the masked form every
 * non-candidate gets 0 and keep_out may alias mask.  keep_out, mean_dist_out and count_out are host or device memory
 * (told apart as sicp_select_in_range tells its in_range_out).
 *
 * Refused with SICP_ERR_INVALID before any device work, the message naming the argument: a NULL keep_out / out /
 * kept_out; rows together with mask; a row out of range; k < 2, k > n, k > 128; std_ratio NaN or infinite; radius not
 * finite or <= 0; min_points < 0; an empty slot or a shard; a ctx with an exchange or an active communicator; a cloud
 * of 2^31 points or more; and, radius filter, a ball whose box of grid cells is larger than
 * SICP_OUTLIER_MAX_BOX_CELLS -- see sicp_outlier_radius_cells.
 *
 * Both filters run on the ctx's stream and are complete on return.  Their scratch (8 bytes per position, the
 * candidate list, 16 k bytes per candidate of one chunk) stays with the ctx and goes with sicp_ctx_destroy.
 */
#ifndef SIMPLEICP_HIP_OUTLIER_H
#define SIMPLEICP_HIP_OUTLIER_H

#include "simpleicp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: sicp_outlier_statistical, sicp_outlier_radius, sicp_outlier_radius_cells. */
#define SICP_OUTLIER_VERSION 1

/* Largest neighbour count of the statistical filter (the one-sweep k-NN's). */
#define SICP_OUTLIER_MAX_K 128

/* The radius filter walks, per candidate, the box of grid cells around its ball: per axis at most
 * min(cells of the grid, floor(2 radius / h) + 3) of them, h the cell size of the slot's grid (always the grid the points
 * were binned for, never a coarse twin).  A call whose box holds more cells than this is
 * refused -- the cost of a candidate grows with it, and nothing is truncated.  At the library's 16 points per occupied
 * cell 4096 cells are a ball of some 28 point spacings of a surface. */
#define SICP_OUTLIER_MAX_BOX_CELLS 4096

int sicp_outlier_version(void);

typedef struct sicp_outlier_stats {
    int64_t n_candidates, n_kept;
    double mean, std, threshold;
} sicp_outlier_stats;

/* rows: host int64, m entries; mask: device memory, n bytes (n = the slot's size); both NULL: every point (m ignored).
 * keep_out: verdict bytes (1 kept, 0 dropped); mean_dist_out (nullable): the d_i; *out: the record (host). */
int sicp_outlier_statistical(sicp_ctx *ctx, int slot, const int64_t *rows, int64_t m, const uint8_t *mask, int k,
                             double std_ratio, uint8_t *keep_out, double *mean_dist_out, sicp_outlier_stats *out);

/* count_out (nullable): min(count_i, min_points + 1) as uint32 (counts are below 2^31); *kept_out: how many were kept. */
int sicp_outlier_radius(sicp_ctx *ctx, int slot, const int64_t *rows, int64_t m, const uint8_t *mask, double radius,
                        int64_t min_points, uint8_t *keep_out, uint32_t *count_out, int64_t *kept_out);

/* The box of grid cells sicp_outlier_radius would walk for this radius on this slot (its grid is built if it has none):
 * out4 = cells along x, y, z and their product.  The call is accepted iff out4[3] <= SICP_OUTLIER_MAX_BOX_CELLS. */
int sicp_outlier_radius_cells(sicp_ctx *ctx, int slot, double radius, int64_t out4[4]);

#ifdef __cplusplus
}
#endif

#endif
