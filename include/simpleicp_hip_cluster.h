/*
 * simpleicp_hip_cluster.h -- companion C ABI of libsimpleicp_hip.so: density-based clustering of a cloud (DBSCAN labels).
 *
 * This header includes simpleicp_hip.h and does not change it: SICP_ABI_VERSION stays what it is, these entries
 * have SICP_CLUSTER_VERSION of their own.  The conventions of simpleicp_hip.h hold.
 *
 * The rules, arithmetic contract (U) of DESIGN.md section 23.
 *
 * Neighbours.  j is a neighbour of i iff d2(i, j) < radius * radius: d2 is contract (D)'s
 * fma(dz, dz, fma(dy, dy, dx * dx)) of the coordinate differences, the square one rounded multiplication, the
 * comparison strict -- the radius filter's test (contract (O), simpleicp_hip_outlier.h).  The differences negate
 * exactly, so the relation is symmetric bit for bit; i is its own neighbour.
 *
 *   core_i    i has at least min_points neighbours, itself included (min_points = 1: every point is core)
 *   clusters  the connected components of the core points under the neighbour relation.  A component's label is
 *             the number of components whose lowest core index is smaller: labels are 0, 1, 2, ... in the order of
 *             each cluster's first core point
 *   border    a point that is not core and has a core neighbour takes the smallest label among its core neighbours'
 *             clusters; it never connects two clusters
 *   noise     every other point: label -1
 *
 * The result is unique: no seed, no floating-point atomic and no order of arrival has a say in any byte of it.
 * Where no pair of points lies at exactly `radius` it is sklearn.cluster.DBSCAN(eps = radius,
 * min_samples = min_points).fit(X).labels_, cluster order and border assignment included (sklearn and Open3D
 * compare with <=).
 *
 * labels_out (n int32) and core_out (n bytes, 1 = core; nullable) are host or device memory (told apart as
 * sicp_select_in_range tells its in_range_out) and leave through staging buffers, as the outlier filters' outputs do.
 *
 * Refused with SICP_ERR_INVALID before any device work, the message naming the argument: a NULL labels_out or out;
 * radius not finite or <= 0; min_points < 1; an empty slot or a shard; a ctx with an exchange or an active
 * communicator; a cloud of 2^31 points or more.  Refused likewise once the slot's grid is there (it is built if the slot
 * has none, as the radius filter builds it), before anything is computed or written: a ball whose box of grid cells is
 * larger than SICP_OUTLIER_MAX_BOX_CELLS -- the radius filter's rule on the same grid, so sicp_outlier_radius_cells
 * (simpleicp_hip_outlier.h) tells whether a call will be accepted.
 *
 * The call runs on the ctx's stream and is complete on return.  No kernel of it waits for another wave or workgroup
 * (no grid barrier, no flag, no ticket), so it runs beside anything the threading rules of INTEGRATION.md allow.
 * Its scratch -- 25 bytes per point: 17 of working memory (parent, root, rank and size words, the core byte) and 8 of staging
 * (the labels, the capped counts) -- stays with the ctx and goes with sicp_ctx_destroy.
 */
#ifndef SIMPLEICP_HIP_CLUSTER_H
#define SIMPLEICP_HIP_CLUSTER_H

#include "simpleicp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: sicp_cluster. */
#define SICP_CLUSTER_VERSION 1

int sicp_cluster_version(void);

/* n_points = n_core + n_border + n_noise.  largest_label / largest_size: the cluster with the most members (core and
 * border), of equal sizes the lowest label; no cluster at all: -1 and 0. */
typedef struct sicp_cluster_stats {
    int64_t n_points, n_core, n_border, n_noise, n_clusters, largest_label, largest_size;
} sicp_cluster_stats;

/* labels_out: the label of every point of the slot (-1: noise); core_out (nullable): 1 where the point is core;
 * *out: the record (host). */
int sicp_cluster(sicp_ctx *ctx, int slot, double radius, int64_t min_points, int32_t *labels_out, uint8_t *core_out,
                 sicp_cluster_stats *out);

#ifdef __cplusplus
}
#endif

#endif
