/*
 * simpleicp_hip_regions.h -- companion C ABI of libsimpleicp_hip.so: smooth regions of a cloud -- region growing over the normals
 * (PCL's RegionGrowing, CloudCompare's facet extraction): every patch of the surface, flat or curved, whose neighbouring normals
 * agree gets one label, and patches end where the surface creases.  PCL's result depends on the order of its seed queue; this
 * one depends on the inputs alone.
 *
 * This header includes simpleicp_hip.h and does not change it: SICP_ABI_VERSION stays what it is, these entries have
 * SICP_REGIONS_VERSION of their own.  The conventions of simpleicp_hip.h and simpleicp_hip_fpfh.h hold.  The entry runs on the
 * ctx's stream and is complete on return; `normals`, `seeds` and `labels_out` are host memory or memory of the ctx's device (told
 * apart as sicp_select_in_range tells its output); *out is host memory.
 *
 * ---- contract (J), sicp_regions ----
 * The slot's cloud of n points, 1 <= n < 2^31; normals (n, 3) float32, upcast exactly; 2 <= k <= SICP_FPFH_MAX_K, k <= n; radius:
 * a double > 0, +inf: none; cos_min: a double, 0 <= cos_min <= 1, with `oriented` -1 <= cos_min <= 1; seeds: n bytes, NULL: all
 * ones; min_size >= 1.  Everything is float64, every operation rounded on its own, no fused multiply-add, no libm call.
 *  1. Void points.  Point i is VOID iff a component of its normal is not finite or all three are zero: contract (H)'s rule.  A
 *     void point has no edges and is never labelled.
 *  2. Edges.  {i, j}, i != j, is an EDGE iff j is among ranks 0 .. k-1 of the slot's k-NN search for point i (contracts (D) and
 *     (K)) with d2 < radius * radius, or i among those of j likewise, and neither is void.  radius * radius is one rounded
 *     product and the comparison is strict -- contract (F)'s radius rule; radius = +inf: no test.  Edges are undirected; exact
 *     duplicates are ordinary neighbours.
 *  3. Agreement.  s_ij = (nx_i * nx_j + ny_i * ny_j) + nz_i * nz_j, contract (H)'s weight, symmetric bit for bit; t_ij =
 *     fabs(s_ij), with `oriented` t_ij = s_ij.  An edge LINKS iff t_ij >= cos_min: the comparison is not strict (-0.0 >= 0.0),
 *     and a NaN never links.
 *  4. Smooth points.  Point i is SMOOTH iff it is not void and seeds[i] != 0.  Only smooth points pass a label on.
 *  5. Regions.  The connected components of the smooth points under the linking edges between them.  A region's ROOT is its
 *     lowest index.
 *  6. Border points.  A point that is neither smooth nor void and has a linking edge to a smooth point is a BORDER point of the
 *     region with the lowest root among those smooth neighbours.  The edge may come from either end's list.  A border point
 *     never connects two regions.  A point that is neither smooth, void nor border is LOOSE.
 *  7. Size and survival.  A region's size is the number of its smooth points plus its border points.  It SURVIVES iff
 *     size >= min_size.  The surviving regions are numbered 0, 1, 2, ... in the order of their roots.
 *  8. Labels.  labels_out[i] = the number of i's region if it survives, else -1: every member of a dropped region gets -1 -- its
 *     border points do not fall through to their second choice --, and so does every void and every loose point.
 *  9. The record, all int64.  n_points = n; n_void; n_smooth; n_border (the border points of dropped regions included);
 *     n_regions_all = the regions of step 5; n_regions = those that survive; n_labelled = the labels that are not -1;
 *     largest_label, largest_size: the surviving region with the most members, of equal sizes the lowest label; none: -1 and 0.
 * Every byte of the outputs depends on the inputs alone: no seed, no order of arrival, integer atomics only.
 *
 * Refused with SICP_ERR_INVALID before any device work, the message naming the argument, the outputs untouched: a NULL ctx,
 * normals, labels_out or out (seeds is nullable); a slot that is no slot, is empty or holds a shard; k < 2, k > SICP_FPFH_MAX_K
 * or k > n; radius NaN or not > 0; cos_min NaN, above 1, or below 0 (with `oriented`: below -1); min_size < 1; a ctx with an
 * exchange or an active communicator; 2^31 points or more.
 *
 * No kernel of the call waits for another wave or workgroup (no grid barrier, no flag, no ticket).  Working memory, 4 k + 17
 * bytes per point -- the lists as an (k, n) int32 table (-1: a rank outside the radius), four words of union, root, rank and size,
 * the byte that tells void, smooth and the rest apart -- and up to 17 more where normals, seeds and labels_out are host memory;
 * with the k-NN search's own chunk buffers it stays with the ctx, is shared with sicp_orient and sicp_cluster, is reused from
 * call to call and goes with sicp_ctx_destroy.  (Searching twice and keeping no table would save the 4 k bytes and cost a second
 * k-NN pass, which is most of the call.)  Switch, read at sicp_ctx_create: SICP_REGIONS_CHUNK (points per k-NN search; 0 or
 * unset: chosen per call as sicp_fpfh chooses its own).
 */
#ifndef SIMPLEICP_HIP_REGIONS_H
#define SIMPLEICP_HIP_REGIONS_H

#include "simpleicp_hip.h"
#include "simpleicp_hip_fpfh.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: sicp_regions. */
#define SICP_REGIONS_VERSION 1

int sicp_regions_version(void);

typedef struct sicp_regions_stats {
    int64_t n_points, n_void, n_smooth, n_border, n_regions_all, n_regions, n_labelled, largest_label, largest_size;
} sicp_regions_stats;

/* normals: (n, 3) float32; seeds (nullable): (n) uint8; labels_out: (n) int32; *out: host. */
int sicp_regions(sicp_ctx *ctx, int slot, const float *normals, int k, double radius, double cos_min, int oriented,
                 const uint8_t *seeds, int64_t min_size, int32_t *labels_out, sicp_regions_stats *out);

#ifdef __cplusplus
}
#endif

#endif
