/*
 * simpleicp_hip_normals.h -- companion C ABI of libsimpleicp_hip.so: rejection of correspondences by the angle
 * between the normals of the fixed point and of its matched movable point.
 *
 * This header includes simpleicp_hip.h and does not change it: SICP_ABI_VERSION stays what it is, these entries
 * have SICP_NORMALS_VERSION of their own.  The conventions of simpleicp_hip.h hold.
 *
 * The rule, arithmetic contract (N) of DESIGN.md section 3.  For correspondence q with matched movable point m
 * (global index) under the iteration's H:
 *   n1  = the fixed point's normal (sicp_icp_setup), float32 upcast to float64;
 *   n2  = the normal of movable point m in the movable cloud's OWN frame, float32 upcast;
 *   n2' = R n2, R = H[:3,:3], each component (R_i0 * n2x + R_i1 * n2y) + R_i2 * n2z, every operation rounded;
 *   c   = (n1x * n2'x + n1y * n2'y) + n1z * n2'z;
 *   keep iff fabs(c) >= cos_max (normals are unoriented; NaN fails).
 * Inside an iteration it is a row filter applied together with the planarity test, BEFORE median / MAD.
 *
 * Where n2 comes from: the column set by sicp_cloud_set_normals when the slot has one, else a per-point cache on
 * the device that is filled on demand: the normal of point m is what sicp_estimate_normals(ctx, SICP_MOV, {m}, k,
 * ...) returns, bit for bit (k nearest neighbours among ALL points resident in the slot, self included).  The
 * cache is allocated when the rejection is first used on the ctx (12 bytes + 1 bit per point of the slot) and
 * emptied by an upload or sicp_cloud_transform of the slot, or when k changes.
 *
 * Not supported, refused with SICP_ERR_INVALID: a ctx with an exchange (sicp_set_exchange, an active
 * communicator) -- the matched point may live on another rank.  sicp_icp_run_batch sends a member whose ctx has the
 * rejection on down its fallback road (sicp_icp_run on its own ctx, counted in fallback_count).
 */
#ifndef SIMPLEICP_HIP_NORMALS_H
#define SIMPLEICP_HIP_NORMALS_H

#include "simpleicp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: sicp_cloud_set_normals, sicp_normal_angle_set, sicp_corr_reject_normal_angle, sicp_normal_angle_info,
 *    sicp_normal_cache_read. */
#define SICP_NORMALS_VERSION 1

int sicp_normals_version(void);

/* The cloud's normal columns (nx, ny, nz) by GLOBAL point index, with the semantics of sicp_cloud_set_planarity:
 * rows == NULL: normals is a dense (n_global, 3) float32 block (m == n_global); else m (row, normal) pairs, NaN
 * elsewhere.  normals == NULL: the cloud has no such columns (the state after every upload of the slot). */
int sicp_cloud_set_normals(sicp_ctx *ctx, int slot, const int64_t *rows, const float *normals /* (m,3) */, int64_t m,
                           int64_t n_global);

/* A ctx setting that sicp_icp_run and sicp_icp_iterate honour: reject by contract (N) with this cos_max; k: the
 * neighbourhood of the on-demand normals (2 <= k <= 128; unused when the movable slot has normal columns).
 * cos_max NaN or <= 0: off -- the state of a new ctx; nothing is launched or allocated for it then. */
int sicp_normal_angle_set(sicp_ctx *ctx, double cos_max, int k);

/* The operator (after sicp_corr_match, in any order with the other two rejections): correspondences whose normals
 * fail (N) under H (row-major 4x4; NULL = identity) die.  pc2_normals: (Q,3) float32 per correspondence, or NULL =
 * the movable slot's columns / the on-demand cache as above.  *n_alive_out: correspondences still alive. */
int sicp_corr_reject_normal_angle(sicp_ctx *ctx, double cos_max, int k, const double *H, const float *pc2_normals,
                                  int64_t *n_alive_out);

/* Since sicp_icp_setup: out4[0] normals estimated on demand (cache entries filled), [1] correspondences the verdict
 * dropped in the last iteration (or operator call), [2] bytes of the cache, 12 n + 4 ceil(n / 32) (0: none), [3] iterations whose miss
 * list was empty. */
int sicp_normal_angle_info(sicp_ctx *ctx, int64_t out4[4]);

/* DIAGNOSTIC, for tests -- it downloads the whole cache; not for a hot path.  The movable slot's cache as it stands: normals_out (n,3) float32 by local index, have_out n bytes -- 1: the
 * point's normal has been estimated (it may be NaN), 0: not yet (its row of normals_out is NaN).  No cache: all 0. */
int sicp_normal_cache_read(sicp_ctx *ctx, float *normals_out, uint8_t *have_out);

#ifdef __cplusplus
}
#endif

#endif
