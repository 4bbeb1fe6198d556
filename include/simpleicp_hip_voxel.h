/*
 * simpleicp_hip_voxel.h -- companion C ABI of libsimpleicp_hip.so: spatially even selection, at most one point per
 * voxel of a lattice.
 *
 * This header includes simpleicp_hip.h and does not change it: SICP_ABI_VERSION stays what it is, these entries
 * have SICP_VOXEL_VERSION of their own.  The conventions of simpleicp_hip.h hold.
 *
 * The rule, arithmetic contract (V) of DESIGN.md section 13.  For a cell size c (finite, > 0) and an origin o (three
 * finite doubles):
 *   voxel of a point = ( floor((x - o_x) / c), floor((y - o_y) / c), floor((z - o_z) / c) ), evaluated in float64 with
 *     IEEE subtraction and division in exactly this form (no reciprocal, no FMA): numpy's np.floor((X - o) / c), bit
 *     for bit; -0.0 and points on a lattice plane fall where that formula puts them;
 *   among the candidates, the one with the LOWEST INDEX in each occupied voxel is kept, all others are dropped (two
 *     entries of `rows` naming the same point: the earlier entry).
 * The verdicts depend on the input alone -- not on launch geometry, insertion order or repetition.
 *
 * Refused with SICP_ERR_INVALID: a lattice that spans more than 2^21 cells along an axis over the slot's bounding box
 * (the message names the axis and the extent; nothing is truncated), and a ctx with an exchange (sicp_set_exchange,
 * an active communicator) or a slot that holds a shard -- the lowest index of a voxel may live on another rank.
 *
 * Both entries run on the ctx's stream and are complete on return.  Their hash table (16 bytes per slot, at least
 * two slots per candidate) stays with the ctx, is reused from call to call and goes with sicp_ctx_destroy.
 */
#ifndef SIMPLEICP_HIP_VOXEL_H
#define SIMPLEICP_HIP_VOXEL_H

#include "simpleicp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: sicp_voxel_select, sicp_voxel_select_masked. */
#define SICP_VOXEL_VERSION 1

int sicp_voxel_version(void);

/* The candidates are the m rows `rows` of the slot (host int64; NULL: every point of the slot, m is ignored).
 * origin: three doubles, NULL = (0, 0, 0).  keep_out: m verdict bytes (1 kept, 0 dropped), one per candidate in the
 * order of `rows`, host or device memory (told apart as sicp_select_in_range tells its in_range_out).  *kept_out: how
 * many were kept. */
int sicp_voxel_select(sicp_ctx *ctx, int slot, const int64_t *rows, int64_t m, double cell, const double *origin,
                      uint8_t *keep_out, int64_t *kept_out);

/* The candidates are the points of the slot whose mask byte is non-zero.  mask: device memory, n bytes (n = the
 * slot's size), as sicp_select_in_range leaves its verdicts; keep_out: device memory, n bytes, may alias mask --
 * 1 for a candidate that is kept, 0 for every other point.  The step between sicp_select_in_range and
 * sicp_select_n_device on the device road. */
int sicp_voxel_select_masked(sicp_ctx *ctx, int slot, const uint8_t *mask, int64_t n, double cell, const double *origin,
                             uint8_t *keep_out, int64_t *kept_out);

#ifdef __cplusplus
}
#endif

#endif
