/*
 * simpleicp_hip_farthest.h -- companion C ABI of libsimpleicp_hip.so: farthest point sampling -- exactly m points of a cloud,
 * evenly spread in space, one pick after the other, each the point farthest from those already taken.  Open3D's
 * farthest_point_down_sample, pytorch3d's sample_farthest_points, the sampling layer of the PointNet++ family; what
 * `correspondences = 1000` asks of a selection: a count, not a cell size.
 *
 * This header includes simpleicp_hip.h and does not change it: SICP_ABI_VERSION stays what it is, these entries have
 * SICP_FARTHEST_VERSION of their own.  The conventions of simpleicp_hip.h and simpleicp_hip_plane.h hold.  The entry touches no
 * cloud slot: the ctx gives its stream and its buffers.  It runs on the ctx's stream and is complete on return; every array pointer
 * is host memory or memory of the ctx's device (told apart as sicp_plane_triplets tells its pointers apart); *out is host memory.
 *
 * ---- contract (S), sicp_farthest ----
 * X (n, 3) float64 rows; mask (n) uint8, nullable; 1 <= n < 2^31; 1 <= m <= n; -1 <= start < n.  Everything is float64, every
 * operation rounded on its own except the two fused multiply-adds named below; no libm call takes part.
 *  1. Candidates.  Row i is a CANDIDATE iff its mask byte is non-zero (NULL mask: every row) and its three coordinates are finite.
 *  2. Distance.  d2(i, s) is contract (D) as it stands: dx = x_i - x_s, dy = y_i - y_s, dz = z_i - z_s,
 *         d2 = fma(dz, dz, fma(dy, dy, dx * dx))
 *     (one multiplication, two fused multiply-adds).  It may overflow to +inf; it is never NaN (the coordinates are finite) and
 *     never -0.0.
 *  3. First pick.  s_0 = start; start == -1: s_0 is the lowest-index candidate.  If start >= 0 is not a candidate, or there is no
 *     candidate, nothing is selected: n_selected = 0.  D_0 = +inf.  m_i = d2(i, s_0) for every candidate i.
 *  4. Pick t = 1, 2, ..., while t < m.  s_t is the candidate with the largest m_i; of equal values, the lowest index.  It is taken
 *     only if m_{s_t} > 0; otherwise the selection ends with n_selected = t.  (So a row is never taken twice, and an exact
 *     duplicate of a taken row is never taken: m of both is 0.)  D_t = m_{s_t}.  Then, for every candidate i,
 *         m_i = (d2(i, s_t) < m_i) ? d2(i, s_t) : m_i.
 *     A selection that is not ended has n_selected = m.
 *  5. Outputs.  idx_out[t] = s_t and d2_out[t] = D_t for t < n_selected; the entries from n_selected on are -1 and +0.0.  D_1, D_2,
 *     ... never increase: D_t is the covering radius (squared) of the picks 0 .. t-1 over the candidates.
 *  6. The record.  n_points = n; n_candidates = the candidates of step 1; n_selected; cover_d2 = the largest m_i after the last
 *     pick: +0.0 without a pick, possibly +inf.
 * A sequence, not a set: the first k picks of a call for m are the call for k.  Every byte of the outputs depends on the inputs
 * alone -- not on the path taken (below), the grid or the order of arrival; no floating-point atomic takes part.
 *
 * Refused with SICP_ERR_INVALID before any device work, the message naming the argument, the outputs untouched: a NULL ctx, X,
 * idx_out or out (mask and d2_out are nullable); n < 1 or n >= 2^31; m < 1 or m > n; start < -1 or start >= n; a ctx with an
 * exchange or an active communicator.
 *
 * Two paths give the same bytes.  Up to SICP_FARTHEST_ONE_MAX rows (at most SICP_FARTHEST_ONE_LIMIT) one workgroup holds the cloud
 * and every m_i in registers and makes all m picks in one launch; beyond, one launch per pick updates m_i in device memory (8 bytes
 * a row, with the workgroups' partial maxima and the staged copy of whatever array is host memory they stay with the ctx and go
 * with sicp_ctx_destroy), all m enqueued without a host round trip.  Switches, read at sicp_ctx_create: SICP_FARTHEST_ONE_MAX (the
 * largest n on the single-workgroup path; 0: never), SICP_FARTHEST_SPAN (rows a workgroup of the stepped path takes, rounded up
 * to whole waves of 64; tests; 0 or unset: chosen per call).
 */
#ifndef SIMPLEICP_HIP_FARTHEST_H
#define SIMPLEICP_HIP_FARTHEST_H

#include "simpleicp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: sicp_farthest. */
#define SICP_FARTHEST_VERSION 1

/* Most rows the single-workgroup path holds: 1 024 lanes of 12 rows each. */
#define SICP_FARTHEST_ONE_LIMIT 12288

int sicp_farthest_version(void);

typedef struct sicp_farthest_stats { int64_t n_points, n_candidates, n_selected; double cover_d2; } sicp_farthest_stats;

/* idx_out: (m) int64; d2_out (nullable): (m) float64; *out: the record (host). */
int sicp_farthest(sicp_ctx *ctx, const double *X, const uint8_t *mask, int64_t n, int64_t m, int64_t start,
                  int64_t *idx_out, double *d2_out, sicp_farthest_stats *out);

#ifdef __cplusplus
}
#endif

#endif
