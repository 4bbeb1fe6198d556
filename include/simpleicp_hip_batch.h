/*
 * simpleicp_hip_batch.h -- companion C ABI of libsimpleicp_hip.so: many ICP runs in one call.
 *
 * The reference registers one pair per call and has no batch API; this header adds one beside
 * simpleicp_hip.h (which it includes and does not change: SICP_ABI_VERSION stays what it is, the
 * batch has SICP_BATCH_VERSION of its own).  The conventions of simpleicp_hip.h hold.
 *
 * A batch is a list of members, each a ctx prepared exactly as for sicp_icp_run (both clouds
 * uploaded, sicp_icp_setup done) with that call's arguments.  The members' iterations are
 * enqueued together on the first member's stream: per iteration ONE match launch for every
 * member (a per-block member map over a member table in device memory) and one single-workgroup
 * tail launch per k_icp_tail instantiation present (members grouped by the instantiation a lone
 * run would take for their Q), one workgroup per member.  Up to the members' chain depth of
 * iterations are in flight; the call returns when every member has stopped (converged, failed)
 * or reached its own max_iterations.
 *
 * Contract
 *   - Every member gets exactly what sicp_icp_run(ctx, &params, max_iterations, min_change,
 *     results, &iterations) would give on its own: every field of every result, the iteration
 *     count, the status; its ctx is left in the state that call leaves (sicp_icp_get_state,
 *     sicp_icp_uncertainties, sicp_icp_normal_equations and a later sicp_icp_run answer the same).
 *   - Failures stay per member (status, error); the call returns SICP_OK once every member has
 *     been attempted.
 *   - SICP_ERR_INVALID and nothing launched for: a NULL or empty list, a NULL ctx or results, the
 *     same ctx twice, ctxs on different devices, a member without sicp_icp_setup, a member with an
 *     exchange or communicator attached.
 *   - Members the batched kernels do not cover -- Q > 2048, a forced non-grid 1-NN flavour
 *     (SICP_KNN1), the host solver (SICP_SOLVE=host), timing / work counting / traces on, or
 *     arguments sicp_icp_run would refuse -- run through sicp_icp_run on their own ctx inside the
 *     same call (path = 2) and are counted in *fallback_count.
 */
#ifndef SIMPLEICP_HIP_BATCH_H
#define SIMPLEICP_HIP_BATCH_H

#include "simpleicp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: sicp_icp_run_batch, sicp_batch_member, sicp_ctx_lean. */
#define SICP_BATCH_VERSION 1

#define SICP_BATCH_PATH_BATCHED  1   /* the member ran in the batched launches          */
#define SICP_BATCH_PATH_FALLBACK 2   /* ... through sicp_icp_run on its own ctx          */

typedef struct sicp_batch_member {
    sicp_ctx *ctx;               /* both clouds uploaded, sicp_icp_setup done                      */
    sicp_iter_params params;     /* as for sicp_icp_run                                            */
    int64_t max_iterations;
    double  min_change;
    sicp_iter_result *results;   /* max_iterations entries, caller-owned (host memory)             */
    int64_t iterations;          /* out                                                            */
    int     status;              /* out: SICP_OK / SICP_ERR_TOO_FEW / SICP_ERR_NUMERIC / ...        */
    int     path;                /* out: SICP_BATCH_PATH_*                                         */
    char    error[256];          /* out: what sicp_last_error() would say after a lone run's failure
                                    ("" on SICP_OK)                                                */
} sicp_batch_member;

int sicp_batch_version(void);

/* Makes ctx a lean batch member: its staged uploads and sicp_cloud_download_both go through ONE pinned
 * ring that all lean contexts of the process share (48 MiB of pinned host memory per process instead of
 * per ctx; calls that use it are serialised across lean contexts). */
int sicp_ctx_lean(sicp_ctx *ctx);

/* Runs every member's loop (see above).  fallback_count (nullable): members that took the
 * sicp_icp_run path. */
int sicp_icp_run_batch(sicp_batch_member *members, int64_t count, int64_t *fallback_count);

#ifdef __cplusplus
}
#endif

#endif
