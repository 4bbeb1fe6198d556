/*
 * simpleicp_hip_chain.h -- companion C ABI of libsimpleicp_hip.so: what the device-chained loop of the last run did.
 *
 * This header includes simpleicp_hip.h and does not change it: SICP_ABI_VERSION stays what it is, these entries
 * have SICP_CHAIN_VERSION of their own.  The conventions of simpleicp_hip.h hold.
 *
 * A chained run of few correspondences (one tail workgroup per iteration) on one GPU hands over from the tail of an
 * iteration to the match of the next through a ticket in device memory: the match is launched early on a second
 * stream of the ctx and waits for that ticket instead of a kernel boundary ("The tail -> match
 * hand-over").  Results are the single-stream chain's, bit for bit; SICP_CHAIN_PRELAUNCH=0 in the environment of
 * sicp_ctx_create keeps the single-stream chain.
 */
#ifndef SIMPLEICP_HIP_CHAIN_H
#define SIMPLEICP_HIP_CHAIN_H

#include "simpleicp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SICP_CHAIN_VERSION 1

int sicp_chain_version(void);
/* out2[0]: matches launched early (waiting for a ticket) in the last sicp_icp_run / sicp_icp_iterate of this ctx -- 0 when
 * the run took the single-stream chain --, out2[1]: since the ctx was created. */
int sicp_chain_info(sicp_ctx *ctx, int64_t out2[2]);

#ifdef __cplusplus
}
#endif
#endif /* SIMPLEICP_HIP_CHAIN_H */
