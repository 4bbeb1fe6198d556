// sicp_union_dev.h -- what the units that label connected components share (device code only; sicp_cluster.hip, sicp_regions.hip):
// the lock-free union-find over uint32 parent[n] and the scan of the rank scan's block sums.  Everything has internal linkage:
// every unit that includes it gets functions and a kernel of its own.
#ifndef SICP_UNION_DEV_H
#define SICP_UNION_DEV_H

#include "sicp_lanes.h"

namespace sicp {
namespace {

constexpr int CL_BLOCK = 256;

// ---- the union-find over uint32 parent[n] ---------------------------------------------------------------------------------------
// Every access while unions are in flight is an agent-scope relaxed atomic: the XCDs' L2s are not coherent, a plain load may be
// stale.  (Staleness would not even break it -- an old value of parent[x] is still an ancestor of x, and the compare-and-swap is
// decided where all of them meet -- but it would cost retries.)
__device__ __forceinline__ uint32_t uf_load(uint32_t *parent, uint32_t x)
{
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool uf_cas(uint32_t *parent, uint32_t x, uint32_t &expected, uint32_t desired)
{
    return __hip_atomic_compare_exchange_strong(parent + x, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the root of x; path halving on the way: parent[x] goes from x's parent to its grandparent -- an ancestor of x, nothing else is
// ever written into a word that is not a root -- and a halving that loses its race is skipped
__device__ __forceinline__ uint32_t uf_find(uint32_t *parent, uint32_t x)
{
    uint32_t p = uf_load(parent, x);
    while (p != x) {
        const uint32_t gp = uf_load(parent, p);
        if (gp != p) { uint32_t e = p; (void)uf_cas(parent, x, e, gp); }
        x = p; p = gp;
    }
    return x;
}
// unites the sets of a and b and returns their root: the larger root is hooked under the smaller one, by a compare-and-swap that
// expects it to be a root still; a failure means another lane hooked it first -- start again from where it hangs now
__device__ __forceinline__ uint32_t uf_union(uint32_t *parent, uint32_t a, uint32_t b)
{
    for (;;) {
        a = uf_find(parent, a); b = uf_find(parent, b);
        if (a == b) return a;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        uint32_t e = a;
        if (uf_cas(parent, a, e, b)) return b;
        a = e;
    }
}

// exclusive prefix sum of the nb block sums, in place, by one workgroup; *total = their sum (the number of clusters)
__global__ __launch_bounds__(CL_BLOCK) void k_cl_scan_sums(uint32_t *__restrict__ sums, long nb, unsigned long long *__restrict__ total)
{
    __shared__ uint32_t wtot[CL_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (long base = 0; base < nb; base += CL_BLOCK) {
        const long e = base + threadIdx.x;
        const uint32_t v = e < nb ? sums[e] : 0u;
        const uint32_t inc = wscan_u32(v);
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < CL_BLOCK / 64; ++w) { before += w < wave ? wtot[w] : 0u; all += wtot[w]; }
        if (e < nb) sums[e] = carry + before + inc - v;
        carry += all;
        __syncthreads();                                           // (wtot is written again)
    }
    if (threadIdx.x == 0) *total = carry;
}

}  // namespace
}  // namespace sicp

#endif
