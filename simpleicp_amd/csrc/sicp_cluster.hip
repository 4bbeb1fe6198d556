// sicp_cluster.hip -- DBSCAN labels of a cloud (include/simpleicp_hip_cluster.h; contract (U)).
//
// Core flags: the radius filter's k_ball_count (sicp_outlier.hip, through ball_count_enqueue) with cap = min_points.  Union: k_ball_union
// walks every core point's ball (ball_walk: sicp_ball_dev.h) and unites it with the core hits of lower index in a lock-free union-find
// (uf_find / uf_union: a root is only ever hooked under a smaller root, so a component's root ends up its lowest core index whatever
// the order of arrival).  k_cl_flatten leaves every core point's root and the block sums of the root flags; k_ball_border gives a
// point that is not core the smallest root among its core hits; k_cl_scan_sums / k_cl_apply rank the roots in index order (the
// labels); k_cl_labels writes the labels, counts border and noise and adds up the clusters' sizes; k_cl_largest finds the largest.
// No kernel waits for another wave or workgroup: the only loops over memory another wave writes are uf_find's walk towards a root
// (parents only ever decrease) and uf_union's retry after a failed compare-and-swap (another lane's succeeded).  Integer atomics only.
#include "sicp_host.h"
#include "sicp_ball_dev.h"
#include "sicp_union_dev.h"
#include "../../include/simpleicp_hip_cluster.h"

namespace sicp {
namespace {

constexpr int CL_PER = 4;                          // consecutive points per thread of k_cl_flatten / k_cl_apply
constexpr int CL_SPAN = CL_BLOCK * CL_PER;         // points per workgroup of the rank scan
constexpr int CL_RUN = 16;                         // consecutive rows of 64 points per wave of k_cl_labels
constexpr int CL_MAX_BLOCKS = 1024;
constexpr uint32_t CL_NONE = 0xffffffffu;          // root of a point without a cluster

__global__ __launch_bounds__(CL_BLOCK) void k_cl_fill(uint32_t *__restrict__ parent, long n)
{
    const long stride = (long)gridDim.x * CL_BLOCK;
    for (long e = (long)blockIdx.x * CL_BLOCK + threadIdx.x; e < n; e += stride) parent[e] = (uint32_t)e;
}

// ---- the two walks (ball_group_point, ball_walk: sicp_ball_dev.h; neither ever has enough: the visitors answer 1) ------------
// Every core point i of the chunk [lo, lo + Q) is united with its core neighbours j < i (each edge is seen once, from its higher
// end).  ri: the root of i as far as the group knows; a hit that is that root, or whose root is, costs no write.
__global__ __launch_bounds__(BALL_BLOCK) void k_ball_union(const double *__restrict__ qx, const double *__restrict__ qy,
                                                           const double *__restrict__ qz, const uint32_t *__restrict__ order,
                                                           const uint32_t *__restrict__ cell_start, const double4 *__restrict__ rec,
                                                           const uint8_t *__restrict__ core, uint32_t *parent, long Q, long lo, GridGeom G,
                                                           double r, double r2)
{
    const int lane = threadIdx.x & 63, sub = lane & (BALL_GS - 1), gbase = lane & ~(BALL_GS - 1);
    const long q = ball_group_point(order, Q);
    if (q < 0) return;
    const uint32_t i = (uint32_t)(lo + q);
    if (!core[i]) return;
    uint32_t ri = i;
    ball_walk(cell_start, rec, G, qx[q], qy[q], qz[q], r, r2, sub, gbase, [&](bool h0, uint32_t j0, bool h1, uint32_t j1) {
        uint32_t mine = ri;
        if (h0 && j0 < i && j0 != mine && core[j0]) {
            const uint32_t rj = uf_find(parent, j0);
            if (rj != mine) mine = uf_union(parent, mine, rj);
        }
        if (h1 && j1 < i && j1 != mine && core[j1]) {
            const uint32_t rj = uf_find(parent, j1);
            if (rj != mine) mine = uf_union(parent, mine, rj);
        }
        ri = gmin<BALL_GS>(mine);                                  // (every lane's root is one of i's set: the smallest is the newest)
        return 1u;
    });
}

// root[i] of the core points (the others': CL_NONE until k_ball_border), and per workgroup of CL_SPAN points the number of roots.
// The kernel boundary is behind the unions; the finds still halve paths (a chain hooked in one volley is as long as the volley),
// so they keep the atomic accesses.
__global__ __launch_bounds__(CL_BLOCK) void k_cl_flatten(const uint8_t *__restrict__ core, uint32_t *parent, uint32_t *__restrict__ root,
                                                         long n, uint32_t *__restrict__ sums)
{
    const long base = (long)blockIdx.x * CL_SPAN + (long)threadIdx.x * CL_PER;
    unsigned roots = 0;
#pragma unroll
    for (int u = 0; u < CL_PER; ++u) {
        const long e = base + u;
        if (e < n) {
            const uint32_t rt = core[e] ? uf_find(parent, (uint32_t)e) : CL_NONE;
            root[e] = rt;
            roots += rt == (uint32_t)e ? 1u : 0u;
        }
    }
    roots = block_sum_u32<CL_BLOCK / 64>(roots);
    if (threadIdx.x == 0) sums[blockIdx.x] = roots;
}

// A point of the chunk that is not core takes the smallest root among its core neighbours (root order is label order); none: noise.
__global__ __launch_bounds__(BALL_BLOCK) void k_ball_border(const double *__restrict__ qx, const double *__restrict__ qy,
                                                            const double *__restrict__ qz, const uint32_t *__restrict__ order,
                                                            const uint32_t *__restrict__ cell_start, const double4 *__restrict__ rec,
                                                            const uint8_t *__restrict__ core, uint32_t *root, long Q, long lo, GridGeom G,
                                                            double r, double r2)
{
    const int lane = threadIdx.x & 63, sub = lane & (BALL_GS - 1), gbase = lane & ~(BALL_GS - 1);
    const long q = ball_group_point(order, Q);
    if (q < 0) return;
    const long i = lo + q;
    if (core[i]) return;
    uint32_t best = CL_NONE;
    ball_walk(cell_start, rec, G, qx[q], qy[q], qz[q], r, r2, sub, gbase, [&](bool h0, uint32_t j0, bool h1, uint32_t j1) {
        // (root[j] of a core point was written by k_cl_flatten; this kernel writes the others' words only)
        if (h0 && core[j0]) { const uint32_t rj = root[j0]; best = rj < best ? rj : best; }
        if (h1 && core[j1]) { const uint32_t rj = root[j1]; best = rj < best ? rj : best; }
        return 1u;
    });
    best = gmin<BALL_GS>(best);
    if (sub == 0) root[i] = best;
}

// rank[i] of every root i: the number of roots below it -- its cluster's label; size[label] = 0 for k_cl_labels to add to
__global__ __launch_bounds__(CL_BLOCK) void k_cl_apply(const uint32_t *__restrict__ root, long n, const uint32_t *__restrict__ sums,
                                                       uint32_t *__restrict__ rank, uint32_t *__restrict__ size)
{
    __shared__ uint32_t wtot[CL_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long base = (long)blockIdx.x * CL_SPAN + (long)threadIdx.x * CL_PER;
    bool f[CL_PER];
    uint32_t cnt = 0;
#pragma unroll
    for (int u = 0; u < CL_PER; ++u) {
        const long e = base + u;
        f[u] = e < n && root[e] == (uint32_t)e;
        cnt += f[u] ? 1u : 0u;
    }
    const uint32_t inc = wscan_u32(cnt);
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    uint32_t at = sums[blockIdx.x] + inc - cnt;
#pragma unroll
    for (int w = 0; w < CL_BLOCK / 64; ++w) at += w < wave ? wtot[w] : 0u;
#pragma unroll
    for (int u = 0; u < CL_PER; ++u)
        if (f[u]) { rank[base + u] = at; size[at] = 0u; ++at; }
}

// counter words of the call (c->cand_small)
enum { CL_CORE = 0, CL_BORDER = 1, CL_NOISE = 2, CL_CLUSTERS = 3, CL_BEST = 4 };

// labels[i] = rank[root[i]] or -1; core, border and noise counted by ballots, one atomic per wave and counter; the clusters' sizes by
// integer atomics, one per run of equal labels a wave meets in its CL_RUN rows of 64 consecutive points
__global__ __launch_bounds__(CL_BLOCK) void k_cl_labels(const uint8_t *__restrict__ core, const uint32_t *__restrict__ root,
                                                        const uint32_t *__restrict__ rank, long n, int32_t *__restrict__ labels,
                                                        uint32_t *__restrict__ size, unsigned long long *__restrict__ counters)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long wbase = ((long)blockIdx.x * (CL_BLOCK / 64) + wave) * (CL_RUN * 64);
    unsigned n_core = 0, n_border = 0, n_noise = 0;
    uint32_t run_label = CL_NONE, run = 0;                         // (wave-uniform)
    for (int it = 0; it < CL_RUN && wbase + it * 64 < n; ++it) {
        const long e = wbase + it * 64 + lane;
        const bool in = e < n;
        const uint32_t rt = in ? root[e] : CL_NONE;
        const bool has = rt != CL_NONE;
        const uint32_t lab = has ? rank[rt] : CL_NONE;
        if (in) labels[e] = has ? (int32_t)lab : -1;
        const bool is_core = in && core[e] != 0;
        n_core += (unsigned)__popcll((long long)__ballot(is_core));
        n_noise += (unsigned)__popcll((long long)__ballot(in && !has));
        n_border += (unsigned)__popcll((long long)__ballot(has && !is_core));
        unsigned long long todo = __ballot(has);
        while (todo) {
            const int first = __ffsll((long long)todo) - 1;
            const uint32_t l = (uint32_t)__builtin_amdgcn_readlane((int)lab, first);
            const unsigned long long same = __ballot(has && lab == l);
            const uint32_t m = (uint32_t)__popcll((long long)same);
            if (l == run_label) {
                run += m;
            } else {
                if (run && lane == 0) atomicAdd(size + run_label, run);
                run_label = l; run = m;
            }
            todo &= ~same;
        }
    }
    if (lane == 0) {
        if (run) atomicAdd(size + run_label, run);
        if (n_core) atomicAdd(counters + CL_CORE, (unsigned long long)n_core);
        if (n_border) atomicAdd(counters + CL_BORDER, (unsigned long long)n_border);
        if (n_noise) atomicAdd(counters + CL_NOISE, (unsigned long long)n_noise);
    }
}

// the largest cluster: max over the labels of (size << 32 | ~label) -- of equal sizes the lowest label wins
__global__ __launch_bounds__(CL_BLOCK) void k_cl_largest(const uint32_t *__restrict__ size, unsigned long long *counters)
{
    const unsigned long long clusters = counters[CL_CLUSTERS];     // (k_cl_scan_sums's, a kernel boundary ago)
    const unsigned long long stride = (unsigned long long)gridDim.x * CL_BLOCK;
    unsigned long long best = 0;
    for (unsigned long long l = (unsigned long long)blockIdx.x * CL_BLOCK + threadIdx.x; l < clusters; l += stride) {
        const unsigned long long key = ((unsigned long long)size[l] << 32) | (unsigned long long)(CL_NONE - (uint32_t)l);
        best = key > best ? key : best;
    }
    unsigned long long o;
    o = lane_xor64<32>(best); best = o > best ? o : best;
    o = lane_xor64<16>(best); best = o > best ? o : best;
    o = lane_xor64<8>(best);  best = o > best ? o : best;
    o = lane_xor64<4>(best);  best = o > best ? o : best;
    o = lane_xor64<2>(best);  best = o > best ? o : best;
    o = lane_xor64<1>(best);  best = o > best ? o : best;
    if ((threadIdx.x & 63) == 0 && best) atomicMax(counters + CL_BEST, best);
}

}  // namespace
}  // namespace sicp

namespace {

static_assert(CL_BEST < CAND_WORDS, "the record's counters fit the ctx's counter words");

}  // namespace

SICP_EXPORT int sicp_cluster_version(void) { return SICP_CLUSTER_VERSION; }

SICP_EXPORT int sicp_cluster(sicp_ctx *c, int slot, double radius, int64_t min_points, int32_t *labels_out, uint8_t *core_out,
                             sicp_cluster_stats *out)
{
    CHK(check_slot(c, slot, true));
    if (!labels_out) return fail(SICP_ERR_INVALID, "labels_out is null");
    if (!out) return fail(SICP_ERR_INVALID, "out is null");
    if (!std::isfinite(radius) || !(radius > 0.0)) return fail(SICP_ERR_INVALID, "radius must be finite and > 0");
    if (min_points < 1) return fail(SICP_ERR_INVALID, "min_points must be >= 1");
    CHK(check_whole_cloud(c, slot, "clustering", "a point's neighbours may live on another rank"));
    HIPCHK(hipSetDevice(c->device));
    return op_run(c, [&]() -> int {
        GridLevel lv;
        CHK(ball_level(c, slot, radius, &lv));
        const long n = (long)c->cloud[slot].n, nb = cdiv(n, CL_SPAN);
        CHK(c->cand_keep.reserve((size_t)n));
        CHK(c->ol_cnt.reserve((size_t)n));
        CHK(c->cl_parent.reserve((size_t)n));
        CHK(c->cl_root.reserve((size_t)n));
        CHK(c->cl_rank.reserve((size_t)(n + nb)));
        CHK(c->cl_size.reserve((size_t)n));
        CHK(c->cl_labels.reserve((size_t)n));
        CHK(counters_clear(c));
        uint8_t *core = c->cand_keep.p;
        uint32_t *parent = c->cl_parent.p, *root = c->cl_root.p, *rank = c->cl_rank.p, *sums = c->cl_rank.p + n;
        unsigned long long *counters = c->cand_small.p;
        const double r2 = radius * radius;
        const unsigned cap = (unsigned)std::min<int64_t>(min_points, 1LL << 31);       // counts stay below 2^31
        BallChunks W{c, slot, lv, nullptr, n, c->cluster_chunk};
        CHK(W.reserve());
        const dim3 flat(std::min(cdiv(n, CL_BLOCK), (unsigned)CL_MAX_BLOCKS));
        // core flags
        for (long lo = 0; lo < n; lo += W.chunk) {
            const long cnt = std::min(W.chunk, n - lo);
            CHK(W.enter(lo, cnt));
            // (no count from the kernel: its one atomic per wave on one word costs more than the walk where most points are core)
            CHK(ball_count_enqueue(W, nullptr, cnt, radius, cap, core + lo, c->ol_cnt.p + lo, nullptr));
        }
        // unions
        hipLaunchKernelGGL(k_cl_fill, flat, dim3(CL_BLOCK), 0, c->stream, parent, n);
        for (long lo = 0; lo < n; lo += W.chunk) {
            const long cnt = std::min(W.chunk, n - lo);
            CHK(W.enter(lo, cnt));
            hipLaunchKernelGGL(k_ball_union, dim3(W.grid(cnt)), dim3(BALL_BLOCK), 0, c->stream, W.qx(), W.qy(), W.qz(), W.order, lv.cell_start,
                               (const double4 *)lv.rec, core, parent, cnt, lo, lv.g, radius, r2);
            HIPCHK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_cl_flatten, dim3((unsigned)nb), dim3(CL_BLOCK), 0, c->stream, core, parent, root, n, sums);
        // borders
        for (long lo = 0; lo < n; lo += W.chunk) {
            const long cnt = std::min(W.chunk, n - lo);
            CHK(W.enter(lo, cnt));
            hipLaunchKernelGGL(k_ball_border, dim3(W.grid(cnt)), dim3(BALL_BLOCK), 0, c->stream, W.qx(), W.qy(), W.qz(), W.order, lv.cell_start,
                               (const double4 *)lv.rec, core, root, cnt, lo, lv.g, radius, r2);
            HIPCHK(hipGetLastError());
        }
        // ranks, labels, record
        hipLaunchKernelGGL(k_cl_scan_sums, dim3(1), dim3(CL_BLOCK), 0, c->stream, sums, nb, counters + CL_CLUSTERS);
        hipLaunchKernelGGL(k_cl_apply, dim3((unsigned)nb), dim3(CL_BLOCK), 0, c->stream, root, n, sums, rank, c->cl_size.p);
        hipLaunchKernelGGL(k_cl_labels, dim3(cdiv(n, CL_RUN * CL_BLOCK)), dim3(CL_BLOCK), 0, c->stream, core, root, rank, n, c->cl_labels.p,
                           c->cl_size.p, counters);
        hipLaunchKernelGGL(k_cl_largest, flat, dim3(CL_BLOCK), 0, c->stream, c->cl_size.p, counters);
        HIPCHK(hipGetLastError());
        CHK(counters_fetch(c));
        // the outputs leave through the staging buffers, host or device memory alike
        HIPCHK(hipMemcpyAsync(labels_out, c->cl_labels.p, (size_t)n * sizeof(int32_t), hipMemcpyDefault, c->stream));
        if (core_out) HIPCHK(hipMemcpyAsync(core_out, core, (size_t)n, hipMemcpyDefault, c->stream));
        CHK(sync(c));
        const unsigned long long *h = counters_host(c);
        out->n_points = (int64_t)n;
        out->n_core = (int64_t)h[CL_CORE];
        out->n_border = (int64_t)h[CL_BORDER];
        out->n_noise = (int64_t)h[CL_NOISE];
        out->n_clusters = (int64_t)h[CL_CLUSTERS];
        out->largest_label = h[CL_CLUSTERS] ? (int64_t)(0xffffffffu - (uint32_t)h[CL_BEST]) : -1;
        out->largest_size = h[CL_CLUSTERS] ? (int64_t)(h[CL_BEST] >> 32) : 0;
        return SICP_OK;
    });
}
