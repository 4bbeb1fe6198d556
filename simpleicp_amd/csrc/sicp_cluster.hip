// sicp_cluster.hip -- DBSCAN labels of a cloud (include/simpleicp_hip_cluster.h; contract (U)).
//
// Core flags: the radius filter's k_ball_count (sicp_outlier.hip, through ball_count_enqueue) with cap = min_points.  Union: k_ball_union
// walks every core point's ball with CL_GS lanes and unites it with the core hits of lower index in a lock-free union-find
// (uf_find / uf_union: a root is only ever hooked under a smaller root, so a component's root ends up its lowest core index whatever
// the order of arrival).  k_cl_flatten leaves every core point's root and the block sums of the root flags; k_ball_border gives a
// point that is not core the smallest root among its core hits; k_cl_scan_sums / k_cl_apply rank the roots in index order (the
// labels); k_cl_labels writes the labels, counts border and noise and adds up the clusters' sizes; k_cl_largest finds the largest.
// No kernel waits for another wave or workgroup: the only loops over memory another wave writes are uf_find's walk towards a root
// (parents only ever decrease) and uf_union's retry after a failed compare-and-swap (another lane's succeeded).  Integer atomics only.
#include "sicp_host.h"
#include "sicp_grid_dev.h"
#include "../../include/simpleicp_hip_cluster.h"

namespace sicp {
namespace {

constexpr int CL_BLOCK = 256;
constexpr int CL_GS = 16;                          // lanes per point of the two walks (k_ball_count's OL_GS: a group is one DPP row)
constexpr int CL_PER = 4;                          // consecutive points per thread of k_cl_flatten / k_cl_apply
constexpr int CL_SPAN = CL_BLOCK * CL_PER;         // points per workgroup of the rank scan
constexpr int CL_RUN = 16;                         // consecutive rows of 64 points per wave of k_cl_labels
constexpr int CL_MAX_BLOCKS = 1024;
constexpr uint32_t CL_NONE = 0xffffffffu;          // root of a point without a cluster

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

__global__ __launch_bounds__(CL_BLOCK) void k_cl_fill(uint32_t *__restrict__ parent, long n)
{
    const long stride = (long)gridDim.x * CL_BLOCK;
    for (long e = (long)blockIdx.x * CL_BLOCK + threadIdx.x; e < n; e += stride) parent[e] = (uint32_t)e;
}

// ---- the ball walk ----------------------------------------------------------------------------------------------------------------
// k_ball_count's walk (sicp_outlier.hip) without its early exit: the CL_GS lanes of a group fetch the record ranges of CL_GS rows of
// the ball's box at once, culled to the ball along x (row_lb2, row_x_clip, row_records: sicp_grid_dev.h), then take the records of
// one row after the other, two per lane and step.  hit(h0, j0, h1, j1), called by all lanes of the group together: is the lane's
// record a neighbour (d2 < r2, contract (D)), and its original index.
template <class Hit>
__device__ __forceinline__ void ball_walk(const uint32_t *__restrict__ cell_start, const double4 *__restrict__ rec, const GridGeom &G,
                                          double ax, double ay, double az, double r, double r2, int sub, int gbase, Hit &&hit)
{
    const double c3[3] = {ax, ay, az};
    // (the margins of the ball that is culled with: k_ball_count's)
    const double rr = r + (1e-9 * r + 1e-15 * (fabs(ax) + fabs(ay) + fabs(az) + r));
    const double rr2 = rr * rr, etol = 1e-6 * G.h;
    int lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double fl = floor((c3[a] - rr - G.mn[a]) * G.inv_h - 1e-6);
        const double fh = floor((c3[a] + rr - G.mn[a]) * G.inv_h + 1e-6);
        lo[a] = fl < 0.0 ? 0 : (fl > (double)(G.dim[a] - 1) ? G.dim[a] - 1 : (int)fl);
        hi[a] = fh < 0.0 ? 0 : (fh > (double)(G.dim[a] - 1) ? G.dim[a] - 1 : (int)fh);
    }
    const int ny = hi[1] - lo[1] + 1, nz = hi[2] - lo[2] + 1;
    const int nrows = ny * nz;                                 // (the host bounds the box: SICP_OUTLIER_MAX_BOX_CELLS)
    for (int rb = 0; rb < nrows; rb += CL_GS) {
        uint32_t b = 0, len = 0;
        const int rw = rb + sub;
        if (rw < nrows) {
            const int oz = rw / ny, oy = rw - oz * ny;
            const int cy = lo[1] + oy, cz = lo[2] + oz;
            const long row = ((long)cz * G.dim[1] + cy) * G.dim[0];
            const double rem = rr2 - row_lb2(G, cy, cz, ay, az, etol);
            if (rem >= 0.0) {
                int xl = lo[0], xh = hi[0];
                row_x_clip(G, ax, rem, etol, xl, xh);
                row_records(cell_start, row, xl, xh, b, len);
            }
        }
        unsigned todo = (unsigned)(__ballot(len > 0) >> gbase) & ((1u << CL_GS) - 1u);
        while (todo) {
            const int j = __ffs((int)todo) - 1;
            todo &= todo - 1u;
            const uint32_t bj = (uint32_t)__shfl((int)b, gbase + j), lj = (uint32_t)__shfl((int)len, gbase + j);
            for (uint32_t o = 0; o < lj; o += 2 * CL_GS) {
                const uint32_t i0 = o + (uint32_t)sub, i1 = i0 + CL_GS;
                const bool ok0 = i0 < lj, ok1 = i1 < lj;
                const double4 P0 = rec[ok0 ? bj + i0 : bj], P1 = rec[ok1 ? bj + i1 : bj];
                const double dx0 = P0.x - ax, dy0 = P0.y - ay, dz0 = P0.z - az;
                const double dx1 = P1.x - ax, dy1 = P1.y - ay, dz1 = P1.z - az;
                const bool h0 = ok0 && fma(dz0, dz0, fma(dy0, dy0, dx0 * dx0)) < r2;
                const bool h1 = ok1 && fma(dz1, dz1, fma(dy1, dy1, dx1 * dx1)) < r2;
                hit(h0, (uint32_t)__double_as_longlong(P0.w), h1, (uint32_t)__double_as_longlong(P1.w));
            }
        }
    }
}

// which point a group of CL_GS lanes takes: slot s of the launch (order: the chunk's points in cell order, one contiguous eighth of
// them per XCD -- the grid is a multiple of 8 blocks then; k_ball_count's rule); -1: none
__device__ __forceinline__ long group_point(const uint32_t *__restrict__ order, long Q)
{
    long blk = blockIdx.x;
    if (order) {
        const long per_xcd = gridDim.x >> 3;
        blk = (long)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    }
    const long slot = blk * (CL_BLOCK / CL_GS) + (threadIdx.x / CL_GS);
    if (slot >= Q) return -1;
    return order ? (long)order[slot] : slot;
}

// Every core point i of the chunk [lo, lo + Q) is united with its core neighbours j < i (each edge is seen once, from its higher
// end).  ri: the root of i as far as the group knows; a hit that is that root, or whose root is, costs no write.
__global__ __launch_bounds__(CL_BLOCK) void k_ball_union(const double *__restrict__ qx, const double *__restrict__ qy,
                                                         const double *__restrict__ qz, const uint32_t *__restrict__ order,
                                                         const uint32_t *__restrict__ cell_start, const double4 *__restrict__ rec,
                                                         const uint8_t *__restrict__ core, uint32_t *parent, long Q, long lo, GridGeom G,
                                                         double r, double r2)
{
    const int lane = threadIdx.x & 63, sub = lane & (CL_GS - 1), gbase = lane & ~(CL_GS - 1);
    const long q = group_point(order, Q);
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
        ri = gmin<CL_GS>(mine);                                    // (every lane's root is one of i's set: the smallest is the newest)
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
__global__ __launch_bounds__(CL_BLOCK) void k_ball_border(const double *__restrict__ qx, const double *__restrict__ qy,
                                                          const double *__restrict__ qz, const uint32_t *__restrict__ order,
                                                          const uint32_t *__restrict__ cell_start, const double4 *__restrict__ rec,
                                                          const uint8_t *__restrict__ core, uint32_t *root, long Q, long lo, GridGeom G,
                                                          double r, double r2)
{
    const int lane = threadIdx.x & 63, sub = lane & (CL_GS - 1), gbase = lane & ~(CL_GS - 1);
    const long q = group_point(order, Q);
    if (q < 0) return;
    const long i = lo + q;
    if (core[i]) return;
    uint32_t best = CL_NONE;
    ball_walk(cell_start, rec, G, qx[q], qy[q], qz[q], r, r2, sub, gbase, [&](bool h0, uint32_t j0, bool h1, uint32_t j1) {
        // (root[j] of a core point was written by k_cl_flatten; this kernel writes the others' words only)
        if (h0 && core[j0]) { const uint32_t rj = root[j0]; best = rj < best ? rj : best; }
        if (h1 && core[j1]) { const uint32_t rj = root[j1]; best = rj < best ? rj : best; }
    });
    best = gmin<CL_GS>(best);
    if (sub == 0) root[i] = best;
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

// one of the three walks over the cloud, a chunk at a time: the chunk's columns gathered, its cell order built from SICP_ORDER_MIN_Q
// points on; a cloud that fits one chunk keeps both for the walks that follow
struct ChunkWalk {
    sicp_ctx *c; int slot; long n, chunk; double order_h;
    bool kept = false;
    const uint32_t *order = nullptr;
    int enter(long lo, long cnt)
    {
        if (kept) return SICP_OK;
        rows_gather(c, slot, nullptr, lo, cnt);
        order = nullptr;
        if (c->order_min_q > 0 && cnt >= c->order_min_q) {
            const long qpad = round_up(cnt, QPAD);
            CHK(points_order_build(c, c->kq.p, c->kq.p + qpad, c->kq.p + 2 * qpad, cnt, order_h, 1L << 22, c->k_order));
            order = c->k_order.p;
        }
        kept = n <= chunk;
        return SICP_OK;
    }
    unsigned grid(long cnt) const
    {
        const unsigned g = cdiv(cnt, CL_BLOCK / CL_GS);
        return order ? (g + 7u) & ~7u : g;
    }
};

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
        const long chunk = c->cluster_chunk;
        CHK(c->kq.reserve((size_t)3 * round_up(std::min(chunk, n), QPAD)));
        ChunkWalk W{c, slot, n, chunk, 2.0 * lv.g.h};
        const dim3 flat(std::min(cdiv(n, CL_BLOCK), (unsigned)CL_MAX_BLOCKS));
        // core flags
        for (long lo = 0; lo < n; lo += chunk) {
            const long cnt = std::min(chunk, n - lo);
            CHK(W.enter(lo, cnt));
            // (no count from the kernel: its one atomic per wave on one word costs more than the walk where most points are core)
            CHK(ball_count_enqueue(c, c->kq.p, round_up(cnt, QPAD), W.order, nullptr, lv, cnt, radius, cap, core + lo, c->ol_cnt.p + lo,
                                   nullptr));
        }
        // unions
        hipLaunchKernelGGL(k_cl_fill, flat, dim3(CL_BLOCK), 0, c->stream, parent, n);
        for (long lo = 0; lo < n; lo += chunk) {
            const long cnt = std::min(chunk, n - lo), qpad = round_up(cnt, QPAD);
            CHK(W.enter(lo, cnt));
            hipLaunchKernelGGL(k_ball_union, dim3(W.grid(cnt)), dim3(CL_BLOCK), 0, c->stream, c->kq.p, c->kq.p + qpad, c->kq.p + 2 * qpad,
                               W.order, lv.cell_start, (const double4 *)lv.rec, core, parent, cnt, lo, lv.g, radius, r2);
            HIPCHK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_cl_flatten, dim3((unsigned)nb), dim3(CL_BLOCK), 0, c->stream, core, parent, root, n, sums);
        // borders
        for (long lo = 0; lo < n; lo += chunk) {
            const long cnt = std::min(chunk, n - lo), qpad = round_up(cnt, QPAD);
            CHK(W.enter(lo, cnt));
            hipLaunchKernelGGL(k_ball_border, dim3(W.grid(cnt)), dim3(CL_BLOCK), 0, c->stream, c->kq.p, c->kq.p + qpad, c->kq.p + 2 * qpad,
                               W.order, lv.cell_start, (const double4 *)lv.rec, core, root, cnt, lo, lv.g, radius, r2);
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
