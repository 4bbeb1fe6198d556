// sicp_regions.hip -- smooth regions of a cloud (include/simpleicp_hip_regions.h; contract (J)).
//
// Lists: every chunk of points goes through the slot's k-NN search (rows_knn, as sicp_orient's chunks do) and k_rg_lists keeps its
// indices as one (k, n) int32 table for the call, -1 where the rank lies outside the radius or names the point itself.  Union:
// k_rg_union walks every smooth point's list and unites it with the smooth entries it links with, in sicp_cluster's lock-free
// union-find (uf_find / uf_union, sicp_union_dev.h: a root is only ever hooked under a smaller root, so a region's root ends up
// its lowest index whatever the order of arrival); either end's list unites, so the symmetric closure costs nothing.  k_rg_flatten
// leaves every smooth point's root and counts the roots.  Border: k_rg_border lets every smooth point offer its root to the plain
// (neither smooth nor void) entries of its list it links with, and every plain point take the smallest root among the smooth
// entries of its own list -- both by an integer minimum on the same word, so an edge counts from whichever end lists it.  Sizes,
// survival, ranks: k_rg_sizes adds up the regions' members, k_rg_alive counts the surviving roots per workgroup, k_cl_scan_sums
// (the cluster unit's) scans those counts, k_rg_rank numbers the survivors in index order and finds the largest, k_rg_labels
// writes the labels.
// No kernel waits for another wave or workgroup: the only loops over memory another wave writes are uf_find's walk towards a root
// (parents only ever decrease) and uf_union's retry after a failed compare-and-swap (another lane's succeeded).  Every other word
// a kernel reads plainly was written before its launch.  Integer atomics only.
#include "sicp_host.h"
#include "sicp_union_dev.h"
#include "../../include/simpleicp_hip_regions.h"

namespace sicp {
namespace {

constexpr int RG_PER = 4;                          // consecutive points per thread of k_rg_alive / k_rg_rank
constexpr int RG_SPAN = CL_BLOCK * RG_PER;         // points per workgroup of the rank scan
constexpr int RG_RUN = 16;                         // consecutive rows of 64 points per wave of k_rg_sizes
constexpr uint32_t RG_NONE = 0xffffffffu;          // root of a point without a region, rank of a root that does not survive
enum : uint8_t { RG_VOID = 0, RG_PLAIN = 1, RG_SMOOTH = 2 };   // a point's kind byte

// counter words of the call (c->cand_small)
enum { RG_N_VOID = 0, RG_N_SMOOTH = 1, RG_N_BORDER = 2, RG_N_ALL = 3, RG_N_REGIONS = 4, RG_N_LABELLED = 6, RG_BEST = 7 };

__device__ __forceinline__ bool rg_void(float x, float y, float z)
{
    const bool fin = fabsf(x) <= 3.4028234663852886e38f && fabsf(y) <= 3.4028234663852886e38f && fabsf(z) <= 3.4028234663852886e38f;
    return !fin || (x == 0.0f && y == 0.0f && z == 0.0f);
}
// does the edge between two normals link?  s_ij and t_ij of the contract
__device__ __forceinline__ bool rg_links(float ax, float ay, float az, float bx, float by, float bz, double cos_min, int oriented)
{
    const double s = ((double)ax * (double)bx + (double)ay * (double)by) + (double)az * (double)bz;
    return (oriented ? s : fabs(s)) >= cos_min;
}
__device__ __forceinline__ void rg_count(unsigned long long *counter, bool set)
{
    const unsigned m = (unsigned)__popcll((long long)__ballot(set));
    if (m && (threadIdx.x & 63) == 0) atomicAdd(counter, (unsigned long long)m);
}

// a chunk's ranked lists idx / d2 (Q, k) as columns lo .. lo + Q of the (k, n) table; a rank that holds no point, the point itself
// or a point that is not strictly inside the radius: -1
__global__ __launch_bounds__(CL_BLOCK) void k_rg_lists(const int64_t *__restrict__ idx, const double *__restrict__ d2, long n, long lo, long Q,
                                                       int k, double r2, int no_radius, int32_t *__restrict__ nbr)
{
    const long e = (long)blockIdx.x * CL_BLOCK + threadIdx.x;
    if (e >= Q * k) return;
    const long q = e / k, r = e - q * k, j = idx[e];
    const bool edge = j >= 0 && j < n && j != lo + q && (no_radius || d2[e] < r2);
    nbr[r * n + lo + q] = edge ? (int32_t)j : -1;
}

// every point's kind, a set of its own, an empty region; the void and the smooth points counted
__global__ __launch_bounds__(CL_BLOCK) void k_rg_init(const float *__restrict__ nrm, const uint8_t *__restrict__ seeds, long n,
                                                      uint8_t *__restrict__ kind, uint32_t *__restrict__ parent, uint32_t *__restrict__ size,
                                                      unsigned long long *__restrict__ counters)
{
    const long i = (long)blockIdx.x * CL_BLOCK + threadIdx.x;
    uint8_t mine = RG_PLAIN;
    if (i < n) {
        if (rg_void(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2])) mine = RG_VOID;
        else if (!seeds || seeds[i] != 0) mine = RG_SMOOTH;
        kind[i] = mine; parent[i] = (uint32_t)i; size[i] = 0u;
    }
    rg_count(counters + RG_N_VOID, i < n && mine == RG_VOID);
    rg_count(counters + RG_N_SMOOTH, i < n && mine == RG_SMOOTH);
}

// Every smooth point i is united with the smooth entries of its list it links with.  mine: the root of i as far as the lane knows;
// an entry that is that root, or whose root is, costs no write.
__global__ __launch_bounds__(CL_BLOCK) void k_rg_union(const int32_t *__restrict__ nbr, const float *__restrict__ nrm,
                                                       const uint8_t *__restrict__ kind, uint32_t *parent, long n, int k, double cos_min,
                                                       int oriented)
{
    const long i = (long)blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= n || kind[i] != RG_SMOOTH) return;
    const float ax = nrm[3 * i], ay = nrm[3 * i + 1], az = nrm[3 * i + 2];
    uint32_t mine = (uint32_t)i;
    for (int r = 0; r < k; ++r) {
        const long j = nbr[(long)r * n + i];
        if (j < 0 || (uint32_t)j == mine || kind[j] != RG_SMOOTH) continue;
        if (!rg_links(ax, ay, az, nrm[3 * j], nrm[3 * j + 1], nrm[3 * j + 2], cos_min, oriented)) continue;
        const uint32_t rj = uf_find(parent, (uint32_t)j);
        if (rj != mine) mine = uf_union(parent, mine, rj);
    }
}

// root[i] of the smooth points (the others': RG_NONE until k_rg_border), the roots counted.  The kernel boundary is behind the
// unions; the finds still halve paths (a chain hooked in one volley is as long as the volley), so they keep the atomic accesses.
__global__ __launch_bounds__(CL_BLOCK) void k_rg_flatten(const uint8_t *__restrict__ kind, uint32_t *parent, uint32_t *__restrict__ root, long n,
                                                         unsigned long long *__restrict__ counters)
{
    const long i = (long)blockIdx.x * CL_BLOCK + threadIdx.x;
    uint32_t rt = RG_NONE;
    if (i < n) {
        if (kind[i] == RG_SMOOTH) rt = uf_find(parent, (uint32_t)i);
        root[i] = rt;
    }
    rg_count(counters + RG_N_ALL, i < n && rt == (uint32_t)i);
}

// root[j] of a plain point j = the smallest root among the smooth points it has a linking edge with.  A smooth point offers its
// root to the plain entries of its list; a plain point takes the minimum over the smooth entries of its own.  The roots of the
// smooth points were written by k_rg_flatten and are only read here; the plain points' words only ever shrink, by atomics.
__global__ __launch_bounds__(CL_BLOCK) void k_rg_border(const int32_t *__restrict__ nbr, const float *__restrict__ nrm,
                                                        const uint8_t *__restrict__ kind, uint32_t *root, long n, int k, double cos_min,
                                                        int oriented)
{
    const long i = (long)blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint8_t ki = kind[i];
    if (ki == RG_VOID) return;
    const float ax = nrm[3 * i], ay = nrm[3 * i + 1], az = nrm[3 * i + 2];
    const uint32_t ri = ki == RG_SMOOTH ? root[i] : RG_NONE;
    uint32_t best = RG_NONE;
    for (int r = 0; r < k; ++r) {
        const long j = nbr[(long)r * n + i];
        if (j < 0) continue;
        const uint8_t kj = kind[j];
        if (kj == RG_VOID || kj == ki) continue;
        if (!rg_links(ax, ay, az, nrm[3 * j], nrm[3 * j + 1], nrm[3 * j + 2], cos_min, oriented)) continue;
        if (ki == RG_SMOOTH) {
            // (the word only shrinks: one that is not above the root already needs no atomic)
            if (__hip_atomic_load(root + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > ri)
                (void)__hip_atomic_fetch_min(root + j, ri, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            const uint32_t rj = root[j];
            best = rj < best ? rj : best;
        }
    }
    if (best != RG_NONE) (void)__hip_atomic_fetch_min(root + i, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// size[root] += the region's members, smooth and border, by integer atomics: one per run of equal roots a wave meets in its RG_RUN
// rows of 64 consecutive points; the border points counted by ballots
__global__ __launch_bounds__(CL_BLOCK) void k_rg_sizes(const uint8_t *__restrict__ kind, const uint32_t *__restrict__ root, long n,
                                                       uint32_t *__restrict__ size, unsigned long long *__restrict__ counters)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long wbase = ((long)blockIdx.x * (CL_BLOCK / 64) + wave) * (RG_RUN * 64);
    unsigned n_border = 0;
    uint32_t run_root = RG_NONE, run = 0;                          // (wave-uniform)
    for (int it = 0; it < RG_RUN && wbase + it * 64 < n; ++it) {
        const long e = wbase + it * 64 + lane;
        const bool in = e < n;
        const uint32_t rt = in ? root[e] : RG_NONE;
        const bool has = rt != RG_NONE;
        n_border += (unsigned)__popcll((long long)__ballot(has && kind[e] == RG_PLAIN));
        unsigned long long todo = __ballot(has);
        while (todo) {
            const int first = __ffsll((long long)todo) - 1;
            const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)rt, first);
            const unsigned long long same = __ballot(has && rt == r);
            const uint32_t m = (uint32_t)__popcll((long long)same);
            if (r == run_root) {
                run += m;
            } else {
                if (run && lane == 0) atomicAdd(size + run_root, run);
                run_root = r; run = m;
            }
            todo &= ~same;
        }
    }
    if (lane == 0) {
        if (run) atomicAdd(size + run_root, run);
        if (n_border) atomicAdd(counters + RG_N_BORDER, (unsigned long long)n_border);
    }
}

__device__ __forceinline__ bool rg_survivor(const uint32_t *__restrict__ root, const uint32_t *__restrict__ size, long e, long n,
                                            unsigned long long min_size)
{
    return e < n && root[e] == (uint32_t)e && (unsigned long long)size[e] >= min_size;
}

// per workgroup of RG_SPAN points the number of roots whose region survives
__global__ __launch_bounds__(CL_BLOCK) void k_rg_alive(const uint32_t *__restrict__ root, const uint32_t *__restrict__ size, long n,
                                                       unsigned long long min_size, uint32_t *__restrict__ sums)
{
    const long base = (long)blockIdx.x * RG_SPAN + (long)threadIdx.x * RG_PER;
    unsigned alive = 0;
#pragma unroll
    for (int u = 0; u < RG_PER; ++u) alive += rg_survivor(root, size, base + u, n, min_size) ? 1u : 0u;
    alive = block_sum_u32<CL_BLOCK / 64>(alive);
    if (threadIdx.x == 0) sums[blockIdx.x] = alive;
}

// rank[i] of every root i: the number of surviving roots below it -- its region's label -- or RG_NONE where the region does not
// survive; the largest region: max over the labels of (size << 32 | ~label) -- of equal sizes the lowest label wins
__global__ __launch_bounds__(CL_BLOCK) void k_rg_rank(const uint32_t *__restrict__ root, const uint32_t *__restrict__ size, long n,
                                                      unsigned long long min_size, const uint32_t *__restrict__ sums, uint32_t *__restrict__ rank,
                                                      unsigned long long *__restrict__ counters)
{
    __shared__ uint32_t wtot[CL_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long base = (long)blockIdx.x * RG_SPAN + (long)threadIdx.x * RG_PER;
    bool f[RG_PER];
    uint32_t cnt = 0;
#pragma unroll
    for (int u = 0; u < RG_PER; ++u) {
        f[u] = rg_survivor(root, size, base + u, n, min_size);
        cnt += f[u] ? 1u : 0u;
    }
    const uint32_t inc = wscan_u32(cnt);
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    uint32_t at = sums[blockIdx.x] + inc - cnt;
#pragma unroll
    for (int w = 0; w < CL_BLOCK / 64; ++w) at += w < wave ? wtot[w] : 0u;
    unsigned long long best = 0;
#pragma unroll
    for (int u = 0; u < RG_PER; ++u) {
        const long e = base + u;
        if (f[u]) {
            const unsigned long long key = ((unsigned long long)size[e] << 32) | (unsigned long long)(RG_NONE - at);
            best = key > best ? key : best;
            rank[e] = at; ++at;
        } else if (e < n) {
            rank[e] = RG_NONE;
        }
    }
    unsigned long long o;
    o = lane_xor64<32>(best); best = o > best ? o : best;
    o = lane_xor64<16>(best); best = o > best ? o : best;
    o = lane_xor64<8>(best);  best = o > best ? o : best;
    o = lane_xor64<4>(best);  best = o > best ? o : best;
    o = lane_xor64<2>(best);  best = o > best ? o : best;
    o = lane_xor64<1>(best);  best = o > best ? o : best;
    if (lane == 0 && best) atomicMax(counters + RG_BEST, best);
}

// labels[i] = rank[root[i]], -1 where there is no root or its region does not survive; the labelled points counted
__global__ __launch_bounds__(CL_BLOCK) void k_rg_labels(const uint32_t *__restrict__ root, const uint32_t *__restrict__ rank, long n,
                                                        int32_t *__restrict__ labels, unsigned long long *__restrict__ counters)
{
    const long i = (long)blockIdx.x * CL_BLOCK + threadIdx.x;
    uint32_t lab = RG_NONE;
    if (i < n) {
        const uint32_t rt = root[i];
        if (rt != RG_NONE) lab = rank[rt];
        labels[i] = lab != RG_NONE ? (int32_t)lab : -1;
    }
    rg_count(counters + RG_N_LABELLED, lab != RG_NONE);
}

}  // namespace
}  // namespace sicp

namespace {

static_assert(RG_BEST < CAND_WORDS, "the record's counters fit the ctx's counter words");

}  // namespace

SICP_EXPORT int sicp_regions_version(void) { return SICP_REGIONS_VERSION; }

SICP_EXPORT int sicp_regions(sicp_ctx *c, int slot, const float *normals, int k, double radius, double cos_min, int oriented,
                             const uint8_t *seeds, int64_t min_size, int32_t *labels_out, sicp_regions_stats *out)
{
    CHK(check_slot(c, slot, true));
    if (!normals) return fail(SICP_ERR_INVALID, "normals is null");
    if (!labels_out) return fail(SICP_ERR_INVALID, "labels_out is null");
    if (!out) return fail(SICP_ERR_INVALID, "out is null");
    Cloud &cl = c->cloud[slot];
    if (k < 2) return fail(SICP_ERR_INVALID, "k must be >= 2 (%d given)", k);
    if (k > SICP_FPFH_MAX_K) return fail(SICP_ERR_INVALID, "k must be <= %d (%d given)", SICP_FPFH_MAX_K, k);
    if (k > cl.n) return fail(SICP_ERR_INVALID, "k (%d) exceeds the number of points (%lld)", k, (long long)cl.n);
    if (std::isnan(radius) || !(radius > 0.0)) return fail(SICP_ERR_INVALID, "radius must be > 0 (+inf: none)");
    if (!(cos_min <= 1.0) || !(cos_min >= (oriented ? -1.0 : 0.0)))
        return fail(SICP_ERR_INVALID, "cos_min must be >= %d and <= 1", oriented ? -1 : 0);
    if (min_size < 1) return fail(SICP_ERR_INVALID, "min_size must be >= 1");
    CHK(check_whole_cloud(c, slot, "sicp_regions", "a point's neighbours may live on another rank"));
    HIPCHK(hipSetDevice(c->device));
    return op_run(c, [&]() -> int {
        const long n = (long)cl.n, nb = cdiv(n, RG_SPAN);
        const float *nrm;
        const uint8_t *sd = nullptr;
        int32_t *labels;
        CHK(c->or_nbr.reserve((size_t)k * n));
        CHK(c->cand_keep.reserve((size_t)n));
        CHK(c->cl_parent.reserve((size_t)n));
        CHK(c->cl_root.reserve((size_t)n));
        CHK(c->cl_rank.reserve((size_t)(n + nb)));
        CHK(c->cl_size.reserve((size_t)n));
        CHK(stage_in(c, normals, (size_t)3 * n, c->or_nrm, &nrm));
        if (seeds) CHK(stage_in(c, seeds, (size_t)n, c->or_flip, &sd));
        CHK(stage_out(c, labels_out, (size_t)n, c->cl_labels, &labels));
        CHK(counters_clear(c));
        const int32_t *nbr = c->or_nbr.p;
        uint8_t *kind = c->cand_keep.p;
        uint32_t *parent = c->cl_parent.p, *root = c->cl_root.p, *rank = c->cl_rank.p, *sums = c->cl_rank.p + n, *size = c->cl_size.p;
        unsigned long long *counters = c->cand_small.p;
        const unsigned long long alive_from = (unsigned long long)min_size;
        const int dir = oriented ? 1 : 0;
        const dim3 pts(cdiv(n, CL_BLOCK)), spans((unsigned)nb), block(CL_BLOCK);
        // lists
        const double r2 = radius * radius;
        const long chunk = knn_chunk(c->regions_chunk, k);
        CHK(knn_chunk_reserve(c, std::min(chunk, n), k));
        for (long lo = 0; lo < n; lo += chunk) {
            const long cnt = std::min(chunk, n - lo);
            CHK(rows_knn(c, slot, nullptr, lo, cnt, k));
            hipLaunchKernelGGL(k_rg_lists, dim3(cdiv(cnt * k, CL_BLOCK)), block, 0, c->stream, c->k_idx.p, c->k_d2.p, n, lo, cnt, k, r2,
                               std::isinf(radius) ? 1 : 0, c->or_nbr.p);
            HIPCHK(hipGetLastError());
        }
        // regions, borders
        hipLaunchKernelGGL(k_rg_init, pts, block, 0, c->stream, nrm, sd, n, kind, parent, size, counters);
        hipLaunchKernelGGL(k_rg_union, pts, block, 0, c->stream, nbr, nrm, kind, parent, n, k, cos_min, dir);
        hipLaunchKernelGGL(k_rg_flatten, pts, block, 0, c->stream, kind, parent, root, n, counters);
        hipLaunchKernelGGL(k_rg_border, pts, block, 0, c->stream, nbr, nrm, kind, root, n, k, cos_min, dir);
        // sizes, survival, ranks, labels, record
        hipLaunchKernelGGL(k_rg_sizes, dim3(cdiv(n, RG_RUN * CL_BLOCK)), block, 0, c->stream, kind, root, n, size, counters);
        hipLaunchKernelGGL(k_rg_alive, spans, block, 0, c->stream, root, size, n, alive_from, sums);
        hipLaunchKernelGGL(k_cl_scan_sums, dim3(1), block, 0, c->stream, sums, nb, counters + RG_N_REGIONS);
        hipLaunchKernelGGL(k_rg_rank, spans, block, 0, c->stream, root, size, n, alive_from, sums, rank, counters);
        hipLaunchKernelGGL(k_rg_labels, pts, block, 0, c->stream, root, rank, n, labels, counters);
        HIPCHK(hipGetLastError());
        CHK(counters_fetch(c));
        CHK(stage_leave(c, labels_out, (size_t)n, labels));
        CHK(sync(c));
        const unsigned long long *h = counters_host(c);
        out->n_points = (int64_t)n;
        out->n_void = (int64_t)h[RG_N_VOID];
        out->n_smooth = (int64_t)h[RG_N_SMOOTH];
        out->n_border = (int64_t)h[RG_N_BORDER];
        out->n_regions_all = (int64_t)h[RG_N_ALL];
        out->n_regions = (int64_t)h[RG_N_REGIONS];
        out->n_labelled = (int64_t)h[RG_N_LABELLED];
        out->largest_label = h[RG_N_REGIONS] ? (int64_t)(0xffffffffu - (uint32_t)h[RG_BEST]) : -1;
        out->largest_size = h[RG_N_REGIONS] ? (int64_t)(h[RG_BEST] >> 32) : 0;
        return SICP_OK;
    });
}
