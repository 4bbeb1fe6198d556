// sicp_orient.hip -- normals oriented consistently (include/simpleicp_hip_orient.h; contract (H)).
//
// Lists: every chunk of points goes through the slot's k-NN search (rows_knn, as sicp_fpfh's chunks do) and k_or_lists keeps its
// indices as one (k, n) int32 table for the call.  Forest: Boruvka rounds of four launches.  k_or_offer<1> walks every point's list
// and offers each edge that leaves the point's component to BOTH components' maxima of c (an integer atomicMax on the bits of a
// non-negative double, plus one: 0 is "no offer"); k_or_offer<2>, a kernel boundary later, walks again and takes the minimum of
// lo << 31 | hi among the offers whose c is the winner's; k_or_hook lets every root with a winner hang itself under the root at the
// other end, with the parity of the two signs and the edge's disagreement (of a mutual pair the lower root stays: the order is
// total, so there is no other cycle); k_or_flatten gives every point its new root and sign.  The host reads one word per round and
// stops behind the round that hooked nothing.  Then k_or_vote finds every component's lowest index and counts its votes, and
// k_or_apply writes the normals, the flipped bytes and the record.
// No kernel waits for another wave or workgroup.  The only loop over memory another wave writes is or_find's walk towards a root in
// k_or_flatten: the words it reads are agent-scope atomics, the hooks of the round are a kernel boundary behind it and form a forest,
// and a compare-and-swap only ever replaces an ancestor by a farther ancestor, so the walk ends whatever the scheduling.  Every
// other word a kernel reads plainly was written before its launch.  Integer atomics only.
#include "sicp_host.h"
#include "sicp_lanes.h"
#include "../../include/simpleicp_hip_orient.h"

namespace sicp {
namespace {

constexpr int OR_BLOCK = 256;
constexpr uint32_t OR_ROOT = 0x7fffffffu;          // a union word: the parent (comp: the root) in the low 31 bits ...
constexpr uint32_t OR_SIGN = 0x80000000u;          // ... and the parity of disagreements on the way there
constexpr unsigned long long OR_NO_EDGE = ~0ull;

// counter words of the call (c->cand_small)
enum { OR_HOOKED = 0, OR_VOID = 1, OR_COMPONENTS = 2, OR_FLIPPED = 3, OR_VOTED = 4 };

__device__ __forceinline__ bool or_void(float x, float y, float z)
{
    const bool fin = fabsf(x) <= 3.4028234663852886e38f && fabsf(y) <= 3.4028234663852886e38f && fabsf(z) <= 3.4028234663852886e38f;
    return !fin || (x == 0.0f && y == 0.0f && z == 0.0f);
}
// s_ij of the contract
__device__ __forceinline__ double or_dot(float ax, float ay, float az, float bx, float by, float bz)
{
    return ((double)ax * (double)bx + (double)ay * (double)by) + (double)az * (double)bz;
}
__device__ __forceinline__ unsigned long long or_edge(uint32_t i, uint32_t j)
{
    return i < j ? ((unsigned long long)i << 31) | j : ((unsigned long long)j << 31) | i;
}
__device__ __forceinline__ void or_count(unsigned long long *counter, bool set)
{
    const unsigned m = (unsigned)__popcll((long long)__ballot(set));
    if (m && (threadIdx.x & 63) == 0) atomicAdd(counter, (unsigned long long)m);
}

// a chunk's ranked lists idx (Q, k) as columns lo .. lo + Q of the (k, n) table; a rank that holds no point: -1
__global__ __launch_bounds__(OR_BLOCK) void k_or_lists(const int64_t *__restrict__ idx, long n, long lo, long Q, int k, int32_t *__restrict__ nbr)
{
    const long e = (long)blockIdx.x * OR_BLOCK + threadIdx.x;
    if (e >= Q * k) return;
    const long q = e / k, r = e - q * k, j = idx[e];
    nbr[r * n + lo + q] = j >= 0 && j < n ? (int32_t)j : -1;
}

// every point a component of its own; the void points counted
__global__ __launch_bounds__(OR_BLOCK) void k_or_init(const float *__restrict__ nrm, long n, uint32_t *__restrict__ comp, uint32_t *__restrict__ par,
                                                      unsigned long long *__restrict__ bestc, unsigned long long *__restrict__ beste,
                                                      unsigned long long *__restrict__ counters)
{
    const long i = (long)blockIdx.x * OR_BLOCK + threadIdx.x;
    const bool in = i < n;
    if (in) { comp[i] = (uint32_t)i; par[i] = (uint32_t)i; bestc[i] = 0ull; beste[i] = OR_NO_EDGE; }
    or_count(counters + OR_VOID, in && or_void(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]));
}

// PASS 1: bestc[root] = max over the edges that leave the component of bits(c) + 1.  PASS 2: beste[root] = min of lo << 31 | hi
// over those of them whose c is that maximum (bestc is a kernel boundary old then).  An edge is offered to both ends' components:
// j's own list need not hold i.  What goes to the point's own component is folded in the lane first: one atomic per point.
template <int PASS>
__global__ __launch_bounds__(OR_BLOCK) void k_or_offer(const int32_t *__restrict__ nbr, const float *__restrict__ nrm,
                                                       const uint32_t *__restrict__ comp, unsigned long long *bestc, unsigned long long *beste,
                                                       long n, int k)
{
    const long i = (long)blockIdx.x * OR_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float ax = nrm[3 * i], ay = nrm[3 * i + 1], az = nrm[3 * i + 2];
    if (or_void(ax, ay, az)) return;
    const uint32_t ci = comp[i] & OR_ROOT;
    const unsigned long long win_i = PASS == 2 ? bestc[ci] : 0ull;
    unsigned long long mine = PASS == 1 ? 0ull : OR_NO_EDGE;
    for (int r = 0; r < k; ++r) {
        const long j = nbr[(long)r * n + i];
        if (j < 0 || j == i) continue;
        const uint32_t cj = comp[j] & OR_ROOT;
        if (cj == ci) continue;
        const float bx = nrm[3 * j], by = nrm[3 * j + 1], bz = nrm[3 * j + 2];
        if (or_void(bx, by, bz)) continue;
        const unsigned long long key = (unsigned long long)__double_as_longlong(fabs(or_dot(ax, ay, az, bx, by, bz))) + 1ull;
        if (PASS == 1) {
            mine = key > mine ? key : mine;
            // (the word only grows: one that is not below the key already needs no atomic)
            if (__hip_atomic_load(bestc + cj, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < key)
                (void)__hip_atomic_fetch_max(bestc + cj, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            const unsigned long long e = or_edge((uint32_t)i, (uint32_t)j);
            if (key == win_i) mine = e < mine ? e : mine;
            if (key == bestc[cj] && __hip_atomic_load(beste + cj, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > e)
                (void)__hip_atomic_fetch_min(beste + cj, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (PASS == 1) {
        if (mine && __hip_atomic_load(bestc + ci, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < mine)
            (void)__hip_atomic_fetch_max(bestc + ci, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (mine != OR_NO_EDGE && __hip_atomic_load(beste + ci, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > mine) {
        (void)__hip_atomic_fetch_min(beste + ci, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Every root with a winning edge (lo, hi) hangs itself under the root at the other end: par[root] = other | parity, the parity of
// root against other being sign(lo) ^ sign(hi) ^ disagree(lo, hi).  Where the other root chose the same edge the lower root stays.
// comp, bestc and beste are read only; par[i] is written by the lane of root i alone.
__global__ __launch_bounds__(OR_BLOCK) void k_or_hook(const float *__restrict__ nrm, const uint32_t *__restrict__ comp,
                                                      const unsigned long long *__restrict__ bestc, const unsigned long long *__restrict__ beste,
                                                      long n, uint32_t *__restrict__ par, unsigned long long *__restrict__ counters)
{
    const long i = (long)blockIdx.x * OR_BLOCK + threadIdx.x;
    bool hooked = false;
    if (i < n && (comp[i] & OR_ROOT) == (uint32_t)i && bestc[i] != 0ull && beste[i] != OR_NO_EDGE) {
        const unsigned long long e = beste[i];                     // (pass 2 met the winner again: there is an edge)
        const uint32_t lo = (uint32_t)(e >> 31), hi = (uint32_t)e & OR_ROOT;
        const uint32_t wl = comp[lo], wh = comp[hi];
        const uint32_t other = (wl & OR_ROOT) == (uint32_t)i ? (wh & OR_ROOT) : (wl & OR_ROOT);
        const bool mutual = bestc[other] != 0ull && beste[other] == e;
        if (!(mutual && (uint32_t)i < other)) {
            const bool dis = or_dot(nrm[3 * lo], nrm[3 * lo + 1], nrm[3 * lo + 2], nrm[3 * hi], nrm[3 * hi + 1], nrm[3 * hi + 2]) < 0.0;
            par[i] = other | (((wl ^ wh) & OR_SIGN) ^ (dis ? OR_SIGN : 0u));
            hooked = true;
        }
    }
    or_count(counters + OR_HOOKED, hooked);
}

// the root of x and, in the sign bit of `sgn`, the parity of x against it; path halving on the way: par[x] goes from x's parent to
// its grandparent with the two parities folded, by a compare-and-swap that is skipped where it loses its race
__device__ __forceinline__ uint32_t or_find(uint32_t *par, uint32_t x, uint32_t &sgn)
{
    uint32_t acc = 0u;
    uint32_t w = __hip_atomic_load(par + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (;;) {
        const uint32_t p = w & OR_ROOT;
        if (p == x) break;
        const uint32_t wp = __hip_atomic_load(par + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((wp & OR_ROOT) != p) {
            uint32_t expected = w;
            (void)__hip_atomic_compare_exchange_strong(par + x, &expected, (wp & OR_ROOT) | ((w ^ wp) & OR_SIGN), __ATOMIC_RELAXED,
                                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        acc ^= w & OR_SIGN;
        x = p; w = wp;
    }
    sgn = acc;
    return x;
}

// comp[i] = the root of i's old root, the signs folded; the offers of the next round (the votes and the anchor behind the last) reset
__global__ __launch_bounds__(OR_BLOCK) void k_or_flatten(uint32_t *__restrict__ comp, uint32_t *par, long n, unsigned long long *__restrict__ bestc,
                                                         unsigned long long *__restrict__ beste)
{
    const long i = (long)blockIdx.x * OR_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t w = comp[i];
    uint32_t sgn;
    const uint32_t root = or_find(par, w & OR_ROOT, sgn);
    comp[i] = root | ((w ^ sgn) & OR_SIGN);
    bestc[i] = 0ull; beste[i] = OR_NO_EDGE;
}

// beste[root] = the component's lowest index (its anchor); with a reference, bestc[root] += pos | neg << 32, the votes of the normals
// as they stand against the ROOT (k_or_apply swaps them where the anchor's sign differs).  One atomic per set of equal roots a wave
// meets in its 64 consecutive points: the lowest lane of the set holds its lowest index.
__global__ __launch_bounds__(OR_BLOCK) void k_or_vote(const double *__restrict__ X, const double *__restrict__ Y, const double *__restrict__ Z,
                                                      const float *__restrict__ nrm, const uint32_t *__restrict__ comp, long n, int have_ref,
                                                      double rx, double ry, double rz, unsigned long long *__restrict__ votes,
                                                      unsigned long long *__restrict__ anchor)
{
    const long i = (long)blockIdx.x * OR_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool live = false, pos = false, neg = false;
    uint32_t root = 0u;
    if (i < n) {
        float fx = nrm[3 * i], fy = nrm[3 * i + 1], fz = nrm[3 * i + 2];
        live = !or_void(fx, fy, fz);
        const uint32_t w = comp[i];
        root = w & OR_ROOT;
        if (live && have_ref) {
            if (w & OR_SIGN) { fx = -fx; fy = -fy; fz = -fz; }
            const double t = ((rx - X[i]) * (double)fx + (ry - Y[i]) * (double)fy) + (rz - Z[i]) * (double)fz;
            pos = t > 0.0; neg = t < 0.0;
        }
    }
    const unsigned long long bpos = __ballot(pos), bneg = __ballot(neg);
    unsigned long long todo = __ballot(live);
    while (todo) {
        const int first = __ffsll((long long)todo) - 1;
        const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)root, first);
        const unsigned long long same = __ballot(live && root == r);
        if (lane == first) {
            (void)__hip_atomic_fetch_min(anchor + r, (unsigned long long)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long v = (unsigned long long)__popcll((long long)(same & bpos)) |
                                         ((unsigned long long)__popcll((long long)(same & bneg)) << 32);
            if (v) (void)__hip_atomic_fetch_add(votes + r, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        todo &= ~same;
    }
}

// the verdicts: flipped = sign against the root ^ the anchor's ^ the component's vote bit; the normals, the bytes, the record
__global__ __launch_bounds__(OR_BLOCK) void k_or_apply(const float *__restrict__ nrm, const uint32_t *__restrict__ comp,
                                                       const unsigned long long *__restrict__ votes, const unsigned long long *__restrict__ anchor,
                                                       long n, int have_ref, int away, float *__restrict__ out, uint8_t *__restrict__ flipped,
                                                       unsigned long long *__restrict__ counters)
{
    const long i = (long)blockIdx.x * OR_BLOCK + threadIdx.x;
    bool is_root = false, flip = false, voted = false;
    if (i < n) {
        const float fx = nrm[3 * i], fy = nrm[3 * i + 1], fz = nrm[3 * i + 2];
        const uint32_t w = comp[i], root = w & OR_ROOT;
        is_root = root == (uint32_t)i;
        if (!or_void(fx, fy, fz)) {
            const uint32_t wa = comp[(uint32_t)anchor[root]];
            bool bit = false;
            if (have_ref) {
                const unsigned long long v = votes[root];
                uint32_t pos = (uint32_t)v, neg = (uint32_t)(v >> 32);
                if (wa & OR_SIGN) { const uint32_t t = pos; pos = neg; neg = t; }
                bit = away ? pos > neg : neg > pos;
            }
            flip = (((w ^ wa) & OR_SIGN) != 0u) != bit;
            voted = is_root && bit;
        }
        out[3 * i] = flip ? -fx : fx; out[3 * i + 1] = flip ? -fy : fy; out[3 * i + 2] = flip ? -fz : fz;
        if (flipped) flipped[i] = flip ? 1 : 0;
    }
    or_count(counters + OR_COMPONENTS, is_root);
    or_count(counters + OR_FLIPPED, flip);
    or_count(counters + OR_VOTED, voted);
}

}  // namespace
}  // namespace sicp

namespace {

static_assert(OR_VOTED < CAND_WORDS, "the record's counters fit the ctx's counter words");
constexpr int OR_MAX_ROUNDS = 32;                  // ceil(log2 n) <= 31 rounds join something, one more joins nothing

}  // namespace

SICP_EXPORT int sicp_orient_version(void) { return SICP_ORIENT_VERSION; }

SICP_EXPORT int sicp_orient(sicp_ctx *c, int slot, const float *normals, int k, const double *reference, int away, float *normals_out,
                            uint8_t *flipped_out, sicp_orient_stats *out)
{
    CHK(check_slot(c, slot, true));
    if (!normals) return fail(SICP_ERR_INVALID, "normals is null");
    if (!normals_out) return fail(SICP_ERR_INVALID, "normals_out is null");
    if (!out) return fail(SICP_ERR_INVALID, "out is null");
    Cloud &cl = c->cloud[slot];
    if (k < 2) return fail(SICP_ERR_INVALID, "k must be >= 2 (%d given)", k);
    if (k > SICP_FPFH_MAX_K) return fail(SICP_ERR_INVALID, "k must be <= %d (%d given)", SICP_FPFH_MAX_K, k);
    if (k > cl.n) return fail(SICP_ERR_INVALID, "k (%d) exceeds the number of points (%lld)", k, (long long)cl.n);
    if (reference && !(std::isfinite(reference[0]) && std::isfinite(reference[1]) && std::isfinite(reference[2])))
        return fail(SICP_ERR_INVALID, "reference must be finite");
    CHK(check_whole_cloud(c, slot, "sicp_orient", "a point's neighbours may live on another rank"));
    HIPCHK(hipSetDevice(c->device));
    return op_run(c, [&]() -> int {
        const long n = (long)cl.n;
        float *dst;
        uint8_t *flip;
        CHK(c->or_nbr.reserve((size_t)k * n));
        CHK(c->or_nrm.reserve((size_t)3 * n));
        CHK(c->or_comp.reserve((size_t)n));
        CHK(c->or_par.reserve((size_t)n));
        CHK(c->or_bestc.reserve((size_t)n));
        CHK(c->or_beste.reserve((size_t)n));
        CHK(stage_out(c, normals_out, (size_t)3 * n, c->or_out, &dst));
        CHK(stage_out(c, flipped_out, (size_t)n, c->or_flip, &flip));
        CHK(counters_clear(c));
        // the normals are always copied: normals_out may be the same array
        HIPCHK(hipMemcpyAsync(c->or_nrm.p, normals, (size_t)3 * n * sizeof(float), hipMemcpyDefault, c->stream));
        const float *nrm = c->or_nrm.p;
        const int32_t *nbr = c->or_nbr.p;
        uint32_t *comp = c->or_comp.p, *par = c->or_par.p;
        unsigned long long *bestc = c->or_bestc.p, *beste = c->or_beste.p, *counters = c->cand_small.p;
        const dim3 pts(cdiv(n, OR_BLOCK)), block(OR_BLOCK);
        // lists
        const long chunk = knn_chunk(c->orient_chunk, k);
        CHK(knn_chunk_reserve(c, std::min(chunk, n), k));
        for (long lo = 0; lo < n; lo += chunk) {
            const long cnt = std::min(chunk, n - lo);
            CHK(rows_knn(c, slot, nullptr, lo, cnt, k));
            hipLaunchKernelGGL(k_or_lists, dim3(cdiv(cnt * k, OR_BLOCK)), block, 0, c->stream, c->k_idx.p, n, lo, cnt, k, c->or_nbr.p);
            HIPCHK(hipGetLastError());
        }
        // forest: the host reads the hooked count of every round and stops behind the round that hooked nothing
        hipLaunchKernelGGL(k_or_init, pts, block, 0, c->stream, nrm, n, comp, par, bestc, beste, counters);
        unsigned long long hooked = 0;
        int rounds = 0;
        for (;;) {
            hipLaunchKernelGGL(k_or_offer<1>, pts, block, 0, c->stream, nbr, nrm, comp, bestc, beste, n, k);
            hipLaunchKernelGGL(k_or_offer<2>, pts, block, 0, c->stream, nbr, nrm, comp, bestc, beste, n, k);
            hipLaunchKernelGGL(k_or_hook, pts, block, 0, c->stream, nrm, comp, bestc, beste, n, par, counters);
            CHK(counters_fetch(c));
            hipLaunchKernelGGL(k_or_flatten, pts, block, 0, c->stream, comp, par, n, bestc, beste);
            HIPCHK(hipGetLastError());
            CHK(sync(c));
            const unsigned long long now = counters_host(c)[OR_HOOKED];
            if (now == hooked) break;
            hooked = now;
            if (++rounds > OR_MAX_ROUNDS) return fail(SICP_ERR_NUMERIC, "sicp_orient: more than %d rounds joined components", OR_MAX_ROUNDS);
        }
        // anchors, votes, verdicts (bestc and beste were reset by the last k_or_flatten: they hold the votes and the anchors now)
        const int have_ref = reference ? 1 : 0;
        hipLaunchKernelGGL(k_or_vote, pts, block, 0, c->stream, cl.x(), cl.y(), cl.z(), nrm, comp, n, have_ref, reference ? reference[0] : 0.0,
                           reference ? reference[1] : 0.0, reference ? reference[2] : 0.0, bestc, beste);
        hipLaunchKernelGGL(k_or_apply, pts, block, 0, c->stream, nrm, comp, bestc, beste, n, have_ref, away ? 1 : 0, dst, flip, counters);
        HIPCHK(hipGetLastError());
        CHK(counters_fetch(c));
        CHK(stage_leave(c, normals_out, (size_t)3 * n, dst));
        CHK(stage_leave(c, flipped_out, (size_t)n, flip));
        CHK(sync(c));
        const unsigned long long *h = counters_host(c);
        out->n_points = (int64_t)n;
        out->n_void = (int64_t)h[OR_VOID];
        out->n_components = (int64_t)h[OR_COMPONENTS];
        out->n_forest_edges = (int64_t)h[OR_HOOKED];
        out->n_flipped = (int64_t)h[OR_FLIPPED];
        out->n_components_voted = (int64_t)h[OR_VOTED];
        out->rounds = (int64_t)rounds;
        return SICP_OK;
    });
}
