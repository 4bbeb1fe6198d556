// sicp_consistency.hip -- matches pruned by pairwise length consistency (include/simpleicp_hip_consistency.h; contract (C),
// DESIGN.md section 21).
//
// Build (k_cons_build): the compatibility matrix as bits, m rows of W = ceil(m / 64) words.  The grid is (blocks of CB_ROWS rows) x
// (chunks of CB_WORDS words); a wave owns CB_RPW rows and walks its chunk's columns 64 at a time: lane l holds column 64 w + l's
// six coordinates in registers for all of the wave's rows, the rows' coordinates lie in LDS (read by broadcast).  The wave's ballot
// of the verdict is word w of the row, its popcount adds to the row's degree.  Lane (w - w0) keeps word w, so a row's chunk leaves
// as one coalesced store of up to 64 words; the degrees leave by one integer atomic add per row and chunk.
//
// Peeling.  The level jumps to the smallest remaining degree: k = max(k, min degree of the rows alive); the frontier {alive,
// degree <= k} gets core k and leaves; every row still alive loses popcount(row & frontier).  Words of the row whose frontier word
// is zero are not read.
// One-launch path (m <= CS_ONE_MAX): one workgroup (k_cons_one) peels the whole graph, degrees and frontier in LDS, the rows
// re-read from L2.
// Sweeps path (any m): a sub-round is k_cons_front (one thread a row: the level from the minimum the last sweep left, the
// frontier's bits, the cores) and k_cons_sweep (CS_G lanes a row, the frontier read into LDS).  The minimum of the remaining degrees
// exists only behind a kernel boundary, hence the two launches; there is no grid barrier, no ticket and no hand-over.  The host
// enqueues CS_BATCH sub-rounds at a time and reads the counter words once per batch; a sub-round behind the end costs its
// workgroups one load.
#include "sicp_host.h"
#include "sicp_lanes.h"
#include "../../include/simpleicp_hip_consistency.h"

namespace sicp {
namespace {

constexpr int CB_BLOCK = 256, CB_WAVES = CB_BLOCK / 64;
constexpr int CB_RPW = 8;                          // rows a wave owns
constexpr int CB_ROWS = CB_WAVES * CB_RPW;         // rows of a workgroup (32)
constexpr int CB_WORDS = 64;                       // words of a column chunk: what one coalesced store of a row holds (4 096 columns)
constexpr int CS_BLOCK = 256;                      // threads of the peeling's kernels of the sweeps path
constexpr int CS_PASSES = 8;                       // ... and the passes of CS_BLOCK / G rows a workgroup of the sweep makes with one copy of the frontier
constexpr int CS_ONE = 1024, CS_ONE_WAVES = CS_ONE / 64;   // the one-launch path's workgroup
constexpr long CS_ONE_MAX = 4096;                  // ... and the most rows it takes: their degrees (16 KB) and frontier in LDS, a row one word a lane
constexpr long CS_ONE_DEFAULT_MAX = 1024;          // ... and the most rows at which it is the default (DESIGN.md section 21 has the record)
constexpr int CS_BATCH = 16;                       // sub-rounds the host enqueues between two looks at the counter words
constexpr long CS_MAX_WORDS = SICP_CONSISTENCY_MAX_ROWS / 64;
constexpr unsigned CS_NONE = 0xffffffffu;          // the minimum over no row
// the counter words (c->cand_small; word CAND_COUNT is not used)
enum { CS_VALID = 0, CS_SUM = 1, CS_MAXDEG = 2, CS_MAXCORE = 3, CS_NMAX = 4, CS_ALIVE = 6, CS_SUBR = 7 };
static_assert(CS_SUBR < CAND_WORDS && CAND_COUNT == 5, "the record's counters fit the ctx's counter words");
// the level words (c->cs_state): [CS_MIN + parity] the smallest remaining degree a sweep left for the sub-round of that parity,
// [CS_LEVEL + parity] the level before it
enum { CS_MIN = 0, CS_LEVEL = 2, CS_STATE_WORDS = 4 };

__device__ __forceinline__ bool finite3(const double (&v)[3]) { return finite_f64(v[0]) && finite_f64(v[1]) && finite_f64(v[2]); }

// contract (D) between two points, and the length
__device__ __forceinline__ double cs_length(const double *u, const double (&v)[3])
{
    const double dx = u[0] - v[0], dy = u[1] - v[1], dz = u[2] - v[2];
    return sqrt(fma(dz, dz, fma(dy, dy, dx * dx)));
}

__device__ __forceinline__ unsigned wave_min_u32(unsigned v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const unsigned o = (unsigned)__shfl_xor((int)v, off); v = o < v ? o : v; }
    return v;
}

// ---- the build ----
__global__ __launch_bounds__(CB_BLOCK) void k_cons_build(const double *__restrict__ src, const double *__restrict__ dst, long m, long W,
                                                         double tolerance, double min_length, unsigned long long *__restrict__ bits,
                                                         int32_t *__restrict__ degree)
{
    __shared__ double rp[CB_ROWS][3], rq[CB_ROWS][3];
    __shared__ int rv[CB_ROWS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long row0 = (long)blockIdx.x * CB_ROWS;
    const long w0 = (long)blockIdx.y * CB_WORDS, w1 = w0 + CB_WORDS < W ? w0 + CB_WORDS : W;
    if (threadIdx.x < CB_ROWS) {
        const long r = row0 + threadIdx.x;
        double p[3] = {0.0, 0.0, 0.0}, q[3] = {0.0, 0.0, 0.0};
        if (r < m) {
#pragma unroll
            for (int i = 0; i < 3; ++i) { p[i] = src[3 * r + i]; q[i] = dst[3 * r + i]; }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) { rp[threadIdx.x][i] = p[i]; rq[threadIdx.x][i] = q[i]; }
        rv[threadIdx.x] = r < m && finite3(p) && finite3(q);
    }
    __syncthreads();
    unsigned long long mine[CB_RPW];
    int deg[CB_RPW];
#pragma unroll
    for (int r = 0; r < CB_RPW; ++r) { mine[r] = 0; deg[r] = 0; }
    for (long w = w0; w < w1; ++w) {
        const long j = 64 * w + lane;
        double p[3] = {0.0, 0.0, 0.0}, q[3] = {0.0, 0.0, 0.0};
        bool cv = false;
        if (j < m) {
#pragma unroll
            for (int i = 0; i < 3; ++i) { p[i] = src[3 * j + i]; q[i] = dst[3 * j + i]; }
            cv = finite3(p) && finite3(q);
        }
#pragma unroll
        for (int r = 0; r < CB_RPW; ++r) {
            const int rr = wave * CB_RPW + r;
            bool ok = false;
            if (rv[rr] && cv && row0 + rr != j) {                      // (rv: the same for the whole wave)
                const double a = cs_length(rp[rr], p), b = cs_length(rq[rr], q);
                ok = finite_f64(a) && finite_f64(b) && fabs(a - b) <= tolerance && a >= min_length && b >= min_length;
            }
            const unsigned long long word = (unsigned long long)__ballot(ok);
            if (lane == (int)(w - w0)) mine[r] = word;
            deg[r] += __popcll(word);
        }
    }
#pragma unroll
    for (int r = 0; r < CB_RPW; ++r) {
        const long i = row0 + wave * CB_RPW + r;
        if (i < m) {
            if (w0 + lane < w1) bits[i * W + w0 + lane] = mine[r];
            if (lane == 0 && deg[r]) atomicAdd(degree + i, deg[r]);
        }
    }
}

// the degrees' record, the valid rows, the rows alive (all), and for the sweeps path (work != null) the remaining degrees and
// the first sub-round's minimum
__global__ __launch_bounds__(CS_BLOCK) void k_cons_begin(const double *__restrict__ src, const double *__restrict__ dst,
                                                         const int32_t *__restrict__ degree, long m, int32_t *__restrict__ work,
                                                         unsigned *__restrict__ st, unsigned long long *__restrict__ cnt)
{
    const long i = (long)blockIdx.x * CS_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool valid = false;
    unsigned d = 0;
    if (i < m) {
        double p[3], q[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { p[k] = src[3 * i + k]; q[k] = dst[3 * i + k]; }
        valid = finite3(p) && finite3(q);
        d = (unsigned)degree[i];
        if (work) work[i] = (int32_t)d;
    }
    const unsigned n_valid = (unsigned)__popcll((unsigned long long)__ballot(valid));
    const unsigned n_rows = (unsigned)__popcll((unsigned long long)__ballot(i < m));
    const unsigned mn = wave_min_u32(i < m ? d : CS_NONE);
    unsigned mx = d, sum = d;                                          // (d = 0 beyond m)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)mx, off);
        mx = o > mx ? o : mx;
        sum += (unsigned)__shfl_xor((int)sum, off);
    }
    if (lane == 0 && n_rows) {
        if (n_valid) atomicAdd(cnt + CS_VALID, (unsigned long long)n_valid);
        if (sum) atomicAdd(cnt + CS_SUM, (unsigned long long)sum);
        atomicMax(cnt + CS_MAXDEG, (unsigned long long)mx);
        atomicAdd(cnt + CS_ALIVE, (unsigned long long)n_rows);
        if (st) atomicMin(st + CS_MIN, mn);
    }
}

// what a row still alive loses: popcount(row & frontier) over the words sub, sub + G, ... -- summed over the row's G lanes (a
// power of two <= 64, aligned in the wave); called by every lane of the wave
__device__ __forceinline__ int cs_row_loss(const unsigned long long *__restrict__ row, const unsigned long long *F, long W, int sub, int G,
                                           bool alive)
{
    int n = 0;
    if (alive) {
        for (long w = sub; w < W; w += G) {
            const unsigned long long f = F[w];
            if (f) n += __popcll(row[w] & f);
        }
    }
    for (int off = G >> 1; off > 0; off >>= 1) n += __shfl_xor(n, off);
    return n;
}

// ---- the one-launch path ----
__global__ __launch_bounds__(CS_ONE) void k_cons_one(const unsigned long long *__restrict__ bits, const int32_t *__restrict__ degree, long m,
                                                     long W, int G, int32_t *__restrict__ core, unsigned long long *__restrict__ cnt)
{
    __shared__ int deg[CS_ONE_MAX];
    __shared__ unsigned long long F[CS_ONE_MAX / 64];
    __shared__ unsigned wmin[CS_ONE_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long i = threadIdx.x; i < m; i += CS_ONE) deg[i] = degree[i];
    __syncthreads();
    int k = 0;
    unsigned long long subrounds = 0;
    for (;;) {
        unsigned mn = CS_NONE;
        for (long i = threadIdx.x; i < m; i += CS_ONE) {
            const int d = deg[i];
            if (d >= 0 && (unsigned)d < mn) mn = (unsigned)d;
        }
        mn = wave_min_u32(mn);
        if (lane == 0) wmin[wave] = mn;
        __syncthreads();
        mn = CS_NONE;
#pragma unroll
        for (int v = 0; v < CS_ONE_WAVES; ++v) mn = wmin[v] < mn ? wmin[v] : mn;
        __syncthreads();                                               // (wmin is written again)
        if (mn == CS_NONE) break;                                      // (the same for the whole workgroup)
        k = (int)mn > k ? (int)mn : k;
        ++subrounds;
        for (long base = 0; base < m; base += CS_ONE) {
            const long i = base + threadIdx.x;
            const int d = i < m ? deg[i] : -1;
            const bool in = d >= 0 && d <= k;
            const unsigned long long word = (unsigned long long)__ballot(in);
            if (lane == 0 && base + 64 * wave < m) F[(base >> 6) + wave] = word;
            if (in) { core[i] = k; deg[i] = -1; }
        }
        __syncthreads();
        const int per = CS_ONE / G, sub = threadIdx.x % G;
        for (long base = 0; base < m; base += per) {
            const long row = base + threadIdx.x / G;
            const int d = row < m ? deg[row] : -1;
            const int loss = cs_row_loss(bits + (row < m ? row : 0) * W, F, W, sub, G, d >= 0);
            if (sub == 0 && d >= 0) deg[row] = d - loss;
        }
        __syncthreads();
    }
    // the record: the last level is the largest core number
    if (k >= 1) {
        unsigned n = 0;
        for (long base = 0; base < m; base += CS_ONE) {
            const long i = base + threadIdx.x;
            n += (unsigned)__popcll((unsigned long long)__ballot(i < m && core[i] == k));
        }
        if (lane == 0 && n) atomicAdd(cnt + CS_NMAX, (unsigned long long)n);
    }
    if (threadIdx.x == 0) { cnt[CS_MAXCORE] = (unsigned long long)k; cnt[CS_SUBR] = subrounds; cnt[CS_ALIVE] = 0; }
}

// ---- the sweeps path ----
// sub-round `par`ity: the level, the frontier's bits (every word of front is written), the cores; the rows leave
__global__ __launch_bounds__(CS_BLOCK) void k_cons_front(int32_t *__restrict__ work, long m, int par, unsigned *__restrict__ st,
                                                         unsigned long long *__restrict__ front, int32_t *__restrict__ core,
                                                         unsigned long long *__restrict__ cnt)
{
    const unsigned mn = st[CS_MIN + par];
    if (mn == CS_NONE) return;                                         // nobody is alive: one load
    const unsigned before = st[CS_LEVEL + par];
    const int k = (int)(mn > before ? mn : before);
    const long i = (long)blockIdx.x * CS_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int d = i < m ? work[i] : -1;
    const bool in = d >= 0 && d <= k;
    const unsigned long long word = (unsigned long long)__ballot(in);
    if (in) { core[i] = k; work[i] = -1; }
    if (lane == 0 && i < m) {                                          // (i: the wave's first row, a multiple of 64)
        front[i >> 6] = word;
        if (word) atomicAdd(cnt + CS_ALIVE, (unsigned long long)-(long long)__popcll(word));
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st[CS_MIN + (par ^ 1)] = CS_NONE;                              // (the sweep behind this launch takes its minimum there)
        st[CS_LEVEL + (par ^ 1)] = (unsigned)k;
        cnt[CS_MAXCORE] = (unsigned long long)k;
        cnt[CS_SUBR] += 1;
    }
}

// ... every row still alive loses its partners in the frontier; the smallest of what remains goes to the next sub-round
__global__ __launch_bounds__(CS_BLOCK) void k_cons_sweep(const unsigned long long *__restrict__ bits, const unsigned long long *__restrict__ front,
                                                         int32_t *__restrict__ work, long m, long W, int G, int par,
                                                         unsigned *__restrict__ st, const unsigned long long *__restrict__ cnt)
{
    __shared__ unsigned long long F[CS_MAX_WORDS];
    if (cnt[CS_ALIVE] == 0) {                                          // the graph is empty: one load
        if (blockIdx.x == 0 && threadIdx.x == 0) st[CS_MIN] = st[CS_MIN + 1] = CS_NONE;    // (every later sub-round sees it)
        return;
    }
    for (long w = threadIdx.x; w < W; w += CS_BLOCK) F[w] = front[w];
    __syncthreads();
    const int per = CS_BLOCK / G, sub = threadIdx.x % G;
    unsigned mn = CS_NONE;
#pragma unroll 1
    for (int pass = 0; pass < CS_PASSES; ++pass) {                     // (as many passes in every lane: the shuffles are the wave's)
        const long row = ((long)blockIdx.x * CS_PASSES + pass) * per + threadIdx.x / G;
        const int d = row < m ? work[row] : -1;
        const int loss = cs_row_loss(bits + (row < m ? row : 0) * W, F, W, sub, G, d >= 0);
        if (sub == 0 && d >= 0) work[row] = d - loss;
        if (d >= 0 && (unsigned)(d - loss) < mn) mn = (unsigned)(d - loss);
    }
    mn = wave_min_u32(mn);
    if ((threadIdx.x & 63) == 0 && mn != CS_NONE) atomicMin(st + CS_MIN + (par ^ 1), mn);
}

// the rows of the largest core number, once nobody is alive
__global__ __launch_bounds__(CS_BLOCK) void k_cons_tally(const int32_t *__restrict__ core, long m, unsigned long long *__restrict__ cnt)
{
    if (cnt[CS_ALIVE] != 0) return;
    const long long k = (long long)cnt[CS_MAXCORE];
    if (k < 1) return;
    const long i = (long)blockIdx.x * CS_BLOCK + threadIdx.x;
    const unsigned n = (unsigned)__popcll((unsigned long long)__ballot(i < m && core[i] == k));
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(cnt + CS_NMAX, (unsigned long long)n);
}

}  // namespace
}  // namespace sicp

SICP_EXPORT int sicp_consistency_version(void) { return SICP_CONSISTENCY_VERSION; }

SICP_EXPORT int sicp_match_consistency(sicp_ctx *c, const double *src, const double *dst, int64_t m, double tolerance, double min_length,
                                       int32_t *degree_out, int32_t *core_out, sicp_consistency_stats *out)
{
    CHK(check_rows_ctx(c, "sicp_match_consistency"));
    CHK(check_matched(src, dst));
    if (!degree_out) return fail(SICP_ERR_INVALID, "degree_out is null");
    if (!core_out) return fail(SICP_ERR_INVALID, "core_out is null");
    if (!out) return fail(SICP_ERR_INVALID, "out is null");
    if (m < 3) return fail(SICP_ERR_INVALID, "m must be >= 3 (%lld given)", (long long)m);
    if (m > SICP_CONSISTENCY_MAX_ROWS)
        return fail(SICP_ERR_INVALID, "m must be <= %d (%lld given): thin the matches first", SICP_CONSISTENCY_MAX_ROWS, (long long)m);
    if (!std::isfinite(tolerance) || !(tolerance > 0.0)) return fail(SICP_ERR_INVALID, "tolerance must be finite and > 0");
    if (!std::isfinite(min_length) || min_length < 0.0) return fail(SICP_ERR_INVALID, "min_length must be finite and >= 0");
    HIPCHK(hipSetDevice(c->device));
    return op_run(c, [&]() -> int {
        const long M = (long)m, W = (M + 63) / 64;
        const double *s, *d;
        int32_t *deg, *core;
        CHK(stage_in(c, src, (size_t)3 * M, c->gl_src, &s));
        CHK(stage_in(c, dst, (size_t)3 * M, c->gl_dst, &d));
        CHK(stage_out(c, degree_out, (size_t)M, c->gl_idx, &deg));
        CHK(stage_out(c, core_out, (size_t)M, c->cs_core, &core));
        CHK(c->cs_bits.reserve((size_t)M * W));
        CHK(counters_clear(c));
        unsigned long long *cnt = c->cand_small.p;
        HIPCHK(hipMemsetAsync(deg, 0, (size_t)M * sizeof(int32_t), c->stream));
        hipLaunchKernelGGL(k_cons_build, dim3(cdiv(M, CB_ROWS), cdiv(W, CB_WORDS)), dim3(CB_BLOCK), 0, c->stream, s, d, M, W, tolerance,
                           min_length, c->cs_bits.p, deg);
        HIPCHK(hipGetLastError());
        int G = 1;                                                     // lanes a row of the peeling: the power of two that covers W, 64 at most
        while (G < 64 && G < W) G *= 2;
        const bool fits = M <= CS_ONE_MAX;
        const bool one = fits && (c->consistency_path == 2 || (c->consistency_path == 0 && M <= CS_ONE_DEFAULT_MAX));
        const dim3 rows(cdiv(M, CS_BLOCK));
        if (one) {
            hipLaunchKernelGGL(k_cons_begin, rows, dim3(CS_BLOCK), 0, c->stream, s, d, deg, M, (int32_t *)nullptr, (unsigned *)nullptr, cnt);
            hipLaunchKernelGGL(k_cons_one, dim3(1), dim3(CS_ONE), 0, c->stream, c->cs_bits.p, deg, M, W, G, core, cnt);
            HIPCHK(hipGetLastError());
            CHK(counters_fetch(c));
        } else {
            CHK(c->cs_work.reserve((size_t)M));
            CHK(c->cs_front.reserve((size_t)CS_MAX_WORDS));
            CHK(c->cs_state.reserve(CS_STATE_WORDS));
            unsigned *st = c->cs_state.p;
            HIPCHK(hipMemsetAsync(st + CS_MIN, 0xff, 2 * sizeof(unsigned), c->stream));
            HIPCHK(hipMemsetAsync(st + CS_LEVEL, 0, 2 * sizeof(unsigned), c->stream));
            hipLaunchKernelGGL(k_cons_begin, rows, dim3(CS_BLOCK), 0, c->stream, s, d, deg, M, c->cs_work.p, st, cnt);
            HIPCHK(hipGetLastError());
            const dim3 sweep(cdiv(M, (long)CS_PASSES * (CS_BLOCK / G)));
            for (long sub = 0;;) {                                     // (every sub-round with somebody alive takes a row: at most m)
                for (int b = 0; b < CS_BATCH; ++b, ++sub) {
                    const int par = (int)(sub & 1);
                    hipLaunchKernelGGL(k_cons_front, rows, dim3(CS_BLOCK), 0, c->stream, c->cs_work.p, M, par, st, c->cs_front.p, core, cnt);
                    hipLaunchKernelGGL(k_cons_sweep, sweep, dim3(CS_BLOCK), 0, c->stream, c->cs_bits.p, c->cs_front.p, c->cs_work.p, M, W, G,
                                       par, st, cnt);
                }
                hipLaunchKernelGGL(k_cons_tally, rows, dim3(CS_BLOCK), 0, c->stream, core, M, cnt);
                HIPCHK(hipGetLastError());
                CHK(counters_fetch(c));
                CHK(sync(c));
                if (counters_host(c)[CS_ALIVE] == 0) break;
                if (sub > M) return fail(SICP_ERR_NUMERIC, "sicp_match_consistency: the peeling did not end");
            }
        }
        CHK(stage_leave(c, degree_out, (size_t)M, deg));
        CHK(stage_leave(c, core_out, (size_t)M, core));
        CHK(sync(c));
        const unsigned long long *hs = counters_host(c);
        out->n_rows = m;
        out->n_valid = (int64_t)hs[CS_VALID];
        out->n_edges = (int64_t)(hs[CS_SUM] / 2);
        out->max_degree = (int64_t)hs[CS_MAXDEG];
        out->max_core = (int64_t)hs[CS_MAXCORE];
        out->n_max_core = (int64_t)hs[CS_NMAX];
        out->n_subrounds = (int64_t)hs[CS_SUBR];
        return SICP_OK;
    });
}
