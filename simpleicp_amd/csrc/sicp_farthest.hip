// sicp_farthest.hip -- farthest point sampling (include/simpleicp_hip_farthest.h; contract (S)).
//
// A pick is an argmax over m_i (larger value, then lower index) and an update m_i = min(m_i, d2(i, winner)): a sequence of m
// dependent steps, each a sweep over the cloud.  Two paths, the same bits:
//  * one workgroup (k_fp_one, n <= the ctx's farthest_one_max <= 12 288): 1 024 lanes hold R rows each -- coordinates and m_i in
//    registers, row lane + 1 024 j -- and make all m picks in one launch.  Per pick: the lane's update and argmax, the wave's
//    (value, index) maximum by DPP / permlane swaps, the 16 waves' through LDS and four more steps, then the winner's owner
//    publishes its coordinates in LDS: two barriers a pick, nothing but the outputs goes to memory.
//  * stepped (any n): m_i lives in device memory (-1.0 marks a row that is no candidate: it never wins and never updates); one
//    launch per pick, all of them enqueued blind.  Launch t first folds the per-workgroup partial maxima its predecessor left --
//    every workgroup does, redundantly, as k_lm_all folds its partials --, which settles the winner s_t or "ended"; workgroup 0
//    writes idx_out[t] / d2_out[t]; then every workgroup updates the m_i of its spans with s_t's row, and leaves its partial
//    maximum in the buffer of the other parity.  A workgroup that finds the selection ended leaves an ended partial again.  One
//    closing launch folds the last partials into cover_d2 and fills the outputs from n_selected on.
// No kernel waits for another wave or workgroup beyond __syncthreads; the only atomics are integer counts.
#include "sicp_host.h"
#include "sicp_lanes.h"
#include "../../include/simpleicp_hip_farthest.h"

namespace sicp {
namespace {

constexpr int FP_BLOCK = 256, FP_WAVES = FP_BLOCK / 64;   // a workgroup of the stepped path
constexpr int FP_MAX_WGS = 1024;                   // its grid limit: the workgroups stride over the spans from there on
constexpr long FP_MIN_SPAN = 256;                  // fewest rows a workgroup takes where the call chooses
constexpr int FP_ONE_BLOCK = 1024, FP_ONE_WAVES = FP_ONE_BLOCK / 64;   // the single workgroup
constexpr int FP_ONE_ROWS = 12;                    // most rows a lane of it holds: 96 VGPRs of data, 128 in all (13 compile without scratch too, 14 spill: profiles/farthest/)
static_assert((long)FP_ONE_BLOCK * FP_ONE_ROWS == SICP_FARTHEST_ONE_LIMIT, "the header states the single-workgroup limit");
static_assert(FP_ONE_WAVES == 16, "fp_best_row16 folds the waves' maxima inside a DPP row");
constexpr uint32_t FP_NONE = 0x7fffffffu;          // the index of "no row": above every row (n < 2^31)
enum { FP_SELECTED = 0, FP_CAND = 1, FP_COVER = 2 };   // the counter words: n_selected, n_candidates, the bits of cover_d2

// a workgroup's partial maximum between two launches: the value (-1.0: none, or the selection is ended) and its row
struct FpPart { double v; long long i; };
static_assert(sizeof(FpPart) == 2 * sizeof(double), "the partials lie in a buffer of doubles");

// contract (D)
__device__ __forceinline__ double fp_d2(double x, double y, double z, double sx, double sy, double sz)
{
    const double dx = x - sx, dy = y - sy, dz = z - sz;
    return fma(dz, dz, fma(dy, dy, dx * dx));
}

__device__ __forceinline__ bool fp_candidate(const double *__restrict__ X, const uint8_t *__restrict__ mask, long i, double &x, double &y,
                                             double &z)
{
    x = X[3 * i]; y = X[3 * i + 1]; z = X[3 * i + 2];
    return (!mask || mask[i] != 0) && finite_f64(x) && finite_f64(y) && finite_f64(z);
}

// (v, i) = the better of (v, i) and (ov, oi): the larger value, of equal values the lower row
__device__ __forceinline__ void fp_better(double &v, uint32_t &i, double ov, uint32_t oi)
{
    const bool take = ov > v || (ov == v && oi < i);
    v = take ? ov : v;
    i = take ? oi : i;
}
template <int J>
__device__ __forceinline__ void fp_best_step(double &v, uint32_t &i)
{
    const double ov = lane_xor_f64<J>(v);
    const uint32_t oi = lane_xor32<J>(i);
    fp_better(v, i, ov, oi);
}
// ... over the 16 lanes of a DPP row, over the wave: every lane ends up with the best pair
__device__ __forceinline__ void fp_best_row16(double &v, uint32_t &i)
{
    fp_best_step<8>(v, i); fp_best_step<4>(v, i); fp_best_step<2>(v, i); fp_best_step<1>(v, i);
}
__device__ __forceinline__ void fp_best_wave(double &v, uint32_t &i)
{
    fp_best_step<32>(v, i); fp_best_step<16>(v, i);
    fp_best_row16(v, i);
}

// ---- the stepped path ----
// the workgroup's (v, i) -> every thread has the workgroup's best (one barrier; wp: FP_WAVES pairs of LDS)
__device__ __forceinline__ void fp_best_block(double &v, uint32_t &i, FpPart *wp)
{
    fp_best_wave(v, i);
    if ((threadIdx.x & 63) == 0) { wp[threadIdx.x >> 6].v = v; wp[threadIdx.x >> 6].i = (long long)i; }
    __syncthreads();
    v = wp[0].v; i = (uint32_t)wp[0].i;
#pragma unroll
    for (int w = 1; w < FP_WAVES; ++w) fp_better(v, i, wp[w].v, (uint32_t)wp[w].i);
}

// the best of the g partials a launch left, in every thread
__device__ __forceinline__ void fp_fold(const FpPart *__restrict__ part, int g, double &v, uint32_t &i, FpPart *wp)
{
    v = -1.0; i = FP_NONE;
    for (int j = threadIdx.x; j < g; j += FP_BLOCK) fp_better(v, i, part[j].v, (uint32_t)part[j].i);
    fp_best_block(v, i, wp);
}

// m_i = +inf for a candidate, -1.0 for any other row; the partials of the first pick: the workgroup's lowest candidate (start < 0)
// or row `start` if it is a candidate, with +inf; st[FP_CAND] += the candidates
__global__ __launch_bounds__(FP_BLOCK) void k_fp_init(const double *__restrict__ X, const uint8_t *__restrict__ mask, double *__restrict__ mi,
                                                      FpPart *__restrict__ part, unsigned long long *__restrict__ st, long n, long span,
                                                      long start)
{
    __shared__ FpPart wp[FP_WAVES];
    const double inf = __builtin_inf();
    const long nspans = (n + span - 1) / span;
    double bv = -1.0;
    uint32_t bi = FP_NONE;
    unsigned cand = 0;
    for (long sp = blockIdx.x; sp < nspans; sp += gridDim.x) {
        const long lo = sp * span, hi = lo + span < n ? lo + span : n;
        for (long i = lo + threadIdx.x; i < hi; i += FP_BLOCK) {
            double x, y, z;
            const bool c = fp_candidate(X, mask, i, x, y, z);
            mi[i] = c ? inf : -1.0;
            cand += c ? 1u : 0u;
            if (c && (start < 0 || i == start) && bv < 0.0) { bv = inf; bi = (uint32_t)i; }   // (a thread's rows ascend)
        }
    }
    cand = wsum_u32(cand);
    if ((threadIdx.x & 63) == 0 && cand) atomicAdd(st + FP_CAND, (unsigned long long)cand);
    fp_best_block(bv, bi, wp);
    if (threadIdx.x == 0) { part[blockIdx.x].v = bv; part[blockIdx.x].i = (long long)bi; }
}

// Pick t: the winner of the partials at `prev`, the update of every m_i with its row, the workgroup's new partial at `next`.
__global__ __launch_bounds__(FP_BLOCK) void k_fp_pick(const double *__restrict__ X, double *__restrict__ mi, const FpPart *__restrict__ prev,
                                                      FpPart *__restrict__ next, int64_t *__restrict__ idx_out, double *__restrict__ d2_out,
                                                      unsigned long long *__restrict__ st, long n, long span, long t)
{
    __shared__ FpPart wp[FP_WAVES], wq[FP_WAVES];
    double v;
    uint32_t s;
    fp_fold(prev, (int)gridDim.x, v, s, wp);
    if (!(v > 0.0)) {                                                  // ended (the same in every thread of every workgroup)
        if (threadIdx.x == 0) { next[blockIdx.x].v = -1.0; next[blockIdx.x].i = (long long)FP_NONE; }
        return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        idx_out[t] = (int64_t)s;
        if (d2_out) d2_out[t] = v;
        st[FP_SELECTED] = (unsigned long long)(t + 1);
    }
    const double sx = X[3 * (long)s], sy = X[3 * (long)s + 1], sz = X[3 * (long)s + 2];
    const long nspans = (n + span - 1) / span;
    double bv = -1.0;
    uint32_t bi = FP_NONE;
    for (long sp = blockIdx.x; sp < nspans; sp += gridDim.x) {
        const long lo = sp * span, hi = lo + span < n ? lo + span : n;
        for (long i = lo + threadIdx.x; i < hi; i += FP_BLOCK) {
            double m = mi[i];
            if (m >= 0.0) {
                const double d = fp_d2(X[3 * i], X[3 * i + 1], X[3 * i + 2], sx, sy, sz);
                if (d < m) { m = d; mi[i] = d; }
                if (m > bv) { bv = m; bi = (uint32_t)i; }              // (a thread's rows ascend: the lowest of equal values stays)
            }
        }
    }
    fp_best_block(bv, bi, wq);
    if (threadIdx.x == 0) { next[blockIdx.x].v = bv; next[blockIdx.x].i = (long long)bi; }
}

// Behind the last pick, one workgroup: cover_d2 from the g partials at `prev`, the outputs from n_selected on
__global__ __launch_bounds__(FP_BLOCK) void k_fp_close(const FpPart *__restrict__ prev, int g, int64_t *__restrict__ idx_out,
                                                       double *__restrict__ d2_out, unsigned long long *__restrict__ st, long m)
{
    __shared__ FpPart wp[FP_WAVES];
    double v;
    uint32_t s;
    fp_fold(prev, g, v, s, wp);
    const long taken = (long)st[FP_SELECTED];
    for (long k = taken + threadIdx.x; k < m; k += FP_BLOCK) {
        idx_out[k] = -1;
        if (d2_out) d2_out[k] = 0.0;
    }
    if (threadIdx.x == 0) st[FP_COVER] = (unsigned long long)__double_as_longlong(v > 0.0 ? v : 0.0);
}

// ---- the single workgroup ----
// the workgroup's (v, i) -> every thread has the workgroup's best (one barrier)
__device__ __forceinline__ void fp_one_best(double &v, uint32_t &i, double *wv, uint32_t *wi)
{
    const int lane = threadIdx.x & 63;
    fp_best_wave(v, i);
    if (lane == 0) { wv[threadIdx.x >> 6] = v; wi[threadIdx.x >> 6] = i; }
    __syncthreads();
    v = wv[lane & 15]; i = wi[lane & 15];                              // (every DPP row of the wave holds the 16 waves' pairs)
    fp_best_row16(v, i);
}

// All m picks of a cloud of n <= 1 024 R rows (R = 1, 2, 4, 8, 12).  Lane l holds the rows l + 1 024 j, j < R.
template <int R>
__global__ __launch_bounds__(FP_ONE_BLOCK) void k_fp_one(const double *__restrict__ X, const uint8_t *__restrict__ mask,
                                                         int64_t *__restrict__ idx_out, double *__restrict__ d2_out,
                                                         unsigned long long *__restrict__ st, long n, long m, long start)
{
    __shared__ double wv[FP_ONE_WAVES], win[3];
    __shared__ uint32_t wi[FP_ONE_WAVES];
    const double inf = __builtin_inf();
    double x[R], y[R], z[R], mm[R];
    double bv = -1.0;
    uint32_t bi = FP_NONE;
    unsigned cand = 0;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const long i = (long)threadIdx.x + (long)j * FP_ONE_BLOCK;
        bool c = false;
        x[j] = y[j] = z[j] = 0.0;
        if (i < n) c = fp_candidate(X, mask, i, x[j], y[j], z[j]);
        mm[j] = c ? inf : -1.0;
        cand += c ? 1u : 0u;
        if (c && (start < 0 || i == start) && bv < 0.0) { bv = inf; bi = (uint32_t)i; }
    }
    cand = wsum_u32(cand);
    if ((threadIdx.x & 63) == 0 && cand) atomicAdd(st + FP_CAND, (unsigned long long)cand);
    fp_one_best(bv, bi, wv, wi);
    long t = 0;
    while (bv > 0.0 && t < m) {
        if (threadIdx.x == 0) {
            idx_out[t] = (int64_t)bi;
            if (d2_out) d2_out[t] = bv;
        }
        if ((bi & (FP_ONE_BLOCK - 1)) == threadIdx.x) {                // the owner (selects on scalars: indexed by jj the rows would go to scratch)
            const int jj = (int)(bi / FP_ONE_BLOCK);
            double px = x[0], py = y[0], pz = z[0];
#pragma unroll
            for (int j = 1; j < R; ++j) {
                px = jj == j ? x[j] : px; py = jj == j ? y[j] : py; pz = jj == j ? z[j] : pz;
            }
            win[0] = px; win[1] = py; win[2] = pz;
        }
        __syncthreads();
        const double sx = win[0], sy = win[1], sz = win[2];
        ++t;
        bv = -1.0; bi = FP_NONE;
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const double d = fp_d2(x[j], y[j], z[j], sx, sy, sz);
            const double mj = (mm[j] >= 0.0 && d < mm[j]) ? d : mm[j];
            mm[j] = mj;
            if (mj > bv) { bv = mj; bi = threadIdx.x + (uint32_t)j * FP_ONE_BLOCK; }   // (j ascends: the lowest of equal values stays)
        }
        fp_one_best(bv, bi, wv, wi);                                   // (its barrier also fences `win`)
    }
    for (long k = t + threadIdx.x; k < m; k += FP_ONE_BLOCK) {
        idx_out[k] = -1;
        if (d2_out) d2_out[k] = 0.0;
    }
    if (threadIdx.x == 0) {
        st[FP_SELECTED] = (unsigned long long)t;
        st[FP_COVER] = (unsigned long long)__double_as_longlong(bv > 0.0 ? bv : 0.0);
    }
}

}  // namespace
}  // namespace sicp

namespace {

template <int R>
void one_launch(sicp_ctx *c, const double *x, const uint8_t *msk, int64_t *idx, double *d2, long n, long m, long start)
{
    hipLaunchKernelGGL(k_fp_one<R>, dim3(1), dim3(FP_ONE_BLOCK), 0, c->stream, x, msk, idx, d2, c->cand_small.p, n, m, start);
}

}  // namespace

SICP_EXPORT int sicp_farthest_version(void) { return SICP_FARTHEST_VERSION; }

SICP_EXPORT int sicp_farthest(sicp_ctx *c, const double *X, const uint8_t *mask, int64_t n, int64_t m, int64_t start, int64_t *idx_out,
                              double *d2_out, sicp_farthest_stats *out)
{
    CHK(check_rows_ctx(c, "sicp_farthest"));
    if (!X) return fail(SICP_ERR_INVALID, "X is null");
    if (n < 1) return fail(SICP_ERR_INVALID, "n must be >= 1 (%lld given)", (long long)n);
    if (n >= (1LL << 31)) return fail(SICP_ERR_INVALID, "n must be < 2^31 (%lld given)", (long long)n);
    if (!idx_out) return fail(SICP_ERR_INVALID, "idx_out is null");
    if (!out) return fail(SICP_ERR_INVALID, "out is null");
    if (m < 1 || m > n) return fail(SICP_ERR_INVALID, "m must be >= 1 and <= n (%lld given, n = %lld)", (long long)m, (long long)n);
    if (start < -1 || start >= n) return fail(SICP_ERR_INVALID, "start must be -1 or a row, 0 .. n-1 (%lld given, n = %lld)", (long long)start, (long long)n);
    HIPCHK(hipSetDevice(c->device));
    return op_run(c, [&]() -> int {
        const double *x;
        const uint8_t *msk = nullptr;
        int64_t *idx;
        double *d2;
        CHK(stage_in(c, X, (size_t)3 * n, c->gl_src, &x));
        if (mask) CHK(stage_in(c, mask, (size_t)n, c->fp_mask, &msk));
        CHK(stage_out(c, idx_out, (size_t)m, c->fp_idx, &idx));
        CHK(stage_out(c, d2_out, (size_t)m, c->fp_d2, &d2));
        CHK(counters_clear(c));
        if (n <= std::min<long>(c->farthest_one_max, SICP_FARTHEST_ONE_LIMIT)) {
            // the fewest rows a lane that hold the cloud: the picks' cost is the lanes' sweep over their rows
            if (n <= 1L * FP_ONE_BLOCK) one_launch<1>(c, x, msk, idx, d2, (long)n, (long)m, (long)start);
            else if (n <= 2L * FP_ONE_BLOCK) one_launch<2>(c, x, msk, idx, d2, (long)n, (long)m, (long)start);
            else if (n <= 4L * FP_ONE_BLOCK) one_launch<4>(c, x, msk, idx, d2, (long)n, (long)m, (long)start);
            else if (n <= 8L * FP_ONE_BLOCK) one_launch<8>(c, x, msk, idx, d2, (long)n, (long)m, (long)start);
            else one_launch<FP_ONE_ROWS>(c, x, msk, idx, d2, (long)n, (long)m, (long)start);
            HIPCHK(hipGetLastError());
        } else {
            // rows per workgroup: the ctx's switch, else whole waves of rows, as many as keep the grid at FP_MAX_WGS workgroups
            const long span = c->farthest_span > 0 ? c->farthest_span
                                                   : std::max<long>(FP_MIN_SPAN, round_up(((long)n + FP_MAX_WGS - 1) / FP_MAX_WGS, 64));
            const unsigned g = (unsigned)std::min<long>(((long)n + span - 1) / span, FP_MAX_WGS);
            CHK(c->fp_m.reserve((size_t)n));
            CHK(c->fp_part.reserve((size_t)2 * 2 * FP_MAX_WGS));
            FpPart *part[2] = {(FpPart *)c->fp_part.p, (FpPart *)c->fp_part.p + FP_MAX_WGS};
            hipLaunchKernelGGL(k_fp_init, dim3(g), dim3(FP_BLOCK), 0, c->stream, x, msk, c->fp_m.p, part[0], c->cand_small.p, (long)n, span,
                               (long)start);
            HIPCHK(hipGetLastError());
            for (long t = 0; t < (long)m; ++t) {                       // (blind: a pick that finds the selection ended does nothing)
                hipLaunchKernelGGL(k_fp_pick, dim3(g), dim3(FP_BLOCK), 0, c->stream, x, c->fp_m.p, (const FpPart *)part[t & 1], part[(t + 1) & 1],
                                   idx, d2, c->cand_small.p, (long)n, span, t);
                HIPCHK(hipGetLastError());
            }
            hipLaunchKernelGGL(k_fp_close, dim3(1), dim3(FP_BLOCK), 0, c->stream, (const FpPart *)part[m & 1], (int)g, idx, d2, c->cand_small.p,
                               (long)m);
            HIPCHK(hipGetLastError());
        }
        CHK(counters_fetch(c));
        CHK(stage_leave(c, idx_out, (size_t)m, idx));
        CHK(stage_leave(c, d2_out, (size_t)m, d2));
        CHK(sync(c));
        const unsigned long long *hs = counters_host(c);
        out->n_points = n;
        out->n_candidates = (int64_t)hs[FP_CAND];
        out->n_selected = (int64_t)hs[FP_SELECTED];
        std::memcpy(&out->cover_d2, &hs[FP_COVER], sizeof(double));
        return SICP_OK;
    });
}
