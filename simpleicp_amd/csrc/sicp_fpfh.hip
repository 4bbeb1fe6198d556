// sicp_fpfh.hip -- FPFH descriptors (include/simpleicp_hip_fpfh.h; contract (F)).
//
// Two passes over chunks of points, shaped like the statistical outlier filter: a chunk's points go through the slot's k-NN search
// (knnk_device), then a kernel reads that chunk's ranked (chunk, k) lists.  Pass 1 (k_fpfh_spfh): one wave per point, lanes over the
// neighbours; every lane forms its pair feature and its three bins, ballots and popcounts turn them into the 33 exact counts and m_i.
// Pass 2 (k_fpfh_final) starts once pass 1 has covered the cloud and searches each chunk AGAIN (the lists are not kept: 16 k bytes
// per point): one wave per point, lanes over the 33 bins, the neighbours walked in rank order, 68 bytes gathered per neighbour.
// Integer atomics count the record; no floating-point atomic takes part.
#include "sicp_host.h"
#include "sicp_lanes.h"
#include "../../include/simpleicp_hip_fpfh.h"

namespace sicp {
namespace {

constexpr int FP_BLOCK = 256;
constexpr int FP_WAVES = FP_BLOCK / 64;
constexpr int FP_MAX_BLOCKS = 4096;                // the waves stride over the chunk's points from there on
constexpr int FP_ROW = SICP_FPFH_BINS + 1;         // a point's counts: 33 bins and m_i

// min(10, max(0, floor(11 * ((f + 1) * 0.5)))), clamped in float64 before the conversion; a NaN gives 0
__device__ __forceinline__ int fp_bin11(double f)
{
    const double t = floor(11.0 * ((f + 1.0) * 0.5));
    return t >= 10.0 ? 10 : (t > 0.0 ? (int)t : 0);
}

// the sector of the direction (b, a): how many of the ten borders it has reached
__device__ __forceinline__ int fp_sector(double a, double b)
{
    constexpr double B[10][2] = SICP_FPFH_BORDERS;
    int below = 0, above = 5;
#pragma unroll
    for (int j = 0; j < 5; ++j) below += (B[j][0] * a - B[j][1] * b) >= 0.0 ? 1 : 0;
#pragma unroll
    for (int j = 5; j < 10; ++j) above += (B[j][0] * a - B[j][1] * b) >= 0.0 ? 1 : 0;
    return a > 0.0 ? above : (a < 0.0 ? below : (b < 0.0 ? 0 : 5));
}

// negate the normals that look away from the viewpoint
__global__ __launch_bounds__(FP_BLOCK) void k_fpfh_orient(const double *__restrict__ X, const double *__restrict__ Y,
                                                          const double *__restrict__ Z, float *__restrict__ nrm, long n, double vx,
                                                          double vy, double vz)
{
    const long stride = (long)gridDim.x * FP_BLOCK;
    for (long i = (long)blockIdx.x * FP_BLOCK + threadIdx.x; i < n; i += stride) {
        const float fx = nrm[3 * i], fy = nrm[3 * i + 1], fz = nrm[3 * i + 2];
        const double s = ((vx - X[i]) * (double)fx + (vy - Y[i]) * (double)fy) + (vz - Z[i]) * (double)fz;
        if (s < 0.0) { nrm[3 * i] = -fx; nrm[3 * i + 1] = -fy; nrm[3 * i + 2] = -fz; }
    }
}

// Pass 1.  Points lo .. lo + Q of the cloud, their ranked lists d2l / idxl (Q, k).  spfh: (n, FP_ROW) counts by point.
// st: [0] += non-void pairs, [1] += void pairs within the radius, [2] += points with m_i == 0.
__global__ __launch_bounds__(FP_BLOCK) void k_fpfh_spfh(const double *__restrict__ X, const double *__restrict__ Y,
                                                        const double *__restrict__ Z, const float *__restrict__ nrm,
                                                        const double *__restrict__ d2l, const int64_t *__restrict__ idxl, long n, long lo,
                                                        long Q, int k, double r2, int no_radius, uint16_t *__restrict__ spfh,
                                                        unsigned long long *__restrict__ st)
{
    const int lane = threadIdx.x & 63;
    const long nw = (long)gridDim.x * FP_WAVES;
    unsigned long long pairs = 0, voids = 0, empty = 0;            // (the same in every lane of the wave)
    for (long q = (long)blockIdx.x * FP_WAVES + (threadIdx.x >> 6); q < Q; q += nw) {
        const long i = lo + q;
        const double px = X[i], py = Y[i], pz = Z[i];
        const double pnx = (double)nrm[3 * i], pny = (double)nrm[3 * i + 1], pnz = (double)nrm[3 * i + 2];
        const bool p_ok = finite_f64(pnx) && finite_f64(pny) && finite_f64(pnz);
        unsigned cnt = 0, m = 0, inside = 0;
        for (int r0 = 1; r0 < k; r0 += 64) {
            const int r = r0 + lane;
            const bool have = r < k;
            const long jl = have ? (long)idxl[q * k + r] : -1;
            const bool there = jl >= 0 && jl < n;                   // (a rank that holds no point counts nowhere and is never read)
            const long j = there ? jl : i;
            const double d2 = have ? d2l[q * k + r] : 0.0;
            const bool in = there && (no_radius || d2 < r2);
            const double qnx = (double)nrm[3 * j], qny = (double)nrm[3 * j + 1], qnz = (double)nrm[3 * j + 2];
            double dx = X[j] - px, dy = Y[j] - py, dz = Z[j] - pz;
            const double f4 = sqrt(d2);
            const double a1 = ((pnx * dx + pny * dy) + pnz * dz) / f4;
            const double a2 = ((qnx * dx + qny * dy) + qnz * dz) / f4;
            const bool swap = fabs(a1) < fabs(a2);
            const double n1x = swap ? qnx : pnx, n1y = swap ? qny : pny, n1z = swap ? qnz : pnz;
            const double n2x = swap ? pnx : qnx, n2y = swap ? pny : qny, n2z = swap ? pnz : qnz;
            const double f3 = swap ? -a2 : a1;
            if (swap) { dx = -dx; dy = -dy; dz = -dz; }
            double vx = dy * n1z - dz * n1y, vy = dz * n1x - dx * n1z, vz = dx * n1y - dy * n1x;
            const double vn = sqrt((vx * vx + vy * vy) + vz * vz);
            vx = vx / vn; vy = vy / vn; vz = vz / vn;
            const double wx = n1y * vz - n1z * vy, wy = n1z * vx - n1x * vz, wz = n1x * vy - n1y * vx;
            const double f2 = (vx * n2x + vy * n2y) + vz * n2z;
            const double a = (wx * n2x + wy * n2y) + wz * n2z;
            const double b = (n1x * n2x + n1y * n2y) + n1z * n2z;
            const bool ok = in && d2 != 0.0 && vn != 0.0 && p_ok && finite_f64(qnx) && finite_f64(qny) && finite_f64(qnz);
            const int b1 = ok ? fp_sector(a, b) : -1, b2 = ok ? fp_bin11(f2) : -1, b3 = ok ? fp_bin11(f3) : -1;
#pragma unroll
            for (int t = 0; t < 11; ++t) {
                const unsigned c1 = (unsigned)__popcll((long long)__ballot(b1 == t));
                const unsigned c2 = (unsigned)__popcll((long long)__ballot(b2 == t));
                const unsigned c3 = (unsigned)__popcll((long long)__ballot(b3 == t));
                cnt += lane == t ? c1 : (lane == 11 + t ? c2 : (lane == 22 + t ? c3 : 0u));
            }
            m += (unsigned)__popcll((long long)__ballot(ok));
            inside += (unsigned)__popcll((long long)__ballot(in));
        }
        if (lane < FP_ROW) spfh[i * FP_ROW + lane] = (uint16_t)(lane == SICP_FPFH_BINS ? m : cnt);
        pairs += m; voids += inside - m; empty += m == 0 ? 1 : 0;
    }
    if (lane == 0) {
        if (pairs) atomicAdd(st, pairs);
        if (voids) atomicAdd(st + 1, voids);
        if (empty) atomicAdd(st + 2, empty);
    }
}

// Pass 2.  Lane b < 33 owns bin b.  out: (n, 33) by point.
__global__ __launch_bounds__(FP_BLOCK) void k_fpfh_final(const double *__restrict__ d2l, const int64_t *__restrict__ idxl, long n, long lo,
                                                         long Q, int k, double r2, int no_radius, const uint16_t *__restrict__ spfh,
                                                         float *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int bin = lane < SICP_FPFH_BINS ? lane : SICP_FPFH_BINS - 1;       // (the idle lanes shadow the last bin)
    const int g0 = (bin / 11) * 11;
    const long nw = (long)gridDim.x * FP_WAVES;
    for (long q = (long)blockIdx.x * FP_WAVES + (threadIdx.x >> 6); q < Q; q += nw) {
        const long i = lo + q;
        double W = 0.0;
        for (int r = 1; r < k; ++r) {
            const long jl = (long)idxl[q * k + r];
            const bool there = jl >= 0 && jl < n;
            const long j = there ? jl : i;
            const double d2 = d2l[q * k + r];
            const unsigned c = spfh[j * FP_ROW + bin], m = spfh[j * FP_ROW + SICP_FPFH_BINS];
            // a neighbour with a non-finite normal has m == 0; every term is >= +0.0, so leaving one out and adding +0.0 are the same
            const bool use = there && (no_radius || d2 < r2) && d2 != 0.0 && m != 0u;
            const double S = (100.0 * (double)c) / (double)(m ? m : 1u);
            W = W + (use ? S / d2 : 0.0);
        }
        double T = __shfl(W, g0);
#pragma unroll
        for (int t = 1; t < 11; ++t) T = T + __shfl(W, g0 + t);
        const unsigned ci = spfh[i * FP_ROW + bin], mi = spfh[i * FP_ROW + SICP_FPFH_BINS];
        const double Si = mi ? (100.0 * (double)ci) / (double)mi : 0.0;
        const double F = Si + (T > 0.0 ? (W * 100.0) / T : 0.0);
        if (lane < SICP_FPFH_BINS) out[i * SICP_FPFH_BINS + lane] = (float)F;
    }
}

}  // namespace
}  // namespace sicp

namespace {

enum { FP_PAIRS = 0, FP_VOID = 1, FP_EMPTY = 2 };              // counter words
static_assert(FP_EMPTY < CAND_WORDS, "the record's counters fit the ctx's counter words");

}  // namespace

SICP_EXPORT int sicp_fpfh_version(void) { return SICP_FPFH_VERSION; }

SICP_EXPORT int sicp_fpfh(sicp_ctx *c, int slot, const float *normals, int k, double radius, const double *viewpoint, float *fpfh_out,
                          uint16_t *spfh_counts_out, sicp_fpfh_stats *out)
{
    CHK(check_slot(c, slot, true));
    if (!normals) return fail(SICP_ERR_INVALID, "normals is null");
    if (!fpfh_out) return fail(SICP_ERR_INVALID, "fpfh_out is null");
    if (!out) return fail(SICP_ERR_INVALID, "out is null");
    Cloud &cl = c->cloud[slot];
    if (k < 2) return fail(SICP_ERR_INVALID, "k must be >= 2 (%d given)", k);
    if (k > SICP_FPFH_MAX_K) return fail(SICP_ERR_INVALID, "k must be <= %d (%d given)", SICP_FPFH_MAX_K, k);
    if (k > cl.n) return fail(SICP_ERR_INVALID, "k (%d) exceeds the number of points (%lld)", k, (long long)cl.n);
    if (std::isnan(radius) || !(radius > 0.0)) return fail(SICP_ERR_INVALID, "radius must be > 0 (+inf: none)");
    if (viewpoint && !(std::isfinite(viewpoint[0]) && std::isfinite(viewpoint[1]) && std::isfinite(viewpoint[2])))
        return fail(SICP_ERR_INVALID, "viewpoint must be finite");
    CHK(check_whole_cloud(c, slot, "sicp_fpfh", "a point's neighbours may live on another rank"));
    HIPCHK(hipSetDevice(c->device));
    return op_run(c, [&]() -> int {
        const long n = (long)cl.n;
        float *dst;
        CHK(c->fp_nrm.reserve((size_t)3 * n));
        CHK(c->fp_cnt.reserve((size_t)FP_ROW * n));
        CHK(stage_out(c, fpfh_out, (size_t)SICP_FPFH_BINS * n, c->fp_out, &dst));
        CHK(counters_clear(c));
        // the normals are always copied (no stage_in): k_fpfh_orient writes them
        HIPCHK(hipMemcpyAsync(c->fp_nrm.p, normals, (size_t)3 * n * sizeof(float), hipMemcpyDefault, c->stream));
        if (viewpoint) {
            hipLaunchKernelGGL(k_fpfh_orient, dim3(std::min(cdiv(n, FP_BLOCK), (unsigned)FP_MAX_BLOCKS)), dim3(FP_BLOCK), 0, c->stream,
                               cl.x(), cl.y(), cl.z(), c->fp_nrm.p, n, viewpoint[0], viewpoint[1], viewpoint[2]);
            HIPCHK(hipGetLastError());
        }
        const long chunk = knn_chunk(c->fpfh_chunk, k);
        CHK(knn_chunk_reserve(c, std::min(chunk, n), k));
        const bool no_radius = std::isinf(radius);
        const double r2 = radius * radius;
        for (int pass = 1; pass <= 2; ++pass)
            for (long lo = 0; lo < n; lo += chunk) {
                const long cnt = std::min(chunk, n - lo);
                CHK(rows_knn(c, slot, nullptr, lo, cnt, k));
                const unsigned g = std::min(cdiv(cnt, FP_WAVES), (unsigned)FP_MAX_BLOCKS);
                if (pass == 1)
                    hipLaunchKernelGGL(k_fpfh_spfh, dim3(g), dim3(FP_BLOCK), 0, c->stream, cl.x(), cl.y(), cl.z(), c->fp_nrm.p, c->k_d2.p,
                                       c->k_idx.p, n, lo, cnt, k, r2, no_radius ? 1 : 0, c->fp_cnt.p, c->cand_small.p);
                else
                    hipLaunchKernelGGL(k_fpfh_final, dim3(g), dim3(FP_BLOCK), 0, c->stream, c->k_d2.p, c->k_idx.p, n, lo, cnt, k, r2,
                                       no_radius ? 1 : 0, c->fp_cnt.p, dst);
                HIPCHK(hipGetLastError());
            }
        CHK(counters_fetch(c));
        CHK(stage_leave(c, fpfh_out, (size_t)SICP_FPFH_BINS * n, dst));
        if (spfh_counts_out)
            HIPCHK(hipMemcpyAsync(spfh_counts_out, c->fp_cnt.p, (size_t)FP_ROW * n * sizeof(uint16_t), hipMemcpyDefault, c->stream));
        CHK(sync(c));
        const unsigned long long *h = counters_host(c);
        out->n_points = (int64_t)n;
        out->n_pairs = (int64_t)h[FP_PAIRS];
        out->n_void_pairs = (int64_t)h[FP_VOID];
        out->n_empty = (int64_t)h[FP_EMPTY];
        return SICP_OK;
    });
}
