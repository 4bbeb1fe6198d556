// sicp_nangle.hip -- rejection by the angle between normals (include/simpleicp_hip_normals.h): the verdict
// kernels, the on-demand cache of the movable cloud's normals, the hooks the iteration roads call and the companion ABI's exports.
//
// Per iteration, behind the last launch that writes `flag` and before the first that reads it:
//   k_na_verdict   one lane per correspondence: the movable normal is there (the slot's columns, or the cache) -> contract (N),
//                  flag &= verdict; it is not -> (q, m) goes to the miss list (ballot + mbcnt, one atomic per wave);
//   the k-NN sweep (sicp_grid.hip) over the list: k_grid_knn_sweep, unchanged, in its "only these slots" form -- the list's
//                  length from device memory, the listed points' coordinates straight from the cloud's columns, covariances by
//                  list position; from 32 768 correspondences on k_grid_knn_sweep4_list first (four entries per wave), the
//                  one-per-wave kernel then does what it spills;
//   k_na_finish    one lane per list entry: eigen step (sicp_normals.h: the same device code as k_cov_normals), the normal goes
//                  into the cache, the verdict of the entry's correspondence into flag.
// The launches of 2 and 3 are sized for the worst case and leave at their count: no host round trip inside the chained loop.  The
// list's counters alternate between iterations (each k_na_finish clears the other pair), so nothing is reset in between.
#include "sicp_host.h"
#include "sicp_normals.h"
#include "../../include/simpleicp_hip_normals.h"

namespace sicp {

// counters (uint32): [0], [1] miss-list length by parity | [2], [3] correspondences dropped by parity | [4], [5] entries the
// four-per-wave sweep left to the one-per-wave kernel, by parity | [6] cache entries filled | [7] iterations whose miss list was
// empty | [8] parity of the last iteration that ran
constexpr int NA_MISS = 0, NA_DROP = 2, NA_SPILL = 4, NA_PER_RUN = 6, NA_FILLED = 6, NA_EMPTY = 7, NA_LAST = 8, NA_WORDS = 12;

struct NaArgs {
    const int64_t *m_idx;         // (Q) matched movable index, global
    const float *n1;              // (Q,3) fixed normals
    uint8_t *flag;                // (Q) in / out
    long Q;
    const float *col;             // movable normals by GLOBAL index (col_n points), or null: the cache below
    long col_n;
    const float *per_q;           // (Q,3) movable normals per correspondence (the operator's own column), or null
    float *cache;                 // (n,3) by local index
    uint32_t *have;               // one bit per local index: the cache holds this point's normal (which may be NaN)
    int64_t idx_base; long n;
    uint32_t *list_q, *list_m;    // the miss list: correspondence, local index of its matched point
    const double *cov;            // (list position, 6) covariances the sweep left
    unsigned *cnt;
    double cos_max;
    int par;
    int use_H;                    // H by value (else the loop state's)
    const IcpDev *st;             // nullable: the chained run's loop state (H, stop flag)
    Xf H;
};

// contract (N): every operation separately rounded (-ffp-contract=off)
__device__ __forceinline__ bool na_keep(const float *__restrict__ n1, float n2x, float n2y, float n2z, const double *R, double cos_max)
{
    const double ax = (double)n1[0], ay = (double)n1[1], az = (double)n1[2];
    const double bx = (double)n2x, by = (double)n2y, bz = (double)n2z;
    const double rx = (R[0] * bx + R[1] * by) + R[2] * bz;
    const double ry = (R[4] * bx + R[5] * by) + R[6] * bz;
    const double rz = (R[8] * bx + R[9] * by) + R[10] * bz;
    const double c = (ax * rx + ay * ry) + az * rz;
    return fabs(c) >= cos_max;                                   // (NaN fails)
}

__device__ __forceinline__ unsigned wave_rank(unsigned long long m)
{
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

__global__ __launch_bounds__(256) void k_na_verdict(const NaArgs A)
{
    if (A.st && A.st->stop) return;
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    const double *R = A.use_H ? A.H.m : A.st->H.m;
    bool miss = false, drop = false;
    uint32_t ml = 0;
    if (q < A.Q && A.flag[q]) {
        const int64_t m = A.m_idx[q];
        float n2[3] = {__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
        bool have = true;
        if (A.per_q) {
            n2[0] = A.per_q[3 * q]; n2[1] = A.per_q[3 * q + 1]; n2[2] = A.per_q[3 * q + 2];
        } else if (A.col) {
            if (m >= 0 && m < (int64_t)A.col_n) { n2[0] = A.col[3 * m]; n2[1] = A.col[3 * m + 1]; n2[2] = A.col[3 * m + 2]; }
        } else {
            const int64_t l = m - A.idx_base;
            if (l >= 0 && l < (int64_t)A.n) {
                ml = (uint32_t)l;
                have = (A.have[ml >> 5] >> (ml & 31u)) & 1u;
                if (have) { n2[0] = A.cache[3 * (long)ml]; n2[1] = A.cache[3 * (long)ml + 1]; n2[2] = A.cache[3 * (long)ml + 2]; }
            }
        }
        if (have) {
            if (!na_keep(A.n1 + 3 * q, n2[0], n2[1], n2[2], R, A.cos_max)) { A.flag[q] = 0; drop = true; }
        } else {
            miss = true;
        }
    }
    const unsigned long long mm = __ballot(miss);
    if (mm) {
        unsigned base = 0;
        const int first = __ffsll((long long)mm) - 1;
        if ((int)(threadIdx.x & 63) == first) base = atomicAdd(A.cnt + NA_MISS + A.par, (unsigned)__popcll((long long)mm));
        base = (unsigned)__builtin_amdgcn_readlane((int)base, first);
        if (miss) {
            const unsigned pos = base + wave_rank(mm);
            A.list_q[pos] = (uint32_t)q; A.list_m[pos] = ml;
        }
    }
    const unsigned long long dm = __ballot(drop);
    if (dm && (int)(threadIdx.x & 63) == __ffsll((long long)dm) - 1) atomicAdd(A.cnt + NA_DROP + A.par, (unsigned)__popcll((long long)dm));
}

__global__ __launch_bounds__(256) void k_na_finish(const NaArgs A)
{
    const bool stopped = A.st && A.st->stop;
    const unsigned count = A.cnt[NA_MISS + A.par];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        A.cnt[NA_MISS + (A.par ^ 1)] = 0;                        // (the next iteration's lists start empty)
        A.cnt[NA_SPILL + (A.par ^ 1)] = 0;
        if (!stopped) {
            A.cnt[NA_DROP + (A.par ^ 1)] = 0;
            A.cnt[NA_LAST] = (unsigned)A.par;
            if (count == 0) A.cnt[NA_EMPTY] += 1;
        }
    }
    if (stopped) return;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if ((long)(blockIdx.x * 256) >= (long)count) return;
    bool fresh = false, drop = false;
    if (p < (long)count) {
        const uint32_t ml = A.list_m[p], q = A.list_q[p];
        double c6[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) c6[i] = A.cov[6 * p + i];
        float nrm[3] = {__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")}, pl = __builtin_nanf("");
        if (c6[0] == c6[0]) normal_from_cov(c6, nrm, &pl);                   // (NaN: fewer than k points)
        // (two correspondences matched to the same point both get here: same bits, and one of them finds the bit clear)
        A.cache[3 * (long)ml] = nrm[0]; A.cache[3 * (long)ml + 1] = nrm[1]; A.cache[3 * (long)ml + 2] = nrm[2];
        const uint32_t bit = 1u << (ml & 31u);
        fresh = !(atomicOr(A.have + (ml >> 5), bit) & bit);
        const double *R = A.use_H ? A.H.m : A.st->H.m;
        if (!na_keep(A.n1 + 3 * (long)q, nrm[0], nrm[1], nrm[2], R, A.cos_max)) { A.flag[q] = 0; drop = true; }
    }
    const unsigned long long fm = __ballot(fresh);
    if (fm && (int)(threadIdx.x & 63) == __ffsll((long long)fm) - 1) atomicAdd(A.cnt + NA_FILLED, (unsigned)__popcll((long long)fm));
    const unsigned long long dm = __ballot(drop);
    if (dm && (int)(threadIdx.x & 63) == __ffsll((long long)dm) - 1) atomicAdd(A.cnt + NA_DROP + A.par, (unsigned)__popcll((long long)dm));
}

__global__ __launch_bounds__(256) void k_na_iota(uint32_t *__restrict__ v, long n)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) v[i] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void k_na_scatter3(float *__restrict__ dst, const int64_t *__restrict__ rows, const float *__restrict__ v, long m)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const int64_t r = rows[i];
    dst[3 * r] = v[3 * i]; dst[3 * r + 1] = v[3 * i + 1]; dst[3 * r + 2] = v[3 * i + 2];
}

}  // namespace sicp

namespace sicph {

namespace {

const char *const NA_WHO = "rejection by the angle between normals", *const NA_WHY = "the matched point may live on another rank";

// buffers of Q correspondences and the movable slot's cache, ready for an iteration's launches (before a run's first launch,
// before an operator call).  Emptied cache: an upload or transform of the slot, another k.
int na_prepare(sicp_ctx *c, int k, bool need_cache)
{
    NormalAngle &N = c->na;
    Cloud &cl = c->cloud[SICP_MOV];
    const long Q = c->Q;
    CHK(check_no_exchange(c, NA_WHO, NA_WHY));
    if (!N.cnt.p) {
        CHK(N.cnt.reserve(sicp::NA_WORDS));
        HIPCHK(hipMemsetAsync(N.cnt.p, 0, sicp::NA_WORDS * sizeof(unsigned), c->stream));
        N.counters_stale = false;
    }
    if (N.counters_stale) {                              // (sicp_icp_setup: the figures of sicp_normal_angle_info start again)
        HIPCHK(hipMemsetAsync(N.cnt.p, 0, sicp::NA_WORDS * sizeof(unsigned), c->stream));
        N.counters_stale = false;
    } else {
        // a run starts at parity 0 with both pairs clean, whatever launches the last one left behind its end
        HIPCHK(hipMemsetAsync(N.cnt.p, 0, sicp::NA_PER_RUN * sizeof(unsigned), c->stream));
    }
    N.par = 0;
    if (!need_cache) return SICP_OK;
    if (k < 2) return fail(SICP_ERR_INVALID, "neighbors must be >= 2");
    if (!grid_knn_sweep_handles(k)) return fail(SICP_ERR_INVALID, "normals on demand take at most 128 neighbors (%d asked for)", k);
    if (k > cl.n) return fail(SICP_ERR_INVALID, "neighbors (%d) exceeds the number of points (%lld)", k, (long long)cl.n);
    if (cl.n >= (1LL << 31)) return fail(SICP_ERR_INVALID, "normals on demand need a cloud the grid can bin");
    CHK(grid_build(c, SICP_MOV));
    const size_t words = (size_t)((cl.n + 31) / 32);
    if (!cl.nrm2_valid || cl.nrm2_k != k || cl.nrm2.cap < (size_t)3 * cl.n || cl.nrm2_have.cap < words) {
        CHK(cl.nrm2.reserve((size_t)3 * cl.n));
        CHK(cl.nrm2_have.reserve(words));
        HIPCHK(hipMemsetAsync(cl.nrm2_have.p, 0, words * sizeof(uint32_t), c->stream));
        cl.nrm2_valid = true; cl.nrm2_k = k;
    }
    if (N.list_q.cap < (size_t)Q) {
        CHK(N.list_q.reserve(Q)); CHK(N.list_m.reserve(Q)); CHK(N.cov.reserve((size_t)6 * Q));
        // `iota`: doubles as the four-per-wave sweep's spill list (large Q), else holds 0, 1, 2, ... -- the one-per-wave sweep's "only
        // these slots" form then walks every position of the miss list.  (A null slot list meaning "all positions" would need no
        // buffer, but would change k_grid_knn_sweep itself: the existing instantiations are used as they are.)
        CHK(N.iota.reserve(Q));
        N.iota_n = 0;
    }
    return SICP_OK;
}

// one iteration's launches on `flag`
int na_enqueue(sicp_ctx *c, double cos_max, int k, uint8_t *flag, const IcpDev *st, const Xf *H, const float *per_q)
{
    NormalAngle &N = c->na;
    Cloud &cl = c->cloud[SICP_MOV];
    const long Q = c->Q;
    sicp::NaArgs A = {};
    A.m_idx = c->m_idx.p; A.n1 = c->normals.p; A.flag = flag; A.Q = Q;
    A.col = cl.nv_n > 0 ? cl.nv.p : nullptr; A.col_n = cl.nv_n;
    A.per_q = per_q;
    A.cache = cl.nrm2.p; A.have = cl.nrm2_have.p; A.idx_base = cl.idx_base; A.n = cl.n;
    A.list_q = N.list_q.p; A.list_m = N.list_m.p; A.cov = N.cov.p; A.cnt = N.cnt.p;
    A.cos_max = cos_max; A.par = N.par;
    A.use_H = H ? 1 : 0; A.st = st;
    if (H) A.H = *H;
    hipLaunchKernelGGL(sicp::k_na_verdict, dim3(cdiv(Q, 256)), dim3(256), 0, c->stream, A);
    const bool cached = !per_q && !A.col;
    if (cached) {
        // many correspondences (a first iteration misses everywhere): four list entries per wave, as launch_grid_knn_sweep chooses
        const bool four = Q >= 32768 && k <= 32;
        // (iota_n: how many leading words of `iota` hold 0, 1, 2, ... -- a setup with more correspondences than that, or a spill
        // list written over them, and they are written again before the sweep walks them)
        if (!four && N.iota_n < Q) {
            hipLaunchKernelGGL(sicp::k_na_iota, dim3(cdiv(Q, 256)), dim3(256), 0, c->stream, N.iota.p, Q);
            N.iota_n = Q;
        }
        if (four) N.iota_n = 0;
        launch_grid_knn_sweep_list(c->stream, cl.x(), cl.y(), cl.z(), N.list_m.p, N.iota.p, N.cnt.p + sicp::NA_MISS + N.par, Q, k,
                                   cl.grid.g, cl.grid.avg_per_cell, cl.grid.cell_start.p, cl.grid.rec.p, cl.rmax, N.cov.p,
                                   four ? N.iota.p : nullptr, four ? N.cnt.p + sicp::NA_SPILL + N.par : nullptr);
    }
    // (normals that were all there: nothing is listed, one block keeps the counters' books)
    hipLaunchKernelGGL(sicp::k_na_finish, dim3(cached ? cdiv(Q, 256) : 1u), dim3(256), 0, c->stream, A);
    N.par ^= 1;
    HIPCHK(hipGetLastError());
    return SICP_OK;
}

}  // namespace

bool normal_angle_on(const sicp_ctx *c) { return c->na.cos_max > 0.0; }

int normal_angle_prepare(sicp_ctx *c)
{
    return na_prepare(c, c->na.k, c->cloud[SICP_MOV].nv_n == 0);
}

int normal_angle_enqueue(sicp_ctx *c, const IcpDev *st, const Xf *H)
{
    return na_enqueue(c, c->na.cos_max, c->na.k, c->flag.p, st, H, nullptr);
}

}  // namespace sicph

SICP_EXPORT int sicp_normals_version(void) { return SICP_NORMALS_VERSION; }

SICP_EXPORT int sicp_cloud_set_normals(sicp_ctx *c, int slot, const int64_t *rows, const float *normals, int64_t m, int64_t n_global)
{
    CHK(check_slot(c, slot, true));
    Cloud &cl = c->cloud[slot];
    if (!normals) { cl.nv_n = 0; return SICP_OK; }
    if (n_global < cl.idx_base + cl.n) return fail(SICP_ERR_INVALID, "n_global is smaller than the cloud");
    if (m < 0 || (!rows && m != n_global)) return fail(SICP_ERR_INVALID, "dense normal columns need n_global rows");
    HIPCHK(hipSetDevice(c->device));
    CHK(cl.nv.reserve((size_t)3 * n_global));
    if (!rows) {
        HIPCHK(hipMemcpyAsync(cl.nv.p, normals, (size_t)3 * m * sizeof(float), hipMemcpyDefault, c->stream));
        cl.nv_n = n_global;
        return sync(c);
    }
    CHK(check_rows(rows, m, n_global, "normal rows"));
    DevBuf<int64_t> d_rows; DevBuf<float> d_vals;
    int rc = d_rows.reserve((size_t)std::max<int64_t>(m, 1));
    if (rc == SICP_OK) rc = d_vals.reserve((size_t)3 * std::max<int64_t>(m, 1));
    auto body = [&]() -> int {
        HIPCHK(hipMemcpyAsync(d_rows.p, rows, (size_t)m * sizeof(int64_t), hipMemcpyDefault, c->stream));
        HIPCHK(hipMemcpyAsync(d_vals.p, normals, (size_t)3 * m * sizeof(float), hipMemcpyDefault, c->stream));
        launch_fill_f32(c->stream, cl.nv.p, 3 * n_global, std::numeric_limits<float>::quiet_NaN());
        if (m > 0) hipLaunchKernelGGL(sicp::k_na_scatter3, dim3(cdiv(m, 256)), dim3(256), 0, c->stream, cl.nv.p, d_rows.p, d_vals.p, (long)m);
        HIPCHK(hipGetLastError());
        return sync(c);
    };
    if (rc == SICP_OK) rc = body();
    (void)hipStreamSynchronize(c->stream);                // (always, not op_run: the local buffers are released next)
    d_rows.release(); d_vals.release();
    if (rc == SICP_OK) cl.nv_n = n_global;
    return rc;
}

SICP_EXPORT int sicp_normal_angle_set(sicp_ctx *c, double cos_max, int k)
{
    if (!c) return fail(SICP_ERR_INVALID, "null ctx");
    if (std::isnan(cos_max) || cos_max <= 0.0) { c->na.cos_max = 0.0; return SICP_OK; }
    if (cos_max > 1.0) return fail(SICP_ERR_INVALID, "cos_max must be <= 1");
    if (k < 2) return fail(SICP_ERR_INVALID, "neighbors must be >= 2");
    CHK(check_no_exchange(c, NA_WHO, NA_WHY));
    c->na.cos_max = cos_max; c->na.k = k;
    return SICP_OK;
}

SICP_EXPORT int sicp_corr_reject_normal_angle(sicp_ctx *c, double cos_max, int k, const double *H, const float *pc2_normals,
                                              int64_t *n_alive_out)
{
    CHK(check_corr(c));
    if (std::isnan(cos_max) || cos_max <= 0.0 || cos_max > 1.0) return fail(SICP_ERR_INVALID, "cos_max must lie in (0, 1]");
    CHK(check_slot(c, SICP_MOV, true));
    HIPCHK(hipSetDevice(c->device));
    const long Q = c->Q;
    Xf X = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}};
    if (H) H16_to_Xf(H, &X);
    const float *per_q = nullptr;
    if (pc2_normals) {
        CHK(c->na.per_q.reserve((size_t)3 * Q));
        HIPCHK(hipMemcpyAsync(c->na.per_q.p, pc2_normals, (size_t)3 * Q * sizeof(float), hipMemcpyDefault, c->stream));
        per_q = c->na.per_q.p;
    }
    CHK(na_prepare(c, k, !per_q && c->cloud[SICP_MOV].nv_n == 0));
    CHK(na_enqueue(c, cos_max, k, c->keep.p, nullptr, &X, per_q));
    double *h_st;
    CHK(corr_alive_stats(c, nullptr, &h_st));
    if (n_alive_out) *n_alive_out = (int64_t)h_st[4];
    return SICP_OK;
}

SICP_EXPORT int sicp_normal_angle_info(sicp_ctx *c, int64_t out4[4])
{
    if (!c || !out4) return fail(SICP_ERR_INVALID, "null argument");
    out4[0] = out4[1] = out4[2] = out4[3] = 0;
    const Cloud &cl = c->cloud[SICP_MOV];
    if (cl.nrm2_valid) out4[2] = (int64_t)(12 * cl.n + 4 * ((cl.n + 31) / 32));
    if (!c->na.cnt.p || c->na.counters_stale) return SICP_OK;
    HIPCHK(hipSetDevice(c->device));
    unsigned h[sicp::NA_WORDS];
    CHK(sync(c));
    HIPCHK(hipMemcpy(h, c->na.cnt.p, sizeof h, hipMemcpyDeviceToHost));
    out4[0] = h[sicp::NA_FILLED];
    out4[1] = h[sicp::NA_DROP + (h[sicp::NA_LAST] & 1u)];
    out4[3] = h[sicp::NA_EMPTY];
    return SICP_OK;
}

SICP_EXPORT int sicp_normal_cache_read(sicp_ctx *c, float *normals_out, uint8_t *have_out)
{
    if (!normals_out || !have_out) return fail(SICP_ERR_INVALID, "null argument");
    CHK(check_slot(c, SICP_MOV, true));
    const Cloud &cl = c->cloud[SICP_MOV];
    const long n = cl.n;
    std::vector<uint32_t> bits((size_t)((n + 31) / 32), 0u);
    std::vector<float> nv((size_t)3 * n);
    if (cl.nrm2_valid) {
        HIPCHK(hipSetDevice(c->device));
        CHK(sync(c));
        HIPCHK(hipMemcpy(bits.data(), cl.nrm2_have.p, bits.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(nv.data(), cl.nrm2.p, nv.size() * sizeof(float), hipMemcpyDeviceToHost));
    }
    for (long i = 0; i < n; ++i) {
        const bool have = (bits[(size_t)(i >> 5)] >> (i & 31)) & 1u;
        have_out[i] = have ? 1 : 0;
        for (int a = 0; a < 3; ++a) normals_out[3 * i + a] = have ? nv[(size_t)3 * i + a] : std::numeric_limits<float>::quiet_NaN();
    }
    return SICP_OK;
}
