// sicp_device.hip -- clouds that already live in device memory (include/simpleicp_hip_device.h): the strided ingest, the selection on
// the device and the strided egress.  Nothing coordinate-sized crosses the host link on this road: the clouds are read where the caller
// holds them (k_ingest), the overlap verdicts are compacted into the kept rows on the device (k_mask_count, k_scan_counts,
// k_mask_compact), only the Q picked positions are computed on the host (numpy's linspace, bit for bit) and the transformed movable
// cloud is written straight into the caller's buffer (k_egress).
#include "sicp_host.h"
#include "sicp_lanes.h"
#include "sicp_grid_dev.h"
#include "../../include/simpleicp_hip_device.h"

namespace sicp {
namespace {

constexpr int DV_BLOCK = 256;
constexpr int INGEST_TILE = 2 * DV_BLOCK;    // points per block and step of k_ingest (two per lane)
constexpr int SEL_TILE = 4 * DV_BLOCK;       // mask bytes per block of the compaction (four per lane)

// k_ingest's grid: blocks at most, grid-stride loops beyond.  Measured at 10 M points, float64 / float32: 1 024 blocks 103 / 78 us,
// 2 048 112 / 95, 4 096 161 / 155 -- the seven same-address atomics per block cost more than the extra blocks give
// (profiles/tensors/ingest_grid_ab.txt)
#ifndef SICP_INGEST_BLOCKS
#define SICP_INGEST_BLOCKS 1024
#endif

// The strided (n, 3) view -> the slot's padded columns, widened exactly, and in the same pass what k_cloud_stats measures (min / max keys
// per axis, the largest squared norm with the same fma order, a NaN / inf sticks): min / max reductions, exact in any order.  CONTIG
// (row_stride 3, col_stride 1): a step's 3 x 512 elements are read as contiguous words through LDS, so every load instruction of a wave
// covers one contiguous range; otherwise each lane reads its points' three elements where they lie.
template <class T, bool CONTIG>
__global__ __launch_bounds__(DV_BLOCK) void k_ingest(const T *__restrict__ base, long n, long npad, long rs, long cs,
                                                     double *__restrict__ x, double *__restrict__ y, double *__restrict__ z,
                                                     unsigned long long *__restrict__ out)
{
    __shared__ T st[CONTIG ? 3 * INGEST_TILE : 1];
    __shared__ double red[4][8];
    double lo[3] = {__builtin_inf(), __builtin_inf(), __builtin_inf()};
    double nh[3] = {__builtin_inf(), __builtin_inf(), __builtin_inf()};      // minus the maxima
    double m = 0.0;
    bool bad = false;
    const long ntiles = npad / INGEST_TILE;                                    // (npad: a multiple of TILE_PTS)
    // CONTIG: tile t's 6 words per lane; the next tile's are loaded before this one is staged, so loads stay in flight while
    // the block waits at its barriers and stores the columns
    T r[CONTIG ? 6 : 1];
    auto load_tile = [&](long t) {
        const long e0 = 3 * t * INGEST_TILE, eend = 3 * n;
#pragma unroll
        for (int k = 0; k < 6; ++k) { const long e = e0 + threadIdx.x + DV_BLOCK * k; r[k] = e < eend ? base[e] : T(0); }
    };
    if constexpr (CONTIG) {
        if ((long)blockIdx.x < ntiles) load_tile(blockIdx.x);
    }
    for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long p0 = t * INGEST_TILE;
        double v[2][3];
        if constexpr (CONTIG) {
            T cur[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) cur[k] = r[k];
            if (t + gridDim.x < ntiles) load_tile(t + gridDim.x);
            __syncthreads();                                                   // (the last step's readers are through with st)
#pragma unroll
            for (int k = 0; k < 6; ++k) st[threadIdx.x + DV_BLOCK * k] = cur[k];
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int j = 3 * (DV_BLOCK * u + (int)threadIdx.x);
                v[u][0] = (double)st[j]; v[u][1] = (double)st[j + 1]; v[u][2] = (double)st[j + 2];
            }
        } else {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const long i = p0 + DV_BLOCK * u + threadIdx.x;
                const T *p = base + (i < n ? i : 0) * rs;
                v[u][0] = (double)p[0]; v[u][1] = (double)p[cs]; v[u][2] = (double)p[2 * cs];
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const long i = p0 + DV_BLOCK * u + threadIdx.x;
            if (i < n) {
                x[i] = v[u][0]; y[i] = v[u][1]; z[i] = v[u][2];
#pragma unroll
                for (int a = 0; a < 3; ++a) { lo[a] = fmin(lo[a], v[u][a]); nh[a] = fmin(nh[a], -v[u][a]); }
                const double nn = fma(v[u][2], v[u][2], fma(v[u][1], v[u][1], v[u][0] * v[u][0]));
                bad = bad || !(nn < __builtin_inf());
                m = fmax(m, nn);
            } else {
                x[i] = SICP_PAD_COORD; y[i] = SICP_PAD_COORD; z[i] = SICP_PAD_COORD;
            }
        }
    }
    // the block's fold and its 7 atomics: k_cloud_stats' own
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = wmin_d(lo[a]); nh[a] = wmin_d(nh[a]); }
    m = -wmin_d(-m);
    const bool anybad = __ballot(bad) != 0ull;
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { red[wid][a] = lo[a]; red[wid][3 + a] = nh[a]; }
        red[wid][6] = m; red[wid][7] = anybad ? 1.0 : 0.0;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        const int a = threadIdx.x;
        if (a < 6) {
            const double w = fmin(fmin(red[0][a], red[1][a]), fmin(red[2][a], red[3][a]));
            if (a < 3) atomicMin(out + a, okey(w)); else atomicMax(out + a, okey(-w));
        } else {
            double w = fmax(fmax(red[0][6], red[1][6]), fmax(red[2][6], red[3][6]));
            if (red[0][7] + red[1][7] + red[2][7] + red[3][7] > 0.0) w = __builtin_nan("");
            atomicMax(out + 6, (unsigned long long)__double_as_longlong(w));
        }
    }
}

// The slot's points under H (contract (T)) into a strided (n, 3) view of T, one 256-point tile per block.  CONTIG: the tile's 768
// values are staged in LDS and leave as contiguous words.
template <class T, bool CONTIG>
__global__ __launch_bounds__(DV_BLOCK) void k_egress(const double *__restrict__ x, const double *__restrict__ y,
                                                     const double *__restrict__ z, long n, Xf H, T *__restrict__ out, long rs, long cs)
{
    __shared__ T st[CONTIG ? 3 * DV_BLOCK : 1];
    const long p0 = (long)blockIdx.x * DV_BLOCK, i = p0 + threadIdx.x;
    double X = 0.0, Y = 0.0, Z = 0.0;
    if (i < n) xf(H, x[i], y[i], z[i], X, Y, Z);          // contract (T): sicp_grid_dev.h's, k_transform's operations
    if constexpr (CONTIG) {
        st[3 * threadIdx.x] = (T)X; st[3 * threadIdx.x + 1] = (T)Y; st[3 * threadIdx.x + 2] = (T)Z;
        __syncthreads();
        const long e0 = 3 * p0, eend = 3 * n;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const long e = e0 + threadIdx.x + DV_BLOCK * k;
            if (e < eend) out[e] = st[threadIdx.x + DV_BLOCK * k];
        }
    } else if (i < n) {
        T *o = out + i * rs;
        o[0] = (T)X; o[cs] = (T)Y; o[2 * cs] = (T)Z;
    }
}

// a lane's four mask bytes [b, b + 4) (zero past n) as flags
__device__ __forceinline__ unsigned mask_flags(const uint8_t *__restrict__ mask, long b, long n)
{
    unsigned f = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) f |= (b + k < n && mask[b + k] != 0) ? (1u << k) : 0u;
    return f;
}

// exclusive prefix of v over the block's 256 lanes (wave scans + the four wave totals through LDS); *total: the block's sum
__device__ __forceinline__ unsigned block_excl_scan(unsigned v, unsigned *total)
{
    __shared__ unsigned wtot[4];
    const unsigned incl = wscan_u32(v);
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 63) wtot[wid] = incl;
    __syncthreads();
    unsigned before = 0;
    for (int w = 0; w < wid; ++w) before += wtot[w];
    *total = wtot[0] + wtot[1] + wtot[2] + wtot[3];
    return before + incl - v;
}

// kept rows per block of SEL_TILE mask bytes
__global__ __launch_bounds__(DV_BLOCK) void k_mask_count(const uint8_t *__restrict__ mask, long n, uint32_t *__restrict__ cnt)
{
    const unsigned c = (unsigned)__builtin_popcount(mask_flags(mask, (long)blockIdx.x * SEL_TILE + 4L * threadIdx.x, n));
    unsigned total;
    (void)block_excl_scan(c, &total);
    if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}

// one block of 1024 lanes: exclusive scan of nb block counts into off, the sum into *total
__global__ __launch_bounds__(1024) void k_scan_counts(const uint32_t *__restrict__ cnt, long nb, uint32_t *__restrict__ off,
                                                      uint32_t *__restrict__ total)
{
    __shared__ unsigned wtot[16];
    __shared__ unsigned carry_s;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (long c0 = 0; c0 < nb; c0 += 1024) {
        const long i = c0 + threadIdx.x;
        const unsigned v = i < nb ? cnt[i] : 0u;
        const unsigned incl = wscan_u32(v);
        if (lane == 63) wtot[wid] = incl;
        __syncthreads();
        unsigned before = carry_s, chunk = 0;
        for (int w = 0; w < 16; ++w) { if (w < wid) before += wtot[w]; chunk += wtot[w]; }
        if (i < nb) off[i] = before + incl - v;
        __syncthreads();                                                  // (everyone has read carry_s and wtot)
        if (threadIdx.x == 0) carry_s += chunk;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry_s;
}

// the kept rows in index order: block b writes its rows from off[b] on
__global__ __launch_bounds__(DV_BLOCK) void k_mask_compact(const uint8_t *__restrict__ mask, long n, const uint32_t *__restrict__ off,
                                                           int64_t *__restrict__ kept)
{
    const long b = (long)blockIdx.x * SEL_TILE + 4L * threadIdx.x;
    const unsigned f = mask_flags(mask, b, n);
    unsigned total;
    long o = (long)off[blockIdx.x] + block_excl_scan((unsigned)__builtin_popcount(f), &total);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (f & (1u << k)) kept[o++] = b + k;
}

// sel[j] = kept[pos[j]] (kept null: every row is kept, sel[j] = pos[j])
__global__ __launch_bounds__(DV_BLOCK) void k_take(const int64_t *__restrict__ kept, const int64_t *__restrict__ pos, long q,
                                                   int64_t *__restrict__ sel)
{
    const long j = (long)blockIdx.x * DV_BLOCK + threadIdx.x;
    if (j < q) sel[j] = kept ? kept[pos[j]] : pos[j];
}

template <class T>
void launch_ingest(hipStream_t s, const T *base, long n, long npad, long rs, long cs, double *x, double *y, double *z,
                   unsigned long long *out7)
{
    long g = npad / INGEST_TILE;
    if (g > SICP_INGEST_BLOCKS) g = SICP_INGEST_BLOCKS;
    if (rs == 3 && cs == 1) hipLaunchKernelGGL((k_ingest<T, true>), dim3((unsigned)g), dim3(DV_BLOCK), 0, s, base, n, npad, rs, cs, x, y, z, out7);
    else hipLaunchKernelGGL((k_ingest<T, false>), dim3((unsigned)g), dim3(DV_BLOCK), 0, s, base, n, npad, rs, cs, x, y, z, out7);
}

template <class T>
void launch_egress(hipStream_t s, const double *x, const double *y, const double *z, long n, const Xf &H, T *out, long rs, long cs)
{
    if (rs == 3 && cs == 1) hipLaunchKernelGGL((k_egress<T, true>), dim3(cdiv(n, DV_BLOCK)), dim3(DV_BLOCK), 0, s, x, y, z, n, H, out, rs, cs);
    else hipLaunchKernelGGL((k_egress<T, false>), dim3(cdiv(n, DV_BLOCK)), dim3(DV_BLOCK), 0, s, x, y, z, n, H, out, rs, cs);
}

}  // namespace
}  // namespace sicp

namespace {

int check_strides(int dtype, int64_t rs, int64_t cs)
{
    if (dtype != SICP_DT_F32 && dtype != SICP_DT_F64) return fail(SICP_ERR_INVALID, "dtype must be SICP_DT_F32 or SICP_DT_F64");
    if (rs < 0 || cs < 0) return fail(SICP_ERR_INVALID, "strides must be >= 0");
    return SICP_OK;
}

}  // namespace

SICP_EXPORT int sicp_device_version(void) { return SICP_DEVICE_VERSION; }

SICP_EXPORT int sicp_cloud_upload_strided(sicp_ctx *c, int slot, const void *base, int dtype, int64_t n, int64_t row_stride,
                                          int64_t col_stride, int64_t index_base)
{
    if (!c) return fail(SICP_ERR_INVALID, "null ctx");
    if (!base) return fail(SICP_ERR_INVALID, "base is null");
    CHK(check_strides(dtype, row_stride, col_stride));
    CHK(check_slot(c, slot, false));
    HIPCHK(hipSetDevice(c->device));
    CHK(check_device_ptr(c, base, "base"));
    CHK(upload_begin(c, slot, n, index_base));
    Cloud &cl = c->cloud[slot];
    unsigned long long *d_st = (unsigned long long *)(c->small.p + 40);       // (cloud_stats' own scratch words)
    const unsigned long long h_init[7] = {~0ull, ~0ull, ~0ull, 0ull, 0ull, 0ull, 0ull};
    HIPCHK(hipMemcpyAsync(d_st, h_init, sizeof h_init, hipMemcpyHostToDevice, c->stream));
    if (dtype == SICP_DT_F64) launch_ingest(c->stream, (const double *)base, n, cl.npad, row_stride, col_stride, cl.x(), cl.y(), cl.z(), d_st);
    else launch_ingest(c->stream, (const float *)base, n, cl.npad, row_stride, col_stride, cl.x(), cl.y(), cl.z(), d_st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->h_small + 40, d_st, 7 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    CHK(sync(c));
    unsigned long long hk[7]; std::memcpy(hk, c->h_small + 40, sizeof hk);
    if (slot == SICP_MOV) { c->have_prev_match = false; c->slot_cnt = -1; }
    return cloud_stats_take(c, slot, hk);
}

SICP_EXPORT int sicp_select_positions(int64_t m, int64_t Q, int64_t *pos_out, int64_t *count_out)
{
    if (!pos_out || !count_out) return fail(SICP_ERR_INVALID, "null argument");
    if (m < 0 || Q <= 0) return fail(SICP_ERR_INVALID, "m must be >= 0 and Q > 0");
    if (m <= Q) {
        for (int64_t j = 0; j < m; ++j) pos_out[j] = j;
        *count_out = m;
        return SICP_OK;
    }
    // numpy.linspace(0, m - 1, Q): step = delta / div, y = arange(Q) * step, y[-1] = stop; np.round = half to even (nearbyint
    // in the default rounding mode).  m > Q >= 1, so step > 1 and the positions are strictly increasing (np.unique keeps them all).
    const double delta = (double)(m - 1);
    if (Q == 1) { pos_out[0] = 0; *count_out = 1; return SICP_OK; }
    const double step = delta / (double)(Q - 1);
    for (int64_t j = 0; j < Q - 1; ++j) pos_out[j] = (int64_t)std::nearbyint((double)j * step);
    pos_out[Q - 1] = m - 1;
    *count_out = Q;
    return SICP_OK;
}

SICP_EXPORT int sicp_select_n_device(sicp_ctx *c, const uint8_t *mask, int64_t n, int64_t Q, int64_t *sel_out, int64_t *q_out)
{
    if (!c) return fail(SICP_ERR_INVALID, "null ctx");
    if (!sel_out || !q_out) return fail(SICP_ERR_INVALID, "null argument");
    if (n <= 0 || n >= (int64_t)0xffffffffLL) return fail(SICP_ERR_INVALID, "n must be in [1, 2^32 - 2]");
    if (Q <= 0) return fail(SICP_ERR_INVALID, "Q must be > 0");
    HIPCHK(hipSetDevice(c->device));
    CHK(check_device_ptr(c, sel_out, "sel_out"));
    if (mask) CHK(check_device_ptr(c, mask, "mask"));
    int64_t m = n;
    // the kept rows live for this call only: stream-ordered memory from the device's pool, given back on the ctx's stream behind
    // k_take -- a (pooled) context holds no m-sized buffer between runs, and no hipFree synchronises the device
    struct StreamBuf {
        int64_t *p = nullptr;
        hipStream_t s = nullptr;
        ~StreamBuf() { if (p) (void)hipFreeAsync(p, s); }
    } kept{nullptr, c->stream};
    if (mask) {
        const long nb = (long)cdiv(n, SEL_TILE);
        CHK(c->sel_blk.reserve((size_t)2 * nb + 1));
        uint32_t *cnt = c->sel_blk.p, *off = cnt + nb, *tot = off + nb;
        hipLaunchKernelGGL(k_mask_count, dim3((unsigned)nb), dim3(DV_BLOCK), 0, c->stream, mask, (long)n, cnt);
        hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, c->stream, cnt, nb, off, tot);
        HIPCHK(hipGetLastError());
        uint32_t m32 = 0;
        HIPCHK(hipMemcpyAsync(&m32, tot, sizeof m32, hipMemcpyDeviceToHost, c->stream));
        CHK(sync(c));
        m = m32;
        if (m > 0) {
            HIPCHK(hipMallocAsync((void **)&kept.p, (size_t)m * sizeof(int64_t), c->stream));
            hipLaunchKernelGGL(k_mask_compact, dim3((unsigned)nb), dim3(DV_BLOCK), 0, c->stream, mask, (long)n, off, kept.p);
            HIPCHK(hipGetLastError());
        }
    }
    *q_out = 0;
    if (m == 0) return SICP_OK;
    const int64_t q = std::min<int64_t>(m, Q);
    std::vector<int64_t> pos((size_t)q);
    int64_t cnt_pos = 0;
    CHK(sicp_select_positions(m, Q, pos.data(), &cnt_pos));
    CHK(c->sel_pos.reserve((size_t)q));
    HIPCHK(hipMemcpyAsync(c->sel_pos.p, pos.data(), (size_t)q * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_take, dim3(cdiv(q, DV_BLOCK)), dim3(DV_BLOCK), 0, c->stream, kept.p, c->sel_pos.p, (long)q, sel_out);
    HIPCHK(hipGetLastError());
    if (kept.p) { HIPCHK(hipFreeAsync(kept.p, c->stream)); kept.p = nullptr; }
    CHK(sync(c));
    *q_out = q;
    return SICP_OK;
}

SICP_EXPORT int sicp_cloud_write_strided(sicp_ctx *c, int slot, const double H[16], void *out, int dtype, int64_t row_stride,
                                         int64_t col_stride)
{
    CHK(check_slot(c, slot, true));
    if (!H || !out) return fail(SICP_ERR_INVALID, "null argument");
    CHK(check_strides(dtype, row_stride, col_stride));
    HIPCHK(hipSetDevice(c->device));
    CHK(check_device_ptr(c, out, "out"));
    Xf X; H16_to_Xf(H, &X);
    Cloud &cl = c->cloud[slot];
    if (dtype == SICP_DT_F64) launch_egress(c->stream, cl.x(), cl.y(), cl.z(), cl.n, X, (double *)out, row_stride, col_stride);
    else launch_egress(c->stream, cl.x(), cl.y(), cl.z(), cl.n, X, (float *)out, row_stride, col_stride);
    HIPCHK(hipGetLastError());
    return sync(c);
}
