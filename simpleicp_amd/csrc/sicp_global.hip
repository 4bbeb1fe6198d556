// sicp_global.hip -- descriptor matching and RANSAC poses (include/simpleicp_hip_global.h; contracts (M) and (R)).
//
// Matching (k_match): one query row per lane, held in registers; a tile of target rows in LDS, every lane reading the same row at a
// time (broadcast reads).  The grid's second dimension splits the target into chunks so that a few thousand queries still fill the
// machine; a chunk's winner joins the query's 64-bit key (bits(d2) << 32) | j through an integer atomicMin -- for d2 >= +0 the bit
// pattern orders like the value, so the key's order IS the contract's (d2, j).  The row width is a template parameter (4, 16, 36,
// 64): the columns past dim hold 0 on both sides and add +0.0 to a sum that is >= +0, which changes no bit.
// RANSAC (k_ransac): one wave per hypothesis, every lane forming the same pose, then the lanes striding over the m rows; counts by
// ballot and popcount; the row's residual, the pose's store and the kernel that picks the lowest index among the best
// (k_pose_best) are sicp_pose_dev.h's.  Integer atomics only.
#include "sicp_pose_dev.h"
#include "../../include/simpleicp_hip_global.h"

namespace sicp {
namespace {

constexpr int MT_BLOCK = 256;                      // queries per workgroup
constexpr int MT_TILE = 128;                       // target rows in LDS at a time (64 columns: 32 KiB)
constexpr int MT_MAX_QBLOCKS = 8192, MT_MAX_CHUNKS = 1024;   // grid limits: the blocks stride from there on
constexpr int MT_FILL = 2048;                      // workgroups the chunking aims at
constexpr unsigned long long MT_NONE = ~0ull;      // a key no row has joined
constexpr int RS_BLOCK = 256, RS_WAVES = RS_BLOCK / 64;
constexpr int RS_MAX_BLOCKS = 16384;

template <int DP>
__global__ __launch_bounds__(MT_BLOCK) void k_match(const float *__restrict__ query, const float *__restrict__ target,
                                                    unsigned long long *__restrict__ key, long nq, long nt, int dim, long chunk,
                                                    long nchunks)
{
    __shared__ __attribute__((aligned(16))) float tile[MT_TILE * DP];
    const long nqb = (nq + MT_BLOCK - 1) / MT_BLOCK;
    for (long qb = blockIdx.x; qb < nqb; qb += gridDim.x) {
        const long i = qb * MT_BLOCK + threadIdx.x;
        float q[DP];
#pragma unroll
        for (int b = 0; b < DP; ++b) q[b] = (i < nq && b < dim) ? query[i * dim + b] : 0.0f;
        for (long ch = blockIdx.y; ch < nchunks; ch += gridDim.y) {
            const long lo = ch * chunk, hi = lo + chunk < nt ? lo + chunk : nt;
            float best = __builtin_inff();
            long bj = -1;
            for (long t0 = lo; t0 < hi; t0 += MT_TILE) {
                const int rows = hi - t0 < MT_TILE ? (int)(hi - t0) : MT_TILE;
                __syncthreads();                                   // (the last tile has been read by everyone)
                for (int e = threadIdx.x; e < rows * DP; e += MT_BLOCK) {
                    const int r = e / DP, b = e - r * DP;
                    tile[e] = b < dim ? target[(t0 + r) * dim + b] : 0.0f;
                }
                __syncthreads();
#pragma unroll 2
                for (int r = 0; r < rows; ++r) {
                    const float *g = tile + r * DP;
                    const float t = q[0] - g[0];
                    float d2 = t * t;
#pragma unroll
                    for (int b = 1; b < DP; ++b) {
                        const float u = q[b] - g[b];
                        d2 = d2 + u * u;
                    }
                    if (d2 < best) { best = d2; bj = t0 + r; }     // (ascending j: a tie keeps the lower index; NaN and +inf never win)
                }
            }
            if (i < nq && bj >= 0) atomicMin(key + i, ((unsigned long long)__float_as_uint(best) << 32) | (unsigned long long)bj);
        }
    }
}

// keys -> idx_out / d2_out (nullable); st[0] += queries no row has joined
__global__ __launch_bounds__(MT_BLOCK) void k_match_finish(const unsigned long long *__restrict__ key, long nq, int32_t *__restrict__ idx,
                                                           float *__restrict__ d2, unsigned long long *__restrict__ st)
{
    const long stride = (long)gridDim.x * MT_BLOCK;
    unsigned long long none = 0;
    for (long base = (long)blockIdx.x * MT_BLOCK; base < nq; base += stride) {
        const long i = base + threadIdx.x;
        const unsigned long long k = i < nq ? key[i] : 0ull;
        const bool un = k == MT_NONE;
        if (i < nq) {
            idx[i] = un ? -1 : (int32_t)(k & 0xffffffffull);
            if (d2) d2[i] = un ? __builtin_inff() : __uint_as_float((unsigned)(k >> 32));
        }
        none += (unsigned long long)__popcll((long long)__ballot(un));
    }
    if ((threadIdx.x & 63) == 0 && none) atomicAdd(st, none);
}

struct V3 { double x, y, z; };
__device__ __forceinline__ V3 rs_load(const double *__restrict__ a, long i) { return V3{a[3 * i], a[3 * i + 1], a[3 * i + 2]}; }
__device__ __forceinline__ V3 rs_sub(const V3 &a, const V3 &b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double rs_dot(const V3 &a, const V3 &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 rs_div(const V3 &a, double s) { return V3{a.x / s, a.y / s, a.z / s}; }
__device__ __forceinline__ V3 rs_cross(const V3 &a, const V3 &b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double rs_len2(const V3 &a, const V3 &b) { const V3 d = rs_sub(a, b); return rs_dot(d, d); }
// one pair of the edge check: does it prune?  (a NaN compares false: it prunes nothing)
__device__ __forceinline__ bool rs_prunes(double ls2, double lt2, double r2) { return ls2 < r2 * lt2 || lt2 < r2 * ls2; }

// the frame and the centroid of a triangle (contract (R), step 3)
__device__ __forceinline__ void rs_frame(const V3 &a0, const V3 &a1, const V3 &a2, V3 &e1, V3 &e2, V3 &e3, V3 &c)
{
    const V3 u = rs_sub(a1, a0);
    e1 = rs_div(u, sqrt(rs_dot(u, u)));
    const V3 v = rs_sub(a2, a0);
    const double s = rs_dot(e1, v);
    const V3 w = V3{v.x - s * e1.x, v.y - s * e1.y, v.z - s * e1.z};
    e2 = rs_div(w, sqrt(rs_dot(w, w)));
    e3 = rs_cross(e1, e2);
    c = V3{((a0.x + a1.x) + a2.x) / 3.0, ((a0.y + a1.y) + a2.y) / 3.0, ((a0.z + a1.z) + a2.z) / 3.0};
}

// One wave per hypothesis.  poses (nullable): (h, 12); inl: (h).
// st: [POSE_VOID] += void, [RS_PRUNED] += pruned, [POSE_BEST1] = max over the hypotheses of inliers + 1.
constexpr int RS_PRUNED = 1;
__global__ __launch_bounds__(RS_BLOCK) void k_ransac(const double *__restrict__ src, const double *__restrict__ dst,
                                                     const int32_t *__restrict__ tri, double *__restrict__ poses,
                                                     int32_t *__restrict__ inl, unsigned long long *__restrict__ st, long m, long h,
                                                     double md2, double r2)
{
    const int lane = threadIdx.x & 63;
    const long nw = (long)gridDim.x * RS_WAVES;
    unsigned long long n_void = 0, n_pruned = 0, best1 = 0;        // (the same in every lane of the wave)
    for (long k = (long)blockIdx.x * RS_WAVES + (threadIdx.x >> 6); k < h; k += nw) {
        const long i0 = tri[3 * k], i1 = tri[3 * k + 1], i2 = tri[3 * k + 2];
        Xf H;
#pragma unroll
        for (int j = 0; j < 12; ++j) H.m[j] = 0.0;
        int verdict = -1;
        if (i0 >= 0 && i0 < m && i1 >= 0 && i1 < m && i2 >= 0 && i2 < m && i0 != i1 && i0 != i2 && i1 != i2) {
            const V3 p0 = rs_load(src, i0), p1 = rs_load(src, i1), p2 = rs_load(src, i2);
            const V3 q0 = rs_load(dst, i0), q1 = rs_load(dst, i1), q2 = rs_load(dst, i2);
            if (rs_prunes(rs_len2(p0, p1), rs_len2(q0, q1), r2) || rs_prunes(rs_len2(p0, p2), rs_len2(q0, q2), r2) ||
                rs_prunes(rs_len2(p1, p2), rs_len2(q1, q2), r2)) {
                verdict = -2;
            } else {
                V3 a1, a2, a3, cp, b1, b2, b3, cq;
                rs_frame(p0, p1, p2, a1, a2, a3, cp);
                rs_frame(q0, q1, q2, b1, b2, b3, cq);
                const double A1[3] = {a1.x, a1.y, a1.z}, A2[3] = {a2.x, a2.y, a2.z}, A3[3] = {a3.x, a3.y, a3.z};
                const double B1[3] = {b1.x, b1.y, b1.z}, B2[3] = {b2.x, b2.y, b2.z}, B3[3] = {b3.x, b3.y, b3.z};
                const double CQ[3] = {cq.x, cq.y, cq.z};
                bool ok = true;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) H.m[4 * r + j] = (B1[r] * A1[j] + B2[r] * A2[j]) + B3[r] * A3[j];
                    H.m[4 * r + 3] = CQ[r] - ((H.m[4 * r] * cp.x + H.m[4 * r + 1] * cp.y) + H.m[4 * r + 2] * cp.z);
#pragma unroll
                    for (int j = 0; j < 4; ++j) ok = ok && finite_f64(H.m[4 * r + j]);
                }
                if (ok) verdict = 0;
                else {
#pragma unroll
                    for (int j = 0; j < 12; ++j) H.m[j] = 0.0;
                }
            }
        }
        int cnt = 0;
        if (verdict == 0) {
            for (long c0 = 0; c0 < m; c0 += 64) {
                const long c = c0 + lane;
                bool in = false;
                if (c < m) {
                    double p[3], q[3];
                    in = pose_row(src, dst, c, H, p, q) < md2;
                }
                cnt += __popcll((long long)__ballot(in));
            }
            best1 = best1 > (unsigned long long)cnt + 1 ? best1 : (unsigned long long)cnt + 1;
        }
        n_void += verdict == -1 ? 1 : 0;
        n_pruned += verdict == -2 ? 1 : 0;
        if (lane == 0) {
            inl[k] = verdict == 0 ? cnt : verdict;
            if (poses) pose_store(H, poses + 12 * k);
        }
    }
    if (lane == 0) {
        if (n_void) atomicAdd(st + POSE_VOID, n_void);
        if (n_pruned) atomicAdd(st + RS_PRUNED, n_pruned);
        if (best1) atomicMax(st + POSE_BEST1, best1);
    }
}

}  // namespace
}  // namespace sicp

namespace {

template <int DP>
void launch_match(sicp_ctx *c, dim3 grid, const float *q, const float *t, long nq, long nt, int dim, long chunk, long nchunks)
{
    hipLaunchKernelGGL(k_match<DP>, grid, dim3(MT_BLOCK), 0, c->stream, q, t, c->gl_key.p, nq, nt, dim, chunk, nchunks);
}

}  // namespace

SICP_EXPORT int sicp_global_version(void) { return SICP_GLOBAL_VERSION; }

SICP_EXPORT int sicp_feature_match(sicp_ctx *c, const float *query, int64_t nq, const float *target, int64_t nt, int dim,
                                   int32_t *idx_out, float *d2_out, sicp_match_stats *out)
{
    CHK(check_rows_ctx(c, "sicp_feature_match"));
    if (!query) return fail(SICP_ERR_INVALID, "query is null");
    if (!target) return fail(SICP_ERR_INVALID, "target is null");
    if (!idx_out) return fail(SICP_ERR_INVALID, "idx_out is null");
    if (!out) return fail(SICP_ERR_INVALID, "out is null");
    if (nq < 1) return fail(SICP_ERR_INVALID, "nq must be >= 1 (%lld given)", (long long)nq);
    if (nt < 1) return fail(SICP_ERR_INVALID, "nt must be >= 1 (%lld given)", (long long)nt);
    if (nt >= (1LL << 31)) return fail(SICP_ERR_INVALID, "nt must be < 2^31 (%lld given)", (long long)nt);
    if (dim < 1 || dim > SICP_MATCH_MAX_DIM) return fail(SICP_ERR_INVALID, "dim must be >= 1 and <= %d (%d given)", SICP_MATCH_MAX_DIM, dim);
    HIPCHK(hipSetDevice(c->device));
    return op_run(c, [&]() -> int {
        const float *q, *t;
        int32_t *idx;
        float *d2;
        CHK(stage_in(c, query, (size_t)nq * dim, c->gl_q, &q));
        CHK(stage_in(c, target, (size_t)nt * dim, c->gl_t, &t));
        CHK(stage_out(c, idx_out, (size_t)nq, c->gl_idx, &idx));
        CHK(stage_out(c, d2_out, (size_t)nq, c->gl_d2, &d2));
        CHK(c->gl_key.reserve((size_t)nq));
        CHK(counters_clear(c));
        HIPCHK(hipMemsetAsync(c->gl_key.p, 0xff, (size_t)nq * sizeof(unsigned long long), c->stream));
        // target rows per chunk: the ctx's switch, else whole tiles, as many chunks as bring the grid to MT_FILL workgroups
        const long nqb = (nq + MT_BLOCK - 1) / MT_BLOCK;
        const long want = std::max<long>(1, MT_FILL / nqb);
        const long chunk = c->match_chunk > 0 ? c->match_chunk : round_up(std::max<long>(1, (nt + want - 1) / want), MT_TILE);
        const long nchunks = (nt + chunk - 1) / chunk;
        const dim3 grid((unsigned)std::min<long>(nqb, MT_MAX_QBLOCKS), (unsigned)std::min<long>(nchunks, MT_MAX_CHUNKS));
        if (dim <= 4) launch_match<4>(c, grid, q, t, nq, nt, dim, chunk, nchunks);
        else if (dim <= 16) launch_match<16>(c, grid, q, t, nq, nt, dim, chunk, nchunks);
        else if (dim <= 36) launch_match<36>(c, grid, q, t, nq, nt, dim, chunk, nchunks);
        else launch_match<64>(c, grid, q, t, nq, nt, dim, chunk, nchunks);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_match_finish, dim3((unsigned)std::min<long>(nqb, MT_MAX_QBLOCKS)), dim3(MT_BLOCK), 0, c->stream, c->gl_key.p,
                           (long)nq, idx, d2, c->cand_small.p);
        HIPCHK(hipGetLastError());
        CHK(counters_fetch(c));
        CHK(stage_leave(c, idx_out, (size_t)nq, idx));
        CHK(stage_leave(c, d2_out, (size_t)nq, d2));
        CHK(sync(c));
        out->n_query = nq;
        out->n_target = nt;
        out->n_unmatched = (int64_t)counters_host(c)[0];
        return SICP_OK;
    });
}

SICP_EXPORT int sicp_ransac_triplets(sicp_ctx *c, const double *src, const double *dst, int64_t m, const int32_t *triples, int64_t h,
                                     double max_distance, double edge_ratio, double *poses_out, int32_t *inliers_out,
                                     sicp_ransac_stats *out)
{
    CHK(check_rows_ctx(c, "sicp_ransac_triplets"));
    CHK(check_matched(src, dst));
    if (!triples) return fail(SICP_ERR_INVALID, "triples is null");
    if (!inliers_out) return fail(SICP_ERR_INVALID, "inliers_out is null");
    if (!out) return fail(SICP_ERR_INVALID, "out is null");
    CHK(check_matched_count(m));
    if (h < 1) return fail(SICP_ERR_INVALID, "h must be >= 1 (%lld given)", (long long)h);
    CHK(check_max_distance(max_distance, false));
    if (!(edge_ratio >= 0.0 && edge_ratio <= 1.0)) return fail(SICP_ERR_INVALID, "edge_ratio must be >= 0 and <= 1");
    HIPCHK(hipSetDevice(c->device));
    return op_run(c, [&]() -> int {
        PoseRows R;
        const int32_t *tri;
        CHK(pose_rows_enter(c, src, dst, m, nullptr, h, poses_out, inliers_out, &R));
        CHK(stage_in(c, triples, (size_t)3 * h, c->gl_tri, &tri));
        hipLaunchKernelGGL(k_ransac, dim3((unsigned)std::min<long>((h + RS_WAVES - 1) / RS_WAVES, RS_MAX_BLOCKS)), dim3(RS_BLOCK), 0, c->stream,
                           R.src, R.dst, tri, R.poses, R.inl, c->cand_small.p, (long)m, (long)h, max_distance * max_distance,
                           edge_ratio * edge_ratio);
        HIPCHK(hipGetLastError());
        CHK(pose_best_enqueue(c, k_pose_best, R.inl, (long)h));
        CHK(pose_rows_leave(c, poses_out, inliers_out, h, R, out));
        out->n_hypotheses = h;
        out->n_pruned = (int64_t)counters_host(c)[RS_PRUNED];
        return SICP_OK;
    });
}
