// sicp_keypoints.hip -- ISS keypoints (include/simpleicp_hip_keypoints.h; contract (I)).
//
// Two passes, shaped like sicp_fpfh.hip: a chunk's points go through the slot's k-NN search (rows_knn), then a kernel reads that
// chunk's ranked (chunk, k) lists.  Pass 1 (k_iss_saliency): a wave owns 64 consecutive points of the chunk; for each of them the
// lanes load that point's list row, gather the coordinates and form the three means and the six centred sums by xor-butterflies --
// the adjacent-pair tree of the contract --, lane p keeps point p's numbers; then all 64 lanes run jacobi3, each on its own point.
// The salient points' rows are collected on the way (wave_append: one atomic per 64 points, as k_ol_compact collects a mask's).
// Pass 2 (k_iss_nms) searches only those rows, with k_n: one wave per salient row, lanes over the ranks, each reads its
// neighbour's saliency, one ballot decides the row.  Integer atomics count the record; no floating-point atomic takes part.
#include "sicp_host.h"
#include "sicp_lanes.h"
#include "sicp_normals.h"
#include "../../include/simpleicp_hip_keypoints.h"

namespace sicp {
namespace {

constexpr int KP_BLOCK = 256;
constexpr int KP_WAVES = KP_BLOCK / 64;
constexpr int KP_MAX_BLOCKS = 4096;                // the waves stride over the chunk from there on
enum { KP_SALIENT = 0, KP_KEYPOINTS = 1, KP_SMALL = 2, KP_CLIP_S = 3, KP_CLIP_N = 4 };   // counter words; KP_SALIENT is the row list's cursor too

__device__ __forceinline__ double kp_first(double v)
{
    return __longlong_as_double((long long)first_lane_u64((unsigned long long)__double_as_longlong(v)));
}

// The adjacent-pair tree over the terms of lanes 0 .. span-1 (span a power of two, the same in every lane; all 64 lanes call):
// level J pairs lane l with lane l ^ J, so after the levels J < span lane 0 holds the tree's root, which every lane gets.  The
// levels from span on are left out, not fed with +0.0: a root of -0.0 stays -0.0.
__device__ __forceinline__ double kp_tree(double v, int span)
{
    if (span > 1) v = v + lane_xor_f64<1>(v);
    if (span > 2) v = v + lane_xor_f64<2>(v);
    if (span > 4) v = v + lane_xor_f64<4>(v);
    if (span > 8) v = v + lane_xor_f64<8>(v);
    if (span > 16) v = v + lane_xor_f64<16>(v);
    if (span > 32) v = v + lane_xor_f64<32>(v);
    return kp_first(v);
}

// Pass 1.  Points lo .. lo + Q of the cloud, their ranked lists d2l / idxl (Q, k).  sal: s_i by point; eig (nullable): (n, 3);
// keep: zeroed for every point here (pass 2 sets the keypoints'); rows: the salient points, from the cursor st[KP_SALIENT] on.
__global__ __launch_bounds__(KP_BLOCK) void k_iss_saliency(const double *__restrict__ X, const double *__restrict__ Y,
                                                           const double *__restrict__ Z, const double *__restrict__ d2l,
                                                           const int64_t *__restrict__ idxl, double *__restrict__ sal,
                                                           double *__restrict__ eig, uint8_t *__restrict__ keep, long n, long lo, long Q,
                                                           int k, double r2, int no_radius, double gamma21, double gamma32,
                                                           long long min_nb, int64_t *__restrict__ rows,
                                                           unsigned long long *__restrict__ st)
{
    const int lane = threadIdx.x & 63;
    const bool two = k > 64;                                       // two ranks a lane: 2 lane and 2 lane + 1 (the tree's first level)
    int K = 2;
    while (K < k) K *= 2;
    const int span = two ? K / 2 : K;
    const int ra = two ? 2 * lane : lane, rb = 2 * lane + 1;
    const long groups = (Q + 63) / 64, nw = (long)gridDim.x * KP_WAVES;
    unsigned long long n_small = 0, n_clip = 0;                    // (the same in every lane of the wave)
    for (long g = (long)blockIdx.x * KP_WAVES + (threadIdx.x >> 6); g < groups; g += nw) {
        const long base = g * 64;
        const int cntw = (int)(Q - base < 64 ? Q - base : 64);
        double s00 = 0.0, s01 = 0.0, s02 = 0.0, s11 = 0.0, s12 = 0.0, s22 = 0.0;
        unsigned mine_m = 0;
        bool mine_clip = false;
        for (int t = 0; t < cntw; ++t) {
            const long q = base + t, i = lo + q;
            const bool have_a = ra < k, have_b = two && rb < k;
            const long ja_l = have_a ? (long)idxl[q * k + ra] : -1, jb_l = have_b ? (long)idxl[q * k + rb] : -1;
            const bool there_a = ja_l >= 0 && ja_l < n, there_b = jb_l >= 0 && jb_l < n;   // (a rank that holds no point counts nowhere)
            const double d2a = have_a ? d2l[q * k + ra] : 0.0, d2b = have_b ? d2l[q * k + rb] : 0.0;
            const bool in_a = there_a && (no_radius || d2a < r2), in_b = there_b && (no_radius || d2b < r2);
            const long ja = there_a ? ja_l : i, jb = there_b ? jb_l : i;
            const double xa = in_a ? X[ja] : 0.0, ya = in_a ? Y[ja] : 0.0, za = in_a ? Z[ja] : 0.0;
            double xb = 0.0, yb = 0.0, zb = 0.0;
            if (two) { xb = in_b ? X[jb] : 0.0; yb = in_b ? Y[jb] : 0.0; zb = in_b ? Z[jb] : 0.0; }
            const unsigned m = (unsigned)__popcll((long long)__ballot(in_a)) + (unsigned)__popcll((long long)__ballot(in_b));
            const bool clip = __ballot((in_a && ra == k - 1) || (in_b && rb == k - 1)) != 0ull && !no_radius;
            const double md = (double)m;
            const double cx = kp_tree(two ? xa + xb : xa, span) / md;
            const double cy = kp_tree(two ? ya + yb : ya, span) / md;
            const double cz = kp_tree(two ? za + zb : za, span) / md;
            const double ax = xa - cx, ay = ya - cy, az = za - cz, bx = xb - cx, by = yb - cy, bz = zb - cz;
            // (a rank that does not count contributes +0.0, whatever its difference would be)
#define KP_SUM(u, v, w, z) kp_tree(two ? (in_a ? (u) * (v) : 0.0) + (in_b ? (w) * (z) : 0.0) : (in_a ? (u) * (v) : 0.0), span)
            const double t00 = KP_SUM(ax, ax, bx, bx), t01 = KP_SUM(ax, ay, bx, by), t02 = KP_SUM(ax, az, bx, bz);
            const double t11 = KP_SUM(ay, ay, by, by), t12 = KP_SUM(ay, az, by, bz), t22 = KP_SUM(az, az, bz, bz);
#undef KP_SUM
            if (lane == t) {
                s00 = t00; s01 = t01; s02 = t02; s11 = t11; s12 = t12; s22 = t22;
                mine_m = m; mine_clip = clip;
            }
        }
        // every lane its own point
        const bool valid = lane < cntw;
        const long i = lo + base + (valid ? lane : 0);
        const double md = (double)mine_m;
        double C[3][3], V[3][3];
        C[0][0] = s00 / md; C[0][1] = s01 / md; C[0][2] = s02 / md; C[1][1] = s11 / md; C[1][2] = s12 / md; C[2][2] = s22 / md;
        if (!valid || mine_m == 0u) { C[0][0] = 0.0; C[0][1] = 0.0; C[0][2] = 0.0; C[1][1] = 0.0; C[1][2] = 0.0; C[2][2] = 0.0; }
        C[1][0] = C[0][1]; C[2][0] = C[0][2]; C[2][1] = C[1][2];
        jacobi3(C, V);
        const double w[3] = {C[0][0], C[1][1], C[2][2]};
        int l = 0, h = 0;                                         // normal_from_cov's order
#pragma unroll
        for (int c = 1; c < 3; ++c) { if (w[c] < w[l]) l = c; if (w[c] > w[h]) h = c; }
        if (l == h) { l = 2; h = 0; }
        const int mid = 3 - l - h;
        double e1 = 0.0, e2 = 0.0, e3 = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c == h) e1 = w[c];
            if (c == mid) e2 = w[c];
            if (c == l) e3 = w[c];
        }
        const bool small = (long long)mine_m < min_nb;
        const bool salient = valid && !small && e2 < gamma21 * e1 && e3 < gamma32 * e2 && e3 > 0.0;
        if (valid) {
            sal[i] = salient ? e3 : 0.0;
            keep[i] = 0;
            if (eig) { eig[3 * i] = e1; eig[3 * i + 1] = e2; eig[3 * i + 2] = e3; }
        }
        n_small += (unsigned long long)__popcll((long long)__ballot(valid && small));
        n_clip += (unsigned long long)__popcll((long long)__ballot(valid && mine_clip));
        const unsigned long long at = wave_append(st + KP_SALIENT, salient);
        if (salient) rows[at] = i;
    }
    if (lane == 0) {
        if (n_small) atomicAdd(st + KP_SMALL, n_small);
        if (n_clip) atomicAdd(st + KP_CLIP_S, n_clip);
    }
}

// Pass 2.  The salient rows rows[0 .. Q) of this chunk, their ranked lists (Q, k); sal by point; keep by point.
__global__ __launch_bounds__(KP_BLOCK) void k_iss_nms(const double *__restrict__ d2l, const int64_t *__restrict__ idxl,
                                                      const int64_t *__restrict__ rows, const double *__restrict__ sal,
                                                      uint8_t *__restrict__ keep, long n, long Q, int k, double r2, int no_radius,
                                                      long long min_nb, unsigned long long *__restrict__ st)
{
    const int lane = threadIdx.x & 63;
    const long nw = (long)gridDim.x * KP_WAVES;
    unsigned long long n_key = 0, n_clip = 0;
    for (long q = (long)blockIdx.x * KP_WAVES + (threadIdx.x >> 6); q < Q; q += nw) {
        const long i = (long)rows[q];
        const double si = sal[i];
        unsigned cnt = 0;
        bool beaten = false, clip = false;
        for (int r0 = 0; r0 < k; r0 += 64) {
            const int r = r0 + lane;
            const bool have = r < k;
            const long jl = have ? (long)idxl[q * k + r] : -1;
            const bool there = jl >= 0 && jl < n;
            const long j = there ? jl : i;
            const double d2 = have ? d2l[q * k + r] : 0.0;
            const bool in = there && (no_radius || d2 < r2);
            const double sj = sal[j];
            const bool wins = si > sj || (si == sj && i < j);
            cnt += (unsigned)__popcll((long long)__ballot(in));
            beaten = beaten || __ballot(in && j != i && !wins) != 0ull;
            clip = clip || __ballot(in && r == k - 1) != 0ull;
        }
        const bool key = (long long)cnt >= min_nb && !beaten;
        if (lane == 0) keep[i] = key ? 1 : 0;
        n_key += key ? 1 : 0;
        n_clip += (clip && !no_radius) ? 1 : 0;
    }
    if (lane == 0) {
        if (n_key) atomicAdd(st + KP_KEYPOINTS, n_key);
        if (n_clip) atomicAdd(st + KP_CLIP_N, n_clip);
    }
}

}  // namespace
}  // namespace sicp

namespace {

static_assert(KP_CLIP_N < CAND_WORDS, "the record's counters fit the ctx's counter words");

int kp_check_k(const char *name, int k, int64_t n)
{
    if (k < 2) return fail(SICP_ERR_INVALID, "%s must be >= 2 (%d given)", name, k);
    if (k > SICP_KEYPOINT_MAX_K) return fail(SICP_ERR_INVALID, "%s must be <= %d (%d given)", name, SICP_KEYPOINT_MAX_K, k);
    if (k > n) return fail(SICP_ERR_INVALID, "%s (%d) exceeds the number of points (%lld)", name, k, (long long)n);
    return SICP_OK;
}

}  // namespace

SICP_EXPORT int sicp_keypoints_version(void) { return SICP_KEYPOINTS_VERSION; }

SICP_EXPORT int sicp_keypoints(sicp_ctx *c, int slot, int k_s, double salient_radius, int k_n, double nms_radius, double gamma21,
                               double gamma32, int64_t min_neighbors, uint8_t *keep_out, double *saliency_out, double *eig_out,
                               sicp_keypoint_stats *out)
{
    CHK(check_slot(c, slot, true));
    if (!keep_out) return fail(SICP_ERR_INVALID, "keep_out is null");
    if (!out) return fail(SICP_ERR_INVALID, "out is null");
    Cloud &cl = c->cloud[slot];
    CHK(kp_check_k("k_s", k_s, cl.n));
    CHK(kp_check_k("k_n", k_n, cl.n));
    if (std::isnan(salient_radius) || !(salient_radius > 0.0)) return fail(SICP_ERR_INVALID, "salient_radius must be > 0 (+inf: none)");
    if (std::isnan(nms_radius) || !(nms_radius > 0.0)) return fail(SICP_ERR_INVALID, "nms_radius must be > 0 (+inf: none)");
    if (!std::isfinite(gamma21) || !(gamma21 > 0.0)) return fail(SICP_ERR_INVALID, "gamma21 must be finite and > 0");
    if (!std::isfinite(gamma32) || !(gamma32 > 0.0)) return fail(SICP_ERR_INVALID, "gamma32 must be finite and > 0");
    if (min_neighbors < 1) return fail(SICP_ERR_INVALID, "min_neighbors must be >= 1 (%lld given)", (long long)min_neighbors);
    CHK(check_whole_cloud(c, slot, "sicp_keypoints", "a point's neighbours may live on another rank"));
    HIPCHK(hipSetDevice(c->device));
    return op_run(c, [&]() -> int {
        const long n = (long)cl.n;
        uint8_t *keep;
        double *sal, *eig;
        CHK(stage_out(c, keep_out, (size_t)n, c->cand_keep, &keep));
        CHK(stage_out(c, saliency_out, (size_t)n, c->kp_sal, &sal));
        if (!sal) { CHK(c->kp_sal.reserve((size_t)n)); sal = c->kp_sal.p; }
        CHK(stage_out(c, eig_out, (size_t)3 * n, c->kp_eig, &eig));
        CHK(c->cand_rows.reserve((size_t)n));
        CHK(counters_clear(c));
        // pass 1: every point, k_s
        const long chunk_s = knn_chunk(c->keypoint_chunk, k_s);
        CHK(knn_chunk_reserve(c, std::min(chunk_s, n), k_s));
        for (long lo = 0; lo < n; lo += chunk_s) {
            const long cnt = std::min(chunk_s, n - lo);
            CHK(rows_knn(c, slot, nullptr, lo, cnt, k_s));
            const unsigned g = std::min(cdiv(cdiv(cnt, 64), KP_WAVES), (unsigned)KP_MAX_BLOCKS);
            hipLaunchKernelGGL(k_iss_saliency, dim3(g), dim3(KP_BLOCK), 0, c->stream, cl.x(), cl.y(), cl.z(), c->k_d2.p, c->k_idx.p, sal, eig,
                               keep, n, lo, cnt, k_s, salient_radius * salient_radius, std::isinf(salient_radius) ? 1 : 0, gamma21, gamma32,
                               (long long)min_neighbors, c->cand_rows.p, c->cand_small.p);
            HIPCHK(hipGetLastError());
        }
        CHK(counters_fetch(c));
        CHK(sync(c));                                              // (the number of salient rows sizes pass 2)
        const long ns = (long)counters_host(c)[KP_SALIENT];
        // pass 2: the salient rows, k_n
        const long chunk_n = knn_chunk(c->keypoint_chunk, k_n);
        if (ns > 0) CHK(knn_chunk_reserve(c, std::min(chunk_n, ns), k_n));
        for (long lo = 0; lo < ns; lo += chunk_n) {
            const long cnt = std::min(chunk_n, ns - lo);
            CHK(rows_knn(c, slot, c->cand_rows.p, lo, cnt, k_n));
            const unsigned g = std::min(cdiv(cnt, KP_WAVES), (unsigned)KP_MAX_BLOCKS);
            hipLaunchKernelGGL(k_iss_nms, dim3(g), dim3(KP_BLOCK), 0, c->stream, c->k_d2.p, c->k_idx.p, c->cand_rows.p + lo, sal, keep, n, cnt,
                               k_n, nms_radius * nms_radius, std::isinf(nms_radius) ? 1 : 0, (long long)min_neighbors, c->cand_small.p);
            HIPCHK(hipGetLastError());
        }
        CHK(counters_fetch(c));
        CHK(stage_leave(c, keep_out, (size_t)n, keep));
        CHK(stage_leave(c, saliency_out, (size_t)n, sal));
        CHK(stage_leave(c, eig_out, (size_t)3 * n, eig));
        CHK(sync(c));
        const unsigned long long *h = counters_host(c);
        out->n_points = (int64_t)n;
        out->n_salient = (int64_t)h[KP_SALIENT];
        out->n_keypoints = (int64_t)h[KP_KEYPOINTS];
        out->n_small = (int64_t)h[KP_SMALL];
        out->n_clipped_salient = (int64_t)h[KP_CLIP_S];
        out->n_clipped_nms = (int64_t)h[KP_CLIP_N];
        return SICP_OK;
    });
}
