// sicp_denoise.hip -- moving-least-squares smoothing at order 0/1 (include/simpleicp_hip_denoise.h; contract (W), DESIGN.md
// section 28): every point projected onto the plane fitted to its neighbourhood.
//
// One pass, shaped like sicp_keypoints.hip's first: a chunk's points go through the slot's k-NN search (rows_knn), then
// k_mls_project reads that chunk's ranked (chunk, k) lists.  A wave owns 64 consecutive points of the chunk; for each of them the
// lanes load that point's list row, gather the coordinates and form W, the three weighted means and the six weighted centred sums
// by xor-butterflies -- the adjacent-pair tree of the contract --, lane p keeps point p's numbers; then all 64 lanes run jacobi3
// with its eigenvectors, each on its own point, project and store.  Integer atomics count the record and take the maximum of the
// displacements' bit patterns; no floating-point atomic takes part, no wave waits for another.
#include "sicp_host.h"
#include "sicp_lanes.h"
#include "sicp_normals.h"
#include "../../include/simpleicp_hip_denoise.h"

namespace sicp {
namespace {

constexpr int DN_BLOCK = 256;
constexpr int DN_WAVES = DN_BLOCK / 64;
constexpr int DN_MAX_BLOCKS = 4096;                // the waves stride over the chunk from there on
enum { DN_SMALL = 0, DN_MOVED = 1, DN_CLIP = 2, DN_MAX = 3 };   // counter words; DN_MAX holds the bits of the largest fabs(g)

__device__ __forceinline__ double dn_first(double v)
{
    return __longlong_as_double((long long)first_lane_u64((unsigned long long)__double_as_longlong(v)));
}

// The adjacent-pair tree over the terms of lanes 0 .. span-1 (span a power of two, the same in every lane; all 64 lanes call), as
// sicp_keypoints.hip forms it: level J pairs lane l with lane l ^ J, lane 0 ends with the root, which every lane gets.  The levels
// from span on are left out, not fed with +0.0: a root of -0.0 stays -0.0.
__device__ __forceinline__ double dn_tree(double v, int span)
{
    if (span > 1) v = v + lane_xor_f64<1>(v);
    if (span > 2) v = v + lane_xor_f64<2>(v);
    if (span > 4) v = v + lane_xor_f64<4>(v);
    if (span > 8) v = v + lane_xor_f64<8>(v);
    if (span > 16) v = v + lane_xor_f64<16>(v);
    if (span > 32) v = v + lane_xor_f64<32>(v);
    return dn_first(v);
}

__device__ __forceinline__ unsigned long long dn_wave_max(unsigned long long v)
{
    unsigned long long o;
    o = lane_xor64<32>(v); v = o > v ? o : v;
    o = lane_xor64<16>(v); v = o > v ? o : v;
    o = lane_xor64<8>(v); v = o > v ? o : v;
    o = lane_xor64<4>(v); v = o > v ? o : v;
    o = lane_xor64<2>(v); v = o > v ? o : v;
    o = lane_xor64<1>(v); v = o > v ? o : v;
    return v;
}

// Points lo .. lo + Q of the cloud, their ranked lists d2l / idxl (Q, k).  P: (n, 3) points out; N (nullable): (n, 3) float32
// normals; G (nullable): (n) displacements.  Every index that reaches X / Y / Z, P, N or G lies in 0 .. n-1: a list entry outside
// that range counts nowhere and is never dereferenced.
__global__ __launch_bounds__(DN_BLOCK) void k_mls_project(const double *__restrict__ X, const double *__restrict__ Y,
                                                          const double *__restrict__ Z, const double *__restrict__ d2l,
                                                          const int64_t *__restrict__ idxl, double *__restrict__ P,
                                                          float *__restrict__ N, double *__restrict__ G, long n, long lo, long Q, int k,
                                                          double r2, int no_radius, double b2, int no_bandwidth, double strength,
                                                          long long min_nb, unsigned long long *__restrict__ st)
{
    const int lane = threadIdx.x & 63;
    const bool two = k > 64;                                       // two ranks a lane: 2 lane and 2 lane + 1 (the tree's first level)
    int K = 2;
    while (K < k) K *= 2;
    const int span = two ? K / 2 : K;
    const int ra = two ? 2 * lane : lane, rb = 2 * lane + 1;
    const long groups = (Q + 63) / 64, nw = (long)gridDim.x * DN_WAVES;
    unsigned long long n_small = 0, n_moved = 0, n_clip = 0, top = 0;   // (the counts the same in every lane of the wave; top the lane's own)
    for (long g = (long)blockIdx.x * DN_WAVES + (threadIdx.x >> 6); g < groups; g += nw) {
        const long base = g * 64;
        const int cntw = (int)(Q - base < 64 ? Q - base : 64);
        double sW = 0.0, mx = 0.0, my = 0.0, mz = 0.0, s00 = 0.0, s01 = 0.0, s02 = 0.0, s11 = 0.0, s12 = 0.0, s22 = 0.0;
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
            double wa = 1.0, wb = 1.0;
            if (!no_bandwidth) {
                const double ta = 1.0 - d2a / b2, tb = 1.0 - d2b / b2;
                wa = ta > 0.0 ? ta * ta : 0.0;
                wb = tb > 0.0 ? tb * tb : 0.0;
            }
            // (a rank that does not count contributes +0.0, whatever its product would be)
#define DN_SUM(ta, tb) dn_tree(two ? (in_a ? (ta) : 0.0) + (in_b ? (tb) : 0.0) : (in_a ? (ta) : 0.0), span)
            const double W = DN_SUM(wa, wb);
            const double cx = DN_SUM(wa * xa, wb * xb) / W;
            const double cy = DN_SUM(wa * ya, wb * yb) / W;
            const double cz = DN_SUM(wa * za, wb * zb) / W;
            const double ax = xa - cx, ay = ya - cy, az = za - cz, bx = xb - cx, by = yb - cy, bz = zb - cz;
            const double t00 = DN_SUM(wa * (ax * ax), wb * (bx * bx)), t01 = DN_SUM(wa * (ax * ay), wb * (bx * by));
            const double t02 = DN_SUM(wa * (ax * az), wb * (bx * bz)), t11 = DN_SUM(wa * (ay * ay), wb * (by * by));
            const double t12 = DN_SUM(wa * (ay * az), wb * (by * bz)), t22 = DN_SUM(wa * (az * az), wb * (bz * bz));
#undef DN_SUM
            if (lane == t) {
                sW = W; mx = cx; my = cy; mz = cz;
                s00 = t00; s01 = t01; s02 = t02; s11 = t11; s12 = t12; s22 = t22;
                mine_m = m; mine_clip = clip;
            }
        }
        // every lane its own point
        const bool valid = lane < cntw;
        const long i = lo + base + (valid ? lane : 0);
        const bool small = (long long)mine_m < min_nb;
        double C[3][3], V[3][3];
        C[0][0] = s00 / sW; C[0][1] = s01 / sW; C[0][2] = s02 / sW; C[1][1] = s11 / sW; C[1][2] = s12 / sW; C[2][2] = s22 / sW;
        if (!valid || small) { C[0][0] = 0.0; C[0][1] = 0.0; C[0][2] = 0.0; C[1][1] = 0.0; C[1][2] = 0.0; C[2][2] = 0.0; }
        C[1][0] = C[0][1]; C[2][0] = C[0][2]; C[2][1] = C[1][2];
        jacobi3(C, V);
        const double w[3] = {C[0][0], C[1][1], C[2][2]};
        int l = 0, h = 0;                                         // normal_from_cov's column and sign
#pragma unroll
        for (int c = 1; c < 3; ++c) { if (w[c] < w[l]) l = c; if (w[c] > w[h]) h = c; }
        if (l == h) l = 2;
        double n0 = 0.0, n1 = 0.0, n2 = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (c == l) { n0 = V[0][c]; n1 = V[1][c]; n2 = V[2][c]; }
        int big = 0; double bigv = fabs(n0);
        if (fabs(n1) > bigv) { big = 1; bigv = fabs(n1); }
        if (fabs(n2) > bigv) { big = 2; }
        const double lead = (big == 0) ? n0 : (big == 1) ? n1 : n2;
        if (lead < 0) { n0 = -n0; n1 = -n1; n2 = -n2; }
        const double xi = X[i], yi = Y[i], zi = Z[i];
        double gd = 0.0, ox = xi, oy = yi, oz = zi;
        if (small) { n0 = 0.0; n1 = 0.0; n2 = 0.0; }
        else {
            const double hd = ((xi - mx) * n0 + (yi - my) * n1) + (zi - mz) * n2;
            gd = strength * hd;
            ox = xi - gd * n0; oy = yi - gd * n1; oz = zi - gd * n2;
        }
        if (valid) {
            P[3 * i] = ox; P[3 * i + 1] = oy; P[3 * i + 2] = oz;
            if (N) { N[3 * i] = (float)n0; N[3 * i + 1] = (float)n1; N[3 * i + 2] = (float)n2; }
            if (G) G[i] = gd;
            const unsigned long long bits = (unsigned long long)__double_as_longlong(fabs(gd));
            top = bits > top ? bits : top;
        }
        n_small += (unsigned long long)__popcll((long long)__ballot(valid && small));
        n_moved += (unsigned long long)__popcll((long long)__ballot(valid && gd != 0.0));
        n_clip += (unsigned long long)__popcll((long long)__ballot(valid && mine_clip));
    }
    top = dn_wave_max(top);
    if (lane == 0) {
        if (n_small) atomicAdd(st + DN_SMALL, n_small);
        if (n_moved) atomicAdd(st + DN_MOVED, n_moved);
        if (n_clip) atomicAdd(st + DN_CLIP, n_clip);
        if (top) atomicMax(st + DN_MAX, top);
    }
}

}  // namespace
}  // namespace sicp

namespace {

static_assert(DN_MAX < CAND_WORDS, "the record's counters fit the ctx's counter words");

}  // namespace

SICP_EXPORT int sicp_denoise_version(void) { return SICP_DENOISE_VERSION; }

SICP_EXPORT int sicp_denoise(sicp_ctx *c, int slot, int k, double radius, double bandwidth, double strength, int64_t min_neighbors,
                             double *points_out, float *normals_out, double *displacement_out, sicp_denoise_stats *out)
{
    CHK(check_slot(c, slot, true));
    if (!points_out) return fail(SICP_ERR_INVALID, "points_out is null");
    if (!out) return fail(SICP_ERR_INVALID, "out is null");
    Cloud &cl = c->cloud[slot];
    if (k < 2) return fail(SICP_ERR_INVALID, "k must be >= 2 (%d given)", k);
    if (k > SICP_KEYPOINT_MAX_K) return fail(SICP_ERR_INVALID, "k must be <= %d (%d given)", SICP_KEYPOINT_MAX_K, k);
    if (k > cl.n) return fail(SICP_ERR_INVALID, "k (%d) exceeds the number of points (%lld)", k, (long long)cl.n);
    if (std::isnan(radius) || !(radius > 0.0)) return fail(SICP_ERR_INVALID, "radius must be > 0 (+inf: none)");
    if (std::isnan(bandwidth) || !(bandwidth > 0.0)) return fail(SICP_ERR_INVALID, "bandwidth must be > 0 (+inf: none)");
    if (!std::isfinite(strength) || strength < 0.0 || strength > 1.0) return fail(SICP_ERR_INVALID, "strength must be finite, >= 0 and <= 1");
    if (min_neighbors < 1) return fail(SICP_ERR_INVALID, "min_neighbors must be >= 1 (%lld given)", (long long)min_neighbors);
    CHK(check_whole_cloud(c, slot, "sicp_denoise", "a point's neighbours may live on another rank"));
    HIPCHK(hipSetDevice(c->device));
    return op_run(c, [&]() -> int {
        const long n = (long)cl.n;
        double *pts, *disp;
        float *nrm;
        // (the staging buffers are the keypoints' and the orientation's: an operator call is over before the next begins)
        CHK(stage_out(c, points_out, (size_t)3 * n, c->kp_eig, &pts));
        CHK(stage_out(c, normals_out, (size_t)3 * n, c->or_out, &nrm));
        CHK(stage_out(c, displacement_out, (size_t)n, c->kp_sal, &disp));
        CHK(counters_clear(c));
        const long chunk = knn_chunk(c->denoise_chunk, k);
        CHK(knn_chunk_reserve(c, std::min(chunk, n), k));
        for (long lo = 0; lo < n; lo += chunk) {
            const long cnt = std::min(chunk, n - lo);
            CHK(rows_knn(c, slot, nullptr, lo, cnt, k));
            const unsigned g = std::min(cdiv(cdiv(cnt, 64), DN_WAVES), (unsigned)DN_MAX_BLOCKS);
            hipLaunchKernelGGL(k_mls_project, dim3(g), dim3(DN_BLOCK), 0, c->stream, cl.x(), cl.y(), cl.z(), c->k_d2.p, c->k_idx.p, pts, nrm,
                               disp, n, lo, cnt, k, radius * radius, std::isinf(radius) ? 1 : 0, bandwidth * bandwidth,
                               std::isinf(bandwidth) ? 1 : 0, strength, (long long)min_neighbors, c->cand_small.p);
            HIPCHK(hipGetLastError());
        }
        CHK(counters_fetch(c));
        CHK(stage_leave(c, points_out, (size_t)3 * n, pts));
        CHK(stage_leave(c, normals_out, (size_t)3 * n, nrm));
        CHK(stage_leave(c, displacement_out, (size_t)n, disp));
        CHK(sync(c));
        const unsigned long long *h = counters_host(c);
        out->n_points = (int64_t)n;
        out->n_small = (int64_t)h[DN_SMALL];
        out->n_moved = (int64_t)h[DN_MOVED];
        out->n_clipped = (int64_t)h[DN_CLIP];
        std::memcpy(&out->max_displacement, &h[DN_MAX], sizeof(double));
        return SICP_OK;
    });
}
