// sicp_plane.hip -- planes of a cloud (include/simpleicp_hip_plane.h; contracts (P) and (Q)).
//
// Scoring (k_pl_score) is blocked the other way round than k_ransac: there a wave owns a hypothesis and sweeps all rows, right for
// a few hundred matches; here a LANE owns a hypothesis (HPL of them) -- its four plane numbers stay in registers, its count is a
// private integer -- and the workgroup stages a tile of rows into LDS, a masked-out row as NaN so that it fails the test without a
// branch.  Every lane reads the same LDS address for a row (a broadcast read), and after its span of rows adds its integer to
// inliers[k] with one integer atomic: the sums are exact whatever the grid.  The grid is (spans of rows) x (blocks of hypotheses):
// the cloud is read once per hypothesis block, not once per hypothesis.  The void verdict and the plane come from a kernel of
// their own before the sweep (k_pl_planes, one thread per hypothesis); the record's best index is sicp_pose_dev.h's k_pose_best.
// Refit: the pose refit's two sweeps per round (sicp_posefit.hip) for one cloud and a plane -- first stage per span of 1 024 rows
// (k_pl_sweep: sweep A the three coordinates and the count, sweep B the six centred products), second stage one workgroup per
// plane (k_pl_fold_a settles "keep the best" and the centroid, k_pl_fold_b leaves the six sums), then one thread per plane runs
// jacobi3 and settles the next plane (k_pl_settle); the tree is sicp_pairtree.h's.  Integer atomics only; no kernel waits for another wave or workgroup.
#include "sicp_pose_dev.h"
#include "sicp_normals.h"
#include "../../include/simpleicp_hip_plane.h"

namespace sicp {
namespace {

constexpr int PL_BLOCK = 256;                      // lanes of a scoring workgroup
constexpr int PL_TILE = 1024;                      // rows in LDS at a time (24 KiB)
constexpr long PL_MAX_SPAN = 16L * PL_TILE;        // most rows a workgroup takes where the call chooses
constexpr int PL_FILL = 2048;                      // workgroups the choice of the span aims at
constexpr int PL_MAX_HBLOCKS = 1024;               // grid limit of the hypotheses' dimension: the workgroups stride from there on
constexpr int PL_CAND = 1;                         // the operator's counter word: candidate rows; the refit's: improved planes
constexpr int PL_IMPROVED = 1;
constexpr int PL_A = 3, PL_B = 6;                  // terms of sweep A (the coordinates) and of sweep B (the centred products)

// a row's residual under the plane (a, b, c, d): the contracts' one expression
__device__ __forceinline__ double pl_resid(double a, double b, double c, double d, double x, double y, double z)
{
    return fma(c, z, fma(b, y, a * x)) + d;
}

__device__ __forceinline__ unsigned long long wmax_u64(unsigned long long v)
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

// One thread per hypothesis: the verdict and the plane (contract (P), steps 1 and 2).  planes: (h, 4); inl: 0 or -1.
__global__ __launch_bounds__(POSE_BLOCK) void k_pl_planes(const double *__restrict__ X, const uint8_t *__restrict__ mask,
                                                          const int32_t *__restrict__ tri, double *__restrict__ planes,
                                                          int32_t *__restrict__ inl, unsigned long long *__restrict__ st, long n, long h)
{
    const long k = (long)blockIdx.x * POSE_BLOCK + threadIdx.x;
    bool is_void = false;
    if (k < h) {
        const long i0 = tri[3 * k], i1 = tri[3 * k + 1], i2 = tri[3 * k + 2];
        double a = 0.0, b = 0.0, c = 0.0, d = 0.0;
        bool ok = false;
        if (i0 >= 0 && i0 < n && i1 >= 0 && i1 < n && i2 >= 0 && i2 < n && i0 != i1 && i0 != i2 && i1 != i2 &&
            (!mask || (mask[i0] && mask[i1] && mask[i2]))) {
            const double p0x = X[3 * i0], p0y = X[3 * i0 + 1], p0z = X[3 * i0 + 2];
            const double ux = X[3 * i1] - p0x, uy = X[3 * i1 + 1] - p0y, uz = X[3 * i1 + 2] - p0z;
            const double vx = X[3 * i2] - p0x, vy = X[3 * i2 + 1] - p0y, vz = X[3 * i2 + 2] - p0z;
            const double wx = uy * vz - uz * vy, wy = uz * vx - ux * vz, wz = ux * vy - uy * vx;
            const double len = sqrt((wx * wx + wy * wy) + wz * wz);
            a = wx / len; b = wy / len; c = wz / len;
            d = -((a * p0x + b * p0y) + c * p0z);
            ok = finite_f64(a) && finite_f64(b) && finite_f64(c) && finite_f64(d);
        }
        planes[4 * k] = ok ? a : 0.0; planes[4 * k + 1] = ok ? b : 0.0; planes[4 * k + 2] = ok ? c : 0.0; planes[4 * k + 3] = ok ? d : 0.0;
        inl[k] = ok ? 0 : -1;
        is_void = !ok;
    }
    const unsigned long long who = (unsigned long long)__ballot(is_void);
    if ((threadIdx.x & 63) == 0 && who) atomicAdd(st + POSE_VOID, (unsigned long long)__popcll((long long)who));
}

// The sweep: workgroup (x, y) takes the rows [x * span, +span) and the hypotheses of the blocks y, y + gridDim.y, ...; lane t of
// block hb owns the hypotheses (hb * HPL + j) * PL_BLOCK + t.  inl[k] (0 for a valid hypothesis, -1 for a void one, which takes no
// part) += the lane's count; st[PL_CAND] += the candidate rows, counted once per span by the workgroups of y == 0.
template <int HPL>
__global__ __launch_bounds__(PL_BLOCK) void k_pl_score(const double *__restrict__ X, const uint8_t *__restrict__ mask,
                                                       const double *__restrict__ planes, int32_t *inl, unsigned long long *st, long n, long h,
                                                       long span, double md)
{
    __shared__ double sx[PL_TILE], sy[PL_TILE], sz[PL_TILE];
    const long lo = (long)blockIdx.x * span, hi = lo + span < n ? lo + span : n;
    const long nhb = (h + (long)PL_BLOCK * HPL - 1) / ((long)PL_BLOCK * HPL);
    const double nan = __builtin_nan("");
    unsigned cand = 0;
    for (long hb = blockIdx.y; hb < nhb; hb += gridDim.y) {
        double a[HPL], b[HPL], c[HPL], d[HPL];
        unsigned cnt[HPL];
        bool live[HPL];
#pragma unroll
        for (int j = 0; j < HPL; ++j) {
            const long k = (hb * HPL + j) * PL_BLOCK + threadIdx.x;
            live[j] = k < h && __hip_atomic_load(inl + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 0;   // (other workgroups are adding to it)
            a[j] = live[j] ? planes[4 * k] : nan; b[j] = live[j] ? planes[4 * k + 1] : nan;
            c[j] = live[j] ? planes[4 * k + 2] : nan; d[j] = live[j] ? planes[4 * k + 3] : nan;
            cnt[j] = 0;
        }
        const bool count_rows = blockIdx.y == 0 && hb == 0;
        for (long t0 = lo; t0 < hi; t0 += PL_TILE) {
            const int rows = hi - t0 < PL_TILE ? (int)(hi - t0) : PL_TILE;
            __syncthreads();                                       // (the last tile has been read by everyone)
            for (int e = threadIdx.x; e < rows; e += PL_BLOCK) {
                const long i = t0 + e;
                const bool m = !mask || mask[i] != 0;
                if (count_rows) cand += m ? 1u : 0u;
                sx[e] = m ? X[3 * i] : nan; sy[e] = m ? X[3 * i + 1] : nan; sz[e] = m ? X[3 * i + 2] : nan;
            }
            __syncthreads();
#pragma unroll 8
            for (int p = 0; p < rows; ++p) {
                const double x = sx[p], y = sy[p], z = sz[p];
#pragma unroll
                for (int j = 0; j < HPL; ++j) cnt[j] += fabs(pl_resid(a[j], b[j], c[j], d[j], x, y, z)) < md ? 1u : 0u;
            }
        }
#pragma unroll
        for (int j = 0; j < HPL; ++j)
            if (live[j] && cnt[j]) atomicAdd(inl + (hb * HPL + j) * PL_BLOCK + threadIdx.x, (int32_t)cnt[j]);
    }
    if (blockIdx.y == 0) {
        cand = wsum_u32(cand);
        if ((threadIdx.x & 63) == 0 && cand) atomicAdd(st + PL_CAND, (unsigned long long)cand);
    }
}

// st[POSE_BEST1] = max over the hypotheses of inliers + 1 (0: none is valid)
__global__ __launch_bounds__(POSE_BLOCK) void k_pl_max(const int32_t *__restrict__ inl, long h, unsigned long long *__restrict__ st)
{
    const long stride = (long)gridDim.x * POSE_BLOCK;
    unsigned long long best1 = 0;
    for (long k = (long)blockIdx.x * POSE_BLOCK + threadIdx.x; k < h; k += stride) {
        const unsigned long long v = inl[k] >= 0 ? (unsigned long long)inl[k] + 1 : 0ull;
        best1 = v > best1 ? v : best1;
    }
    best1 = wmax_u64(best1);
    if ((threadIdx.x & 63) == 0 && best1) atomicMax(st + POSE_BEST1, best1);
}

// ---- the refit (contract (Q)) ----
// a plane's state between the launches
struct PlState {
    double cur[4], best[4], c[3], s[6];                // the current plane, the best one, cur's centroid and centred sums
    long long done;                                // 0: rounds go on; 1: they are over; 2: the input plane was void
    long long best_cnt, in_cnt, n;                 // counts of best / of the input plane (-2: not scored yet; -1: there is none) / of cur
};
constexpr int PL_WORDS = sizeof(PlState) / sizeof(double);
static_assert(sizeof(PlState) % sizeof(double) == 0, "the states lie in a buffer of doubles");

__global__ __launch_bounds__(POSE_BLOCK) void k_pl_init(const double *__restrict__ planes_in, long b, PlState *__restrict__ st)
{
    const long k = (long)blockIdx.x * POSE_BLOCK + threadIdx.x;
    if (k >= b) return;
    PlState S;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        S.cur[j] = planes_in[4 * k + j];
        ok = ok && finite_f64(S.cur[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) S.best[j] = ok ? S.cur[j] : 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) S.c[j] = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) S.s[j] = 0.0;
    S.done = ok ? 0 : 2;
    S.best_cnt = -1;
    S.in_cnt = ok ? -2 : -1;
    S.n = 0;
    st[k] = S;
}

// First stage of a sweep over (spans of PT_SPAN rows) x (planes): every thread rebuilds the mask of its row from the plane and
// forms its T terms (PL_A: the coordinates, the spans' counts leave too; PL_B: the six centred products), +0.0 for a row outside
// the mask.  part: per plane T rows of nb doubles, span s's sums in column s; cnt (PL_A): per plane nb counts.
template <int T>
__global__ __launch_bounds__(PT_BLOCK) void k_pl_sweep(const double *__restrict__ X, const uint8_t *__restrict__ mask,
                                                       const PlState *__restrict__ st, long n, long b, long P, double md,
                                                       double *__restrict__ part, long nb, unsigned *__restrict__ cnt)
{
    __shared__ double node[PT_TILES * PT_WAVES][T];
    __shared__ unsigned found[PT_TILES * PT_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long base = (long)blockIdx.x * PT_SPAN;
    for (long k = blockIdx.y; k < b; k += gridDim.y) {
        const PlState *S = st + k;
        if (S->done) continue;                                         // (the same for the whole workgroup)
        const double pa = S->cur[0], pb = S->cur[1], pc = S->cur[2], pd = S->cur[3];
        const double cx = S->c[0], cy = S->c[1], cz = S->c[2];
#pragma unroll
        for (int t = 0; t < PT_TILES; ++t) {
            const long e = base + (long)t * PT_BLOCK + threadIdx.x;
            double v[T];
            bool in = false;
            if (e < n && (!mask || mask[e] != 0)) {
                const double x = X[3 * e], y = X[3 * e + 1], z = X[3 * e + 2];
                in = fabs(pl_resid(pa, pb, pc, pd, x, y, z)) < md;
                if constexpr (T == PL_A) {
                    v[0] = x; v[1] = y; v[2] = z;
                } else {
                    const double dx = x - cx, dy = y - cy, dz = z - cz;
                    v[0] = dx * dx; v[1] = dx * dy; v[2] = dx * dz; v[3] = dy * dy; v[4] = dy * dz; v[5] = dz * dz;
                }
            }
            if (!in) {
#pragma unroll
                for (int j = 0; j < T; ++j) v[j] = 0.0;
            }
            const unsigned long long hits = (unsigned long long)__ballot(in);
            pt_wave(v, e, P);
            if (lane == 0) {
#pragma unroll
                for (int j = 0; j < T; ++j) node[t * PT_WAVES + wave][j] = v[j];
                if (T == PL_A) found[t * PT_WAVES + wave] = (unsigned)__popcll((long long)hits);
            }
        }
        const double s = pt_nodes<PT_TILES * PT_WAVES>(node, base, P);   // (its barriers also fence `found`)
        if (threadIdx.x < T) part[((long)k * T + threadIdx.x) * nb + blockIdx.x] = s;
        if constexpr (T == PL_A) {
            if (threadIdx.x == T) {
                unsigned m = 0;
                for (int i = 0; i < PT_TILES * PT_WAVES; ++i) m += found[i];
                cnt[k * nb + blockIdx.x] = m;
            }
            __syncthreads();                                           // (`found` may be written again)
        }
    }
}

// Second stage of sweep A, one workgroup per plane: the tree over the nb partials (between part and part2), the counts as integers;
// then cur's count settles "keep the best", and the centroid is formed.  last: the scoring sweep behind the last round -- instead
// of the centroid the outputs and the record's counters.
__global__ __launch_bounds__(PT_FOLD) void k_pl_fold_a(PlState *__restrict__ st, double *part, double *part2, const unsigned *__restrict__ cnt,
                                                        long nb, long nb2, long b, int last, double *__restrict__ planes_out,
                                                        int32_t *__restrict__ inl_out, unsigned long long *__restrict__ counters)
{
    __shared__ double node[PT_FOLD_WAVES][PL_A];
    __shared__ unsigned long long total[PT_FOLD_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long k = blockIdx.x; k < b; k += gridDim.x) {
        PlState *S = st + k;
        const bool over = S->done != 0;                                // (read by every thread before thread 0 may change it)
        __syncthreads();
        if (over && !last) continue;
        double *a = part + k * PL_A * nb;
        long sa = nb;
        if (!over) {
            unsigned long long m = 0;
            for (long i = threadIdx.x; i < nb; i += PT_FOLD) m += cnt[k * nb + i];
            m = wsum_u64(m);
            if (lane == 0) total[wave] = m;
            pt_fold(a, sa, part2 + k * PL_A * nb2, nb2, nb, node);
        }
        if (threadIdx.x == 0) {
            if (!over) {
                long long m = 0;
                for (int w = 0; w < PT_FOLD_WAVES; ++w) m += (long long)total[w];
                S->n = m;
                if (S->in_cnt == -2) {
                    S->in_cnt = S->best_cnt = m;                       // (best is the input plane already)
                } else if (m > S->best_cnt) {
                    S->best_cnt = m;
#pragma unroll
                    for (int j = 0; j < 4; ++j) S->best[j] = S->cur[j];
                }
                if (!last) {
                    if (m < 3) {
                        S->done = 1;                                   // the round yields nothing
                    } else {
                        const double dm = (double)m;
#pragma unroll
                        for (int j = 0; j < 3; ++j) S->c[j] = a[(long)j * sa] / dm;
                    }
                }
            }
            if (last) {
                const long long bc = S->best_cnt;
#pragma unroll
                for (int j = 0; j < 4; ++j) planes_out[4 * k + j] = bc >= 0 ? S->best[j] : 0.0;
                inl_out[k] = (int32_t)bc;
                if (S->done == 2) atomicAdd(counters + POSE_VOID, 1ull);
                if (bc > S->in_cnt) atomicAdd(counters + PL_IMPROVED, 1ull);
                if (bc >= 0) atomicMax(counters + POSE_BEST1, (unsigned long long)bc + 1);
            }
        }
        __syncthreads();
    }
}

// Second stage of sweep B, one workgroup per plane: the tree; the six sums go into the plane's state.
__global__ __launch_bounds__(PT_FOLD) void k_pl_fold_b(PlState *__restrict__ st, double *part, double *part2, long nb, long nb2, long b)
{
    __shared__ double node[PT_FOLD_WAVES][PL_B];
    for (long k = blockIdx.x; k < b; k += gridDim.x) {
        PlState *S = st + k;
        if (S->done != 0) continue;                                    // (the same for the whole workgroup; nobody changes it here)
        double *a = part + k * PL_B * nb;
        long sa = nb;
        pt_fold(a, sa, part2 + k * PL_B * nb2, nb2, nb, node);
        if (threadIdx.x < PL_B) S->s[threadIdx.x] = a[(long)threadIdx.x * sa];
        __syncthreads();                                               // (the buffers may be written again)
    }
}

// One thread per plane behind sweep B: jacobi3 on the six sums and the next plane.  A plane that is not finite, or that repeats
// cur bit for bit, ends the rounds; any other becomes cur.  (A kernel of its own: 65 planes are 65 lanes here, not 65 workgroups
// with one lane at work each.)
__global__ __launch_bounds__(POSE_BLOCK) void k_pl_settle(PlState *__restrict__ st, long b)
{
    const long k = (long)blockIdx.x * POSE_BLOCK + threadIdx.x;
    if (k >= b) return;
    PlState *S = st + k;
    if (S->done != 0) return;
    double A[3][3], V[3][3];
    A[0][0] = S->s[0]; A[0][1] = S->s[1]; A[0][2] = S->s[2]; A[1][1] = S->s[3]; A[1][2] = S->s[4]; A[2][2] = S->s[5];
    A[1][0] = A[0][1]; A[2][0] = A[0][2]; A[2][1] = A[1][2];
    jacobi3(A, V);
    // the column of the smallest diagonal entry, the lowest on a tie (selects on scalars: indexed by the verdict, V would go to scratch)
    const double v00 = V[0][0], v01 = V[0][1], v02 = V[0][2], v10 = V[1][0], v11 = V[1][1], v12 = V[1][2], v20 = V[2][0], v21 = V[2][1],
                 v22 = V[2][2];
    const bool one = A[1][1] < A[0][0];
    const double w = one ? A[1][1] : A[0][0];
    const bool two = A[2][2] < w;
    double nx = two ? v02 : one ? v01 : v00, ny = two ? v12 : one ? v11 : v10, nz = two ? v22 : one ? v21 : v20;
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    nx = nx / len; ny = ny / len; nz = nz / len;
    const double cur[4] = {S->cur[0], S->cur[1], S->cur[2], S->cur[3]};
    if ((nx * cur[0] + ny * cur[1]) + nz * cur[2] < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
    const double o[4] = {nx, ny, nz, -((nx * S->c[0] + ny * S->c[1]) + nz * S->c[2])};
    bool ok = true, same = true;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        ok = ok && finite_f64(o[j]);
        same = same && __double_as_longlong(o[j]) == __double_as_longlong(cur[j]);
    }
    if (!ok || same) {
        S->done = 1;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) S->cur[j] = o[j];
    }
}

// keep[i] = row i is an inlier of the output plane of state 0 (all 0 for a void output)
__global__ __launch_bounds__(POSE_BLOCK) void k_pl_keep(const double *__restrict__ X, const uint8_t *__restrict__ mask,
                                                        const PlState *__restrict__ st, long n, double md, uint8_t *__restrict__ keep)
{
    const bool there = st->best_cnt >= 0;
    const double pa = st->best[0], pb = st->best[1], pc = st->best[2], pd = st->best[3];
    const long stride = (long)gridDim.x * POSE_BLOCK;
    for (long i = (long)blockIdx.x * POSE_BLOCK + threadIdx.x; i < n; i += stride) {
        bool in = false;
        if (there && (!mask || mask[i] != 0)) in = fabs(pl_resid(pa, pb, pc, pd, X[3 * i], X[3 * i + 1], X[3 * i + 2])) < md;
        keep[i] = in ? 1 : 0;
    }
}

}  // namespace
}  // namespace sicp

namespace {

// the checks both entries make, in their order; the rows and the mask as the kernels take them
int check_cloud_rows(const double *X, int64_t n)
{
    if (!X) return fail(SICP_ERR_INVALID, "X is null");
    if (n < 3) return fail(SICP_ERR_INVALID, "n must be >= 3 (%lld given)", (long long)n);
    if (n >= (1LL << 31)) return fail(SICP_ERR_INVALID, "n must be < 2^31 (%lld given)", (long long)n);
    return SICP_OK;
}

int cloud_rows_enter(sicp_ctx *c, const double *X, int64_t n, const uint8_t *mask, const double **x, const uint8_t **m)
{
    CHK(stage_in(c, X, (size_t)3 * n, c->gl_src, x));
    *m = nullptr;
    if (mask) CHK(stage_in(c, mask, (size_t)n, c->pl_mask, m));
    CHK(counters_clear(c));
    HIPCHK(hipMemsetAsync(c->cand_small.p + POSE_BEST, 0xff, sizeof(unsigned long long), c->stream));
    return SICP_OK;
}

// the record's shared fields, behind counters_fetch and sync
template <class Stats>
void best_fields(const sicp_ctx *c, Stats *out)
{
    const unsigned long long *hs = counters_host(c);
    out->n_void = (int64_t)hs[POSE_VOID];
    out->best = hs[POSE_BEST1] ? (int64_t)hs[POSE_BEST] : -1;
    out->best_inliers = (int64_t)hs[POSE_BEST1] - 1;
}

}  // namespace

SICP_EXPORT int sicp_plane_version(void) { return SICP_PLANE_VERSION; }

SICP_EXPORT int sicp_plane_triplets(sicp_ctx *c, const double *X, int64_t n, const uint8_t *mask, const int32_t *triples, int64_t h,
                                    double max_distance, double *planes_out, int32_t *inliers_out, sicp_plane_stats *out)
{
    CHK(check_rows_ctx(c, "sicp_plane_triplets"));
    CHK(check_cloud_rows(X, n));
    if (!triples) return fail(SICP_ERR_INVALID, "triples is null");
    if (!inliers_out) return fail(SICP_ERR_INVALID, "inliers_out is null");
    if (!out) return fail(SICP_ERR_INVALID, "out is null");
    if (h < 1) return fail(SICP_ERR_INVALID, "h must be >= 1 (%lld given)", (long long)h);
    if (h >= (1LL << 31)) return fail(SICP_ERR_INVALID, "h must be < 2^31 (%lld given)", (long long)h);
    CHK(check_max_distance(max_distance, false));
    HIPCHK(hipSetDevice(c->device));
    return op_run(c, [&]() -> int {
        const double *x;
        const uint8_t *m;
        const int32_t *tri;
        double *planes;
        int32_t *inl;
        CHK(cloud_rows_enter(c, X, n, mask, &x, &m));
        CHK(stage_in(c, triples, (size_t)3 * h, c->gl_tri, &tri));
        CHK(stage_out(c, planes_out, (size_t)4 * h, c->gl_pose, &planes));
        if (!planes) {                                                 // (the sweep reads them whether or not the caller does)
            CHK(c->pl_plane.reserve((size_t)4 * h));
            planes = c->pl_plane.p;
        }
        CHK(stage_out(c, inliers_out, (size_t)h, c->gl_idx, &inl));
        hipLaunchKernelGGL(k_pl_planes, dim3(cdiv((long)h, (long)POSE_BLOCK)), dim3(POSE_BLOCK), 0, c->stream, x, m, tri, planes, inl,
                           c->cand_small.p, (long)n, (long)h);
        HIPCHK(hipGetLastError());
        // two hypotheses per lane once a workgroup's 256 lanes do not hold them all: a row read from LDS serves both.  Rows per
        // workgroup: the ctx's switch, else whole tiles, as many spans as bring the grid to PL_FILL workgroups
        const int hpl = h > PL_BLOCK ? 2 : 1;
        const long gy = std::min<long>(cdiv((long)h, (long)PL_BLOCK * hpl), PL_MAX_HBLOCKS);
        const long want = std::max<long>(1, PL_FILL / gy);
        const long span = c->plane_span > 0 ? c->plane_span
                                            : std::min<long>(round_up(std::max<long>(1, ((long)n + want - 1) / want), PL_TILE), PL_MAX_SPAN);
        const dim3 grid(cdiv((long)n, span), (unsigned)gy);
        if (hpl == 2)
            hipLaunchKernelGGL(k_pl_score<2>, grid, dim3(PL_BLOCK), 0, c->stream, x, m, (const double *)planes, inl, c->cand_small.p, (long)n,
                               (long)h, span, max_distance);
        else
            hipLaunchKernelGGL(k_pl_score<1>, grid, dim3(PL_BLOCK), 0, c->stream, x, m, (const double *)planes, inl, c->cand_small.p, (long)n,
                               (long)h, span, max_distance);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_pl_max, dim3(std::min(cdiv((long)h, (long)POSE_BLOCK), (unsigned)POSE_BEST_BLOCKS)), dim3(POSE_BLOCK), 0, c->stream,
                           (const int32_t *)inl, (long)h, c->cand_small.p);
        HIPCHK(hipGetLastError());
        CHK(pose_best_enqueue(c, k_pose_best, inl, (long)h));
        CHK(counters_fetch(c));
        CHK(stage_leave(c, planes_out, (size_t)4 * h, planes));
        CHK(stage_leave(c, inliers_out, (size_t)h, inl));
        CHK(sync(c));
        best_fields(c, out);
        out->n_points = n;
        out->n_candidates = mask ? (int64_t)counters_host(c)[PL_CAND] : n;
        out->n_hypotheses = h;
        return SICP_OK;
    });
}

SICP_EXPORT int sicp_plane_refit(sicp_ctx *c, const double *X, int64_t n, const uint8_t *mask, const double *planes_in, int64_t b,
                                 double max_distance, int rounds, double *planes_out, int32_t *inliers_out, uint8_t *keep_out,
                                 sicp_plane_refit_stats *out)
{
    CHK(check_rows_ctx(c, "sicp_plane_refit"));
    CHK(check_cloud_rows(X, n));
    if (!planes_in) return fail(SICP_ERR_INVALID, "planes_in is null");
    if (!planes_out) return fail(SICP_ERR_INVALID, "planes_out is null");
    if (!inliers_out) return fail(SICP_ERR_INVALID, "inliers_out is null");
    if (!out) return fail(SICP_ERR_INVALID, "out is null");
    if (b < 1) return fail(SICP_ERR_INVALID, "b must be >= 1 (%lld given)", (long long)b);
    if (b >= (1LL << 31)) return fail(SICP_ERR_INVALID, "b must be < 2^31 (%lld given)", (long long)b);
    if (rounds < 1 || rounds > SICP_PLANE_MAX_ROUNDS)
        return fail(SICP_ERR_INVALID, "rounds must be >= 1 and <= %d (%d given)", SICP_PLANE_MAX_ROUNDS, rounds);
    CHK(check_max_distance(max_distance, false));
    if (keep_out && b != 1) return fail(SICP_ERR_INVALID, "keep_out is given: b must be 1 then (%lld given)", (long long)b);
    HIPCHK(hipSetDevice(c->device));
    return op_run(c, [&]() -> int {
        const double *x, *pin;
        const uint8_t *m;
        double *planes;
        int32_t *inl;
        uint8_t *keep;
        CHK(cloud_rows_enter(c, X, n, mask, &x, &m));
        CHK(stage_in(c, planes_in, (size_t)4 * b, c->pf_in, &pin));
        CHK(stage_out(c, planes_out, (size_t)4 * b, c->gl_pose, &planes));
        CHK(stage_out(c, inliers_out, (size_t)b, c->gl_idx, &inl));
        CHK(stage_out(c, keep_out, (size_t)n, c->pl_keep, &keep));
        const PoseGrids G = pose_grids((long)n, (long)b, PT_SPAN, PT_FOLD);
        CHK(c->pl_state.reserve((size_t)b * PL_WORDS));
        CHK(c->pf_part.reserve((size_t)b * PL_B * G.nb));
        CHK(c->pf_part2.reserve((size_t)b * PL_B * G.nb2));
        CHK(c->pf_cnt.reserve((size_t)b * G.nb));
        PlState *st = (PlState *)c->pl_state.p;
        hipLaunchKernelGGL(k_pl_init, G.poses, dim3(POSE_BLOCK), 0, c->stream, pin, (long)b, st);
        HIPCHK(hipGetLastError());
        for (int r = 0; r <= rounds; ++r) {                           // (the pass behind the last round only scores its plane)
            const int last = r == rounds;
            hipLaunchKernelGGL(k_pl_sweep<PL_A>, G.sweep, dim3(PT_BLOCK), 0, c->stream, x, m, (const PlState *)st, (long)n, (long)b, G.P,
                               max_distance, c->pf_part.p, G.nb, c->pf_cnt.p);
            hipLaunchKernelGGL(k_pl_fold_a, G.fold, dim3(PT_FOLD), 0, c->stream, st, c->pf_part.p, c->pf_part2.p, (const unsigned *)c->pf_cnt.p,
                               G.nb, G.nb2, (long)b, last, planes, inl, c->cand_small.p);
            if (!last) {
                hipLaunchKernelGGL(k_pl_sweep<PL_B>, G.sweep, dim3(PT_BLOCK), 0, c->stream, x, m, (const PlState *)st, (long)n, (long)b, G.P,
                                   max_distance, c->pf_part.p, G.nb, c->pf_cnt.p);
                hipLaunchKernelGGL(k_pl_fold_b, G.fold, dim3(PT_FOLD), 0, c->stream, st, c->pf_part.p, c->pf_part2.p, G.nb, G.nb2, (long)b);
                hipLaunchKernelGGL(k_pl_settle, G.poses, dim3(POSE_BLOCK), 0, c->stream, st, (long)b);
            }
            HIPCHK(hipGetLastError());
        }
        if (keep) {
            hipLaunchKernelGGL(k_pl_keep, dim3(std::min(cdiv((long)n, (long)POSE_BLOCK), 65536u)), dim3(POSE_BLOCK), 0, c->stream, x, m,
                               (const PlState *)st, (long)n, max_distance, keep);
            HIPCHK(hipGetLastError());
        }
        CHK(pose_best_enqueue(c, k_pose_best, inl, (long)b));
        CHK(counters_fetch(c));
        CHK(stage_leave(c, planes_out, (size_t)4 * b, planes));
        CHK(stage_leave(c, inliers_out, (size_t)b, inl));
        CHK(stage_leave(c, keep_out, (size_t)n, keep));
        CHK(sync(c));
        best_fields(c, out);
        out->n_planes = b;
        out->n_improved = (int64_t)counters_host(c)[PL_IMPROVED];
        return SICP_OK;
    });
}
