// sicp_robust.hip -- robust poses of matched rows (include/simpleicp_hip_robust.h; contract (G)).
//
// Sweeps path (any m, any b): the shape is sicp_posefit.hip's.  First stage (k_rb_sweep): the grid is (spans of PT_SPAN rows) x
// (poses); every thread rebuilds d2 and the weight of its row from the pose's state (contracts (T) and (D): nine fused
// multiply-adds, then one division and one multiplication) -- no weight is stored anywhere --, forms its terms -- sweep A: the
// weight and the six weighted coordinates, sweep B: the nine weighted centred products -- and the pair tree (sicp_pairtree.h) leaves
// one partial per term, span and pose.  Second stage (k_rb_fold_a, k_rb_fold_b): one workgroup per pose folds the partials; one
// lane forms the centroids after sweep A, runs Horn's fit (sicp_horn.h) and the scale step after sweep B.  The rounds are enqueued
// back to back; a pose whose rounds are over (RbState::done) costs its workgroups one load.  The automatic scale is one more first
// stage (k_rb_max) whose maximum is an integer atomicMax on the bit pattern.  Counts by ballot and popcount; the counts and the
// record's counters are integer atomics.
//
// One-launch path (m <= RB_ONE_MAX): one workgroup of RB_ONE lanes per pose runs the start, all rounds and the scoring in one
// launch (k_rb_one).  It cuts the tree where the sweeps path cuts it -- 64 rows a wave, the waves of an aligned span of PT_SPAN rows
// through LDS (pt_wave, pt_nodes), the at most 16 span sums in pair order -- so its bits are the sweeps path's.
#include "sicp_host.h"
#include "sicp_grid_dev.h"
#include "sicp_pairtree.h"
#include "sicp_horn.h"
#include "../../include/simpleicp_hip_robust.h"

namespace sicp {
namespace {

constexpr int RB_A = 7, RB_B = 9;                  // terms of sweep A (W | w p | w q) and of sweep B (K row-major)
constexpr int RB_MAX_POSES_Y = 32768;              // grid limit of the poses' dimension: the workgroups stride from there on
constexpr int RB_BLOCK = 256;
constexpr int RB_ONE = 512, RB_ONE_WAVES = RB_ONE / 64;    // the one-launch path's workgroup (256 registers a lane: Horn's fit spills at 128)
constexpr int RB_ONE_TILES = (int)(PT_SPAN / RB_ONE);      // ... and the steps in which it takes a span of the tree
constexpr int RB_ONE_SPANS = 16;                   // ... and the most spans it takes (a power of two)
constexpr long RB_ONE_MAX = RB_ONE_SPANS * PT_SPAN;
constexpr long RB_ONE_DEFAULT_MAX = PT_SPAN;       // ... and the most rows at which it is the default: one span (measured: faster at 400
                                                   // rows, slower at 4 096; DESIGN.md section 20 has the record)
static_assert(RB_ONE * RB_ONE_TILES == PT_SPAN && RB_ONE_WAVES * RB_ONE_TILES == PT_TILES * PT_WAVES,
              "the one-launch path cuts a span into the first stage's nodes");

// a pose's state between the launches.  Poses are R row-major, then t.
struct RbState {
    double cur[12], cp[3], cq[3], s;
    unsigned long long mx;                         // the automatic scale: 1 + the bits of the largest d2 that counts (0: no row does)
    long long done;                                // 0: rounds go on; 1: they are over; 2: the pose is void
    unsigned long long n;                          // the inliers of cur (the scoring pass)
};
constexpr int RB_WORDS = sizeof(RbState) / sizeof(double);
static_assert(sizeof(RbState) % sizeof(double) == 0, "the states lie in a buffer of doubles");

enum { RB_VOID = 0, RB_BEST1 = 2, RB_BEST = 3 };   // the counter words (st[RB_BEST1] = max of inliers + 1)

__device__ __forceinline__ Xf rb_xf(const double *pose)
{
    Xf H;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        H.m[4 * r] = pose[3 * r]; H.m[4 * r + 1] = pose[3 * r + 1]; H.m[4 * r + 2] = pose[3 * r + 2];
        H.m[4 * r + 3] = pose[9 + r];
    }
    return H;
}

// row e under the pose H: its coordinates, d2 (contracts (T) and (D)); true: the row counts
__device__ __forceinline__ bool rb_row(const double *__restrict__ src, const double *__restrict__ dst, long e, const Xf &H, double (&p)[3],
                                       double (&q)[3], double &d2)
{
#pragma unroll
    for (int i = 0; i < 3; ++i) { p[i] = src[3 * e + i]; q[i] = dst[3 * e + i]; }
    double X, Y, Z;
    xf(H, p[0], p[1], p[2], X, Y, Z);
    const double dx = X - q[0], dy = Y - q[1], dz = Z - q[2];
    d2 = fma(dz, dz, fma(dy, dy, dx * dx));
    return finite_f64(p[0]) && finite_f64(p[1]) && finite_f64(p[2]) && finite_f64(q[0]) && finite_f64(q[1]) && finite_f64(q[2]) &&
           finite_f64(d2);
}

// the T terms of row e in a round (step 1): +0.0 for a row that does not count or lies beyond m
template <int T>
__device__ __forceinline__ void rb_terms(const double *__restrict__ src, const double *__restrict__ dst, long e, long m, const Xf &H, double s,
                                         const double (&cp)[3], const double (&cq)[3], double (&v)[T])
{
    bool in = false;
    if (e < m) {
        double p[3], q[3], d2;
        in = rb_row(src, dst, e, H, p, q, d2);
        const double u = s / (s + d2);
        const double w = u * u;
        if constexpr (T == RB_A) {
            v[0] = w;
#pragma unroll
            for (int i = 0; i < 3; ++i) { v[1 + i] = w * p[i]; v[4 + i] = w * q[i]; }
        } else {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double a = w * (p[i] - cp[i]);
#pragma unroll
                for (int j = 0; j < 3; ++j) v[3 * i + j] = a * (q[j] - cq[j]);
            }
        }
    }
    if (!in) {
#pragma unroll
        for (int j = 0; j < T; ++j) v[j] = 0.0;
    }
}

// the start of step 0 for a thread's pose; false: void
__device__ __forceinline__ bool rb_start(const double *__restrict__ poses_in, long k, double (&cur)[12])
{
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        cur[j] = poses_in ? poses_in[12 * k + j] : (j == 0 || j == 4 || j == 8 ? 1.0 : 0.0);
        ok = ok && finite_f64(cur[j]);
    }
    return ok;
}

// s from the maximum's word (automatic) or as given, not below md2; false: no row counts
__device__ __forceinline__ bool rb_scale(unsigned long long mx, double start_scale, double md2, double &s)
{
    if (start_scale == 0.0) {
        if (mx == 0) return false;
        s = 2.0 * __longlong_as_double((long long)(mx - 1));
    } else {
        s = start_scale;
    }
    if (s < md2) s = md2;
    return true;
}

// sweep A's sums -> the centroids; false: the round yields nothing
__device__ __forceinline__ bool rb_centroids(const double (&a)[RB_A], double (&cp)[3], double (&cq)[3])
{
    const double W = a[0];
    if (!(finite_f64(W) && W > 0.0)) return false;
#pragma unroll
    for (int j = 0; j < 3; ++j) { cp[j] = a[1 + j] / W; cq[j] = a[4 + j] / W; }
    return true;
}

__device__ __forceinline__ unsigned long long wmax_u64(unsigned long long v)
{
    unsigned long long o;
    o = lane_xor64<32>(v); v = o > v ? o : v;
    o = lane_xor64<16>(v); v = o > v ? o : v;
    o = lane_xor64<8>(v);  v = o > v ? o : v;
    o = lane_xor64<4>(v);  v = o > v ? o : v;
    o = lane_xor64<2>(v);  v = o > v ? o : v;
    o = lane_xor64<1>(v);  v = o > v ? o : v;
    return v;
}

// what a pose leaves (step 2) and adds to the record's counters
__device__ __forceinline__ void rb_leave(long k, bool is_void, const double *cur, double s, unsigned long long n, double *__restrict__ poses_out,
                                         int32_t *__restrict__ inl_out, double *__restrict__ scales_out, unsigned long long *__restrict__ counters)
{
#pragma unroll
    for (int j = 0; j < 12; ++j) poses_out[12 * k + j] = is_void ? 0.0 : cur[j];
    inl_out[k] = is_void ? -1 : (int32_t)n;
    scales_out[k] = is_void ? 0.0 : s;
    if (is_void) atomicAdd(counters + RB_VOID, 1ull);
    else atomicMax(counters + RB_BEST1, n + 1);
}

// ---- the sweeps path ----
__global__ __launch_bounds__(RB_BLOCK) void k_rb_init(const double *__restrict__ poses_in, long b, double start_scale, double md2,
                                                      RbState *__restrict__ st)
{
    const long k = (long)blockIdx.x * RB_BLOCK + threadIdx.x;
    if (k >= b) return;
    RbState S;
    const bool ok = rb_start(poses_in, k, S.cur);
#pragma unroll
    for (int j = 0; j < 3; ++j) S.cp[j] = S.cq[j] = 0.0;
    S.s = start_scale < md2 ? md2 : start_scale;                      // (automatic: k_rb_auto sets it)
    S.mx = 0;
    S.done = ok ? 0 : 2;
    S.n = 0;
    st[k] = S;
}

// the automatic scale, first stage: the largest d2 that counts under the start, as 1 + its bits
__global__ __launch_bounds__(PT_BLOCK) void k_rb_max(const double *__restrict__ src, const double *__restrict__ dst, RbState *__restrict__ st,
                                                     long m, long b)
{
    const int lane = threadIdx.x & 63;
    const long base = (long)blockIdx.x * PT_SPAN;
    for (long k = blockIdx.y; k < b; k += gridDim.y) {
        RbState *S = st + k;
        if (S->done) continue;
        const Xf H = rb_xf(S->cur);
        unsigned long long mx = 0;
#pragma unroll
        for (int t = 0; t < PT_TILES; ++t) {
            const long e = base + (long)t * PT_BLOCK + threadIdx.x;
            if (e < m) {
                double p[3], q[3], d2;
                if (rb_row(src, dst, e, H, p, q, d2)) {
                    const unsigned long long v = (unsigned long long)__double_as_longlong(d2) + 1;
                    mx = v > mx ? v : mx;
                }
            }
        }
        mx = wmax_u64(mx);
        if (lane == 0 && mx) atomicMax(&S->mx, mx);
    }
}

__global__ __launch_bounds__(RB_BLOCK) void k_rb_auto(RbState *__restrict__ st, long b, double md2)
{
    const long k = (long)blockIdx.x * RB_BLOCK + threadIdx.x;
    if (k >= b || st[k].done) return;
    double s;
    if (rb_scale(st[k].mx, 0.0, md2, s)) st[k].s = s;
    else st[k].done = 2;
}

// First stage of a round.  part: per pose T rows of nb doubles, span s's sums in column s.
template <int T>
__global__ __launch_bounds__(PT_BLOCK) void k_rb_sweep(const double *__restrict__ src, const double *__restrict__ dst,
                                                       const RbState *__restrict__ st, long m, long b, long P, double *__restrict__ part, long nb)
{
    __shared__ double node[PT_TILES * PT_WAVES][T];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long base = (long)blockIdx.x * PT_SPAN;
    for (long k = blockIdx.y; k < b; k += gridDim.y) {
        const RbState *S = st + k;
        if (S->done) continue;                                         // (the same for the whole workgroup)
        const Xf H = rb_xf(S->cur);
        const double s = S->s;
        double cp[3] = {0.0, 0.0, 0.0}, cq[3] = {0.0, 0.0, 0.0};
        if constexpr (T == RB_B) {
#pragma unroll
            for (int j = 0; j < 3; ++j) { cp[j] = S->cp[j]; cq[j] = S->cq[j]; }
        }
#pragma unroll
        for (int t = 0; t < PT_TILES; ++t) {
            const long e = base + (long)t * PT_BLOCK + threadIdx.x;
            double v[T];
            rb_terms<T>(src, dst, e, m, H, s, cp, cq, v);
            pt_wave(v, e, P);
            if (lane == 0) {
#pragma unroll
                for (int j = 0; j < T; ++j) node[t * PT_WAVES + wave][j] = v[j];
            }
        }
        const double sum = pt_nodes<PT_TILES * PT_WAVES>(node, base, P);
        if (threadIdx.x < T) part[((long)k * T + threadIdx.x) * nb + blockIdx.x] = sum;
    }
}

// Second stage of sweep A, one workgroup per pose: the tree over the nb partials (between part and part2), then the centroids.
__global__ __launch_bounds__(PT_FOLD) void k_rb_fold_a(RbState *__restrict__ st, double *part, double *part2, long nb, long nb2, long b)
{
    __shared__ double node[PT_FOLD_WAVES][RB_A];
    for (long k = blockIdx.x; k < b; k += gridDim.x) {
        RbState *S = st + k;
        const bool over = S->done != 0;                                // (read by every thread before thread 0 may change it)
        __syncthreads();
        if (over) continue;
        double *a = part + k * RB_A * nb;
        long sa = nb;
        pt_fold(a, sa, part2 + k * RB_A * nb2, nb2, nb, node);
        if (threadIdx.x == 0) {
            double sums[RB_A], cp[3], cq[3];
#pragma unroll
            for (int j = 0; j < RB_A; ++j) sums[j] = a[(long)j * sa];
            if (!rb_centroids(sums, cp, cq)) {
                S->done = 1;                                           // the round yields nothing
            } else {
#pragma unroll
                for (int j = 0; j < 3; ++j) { S->cp[j] = cp[j]; S->cq[j] = cq[j]; }
            }
        }
        __syncthreads();
    }
}

// Second stage of sweep B: the nine sums, then one lane runs Horn's fit and the scale step.
__global__ __launch_bounds__(PT_FOLD) void k_rb_fold_b(RbState *__restrict__ st, double *part, double *part2, long nb, long nb2, long b,
                                                        double md2, double divisor)
{
    __shared__ double node[PT_FOLD_WAVES][RB_B];
    for (long k = blockIdx.x; k < b; k += gridDim.x) {
        RbState *S = st + k;
        const bool over = S->done != 0;
        __syncthreads();
        if (over) continue;
        double *a = part + k * RB_B * nb;
        long sa = nb;
        pt_fold(a, sa, part2 + k * RB_B * nb2, nb2, nb, node);
        if (threadIdx.x == 0) {
            double K[9], o[12];
#pragma unroll
            for (int j = 0; j < 9; ++j) K[j] = a[(long)j * sa];
            const double cp[3] = {S->cp[0], S->cp[1], S->cp[2]}, cq[3] = {S->cq[0], S->cq[1], S->cq[2]};
            if (!pf_pose(K, cp, cq, o)) {
                S->done = 1;
            } else {
#pragma unroll
                for (int j = 0; j < 12; ++j) S->cur[j] = o[j];
                double s = S->s / divisor;
                if (s < md2) s = md2;
                S->s = s;
            }
        }
        __syncthreads();
    }
}

// the scoring pass: the rows with d2 < md2 under the latest pose
__global__ __launch_bounds__(PT_BLOCK) void k_rb_score(const double *__restrict__ src, const double *__restrict__ dst, RbState *__restrict__ st,
                                                       long m, long b, double md2)
{
    const int lane = threadIdx.x & 63;
    const long base = (long)blockIdx.x * PT_SPAN;
    for (long k = blockIdx.y; k < b; k += gridDim.y) {
        RbState *S = st + k;
        if (S->done == 2) continue;
        const Xf H = rb_xf(S->cur);
        unsigned n = 0;
#pragma unroll
        for (int t = 0; t < PT_TILES; ++t) {
            const long e = base + (long)t * PT_BLOCK + threadIdx.x;
            bool in = false;
            if (e < m) {
                double p[3], q[3], d2;
                rb_row(src, dst, e, H, p, q, d2);
                in = d2 < md2;
            }
            n += (unsigned)__popcll((unsigned long long)__ballot(in));
        }
        if (lane == 0 && n) atomicAdd(&S->n, (unsigned long long)n);
    }
}

__global__ __launch_bounds__(RB_BLOCK) void k_rb_finish(const RbState *__restrict__ st, long b, double *__restrict__ poses_out,
                                                        int32_t *__restrict__ inl_out, double *__restrict__ scales_out,
                                                        unsigned long long *__restrict__ counters)
{
    const long k = (long)blockIdx.x * RB_BLOCK + threadIdx.x;
    if (k >= b) return;
    const RbState *S = st + k;
    rb_leave(k, S->done == 2, S->cur, S->s, S->n, poses_out, inl_out, scales_out, counters);
}

// st[RB_BEST] (all ones before) = the lowest k whose inliers + 1 == st[RB_BEST1]
__global__ __launch_bounds__(RB_BLOCK) void k_rb_best(const int32_t *__restrict__ inl, long b, unsigned long long *__restrict__ st)
{
    const unsigned long long best1 = st[RB_BEST1];
    if (best1 == 0) return;
    const int lane = threadIdx.x & 63;
    const long stride = (long)gridDim.x * RB_BLOCK;
    for (long base = (long)blockIdx.x * RB_BLOCK; base < b; base += stride) {
        const long k = base + threadIdx.x;
        const bool is = k < b && inl[k] >= 0 && (unsigned long long)inl[k] + 1 == best1;
        const unsigned long long who = (unsigned long long)__ballot(is);
        if (who && lane == __ffsll((long long)who) - 1) atomicMin(st + RB_BEST, (unsigned long long)k);
    }
}

// ---- the one-launch path ----
// what the lanes of a workgroup share about their pose
struct RbOne {
    double cur[12], cp[3], cq[3], s;
    unsigned long long mx;
    unsigned n;
    int done;
};

// one sweep over the rows: span after span through pt_wave and pt_nodes (the first stage's cut), the span sums in pair order (the
// second stage's); thread j < T returns term j's sum.  Called by all threads; P2x64 = 64 x the next power of two >= nb.
template <int T>
__device__ __forceinline__ double rb_one_sweep(const double *__restrict__ src, const double *__restrict__ dst, long m, long P, int nb, long P2x64,
                                               const RbOne &S, double (*node)[T], double (*spn)[T])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Xf H = rb_xf(S.cur);
    const double s = S.s;
    const double cp[3] = {S.cp[0], S.cp[1], S.cp[2]}, cq[3] = {S.cq[0], S.cq[1], S.cq[2]};
    for (int sp = 0; sp < RB_ONE_SPANS; ++sp) {
        double sum = 0.0;
        if (sp < nb) {                                                 // (the same for the whole workgroup)
            const long base = (long)sp * PT_SPAN;
#pragma unroll 1
            for (int t = 0; t < RB_ONE_TILES; ++t) {
                const long e = base + (long)t * RB_ONE + threadIdx.x;
                double v[T];
                rb_terms<T>(src, dst, e, m, H, s, cp, cq, v);
                pt_wave(v, e, P);
                if (lane == 0) {
#pragma unroll
                    for (int j = 0; j < T; ++j) node[t * RB_ONE_WAVES + wave][j] = v[j];
                }
            }
            sum = pt_nodes<RB_ONE_TILES * RB_ONE_WAVES>(node, base, P);
        }
        if (threadIdx.x < T) spn[sp][threadIdx.x] = sum;              // (beyond nb: the tree's padding)
    }
    return pt_nodes<RB_ONE_SPANS>(spn, 0, P2x64);
}

__global__ __launch_bounds__(RB_ONE) void k_rb_one(const double *__restrict__ src, const double *__restrict__ dst,
                                                   const double *__restrict__ poses_in, long m, long b, long P, double md2, int rounds,
                                                   double divisor, double start_scale, double *__restrict__ poses_out,
                                                   int32_t *__restrict__ inl_out, double *__restrict__ scales_out,
                                                   unsigned long long *__restrict__ counters)
{
    __shared__ double node_a[RB_ONE_TILES * RB_ONE_WAVES][RB_A], spn_a[RB_ONE_SPANS][RB_A];
    __shared__ double node_b[RB_ONE_TILES * RB_ONE_WAVES][RB_B], spn_b[RB_ONE_SPANS][RB_B];
    __shared__ double tot[RB_B];
    __shared__ RbOne S;
    const int lane = threadIdx.x & 63;
    const int nb = (int)((m + PT_SPAN - 1) / PT_SPAN);
    long P2x64 = 64;
    while (P2x64 < 64L * nb) P2x64 *= 2;
    for (long k = blockIdx.x; k < b; k += gridDim.x) {
        if (threadIdx.x == 0) {
            S.done = rb_start(poses_in, k, S.cur) ? 0 : 2;
#pragma unroll
            for (int j = 0; j < 3; ++j) S.cp[j] = S.cq[j] = 0.0;
            S.s = 0.0;
            S.mx = 0;
            S.n = 0;
        }
        __syncthreads();
        if (S.done == 0) {                                             // (the same for the whole workgroup, here and below)
            if (start_scale == 0.0) {
                const Xf H = rb_xf(S.cur);
                unsigned long long mx = 0;
                for (long e = threadIdx.x; e < m; e += RB_ONE) {
                    double p[3], q[3], d2;
                    if (rb_row(src, dst, e, H, p, q, d2)) {
                        const unsigned long long v = (unsigned long long)__double_as_longlong(d2) + 1;
                        mx = v > mx ? v : mx;
                    }
                }
                mx = wmax_u64(mx);
                if (lane == 0 && mx) atomicMax(&S.mx, mx);
                __syncthreads();
            }
            if (threadIdx.x == 0) {
                double s;
                if (rb_scale(S.mx, start_scale, md2, s)) S.s = s;
                else S.done = 2;
            }
            __syncthreads();
        }
        for (int r = 0; r < rounds && S.done == 0; ++r) {
            const double sa = rb_one_sweep<RB_A>(src, dst, m, P, nb, P2x64, S, node_a, spn_a);
            if (threadIdx.x < RB_A) tot[threadIdx.x] = sa;
            __syncthreads();
            if (threadIdx.x == 0) {
                double sums[RB_A], cp[3], cq[3];
#pragma unroll
                for (int j = 0; j < RB_A; ++j) sums[j] = tot[j];
                if (!rb_centroids(sums, cp, cq)) {
                    S.done = 1;
                } else {
#pragma unroll
                    for (int j = 0; j < 3; ++j) { S.cp[j] = cp[j]; S.cq[j] = cq[j]; }
                }
            }
            __syncthreads();
            if (S.done) break;
            const double sb = rb_one_sweep<RB_B>(src, dst, m, P, nb, P2x64, S, node_b, spn_b);
            if (threadIdx.x < RB_B) tot[threadIdx.x] = sb;
            __syncthreads();
            if (threadIdx.x == 0) {
                double K[9], o[12];
#pragma unroll
                for (int j = 0; j < 9; ++j) K[j] = tot[j];
                const double cp[3] = {S.cp[0], S.cp[1], S.cp[2]}, cq[3] = {S.cq[0], S.cq[1], S.cq[2]};
                if (!pf_pose(K, cp, cq, o)) {
                    S.done = 1;
                } else {
#pragma unroll
                    for (int j = 0; j < 12; ++j) S.cur[j] = o[j];
                    double s = S.s / divisor;
                    if (s < md2) s = md2;
                    S.s = s;
                }
            }
            __syncthreads();
        }
        if (S.done != 2) {
            const Xf H = rb_xf(S.cur);
            unsigned n = 0;
            for (long base = 0; base < m; base += RB_ONE) {
                const long e = base + threadIdx.x;
                bool in = false;
                if (e < m) {
                    double p[3], q[3], d2;
                    rb_row(src, dst, e, H, p, q, d2);
                    in = d2 < md2;
                }
                n += (unsigned)__popcll((unsigned long long)__ballot(in));
            }
            if (lane == 0 && n) atomicAdd(&S.n, n);
            __syncthreads();
        }
        if (threadIdx.x == 0) rb_leave(k, S.done == 2, S.cur, S.s, (unsigned long long)S.n, poses_out, inl_out, scales_out, counters);
        __syncthreads();                                               // (S is written again)
    }
}

}  // namespace
}  // namespace sicp

namespace {
static_assert(RB_BEST < CAND_WORDS && RB_BEST != CAND_COUNT && RB_BEST1 != CAND_COUNT, "the record's counters fit the ctx's counter words");
}

SICP_EXPORT int sicp_robust_version(void) { return SICP_ROBUST_VERSION; }

SICP_EXPORT int sicp_pose_robust(sicp_ctx *c, const double *src, const double *dst, int64_t m, const double *poses_in, int64_t b,
                                 double max_distance, int rounds, double divisor, double start_scale, double *poses_out,
                                 int32_t *inliers_out, double *scales_out, sicp_robust_stats *out)
{
    if (!c) return fail(SICP_ERR_INVALID, "null ctx");
    CHK(check_no_exchange(c, "sicp_pose_robust", "the rows of one rank are not the job's"));
    if (!src) return fail(SICP_ERR_INVALID, "src is null");
    if (!dst) return fail(SICP_ERR_INVALID, "dst is null");
    if (!poses_out) return fail(SICP_ERR_INVALID, "poses_out is null");
    if (!inliers_out) return fail(SICP_ERR_INVALID, "inliers_out is null");
    if (!scales_out) return fail(SICP_ERR_INVALID, "scales_out is null");
    if (!out) return fail(SICP_ERR_INVALID, "out is null");
    if (m < 3) return fail(SICP_ERR_INVALID, "m must be >= 3 (%lld given)", (long long)m);
    if (m >= (1LL << 31)) return fail(SICP_ERR_INVALID, "m must be < 2^31 (%lld given)", (long long)m);
    if (b < 1) return fail(SICP_ERR_INVALID, "b must be >= 1 (%lld given)", (long long)b);
    if (b >= (1LL << 31)) return fail(SICP_ERR_INVALID, "b must be < 2^31 (%lld given)", (long long)b);
    if (!poses_in && b != 1) return fail(SICP_ERR_INVALID, "poses_in is null: b must be 1 then (%lld given)", (long long)b);
    if (rounds < 1 || rounds > SICP_ROBUST_MAX_ROUNDS)
        return fail(SICP_ERR_INVALID, "rounds must be >= 1 and <= %d (%d given)", SICP_ROBUST_MAX_ROUNDS, rounds);
    if (!std::isfinite(max_distance) || !(max_distance > 0.0)) return fail(SICP_ERR_INVALID, "max_distance must be finite and > 0");
    if (!std::isfinite(divisor) || !(divisor > 1.0)) return fail(SICP_ERR_INVALID, "divisor must be finite and > 1");
    if (!std::isfinite(start_scale) || start_scale < 0.0) return fail(SICP_ERR_INVALID, "start_scale must be finite and > 0, or 0 (automatic)");
    HIPCHK(hipSetDevice(c->device));
    return op_run(c, [&]() -> int {
        const double *s, *d, *pin = nullptr;
        double *poses, *scales;
        int32_t *inl;
        CHK(stage_in(c, src, (size_t)3 * m, c->gl_src, &s));
        CHK(stage_in(c, dst, (size_t)3 * m, c->gl_dst, &d));
        if (poses_in) CHK(stage_in(c, poses_in, (size_t)12 * b, c->pf_in, &pin));
        CHK(stage_out(c, poses_out, (size_t)12 * b, c->gl_pose, &poses));
        CHK(stage_out(c, inliers_out, (size_t)b, c->gl_idx, &inl));
        CHK(stage_out(c, scales_out, (size_t)b, c->rb_scale, &scales));
        CHK(counters_clear(c));
        HIPCHK(hipMemsetAsync(c->cand_small.p + RB_BEST, 0xff, sizeof(unsigned long long), c->stream));
        long P = 1;
        while (P < m) P *= 2;
        const double md2 = max_distance * max_distance;
        const bool fits = m <= RB_ONE_MAX;
        const bool one = fits && (c->robust_path == 2 || (c->robust_path == 0 && m <= RB_ONE_DEFAULT_MAX));
        if (one) {
            hipLaunchKernelGGL(k_rb_one, dim3((unsigned)std::min<long>(b, RB_MAX_POSES_Y)), dim3(RB_ONE), 0, c->stream, s, d, pin, (long)m,
                               (long)b, P, md2, rounds, divisor, start_scale, poses, inl, scales, c->cand_small.p);
            HIPCHK(hipGetLastError());
        } else {
            const long nb = cdiv((long)m, PT_SPAN), nb2 = cdiv(nb, (long)PT_FOLD);
            CHK(c->rb_state.reserve((size_t)b * RB_WORDS));
            CHK(c->pf_part.reserve((size_t)b * RB_B * nb));
            CHK(c->pf_part2.reserve((size_t)b * RB_B * nb2));
            RbState *st = (RbState *)c->rb_state.p;
            const dim3 sweep_grid((unsigned)nb, (unsigned)std::min<long>(b, RB_MAX_POSES_Y));
            const dim3 fold_grid((unsigned)std::min<long>(b, RB_MAX_POSES_Y));
            const dim3 pose_grid((unsigned)cdiv((long)b, (long)RB_BLOCK));
            hipLaunchKernelGGL(k_rb_init, pose_grid, dim3(RB_BLOCK), 0, c->stream, pin, (long)b, start_scale, md2, st);
            if (start_scale == 0.0) {
                hipLaunchKernelGGL(k_rb_max, sweep_grid, dim3(PT_BLOCK), 0, c->stream, s, d, st, (long)m, (long)b);
                hipLaunchKernelGGL(k_rb_auto, pose_grid, dim3(RB_BLOCK), 0, c->stream, st, (long)b, md2);
            }
            HIPCHK(hipGetLastError());
            for (int r = 0; r < rounds; ++r) {
                hipLaunchKernelGGL(k_rb_sweep<RB_A>, sweep_grid, dim3(PT_BLOCK), 0, c->stream, s, d, st, (long)m, (long)b, P, c->pf_part.p, nb);
                hipLaunchKernelGGL(k_rb_fold_a, fold_grid, dim3(PT_FOLD), 0, c->stream, st, c->pf_part.p, c->pf_part2.p, nb, nb2, (long)b);
                hipLaunchKernelGGL(k_rb_sweep<RB_B>, sweep_grid, dim3(PT_BLOCK), 0, c->stream, s, d, st, (long)m, (long)b, P, c->pf_part.p, nb);
                hipLaunchKernelGGL(k_rb_fold_b, fold_grid, dim3(PT_FOLD), 0, c->stream, st, c->pf_part.p, c->pf_part2.p, nb, nb2, (long)b, md2,
                                   divisor);
                HIPCHK(hipGetLastError());
            }
            hipLaunchKernelGGL(k_rb_score, sweep_grid, dim3(PT_BLOCK), 0, c->stream, s, d, st, (long)m, (long)b, md2);
            hipLaunchKernelGGL(k_rb_finish, pose_grid, dim3(RB_BLOCK), 0, c->stream, st, (long)b, poses, inl, scales, c->cand_small.p);
            HIPCHK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_rb_best, dim3((unsigned)std::min<long>(cdiv((long)b, (long)RB_BLOCK), 1024)), dim3(RB_BLOCK), 0, c->stream, inl,
                           (long)b, c->cand_small.p);
        HIPCHK(hipGetLastError());
        CHK(counters_fetch(c));
        CHK(stage_leave(c, poses_out, (size_t)12 * b, poses));
        CHK(stage_leave(c, inliers_out, (size_t)b, inl));
        CHK(stage_leave(c, scales_out, (size_t)b, scales));
        CHK(sync(c));
        const unsigned long long *hs = counters_host(c);
        out->n_poses = b;
        out->n_void = (int64_t)hs[RB_VOID];
        out->best = hs[RB_BEST1] ? (int64_t)hs[RB_BEST] : -1;
        out->best_inliers = (int64_t)hs[RB_BEST1] - 1;
        return SICP_OK;
    });
}
