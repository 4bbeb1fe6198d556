// sicp_robust.hip -- robust poses of matched rows (include/simpleicp_hip_robust.h; contract (G)).
//
// Sweeps path (any m, any b): the frame is sicp_pose_dev.h's; this file holds what is the robust fit's own.  First stage
// (k_pose_sweep<RbTerms>): every thread rebuilds d2 and the weight of its row from the pose's state (one division and one
// multiplication behind the row's residual) -- no weight is stored anywhere --, forms its terms -- sweep A: the weight and the six
// weighted coordinates, sweep B: the nine weighted centred products.  Second stage (k_pose_fold<RbSettleA>, <RbSettleB>): one lane
// forms the centroids after sweep A (rb_settle_a), runs Horn's fit (sicp_horn.h) and the scale step after sweep B (rb_settle_b).
// The rounds are enqueued back to back; a pose whose rounds are over (RbState::done) costs its workgroups one load.  The automatic
// scale is one more first stage (k_rb_max) whose maximum is an integer atomicMax on the bit pattern.  Counts by ballot and
// popcount; the counts and the record's counters are integer atomics.
//
// One-launch path (m <= RB_ONE_MAX): one workgroup of RB_ONE lanes per pose runs the start, all rounds and the scoring in one
// launch (k_rb_one), through the same steps: rb_begin, rb_rows_max, rb_settle_scale, pose_tile, rb_settle_a, rb_settle_b,
// rb_rows_score, rb_leave.  It cuts the tree where the sweeps path cuts it -- 64 rows a wave, the waves of an aligned span of
// PT_SPAN rows through LDS (pt_wave, pt_nodes), the at most 16 span sums in pair order -- so its bits are the sweeps path's.
#include "sicp_pose_dev.h"
#include "sicp_horn.h"
#include "../../include/simpleicp_hip_robust.h"

namespace sicp {
namespace {

constexpr int RB_A = 7, RB_B = 9;                  // terms of sweep A (W | w p | w q) and of sweep B (K row-major)
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

// does row e count: six finite coordinates and a finite d2
__device__ __forceinline__ bool rb_counts(const double (&p)[3], const double (&q)[3], double d2)
{
    return finite_f64(p[0]) && finite_f64(p[1]) && finite_f64(p[2]) && finite_f64(q[0]) && finite_f64(q[1]) && finite_f64(q[2]) &&
           finite_f64(d2);
}

// a row's terms in a round (step 1), from a pose's state in global memory or in LDS (T = RB_A or RB_B)
template <int N, class S_ = RbState>
struct RbTerms {
    static constexpr int T = N;
    static constexpr bool COUNTS = false;
    using State = S_;
    double s, cp[3], cq[3];
    __device__ __forceinline__ RbTerms(const S_ &S, double) : s(S.s)
    {
#pragma unroll
        for (int j = 0; j < 3; ++j) { cp[j] = N == RB_B ? S.cp[j] : 0.0; cq[j] = N == RB_B ? S.cq[j] : 0.0; }
    }
    __device__ __forceinline__ bool operator()(const double (&p)[3], const double (&q)[3], double d2, double (&v)[N]) const
    {
        const double u = s / (s + d2);
        const double w = u * u;
        if constexpr (N == RB_A) {
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
        return rb_counts(p, q, d2);
    }
};

// step 0 for pose k, in global memory or in LDS: the start (the identity without poses_in), nothing settled yet; done = 2: void
template <class S>
__device__ __forceinline__ void rb_begin(S &st, const double *__restrict__ poses_in, long k)
{
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        st.cur[j] = poses_in ? poses_in[12 * k + j] : (j == 0 || j == 4 || j == 8 ? 1.0 : 0.0);
        ok = ok && finite_f64(st.cur[j]);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) st.cp[j] = st.cq[j] = 0.0;
    st.s = 0.0;
    st.mx = 0;
    st.n = 0;
    st.done = ok ? 0 : 2;
}

// the start's scale: from the maximum's word (start_scale 0: automatic) or as given, not below md2; no row counts: the pose is void
template <class S>
__device__ __forceinline__ void rb_settle_scale(S &st, double start_scale, double md2)
{
    double s = start_scale;
    if (start_scale == 0.0) {
        if (st.mx == 0) { st.done = 2; return; }
        s = 2.0 * __longlong_as_double((long long)(st.mx - 1));
    }
    st.s = s < md2 ? md2 : s;
}

// sweep A's sums -> the centroids, or the round yields nothing
template <class S>
__device__ __forceinline__ void rb_settle_a(S &st, const double *a)
{
    const double W = a[0];
    if (!(finite_f64(W) && W > 0.0)) { st.done = 1; return; }
#pragma unroll
    for (int j = 0; j < 3; ++j) { st.cp[j] = a[1 + j] / W; st.cq[j] = a[4 + j] / W; }
}

// sweep B's sums -> Horn's pose and the scale step (not below md2), or the round yields nothing
template <class S>
__device__ __forceinline__ void rb_settle_b(S &st, const double (&K)[RB_B], double md2, double divisor)
{
    double o[12];
    const double cp[3] = {st.cp[0], st.cp[1], st.cp[2]}, cq[3] = {st.cq[0], st.cq[1], st.cq[2]};
    if (!pf_pose(K, cp, cq, o)) { st.done = 1; return; }
#pragma unroll
    for (int j = 0; j < 12; ++j) st.cur[j] = o[j];
    const double s = st.s / divisor;
    st.s = s < md2 ? md2 : s;
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

// the rows lo + thread, + STEP, ... below hi under H: the largest d2 that counts as 1 + its bits (0: none), the wave's in every lane
template <int STEP>
__device__ __forceinline__ unsigned long long rb_rows_max(const double *__restrict__ src, const double *__restrict__ dst, const Xf &H, long lo,
                                                          long hi)
{
    unsigned long long mx = 0;
    for (long e = lo + threadIdx.x; e < hi; e += STEP) {
        double p[3], q[3];
        const double d2 = pose_row(src, dst, e, H, p, q);
        if (rb_counts(p, q, d2)) {
            const unsigned long long v = (unsigned long long)__double_as_longlong(d2) + 1;
            mx = v > mx ? v : mx;
        }
    }
    return wmax_u64(mx);
}

// ... those with d2 < md2 (the scoring pass): the wave's count in every lane
template <int STEP>
__device__ __forceinline__ unsigned rb_rows_score(const double *__restrict__ src, const double *__restrict__ dst, const Xf &H, long lo, long hi,
                                                  double md2)
{
    unsigned n = 0;
    for (long base = lo; base < hi; base += STEP) {                    // (as many steps in every lane: the ballot is the wave's)
        const long e = base + threadIdx.x;
        bool in = false;
        if (e < hi) {
            double p[3], q[3];
            in = pose_row(src, dst, e, H, p, q) < md2;
        }
        n += (unsigned)__popcll((unsigned long long)__ballot(in));
    }
    return n;
}

// what a pose leaves (step 2) and adds to the record's counters
__device__ __forceinline__ void rb_leave(long k, bool is_void, const double *cur, double s, unsigned long long n, double *__restrict__ poses_out,
                                         int32_t *__restrict__ inl_out, double *__restrict__ scales_out, unsigned long long *__restrict__ counters)
{
#pragma unroll
    for (int j = 0; j < 12; ++j) poses_out[12 * k + j] = is_void ? 0.0 : cur[j];
    inl_out[k] = is_void ? -1 : (int32_t)n;
    scales_out[k] = is_void ? 0.0 : s;
    if (is_void) atomicAdd(counters + POSE_VOID, 1ull);
    else atomicMax(counters + POSE_BEST1, n + 1);
}

// ---- the sweeps path ----
__global__ __launch_bounds__(POSE_BLOCK) void k_rb_init(const double *__restrict__ poses_in, long b, double start_scale, double md2,
                                                        RbState *__restrict__ st)
{
    const long k = (long)blockIdx.x * POSE_BLOCK + threadIdx.x;
    if (k >= b) return;
    RbState S;
    rb_begin(S, poses_in, k);
    if (start_scale != 0.0) rb_settle_scale(S, start_scale, md2);     // (automatic: s stays 0.0, read by nobody, until k_rb_auto
                                                                      // settles it behind k_rb_max)
    st[k] = S;
}

// the automatic scale, first stage: the largest d2 that counts under the start
__global__ __launch_bounds__(PT_BLOCK) void k_rb_max(const double *__restrict__ src, const double *__restrict__ dst, RbState *__restrict__ st,
                                                     long m, long b)
{
    const long base = (long)blockIdx.x * PT_SPAN, end = base + PT_SPAN < m ? base + PT_SPAN : m;
    for (long k = blockIdx.y; k < b; k += gridDim.y) {
        RbState *S = st + k;
        if (S->done) continue;
        const unsigned long long mx = rb_rows_max<PT_BLOCK>(src, dst, pose_xf(S->cur), base, end);
        if ((threadIdx.x & 63) == 0 && mx) atomicMax(&S->mx, mx);
    }
}

__global__ __launch_bounds__(POSE_BLOCK) void k_rb_auto(RbState *__restrict__ st, long b, double md2)
{
    const long k = (long)blockIdx.x * POSE_BLOCK + threadIdx.x;
    if (k >= b || st[k].done) return;
    rb_settle_scale(st[k], 0.0, md2);
}

// the second stages' settle steps (k_pose_fold)
struct RbSettleA {
    static constexpr int T = RB_A;
    using State = RbState;
    __device__ __forceinline__ void operator()(RbState &S, const double (&sums)[RB_A]) const { rb_settle_a(S, sums); }
};
struct RbSettleB {
    static constexpr int T = RB_B;
    using State = RbState;
    double md2, divisor;
    __device__ __forceinline__ void operator()(RbState &S, const double (&K)[RB_B]) const { rb_settle_b(S, K, md2, divisor); }
};

// the scoring pass: the rows with d2 < md2 under the latest pose
__global__ __launch_bounds__(PT_BLOCK) void k_rb_score(const double *__restrict__ src, const double *__restrict__ dst, RbState *__restrict__ st,
                                                       long m, long b, double md2)
{
    const long base = (long)blockIdx.x * PT_SPAN, end = base + PT_SPAN < m ? base + PT_SPAN : m;
    for (long k = blockIdx.y; k < b; k += gridDim.y) {
        RbState *S = st + k;
        if (S->done == 2) continue;
        const unsigned n = rb_rows_score<PT_BLOCK>(src, dst, pose_xf(S->cur), base, end, md2);
        if ((threadIdx.x & 63) == 0 && n) atomicAdd(&S->n, (unsigned long long)n);
    }
}

__global__ __launch_bounds__(POSE_BLOCK) void k_rb_finish(const RbState *__restrict__ st, long b, double *__restrict__ poses_out,
                                                          int32_t *__restrict__ inl_out, double *__restrict__ scales_out,
                                                          unsigned long long *__restrict__ counters)
{
    const long k = (long)blockIdx.x * POSE_BLOCK + threadIdx.x;
    if (k >= b) return;
    const RbState *S = st + k;
    rb_leave(k, S->done == 2, S->cur, S->s, S->n, poses_out, inl_out, scales_out, counters);
}

// ---- the one-launch path ----
// what the lanes of a workgroup share about their pose
struct RbOne {
    double cur[12], cp[3], cq[3], s;
    unsigned long long mx;
    unsigned n;
    int done;
};

// one sweep over the rows: span after span through pose_tile and pt_nodes (the first stage's cut), the span sums in pair order (the
// second stage's); thread j < T returns term j's sum.  Called by all threads; P2x64 = 64 x the next power of two >= nb.
template <int T>
__device__ __forceinline__ double rb_one_sweep(const double *__restrict__ src, const double *__restrict__ dst, long m, long P, int nb, long P2x64,
                                               const RbOne &S, double (*node)[T], double (*spn)[T])
{
    const int wave = threadIdx.x >> 6;
    const Xf H = pose_xf(S.cur);
    const RbTerms<T, RbOne> terms(S, 0.0);
    for (int sp = 0; sp < RB_ONE_SPANS; ++sp) {
        double sum = 0.0;
        if (sp < nb) {                                                 // (the same for the whole workgroup)
            const long base = (long)sp * PT_SPAN;
#pragma unroll 1
            for (int t = 0; t < RB_ONE_TILES; ++t)
                pose_tile<T>(src, dst, base + (long)t * RB_ONE + threadIdx.x, m, P, H, terms, node, t * RB_ONE_WAVES + wave);
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
        if (threadIdx.x == 0) rb_begin(S, poses_in, k);
        __syncthreads();
        if (S.done == 0) {                                             // (the same for the whole workgroup, here and below)
            if (start_scale == 0.0) {
                const unsigned long long mx = rb_rows_max<RB_ONE>(src, dst, pose_xf(S.cur), 0, m);
                if (lane == 0 && mx) atomicMax(&S.mx, mx);
                __syncthreads();
            }
            if (threadIdx.x == 0) rb_settle_scale(S, start_scale, md2);
            __syncthreads();
        }
        for (int r = 0; r < rounds && S.done == 0; ++r) {
            const double sa = rb_one_sweep<RB_A>(src, dst, m, P, nb, P2x64, S, node_a, spn_a);
            if (threadIdx.x < RB_A) tot[threadIdx.x] = sa;
            __syncthreads();
            if (threadIdx.x == 0) rb_settle_a(S, tot);
            __syncthreads();
            if (S.done) break;
            const double sb = rb_one_sweep<RB_B>(src, dst, m, P, nb, P2x64, S, node_b, spn_b);
            if (threadIdx.x < RB_B) tot[threadIdx.x] = sb;
            __syncthreads();
            if (threadIdx.x == 0) rb_settle_b(S, tot, md2, divisor);
            __syncthreads();
        }
        if (S.done != 2) {
            const unsigned n = rb_rows_score<RB_ONE>(src, dst, pose_xf(S.cur), 0, m, md2);
            if (lane == 0 && n) atomicAdd(&S.n, n);
            __syncthreads();
        }
        if (threadIdx.x == 0) rb_leave(k, S.done == 2, S.cur, S.s, (unsigned long long)S.n, poses_out, inl_out, scales_out, counters);
        __syncthreads();                                               // (S is written again)
    }
}

}  // namespace
}  // namespace sicp

SICP_EXPORT int sicp_robust_version(void) { return SICP_ROBUST_VERSION; }

SICP_EXPORT int sicp_pose_robust(sicp_ctx *c, const double *src, const double *dst, int64_t m, const double *poses_in, int64_t b,
                                 double max_distance, int rounds, double divisor, double start_scale, double *poses_out,
                                 int32_t *inliers_out, double *scales_out, sicp_robust_stats *out)
{
    CHK(check_rows_ctx(c, "sicp_pose_robust"));
    CHK(check_matched(src, dst));
    if (!poses_out) return fail(SICP_ERR_INVALID, "poses_out is null");
    if (!inliers_out) return fail(SICP_ERR_INVALID, "inliers_out is null");
    if (!scales_out) return fail(SICP_ERR_INVALID, "scales_out is null");
    if (!out) return fail(SICP_ERR_INVALID, "out is null");
    CHK(check_matched_count(m));
    CHK(check_poses_rounds(poses_in, b, rounds, SICP_ROBUST_MAX_ROUNDS));
    CHK(check_max_distance(max_distance, false));
    if (!std::isfinite(divisor) || !(divisor > 1.0)) return fail(SICP_ERR_INVALID, "divisor must be finite and > 1");
    if (!std::isfinite(start_scale) || start_scale < 0.0) return fail(SICP_ERR_INVALID, "start_scale must be finite and > 0, or 0 (automatic)");
    HIPCHK(hipSetDevice(c->device));
    return op_run(c, [&]() -> int {
        PoseRows R;
        double *scales;
        CHK(pose_rows_enter(c, src, dst, m, poses_in, b, poses_out, inliers_out, &R));
        CHK(stage_out(c, scales_out, (size_t)b, c->rb_scale, &scales));
        const PoseGrids G = pose_grids((long)m, (long)b, PT_SPAN, PT_FOLD);
        const double md2 = max_distance * max_distance;
        const bool fits = m <= RB_ONE_MAX;
        const bool one = fits && (c->robust_path == 2 || (c->robust_path == 0 && m <= RB_ONE_DEFAULT_MAX));
        if (one) {
            hipLaunchKernelGGL(k_rb_one, G.fold, dim3(RB_ONE), 0, c->stream, R.src, R.dst, R.poses_in, (long)m, (long)b, G.P, md2, rounds, divisor,
                               start_scale, R.poses, R.inl, scales, c->cand_small.p);
            HIPCHK(hipGetLastError());
        } else {
            CHK(c->rb_state.reserve((size_t)b * RB_WORDS));
            CHK(c->pf_part.reserve((size_t)b * RB_B * G.nb));
            CHK(c->pf_part2.reserve((size_t)b * RB_B * G.nb2));
            RbState *st = (RbState *)c->rb_state.p;
            hipLaunchKernelGGL(k_rb_init, G.poses, dim3(POSE_BLOCK), 0, c->stream, R.poses_in, (long)b, start_scale, md2, st);
            if (start_scale == 0.0) {
                hipLaunchKernelGGL(k_rb_max, G.sweep, dim3(PT_BLOCK), 0, c->stream, R.src, R.dst, st, (long)m, (long)b);
                hipLaunchKernelGGL(k_rb_auto, G.poses, dim3(POSE_BLOCK), 0, c->stream, st, (long)b, md2);
            }
            HIPCHK(hipGetLastError());
            for (int r = 0; r < rounds; ++r) {
                hipLaunchKernelGGL(k_pose_sweep<RbTerms<RB_A>>, G.sweep, dim3(PT_BLOCK), 0, c->stream, R.src, R.dst, st, (long)m, (long)b, G.P, md2,
                                   c->pf_part.p, G.nb, (unsigned *)nullptr);
                hipLaunchKernelGGL(k_pose_fold<RbSettleA>, G.fold, dim3(PT_FOLD), 0, c->stream, st, c->pf_part.p, c->pf_part2.p, G.nb, G.nb2,
                                   (long)b, RbSettleA{});
                hipLaunchKernelGGL(k_pose_sweep<RbTerms<RB_B>>, G.sweep, dim3(PT_BLOCK), 0, c->stream, R.src, R.dst, st, (long)m, (long)b, G.P, md2,
                                   c->pf_part.p, G.nb, (unsigned *)nullptr);
                hipLaunchKernelGGL(k_pose_fold<RbSettleB>, G.fold, dim3(PT_FOLD), 0, c->stream, st, c->pf_part.p, c->pf_part2.p, G.nb, G.nb2,
                                   (long)b, RbSettleB{md2, divisor});
                HIPCHK(hipGetLastError());
            }
            hipLaunchKernelGGL(k_rb_score, G.sweep, dim3(PT_BLOCK), 0, c->stream, R.src, R.dst, st, (long)m, (long)b, md2);
            hipLaunchKernelGGL(k_rb_finish, G.poses, dim3(POSE_BLOCK), 0, c->stream, st, (long)b, R.poses, R.inl, scales, c->cand_small.p);
            HIPCHK(hipGetLastError());
        }
        CHK(pose_best_enqueue(c, k_pose_best, R.inl, (long)b));
        CHK(stage_leave(c, scales_out, (size_t)b, scales));
        CHK(pose_rows_leave(c, poses_out, inliers_out, b, R, out));
        out->n_poses = b;
        return SICP_OK;
    });
}
