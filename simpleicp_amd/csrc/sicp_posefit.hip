// sicp_posefit.hip -- least-squares poses of matched rows (include/simpleicp_hip_posefit.h; contract (L)).
//
// The frame is sicp_pose_dev.h's, once per sweep of the contract: this file holds what is the refit's own.  First stage
// (k_pose_sweep<PfTerms>): every thread rebuilds the mask of its row from the pose and forms its terms -- sweep A: the six
// coordinates and the count, sweep B: the nine centred products.  Second stage: after sweep A (k_pf_fold_a, which also folds the
// counts and, behind the last round, writes the outputs: more than the frame's one settle step, so it keeps its own loop) one
// lane settles "keep the best" with the count the sweep carried and forms the centroids, after sweep B (k_pose_fold<PfSettleB>)
// it runs the 4 x 4 Jacobi (sicp_horn.h) and writes the next pose into the pose's state.  The rounds are enqueued back to back; a
// pose whose rounds are over (PfState::done) costs its workgroups one load.  The record's counters are integer atomics.
#include "sicp_pose_dev.h"
#include "sicp_horn.h"
#include "../../include/simpleicp_hip_posefit.h"

namespace sicp {
namespace {

constexpr int PF_A = 6, PF_B = 9;                  // terms of sweep A (p | q) and of sweep B (K row-major)

// a pose's state between the launches.  Poses are R row-major, then t.
struct PfState {
    double cur[12], best[12], cp[3], cq[3];
    long long done;                                // 0: rounds go on; 1: they are over; 2: the input pose was void
    long long plain;                               // 1: no pose yet -- the mask is "six finite coordinates" (a NULL start's first round)
    long long best_cnt, in_cnt, n;                 // counts of best / of the input pose (-2: not scored yet; -1: there is none) / of cur
};
constexpr int PF_WORDS = sizeof(PfState) / sizeof(double);
static_assert(sizeof(PfState) % sizeof(double) == 0, "the states lie in a buffer of doubles");

constexpr int PF_IMPROVED = 1;                     // the refit's own counter word, beside POSE_VOID, POSE_BEST1, POSE_BEST

__global__ __launch_bounds__(POSE_BLOCK) void k_pf_init(const double *__restrict__ poses_in, long b, PfState *__restrict__ st)
{
    const long k = (long)blockIdx.x * POSE_BLOCK + threadIdx.x;
    if (k >= b) return;
    PfState S;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        S.cur[j] = poses_in ? poses_in[12 * k + j] : 0.0;
        ok = ok && finite_f64(S.cur[j]);
    }
#pragma unroll
    for (int j = 0; j < 12; ++j) S.best[j] = poses_in && ok ? S.cur[j] : 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) S.cp[j] = S.cq[j] = 0.0;
    S.done = ok ? 0 : 2;
    S.plain = poses_in ? 0 : 1;
    S.best_cnt = -1;
    S.in_cnt = poses_in && ok ? -2 : -1;
    S.n = 0;
    st[k] = S;
}

// a row's terms in a sweep (T = PF_A: the six coordinates, the spans' counts leave too; PF_B: the nine centred products)
template <int N>
struct PfTerms {
    static constexpr int T = N;
    static constexpr bool COUNTS = N == PF_A;
    using State = PfState;
    double md2, cp[3], cq[3];
    bool plain;
    __device__ __forceinline__ PfTerms(const PfState &S, double md2_) : md2(md2_), plain(S.plain != 0)
    {
#pragma unroll
        for (int j = 0; j < 3; ++j) { cp[j] = N == PF_B ? S.cp[j] : 0.0; cq[j] = N == PF_B ? S.cq[j] : 0.0; }
    }
    __device__ __forceinline__ bool operator()(const double (&p)[3], const double (&q)[3], double d2, double (&v)[N]) const
    {
        if constexpr (N == PF_A) {
            v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = q[0]; v[4] = q[1]; v[5] = q[2];
        } else {
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) v[3 * i + j] = (p[i] - cp[i]) * (q[j] - cq[j]);
        }
        if (plain) return finite_f64(p[0]) && finite_f64(p[1]) && finite_f64(p[2]) && finite_f64(q[0]) && finite_f64(q[1]) && finite_f64(q[2]);
        return d2 < md2;
    }
};

// Second stage of sweep A, one workgroup per pose: the tree over the nb partials (between part and part2), the counts as integers;
// then cur's count settles "keep the best", and the centroids are formed.  last: the scoring sweep behind the last round --
// instead of centroids the outputs and the record's counters.
__global__ __launch_bounds__(PT_FOLD) void k_pf_fold_a(PfState *__restrict__ st, double *part, double *part2, const unsigned *__restrict__ cnt,
                                                        long nb, long nb2, long b, int last, double *__restrict__ poses_out,
                                                        int32_t *__restrict__ inl_out, unsigned long long *__restrict__ counters)
{
    __shared__ double node[PT_FOLD_WAVES][PF_A];
    __shared__ unsigned long long total[PT_FOLD_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long k = blockIdx.x; k < b; k += gridDim.x) {
        PfState *S = st + k;
        const bool over = S->done != 0;                                // (read by every thread before thread 0 may change it)
        __syncthreads();
        if (over && !last) continue;
        double *a = part + k * PF_A * nb;
        long sa = nb;
        if (!over) {
            unsigned long long n = 0;
            for (long i = threadIdx.x; i < nb; i += PT_FOLD) n += cnt[k * nb + i];
            n = wsum_u64(n);
            if (lane == 0) total[wave] = n;
            pt_fold(a, sa, part2 + k * PF_A * nb2, nb2, nb, node);
        }
        if (threadIdx.x == 0) {
            if (!over) {
                long long n = 0;
                for (int w = 0; w < PT_FOLD_WAVES; ++w) n += (long long)total[w];
                S->n = n;
                if (!S->plain) {
                    if (S->in_cnt == -2) {
                        S->in_cnt = S->best_cnt = n;                   // (best is the input pose already)
                    } else if (n > S->best_cnt) {
                        S->best_cnt = n;
#pragma unroll
                        for (int j = 0; j < 12; ++j) S->best[j] = S->cur[j];
                    }
                }
                if (!last) {
                    if (n < 3) {
                        S->done = 1;                                   // the round yields nothing
                    } else {
                        const double dn = (double)n;
#pragma unroll
                        for (int j = 0; j < 3; ++j) { S->cp[j] = a[(long)j * sa] / dn; S->cq[j] = a[(long)(3 + j) * sa] / dn; }
                    }
                }
            }
            if (last) {
                const long long bc = S->best_cnt;
#pragma unroll
                for (int j = 0; j < 12; ++j) poses_out[12 * k + j] = bc >= 0 ? S->best[j] : 0.0;
                inl_out[k] = (int32_t)bc;
                if (S->done == 2) atomicAdd(counters + POSE_VOID, 1ull);
                if (bc > S->in_cnt) atomicAdd(counters + PF_IMPROVED, 1ull);
                if (bc >= 0) atomicMax(counters + POSE_BEST1, (unsigned long long)bc + 1);
            }
        }
        __syncthreads();
    }
}

// Sweep B's sums: one lane runs the Jacobi and the pose.  A pose that is not finite, or that repeats cur bit for bit, ends the
// rounds; any other becomes cur.
struct PfSettleB {
    static constexpr int T = PF_B;
    using State = PfState;
    __device__ __forceinline__ void operator()(PfState &S, const double (&K)[PF_B]) const
    {
        double o[12];
        const double cp[3] = {S.cp[0], S.cp[1], S.cp[2]}, cq[3] = {S.cq[0], S.cq[1], S.cq[2]};
        const bool ok = pf_pose(K, cp, cq, o);
        bool same = S.plain == 0;
#pragma unroll
        for (int j = 0; j < 12; ++j) same = same && __double_as_longlong(o[j]) == __double_as_longlong(S.cur[j]);
        if (!ok || same) {
            S.done = 1;
        } else {
#pragma unroll
            for (int j = 0; j < 12; ++j) S.cur[j] = o[j];
            S.plain = 0;
        }
    }
};

}  // namespace
}  // namespace sicp

SICP_EXPORT int sicp_posefit_version(void) { return SICP_POSEFIT_VERSION; }

SICP_EXPORT int sicp_pose_refit(sicp_ctx *c, const double *src, const double *dst, int64_t m, const double *poses_in, int64_t b,
                                double max_distance, int rounds, double *poses_out, int32_t *inliers_out, sicp_posefit_stats *out)
{
    CHK(check_rows_ctx(c, "sicp_pose_refit"));
    CHK(check_matched(src, dst));
    if (!poses_out) return fail(SICP_ERR_INVALID, "poses_out is null");
    if (!inliers_out) return fail(SICP_ERR_INVALID, "inliers_out is null");
    if (!out) return fail(SICP_ERR_INVALID, "out is null");
    CHK(check_matched_count(m));
    CHK(check_poses_rounds(poses_in, b, rounds, SICP_POSEFIT_MAX_ROUNDS));
    CHK(check_max_distance(max_distance, true));
    HIPCHK(hipSetDevice(c->device));
    return op_run(c, [&]() -> int {
        PoseRows R;
        CHK(pose_rows_enter(c, src, dst, m, poses_in, b, poses_out, inliers_out, &R));
        const PoseGrids G = pose_grids((long)m, (long)b, PT_SPAN, PT_FOLD);
        CHK(c->pf_state.reserve((size_t)b * PF_WORDS));
        CHK(c->pf_part.reserve((size_t)b * PF_B * G.nb));
        CHK(c->pf_part2.reserve((size_t)b * PF_B * G.nb2));
        CHK(c->pf_cnt.reserve((size_t)b * G.nb));
        PfState *st = (PfState *)c->pf_state.p;
        const double md2 = max_distance * max_distance;
        hipLaunchKernelGGL(k_pf_init, G.poses, dim3(POSE_BLOCK), 0, c->stream, R.poses_in, (long)b, st);
        HIPCHK(hipGetLastError());
        for (int r = 0; r <= rounds; ++r) {                           // (the pass behind the last round only scores its pose)
            const int last = r == rounds;
            hipLaunchKernelGGL(k_pose_sweep<PfTerms<PF_A>>, G.sweep, dim3(PT_BLOCK), 0, c->stream, R.src, R.dst, st, (long)m, (long)b, G.P, md2,
                               c->pf_part.p, G.nb, c->pf_cnt.p);
            hipLaunchKernelGGL(k_pf_fold_a, G.fold, dim3(PT_FOLD), 0, c->stream, st, c->pf_part.p, c->pf_part2.p, c->pf_cnt.p, G.nb, G.nb2,
                               (long)b, last, R.poses, R.inl, c->cand_small.p);
            if (!last) {
                hipLaunchKernelGGL(k_pose_sweep<PfTerms<PF_B>>, G.sweep, dim3(PT_BLOCK), 0, c->stream, R.src, R.dst, st, (long)m, (long)b, G.P,
                                   md2, c->pf_part.p, G.nb, c->pf_cnt.p);
                hipLaunchKernelGGL(k_pose_fold<PfSettleB>, G.fold, dim3(PT_FOLD), 0, c->stream, st, c->pf_part.p, c->pf_part2.p, G.nb, G.nb2,
                                   (long)b, PfSettleB{});
            }
            HIPCHK(hipGetLastError());
        }
        CHK(pose_best_enqueue(c, k_pose_best, R.inl, (long)b));
        CHK(pose_rows_leave(c, poses_out, inliers_out, b, R, out));
        out->n_poses = b;
        out->n_improved = (int64_t)counters_host(c)[PF_IMPROVED];
        return SICP_OK;
    });
}
