// sicp_posefit.hip -- least-squares poses of matched rows (include/simpleicp_hip_posefit.h; contract (L)).
//
// The shape is sicp_eval.hip's, once per sweep of the contract.  First stage (k_pf_sweep): the grid is (spans of PT_SPAN rows) x
// (poses); every thread rebuilds the mask of its row from the pose (contracts (T) and (D): nine fused multiply-adds), forms its
// terms -- sweep A: the six coordinates and the count, sweep B: the nine centred products -- and the pair tree (sicp_pairtree.h)
// leaves one partial per term, span and pose.  Second stage (k_pf_fold): one workgroup per pose folds the partials; after sweep A
// one lane settles "keep the best" with the count the sweep carried and forms the centroids, after sweep B it runs the 4 x 4
// Jacobi and writes the next pose into the pose's state.  The rounds are enqueued back to back; a pose whose rounds are over
// (PfState::done) costs its workgroups one load.  Counts by ballot and popcount; the record's counters are integer atomics.
#include "sicp_host.h"
#include "sicp_grid_dev.h"
#include "sicp_pairtree.h"
#include "sicp_horn.h"
#include "../../include/simpleicp_hip_posefit.h"

namespace sicp {
namespace {

constexpr int PF_A = 6, PF_B = 9;                  // terms of sweep A (p | q) and of sweep B (K row-major)
constexpr int PF_MAX_POSES_Y = 32768;              // grid limit of the poses' dimension: the workgroups stride from there on
constexpr int PF_BLOCK = 256;

// a pose's state between the launches.  Poses are R row-major, then t.
struct PfState {
    double cur[12], best[12], cp[3], cq[3];
    long long done;                                // 0: rounds go on; 1: they are over; 2: the input pose was void
    long long plain;                               // 1: no pose yet -- the mask is "six finite coordinates" (a NULL start's first round)
    long long best_cnt, in_cnt, n;                 // counts of best / of the input pose (-2: not scored yet; -1: there is none) / of cur
};
constexpr int PF_WORDS = sizeof(PfState) / sizeof(double);
static_assert(sizeof(PfState) % sizeof(double) == 0, "the states lie in a buffer of doubles");

enum { PF_VOID = 0, PF_IMPROVED = 1, PF_BEST1 = 2, PF_BEST = 3 };   // the counter words (st[PF_BEST1] = max of inliers + 1)

__global__ __launch_bounds__(PF_BLOCK) void k_pf_init(const double *__restrict__ poses_in, long b, PfState *__restrict__ st)
{
    const long k = (long)blockIdx.x * PF_BLOCK + threadIdx.x;
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

// First stage.  part: per pose T rows of nb doubles, span s's sums in column s; cnt (sweep A): per pose nb counts.
template <int T>
__global__ __launch_bounds__(PT_BLOCK) void k_pf_sweep(const double *__restrict__ src, const double *__restrict__ dst,
                                                       const PfState *__restrict__ st, long m, long b, long P, double md2,
                                                       double *__restrict__ part, long nb, unsigned *__restrict__ cnt)
{
    __shared__ double node[PT_TILES * PT_WAVES][T];
    __shared__ unsigned found[PT_TILES * PT_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long base = (long)blockIdx.x * PT_SPAN;
    for (long k = blockIdx.y; k < b; k += gridDim.y) {
        const PfState *S = st + k;
        if (S->done) continue;                                         // (the same for the whole workgroup)
        const bool plain = S->plain != 0;
        Xf H;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            H.m[4 * r] = S->cur[3 * r]; H.m[4 * r + 1] = S->cur[3 * r + 1]; H.m[4 * r + 2] = S->cur[3 * r + 2];
            H.m[4 * r + 3] = S->cur[9 + r];
        }
        double cp[3] = {0.0, 0.0, 0.0}, cq[3] = {0.0, 0.0, 0.0};
        if constexpr (T == PF_B) {
#pragma unroll
            for (int j = 0; j < 3; ++j) { cp[j] = S->cp[j]; cq[j] = S->cq[j]; }
        }
#pragma unroll
        for (int t = 0; t < PT_TILES; ++t) {
            const long e = base + (long)t * PT_BLOCK + threadIdx.x;
            double v[T];
            bool in = false;
            if (e < m) {
                const double px = src[3 * e], py = src[3 * e + 1], pz = src[3 * e + 2];
                const double qx = dst[3 * e], qy = dst[3 * e + 1], qz = dst[3 * e + 2];
                if (plain) {
                    in = finite_f64(px) && finite_f64(py) && finite_f64(pz) && finite_f64(qx) && finite_f64(qy) && finite_f64(qz);
                } else {
                    double X, Y, Z;
                    xf(H, px, py, pz, X, Y, Z);
                    const double dx = X - qx, dy = Y - qy, dz = Z - qz;
                    in = fma(dz, dz, fma(dy, dy, dx * dx)) < md2;
                }
                if constexpr (T == PF_A) {
                    v[0] = px; v[1] = py; v[2] = pz; v[3] = qx; v[4] = qy; v[5] = qz;
                } else {
                    const double a[3] = {px - cp[0], py - cp[1], pz - cp[2]}, g[3] = {qx - cq[0], qy - cq[1], qz - cq[2]};
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int j = 0; j < 3; ++j) v[3 * i + j] = a[i] * g[j];
                }
            }
            if (!in) {
#pragma unroll
                for (int j = 0; j < T; ++j) v[j] = 0.0;
            }
            const unsigned long long hits = __ballot(in);
            pt_wave(v, e, P);
            if (lane == 0) {
#pragma unroll
                for (int j = 0; j < T; ++j) node[t * PT_WAVES + wave][j] = v[j];
                found[t * PT_WAVES + wave] = (unsigned)__popcll(hits);
            }
        }
        const double s = pt_nodes<PT_TILES * PT_WAVES>(node, base, P);   // (its barriers also fence `found`)
        if (threadIdx.x < T) part[((long)k * T + threadIdx.x) * nb + blockIdx.x] = s;
        if (T == PF_A && threadIdx.x == T) {
            unsigned n = 0;
            for (int i = 0; i < PT_TILES * PT_WAVES; ++i) n += found[i];
            cnt[k * nb + blockIdx.x] = n;
        }
        __syncthreads();                                               // (`found` may be written again)
    }
}

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
                if (S->done == 2) atomicAdd(counters + PF_VOID, 1ull);
                if (bc > S->in_cnt) atomicAdd(counters + PF_IMPROVED, 1ull);
                if (bc >= 0) atomicMax(counters + PF_BEST1, (unsigned long long)bc + 1);
            }
        }
        __syncthreads();
    }
}

// Second stage of sweep B: the nine sums, then one lane runs the Jacobi and the pose.  A pose that is not finite, or that
// repeats cur bit for bit, ends the rounds; any other becomes cur.
__global__ __launch_bounds__(PT_FOLD) void k_pf_fold_b(PfState *__restrict__ st, double *part, double *part2, long nb, long nb2, long b)
{
    __shared__ double node[PT_FOLD_WAVES][PF_B];
    for (long k = blockIdx.x; k < b; k += gridDim.x) {
        PfState *S = st + k;
        const bool over = S->done != 0;
        __syncthreads();
        if (over) continue;
        double *a = part + k * PF_B * nb;
        long sa = nb;
        pt_fold(a, sa, part2 + k * PF_B * nb2, nb2, nb, node);
        if (threadIdx.x == 0) {
            double K[9], o[12];
#pragma unroll
            for (int j = 0; j < 9; ++j) K[j] = a[(long)j * sa];
            const double cp[3] = {S->cp[0], S->cp[1], S->cp[2]}, cq[3] = {S->cq[0], S->cq[1], S->cq[2]};
            const bool ok = pf_pose(K, cp, cq, o);
            bool same = S->plain == 0;
#pragma unroll
            for (int j = 0; j < 12; ++j) same = same && __double_as_longlong(o[j]) == __double_as_longlong(S->cur[j]);
            if (!ok || same) {
                S->done = 1;
            } else {
#pragma unroll
                for (int j = 0; j < 12; ++j) S->cur[j] = o[j];
                S->plain = 0;
            }
        }
        __syncthreads();
    }
}

// st[PF_BEST] (all ones before) = the lowest k whose inliers + 1 == st[PF_BEST1]
__global__ __launch_bounds__(PF_BLOCK) void k_pf_best(const int32_t *__restrict__ inl, long b, unsigned long long *__restrict__ st)
{
    const unsigned long long best1 = st[PF_BEST1];
    if (best1 == 0) return;
    const int lane = threadIdx.x & 63;
    const long stride = (long)gridDim.x * PF_BLOCK;
    for (long base = (long)blockIdx.x * PF_BLOCK; base < b; base += stride) {
        const long k = base + threadIdx.x;
        const bool is = k < b && inl[k] >= 0 && (unsigned long long)inl[k] + 1 == best1;
        const unsigned long long who = (unsigned long long)__ballot(is);
        if (who && lane == __ffsll((long long)who) - 1) atomicMin(st + PF_BEST, (unsigned long long)k);
    }
}

}  // namespace
}  // namespace sicp

namespace {
static_assert(PF_BEST < CAND_WORDS && PF_BEST != CAND_COUNT, "the record's counters fit the ctx's counter words");
}

SICP_EXPORT int sicp_posefit_version(void) { return SICP_POSEFIT_VERSION; }

SICP_EXPORT int sicp_pose_refit(sicp_ctx *c, const double *src, const double *dst, int64_t m, const double *poses_in, int64_t b,
                                double max_distance, int rounds, double *poses_out, int32_t *inliers_out, sicp_posefit_stats *out)
{
    if (!c) return fail(SICP_ERR_INVALID, "null ctx");
    CHK(check_no_exchange(c, "sicp_pose_refit", "the rows of one rank are not the job's"));
    if (!src) return fail(SICP_ERR_INVALID, "src is null");
    if (!dst) return fail(SICP_ERR_INVALID, "dst is null");
    if (!poses_out) return fail(SICP_ERR_INVALID, "poses_out is null");
    if (!inliers_out) return fail(SICP_ERR_INVALID, "inliers_out is null");
    if (!out) return fail(SICP_ERR_INVALID, "out is null");
    if (m < 3) return fail(SICP_ERR_INVALID, "m must be >= 3 (%lld given)", (long long)m);
    if (m >= (1LL << 31)) return fail(SICP_ERR_INVALID, "m must be < 2^31 (%lld given)", (long long)m);
    if (b < 1) return fail(SICP_ERR_INVALID, "b must be >= 1 (%lld given)", (long long)b);
    if (b >= (1LL << 31)) return fail(SICP_ERR_INVALID, "b must be < 2^31 (%lld given)", (long long)b);
    if (!poses_in && b != 1) return fail(SICP_ERR_INVALID, "poses_in is null: b must be 1 then (%lld given)", (long long)b);
    if (rounds < 1 || rounds > SICP_POSEFIT_MAX_ROUNDS)
        return fail(SICP_ERR_INVALID, "rounds must be >= 1 and <= %d (%d given)", SICP_POSEFIT_MAX_ROUNDS, rounds);
    if (std::isnan(max_distance) || !(max_distance > 0.0)) return fail(SICP_ERR_INVALID, "max_distance must be > 0 (finite or +inf)");
    HIPCHK(hipSetDevice(c->device));
    return op_run(c, [&]() -> int {
        const double *s, *d, *pin = nullptr;
        double *poses;
        int32_t *inl;
        CHK(stage_in(c, src, (size_t)3 * m, c->gl_src, &s));
        CHK(stage_in(c, dst, (size_t)3 * m, c->gl_dst, &d));
        if (poses_in) CHK(stage_in(c, poses_in, (size_t)12 * b, c->pf_in, &pin));
        CHK(stage_out(c, poses_out, (size_t)12 * b, c->gl_pose, &poses));
        CHK(stage_out(c, inliers_out, (size_t)b, c->gl_idx, &inl));
        const long nb = cdiv((long)m, PT_SPAN), nb2 = cdiv(nb, (long)PT_FOLD);
        CHK(c->pf_state.reserve((size_t)b * PF_WORDS));
        CHK(c->pf_part.reserve((size_t)b * PF_B * nb));
        CHK(c->pf_part2.reserve((size_t)b * PF_B * nb2));
        CHK(c->pf_cnt.reserve((size_t)b * nb));
        CHK(counters_clear(c));
        HIPCHK(hipMemsetAsync(c->cand_small.p + PF_BEST, 0xff, sizeof(unsigned long long), c->stream));
        PfState *st = (PfState *)c->pf_state.p;
        long P = 1;
        while (P < m) P *= 2;
        const double md2 = max_distance * max_distance;
        const dim3 sweep_grid((unsigned)nb, (unsigned)std::min<long>(b, PF_MAX_POSES_Y));
        const dim3 fold_grid((unsigned)std::min<long>(b, PF_MAX_POSES_Y));
        hipLaunchKernelGGL(k_pf_init, dim3((unsigned)cdiv((long)b, (long)PF_BLOCK)), dim3(PF_BLOCK), 0, c->stream, pin, (long)b, st);
        HIPCHK(hipGetLastError());
        for (int r = 0; r <= rounds; ++r) {                           // (the pass behind the last round only scores its pose)
            const int last = r == rounds;
            hipLaunchKernelGGL(k_pf_sweep<PF_A>, sweep_grid, dim3(PT_BLOCK), 0, c->stream, s, d, st, (long)m, (long)b, P, md2, c->pf_part.p,
                               nb, c->pf_cnt.p);
            hipLaunchKernelGGL(k_pf_fold_a, fold_grid, dim3(PT_FOLD), 0, c->stream, st, c->pf_part.p, c->pf_part2.p, c->pf_cnt.p, nb, nb2,
                               (long)b, last, poses, inl, c->cand_small.p);
            if (!last) {
                hipLaunchKernelGGL(k_pf_sweep<PF_B>, sweep_grid, dim3(PT_BLOCK), 0, c->stream, s, d, st, (long)m, (long)b, P, md2,
                                   c->pf_part.p, nb, c->pf_cnt.p);
                hipLaunchKernelGGL(k_pf_fold_b, fold_grid, dim3(PT_FOLD), 0, c->stream, st, c->pf_part.p, c->pf_part2.p, nb, nb2, (long)b);
            }
            HIPCHK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_pf_best, dim3((unsigned)std::min<long>(cdiv((long)b, (long)PF_BLOCK), 1024)), dim3(PF_BLOCK), 0, c->stream, inl,
                           (long)b, c->cand_small.p);
        HIPCHK(hipGetLastError());
        CHK(counters_fetch(c));
        CHK(stage_leave(c, poses_out, (size_t)12 * b, poses));
        CHK(stage_leave(c, inliers_out, (size_t)b, inl));
        CHK(sync(c));
        const unsigned long long *hs = counters_host(c);
        out->n_poses = b;
        out->n_void = (int64_t)hs[PF_VOID];
        out->n_improved = (int64_t)hs[PF_IMPROVED];
        out->best = hs[PF_BEST1] ? (int64_t)hs[PF_BEST] : -1;
        out->best_inliers = (int64_t)hs[PF_BEST1] - 1;
        return SICP_OK;
    });
}
