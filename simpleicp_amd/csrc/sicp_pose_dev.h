// sicp_pose_dev.h -- a pose over matched rows src[c] <-> dst[c] (device code only; the host's part is sicp_host.h's pose frame):
// what sicp_global.hip (contract (R)), sicp_posefit.hip (contract (L)) and sicp_robust.hip (contract (G)) share, one text each
// ("A pose operator's frame").  The pose (12 doubles: R row-major, then t) as an Xf and back; a row's residual
// (contracts (T) and (D)); the first stage of a sweep over (spans of rows) x (poses); the second stage's frame, one workgroup per
// pose; the record's best index.  Horn's fit is sicp_horn.h's, the tree sicp_pairtree.h's.
#ifndef SICP_POSE_DEV_H
#define SICP_POSE_DEV_H

#include "sicp_host.h"
#include "sicp_grid_dev.h"
#include "sicp_pairtree.h"

namespace sicp {

__device__ __forceinline__ Xf pose_xf(const double *pose)
{
    Xf H;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        H.m[4 * r] = pose[3 * r]; H.m[4 * r + 1] = pose[3 * r + 1]; H.m[4 * r + 2] = pose[3 * r + 2];
        H.m[4 * r + 3] = pose[9 + r];
    }
    return H;
}

__device__ __forceinline__ void pose_store(const Xf &H, double *pose)
{
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        pose[3 * r] = H.m[4 * r]; pose[3 * r + 1] = H.m[4 * r + 1]; pose[3 * r + 2] = H.m[4 * r + 2];
        pose[9 + r] = H.m[4 * r + 3];
    }
}

// row e under the pose H: its coordinates and d2 (contracts (T) and (D): nine fused multiply-adds); whether it counts is the caller's
__device__ __forceinline__ double pose_row(const double *__restrict__ src, const double *__restrict__ dst, long e, const Xf &H, double (&p)[3],
                                           double (&q)[3])
{
#pragma unroll
    for (int i = 0; i < 3; ++i) { p[i] = src[3 * e + i]; q[i] = dst[3 * e + i]; }
    double X, Y, Z;
    xf(H, p[0], p[1], p[2], X, Y, Z);
    const double dx = X - q[0], dy = Y - q[1], dz = Z - q[2];
    return fma(dz, dz, fma(dy, dy, dx * dx));
}

// One tile of a first stage: row e's T terms -- terms(p, q, d2, v) says whether the row counts and forms them; +0.0 for a row that
// does not or lies beyond m -- through the wave's levels into node[slot].  Returns the wave's ballot of the rows that count.
template <int T, class Terms>
__device__ __forceinline__ unsigned long long pose_tile(const double *__restrict__ src, const double *__restrict__ dst, long e, long m, long P,
                                                        const Xf &H, const Terms &terms, double (*node)[T], int slot)
{
    double v[T];
    bool in = false;
    if (e < m) {
        double p[3], q[3];
        const double d2 = pose_row(src, dst, e, H, p, q);
        in = terms(p, q, d2, v);
    }
    if (!in) {
#pragma unroll
        for (int j = 0; j < T; ++j) v[j] = 0.0;
    }
    const unsigned long long hits = __ballot(in);
    pt_wave(v, e, P);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < T; ++j) node[slot][j] = v[j];
    }
    return hits;
}

// First stage of a sweep.  Terms names the sweep: Terms::T terms, Terms::State the poses' states (done, cur), Terms::COUNTS whether
// the spans' counts leave too; Terms(S, md2) takes what the rows of one pose share.  part: per pose T rows of nb doubles, span s's
// sums in column s; cnt (COUNTS): per pose nb counts.
template <class Terms>
__global__ __launch_bounds__(PT_BLOCK) void k_pose_sweep(const double *__restrict__ src, const double *__restrict__ dst,
                                                         const typename Terms::State *__restrict__ st, long m, long b, long P, double md2,
                                                         double *__restrict__ part, long nb, unsigned *__restrict__ cnt)
{
    constexpr int T = Terms::T;
    __shared__ double node[PT_TILES * PT_WAVES][T];
    __shared__ unsigned found[Terms::COUNTS ? PT_TILES * PT_WAVES : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long base = (long)blockIdx.x * PT_SPAN;
    for (long k = blockIdx.y; k < b; k += gridDim.y) {
        const typename Terms::State *S = st + k;
        if (S->done) continue;                                         // (the same for the whole workgroup)
        const Xf H = pose_xf(S->cur);
        const Terms terms(*S, md2);
#pragma unroll
        for (int t = 0; t < PT_TILES; ++t) {
            const unsigned long long hits = pose_tile<T>(src, dst, base + (long)t * PT_BLOCK + threadIdx.x, m, P, H, terms, node, t * PT_WAVES + wave);
            if (Terms::COUNTS && lane == 0) found[t * PT_WAVES + wave] = (unsigned)__popcll(hits);
        }
        const double s = pt_nodes<PT_TILES * PT_WAVES>(node, base, P);   // (its barriers also fence `found`)
        if (threadIdx.x < T) part[((long)k * T + threadIdx.x) * nb + blockIdx.x] = s;
        if constexpr (Terms::COUNTS) {
            if (threadIdx.x == T) {
                unsigned n = 0;
                for (int i = 0; i < PT_TILES * PT_WAVES; ++i) n += found[i];
                cnt[k * nb + blockIdx.x] = n;
            }
            __syncthreads();                                           // (`found` may be written again)
        }
    }
}

// Second stage of a sweep, one workgroup per pose: the tree over the nb partials (between part and part2), then thread 0 settles
// the pose's state from the T sums -- settle(S, sums); Settle::T and Settle::State name the sweep, its members what the call fixes.
template <class Settle>
__global__ __launch_bounds__(PT_FOLD) void k_pose_fold(typename Settle::State *__restrict__ st, double *part, double *part2, long nb, long nb2,
                                                       long b, Settle settle)
{
    constexpr int T = Settle::T;
    __shared__ double node[PT_FOLD_WAVES][T];
    for (long k = blockIdx.x; k < b; k += gridDim.x) {
        typename Settle::State *S = st + k;
        const bool over = S->done != 0;                                // (read by every thread before thread 0 may change it)
        __syncthreads();
        if (over) continue;
        double *a = part + k * T * nb;
        long sa = nb;
        pt_fold(a, sa, part2 + k * T * nb2, nb2, nb, node);
        if (threadIdx.x == 0) {
            double sums[T];
#pragma unroll
            for (int j = 0; j < T; ++j) sums[j] = a[(long)j * sa];
            settle(*S, sums);
        }
        __syncthreads();
    }
}

// st[POSE_BEST] (all ones before) = the lowest k whose inliers + 1 == st[POSE_BEST1].  Static: every unit that includes this
// header compiles its own copy and hands it to pose_best_enqueue (sicp_host.h), which owns the grid rule.
static __global__ __launch_bounds__(POSE_BLOCK) void k_pose_best(const int32_t *__restrict__ inl, long n, unsigned long long *__restrict__ st)
{
    const unsigned long long best1 = st[POSE_BEST1];
    if (best1 == 0) return;
    const int lane = threadIdx.x & 63;
    const long stride = (long)gridDim.x * POSE_BLOCK;
    for (long base = (long)blockIdx.x * POSE_BLOCK; base < n; base += stride) {
        const long k = base + threadIdx.x;
        const bool is = k < n && inl[k] >= 0 && (unsigned long long)inl[k] + 1 == best1;
        const unsigned long long who = (unsigned long long)__ballot(is);
        if (who && lane == __ffsll((long long)who) - 1) atomicMin(st + POSE_BEST, (unsigned long long)k);      // (the wave's lowest)
    }
}

}  // namespace sicp

#endif
