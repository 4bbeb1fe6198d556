// sicp_pairtree.h -- the reduction of contract (E) for T terms at once (device code only): sicp_eval.hip sums
// its ten with it, sicp_outlier.hip its one.
//
// Every sum is the balanced adjacent-pair tree over the per-element terms, padded with +0.0 to the next power of two P >= the
// number of elements.  Any aligned power-of-two block of elements is a subtree of that tree, so the tree is cut where the hardware
// is: 64 elements a wave (levels 0-5: lane ^ 1 ... lane ^ 32 exchanges in registers, sicp_lanes.h), the waves of a workgroup and its
// tiles through LDS in the same pair order, the workgroups' partials in a second launch of one workgroup that runs the same code
// level by level.  No floating-point atomics, nothing that depends on the launch geometry: the bits are those of the three numpy
// lines of the contract.  A pair whose upper half starts at or beyond P is no addition of the contract (its padding ends at P): the
// lower half passes through as it is -- adding +0.0 would turn a sum that is -0.0 into +0.0.
#ifndef SICP_PAIRTREE_H
#define SICP_PAIRTREE_H

#include "sicp_lanes.h"

namespace sicp {

constexpr int PT_BLOCK = 256;                      // threads of a workgroup of a first stage = elements of a tile
constexpr int PT_WAVES = PT_BLOCK / 64;
constexpr int PT_TILES = 4;                        // tiles a workgroup of a first stage takes (a power of two): 1024 elements a partial
constexpr long PT_SPAN = (long)PT_BLOCK * PT_TILES;
constexpr int PT_FOLD = 1024;                      // threads of a second stage = nodes of one of its steps (its steps are latency, not bytes)
constexpr int PT_FOLD_WAVES = PT_FOLD / 64;

// one level inside the wave: the element e of this lane and its partner's are the halves (size J each) of one pair
template <int J, int T>
__device__ __forceinline__ void pt_level(double (&v)[T], long e, long P)
{
    const bool add = (e & ~(long)(2 * J - 1)) + J < P;             // the pair's upper half lies (partly) below P
#pragma unroll
    for (int j = 0; j < T; ++j) {
        const double o = lane_xor_f64<J>(v[j]);
        v[j] = add ? v[j] + o : v[j];
    }
}

// levels 0-5: afterwards the lowest lane of the wave holds the sum of its 64 elements (elements e ... e + 63 of a tree of P)
template <int T>
__device__ __forceinline__ void pt_wave(double (&v)[T], long e, long P)
{
    pt_level<1>(v, e, P);
    pt_level<2>(v, e, P);
    pt_level<4>(v, e, P);
    pt_level<8>(v, e, P);
    pt_level<16>(v, e, P);
    pt_level<32>(v, e, P);
}

// the levels above the wave: N (a power of two) wave sums per term in LDS, node i covering the 64 elements from base + 64 i;
// thread j < T folds term j in pair order and returns its sum (the others return 0).  Called by all threads.
template <int N, int T>
__device__ __forceinline__ double pt_nodes(double (*node)[T], long base, long P)
{
    __syncthreads();
    double r = 0.0;
    const int j = threadIdx.x;
    if (j < T) {
        double a[N];
#pragma unroll
        for (int i = 0; i < N; ++i) a[i] = node[i][j];
#pragma unroll
        for (int s = 1; s < N; s *= 2)
#pragma unroll
            for (int i = 0; i < N; i += 2 * s)
                a[i] = base + 64L * (i + s) < P ? a[i] + a[i + s] : a[i];
        r = a[0];
    }
    __syncthreads();                                               // (the nodes may be written again)
    return r;
}

// The second stage, one workgroup of PT_FOLD threads: the tree over nb partials per term (padded with +0.0 to a power of two),
// PT_FOLD nodes a step, level after level between the buffers a and b.  A buffer holds T rows, term j's from j * its stride on
// (T == 1: no stride is read).  Returns with a and sa naming the buffer whose row heads are the T sums, visible to every thread.
template <int T>
__device__ __forceinline__ void pt_fold(double *&a, long &sa, double *b, long sb, long nb, double (*node)[T])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long P = 1;
    while (P < nb) P *= 2;
    long m = nb;                                                   // nodes of this level that exist; the others up to P are +0.0
    while (P > 1) {
        const long tiles = (m + PT_FOLD - 1) / PT_FOLD;
        for (long t = 0; t < tiles; ++t) {
            const long e = t * PT_FOLD + threadIdx.x;
            double v[T];
#pragma unroll
            for (int j = 0; j < T; ++j) v[j] = e < m ? a[(long)j * sa + e] : 0.0;
            pt_wave(v, e, P);
            if (lane == 0) {
#pragma unroll
                for (int j = 0; j < T; ++j) node[wave][j] = v[j];
            }
            const double s = pt_nodes<PT_FOLD_WAVES>(node, t * PT_FOLD, P);
            if (threadIdx.x < T) b[(long)threadIdx.x * sb + t] = s;
        }
        __syncthreads();                                           // this workgroup's own stores, read back by other threads of it
        m = tiles;
        P = P > PT_FOLD ? P / PT_FOLD : 1;
        double *p = a; a = b; b = p;
        const long sp = sa; sa = sb; sb = sp;
    }
    __syncthreads();
}

}  // namespace sicp

#endif
