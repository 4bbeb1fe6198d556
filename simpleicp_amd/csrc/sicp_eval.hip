// sicp_eval.hip -- the reduction of sicp_evaluate (include/simpleicp_hip_eval.h, contract (E) of DESIGN.md section 14): the ten sums
// and the inlier count over the 1-NN results a search left in device memory.
//
// Every sum is the balanced adjacent-pair tree over the per-query terms, padded with +0.0 to the next power of two P >= Q.  Any
// aligned power-of-two block of queries is a subtree of that tree, so the tree is cut where the hardware is: 64 queries a wave
// (levels 0-5: lane ^ 1 ... lane ^ 32 exchanges in registers, sicp_lanes.h), the waves of a workgroup and its tiles through LDS
// in the same pair order, the workgroups' partials in a second launch of one workgroup that runs the same code level by level.
// No floating-point atomics, nothing that depends on the launch geometry: the bits are those of the three numpy lines of the
// contract.  A pair whose upper half starts at or beyond P is no addition of the contract (its padding ends at P): the lower half
// passes through as it is -- adding +0.0 would turn a sum that is -0.0 into +0.0.
#include "sicp_internal.h"
#include "sicp_lanes.h"

namespace sicp {
namespace {

constexpr int EV_BLOCK = 256;                      // threads of a workgroup = queries of a tile
constexpr int EV_WAVES = EV_BLOCK / 64;
constexpr int EV_TILES = 4;                        // tiles a workgroup of k_eval_partials takes (a power of two): 1024 queries a partial
constexpr int EV_TERMS = 10;                       // d2 | x y z | xx yy zz xy xz yz
constexpr long EV_SPAN = (long)EV_BLOCK * EV_TILES;
constexpr int EV_FOLD = 1024;                      // threads of k_eval_fold = nodes of one of its steps (its steps are latency, not bytes)
constexpr int EV_FOLD_WAVES = EV_FOLD / 64;

// one level inside the wave: the element e of this lane and its partner's are the halves (size J each) of one pair
template <int J>
__device__ __forceinline__ void ev_level(double (&v)[EV_TERMS], long e, long P)
{
    const bool add = (e & ~(long)(2 * J - 1)) + J < P;             // the pair's upper half lies (partly) below P
#pragma unroll
    for (int j = 0; j < EV_TERMS; ++j) {
        const double o = lane_xor_f64<J>(v[j]);
        v[j] = add ? v[j] + o : v[j];
    }
}

// levels 0-5: afterwards the lowest lane of the wave holds the sum of its 64 elements (elements e ... e + 63 of a tree of P)
__device__ __forceinline__ void ev_wave(double (&v)[EV_TERMS], long e, long P)
{
    ev_level<1>(v, e, P);
    ev_level<2>(v, e, P);
    ev_level<4>(v, e, P);
    ev_level<8>(v, e, P);
    ev_level<16>(v, e, P);
    ev_level<32>(v, e, P);
}

// the levels above the wave: N (a power of two) wave sums per term in LDS, node i covering the 64 elements from base + 64 i;
// thread j < EV_TERMS folds term j in pair order and returns its sum (the others return 0).  Called by all threads.
template <int N>
__device__ __forceinline__ double ev_nodes(double (*node)[EV_TERMS], long base, long P)
{
    __syncthreads();
    double r = 0.0;
    const int j = threadIdx.x;
    if (j < EV_TERMS) {
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

// part: EV_TERMS rows of `stride` doubles, workgroup b's sums in column b; cnt: its inliers
__global__ __launch_bounds__(EV_BLOCK) void k_eval_partials(const int64_t *__restrict__ idx, const double *__restrict__ d2,
                                                            const double *__restrict__ qx, const double *__restrict__ qy,
                                                            const double *__restrict__ qz, long Q, long P, double *__restrict__ part,
                                                            long stride, long long *__restrict__ cnt)
{
    __shared__ double node[EV_TILES * EV_WAVES][EV_TERMS];
    __shared__ unsigned found[EV_TILES * EV_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long base = (long)blockIdx.x * EV_SPAN;
#pragma unroll
    for (int t = 0; t < EV_TILES; ++t) {
        const long e = base + (long)t * EV_BLOCK + threadIdx.x;    // lane l holds element l: coalesced
        double v[EV_TERMS];
        bool in = false;
        if (e < Q) {
            in = idx[e] >= 0;
            const double x = qx[e], y = qy[e], z = qz[e];
            v[0] = d2[e]; v[1] = x; v[2] = y; v[3] = z;
            v[4] = x * x; v[5] = y * y; v[6] = z * z; v[7] = x * y; v[8] = x * z; v[9] = y * z;
        }
        if (!in) {
#pragma unroll
            for (int j = 0; j < EV_TERMS; ++j) v[j] = 0.0;
        }
        const unsigned long long hits = __ballot(in);
        ev_wave(v, e, P);
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < EV_TERMS; ++j) node[t * EV_WAVES + wave][j] = v[j];
            found[t * EV_WAVES + wave] = (unsigned)__popcll(hits);
        }
    }
    const double s = ev_nodes<EV_TILES * EV_WAVES>(node, base, P);
    if (threadIdx.x < EV_TERMS) part[(long)threadIdx.x * stride + blockIdx.x] = s;
    if (threadIdx.x == EV_TERMS) {
        long long n = 0;
        for (int i = 0; i < EV_TILES * EV_WAVES; ++i) n += found[i];
        cnt[blockIdx.x] = n;
    }
}

// One workgroup: the tree over the nb partials of k_eval_partials (padded with +0.0 to a power of two), 1024 nodes a step, level
// after level between the buffers a (row stride sa) and b (row stride sb); the counts as integers; then the record:
// out[0] = Q, out[1] = inliers (int64 bits), out[2 ... 11] the ten sums.
__global__ __launch_bounds__(EV_FOLD) void k_eval_fold(double *a, long sa, double *b, long sb, long nb, const long long *__restrict__ cnt,
                                                        long Q, double *__restrict__ out)
{
    __shared__ double node[EV_FOLD_WAVES][EV_TERMS];
    __shared__ unsigned long long total[EV_FOLD_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long n = 0;
    for (long i = threadIdx.x; i < nb; i += EV_FOLD) n += (unsigned long long)cnt[i];
    n = wsum_u64(n);
    if (lane == 0) total[wave] = n;
    long P = 1;
    while (P < nb) P *= 2;
    long m = nb;                                                   // nodes of this level that exist; the others up to P are +0.0
    while (P > 1) {
        const long tiles = (m + EV_FOLD - 1) / EV_FOLD;
        for (long t = 0; t < tiles; ++t) {
            const long e = t * EV_FOLD + threadIdx.x;
            double v[EV_TERMS];
#pragma unroll
            for (int j = 0; j < EV_TERMS; ++j) v[j] = e < m ? a[(long)j * sa + e] : 0.0;
            ev_wave(v, e, P);
            if (lane == 0) {
#pragma unroll
                for (int j = 0; j < EV_TERMS; ++j) node[wave][j] = v[j];
            }
            const double s = ev_nodes<EV_FOLD_WAVES>(node, t * EV_FOLD, P);
            if (threadIdx.x < EV_TERMS) b[(long)threadIdx.x * sb + t] = s;
        }
        __syncthreads();                                           // this workgroup's own stores, read back by other threads of it
        m = tiles;
        P = P > EV_FOLD ? P / EV_FOLD : 1;
        double *p = a; a = b; b = p;
        const long sp = sa; sa = sb; sb = sp;
    }
    __syncthreads();
    if (threadIdx.x < EV_TERMS) out[2 + threadIdx.x] = a[(long)threadIdx.x * sa];
    if (threadIdx.x == EV_TERMS) {
        unsigned long long all = 0;
        for (int w = 0; w < EV_FOLD_WAVES; ++w) all += total[w];
        out[0] = __longlong_as_double((long long)Q);
        out[1] = __longlong_as_double((long long)all);
    }
}

}  // namespace

long eval_partials_count(long Q) { return (Q + EV_SPAN - 1) / EV_SPAN; }

// scratch: at least 10 * nb + 10 * ceil(nb / 1024) doubles; counts: nb; out12: 12 doubles (the record's 96 bytes)
void launch_eval(hipStream_t s, const int64_t *idx, const double *d2, const double *qx, const double *qy, const double *qz, long Q,
                 double *scratch, long long *counts, double *out12)
{
    const long nb = eval_partials_count(Q), nb2 = (nb + EV_FOLD - 1) / EV_FOLD;
    long P = 1;
    while (P < Q) P *= 2;
    hipLaunchKernelGGL(k_eval_partials, dim3((unsigned)nb), dim3(EV_BLOCK), 0, s, idx, d2, qx, qy, qz, Q, P, scratch, nb, counts);
    hipLaunchKernelGGL(k_eval_fold, dim3(1), dim3(EV_FOLD), 0, s, scratch, nb, scratch + EV_TERMS * nb, nb2, nb, counts, Q, out12);
}

}  // namespace sicp
