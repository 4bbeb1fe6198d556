// sicp_eval.hip -- the reduction of sicp_evaluate (include/simpleicp_hip_eval.h, contract (E) of DESIGN.md section 14): the ten sums
// and the inlier count over the 1-NN results a search left in device memory.
//
// The ten sums are the tree of contract (E): sicp_pairtree.h holds it, its explanation and the tile constants.
#include "sicp_internal.h"
#include "sicp_pairtree.h"

namespace sicp {
namespace {

constexpr int EV_TERMS = 10;                       // d2 | x y z | xx yy zz xy xz yz

// part: EV_TERMS rows of `stride` doubles, workgroup b's sums in column b; cnt: its inliers
__global__ __launch_bounds__(PT_BLOCK) void k_eval_partials(const int64_t *__restrict__ idx, const double *__restrict__ d2,
                                                            const double *__restrict__ qx, const double *__restrict__ qy,
                                                            const double *__restrict__ qz, long Q, long P, double *__restrict__ part,
                                                            long stride, long long *__restrict__ cnt)
{
    __shared__ double node[PT_TILES * PT_WAVES][EV_TERMS];
    __shared__ unsigned found[PT_TILES * PT_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long base = (long)blockIdx.x * PT_SPAN;
#pragma unroll
    for (int t = 0; t < PT_TILES; ++t) {
        const long e = base + (long)t * PT_BLOCK + threadIdx.x;    // lane l holds element l: coalesced
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
        pt_wave(v, e, P);
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < EV_TERMS; ++j) node[t * PT_WAVES + wave][j] = v[j];
            found[t * PT_WAVES + wave] = (unsigned)__popcll(hits);
        }
    }
    const double s = pt_nodes<PT_TILES * PT_WAVES>(node, base, P);
    if (threadIdx.x < EV_TERMS) part[(long)threadIdx.x * stride + blockIdx.x] = s;
    if (threadIdx.x == EV_TERMS) {
        long long n = 0;
        for (int i = 0; i < PT_TILES * PT_WAVES; ++i) n += found[i];
        cnt[blockIdx.x] = n;
    }
}

// One workgroup: the tree over the nb partials of k_eval_partials (pt_fold, between the buffers a (row stride sa) and b (row stride
// sb)); the counts as integers; then the record:
// out[0] = Q, out[1] = inliers (int64 bits), out[2 ... 11] the ten sums.
__global__ __launch_bounds__(PT_FOLD) void k_eval_fold(double *a, long sa, double *b, long sb, long nb, const long long *__restrict__ cnt,
                                                        long Q, double *__restrict__ out)
{
    __shared__ double node[PT_FOLD_WAVES][EV_TERMS];
    __shared__ unsigned long long total[PT_FOLD_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long n = 0;
    for (long i = threadIdx.x; i < nb; i += PT_FOLD) n += (unsigned long long)cnt[i];
    n = wsum_u64(n);
    if (lane == 0) total[wave] = n;
    pt_fold(a, sa, b, sb, nb, node);
    if (threadIdx.x < EV_TERMS) out[2 + threadIdx.x] = a[(long)threadIdx.x * sa];
    if (threadIdx.x == EV_TERMS) {
        unsigned long long all = 0;
        for (int w = 0; w < PT_FOLD_WAVES; ++w) all += total[w];
        out[0] = __longlong_as_double((long long)Q);
        out[1] = __longlong_as_double((long long)all);
    }
}

}  // namespace

long eval_partials_count(long Q) { return cdiv(Q, PT_SPAN); }

// scratch: at least 10 * nb + 10 * ceil(nb / 1024) doubles; counts: nb; out12: 12 doubles (the record's 96 bytes)
void launch_eval(hipStream_t s, const int64_t *idx, const double *d2, const double *qx, const double *qy, const double *qz, long Q,
                 double *scratch, long long *counts, double *out12)
{
    const long nb = eval_partials_count(Q), nb2 = cdiv(nb, PT_FOLD);
    long P = 1;
    while (P < Q) P *= 2;
    hipLaunchKernelGGL(k_eval_partials, dim3((unsigned)nb), dim3(PT_BLOCK), 0, s, idx, d2, qx, qy, qz, Q, P, scratch, nb, counts);
    hipLaunchKernelGGL(k_eval_fold, dim3(1), dim3(PT_FOLD), 0, s, scratch, nb, scratch + EV_TERMS * nb, nb2, nb, counts, Q, out12);
}

}  // namespace sicp
