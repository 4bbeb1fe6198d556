// sicp_horn.h -- Horn's closed-form rotation (device code only): the 4 x 4 matrix of the centred cross sums, the fixed cyclic
// Jacobi sweeps, the quaternion, R and t -- contract (L) step 1 (include/simpleicp_hip_posefit.h).
// sicp_posefit.hip fits with it under a mask, sicp_robust.hip under weights: one text, the same bits.
// The sweeps and folds around it are sicp_pose_dev.h's.
#ifndef SICP_HORN_H
#define SICP_HORN_H

#include "sicp_lanes.h"
#include "../../include/simpleicp_hip_posefit.h"

namespace sicp {

// one Jacobi rotation of the pair (P, Q), P < Q (contract (L)): A and V from their values before it
template <int P, int Q>
__device__ __forceinline__ void pf_rotate(double (&A)[4][4], double (&V)[4][4])
{
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    A[P][P] = A[P][P] - t * apq;
    A[Q][Q] = A[Q][Q] + t * apq;
    A[P][Q] = A[Q][P] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r != P && r != Q) {
            const double arp = A[r][P], arq = A[r][Q];
            A[r][P] = A[P][r] = c * arp - s * arq;
            A[r][Q] = A[Q][r] = s * arp + c * arq;
        }
        const double vrp = V[r][P], vrq = V[r][Q];
        V[r][P] = c * vrp - s * vrq;
        V[r][Q] = s * vrp + c * vrq;
    }
}

// K (row-major: K[3 i + j] = sum of a_i * g_j), the centroids -> the round's pose (R row-major, then t); false: it is not finite
__device__ __forceinline__ bool pf_pose(const double (&K)[9], const double (&cp)[3], const double (&cq)[3], double (&o)[12])
{
    const double Sxx = K[0], Sxy = K[1], Sxz = K[2], Syx = K[3], Syy = K[4], Syz = K[5], Szx = K[6], Szy = K[7], Szz = K[8];
    double A[4][4], V[4][4];
    A[0][0] = (Sxx + Syy) + Szz;
    A[1][1] = (Sxx - Syy) - Szz;
    A[2][2] = (Syy - Sxx) - Szz;
    A[3][3] = (Szz - Sxx) - Syy;
    A[0][1] = A[1][0] = Syz - Szy;
    A[0][2] = A[2][0] = Szx - Sxz;
    A[0][3] = A[3][0] = Sxy - Syx;
    A[1][2] = A[2][1] = Sxy + Syx;
    A[1][3] = A[3][1] = Szx + Sxz;
    A[2][3] = A[3][2] = Syz + Szy;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < SICP_POSEFIT_SWEEPS; ++sweep) {
        pf_rotate<0, 1>(A, V); pf_rotate<0, 2>(A, V); pf_rotate<0, 3>(A, V);
        pf_rotate<1, 2>(A, V); pf_rotate<1, 3>(A, V); pf_rotate<2, 3>(A, V);
    }
    double top = A[0][0];
    double w = V[0][0], x = V[1][0], y = V[2][0], z = V[3][0];
#pragma unroll
    for (int j = 1; j < 4; ++j) {
        if (A[j][j] > top) { top = A[j][j]; w = V[0][j]; x = V[1][j]; y = V[2][j]; z = V[3][j]; }
    }
    const double nrm = sqrt(((w * w + x * x) + y * y) + z * z);
    w = w / nrm; x = x / nrm; y = y / nrm; z = z / nrm;
    o[0] = ((w * w + x * x) - y * y) - z * z;
    o[1] = (x * y - w * z) * 2.0;
    o[2] = (x * z + w * y) * 2.0;
    o[3] = (x * y + w * z) * 2.0;
    o[4] = ((w * w - x * x) + y * y) - z * z;
    o[5] = (y * z - w * x) * 2.0;
    o[6] = (x * z - w * y) * 2.0;
    o[7] = (y * z + w * x) * 2.0;
    o[8] = ((w * w - x * x) - y * y) + z * z;
    bool ok = true;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        o[9 + r] = cq[r] - ((o[3 * r] * cp[0] + o[3 * r + 1] * cp[1]) + o[3 * r + 2] * cp[2]);
    }
#pragma unroll
    for (int j = 0; j < 12; ++j) ok = ok && finite_f64(o[j]);
    return ok;
}

}  // namespace sicp

#endif
