"""numpy reference of contract (L), the least-squares pose refit (include/simpleicp_hip_posefit.h), written
from the contract text.  TEST INFRASTRUCTURE ONLY.

float64 numpy, one expression per contract line, vectorised over the poses.  The sums are ``eval_ref.tree_sum``'s tree, the
score is ``global_ref.count_inliers``' (contracts (T) and (D) through the correctly rounded ``global_ref.fma``).
"""
import numpy as np

import eval_ref
import global_ref

SWEEPS = 6                                                            # SICP_POSEFIT_SWEEPS of the header
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def inlier_mask(R, t, src, dst, md2):
    """Step 0 for one pose: the rows c with d2(R src[c] + t, dst[c]) < md2 (contracts (T), (D); a NaN fails)."""
    x, y, z = src[:, 0], src[:, 1], src[:, 2]
    with np.errstate(all="ignore"):
        d = []
        for r in range(3):
            acc = global_ref.fma(R[r, 2], z, global_ref.fma(R[r, 1], y, R[r, 0] * x))
            d.append((acc + t[r]) - dst[:, r])
        d2 = global_ref.fma(d[2], d[2], global_ref.fma(d[1], d[1], d[0] * d[0]))
        return d2 < md2


def _tree_columns(T):
    return np.array([eval_ref.tree_sum(T[:, j]) for j in range(T.shape[1])])


def horn_matrix(K):
    """The ten distinct entries of Horn's N from K[i][j] = sum (p_i - cp_i) (q_j - cq_j), as a full symmetric (..., 4, 4)."""
    Sxx, Sxy, Sxz = K[..., 0, 0], K[..., 0, 1], K[..., 0, 2]
    Syx, Syy, Syz = K[..., 1, 0], K[..., 1, 1], K[..., 1, 2]
    Szx, Szy, Szz = K[..., 2, 0], K[..., 2, 1], K[..., 2, 2]
    N = np.empty(K.shape[:-2] + (4, 4))
    N[..., 0, 0] = (Sxx + Syy) + Szz
    N[..., 1, 1] = (Sxx - Syy) - Szz
    N[..., 2, 2] = (Syy - Sxx) - Szz
    N[..., 3, 3] = (Szz - Sxx) - Syy
    N[..., 0, 1] = N[..., 1, 0] = Syz - Szy
    N[..., 0, 2] = N[..., 2, 0] = Szx - Sxz
    N[..., 0, 3] = N[..., 3, 0] = Sxy - Syx
    N[..., 1, 2] = N[..., 2, 1] = Sxy + Syx
    N[..., 1, 3] = N[..., 3, 1] = Szx + Sxz
    N[..., 2, 3] = N[..., 3, 2] = Syz + Szy
    return N


def jacobi(N, sweeps=SWEEPS):
    """The eigenvector of the largest eigenvalue of the symmetric (..., 4, 4) N by cyclic Jacobi: (..., 4), not normalised."""
    A = np.array(N, dtype=np.float64)
    V = np.zeros_like(A)
    for i in range(4):
        V[..., i, i] = 1.0
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q in PAIRS:
                apq = A[..., p, q]
                go = apq != 0.0                                       # (a NaN rotates and spoils the pose: the round yields nothing)
                safe = np.where(go, apq, 1.0)
                theta = (A[..., q, q] - A[..., p, p]) / (2.0 * safe)
                mag = np.abs(theta) + np.sqrt(theta * theta + 1.0)
                t = np.where(theta < 0.0, -1.0, 1.0) / mag
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                B, W = A.copy(), V.copy()
                B[..., p, p] = A[..., p, p] - t * apq
                B[..., q, q] = A[..., q, q] + t * apq
                B[..., p, q] = B[..., q, p] = 0.0
                for r in range(4):
                    if r != p and r != q:
                        B[..., r, p] = B[..., p, r] = c * A[..., r, p] - s * A[..., r, q]
                        B[..., r, q] = B[..., q, r] = s * A[..., r, p] + c * A[..., r, q]
                    W[..., r, p] = c * V[..., r, p] - s * V[..., r, q]
                    W[..., r, q] = s * V[..., r, p] + c * V[..., r, q]
                A = np.where(go[..., None, None], B, A)
                V = np.where(go[..., None, None], W, V)
        d = np.stack([A[..., i, i] for i in range(4)], axis=-1)
        win = np.zeros(d.shape[:-1], np.int64)
        top = d[..., 0]
        for i in (1, 2, 3):
            better = d[..., i] > top                                  # (strict: a tie stays with the lowest index)
            win = np.where(better, i, win)
            top = np.where(better, d[..., i], top)
    return np.take_along_axis(V, win[..., None, None].repeat(4, axis=-2), axis=-1)[..., 0]


def rotation(quat):
    """R (..., 3, 3) of the quaternion (w, x, y, z), normalised first."""
    with np.errstate(all="ignore"):
        w, x, y, z = (quat[..., i] for i in range(4))
        n = np.sqrt(((w * w + x * x) + y * y) + z * z)
        w, x, y, z = w / n, x / n, y / n, z / n
        R = np.empty(quat.shape[:-1] + (3, 3))
        R[..., 0, 0] = ((w * w + x * x) - y * y) - z * z
        R[..., 0, 1] = (x * y - w * z) * 2.0
        R[..., 0, 2] = (x * z + w * y) * 2.0
        R[..., 1, 0] = (x * y + w * z) * 2.0
        R[..., 1, 1] = ((w * w - x * x) + y * y) - z * z
        R[..., 1, 2] = (y * z - w * x) * 2.0
        R[..., 2, 0] = (x * z - w * y) * 2.0
        R[..., 2, 1] = (y * z + w * x) * 2.0
        R[..., 2, 2] = ((w * w - x * x) - y * y) + z * z
    return R


def fit_masked(src, dst, mask, sweeps=SWEEPS, want_quat=False):
    """One round under a mask (step 1): (R (3, 3), t (3,)) or None if it yields nothing."""
    n = int(np.count_nonzero(mask))
    if n < 3:
        return None
    with np.errstate(all="ignore"):
        sp = _tree_columns(np.where(mask[:, None], src, 0.0))
        sq = _tree_columns(np.where(mask[:, None], dst, 0.0))
        cp, cq = sp / float(n), sq / float(n)
        a, b = src - cp, dst - cq
        terms = np.where(mask[:, None], (a[:, :, None] * b[:, None, :]).reshape(-1, 9), 0.0)
        K = _tree_columns(terms).reshape(3, 3)
        quat = jacobi(horn_matrix(K), sweeps)
        if want_quat:
            return quat
        R = rotation(quat)
        t = cq - ((R[:, 0] * cp[0] + R[:, 1] * cp[1]) + R[:, 2] * cp[2])
    if not (np.isfinite(R).all() and np.isfinite(t).all()):
        return None
    return R, t


def refit(src, dst, poses_in, max_distance, rounds):
    """(poses_out (b, 12) float64, inliers_out (b,) int32, record) of contract (L).  poses_in None: the plain fit, b = 1."""
    src, dst = np.ascontiguousarray(src, dtype=np.float64), np.ascontiguousarray(dst, dtype=np.float64)
    with np.errstate(all="ignore"):
        md2 = np.float64(max_distance) * np.float64(max_distance)
    plain = poses_in is None
    P = np.zeros((1, 12)) if plain else np.ascontiguousarray(poses_in, dtype=np.float64).reshape(-1, 12)
    out, inl = np.zeros_like(P), np.full(len(P), -1, np.int32)
    n_void = n_improved = 0
    for k, pose in enumerate(P):
        if plain:
            mask = np.isfinite(src).all(axis=1) & np.isfinite(dst).all(axis=1)
            cur, first, best, best_n = None, -1, None, -1
        else:
            if not np.isfinite(pose).all():
                n_void += 1
                continue
            cur = (pose[:9].reshape(3, 3), pose[9:])
            mask = inlier_mask(cur[0], cur[1], src, dst, md2)
            first = int(mask.sum())
            best, best_n = cur, first
        for _ in range(int(rounds)):
            new = fit_masked(src, dst, mask)
            if new is None:
                break
            if cur is not None and np.array_equal(new[0].view(np.uint64), cur[0].view(np.uint64)) and \
                    np.array_equal(new[1].view(np.uint64), cur[1].view(np.uint64)):
                break                                                 # (every further round would repeat it)
            cur = new
            mask = inlier_mask(cur[0], cur[1], src, dst, md2)
            n = int(mask.sum())
            if n > best_n:                                            # (strict: the earliest pose wins a tie)
                best, best_n = cur, n
        if best is not None:
            out[k, :9], out[k, 9:], inl[k] = best[0].ravel(), best[1], best_n
        n_improved += int(best_n > first)
    have = inl >= 0
    top = int(inl.max()) if have.any() else -1
    rec = dict(n_poses=len(P), n_void=n_void, n_improved=n_improved, best=int(np.flatnonzero(inl == top)[0]) if have.any() else -1,
               best_inliers=top)
    return out, inl, rec


def kabsch(src, dst):
    """Textbook Kabsch (np.linalg.svd with the determinant fix) of matched rows: the yardstick of the reference, not a contract."""
    cp, cq = src.mean(axis=0), dst.mean(axis=0)
    U, _, Vt = np.linalg.svd((dst - cq).T @ (src - cp))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    return R, cq - R @ cp
