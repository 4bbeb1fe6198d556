"""numpy reference of contract (G), the robust pose fit (include/simpleicp_hip_robust.h), written from the
contract text.  TEST INFRASTRUCTURE ONLY.

float64 numpy, one expression per contract line.  The sums are ``eval_ref.tree_sum``'s tree, contracts (T) and (D) go through the
correctly rounded ``global_ref.fma``, Horn's matrix, the Jacobi sweeps and the rotation are ``posefit_ref``'s.
"""
import numpy as np

import eval_ref
import global_ref
import posefit_ref

MAX_ROUNDS = 256                                                      # SICP_ROBUST_MAX_ROUNDS of the header


def residuals(R, t, src, dst):
    """d2_c under the pose (contracts (T), (D)) and the rows that count: six finite coordinates and a finite d2_c."""
    x, y, z = src[:, 0], src[:, 1], src[:, 2]
    with np.errstate(all="ignore"):
        d = []
        for r in range(3):
            acc = global_ref.fma(R[r, 2], z, global_ref.fma(R[r, 1], y, R[r, 0] * x))
            d.append((acc + t[r]) - dst[:, r])
        d2 = global_ref.fma(d[2], d[2], global_ref.fma(d[1], d[1], d[0] * d[0]))
    return d2, np.isfinite(src).all(axis=1) & np.isfinite(dst).all(axis=1) & np.isfinite(d2)


def _tree_columns(T):
    return np.array([eval_ref.tree_sum(T[:, j]) for j in range(T.shape[1])])


def weights(d2, counts, s):
    """Step 1's weights: u = s / (s + d2), w = u * u; +0.0 for a row that does not count."""
    with np.errstate(all="ignore"):
        u = s / (s + d2)
        return np.where(counts, u * u, 0.0)


def one_round(src, dst, R, t, s):
    """Step 1 for one pose: (R, t) or None if the round yields nothing."""
    d2, counts = residuals(R, t, src, dst)
    w = weights(d2, counts, s)
    with np.errstate(all="ignore"):
        a_terms = np.column_stack([w, w[:, None] * src, w[:, None] * dst])
        sums = _tree_columns(np.where(counts[:, None], a_terms, 0.0))
        W = sums[0]
        if not (np.isfinite(W) and W > 0.0):
            return None
        cp, cq = sums[1:4] / W, sums[4:7] / W
        a = w[:, None] * (src - cp)
        g = dst - cq
        K = _tree_columns(np.where(counts[:, None], (a[:, :, None] * g[:, None, :]).reshape(-1, 9), 0.0)).reshape(3, 3)
        Rn = posefit_ref.rotation(posefit_ref.jacobi(posefit_ref.horn_matrix(K)))
        tn = cq - ((Rn[:, 0] * cp[0] + Rn[:, 1] * cp[1]) + Rn[:, 2] * cp[2])
    if not (np.isfinite(Rn).all() and np.isfinite(tn).all()):
        return None
    return Rn, tn


def robust(src, dst, poses_in, max_distance, rounds, divisor, start_scale=0.0, trace=None):
    """(poses_out (b, 12) float64, inliers_out (b,) int32, scales_out (b,) float64, record) of contract (G).  poses_in None: the
    identity, b = 1.  trace: a list that receives (k, round, s) for every round that is run."""
    src, dst = np.ascontiguousarray(src, dtype=np.float64), np.ascontiguousarray(dst, dtype=np.float64)
    md2 = np.float64(max_distance) * np.float64(max_distance)
    divisor, start_scale = np.float64(divisor), np.float64(start_scale)
    P = np.concatenate([np.eye(3).ravel(), np.zeros(3)])[None] if poses_in is None else \
        np.ascontiguousarray(poses_in, dtype=np.float64).reshape(-1, 12)
    out, inl, scales = np.zeros_like(P), np.full(len(P), -1, np.int32), np.zeros(len(P))
    n_void = 0
    for k, pose in enumerate(P):
        if not np.isfinite(pose).all():
            n_void += 1
            continue
        R, t = pose[:9].reshape(3, 3).copy(), pose[9:].copy()
        if start_scale != 0.0:
            s = start_scale
        else:
            d2, counts = residuals(R, t, src, dst)
            if not counts.any():
                n_void += 1
                continue
            with np.errstate(all="ignore"):
                s = np.float64(2.0) * d2[counts].max()
        if s < md2:
            s = md2
        for r in range(int(rounds)):
            if trace is not None:
                trace.append((k, r, float(s)))
            new = one_round(src, dst, R, t, s)
            if new is None:
                break
            R, t = new
            s = s / divisor
            if s < md2:
                s = md2
        d2, _ = residuals(R, t, src, dst)
        with np.errstate(all="ignore"):
            out[k, :9], out[k, 9:], inl[k], scales[k] = R.ravel(), t, int(np.count_nonzero(d2 < md2)), s
    have = inl >= 0
    top = int(inl.max()) if have.any() else -1
    rec = dict(n_poses=len(P), n_void=n_void, best=int(np.flatnonzero(inl == top)[0]) if have.any() else -1, best_inliers=top)
    return out, inl, scales, rec
