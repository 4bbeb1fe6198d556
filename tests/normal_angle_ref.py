"""Reference of the rejection by the angle between normals (contract (N)), built from the oracle's entry
points and plain numpy float64 -- never from the code under test.  TEST INFRASTRUCTURE ONLY.

    n2 of movable point m   orc.knn(X_mov, X_mov[m], k) + orc.normals         (self included, ties by index)
    verdict                 restated below, every operation separately rounded
    one iteration           as orc.icp_iteration, the verdict folded into the planarity column as NaN before orc.reject
                            (the way orc.py folds pc2's planarity verdict)
    a run                   a loop of those with orc.run's convergence rule
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from oracle import orc  # noqa: E402


def cos_of(n1, n2, H):
    """c of contract (N) per row: n1, n2 (Q, 3) float32; H 4x4.  float64, no fused operations (numpy has none)."""
    a = np.asarray(n1, dtype=np.float32).astype(np.float64)
    b = np.asarray(n2, dtype=np.float32).astype(np.float64)
    R = np.asarray(H, dtype=np.float64).reshape(4, 4)[:3, :3]
    r = [(R[i, 0] * b[:, 0] + R[i, 1] * b[:, 1]) + R[i, 2] * b[:, 2] for i in range(3)]
    return (a[:, 0] * r[0] + a[:, 1] * r[1]) + a[:, 2] * r[2]


def verdict(n1, n2, H, cos_max):
    """keep mask of contract (N): |c| >= cos_max, NaN fails."""
    with np.errstate(invalid="ignore"):
        return np.abs(cos_of(n1, n2, H)) >= cos_max


def movable_normals(X_mov, rows, k):
    """float32 normals of the listed points of X_mov: k-NN among ALL points of X_mov (self included), as sicp_estimate_normals."""
    X_mov = np.ascontiguousarray(X_mov, dtype=np.float64)
    rows = np.asarray(rows, dtype=np.int64)
    uniq, inv = np.unique(rows, return_inverse=True)
    nn, _ = orc.knn(X_mov, X_mov[uniq], k=k)
    nv, _ = orc.normals(X_mov, nn)
    return nv[inv]


def iteration(X_mov, p1, n1, planarity, x_prev, w, obs, ow, min_planarity, cos_max, k, mov_normals=None):
    """One iteration with the rejection.  mov_normals: (len(X_mov), 3) float32 columns of the movable cloud, None = estimated.
    Returns orc.icp_iteration's dict plus `angle_ok` (the verdict per correspondence), `n2`, `planar_ok`."""
    H = orc.params_to_H(x_prev)
    nn, _ = orc.knn(X_mov, p1, k=1, H=H)
    nn = nn[:, 0]
    n2 = movable_normals(X_mov, nn, k) if mov_normals is None else np.asarray(mov_normals, dtype=np.float32)[nn]
    ok = verdict(n1, n2, H, cos_max)
    pl = np.where(ok, np.asarray(planarity, dtype=np.float32), np.float32(np.nan))
    r = orc.icp_iteration(X_mov, p1, n1, pl, x_prev, x_prev, w, obs, ow, min_planarity)
    assert np.array_equal(r["nn"], nn)
    r.update(angle_ok=ok, n2=n2, planar_ok=np.asarray(planarity, dtype=np.float32) >= np.float32(min_planarity))
    return r


def run(X_mov, p1, n1, planarity, obs, ow, min_planarity, cos_max, k, w=1.0, min_change=1.0, max_iterations=100, mov_normals=None):
    """The loop of orc.run over `iteration`.  Returns dict(x, H, iterations, stats, first, last, matched) -- matched: every movable
    point any iteration matched to a correspondence that was still alive before the angle test (the points whose normal is needed)."""
    x = np.array(obs, dtype=float)
    stats, first, r, its = [], None, None, []
    matched = set()
    for it in range(max_iterations):
        r = iteration(X_mov, p1, n1, planarity, x, w, obs, ow, min_planarity, cos_max, k, mov_normals)
        r["x_prev"] = x.copy()
        its.append(r)
        if first is None:
            first = r
        matched.update(int(m) for m in r["nn"][r["planar_ok"]])
        w, x = r["w"], r["x"]
        stats.append((r["n"], r["residuals"].mean(), r["residuals"].std()))
        if it > 0:
            def ch(a, b):
                return (0.0 if a == 0 else np.inf) if b == 0 else abs((a - b) / b * 100)
            if ch(stats[it][1], stats[it - 1][1]) < min_change and ch(stats[it][2], stats[it - 1][2]) < min_change:
                break
    return dict(x=x, H=orc.params_to_H(x), iterations=len(stats), stats=stats, first=first, last=r, its=its, matched=matched, w=w)


def dropped_share(first):
    """Share of the planarity-surviving correspondences that the verdict drops in iteration 0 (the tests' data condition)."""
    planar = first["planar_ok"]
    return float((planar & ~first["angle_ok"]).sum()) / max(int(planar.sum()), 1)
