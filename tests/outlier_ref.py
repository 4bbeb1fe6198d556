"""Reference of the outlier filters (contract (O)), built from the oracle's brute-force k-NN (contracts (D)
and (K)), plain numpy float64 and eval_ref.tree_sum -- never from the code under test.  TEST INFRASTRUCTURE ONLY.

    d2_(0) <= ... <= d2_(k-1)   orc.knn(X, X[candidate], k): the candidate itself is d2_(0) = 0
    d_i         s = sqrt(d2_(0)); s = s + sqrt(d2_(1)); ...; d_i = s / k
    t_i         d_i for a candidate, +0.0 for every other position (positions: the entries of `rows`, else all points)
    mean        tree(t) / m                      m = the number of candidates
    u_i         (d_i - mean) * (d_i - mean), +0.0 for a non-candidate
    std         sqrt(tree(u) / (m - 1));  m == 1: 0.0
    threshold   mean + std_ratio * std
    keep_i      d_i <= threshold
    radius      count_i = #{j : d2(i, j) < radius * radius}, keep_i = count_i > min_points, reported min(count_i, min_points + 1)
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from eval_ref import tree_sum  # noqa: E402
from oracle import orc  # noqa: E402


def neighbour_d2(X, k, rows=None):
    """(len(rows) or n, k) squared distances of the k nearest points of X, ascending, for the points `rows` of X (None: all)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    Q = X if rows is None else X[np.asarray(rows, dtype=np.int64)]
    return orc.knn(X, np.ascontiguousarray(Q), k=k)[1]


def mean_distance(d2, k=None):
    """d_i of the contract from ranked squared distances (Q, >= k): rank order, every operation rounded on its own."""
    d2 = np.asarray(d2, dtype=np.float64)
    k = d2.shape[1] if k is None else k
    s = np.sqrt(d2[:, 0])
    for j in range(1, k):
        s = s + np.sqrt(d2[:, j])
    return s / np.float64(k)


def statistics(d, cand, std_ratio):
    """(mean, std, threshold) over the positions: d (N,) mean distances, cand (N,) bool."""
    d = np.asarray(d, dtype=np.float64)
    cand = np.asarray(cand, dtype=bool)
    m = int(np.count_nonzero(cand))
    if m == 0:
        return 0.0, 0.0, 0.0
    mean = tree_sum(np.where(cand, d, 0.0)) / np.float64(m)
    c = d - mean
    std = np.sqrt(tree_sum(np.where(cand, c * c, 0.0)) / np.float64(m - 1)) if m > 1 else np.float64(0.0)
    return float(mean), float(std), float(mean + np.float64(std_ratio) * std)


def statistical(X, k, std_ratio, rows=None, mask=None, d2=None):
    """Contract (O), statistical filter.  Returns dict(keep (N,) bool, d (N,) float64, n_candidates, n_kept, mean, std, threshold),
    N = len(rows) or len(X).  d2: (n, >= k) ranked squared distances of ALL points of X, computed once by the caller and shared."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    n = len(X)
    if rows is not None:
        rows = np.asarray(rows, dtype=np.int64)
        dd = neighbour_d2(X, k, rows) if d2 is None else np.asarray(d2)[rows]
        d = mean_distance(dd, k)
        cand = np.ones(len(rows), bool)
    else:
        cand = np.ones(n, bool) if mask is None else np.asarray(mask) != 0
        d = np.zeros(n)
        idx = np.flatnonzero(cand)
        if len(idx):
            dd = neighbour_d2(X, k, idx) if d2 is None else np.asarray(d2)[idx]
            d[idx] = mean_distance(dd, k)
    mean, std, thr = statistics(d, cand, std_ratio)
    keep = cand & (d <= thr)
    return dict(keep=keep, d=d, n_candidates=int(cand.sum()), n_kept=int(keep.sum()), mean=mean, std=std, threshold=thr)


def all_d2(X):
    """(n, n) every point's squared distances to all points, ascending (n <= 2000: the radius filter's full matrix)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    assert len(X) <= 2000
    return orc.knn(X, X, k=len(X))[1]


def radius(X, r, min_points, rows=None, mask=None, D2=None):
    """Contract (O), radius filter.  Returns dict(keep (N,) bool, count (N,) uint32 capped at min_points + 1, n_kept).
    D2: all_d2(X), computed once by the caller and shared."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    D2 = all_d2(X) if D2 is None else D2
    full = np.count_nonzero(D2 < np.float64(r) * np.float64(r), axis=1).astype(np.int64)
    if rows is not None:
        cnt = full[np.asarray(rows, dtype=np.int64)]
        cand = np.ones(len(cnt), bool)
    else:
        cand = np.ones(len(X), bool) if mask is None else np.asarray(mask) != 0
        cnt = np.where(cand, full, 0)
    keep = cand & (cnt > min_points)
    return dict(keep=keep, count=np.where(cand, np.minimum(cnt, min_points + 1), 0).astype(np.uint32), n_kept=int(keep.sum()))
