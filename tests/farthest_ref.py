"""Reference of farthest point sampling (contract (S); include/simpleicp_hip_farthest.h) in numpy, one
expression a contract line; the fused multiply-adds of contract (D) are global_ref.fma.  Keep coordinates away from underflow:
global_ref.fma is exact for products that neither overflow nor underflow (an overflow falls back to a * b + c, which is +inf
where the fused result is)."""
import numpy as np

from global_ref import fma

KEYS = ("n_points", "n_candidates", "n_selected", "cover_d2")


def candidates(X, mask=None):
    """step 1: mask byte non-zero (None: every row) and three finite coordinates"""
    X = np.asarray(X, dtype=np.float64)
    ok = np.isfinite(X).all(axis=1)
    return ok if mask is None else ok & (np.asarray(mask) != 0)


def d2_to(X, s):
    """step 2, contract (D): every row's squared distance to row s"""
    with np.errstate(all="ignore"):
        dx, dy, dz = X[:, 0] - X[s, 0], X[:, 1] - X[s, 1], X[:, 2] - X[s, 2]
        return fma(dz, dz, fma(dy, dy, dx * dx))


def farthest(X, mask, m, start=-1):
    """(idx (m,) int64, d2 (m,) float64, the record as a dict with KEYS)"""
    X = np.ascontiguousarray(X, dtype=np.float64)
    n = len(X)
    assert X.ndim == 2 and X.shape[1] == 3 and 1 <= m <= n and -1 <= start < n
    cand = candidates(X, mask)
    idx, d2 = np.full(m, -1, np.int64), np.zeros(m, np.float64)
    rec = dict(n_points=n, n_candidates=int(cand.sum()), n_selected=0, cover_d2=0.0)
    # step 3
    s = int(start) if start >= 0 else (int(np.flatnonzero(cand)[0]) if cand.any() else -1)
    if s < 0 or not cand[s]:
        return idx, d2, rec
    mi = np.where(cand, np.inf, -1.0)                  # (-1.0: no candidate -- below every m_i, so np.argmax never takes it)
    D, t = np.inf, 0
    while True:
        idx[t], d2[t] = s, D
        t += 1
        d = d2_to(X, s)
        mi = np.where(cand & (d < mi), d, mi)
        s = int(np.argmax(mi))                         # step 4: the largest m_i, the lowest index of equal values
        D = float(mi[s])
        if t == m or not D > 0.0:
            break
    rec["n_selected"] = t
    rec["cover_d2"] = D if D > 0.0 else 0.0
    return idx, d2, rec


# ---- constructed inputs ----
def lattice(k):
    """the k x k x k integer lattice, row order x fastest: ties everywhere"""
    g = np.arange(k, dtype=np.float64)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    return np.column_stack([x.ravel(), y.ravel(), z.ravel()])


def repeated(p, times, seed=0):
    """p distinct points, each `times` times, shuffled"""
    rng = np.random.default_rng(seed)
    P = rng.uniform(-5.0, 5.0, (p, 3))
    return np.repeat(P, times, axis=0)[rng.permutation(p * times)]


def cloud(seed, n):
    return np.random.default_rng(seed).uniform(-10.0, 10.0, (n, 3))
