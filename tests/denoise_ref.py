"""Reference of the moving-least-squares smoothing (contract (W); include/simpleicp_hip_denoise.h), built from
the oracle's brute-force k-NN (contracts (D) and (K)), contract (E)'s tree over rows (iss_ref.tree_rows) and plain numpy float64 --
never from the code under test.  TEST INFRASTRUCTURE ONLY.

Every numpy operation below is one IEEE operation per element (numpy fuses nothing), so the expressions ARE the contract.
jacobi3v is simpleicp_amd/csrc/sicp_normals.h's jacobi3 transcribed WITH its eigenvectors, vectorised over the points with masks
the way iss_ref.jacobi3 is: the a_pq == 0 skip and the off == 0 exit change nothing once met.  Its diagonals are iss_ref.jacobi3's
bit for bit (asserted at every call).
"""
import numpy as np

import iss_ref
from iss_ref import in_radius, orc, tree_rows

KEYS = ("n_points", "n_small", "n_moved", "n_clipped", "max_displacement")
DEFAULTS = dict(neighbors=16, radius=None, bandwidth=None, strength=1.0, min_neighbors=3)
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def jacobi3v(C6):
    """(diagonal (n, 3), eigenvectors V (n, 3, 3): column c belongs to diagonal c) the cyclic Jacobi iteration leaves of the
    symmetric matrices with upper triangles C6 (n, 6): 00 01 02 11 12 22."""
    C6 = np.asarray(C6, dtype=np.float64)
    a = np.empty((len(C6), 3, 3))
    a[:, 0, 0], a[:, 0, 1], a[:, 0, 2], a[:, 1, 1], a[:, 1, 2], a[:, 2, 2] = (C6[:, c] for c in range(6))
    a[:, 1, 0], a[:, 2, 0], a[:, 2, 1] = a[:, 0, 1], a[:, 0, 2], a[:, 1, 2]
    v = np.zeros((len(C6), 3, 3))
    v[:, 0, 0] = v[:, 1, 1] = v[:, 2, 2] = 1.0
    with np.errstate(all="ignore"):
        for _ in range(64):
            off = (np.abs(a[:, 0, 1]) + np.abs(a[:, 0, 2])) + np.abs(a[:, 1, 2])
            if not (off != 0.0).any():
                break
            for p, q in ((0, 1), (0, 2), (1, 2)):
                r = 3 - p - q
                apq = a[:, p, q].copy()
                do = ~(apq == 0.0)
                theta = (a[:, q, q] - a[:, p, p]) / (2.0 * apq)
                t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                arp, arq = a[:, r, p].copy(), a[:, r, q].copy()
                a[:, p, p] = np.where(do, a[:, p, p] - t * apq, a[:, p, p])
                a[:, q, q] = np.where(do, a[:, q, q] + t * apq, a[:, q, q])
                a[:, p, q] = a[:, q, p] = np.where(do, 0.0, apq)
                a[:, r, p] = a[:, p, r] = np.where(do, c * arp - s * arq, arp)
                a[:, r, q] = a[:, q, r] = np.where(do, s * arp + c * arq, arq)
                for i in range(3):
                    vip, viq = v[:, i, p].copy(), v[:, i, q].copy()
                    v[:, i, p] = np.where(do, c * vip - s * viq, vip)
                    v[:, i, q] = np.where(do, s * vip + c * viq, viq)
    w = np.stack([a[:, 0, 0], a[:, 1, 1], a[:, 2, 2]], axis=1)
    assert np.array_equal(w.view(np.uint64), iss_ref.jacobi3(C6).view(np.uint64))
    return w, v


def plane_normal(w, v):
    """normal_from_cov's column and sign: the column of the first smallest diagonal entry (all equal: column 2), negated iff its
    component of largest magnitude -- the first of equals -- is negative.  (n, 3) float64."""
    at = np.arange(len(w))
    lo, hi = np.zeros(len(w), np.int64), np.zeros(len(w), np.int64)
    for c in (1, 2):
        lo = np.where(w[:, c] < w[at, lo], c, lo)
        hi = np.where(w[:, c] > w[at, hi], c, hi)
    lo = np.where(lo == hi, 2, lo)
    nv = v[at, :, lo]
    big = np.zeros(len(w), np.int64)
    for c in (1, 2):
        big = np.where(np.abs(nv[:, c]) > np.abs(nv[at, big]), c, big)
    return np.where((nv[at, big] < 0)[:, None], -nv, nv)


def fit(X, idx, d2, radius, bandwidth):
    """Steps 1 to 4 on given lists: (m (n,), W (n,), c (n, 3), C6 (n, 6), ins (n, k))."""
    there = idx >= 0
    ins = there & in_radius(d2, radius)
    with np.errstate(all="ignore"):
        if np.isinf(bandwidth):
            w = np.ones(d2.shape)
        else:
            t = 1.0 - d2 / (np.float64(bandwidth) * np.float64(bandwidth))
            w = np.where(t > 0, t * t, 0.0)
        P = X[np.where(there, idx, 0)]
        W = tree_rows(np.where(ins, w, 0.0))
        c = np.stack([tree_rows(np.where(ins, w * P[:, :, a], 0.0)) / W for a in range(3)], axis=1)
        d = [P[:, :, a] - c[:, a, None] for a in range(3)]
        C6 = np.stack([tree_rows(np.where(ins, w * (d[a] * d[b]), 0.0)) / W for a, b in PAIRS], axis=1)
    return ins.sum(axis=1), W, c, C6, ins


def denoise(X, neighbors=16, radius=None, bandwidth=None, strength=1.0, min_neighbors=3, knn=None):
    """Contract (W), one round.  knn: X's ranked lists (idx, d2) of at least `neighbors` ranks, if the caller has them (the list of
    a smaller k is the prefix of a larger k's).  Returns dict(points (n, 3) f64, normals (n, 3) f32, displacement (n,) f64, and
    the record)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    n, k = len(X), int(neighbors)
    r = np.inf if radius is None else float(radius)
    b = np.inf if bandwidth is None else float(bandwidth)
    idx, d2 = orc.knn(X, X, k=k) if knn is None else (knn[0][:, :k], knn[1][:, :k])
    m, _, c, C6, ins = fit(X, idx, d2, r, b)
    small = m < min_neighbors
    C6[small] = 0.0
    nv = plane_normal(*jacobi3v(C6))
    with np.errstate(all="ignore"):
        h = ((X[:, 0] - c[:, 0]) * nv[:, 0] + (X[:, 1] - c[:, 1]) * nv[:, 1]) + (X[:, 2] - c[:, 2]) * nv[:, 2]
        g = np.float64(strength) * h
        out = X - g[:, None] * nv
    out[small], nv[small], g[small] = X[small], 0.0, 0.0
    return dict(points=out, normals=nv.astype(np.float32), displacement=g, n_points=n, n_small=int(small.sum()),
                n_moved=int((g != 0.0).sum()), n_clipped=0 if np.isinf(r) else int(ins[:, k - 1].sum()),
                max_displacement=float(np.abs(g).max()) if n else 0.0)


def denoise_rounds(X, rounds=1, **kw):
    """`rounds` rounds, each on the output of the one before as a cloud of its own; the last round's dict."""
    for _ in range(rounds):
        ref = denoise(X, **kw)
        X = ref["points"]
    return ref
