"""Reference of the evaluation (contract (E)), built from the oracle's 1-NN and plain numpy float64 -- never
from the code under test.  TEST INFRASTRUCTURE ONLY.

    (idx_i, d2_i)    orc.knn(searched cloud, queries, k = 1, H, max_dist)       (contracts (T), (D), (K), strict bound)
    terms            d2 | x y z | xx yy zz xy xz yz of the inliers, +0.0 for every other query
    S_j              the balanced adjacent-pair tree: pad with +0.0 to a power of two, a = a[0::2] + a[1::2] until one is left
    information      sum of G^T G row by row, G = [ -[p]x | I ]
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from oracle import orc  # noqa: E402


def tree_sum(t):
    """The tree of contract (E) over a vector of float64 terms."""
    t = np.asarray(t, dtype=np.float64)
    P = 1
    while P < len(t):
        P *= 2
    a = np.concatenate([t, np.zeros(P - len(t))])
    while len(a) > 1:
        a = a[0::2] + a[1::2]
    return a[0]


def terms(Xq, idx, d2):
    """(Q, 10) terms of the queries Xq with the 1-NN results (idx, d2)."""
    Xq = np.asarray(Xq, dtype=np.float64)
    x, y, z = Xq[:, 0], Xq[:, 1], Xq[:, 2]
    t = np.column_stack([np.asarray(d2, dtype=np.float64), x, y, z, x * x, y * y, z * z, x * y, x * z, y * z])
    t[np.asarray(idx) < 0] = 0.0
    return t


def record(t, inlier):
    """dict(n_queries, n_inliers, sums (10,)) of a (Q, 10) term array."""
    return dict(n_queries=len(t), n_inliers=int(np.count_nonzero(inlier)), sums=np.array([tree_sum(t[:, j]) for j in range(10)]))


def neighbours(X_query, X_search, H=None, max_distance=np.inf):
    """(idx (Q,), d2 (Q,)) of every query, from the oracle."""
    idx, d2 = orc.knn(X_search, np.ascontiguousarray(X_query, dtype=np.float64), k=1, H=H, max_dist=max_distance)
    return idx[:, 0], d2[:, 0]


def evaluate(X_query, X_search, H=None, max_distance=np.inf, rows=None, nn=None):
    """Contract (E): the rows `rows` (None = all, in order) of X_query against H * X_search.  nn: (idx, d2) of ALL points of X_query
    for these (X_search, H, max_distance), computed once by the caller and shared (the queries' results do not depend on each
    other)."""
    X_query = np.ascontiguousarray(X_query, dtype=np.float64)
    Xq = X_query if rows is None else X_query[np.asarray(rows, dtype=np.int64)]
    if nn is None:
        idx, d2 = neighbours(Xq, X_search, H, max_distance)
    else:
        idx, d2 = (nn[0], nn[1]) if rows is None else (nn[0][rows], nn[1][rows])
    return record(terms(Xq, idx, d2), idx >= 0)


def information_rows(P):
    """sum over the rows p of G^T G, G = [ -[p]x | I ] (3 x 6), one point after the other."""
    L = np.zeros((6, 6))
    for x, y, z in np.asarray(P, dtype=np.float64):
        G = np.array([[0.0, z, -y, 1.0, 0.0, 0.0], [-z, 0.0, x, 0.0, 1.0, 0.0], [y, -x, 0.0, 0.0, 0.0, 1.0]])
        L += G.T @ G
    return L


def information_rows_exact(P):
    """The same sum in exact rational arithmetic (the float64 coordinates are rationals), rounded once at the end."""
    from fractions import Fraction
    L = [[Fraction(0)] * 6 for _ in range(6)]
    for x, y, z in np.asarray(P, dtype=np.float64):
        x, y, z = Fraction(x), Fraction(y), Fraction(z)
        G = [[0, z, -y, 1, 0, 0], [-z, 0, x, 0, 1, 0], [y, -x, 0, 0, 0, 1]]
        for i in range(6):
            for j in range(6):
                L[i][j] += sum(G[k][i] * G[k][j] for k in range(3))
    return np.array([[float(v) for v in row] for row in L])
