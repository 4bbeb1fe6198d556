"""Reference of the consistent normal orientation (contract (H); include/simpleicp_hip_orient.h), built from
the oracle's brute-force k-NN (contracts (D) and (K)) and plain numpy float64 -- never from the code under test.  TEST
INFRASTRUCTURE ONLY, meant for a few thousand points.

Every numpy operation below is one IEEE operation per element (numpy fuses nothing), so the expressions ARE the contract.  The
forest is Kruskal's over the edges sorted by the total order with a plain union-find, the signs a breadth-first search from every
anchor; the round count is Boruvka's algorithm replayed on the edges' ranks.
"""
import sys
from collections import deque
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from oracle import orc  # noqa: E402

KEYS = ("n_points", "n_void", "n_components", "n_forest_edges", "n_flipped", "n_components_voted", "rounds")


def dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def lists(X, k):
    """The ranked k-NN lists (n, k) of every point of X among X."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    return orc.knn(X, X, k=k)[0]


def void_points(N):
    return ~np.isfinite(N).all(axis=1) | (N == 0.0).all(axis=1)


def graph(idx, N):
    """(lo, hi, s): the edges, each once with lo < hi, and their signed dots."""
    n, k = idx.shape
    void = void_points(N)
    i = np.repeat(np.arange(n, dtype=np.int64), k)
    j = idx.ravel().astype(np.int64)
    ok = (j >= 0) & (j < n)
    j = np.where(ok, j, 0)
    ok &= (i != j) & ~void[i] & ~void[j]
    lo, hi = np.minimum(i, j)[ok], np.maximum(i, j)[ok]
    key = np.unique(lo * n + hi)
    lo, hi = key // n, key % n
    with np.errstate(all="ignore"):
        s = dot(N[lo, 0], N[lo, 1], N[lo, 2], N[hi, 0], N[hi, 1], N[hi, 2])
    return lo, hi, s


def total_order(lo, hi, s):
    """The edges' positions, first to last: larger c first, then smaller lo, then smaller hi."""
    return np.lexsort((hi, lo, -np.abs(s)))


class _UnionFind:
    def __init__(self, n):
        self.p = list(range(n))

    def find(self, x):
        p = self.p
        while p[x] != x:
            p[x] = p[p[x]]
            x = p[x]
        return x

    def union(self, a, b):
        a, b = self.find(a), self.find(b)
        if a == b:
            return False
        self.p[max(a, b)] = min(a, b)
        return True


def forest(n, lo, hi, order):
    """The positions (into lo / hi) of the forest's edges: Kruskal over the total order."""
    uf = _UnionFind(n)
    return np.array([e for e in order.tolist() if uf.union(int(lo[e]), int(hi[e]))], dtype=np.int64)


def boruvka_rounds(n, lo, hi, order):
    """The rounds of Boruvka's algorithm that join anything."""
    E = len(lo)
    rank = np.empty(E, np.int64)
    rank[order] = np.arange(E)
    comp = np.arange(n)
    uf = _UnionFind(n)
    rounds = 0
    while True:
        a, b = comp[lo], comp[hi]
        out = a != b
        if not out.any():
            return rounds
        best = np.full(n, E, np.int64)
        np.minimum.at(best, a[out], rank[out])
        np.minimum.at(best, b[out], rank[out])
        for e in order[np.unique(best[best < E])].tolist():
            uf.union(int(lo[e]), int(hi[e]))
        comp = np.array([uf.find(x) for x in range(n)])
        rounds += 1


def orient(X, normals, k, viewpoint=None, away_from=None, idx=None):
    """Contract (H).  Returns dict(normals (n, 3) float32, flipped (n,) bool, component (n,) -- every point's anchor --, forest
    (m, 2) -- the forest's edges (lo, hi) sorted --, and the record's fields)."""
    assert viewpoint is None or away_from is None
    X = np.ascontiguousarray(X, dtype=np.float64)
    N32 = np.ascontiguousarray(normals, dtype=np.float32)
    N = N32.astype(np.float64)
    n = len(X)
    idx = lists(X, k) if idx is None else idx
    void = void_points(N)
    lo, hi, s = graph(idx, N)
    order = total_order(lo, hi, s)
    tree = forest(n, lo, hi, order)
    # signs: breadth-first from every anchor (ascending index: the first unseen point of a component is its lowest)
    adj = [[] for _ in range(n)]
    for e in tree.tolist():
        d = bool(s[e] < 0.0)
        adj[lo[e]].append((int(hi[e]), d))
        adj[hi[e]].append((int(lo[e]), d))
    flipped = np.zeros(n, bool)
    anchor = np.full(n, -1, np.int64)
    for a in range(n):
        if anchor[a] >= 0:
            continue
        anchor[a] = a
        todo = deque([a])
        while todo:
            u = todo.popleft()
            for v, d in adj[u]:
                if anchor[v] < 0:
                    anchor[v] = a
                    flipped[v] = flipped[u] ^ d
                    todo.append(v)
    voted = 0
    r = viewpoint if viewpoint is not None else away_from
    if r is not None:
        r = np.asarray(r, dtype=np.float64)
        M = np.where(flipped[:, None], -N, N)
        with np.errstate(all="ignore"):
            t = dot(r[0] - X[:, 0], r[1] - X[:, 1], r[2] - X[:, 2], M[:, 0], M[:, 1], M[:, 2])
        pos = np.bincount(anchor[~void & (t > 0.0)], minlength=n)
        neg = np.bincount(anchor[~void & (t < 0.0)], minlength=n)
        turn = (neg > pos) if viewpoint is not None else (pos > neg)
        voted = int(turn.sum())
        flipped ^= turn[anchor]
    assert not flipped[void].any()
    out = np.where(flipped[:, None], -N32, N32)
    n_comp = int((anchor == np.arange(n)).sum())
    assert len(tree) == n - n_comp
    pairs = np.column_stack([lo[tree], hi[tree]]) if len(tree) else np.zeros((0, 2), np.int64)
    return dict(normals=out, flipped=flipped, component=anchor, forest=pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))],
                n_points=n, n_void=int(void.sum()), n_components=n_comp, n_forest_edges=len(tree), n_flipped=int(flipped.sum()),
                n_components_voted=voted, rounds=boruvka_rounds(n, lo, hi, order))


def record(ref):
    return {key: int(ref[key]) for key in KEYS}


# ---- clouds with known outward normals ----
def sphere(seed, n, centre=(0.0, 0.0, 0.0), radius=1.0):
    """(X, outward unit normals): n points spread over a sphere."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    return np.ascontiguousarray(np.asarray(centre) + radius * v), v


def torus(seed, n, R=2.0, r=0.7):
    """(X, outward unit normals): n points spread over a torus around the z axis."""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    X = np.column_stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)])
    N = np.column_stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)])
    return np.ascontiguousarray(X), N


def coin(seed, N):
    """(N with every row negated by a seeded coin as float32, the coin)"""
    c = np.random.default_rng(seed).integers(0, 2, len(N)).astype(bool)
    return np.where(c[:, None], -N, N).astype(np.float32), c


def patches(seed=5, count=1000, per=5):
    """`count` patches of `per` points each, 100 apart on a lattice, with unit-ish normals negated by a coin; shuffled."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(count ** (1 / 3)))
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:count].astype(np.float64) * 100.0
    X = (g[:, None, :] + rng.uniform(0.0, 1.0, (count, per, 3))).reshape(-1, 3)
    N = np.tile(np.array([0.0, 0.0, 1.0]), (len(X), 1)) + rng.normal(0, 0.05, (len(X), 3))
    p = rng.permutation(len(X))
    return np.ascontiguousarray(X[p]), coin(seed + 1, N[p])[0]


def surface(seed, n, noise=0.01):
    """A wavy height field with its analytic normals, jittered: (X, N float64)."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-1.0, 1.0, (n, 2))
    z = 0.3 * np.sin(3.0 * xy[:, 0]) * np.cos(2.0 * xy[:, 1])
    gx = 0.9 * np.cos(3.0 * xy[:, 0]) * np.cos(2.0 * xy[:, 1])
    gy = -0.6 * np.sin(3.0 * xy[:, 0]) * np.sin(2.0 * xy[:, 1])
    N = np.column_stack([-gx, -gy, np.ones(n)])
    N /= np.linalg.norm(N, axis=1)[:, None]
    X = np.column_stack([xy, z]) + rng.normal(0, noise, (n, 3))
    return np.ascontiguousarray(X), N + rng.normal(0, 0.05, (n, 3))
