"""Contract (U) (include/simpleicp_hip_cluster.h) in numpy: DBSCAN labels with a strict radius, clusters
ranked by their lowest core index, border points given the smallest label among their core neighbours.  Nothing in it comes from
the library under test.

Two roads.  ``cluster``: the dense neighbour relation from the oracle's squared distances (contract (D)), for n <= 2000 -- the
matrix ``outlier_ref.all_d2`` sorts row by row, here with the indices that tell whose distance each entry is.  ``cluster_pairs``:
scipy's cKDTree.query_pairs, for clouds whose coordinates are small integers -- every difference, square and sum is exact in any
arithmetic there, so the tree's distances are the contract's -- with a radius that no pair lies at.
"""
import sys
from pathlib import Path

import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from oracle import orc  # noqa: E402

KEYS = ("n_points", "n_core", "n_border", "n_noise", "n_clusters", "largest_label", "largest_size")


def relation(X, r):
    """(n, n) bool: j is a neighbour of i iff d2(i, j) < r * r -- outlier_ref.all_d2's matrix put back in index order."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    n = len(X)
    assert n <= 2000
    idx, d2 = orc.knn(X, X, k=n)
    A = np.zeros((n, n), bool)
    A[np.arange(n)[:, None], idx] = d2 < np.float64(r) * np.float64(r)
    return A


def _finish(n, core, comp_of_core, border_rows, border_cols):
    """Labels and record from the core flags, the component number (any numbering) of every core point, in index order of the core
    points, and the (border point, core neighbour) pairs."""
    labels = np.full(n, -1, np.int64)
    core_idx = np.flatnonzero(core)
    if len(core_idx):
        # rank the components by their lowest core index: the first appearance in index order
        _, first = np.unique(comp_of_core, return_index=True)
        order = np.argsort(first)
        rank = np.empty(len(order), np.int64)
        rank[order] = np.arange(len(order))
        labels[core_idx] = rank[comp_of_core]
    if len(border_rows):
        best = np.full(n, np.iinfo(np.int64).max)
        np.minimum.at(best, border_rows, labels[border_cols])
        hit = np.zeros(n, bool)
        hit[border_rows] = True
        labels[hit] = best[hit]
    sizes = np.bincount(labels[labels >= 0]) if (labels >= 0).any() else np.zeros(0, np.int64)
    n_core = int(core.sum())
    n_noise = int((labels < 0).sum())
    return dict(labels=labels.astype(np.int32), core=core.copy(), n_points=int(n), n_core=n_core, n_border=int(n - n_core - n_noise),
                n_noise=n_noise, n_clusters=int(len(sizes)), largest_label=int(np.argmax(sizes)) if len(sizes) else -1,
                largest_size=int(sizes.max()) if len(sizes) else 0)


def cluster(X, r, min_points, A=None):
    """Contract (U) on the dense relation (n <= 2000).  Returns dict(labels (n,) int32, core (n,) bool, and the record's KEYS).
    A: relation(X, r), computed once by the caller and shared."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    n = len(X)
    A = relation(X, r) if A is None else A
    core = A.sum(axis=1) >= min_points
    core_idx = np.flatnonzero(core)
    comp = np.zeros(0, np.int64)
    if len(core_idx):
        _, comp = connected_components(csr_matrix(A[np.ix_(core_idx, core_idx)]), directed=False)
    B = A & ~core[:, None] & core[None, :]                     # (a point that is not core, a core neighbour of it)
    br, bc = np.nonzero(B)
    return _finish(n, core, comp, br, bc)


def cluster_pairs(X, r, min_points):
    """Contract (U) for clouds with small integer coordinates, of any size: the pairs within r from a k-d tree.  r * r must be no
    integer -- no pair lies at exactly r then, and the tree's <= is the contract's <."""
    from scipy.spatial import cKDTree
    X = np.ascontiguousarray(X, dtype=np.float64)
    assert np.array_equal(X, np.round(X)) and np.abs(X).max() < 2**20 and float(r) * float(r) != round(float(r) * float(r))
    n = len(X)
    pairs = cKDTree(X).query_pairs(float(r), output_type="ndarray")
    a, b = pairs[:, 0], pairs[:, 1]
    count = 1 + np.bincount(a, minlength=n) + np.bincount(b, minlength=n)          # (i is its own neighbour)
    core = count >= min_points
    core_idx = np.flatnonzero(core)
    comp = np.zeros(0, np.int64)
    if len(core_idx):
        both = core[a] & core[b]
        pos = np.cumsum(core) - 1
        g = csr_matrix((np.ones(int(both.sum()), bool), (pos[a[both]], pos[b[both]])), shape=(len(core_idx), len(core_idx)))
        _, comp = connected_components(g, directed=False)
    ab = ~core[a] & core[b]
    ba = core[a] & ~core[b]
    return _finish(n, core, comp, np.concatenate([a[ab], b[ba]]), np.concatenate([b[ab], a[ba]]))


def record(r):
    return {key: r[key] for key in KEYS}


# ---- the clouds the tests share ----
def blobs(seed, n, n_blobs=4, noise=0.25, spread=0.35, box=6.0):
    """n points: Gaussian blobs in a box and uniform noise over it, shuffled (seeded)."""
    rng = np.random.default_rng(seed)
    n_noise = int(round(noise * n))
    centres = rng.uniform(0.0, box, (n_blobs, 3))
    which = rng.integers(0, n_blobs, n - n_noise)
    P = centres[which] + rng.standard_normal((n - n_noise, 3)) * spread
    X = np.vstack([P, rng.uniform(-1.0, box + 1.0, (n_noise, 3))])
    return np.ascontiguousarray(X[rng.permutation(n)])


def bridge():
    """x = 0, .5, 1, 1.5, 2 | 4 | 6, 6.5, 7, 7.5, 8 on a line: with r = 2.1 and min_points = 5 two clusters and the point at 4 a
    border of the first."""
    x = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 4.0, 6.0, 6.5, 7.0, 7.5, 8.0])
    return np.ascontiguousarray(np.column_stack([x, np.zeros(11), np.zeros(11)]))


def serpentine(rows=200, width=500):
    """An integer lattice: `rows` rows of `width` points at y = 0, 2, 4, ..., joined at alternating ends by single points at odd y,
    z = 0 -- one long chain at r = 1.25 (100 200 points at the defaults)."""
    xs = np.arange(width, dtype=np.float64)
    parts = []
    for k in range(rows):
        parts.append(np.column_stack([xs, np.full(width, 2.0 * k), np.zeros(width)]))
        if k + 1 < rows:
            parts.append(np.array([[width - 1.0 if k % 2 == 0 else 0.0, 2.0 * k + 1.0, 0.0]]))
    parts.append(np.array([[width - 1.0 if (rows - 1) % 2 == 0 else 0.0, 2.0 * rows - 1.0, 0.0]]))     # a tail: a border at the far end
    return np.ascontiguousarray(np.vstack(parts))


def patches(count=1000, seed=5):
    """An integer lattice: `count` separate 10 x 10 patches on a grid of pitch 14, and sparse noise between them, shuffled."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(count)))
    g = np.stack(np.meshgrid(np.arange(10.0), np.arange(10.0), indexing="ij"), -1).reshape(-1, 2)
    at = np.array([(i % side, i // side) for i in range(count)], dtype=np.float64) * 14.0
    P = (at[:, None, :] + g[None, :, :]).reshape(-1, 2)
    noise = np.unique(np.column_stack([rng.integers(0, side, 300) * 14.0 + 12.0, rng.integers(0, side, 300) * 14.0 + 12.0]), axis=0)
    X = np.vstack([P, noise])
    X = np.column_stack([X, np.zeros(len(X))])
    return np.ascontiguousarray(X[rng.permutation(len(X))])
