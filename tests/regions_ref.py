"""Reference of the smooth regions (contract (J); include/simpleicp_hip_regions.h), built from the oracle's
brute-force k-NN (contracts (D) and (K)), plain numpy float64 and scipy's connected components -- never from the code under test.
TEST INFRASTRUCTURE ONLY, meant for a few thousand points (the long path: a hundred thousand).

Every numpy operation below is one IEEE operation per element (numpy fuses nothing), so the expressions ARE the contract.
"""
import sys
from pathlib import Path

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from oracle import orc  # noqa: E402

KEYS = ("n_points", "n_void", "n_smooth", "n_border", "n_regions_all", "n_regions", "n_labelled", "largest_label", "largest_size")


def lists(X, k):
    """The ranked k-NN lists (n, k) of every point of X among X and their squared distances."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    return orc.knn(X, X, k=k)


def void_points(N):
    return ~np.isfinite(N).all(axis=1) | (N == 0.0).all(axis=1)


def agreement(N, i, j, oriented):
    """t_ij of the contract for the index vectors i, j: the products and sums written out, in the contract's association."""
    with np.errstate(all="ignore"):
        s = (N[i, 0] * N[j, 0] + N[i, 1] * N[j, 1]) + N[i, 2] * N[j, 2]
    return s if oriented else np.abs(s)


def linking_edges(idx, d2, N, radius, cos_min, oriented):
    """(i, j): the DIRECTED list entries that are linking edges -- j in i's list, within the radius, neither void, t >= cos_min."""
    n, k = idx.shape
    void = void_points(N)
    i = np.repeat(np.arange(n, dtype=np.int64), k)
    j = idx.ravel().astype(np.int64)
    ok = (j >= 0) & (j < n)
    j = np.where(ok, j, 0)
    ok &= i != j
    if not np.isinf(radius):
        ok &= d2.ravel() < np.float64(radius) * np.float64(radius)
    ok &= ~void[i] & ~void[j]
    i, j = i[ok], j[ok]
    with np.errstate(invalid="ignore"):
        link = agreement(N, i, j, oriented) >= np.float64(cos_min)
    return i[link], j[link]


def regions(X, normals, k, cos_min, radius=np.inf, oriented=False, seeds=None, min_size=1, knn=None):
    """Contract (J).  Returns dict(labels (n,) int32, root (n,) int64 -- every member's root, -1: none --, kind (n,) -- 0 void,
    1 neither smooth nor void, 2 smooth --, and the record's fields)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    N = np.ascontiguousarray(normals, dtype=np.float32).astype(np.float64)
    n = len(X)
    idx, d2 = lists(X, k) if knn is None else knn
    void = void_points(N)
    seeds = np.ones(n, bool) if seeds is None else np.asarray(seeds) != 0
    smooth = ~void & seeds
    plain = ~void & ~smooth
    i, j = linking_edges(idx, d2, N, float(radius), cos_min, bool(oriented))
    # regions: the components of the smooth points, their roots the lowest indices
    both = smooth[i] & smooth[j]
    graph = coo_matrix((np.ones(int(both.sum()), np.int8), (i[both], j[both])), shape=(n, n))
    comp = connected_components(graph, directed=False)[1]
    lowest = np.full(n, n, np.int64)
    np.minimum.at(lowest, comp[smooth], np.flatnonzero(smooth))
    root = np.where(smooth, lowest[comp], -1)
    n_all = int((root == np.arange(n)).sum())
    # border points: the lowest root over the linking edges with a smooth point, from either end's list
    best = np.full(n, n, np.int64)
    a = plain[i] & smooth[j]
    np.minimum.at(best, i[a], root[j[a]])
    b = smooth[i] & plain[j]
    np.minimum.at(best, j[b], root[i[b]])
    border = plain & (best < n)
    root = np.where(border, best, root)
    # sizes, survival, ranks
    size = np.bincount(root[root >= 0], minlength=n)
    alive = (size >= min_size) & (root == np.arange(n))
    rank = np.cumsum(alive) - 1
    labels = np.where((root >= 0) & alive[np.maximum(root, 0)], rank[np.maximum(root, 0)], -1).astype(np.int32)
    sizes = size[alive]
    largest = int(np.argmax(sizes)) if len(sizes) else -1      # (argmax: the first of equals)
    return dict(labels=labels, root=root, kind=np.where(void, 0, np.where(smooth, 2, 1)),
                n_points=n, n_void=int(void.sum()), n_smooth=int(smooth.sum()), n_border=int(border.sum()), n_regions_all=n_all,
                n_regions=int(alive.sum()), n_labelled=int((labels >= 0).sum()), largest_label=largest,
                largest_size=int(sizes[largest]) if len(sizes) else 0)


def record(ref):
    return {key: int(ref[key]) for key in KEYS}


def cos_of(max_angle):
    import math
    return math.cos(math.radians(max_angle))


# ---- clouds with analytic normals ----
def cube(seed, m=12, jitter=0.2):
    """The six faces of the unit cube, m x m lattice points each (kept off the edges), jittered inside the face by `jitter`
    lattice steps: (X, outward normals, the face of every point)."""
    rng = np.random.default_rng(seed)
    h = 1.0 / m
    u, v = np.meshgrid((np.arange(m) + 0.5) * h, (np.arange(m) + 0.5) * h, indexing="ij")
    X, N, F = [], [], []
    for f in range(6):
        axis, side = f // 2, f % 2
        uv = np.column_stack([u.ravel(), v.ravel()]) + rng.uniform(-jitter * h, jitter * h, (m * m, 2))
        P = np.insert(uv, axis, float(side), axis=1)
        nrm = np.zeros(3)
        nrm[axis] = 1.0 if side else -1.0
        X.append(P), N.append(np.tile(nrm, (m * m, 1))), F.append(np.full(m * m, f))
    return np.ascontiguousarray(np.vstack(X)), np.vstack(N), np.concatenate(F)


def hinge(seed, angle_deg, m=16, jitter=0.2):
    """Two half-planes that meet along the y axis, the second turned up by angle_deg: (X, normals, the side of every point)."""
    rng = np.random.default_rng(seed)
    h = 1.0 / m
    u, v = np.meshgrid((np.arange(m) + 0.5) * h, (np.arange(m) + 0.5) * h, indexing="ij")
    uv = np.column_stack([u.ravel(), v.ravel()]) + rng.uniform(-jitter * h, jitter * h, (m * m, 2))
    a = np.radians(angle_deg)
    left = np.column_stack([-uv[:, 0], uv[:, 1], np.zeros(m * m)])
    right = np.column_stack([uv[:, 0] * np.cos(a), uv[:, 1], uv[:, 0] * np.sin(a)])
    N = np.vstack([np.tile([0.0, 0.0, 1.0], (m * m, 1)), np.tile([-np.sin(a), 0.0, np.cos(a)], (m * m, 1))])
    return np.ascontiguousarray(np.vstack([left, right])), N, np.repeat([0, 1], m * m)


def cylinder(step_deg=2.0, rows=12, radius=1.0):
    """The mantle of a cylinder around the z axis: generators step_deg apart, `rows` points along each, the spacing along z that
    between generators: (X, outward normals)."""
    phi = np.radians(np.arange(0.0, 360.0, step_deg))
    dz = radius * np.radians(step_deg)
    P, Z = np.meshgrid(phi, np.arange(rows) * dz, indexing="ij")
    N = np.column_stack([np.cos(P.ravel()), np.sin(P.ravel()), np.zeros(P.size)])
    return np.ascontiguousarray(N * radius + np.column_stack([np.zeros(P.size), np.zeros(P.size), Z.ravel()])), N


def noisy_box(seed, n, noise=0.004):
    """n points on the faces of a box with unequal sides, noisy, shuffled."""
    rng = np.random.default_rng(seed)
    ext = np.array([1.0, 0.7, 0.5])
    f = rng.integers(0, 6, n)
    P = rng.uniform(0.0, 1.0, (n, 3)) * ext
    P[np.arange(n), f // 2] = np.where(f % 2 == 1, ext[f // 2], 0.0)
    return np.ascontiguousarray(P + rng.normal(0, noise, (n, 3)))


def noisy_can(seed, n, noise=0.004):
    """n points on a closed cylinder (mantle and two lids), noisy, shuffled."""
    rng = np.random.default_rng(seed)
    part = rng.uniform(0, 1, n)
    phi = rng.uniform(0, 2 * np.pi, n)
    rad = np.where(part < 0.5, 0.5, 0.5 * np.sqrt(rng.uniform(0, 1, n)))
    z = np.where(part < 0.5, rng.uniform(0, 1, n), np.where(part < 0.75, 0.0, 1.0))
    P = np.column_stack([rad * np.cos(phi), rad * np.sin(phi), z])
    return np.ascontiguousarray(P + rng.normal(0, noise, (n, 3)))


def patches(seed=5, count=1000):
    """`count` patches of 2 .. 9 points each, 100 apart on a lattice, with equal normals; shuffled.  (X, N, the patch sizes)"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(count ** (1 / 3)))
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:count].astype(np.float64) * 100.0
    per = rng.integers(2, 10, count)
    X = np.repeat(g, per, axis=0) + rng.uniform(0.0, 1.0, (int(per.sum()), 3))
    p = rng.permutation(len(X))
    return np.ascontiguousarray(X[p]), np.tile(np.array([0.0, 0.0, 1.0], np.float32), (len(X), 1)), per
