"""The reference for contract (V) in numpy, and the clouds the voxel tests run on.

TEST INFRASTRUCTURE ONLY.  ``voxels`` is the contract's formula, ``keep`` the verdicts -- the lowest-index candidate of every
occupied voxel --, ``kept_rows`` the kept rows in ascending order.
"""
import numpy as np


def voxels(X, c, o=(0.0, 0.0, 0.0)):
    """(n, 3) float64 lattice indices: np.floor((X - o) / c), as the contract writes it."""
    return np.floor((np.asarray(X, dtype=np.float64) - np.asarray(o, dtype=np.float64)) / np.float64(c))


def _first_of_each(V):
    """Positions of the first row of every distinct row of V (np.unique sorts stably, so `first` is the lowest position).  Rows whose
    offsets from the column minima fit 21 bits each are compared as one packed integer -- the same partition as axis=0, and the only
    way through 10 M rows in seconds; anything wider takes np.unique(axis=0) itself."""
    V = V + 0.0                                            # (-0.0 and 0.0 are one voxel)
    rel = V - V.min(axis=0)
    if rel.max() < 2.0 ** 21:
        r = rel.astype(np.int64)
        return np.unique((r[:, 0] << 42) | (r[:, 1] << 21) | r[:, 2], return_index=True)[1]
    return np.unique(V, axis=0, return_index=True)[1]


def keep(X, c, o=(0.0, 0.0, 0.0), rows=None, mask=None):
    """Verdicts of contract (V).  rows None and mask None: one bool per point.  rows: one per entry of `rows` (the candidates are
    taken in index order: lowest point index first, an earlier entry before a later one).  mask: one per point, False outside it."""
    X = np.asarray(X, dtype=np.float64)
    if mask is not None:
        cand = np.flatnonzero(np.asarray(mask) != 0)
        out = np.zeros(len(X), bool)
        if len(cand):
            out[cand[_first_of_each(voxels(X[cand], c, o))]] = True
        return out
    if rows is None:
        out = np.zeros(len(X), bool)
        if len(X):
            out[_first_of_each(voxels(X, c, o))] = True
        return out
    rows = np.asarray(rows, dtype=np.int64)
    order = np.argsort(rows, kind="stable")
    out = np.zeros(len(rows), bool)
    if len(rows):
        out[order[_first_of_each(voxels(X[rows[order]], c, o))]] = True
    return out


def kept_rows(X, c, o=(0.0, 0.0, 0.0), rows=None, mask=None):
    k = keep(X, c, o, rows, mask)
    return np.flatnonzero(k) if rows is None else np.sort(np.asarray(rows, dtype=np.int64)[k])


# ---- the clouds of the full-size legs: bench.py's generators (--config C4 and T), one cloud each ----
def uniform_surface(n, seed=0):
    """The fixed cloud of bench.py's synthetic pair: a 10 pts/m^2 surface, centroid removed."""
    L = np.sqrt(n / 10.0)
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, L, n)
    y = rng.uniform(0, L, n)
    z = (20 * np.sin(2 * np.pi * x / 200) * np.cos(2 * np.pi * y / 300)
         + 5 * np.sin(2 * np.pi * x / 37 + 1) * np.sin(2 * np.pi * y / 53) + rng.normal(0, 0.02, n))
    X = np.column_stack((x, y, z))
    return np.ascontiguousarray(X - X.mean(axis=0))


_BOXES = np.array([  # xmin, xmax, ymin, ymax, zmax (from the ground up)
    [-60.0, 60.0, 44.0, 45.0, 14.0], [-60.0, 60.0, -45.0, -44.0, 14.0], [59.0, 60.0, -45.0, 45.0, 14.0], [-60.0, -59.0, -45.0, 45.0, 14.0],
    [12.0, 24.0, 8.0, 20.0, 9.0], [-30.0, -18.0, -22.0, -6.0, 6.0], [-14.0, -8.0, 14.0, 30.0, 11.0], [30.0, 36.0, -30.0, -12.0, 4.0],
    [3.0, 4.2, -6.0, -4.8, 2.4],
])


def terrestrial_scan(want, origin=(0.0, 0.0, 1.8), yaw=0.0, seed=10):
    """One scan of bench.py's terrestrial stand-in (its fixed cloud by default): ground, walls and blocks under uniform ANGULAR
    sampling, so the density falls like 1 / r^2 between 2 m and 80 m; in the scanner's frame."""
    origin = np.asarray(origin, dtype=float)
    rng = np.random.default_rng(seed)
    out = []
    have = 0
    while have < want:
        m = int((want - have) * 1.6) + 1024
        az = rng.uniform(0, 2 * np.pi, m)
        el = rng.uniform(np.deg2rad(-55.0), np.deg2rad(35.0), m)
        d = np.column_stack((np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)))
        t = np.full(m, np.inf)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.minimum(t, np.where(d[:, 2] < 0, -origin[2] / d[:, 2], np.inf))          # the ground, z = 0
            for b in _BOXES:                                                                  # slab test per block
                lo = np.array([b[0], b[2], 0.0]); hi = np.array([b[1], b[3], b[4]])
                t0 = (lo - origin) / d; t1 = (hi - origin) / d
                tn = np.nanmax(np.minimum(t0, t1), axis=1); tf = np.nanmin(np.maximum(t0, t1), axis=1)
                hit = (tn <= tf) & (tn > 0)
                t = np.where(hit, np.minimum(t, tn), t)
        ok = (t >= 2.0) & (t <= 80.0)
        P = origin + d[ok] * (t[ok] + rng.normal(0, 0.004, ok.sum()))[:, None]
        out.append(P); have += len(P)
    P = np.concatenate(out)[:want]
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return np.ascontiguousarray((P - origin) @ R)
