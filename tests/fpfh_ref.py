"""Reference of the FPFH descriptors (contract (F); include/simpleicp_hip_fpfh.h), built from the oracle's
brute-force k-NN (contracts (D) and (K)) and plain numpy float64 -- never from the code under test.  TEST INFRASTRUCTURE ONLY.

Every numpy operation below is one IEEE operation per element (numpy fuses nothing), so the expressions ARE the contract:
dot products as (a*b + c*d) + e*f, the sums of pass 2 as loops in rank order and in bin order.
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from oracle import orc  # noqa: E402

BINS = 33
# (c_j, s_j), j = 1 .. 10: SICP_FPFH_BORDERS of the header, the same literals
BORDERS = [tuple(float.fromhex(v) for v in pair) for pair in (
    ("-0x1.aeb8c8764f0bap-1", "-0x1.14cedf8bb580bp-1"),
    ("-0x1.a9628d9c712b6p-2", "-0x1.d1bb48eee2c13p-1"),
    ("0x1.2375f640f44dbp-3", "-0x1.fac9e043842efp-1"),
    ("0x1.4f49e7f775887p-1", "-0x1.82f19bb3a28a1p-1"),
    ("0x1.eb42a9bcd5057p-1", "-0x1.207e7fd768dbfp-2"),
    ("0x1.eb42a9bcd5057p-1", "0x1.207e7fd768dbfp-2"),
    ("0x1.4f49e7f775887p-1", "0x1.82f19bb3a28a1p-1"),
    ("0x1.2375f640f44dbp-3", "0x1.fac9e043842efp-1"),
    ("-0x1.a9628d9c712b6p-2", "0x1.d1bb48eee2c13p-1"),
    ("-0x1.aeb8c8764f0bap-1", "0x1.14cedf8bb580bp-1"))]


def dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def bin11(f):
    """min(10, max(0, floor(11 * ((f + 1) * 0.5)))) clamped in float64; a NaN gives 0."""
    t = np.floor(11.0 * ((np.asarray(f, dtype=np.float64) + 1.0) * 0.5))
    return np.where(t >= 10.0, 10.0, np.where(t > 0.0, t, 0.0)).astype(np.int64)


def sector(a, b):
    """How many of the ten borders the direction (b, a) has reached."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    below = np.zeros(a.shape, np.int64)
    above = np.full(a.shape, 5, np.int64)
    for j, (c, s) in enumerate(BORDERS):
        reached = (c * a - s * b) >= 0.0
        if j < 5:
            below = below + reached
        else:
            above = above + reached
    return np.where(a > 0.0, above, np.where(a < 0.0, below, np.where(b < 0.0, 0, 5)))


def pair_feature(p, n_p, q, n_q, d2):
    """The pair feature of (p, n_p) with (q, n_q): arrays (..., 3) and d2 (...).  Returns (void, bin of f1, 11 + bin of f2,
    22 + bin of f3, (f2, f3, a, b))."""
    p, n_p, q, n_q = (np.asarray(v, dtype=np.float64) for v in (p, n_p, q, n_q))
    d2 = np.asarray(d2, dtype=np.float64)
    with np.errstate(all="ignore"):
        dp = q - p
        dx, dy, dz = dp[..., 0], dp[..., 1], dp[..., 2]
        f4 = np.sqrt(d2)
        a1 = dot(n_p[..., 0], n_p[..., 1], n_p[..., 2], dx, dy, dz) / f4
        a2 = dot(n_q[..., 0], n_q[..., 1], n_q[..., 2], dx, dy, dz) / f4
        swap = np.abs(a1) < np.abs(a2)
        n1 = np.where(swap[..., None], n_q, n_p)
        n2 = np.where(swap[..., None], n_p, n_q)
        f3 = np.where(swap, -a2, a1)
        dx, dy, dz = np.where(swap, -dx, dx), np.where(swap, -dy, dy), np.where(swap, -dz, dz)
        n1x, n1y, n1z = n1[..., 0], n1[..., 1], n1[..., 2]
        n2x, n2y, n2z = n2[..., 0], n2[..., 1], n2[..., 2]
        vx, vy, vz = dy * n1z - dz * n1y, dz * n1x - dx * n1z, dx * n1y - dy * n1x
        vn = np.sqrt(dot(vx, vy, vz, vx, vy, vz))
        vx, vy, vz = vx / vn, vy / vn, vz / vn
        wx, wy, wz = n1y * vz - n1z * vy, n1z * vx - n1x * vz, n1x * vy - n1y * vx
        f2 = dot(vx, vy, vz, n2x, n2y, n2z)
        a = dot(wx, wy, wz, n2x, n2y, n2z)
        b = dot(n1x, n1y, n1z, n2x, n2y, n2z)
        void = (d2 == 0.0) | (vn == 0.0) | ~np.isfinite(n_p).all(axis=-1) | ~np.isfinite(n_q).all(axis=-1)
        return void, sector(a, b), 11 + bin11(f2), 22 + bin11(f3), (f2, f3, a, b)


def oriented(X, normals, viewpoint):
    """The normals as float64 (exact), turned towards the viewpoint where there is one."""
    X = np.asarray(X, dtype=np.float64)
    N = np.ascontiguousarray(normals, dtype=np.float32).astype(np.float64)
    if viewpoint is None:
        return N
    v = np.asarray(viewpoint, dtype=np.float64)
    with np.errstate(all="ignore"):
        s = dot(v[0] - X[:, 0], v[1] - X[:, 1], v[2] - X[:, 2], N[:, 0], N[:, 1], N[:, 2])
    return np.where((s < 0.0)[:, None], -N, N)


def in_radius(d2, radius):
    d2 = np.asarray(d2, dtype=np.float64)
    if np.isinf(radius):
        return np.ones(d2.shape, bool)
    return d2 < np.float64(radius) * np.float64(radius)


def spfh_counts(X, N, pts, idx, d2, radius):
    """(len(pts), 34) counts -- 33 bins and m -- and the number of ranks 1 .. k-1 within the radius, for the points `pts` with
    their ranked lists idx / d2 (len(pts), k)."""
    inside = in_radius(d2[:, 1:], radius)
    j = idx[:, 1:]
    void, b1, b2, b3, _ = pair_feature(X[pts][:, None, :], N[pts][:, None, :], X[j], N[j], d2[:, 1:])
    ok = inside & ~void
    counts = np.zeros((len(pts), BINS + 1), np.int64)
    rows = np.broadcast_to(np.arange(len(pts))[:, None], ok.shape)
    for b in (b1, b2, b3):
        np.add.at(counts, (rows[ok], b[ok]), 1)
    counts[:, BINS] = ok.sum(axis=1)
    return counts.astype(np.uint16), inside.sum(axis=1)


def spfh_values(counts):
    """S[b] = (100.0 * c[b]) / m, all zeros where m == 0."""
    c = counts[:, :BINS].astype(np.float64)
    m = counts[:, BINS].astype(np.float64)
    with np.errstate(all="ignore"):
        return np.where(m[:, None] > 0, (100.0 * c) / m[:, None], 0.0)


def fpfh(X, normals, k, radius=np.inf, viewpoint=None, rows=None):
    """Contract (F).  Returns dict(counts (m, 34) uint16, fpfh (m, 33) float32, and -- rows None -- n_points, n_pairs,
    n_void_pairs, n_empty).  rows: only these points (their neighbours' SPFH is formed too, nothing else)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    n = len(X)
    radius = np.inf if radius is None else float(radius)
    N = oriented(X, normals, viewpoint)
    want = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    idx, d2 = orc.knn(X, np.ascontiguousarray(X[want]), k=k)
    if rows is None:
        need, idx_need, d2_need = want, idx, d2
    else:
        need = np.unique(np.concatenate([want, idx[:, 1:].ravel()]))
        idx_need, d2_need = orc.knn(X, np.ascontiguousarray(X[need]), k=k)
    counts_need, inside_need = spfh_counts(X, N, need, idx_need, d2_need, radius)
    at = np.full(n, -1, np.int64)
    at[need] = np.arange(len(need))
    S = spfh_values(counts_need)
    m_need = counts_need[:, BINS]
    finite = np.isfinite(N).all(axis=1)
    inside = in_radius(d2, radius)
    W = np.zeros((len(want), BINS))
    for r in range(1, k):                                            # rank order
        j = idx[:, r]
        use = inside[:, r] & (d2[:, r] != 0.0) & finite[j]
        with np.errstate(all="ignore"):
            term = S[at[j]] / d2[:, r][:, None]
        W = np.where(use[:, None], W + term, W)
    F = np.empty((len(want), BINS))
    Si = S[at[want]]
    for g in (0, 11, 22):
        T = W[:, g].copy()
        for t in range(1, 11):                                       # bin order
            T = T + W[:, g + t]
        with np.errstate(all="ignore"):
            add = np.where((T > 0.0)[:, None], (W[:, g:g + 11] * 100.0) / T[:, None], 0.0)
        F[:, g:g + 11] = Si[:, g:g + 11] + add
    out = dict(counts=counts_need[at[want]], fpfh=F.astype(np.float32))
    if rows is None:
        m = m_need.astype(np.int64)
        out.update(n_points=n, n_pairs=int(m.sum()), n_void_pairs=int((inside_need - m).sum()), n_empty=int((m == 0).sum()))
    return out
