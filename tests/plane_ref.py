"""Reference of the planes of a cloud (contracts (P) and (Q); include/simpleicp_hip_plane.h), built from
global_ref.fma, eval_ref.tree_sum and plain numpy float64 -- never from the code under test.  TEST INFRASTRUCTURE ONLY.

Every numpy operation below is one IEEE operation per element (numpy fuses nothing), so the expressions ARE the contract, one
per contract line.  jacobi3 is simpleicp_amd/csrc/sicp_normals.h's transcribed for one matrix, its eigenvectors included
(iss_ref.jacobi3 is the same iteration but keeps the diagonal only).
"""
import numpy as np

import eval_ref
import global_ref

KEYS = ("n_points", "n_candidates", "n_hypotheses", "n_void", "best", "best_inliers")
REFIT_KEYS = ("n_planes", "n_void", "n_improved", "best", "best_inliers")
MAX_ROUNDS = 16


def candidates(X, mask):
    """The candidate rows as a bool vector: mask != 0, every row for None."""
    return np.ones(len(X), bool) if mask is None else np.asarray(mask) != 0


def residual(P, X):
    """r = fma(c, z, fma(b, y, a * x)) + d for the planes P (..., 4) against the rows X (n, 3): (..., n)."""
    P = np.asarray(P, dtype=np.float64)
    a, b, c, d = (P[..., j, None] for j in range(4))
    with np.errstate(all="ignore"):
        return global_ref.fma(c, X[:, 2], global_ref.fma(b, X[:, 1], a * X[:, 0])) + d


def inlier_mask(plane, X, cand, max_distance):
    """The inliers of one plane: candidate rows with fabs(r) < max_distance (strict, a NaN fails)."""
    with np.errstate(all="ignore"):
        return cand & (np.abs(residual(plane, X)) < float(max_distance))


def planes(X, mask, triples):
    """(valid (h,) bool, P (h, 4)) -- contract (P), steps 1 and 2; P is four +0.0 for a void hypothesis."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    tri = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    n, cand = len(X), candidates(X, mask)
    in_range = ((tri >= 0) & (tri < n)).all(axis=1)
    distinct = (tri[:, 0] != tri[:, 1]) & (tri[:, 0] != tri[:, 2]) & (tri[:, 1] != tri[:, 2])
    there = in_range & distinct
    j = np.where(there[:, None], tri, 0)                              # (nothing is dereferenced through a bad index)
    there &= cand[j].all(axis=1)                                      # (after the index checks: a masked-out vertex)
    p0, p1, p2 = X[j[:, 0]], X[j[:, 1]], X[j[:, 2]]
    with np.errstate(all="ignore"):
        u, v = p1 - p0, p2 - p0
        w = global_ref._cross(u, v)
        length = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
        nrm = w / length[:, None]
        d = -((nrm[:, 0] * p0[:, 0] + nrm[:, 1] * p0[:, 1]) + nrm[:, 2] * p0[:, 2])
    P = np.concatenate([nrm, d[:, None]], axis=1)
    valid = there & np.isfinite(P).all(axis=1)
    return valid, np.where(valid[:, None], P, 0.0)


def count_inliers(P, X, cand, max_distance):
    """Step 3 for the planes P (k, 4): the candidate rows with fabs(r) < max_distance, as exact integers."""
    out = np.empty(len(P), np.int64)
    Xc = np.ascontiguousarray(X[cand])                                # (a row that is no candidate never counts)
    with np.errstate(all="ignore"):
        for lo in range(0, len(P), 128):
            out[lo:lo + 128] = (np.abs(residual(P[lo:lo + 128], Xc)) < float(max_distance)).sum(axis=1)
    return out


def best_of(inl):
    """(best, best_inliers): the lowest index among the largest counts >= 0; (-1, -1) if there is none."""
    have = inl >= 0
    if not have.any():
        return -1, -1
    top = int(inl.max())
    return int(np.flatnonzero(inl == top)[0]), top


def triplets(X, mask, triples, max_distance):
    """(planes (h, 4) float64, inliers (h,) int32, record) of contract (P)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    cand = candidates(X, mask)
    valid, P = planes(X, mask, triples)
    inl = np.full(len(P), -1, np.int32)
    if valid.any():
        inl[valid] = count_inliers(P[valid], X, cand, max_distance)
    best, best_inliers = best_of(inl)
    rec = dict(n_points=len(X), n_candidates=int(cand.sum()), n_hypotheses=len(P), n_void=int((~valid).sum()), best=best,
               best_inliers=best_inliers)
    return P, inl, rec


def jacobi3(A):
    """sicp_normals.h's jacobi3 on one symmetric 3 x 3 matrix: (a, v) as it leaves them -- the diagonal of a holds the eigenvalues,
    the columns of v the eigenvectors."""
    a, v = np.array(A, dtype=np.float64), np.eye(3)
    with np.errstate(all="ignore"):
        for _ in range(64):
            off = (np.abs(a[0, 1]) + np.abs(a[0, 2])) + np.abs(a[1, 2])
            if off == 0.0:
                break
            for p, q in ((0, 1), (0, 2), (1, 2)):
                r = 3 - p - q
                if a[p, q] == 0.0:
                    continue
                theta = (a[q, q] - a[p, p]) / (np.float64(2.0) * a[p, q])
                t = np.float64(1.0 if theta >= 0 else -1.0) / (np.abs(theta) + np.sqrt(theta * theta + np.float64(1.0)))
                c = np.float64(1.0) / np.sqrt(t * t + np.float64(1.0))
                s = t * c
                apq = a[p, q]
                a[p, p] = a[p, p] - t * apq
                a[q, q] = a[q, q] + t * apq
                a[p, q] = a[q, p] = 0.0
                arp, arq = a[r, p], a[r, q]
                a[r, p] = a[p, r] = c * arp - s * arq
                a[r, q] = a[q, r] = s * arp + c * arq
                for i in range(3):
                    vip, viq = v[i, p], v[i, q]
                    v[i, p] = c * vip - s * viq
                    v[i, q] = s * vip + c * viq
    return a, v


def fit_masked(X, m, cur):
    """One round under the mask m of the current plane cur (contract (Q), step 1): the plane (4,), or None if it yields nothing."""
    k = int(np.count_nonzero(m))
    if k < 3:
        return None
    with np.errstate(all="ignore"):
        c = np.array([eval_ref.tree_sum(np.where(m, X[:, j], 0.0)) for j in range(3)]) / np.float64(k)
        dx, dy, dz = X[:, 0] - c[0], X[:, 1] - c[1], X[:, 2] - c[2]
        s = [eval_ref.tree_sum(np.where(m, t, 0.0)) for t in (dx * dx, dx * dy, dx * dz, dy * dy, dy * dz, dz * dz)]
        a, v = jacobi3([[s[0], s[1], s[2]], [s[1], s[3], s[4]], [s[2], s[4], s[5]]])
        lo = 0
        if a[1, 1] < a[lo, lo]:
            lo = 1
        if a[2, 2] < a[lo, lo]:
            lo = 2
        nx, ny, nz = v[0, lo], v[1, lo], v[2, lo]
        length = np.sqrt((nx * nx + ny * ny) + nz * nz)
        nx, ny, nz = nx / length, ny / length, nz / length
        if (nx * cur[0] + ny * cur[1]) + nz * cur[2] < 0:
            nx, ny, nz = -nx, -ny, -nz
        d = -((nx * c[0] + ny * c[1]) + nz * c[2])
    out = np.array([nx, ny, nz, d], dtype=np.float64)
    return out if np.isfinite(out).all() else None


def refit(X, mask, planes_in, max_distance, rounds, want_keep=False, rounds_run=None):
    """(planes_out (b, 4) float64, inliers_out (b,) int32, keep (n,) bool or None, record) of contract (Q).  rounds_run (a list):
    gets, per plane that is not void, the number of rounds that yielded a plane of their own."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    cand = candidates(X, mask)
    P = np.ascontiguousarray(planes_in, dtype=np.float64).reshape(-1, 4)
    out, inl = np.zeros_like(P), np.full(len(P), -1, np.int32)
    n_void = n_improved = 0
    for k, plane in enumerate(P):
        if not np.isfinite(plane).all():
            n_void += 1
            continue
        cur = plane.copy()
        m = inlier_mask(cur, X, cand, max_distance)
        first = int(m.sum())
        best, best_n, ran = cur, first, 0
        for _ in range(int(rounds)):
            new = fit_masked(X, m, cur)
            if new is None:
                break
            ran += 1
            if np.array_equal(new.view(np.uint64), cur.view(np.uint64)):
                break                                                 # (every further round would repeat it)
            cur = new
            m = inlier_mask(cur, X, cand, max_distance)
            if int(m.sum()) > best_n:                                 # (strict: the earliest plane wins a tie)
                best, best_n = cur, int(m.sum())
        out[k], inl[k] = best, best_n
        if rounds_run is not None:
            rounds_run.append(ran)
        n_improved += int(best_n > first)
    keep = None
    if want_keep:
        assert len(P) == 1
        keep = inlier_mask(out[0], X, cand, max_distance) if inl[0] >= 0 else np.zeros(len(X), bool)
    best, best_inliers = best_of(inl)
    return out, inl, keep, dict(n_planes=len(P), n_void=n_void, n_improved=n_improved, best=best, best_inliers=best_inliers)


# ---- the Python calls, from the two contracts ----
def draw_triples(n, mask, hypotheses, seed):
    """The triples segment_plane draws: default_rng(seed).integers(0, n, ...) without a mask, integers(0, k, ...) mapped through
    the ascending indices of the k candidate rows with one."""
    rng = np.random.default_rng(seed)
    if mask is None:
        return rng.integers(0, n, (hypotheses, 3), dtype=np.int32)
    rows = np.flatnonzero(np.asarray(mask) != 0)
    return rows[rng.integers(0, len(rows), (hypotheses, 3), dtype=np.int32)].astype(np.int32)


def segment_plane(X, max_distance, hypotheses=1024, seed=0, refine=3, mask=None):
    """(plane (4,), inliers (n,) bool, n_inliers) as segment_plane gives them; None if no hypothesis is valid."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    tri = draw_triples(len(X), mask, hypotheses, seed)
    P, inl, rec = triplets(X, mask, tri, max_distance)
    if rec["best"] < 0:
        return None
    out, cnt, keep, _ = refit(X, mask, P[rec["best"]:rec["best"] + 1], max_distance, refine, want_keep=True)
    return out[0], keep, int(cnt[0])


def segment_planes(X, max_distance, max_planes, min_inliers, hypotheses=1024, seed=0, refine=3):
    """(labels (n,) int32, planes (k, 4)) as segment_planes gives them."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    labels, found = np.full(len(X), -1, np.int32), []
    for j in range(max_planes):
        left = labels == -1
        if left.sum() < 3:
            break
        r = segment_plane(X, max_distance, hypotheses, [seed, j], refine, left)
        if r is None or r[2] < min_inliers:
            break
        labels[r[1]] = j
        found.append(r[0])
    return labels, np.array(found, dtype=np.float64).reshape(-1, 4)


# ---- scenes ----
def plane_scene(seed, n_plane, n_clutter, normal=(0.2, -0.3, 1.0), offset=1.5, extent=10.0, noise=0.0125):
    """n_plane points on a square patch (side 2 * extent) of the plane normal . x = offset, each moved along the unit normal by a
    uniform amount of at most `noise`, and n_clutter points uniform in the cube of that half side, shuffled:
    (X (n, 3), on_plane (n,) bool, unit normal (3,), offset)."""
    rng = np.random.default_rng(seed)
    nrm = np.asarray(normal, dtype=np.float64)
    nrm = nrm / np.linalg.norm(nrm)
    e1 = np.cross(nrm, [1.0, 0.0, 0.0] if abs(nrm[0]) < 0.9 else [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(nrm, e1)
    uv = rng.uniform(-extent, extent, (n_plane, 2))
    on = offset * nrm + uv[:, :1] * e1 + uv[:, 1:] * e2 + rng.uniform(-noise, noise, (n_plane, 1)) * nrm
    X = np.vstack([on, rng.uniform(-extent, extent, (n_clutter, 3))])
    flag = np.arange(len(X)) < n_plane
    order = rng.permutation(len(X))
    return np.ascontiguousarray(X[order]), flag[order], nrm, float(offset)


def tilting_scene():
    """(X (420, 3), P (1, 4)): the plane z = 0 holds all 420 rows within 0.1; their least-squares plane tilts towards the two
    groups of 200 at (x = +10, z = +0.09) and (x = -10, z = -0.09) and loses the 20 rows at (x = +10, z = -0.09)."""
    rng = np.random.default_rng(41)

    def group(k, x, z):
        return np.column_stack([x + rng.uniform(-0.5, 0.5, k), rng.uniform(-5.0, 5.0, k), np.full(k, z)])
    X = np.vstack([group(200, 10.0, 0.09), group(200, -10.0, -0.09), group(20, 10.0, -0.09)])
    return np.ascontiguousarray(X[rng.permutation(len(X))]), np.array([[0.0, 0.0, 1.0, 0.0]])


def two_plane_scene(seed=51):
    """2 000 rows: a large plane (900), a smaller one across it (500), clutter (600) -- what segment_planes peels in two rounds."""
    A = plane_scene(seed, 900, 300)[0]
    B = plane_scene(seed + 1, 500, 300, normal=(1.0, 0.1, 0.2), offset=-2.0)[0]
    X = np.vstack([A, B])
    return np.ascontiguousarray(X[np.random.default_rng(seed).permutation(len(X))])
