"""Every kernel that walks a ball over the dense cell table, on the inputs where the walk's shared geometry (sicp_grid_dev.h:
ball_block, row_lb2, row_x_clip, row_records) can go wrong -- the clamps and the growth to the whole grid, the 1e-6 margins at cell
faces, a row exactly one radius away, grids of one cell or one layer, ties -- against a NumPy brute force that evaluates the
arithmetic contract exactly ((d2, index) ties to the lowest index).  Distances and indices must be EQUAL.  The two walks of
sicp_cluster (k_ball_union, k_ball_border) run on the radius filter's clouds: labels, core bytes and record must be EQUAL to
DBSCAN on the brute force's relation."""
import os
from fractions import Fraction

import numpy as np
import pytest

import cluster_ref

CASES = ["outside_near", "outside_far", "faces", "row_edge", "one_cell", "flat", "three_points", "lattice_ties"]
# walker -> (environment of its context, entry, k).  k-NN walkers take min(k, n): the entry rejects k > n, so the clouds of 3 and of
# 6 points run with k = n (and k = 2) and no (walker, case) pair is left out.
_GRID = {"SICP_KNN1": "grid", "SICP_BOXES": "2"}
_MANY = dict(_GRID, SICP_NN16_MIN_Q="1", SICP_ORDER_MIN_Q="1", SICP_COARSE_MIN_N="1", SICP_NN16F_MIN_Q="1", SICP_FAR_MOVE="1e9")
WALKERS = {
    "nn_wave": (_GRID, "knn", 1),
    "nn16": (dict(_MANY, SICP_NN16="exact"), "knn", 1),
    "nn16f_near": (dict(_MANY, SICP_NN16="near"), "knn", 1),
    "nn16f_far": (dict(_MANY, SICP_NN16="far"), "knn", 1),
    "nn16_g8": (dict(_MANY, SICP_NN16="exact", SICP_NN_GROUP="8"), "match", 1),
    "nn16f_near_g8": (dict(_MANY, SICP_NN16="near", SICP_NN_GROUP="8"), "match", 1),
    "nn16f_far_g8": (dict(_MANY, SICP_NN16="far", SICP_NN_GROUP="8"), "match", 1),
    "knn_rounds_k2": (dict(_GRID, SICP_KNN_SWEEP="0"), "knn", 2),
    "knn_rounds_k17": (dict(_GRID, SICP_KNN_SWEEP="0"), "knn", 17),
    "knn_sweep1_k2": (dict(_GRID, SICP_KNN_SWEEP="1", SICP_KNN_GROUP="1", SICP_KNN_BATCH="5"), "knn", 2),
    "knn_sweep1_k17": (dict(_GRID, SICP_KNN_SWEEP="1", SICP_KNN_GROUP="1", SICP_KNN_BATCH="5"), "knn", 17),
    "knn_sweep4_k2": (dict(_GRID, SICP_KNN_SWEEP="1", SICP_KNN_GROUP="4", SICP_KNN_BATCH="3"), "knn", 2),
    "knn_sweep4_k17": (dict(_GRID, SICP_KNN_SWEEP="1", SICP_KNN_GROUP="4", SICP_KNN_BATCH="3"), "knn", 17),
    "ball_count": (_GRID, "radius", 0),
    "cluster": (_GRID, "cluster", 0),
}
LATTICE = ("row_edge", "lattice_ties")
LATTICE_WIDE = 0.3125              # a radius between the lattice's spacing (0.25: neighbours exactly on the sphere) and its face diagonal
MATCH_KERNEL = {"nn_wave": "k_grid_nn", "nn16": "k_grid_nn16", "nn16f_near": "k_grid_nn16f", "nn16f_far": "k_grid_nn16f",
                "nn16_g8": "k_grid_nn16", "nn16f_near_g8": "k_grid_nn16f", "nn16f_far_g8": "k_grid_nn16f"}


# ---- the brute force ------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))          # (exact, then rounded once: what the device's fma returns)


def _d2_contract(p, q):
    dx, dy, dz = p[0] - q[0], p[1] - q[1], p[2] - q[2]
    return _fma(dz, dz, _fma(dy, dy, dx * dx))


def _plain_d2(P, q):
    d = P - q
    return d[:, 2] * d[:, 2] + (d[:, 1] * d[:, 1] + d[:, 0] * d[:, 0])      # within a few ulps of the contract's value


def brute_knn(P, Q, k):
    """(idx, d2), (Q, k): plain NumPy distances shortlist every point that can be among the k nearest (they are within 1e-15
    relative of the contract's), the contract's value -- fma rounded once -- then ranks the shortlist on (d2, index)."""
    idx, d2 = np.empty((len(Q), k), np.int64), np.empty((len(Q), k))
    for j, q in enumerate(Q):
        D = _plain_d2(P, q)
        kth = np.partition(D, k - 1)[k - 1]
        cand = np.flatnonzero(D <= kth * (1.0 + 1e-12) + 1e-300)
        ex = np.array([_d2_contract(P[i], q) for i in cand])
        order = np.lexsort((cand, ex))[:k]
        idx[j], d2[j] = cand[order], ex[order]
        keys = list(zip(d2[j], idx[j]))
        assert all(a < b for a, b in zip(keys, keys[1:]))          # one expected answer: the order on (d2, index) is strict
    return idx, d2


def brute_count(P, rows, r):
    """points of P (the candidate itself included) with contract d2 < r * r, per candidate row"""
    r2, out = r * r, np.empty(len(rows), np.int64)
    for j, row in enumerate(rows):
        D = _plain_d2(P, P[row])
        sure = D < r2 * (1.0 - 1e-12)
        edge = np.flatnonzero((D <= r2 * (1.0 + 1e-12)) & ~sure)
        out[j] = int(sure.sum()) + sum(1 for i in edge if _d2_contract(P[i], P[row]) < r2)
    return out


def brute_relation(P, r):
    """(n, n) bool: j is a neighbour of i iff the contract's d2 < r * r (i itself included), by brute_count's rule: plain NumPy
    distances decide, the exact value only the pairs within 1e-12 relative of r * r (d2 is symmetric in every bit: each once)"""
    r2, n = r * r, len(P)
    A = np.zeros((n, n), bool)
    for i in range(n):
        D = _plain_d2(P, P[i])
        A[i] = D < r2 * (1.0 - 1e-12)
        for j in np.flatnonzero((D <= r2 * (1.0 + 1e-12)) & ~A[i]):
            if j > i:
                A[i, j] = A[j, i] = _d2_contract(P[j], P[i]) < r2
    return A


def cluster_runs(case, PQ, r):
    """[(radius, relation, [min_points])] of the cluster walker: the radius filter's radius and, on the lattices, LATTICE_WIDE;
    min_points 1 (the labels are the relation's components, ranked by lowest index), the 75th percentile of the counts, and at
    LATTICE_WIDE 7 (an interior point has 7 neighbours, itself included: core; a face point 6: border; edges and corners: noise)"""
    runs = []
    for rad in (r, LATTICE_WIDE) if case in LATTICE else (r,):
        key = ("relation", case, PQ.tobytes(), rad)
        if key not in _REF:
            _REF[key] = brute_relation(PQ, rad)
        A = _REF[key]
        mps = {1, max(1, int(np.percentile(A.sum(axis=1), 75)))} | ({7} if rad == LATTICE_WIDE else set())
        runs.append((rad, A, sorted(mps)))
    return runs


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def _cloud(case):
    rng = np.random.default_rng(31)
    if case in ("outside_near", "outside_far", "faces"):
        return rng.uniform(0.0, 1.0, (1500, 3)) * np.array([4.0, 3.0, 2.0]) + np.array([10.0, -7.0, 1.0])
    if case in ("row_edge", "lattice_ties"):                       # spacing 1/4: lattice planes and mid-planes are representable
        g = np.arange(12) * 0.25
        return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + np.array([-1.0, 2.0, 0.5])
    if case == "one_cell":                                         # 6 points, two of them the corners of their box: dim = 1, 1, 1
        return np.concatenate(([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]], rng.uniform(0.1, 0.9, (4, 3))))
    if case == "flat":                                             # dim_z = 1
        return np.column_stack((rng.uniform(0, 6, 1500), rng.uniform(0, 5, 1500), np.full(1500, 0.5)))
    if case == "three_points":
        return np.array([[0.0, 0.0, 0.0], [1.0, 0.25, 0.0], [0.5, 2.0, 1.0]])
    raise KeyError(case)


def _queries(case, P, mn, h, dim):
    """at most 64 queries; (mn, h, dim): the grid the searched cloud is binned on, as far as the library reports it"""
    rng = np.random.default_rng(32)
    lo, hi = P.min(0), P.max(0)
    diag = float(np.linalg.norm(hi - lo))
    inside = lambda m: lo + rng.uniform(0.0, 1.0, (m, 3)) * (hi - lo)
    if case in ("outside_near", "outside_far"):                   # beyond each face of the box: the clamps, the growth to `all`
        out = []
        for f in ((0.1,) if case == "outside_near" else (100.0,)):
            for a in range(3):
                for side in (lo, hi):
                    for rep in range(3):
                        q = inside(1)[0]
                        q[a] = side[a] + (f * diag if side is hi else -f * diag)
                        out.append(q)
            out.append(hi + f * diag); out.append(lo - f * diag)  # ... and beyond a corner
        return np.array(out)
    if case == "faces":                                           # on cell faces and on the box's faces, and one ulp to either side
        out = []
        for a in range(3):
            at = [lo[a], hi[a]] + [mn[a] + float(i) * h for i in sorted({1, max(1, dim[a] // 2), max(1, dim[a] - 1)})]
            for c in at:
                for v in (c, np.nextafter(c, -np.inf), np.nextafter(c, np.inf)):
                    q = inside(1)[0]
                    q[a] = v
                    out.append(q)
        return np.array(out)[:64]
    if case == "row_edge":
        # (y, z) exactly d from a row's rectangle, d the distance of the answer: off a lattice plane by d along y with x, z on the
        # lattice (the nearest point is exactly d away, straight along y), and d below / above a cell face of the grid along y or z
        out = []
        for d in (0.125, 0.0625, 0.25):
            for i in (2, 5, 9):
                out.append(P[0] + np.array([0.25 * i, 0.25 * i + d, 0.25 * (i + 1)]))
                out.append(P[0] + np.array([0.25 * i, 0.25 * (i + 1), 0.25 * i - d]))
                for a in (1, 2):
                    face = mn[a] + float(min(i, max(1, dim[a] - 1))) * h
                    for v in (face - d, face + d):
                        q = P[0] + np.array([0.25 * i, 0.25 * 3, 0.25 * 4])
                        q[a] = v
                        out.append(q)
        return np.array(out)[:64]
    if case == "lattice_ties":                                    # mid-points of edges, faces and cubes: 2, 4, 8 equidistant neighbours
        out = []
        for off in ((0.125, 0, 0), (0, 0.125, 0), (0.125, 0.125, 0), (0, 0.125, 0.125), (0.125, 0.125, 0.125), (0, 0, 0)):
            for i in (0, 3, 6, 10):
                out.append(P[0] + 0.25 * np.array([i, (i * 5) % 11, (i * 7) % 11]) + np.array(off))
        return np.array(out)
    # one_cell, flat, three_points: inside, on the points themselves, outside on every side
    out = list(inside(8)) + list(P[:: max(1, len(P) // 6)][:6])
    for a in range(3):
        for s in (-1.0, 1.0):
            q = inside(1)[0]
            q[a] = (lo[a] if s < 0 else hi[a]) + s * (0.3 * diag + 0.125)
            out.append(q)
    return np.array(out)


def _radius(case, P):
    if case in ("row_edge", "lattice_ties"):
        return 0.25                                               # the lattice spacing: the strict `<` has points exactly on the sphere
    if case == "three_points":
        return 2.5
    return 0.35 * float(np.linalg.norm(P.max(0) - P.min(0))) / max(1.0, len(P) ** (1.0 / 3.0)) * 2.0


def probe_grid(c, slot, P):
    """(mn, h, dim) of the slot's grid from what the library reports: the cells a ball spans (outlier_radius_cells) are
    min(floor(2 r / h) + 3, dim) per axis -- dim from a huge radius, h from the radius at which the count steps from 3 to 4
    (bisection: h to an ulp or two; the `faces` case puts queries one ulp to either side as well).  h = None: no axis has 4 cells."""
    dim = c.outlier_radius_cells(slot, 1e30)[:3]
    mn, a = P.min(0), int(np.argmax(dim))
    if dim[a] < 4:
        return mn, None, dim
    lo_r, hi_r = 0.0, float(np.linalg.norm(P.max(0) - mn)) + 1.0
    for _ in range(200):
        mid = 0.5 * (lo_r + hi_r)
        if mid <= lo_r or mid >= hi_r:
            break
        if c.outlier_radius_cells(slot, mid)[a] >= 4:
            hi_r = mid
        else:
            lo_r = mid
    return mn, 2.0 * hi_r, dim


def _stand_in_grid(P):
    ex = P.max(0) - P.min(0)
    h = float(ex.max()) / 8.0 if ex.max() > 0 else None
    return P.min(0), h, tuple(int(e // h) + 1 for e in ex) if h else (1, 1, 1)


_REF = {}


def _reference(kind, case, P, Q, k, r=None):
    key = (kind, case, k, P.shape, Q.tobytes(), r)
    if key not in _REF:
        _REF[key] = brute_knn(P, Q, k) if kind == "knn" else brute_count(P, Q, r)
    return _REF[key]


@pytest.mark.parametrize("case", CASES)
def test_brute_force_has_one_answer_per_case(case):
    """No GPU: the brute force alone, on a stand-in grid -- every case has one expected answer under the tie rule (brute_knn
    asserts the strict order), ties included where the case is about them, and the exact and the plain distances agree."""
    P = _cloud(case)
    Q = _queries(case, P, *_stand_in_grid(P))
    assert 0 < len(Q) <= 64 and len(P) <= 2000
    for k in sorted({1, min(2, len(P)), min(17, len(P))}):
        idx, d2 = brute_knn(P, Q, k)
        assert np.all(idx >= 0) and np.all(np.diff(d2, axis=1) >= 0)
        assert np.allclose(d2, np.take_along_axis(np.array([_plain_d2(P, q) for q in Q]), idx, 1), rtol=1e-14, atol=0)
    if case == "lattice_ties":
        _, d2 = brute_knn(P, Q, 8)
        assert (d2[:, 0] == d2[:, 1]).sum() >= 16 and (d2[:, 0] == d2[:, 7]).sum() >= 4


def test_cluster_cases_reach_both_walks():
    """No GPU: on the stand-in grid, the cluster walker's settings give k_ball_union and k_ball_border work in every case -- core
    and border points everywhere, noise and more than one cluster in most -- and the lattices have their pairs exactly on the
    sphere, which must not unite."""
    with_noise = several = 0
    for case in CASES:
        P = _cloud(case)
        PQ = np.concatenate((P, _queries(case, P, *_stand_in_grid(P))))
        assert len(PQ) < 2000
        for rad, A, mps in cluster_runs(case, PQ, _radius(case, P)):
            assert np.array_equal(A, A.T) and A.diagonal().all()
            for mp in mps:
                ref = cluster_ref.cluster(PQ, rad, mp, A)
                print(case, rad, mp, cluster_ref.record(ref))
                if mp == 1:
                    assert ref["core"].all() and ref["n_clusters"] >= 1
            if case in LATTICE and rad == 0.25:
                on_sphere = sum(int((_plain_d2(PQ, q) == rad * rad).sum()) for q in PQ)      # (ordered pairs: each from both ends)
                one = cluster_ref.cluster(PQ, rad, 1, A)
                assert on_sphere > 9000 and one["n_clusters"] > 1600, (on_sphere, one["n_clusters"])
            elif case in LATTICE:
                seven = cluster_ref.cluster(PQ, rad, 7, A)
                assert seven["n_core"] > 0 and seven["n_border"] > 0 and seven["n_noise"] > 0, cluster_ref.record(seven)
            else:
                ref = cluster_ref.cluster(PQ, rad, mps[-1], A)       # (the 75th percentile)
                assert ref["n_core"] >= 1 and ref["n_border"] >= 1, (case, cluster_ref.record(ref))
                with_noise += ref["n_noise"] > 0
                several += ref["n_clusters"] > 1
    assert with_noise >= 4 and several >= 3, (with_noise, several)


# ---- the walkers ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def contexts():
    from simpleicp_amd import _lib
    made = {}

    def get(walker):
        env = WALKERS[walker][0]
        key = tuple(sorted(env.items()))
        if key not in made:
            os.environ.update(env)
            try:
                made[key] = _lib.Context(0)
            finally:
                for name in env:
                    del os.environ[name]
        return made[key]
    yield get
    for c in made.values():
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("walker", list(WALKERS))
def test_ball_walk_equals_brute_force(contexts, walker, case):
    from simpleicp_amd import _lib
    c = contexts(walker)
    _, entry, k = WALKERS[walker]
    P = _cloud(case)
    n = len(P)
    c.upload(_lib.MOV, P)
    Q = _queries(case, P, *probe_grid(c, _lib.MOV, P))
    if case == "one_cell":
        assert c.outlier_radius_cells(_lib.MOV, 1e30)[:3] == (1, 1, 1)
    if case == "flat":
        assert c.outlier_radius_cells(_lib.MOV, 1e30)[2] == 1
    if entry == "knn":
        k = min(k, n)
        c.timing_enable(True, count_work=True); c.timing_reset()
        idx, d2 = c.knn(_lib.MOV, Q, k=k)
        ridx, rd2 = _reference("knn", case, P, Q, k)
        print(walker, case, "k", k, "index mismatches", int((idx != ridx).sum()), "distance mismatches", int((d2 != rd2).sum()))
        assert np.array_equal(idx, ridx)
        assert np.array_equal(d2, rd2)
        if k == 1:
            assert c.last_match_kernel() == MATCH_KERNEL[walker]
        else:
            assert (c.knn_work()["sweeps"] > 0) == ("sweep" in walker)
    elif entry == "match":
        # eight lanes per query exist on the iteration's match only: the queries are the fixed cloud's points, the answer is the
        # index list (the entry returns point-to-plane distances, not d2)
        c.upload(_lib.FIX, Q)
        c.icp_setup(np.arange(len(Q)), np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (len(Q), 1)), np.ones(len(Q), np.float32))
        idx, _ = c.corr_match()
        ridx, _ = _reference("knn", case, P, Q, 1)
        print(walker, case, "index mismatches", int((idx != ridx[:, 0]).sum()))
        assert np.array_equal(idx, ridx[:, 0])
        assert c.last_match_kernel() == MATCH_KERNEL[walker]
    else:
        # the radius filter's candidates are points of the slot: the queries join the cloud (placed on the grid of the cloud that
        # already holds as many points -- the box's faces are then the queries' own where they lie outside)
        r = _radius(case, P)
        rows = np.arange(n, n + len(Q))
        for _ in range(2):
            PQ = np.concatenate((P, Q))
            c.upload(_lib.MOV, PQ)
            Q = _queries(case, P, *probe_grid(c, _lib.MOV, PQ))
        PQ = np.concatenate((P, Q))
        c.upload(_lib.MOV, PQ)
        while c.outlier_radius_cells(_lib.MOV, r)[3] > _lib.OUTLIER_MAX_BOX_CELLS:
            r *= 0.5                                               # (the entry bounds the box a ball may span)
        if entry == "radius":
            keep, cnt, kept = c.outlier_radius(_lib.MOV, r, len(PQ), rows=rows)
            want = _reference("count", case, PQ, rows, 0, r)
            print(walker, case, "r", r, "count mismatches", int((cnt != want).sum()))
            assert np.array_equal(cnt.astype(np.int64), want)
            assert not keep.any() and kept == 0                    # (min_points = n: nobody has more than n neighbours)
            return
        # the two walks of sicp_cluster over every point of the joined cloud
        assert len(PQ) < 2000
        for rad, A, mps in cluster_runs(case, PQ, r):
            assert c.outlier_radius_cells(_lib.MOV, rad)[3] <= _lib.OUTLIER_MAX_BOX_CELLS
            for mp in mps:
                labels, core, st = c.cluster(_lib.MOV, rad, mp)
                ref = cluster_ref.cluster(PQ, rad, mp, A)
                print(walker, case, "r", rad, "min_points", mp, "label mismatches", int((labels != ref["labels"]).sum()),
                      "core mismatches", int((core != ref["core"]).sum()), st.as_dict(), cluster_ref.record(ref))
                assert np.array_equal(labels, ref["labels"])
                assert np.array_equal(core, ref["core"])
                assert st.as_dict() == cluster_ref.record(ref)
                # ... and the walker agrees with the radius filter's walk on the same cloud
                keep, _, kept = c.outlier_radius(_lib.MOV, rad, mp - 1)
                assert np.array_equal(keep, core) and kept == ref["n_core"]
