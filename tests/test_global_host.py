"""Descriptor matching and RANSAC poses (contracts (M) and (R)), the parts that need no GPU: the companion
header and the binding, the refusals that come before any device work, known answers of the references alone
(tests/global_ref.py), and the plumbing of match_features, ransac_pose and register_global on a stand-in context."""
import ctypes as C
import inspect
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import fpfh_ref
import global_ref
import oracle_backend

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "simpleicp_hip_global.h"


# ---- header, exports, binding ----
def test_header_names_are_exported_and_bound():
    from simpleicp_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(sicp_\w+)\s*\(", text))) == sorted(_lib.GLOBAL_EXPORTS) == [
        "sicp_feature_match", "sicp_global_version", "sicp_ransac_triplets"]
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", str(so)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sicp_\w+)", out))
    assert set(_lib.GLOBAL_EXPORTS) <= exported
    others = (set(_lib.EXPORTS) | set(_lib.BATCH_EXPORTS) | set(_lib.DEVICE_EXPORTS) | set(_lib.NORMALS_EXPORTS) | set(_lib.VOXEL_EXPORTS)
              | set(_lib.EVAL_EXPORTS) | set(_lib.OUTLIER_EXPORTS) | set(_lib.CHAIN_EXPORTS) | set(_lib.FPFH_EXPORTS))
    assert not set(_lib.GLOBAL_EXPORTS) & others
    L = _lib.load()
    # the version triple: the header's, the library's, the binding's
    assert "#define SICP_GLOBAL_VERSION 1" in HEADER.read_text()
    assert L.sicp_global_version() == _lib.GLOBAL_VERSION == 1 and _lib.global_version() == 1
    assert f"#define SICP_MATCH_MAX_DIM {_lib.MATCH_MAX_DIM}" in HEADER.read_text() and _lib.MATCH_MAX_DIM == 64
    assert C.sizeof(_lib.MatchStats) == 24 and C.sizeof(_lib.RansacStats) == 40
    assert _lib.FEATURES["global"].exports == _lib.GLOBAL_EXPORTS and _lib.FEATURES["global"].header == HEADER.name
    # the main header and its version are untouched, the other companions keep theirs
    assert L.sicp_abi_version() == _lib.ABI_VERSION == 7
    main = (ROOT / "include" / "simpleicp_hip.h").read_text().lower()
    assert "ransac" not in main and "feature_match" not in main and "global.h" not in main
    assert (_lib.BATCH_VERSION, _lib.DEVICE_VERSION, _lib.NORMALS_VERSION, _lib.VOXEL_VERSION, _lib.EVAL_VERSION, _lib.OUTLIER_VERSION,
            _lib.CHAIN_VERSION, _lib.FPFH_VERSION) == (1,) * 8
    for other in (ROOT / "include").glob("simpleicp_hip_*.h"):
        if other != HEADER:
            assert "ransac" not in other.read_text().lower()
    assert list(inspect.signature(_lib.Context.feature_match).parameters)[1:] == [
        "query", "target", "nq", "nt", "dim", "idx_ptr", "d2_ptr", "want_d2"]
    assert list(inspect.signature(_lib.Context.ransac_triplets).parameters)[1:] == [
        "src", "dst", "triples", "max_distance", "edge_ratio", "m", "h", "poses_ptr", "inliers_ptr", "want_poses"]
    assert any(p.name == "sicp_global.hip" for p in build.SOURCES) and any(p.name == HEADER.name for p in build.HEADERS)


def test_null_ctx_is_refused_not_dereferenced():
    from simpleicp_amd import _lib
    L = _lib.load()
    P = _lib._ptr
    q, idx, ms = np.zeros((4, 33), np.float32), np.full(4, 7, np.int32), _lib.MatchStats()
    assert L.sicp_feature_match(None, P(q), 4, P(q), 4, 33, P(idx), None, C.byref(ms)) == _lib.ERR_INVALID
    assert b"null ctx" in L.sicp_last_error() and np.all(idx == 7)
    X, tri, inl, rs = np.zeros((4, 3)), np.zeros((1, 3), np.int32), np.full(1, 7, np.int32), _lib.RansacStats()
    assert L.sicp_ransac_triplets(None, P(X), P(X), 4, P(tri), 1, 1.0, 0.9, None, P(inl), C.byref(rs)) == _lib.ERR_INVALID
    assert b"null ctx" in L.sicp_last_error() and np.all(inl == 7)


# ---- argument errors before the backend is touched ----
def test_python_argument_errors_come_before_the_backend(monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import backend

    def no_backend(*a, **k):
        raise AssertionError("the backend was called")
    monkeypatch.setattr(backend, "get_context", no_backend)
    for name in ("match_features", "ransac_pose", "register_global"):
        assert name in simpleicp_amd.__all__
    mf, rp, rg = simpleicp_amd.match_features, simpleicp_amd.ransac_pose, simpleicp_amd.register_global
    assert list(inspect.signature(mf).parameters) == ["query", "target", "mutual", "return_distance"]
    assert list(inspect.signature(rp).parameters) == ["src", "dst", "max_distance", "hypotheses", "edge_ratio", "seed", "triples", "top"]
    assert list(inspect.signature(rg).parameters) == ["fixed", "movable", "max_distance", "neighbors", "normal_neighbors",
                                                       "viewpoint_fixed", "viewpoint_movable", "mutual", "ransac_kwargs"]
    assert all(p.kind in (p.KEYWORD_ONLY, p.VAR_KEYWORD) for n, p in inspect.signature(rp).parameters.items() if n not in ("src", "dst"))
    F = np.zeros((5, 33), np.float32)
    with pytest.raises(TypeError, match="float32"):
        mf(F.astype(np.float64), F)
    with pytest.raises(TypeError, match="target"):
        mf(F, [[0.0] * 33])
    with pytest.raises(ValueError, match="same width"):
        mf(F, F[:, :32])
    with pytest.raises(ValueError, match="width"):
        mf(np.zeros((5, 65), np.float32), np.zeros((5, 65), np.float32))
    with pytest.raises(ValueError, match="shape"):
        mf(F[0], F)
    # an empty side has an empty or an all-unmatched answer and needs no backend
    assert mf(F[:0], F).shape == (0,) and np.array_equal(mf(F, F[:0], mutual=True), np.full(5, -1))
    X = np.random.default_rng(0).standard_normal((10, 3))
    for d in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_distance"):
            rp(X, X, max_distance=d)
    for d in ("far", None, True):
        with pytest.raises(TypeError, match="max_distance"):
            rp(X, X, max_distance=d)
    with pytest.raises(TypeError):
        rp(X, X)                                                      # max_distance has no default
    for h in (0, -5):
        with pytest.raises(ValueError, match="hypotheses"):
            rp(X, X, max_distance=1.0, hypotheses=h)
    with pytest.raises(TypeError, match="hypotheses"):
        rp(X, X, max_distance=1.0, hypotheses=10.0)
    for r in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError, match="edge_ratio"):
            rp(X, X, max_distance=1.0, edge_ratio=r)
    with pytest.raises(ValueError, match="top"):
        rp(X, X, max_distance=1.0, top=0)
    with pytest.raises(ValueError, match="seed"):
        rp(X, X, max_distance=1.0, seed=-1)
    with pytest.raises(ValueError, match="triples"):
        rp(X, X, max_distance=1.0, triples=np.zeros((4, 2), np.int32))
    with pytest.raises(TypeError, match="triples"):
        rp(X, X, max_distance=1.0, triples=np.zeros((4, 3)))
    with pytest.raises(ValueError, match="same number"):
        rp(X, X[:9], max_distance=1.0)
    with pytest.raises(ValueError, match="at least 3"):
        rp(X[:2], X[:2], max_distance=1.0)
    with pytest.raises(ValueError, match=r"\(m, 3\)"):
        rp(X[:, :2], X[:, :2], max_distance=1.0)
    with pytest.raises(TypeError, match="unexpected keyword"):
        rg(X, X, max_distance=1.0, hypothesis=10)
    with pytest.raises(ValueError, match="max_distance"):
        rg(X, X, max_distance=-1.0)
    with pytest.raises(ValueError, match="edge_ratio"):
        rg(X, X, max_distance=1.0, edge_ratio=2.0)
    with pytest.raises(ValueError, match="neighbors"):
        rg(X, X, max_distance=1.0, neighbors=1)


def test_a_distributed_job_is_refused(monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import backend, dist
    monkeypatch.setattr(backend, "get_context", lambda: (_ for _ in ()).throw(AssertionError("the backend was called")))
    monkeypatch.setattr(dist, "is_distributed", lambda: True)
    F, X = np.zeros((5, 33), np.float32), np.random.default_rng(0).standard_normal((10, 3))
    for call in (lambda: simpleicp_amd.match_features(F, F), lambda: simpleicp_amd.ransac_pose(X, X, max_distance=1.0),
                 lambda: simpleicp_amd.register_global(X, X, max_distance=1.0)):
        with pytest.raises(simpleicp_amd.SimpleICPException, match="does not run in a torch.distributed job"):
            call()


# ---- known answers of the references alone ----
def test_the_references_fma_is_the_c_librarys():
    libm = C.CDLL("libm.so.6")
    libm.fma.restype = C.c_double
    libm.fma.argtypes = [C.c_double] * 3
    rng = np.random.default_rng(0)
    n = 6000
    a = rng.standard_normal(n) * 10.0 ** rng.integers(-5, 5, n)
    b, c = rng.standard_normal(n), rng.standard_normal(n)
    c[:2000] = -(a[:2000] * b[:2000]) * (1 + rng.integers(-3, 4, 2000) * 2.0 ** -52)      # heavy cancellation
    c[2000:2500] = -(a[2000:2500] * b[2000:2500])
    a[2500:3000] = np.round(a[2500:3000] * 2 ** 20) / 2 ** 20                              # sums near a rounding boundary
    b[2500:3000] = 1 + 2.0 ** -30
    c[2500:3000] = 2.0 ** -53 * rng.integers(-3, 4, 500)
    got = global_ref.fma(a, b, c)
    want = np.array([libm.fma(x, y, z) for x, y, z in zip(a, b, c)])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert (got != a * b + c).sum() > 1000                           # (the test would pass with an unfused stand-in otherwise)
    assert np.isnan(global_ref.fma(np.nan, 1.0, 1.0)) and global_ref.fma(np.inf, 1.0, 1.0) == np.inf


def test_match_reference_by_hand():
    q = np.float32([[0, 0], [3, 4], [np.nan, 0], [1e30, 0]])
    g = np.float32([[3, 4], [0, 0], [0, 0], [np.nan, 1], [-1e30, 0]])
    idx, d2, rec = global_ref.match(q, g)
    # row 0: the tie between rows 1 and 2 goes to 1; row 2: every distance is NaN; row 3: (2e30)^2 overflows, 1e60 does too
    assert idx.tolist() == [1, 0, -1, -1] and d2.tolist() == [0.0, 0.0, np.inf, np.inf] and d2.dtype == np.float32
    assert rec == dict(n_query=4, n_target=5, n_unmatched=2)
    # column order: 1e8 + 1 - 1e8 style sums depend on it
    a = np.float32([[4096.0, 0.5, 0.5]])
    assert global_ref.match(a, np.zeros((1, 3), np.float32))[1][0] == np.float32(np.float32(4096.0 ** 2 + 0.25) + np.float32(0.25))
    assert global_ref.mutual([1, 0, -1, 2], [1, 0, 0]).tolist() == [1, 0, -1, -1]


def test_ransac_reference_known_answers():
    # an exactly representable pose: 90 degrees about z, integer coordinates
    src = np.array([[0, 0, 0], [2, 0, 0], [0, 3, 0], [1, 1, 5], [7, 7, 7]], float)
    Rz, t = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], float), np.array([10.0, -20.0, 30.0])
    dst = src @ Rz.T + t
    dst[4] += (0.0, 0.0, 0.5)
    P, inl, rec = global_ref.ransac(src, dst, [[0, 1, 2]], 0.5, 0.9)
    assert np.array_equal(P[0, :9].reshape(3, 3), Rz) and np.array_equal(P[0, 9:], t)
    assert inl.tolist() == [4] and rec == dict(n_hypotheses=1, n_void=0, n_pruned=0, best=0, best_inliers=4)      # 0.25 < 0.25 fails
    assert global_ref.ransac(src, dst, [[0, 1, 2]], np.nextafter(0.5, 1), 0.9)[1].tolist() == [5]
    # a collinear triple is void at any edge ratio: v' is exactly zero
    col = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0]], float)
    for ratio in (0.0, 0.9):
        P, inl, rec = global_ref.ransac(col, col, [[0, 1, 2]], 0.5, ratio)
        assert inl.tolist() == [-1] and not P.any() and not np.signbit(P).any() and (rec["n_void"], rec["best"], rec["best_inliers"]) == (1, -1, -1)
    # a scaled triangle is pruned at 0.9 and passes at 0
    assert global_ref.ransac(src, 2 * src, [[0, 1, 2]], 0.5, 0.9)[1].tolist() == [-2]
    assert global_ref.ransac(src, 2 * src, [[0, 1, 2]], 0.5, 0.0)[1].tolist() == [0]
    assert global_ref.ransac(src, 1.1 * src, [[0, 1, 2]], 0.5, 0.9)[1][0] >= 0                # 1 / 1.21 >= 0.81: not pruned
    assert global_ref.ransac(src, 1.2 * src, [[0, 1, 2]], 0.5, 0.9)[1].tolist() == [-2]          # 1 / 1.44 < 0.81
    # bad indices and repeats are void, nothing is read through them; ties go to the lower index
    tri = [[0, 1, 1], [-1, 1, 2], [0, 1, 5], [2, 1, 0], [0, 1, 2], [0, 1, 2]]
    P, inl, rec = global_ref.ransac(src, dst, tri, 0.5, 0.9)
    assert inl.tolist() == [-1, -1, -1, 4, 4, 4] and rec == dict(n_hypotheses=6, n_void=3, n_pruned=0, best=3, best_inliers=4)
    # a NaN coordinate in the triple: void; outside it: no inlier
    bad = src.copy()
    bad[1, 2] = np.nan
    assert global_ref.ransac(bad, dst, [[0, 1, 2], [0, 2, 3]], 0.5, 0.9)[1].tolist() == [-1, 3]


# ---- the plumbing on a stand-in context ----
class GlobalOracleContext(oracle_backend.OracleContext):
    """The entry points of the chain, answered by the numpy references."""

    def fpfh(self, slot, normals, k, radius=np.inf, viewpoint=None, fpfh_ptr=None, counts_ptr=None, want_counts=False):
        self._log("fpfh")
        r = fpfh_ref.fpfh(self.cloud[slot][0], normals, k, radius, viewpoint)
        return r["fpfh"], None, {}

    def feature_match(self, query, target, nq=None, nt=None, dim=None, idx_ptr=None, d2_ptr=None, want_d2=True):
        assert idx_ptr is None and query.dtype == target.dtype == np.float32
        self._log("feature_match")
        return global_ref.match(query, target)

    def ransac_triplets(self, src, dst, triples, max_distance, edge_ratio, m=None, h=None, poses_ptr=None, inliers_ptr=None,
                        want_poses=True):
        assert inliers_ptr is None and triples.dtype == np.int32
        self._log("ransac_triplets")
        self.ransac_args = (np.array(src), np.array(dst), np.array(triples), max_distance, edge_ratio)
        return global_ref.ransac(src, dst, triples, max_distance, edge_ratio)


@pytest.fixture
def octx(monkeypatch):
    from simpleicp_amd import backend
    ctx = GlobalOracleContext()
    monkeypatch.setattr(backend, "get_context", lambda: ctx)
    return ctx


def test_match_features_mutual(octx):
    import simpleicp_amd
    rng = np.random.default_rng(3)
    A, B = rng.standard_normal((40, 5)).astype(np.float32), rng.standard_normal((60, 5)).astype(np.float32)
    B[7] = A[3]
    idx = simpleicp_amd.match_features(A, B)
    assert octx.calls == ["feature_match"] and idx.dtype == np.int64 and np.array_equal(idx, global_ref.match(A, B)[0]) and idx[3] == 7
    octx.calls.clear()
    both, d2 = simpleicp_amd.match_features(A, B, mutual=True, return_distance=True)
    assert octx.calls == ["feature_match", "feature_match"]
    back = global_ref.match(B, A)[0]
    assert np.array_equal(both, global_ref.mutual(idx, back)) and both[3] == 7 and 0 < (both >= 0).sum() < 40
    assert d2.dtype == np.float32 and np.array_equal(d2, global_ref.match(A, B)[1])
    A[5] = np.nan                                                     # an unmatched row stays -1 through the gather
    assert simpleicp_amd.match_features(A, B, mutual=True)[5] == -1 and simpleicp_amd.match_features(A, B)[5] == -1


def _noisy_copy(rng, m, wrong):
    src = rng.uniform(-1, 1, (m, 3))
    c, s = np.cos(0.4), np.sin(0.4)
    R, t = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]), np.array([0.3, -0.2, 0.1])
    dst = src @ R.T + t + rng.normal(0, 0.002, (m, 3))
    bad = rng.choice(m, int(wrong * m), replace=False)
    dst[bad] = rng.uniform(-1, 1, (len(bad), 3))
    return src, dst, R, t


def test_ransac_pose_top_and_tie_order(octx):
    import simpleicp_amd
    src, dst, R, t = _noisy_copy(np.random.default_rng(5), 120, 0.3)
    res = simpleicp_amd.ransac_pose(src.astype(np.float32), dst, max_distance=0.02, hypotheses=300, seed=4, top=5)
    s32 = src.astype(np.float32).astype(np.float64)
    tri = np.random.default_rng(4).integers(0, 120, (300, 3), dtype=np.int32)
    assert np.array_equal(octx.ransac_args[0], s32) and np.array_equal(octx.ransac_args[2], tri) and octx.ransac_args[3:] == (0.02, 0.9)
    P, inl, rec = global_ref.ransac(s32, dst, tri, 0.02, 0.9)
    assert res.stats == rec and res.index == rec["best"] and res.inliers == rec["best_inliers"] > 60 and res.n_matches is None
    assert np.array_equal(res.H[:3, :3].ravel(), P[rec["best"], :9]) and np.array_equal(res.H[:3, 3], P[rec["best"], 9:])
    assert np.array_equal(res.H[3], [0, 0, 0, 1]) and np.abs(res.H[:3, :3] - R).max() < 0.05
    order = sorted(np.flatnonzero(inl >= 0), key=lambda k: (-inl[k], k))[:5]
    assert [c[2] for c in res.candidates] == order and [c[1] for c in res.candidates] == [int(inl[k]) for k in order]
    assert res.candidates[0][0] is res.H
    # the caller's triples: two identical ones tie, the lower index leads; void and pruned ones never appear
    mine = np.array([[5, 5, 6], tri[rec["best"]], tri[rec["best"]], [-1, 0, 1]])
    res = simpleicp_amd.ransac_pose(src, dst, max_distance=0.02, triples=mine, top=10)
    assert [c[2] for c in res.candidates] == [1, 2] and res.index == 1 and res.stats["n_void"] == 2
    # nothing valid: no pose
    res = simpleicp_amd.ransac_pose(src, dst, max_distance=0.02, triples=[[0, 0, 1]])
    assert res.H is None and res.inliers == -1 and res.index == -1 and res.candidates == [] and res.stats["best"] == -1


def test_register_global_is_the_three_calls(octx, monkeypatch):
    import simpleicp_amd
    rng = np.random.default_rng(8)
    g = np.linspace(-1, 1, 14)
    u, v = [a.ravel() for a in np.meshgrid(g, g)]
    fixed = np.column_stack([u, v, 0.3 * np.sin(3 * u) * np.cos(2 * v) + 0.2 * u * v]) + rng.normal(0, 1e-3, (196, 3))
    c, s = np.cos(0.5), np.sin(0.5)
    R, t = np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), np.array([0.5, 0.1, -0.4])
    movable = (fixed - t) @ R                                         # R movable + t = fixed
    res = simpleicp_amd.register_global(fixed, movable, max_distance=0.05, neighbors=12, normal_neighbors=8,
                                        viewpoint_fixed=(0, 0, 9), viewpoint_movable=tuple(R.T @ (np.array([0, 0, 9.0]) - t)),
                                        hypotheses=200, seed=1, top=3)
    assert octx.calls == ["upload", "estimate_normals", "fpfh"] * 2 + ["feature_match"] * 2 + ["ransac_triplets"]
    src, dst = octx.ransac_args[0], octx.ransac_args[1]
    assert res.n_matches == len(src) >= 3 and len(res.candidates) <= 3
    # the pairs are (movable point, its fixed partner): rows of the two clouds
    assert all((movable == p).all(axis=1).any() for p in src[:5]) and all((fixed == p).all(axis=1).any() for p in dst[:5])
    assert res.stats == global_ref.ransac(src, dst, octx.ransac_args[2], 0.05, 0.9)[2]
    # fewer than three matches: a result without a pose, and no RANSAC call
    octx.calls.clear()
    res = simpleicp_amd.register_global(fixed[:20], movable[100:120] * 50.0, max_distance=0.05, neighbors=5, normal_neighbors=5)
    if res.n_matches < 3:
        assert res.H is None and res.candidates == [] and "ransac_triplets" not in octx.calls
    from simpleicp_amd import _lib, backend
    monkeypatch.setattr(backend, "get_context", lambda: oracle_backend.OracleContext())      # a backend without the entry points
    with pytest.raises(_lib.BackendError, match="global registration"):
        simpleicp_amd.match_features(np.zeros((3, 2), np.float32), np.ones((3, 2), np.float32))
