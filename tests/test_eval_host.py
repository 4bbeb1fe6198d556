"""Evaluation (contract (E)), the parts that need no GPU: the reference's own properties (tests/eval_ref.py),
the companion header and the binding, the refusals that need no context, Evaluation.information, and run()'s host plumbing on the
stand-in backend of tests/oracle_backend.py."""
import ctypes as C
import inspect
import logging
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import eval_ref
import oracle_backend

ROOT = Path(__file__).resolve().parent.parent
U = 2.0 ** -53


class EvalOracleContext(oracle_backend.OracleContext):
    """The stand-in with the one new entry point, answered by the numpy reference."""

    def evaluate(self, query_slot, search_slot, H=None, max_distance=np.inf, rows=None):
        from simpleicp_amd import _lib
        self._log("evaluate")
        self.eval_args = (query_slot, search_slot, None if H is None else np.array(H, dtype=float), float(max_distance), rows)
        r = eval_ref.evaluate(self.cloud[query_slot][0], self.cloud[search_slot][0], H, max_distance, rows)
        return _lib.EvalRecord(r["n_queries"], r["n_inliers"], r["sums"][0], (C.c_double * 3)(*r["sums"][1:4]),
                               (C.c_double * 6)(*r["sums"][4:10]))


@pytest.fixture
def ectx(monkeypatch):
    from simpleicp_amd import backend
    ctx = EvalOracleContext()
    monkeypatch.setattr(backend, "get_context", lambda: ctx)
    return ctx


# ---- the reference's own properties ----
def test_tree_is_within_the_pairwise_bound_of_the_exact_sum():
    """Pairwise summation over a tree of depth ceil(log2 P): every term passes through at most that many rounded additions, so
    |tree - exact| <= depth * u * sum|t| to first order; one more u covers the second-order terms and fsum's own rounding."""
    rng = np.random.default_rng(1)
    for n in (1, 2, 3, 63, 64, 65, 1000, 4097, 70_001):
        for t in (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 6, n), rng.uniform(1e6, 1e6 + 1, n) ** 2):
            P = 1
            while P < n:
                P *= 2
            bound = (math.ceil(math.log2(P)) + 1) * U * math.fsum(np.abs(t))
            assert abs(eval_ref.tree_sum(t) - math.fsum(t)) <= bound


def test_tree_depends_on_the_order_and_not_on_explicit_padding():
    t = np.array([1e16, 1.0, -1e16, 1.0])                          # (1e16 + 1) + (-1e16 + 1) = 0: both ones are lost
    assert eval_ref.tree_sum(t) == 0.0
    assert eval_ref.tree_sum(t[[0, 2, 1, 3]]) == 2.0               # (1e16 - 1e16) + (1 + 1)
    assert eval_ref.tree_sum(t).tobytes() != eval_ref.tree_sum(t[[0, 2, 1, 3]]).tobytes()
    rng = np.random.default_rng(2)
    for n in (1, 5, 64, 100, 1025):
        v = rng.standard_normal(n) * 1e3
        for pad in (1, 3, 64, 1000):
            assert eval_ref.tree_sum(np.concatenate([v, np.zeros(pad)])).tobytes() == eval_ref.tree_sum(v).tobytes()
    assert eval_ref.tree_sum([]) == 0.0 and not np.signbit(eval_ref.tree_sum([]))


def test_terms_of_the_reference():
    X = np.array([[1.0, 2.0, 3.0], [-0.5, 0.25, 4.0], [7.0, 8.0, 9.0]])
    t = eval_ref.terms(X, np.array([4, -1, 0]), np.array([0.5, np.inf, 2.0]))
    assert np.array_equal(t[0], [0.5, 1, 2, 3, 1, 4, 9, 2, 3, 6])
    assert np.array_equal(t[1], np.zeros(10)) and not np.signbit(t[1]).any()
    r = eval_ref.record(t, np.array([True, False, True]))
    assert r["n_queries"] == 3 and r["n_inliers"] == 2 and r["sums"][0] == 2.5 and r["sums"][9] == 78.0


# ---- header, exports, binding ----
def _header_functions():
    text = (ROOT / "include" / "simpleicp_hip_eval.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sicp_\w+)\s*\(", text)))


def test_header_names_are_exported_and_bound():
    from simpleicp_amd import _lib, build
    assert _header_functions() == sorted(_lib.EVAL_EXPORTS)
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", str(so)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sicp_\w+)", out))
    assert set(_lib.EVAL_EXPORTS) <= exported
    others = (set(_lib.EXPORTS) | set(_lib.BATCH_EXPORTS) | set(_lib.DEVICE_EXPORTS) | set(_lib.NORMALS_EXPORTS)
              | set(_lib.VOXEL_EXPORTS))
    assert not set(_lib.EVAL_EXPORTS) & others
    L = _lib.load()
    assert L.sicp_eval_version() == _lib.EVAL_VERSION == 1 and _lib.eval_version() == 1
    header = (ROOT / "include" / "simpleicp_hip_eval.h").read_text()
    assert "#define SICP_EVAL_VERSION 1" in header
    # the record: the header's fields in the header's order, 96 bytes
    body = re.search(r"typedef struct sicp_eval \{(.*?)\} sicp_eval;", re.sub(r"/\*.*?\*/", "", header, flags=re.S), re.S).group(1)
    names = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body)
    assert names == [f[0] for f in _lib.EvalRecord._fields_] == ["n_queries", "n_inliers", "sum_d2", "sum_p", "sum_pp"]
    assert C.sizeof(_lib.EvalRecord) == 96
    # the main header and its version are untouched, the other companions keep theirs
    assert L.sicp_abi_version() == _lib.ABI_VERSION == 7
    assert "sicp_eval" not in (ROOT / "include" / "simpleicp_hip.h").read_text()
    assert (_lib.BATCH_VERSION, _lib.DEVICE_VERSION, _lib.NORMALS_VERSION, _lib.VOXEL_VERSION) == (1, 1, 1, 1)
    assert callable(_lib.Context.evaluate)
    assert list(inspect.signature(_lib.Context.evaluate).parameters) == ["self", "query_slot", "search_slot", "H", "max_distance", "rows"]


def test_a_stale_library_is_reported(monkeypatch):
    from simpleicp_amd import _lib

    class Old:
        pass
    monkeypatch.setattr(_lib, "load", lambda: Old())
    with pytest.raises(_lib.BackendError, match="simpleicp_hip_eval.h"):
        _lib.eval_version()


def test_null_arguments_are_refused_not_dereferenced():
    """no ctx, so nothing may be touched: the refusals that need no device"""
    from simpleicp_amd import _lib
    L = _lib.load()
    _lib.eval_version()
    rec = _lib.EvalRecord()
    assert L.sicp_evaluate(None, 0, 1, None, 0, None, 1.0, C.byref(rec)) == _lib.ERR_INVALID
    assert b"null ctx" in L.sicp_last_error()
    assert L.sicp_evaluate(None, 0, 1, None, 0, None, 1.0, None) == _lib.ERR_INVALID


# ---- refusals before any backend call ----
@pytest.mark.parametrize("d", [-1.0, float("nan"), "far", {}, [1.0, 2.0]])
def test_bad_distance_is_refused_before_any_backend_call(d, monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import PointCloud, SimpleICP, SimpleICPException, backend

    def no_backend(*a, **k):
        raise AssertionError("the backend was called")
    monkeypatch.setattr(backend, "get_context", no_backend)
    monkeypatch.setattr(backend, "get_batch_contexts", no_backend)
    X = np.random.default_rng(0).standard_normal((50, 3))
    icp = SimpleICP(verbose=False)
    icp.add_point_clouds(PointCloud(X, columns=["x", "y", "z"]), PointCloud(X, columns=["x", "y", "z"]))
    icp.evaluate_distance = d
    with pytest.raises(SimpleICPException, match="evaluate_distance"):
        icp.run()
    with pytest.raises(SimpleICPException, match="evaluate_distance"):
        simpleicp_amd.run_batch([(X, X)], evaluate_distance=d)
    with pytest.raises(SimpleICPException, match="evaluate_distance"):
        simpleicp_amd.run_batch([(X, X)], per_pair=[{"evaluate_distance": d}])
    with pytest.raises(SimpleICPException, match="evaluate_distance"):
        simpleicp_amd.run_tensors(X, X, evaluate_distance=d)
    with pytest.raises(ValueError, match="max_distance"):
        simpleicp_amd.evaluate_registration(X, X, np.eye(4), d)


def test_keywords_accepted_and_misspelt_ones_refused(monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import SimpleICP, backend, batch, cli

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached
    monkeypatch.setattr(backend, "get_batch_contexts", stop)
    X = np.random.default_rng(0).standard_normal((50, 3))
    for fn in (simpleicp_amd.run_batch, simpleicp_amd.run_tensors):
        assert "evaluate_distance" in inspect.signature(fn).parameters
    assert batch._EXTRA_DEFAULTS["evaluate_distance"] is None and "evaluate_distance" not in batch._RUN_DEFAULTS
    assert SimpleICP.evaluate_distance is None and SimpleICP(verbose=False).evaluation is None
    assert "evaluate_distance" not in inspect.signature(SimpleICP.run).parameters    # run()'s signature is the reference's
    assert list(inspect.signature(simpleicp_amd.evaluate_registration).parameters) == ["fix", "mov", "H", "max_distance", "of"]
    with pytest.raises(Reached):                                   # accepted: the call gets as far as the device
        simpleicp_amd.run_batch([(X, X)], evaluate_distance=0.5)
    with pytest.raises(Reached):
        simpleicp_amd.run_batch([(X, X)], per_pair=[{"evaluate_distance": np.inf}])
    with pytest.raises(TypeError, match="evaluate_distanse"):
        simpleicp_amd.run_batch([(X, X)], evaluate_distanse=0.5)
    with pytest.raises(TypeError, match="torch.Tensor"):           # accepted: refused for the clouds, not for the keyword
        simpleicp_amd.run_tensors(X, X, evaluate_distance=0.5)
    with pytest.raises(ValueError, match="of must be"):
        simpleicp_amd.evaluate_registration(X, X, np.eye(4), 1.0, of="both")
    with pytest.raises(ValueError, match="H must be"):
        simpleicp_amd.evaluate_registration(X, X, np.eye(3), 1.0)
    assert simpleicp_amd.BatchResult().evaluation is None
    ap = cli.build_parser()
    assert ap.parse_args(["-f", "a", "-m", "b"]).evaluate_distance is None
    assert ap.parse_args(["-f", "a", "-m", "b", "--evaluate-distance", "0.25"]).evaluate_distance == 0.25


# ---- Evaluation ----
def _evaluation_of(P):
    from simpleicp_amd import Evaluation
    t = eval_ref.terms(P, np.zeros(len(P), np.int64), np.full(len(P), 0.25))
    r = eval_ref.record(t, np.ones(len(P), bool))
    return Evaluation(len(P) + 3, r["n_inliers"], r["sums"][0], tuple(r["sums"][1:4]), tuple(r["sums"][4:10])), t


def _entry_magnitudes(t, n):
    """sum|terms| per entry of the information matrix: the products (or coordinates, or ones) that enter it"""
    a = np.abs(t).sum(axis=0)                                      # sum|t_j|: [1..3] x y z, [4..9] xx yy zz xy xz yz
    mag = np.zeros((6, 6))
    mag[0, 0], mag[1, 1], mag[2, 2] = a[5] + a[6], a[4] + a[6], a[4] + a[5]
    mag[0, 1], mag[0, 2], mag[1, 2] = a[7], a[8], a[9]
    mag[0, 4], mag[0, 5], mag[1, 5] = a[3], a[2], a[1]
    mag[1, 3], mag[2, 3], mag[2, 4] = a[3], a[2], a[1]
    mag[3, 3] = mag[4, 4] = mag[5, 5] = n
    return np.maximum(mag, mag.T)


def test_information_equals_the_row_by_row_sum():
    """Per entry within 8 u sum|terms|.  The cloud sizes are those at which that bound follows from the arithmetic alone.  The
    Evaluation's side rounds a product once, goes through ceil(log2 N) tree additions and at most one more (Syy + Szz).  Against
    the row-by-row sum in float64 -- a rounded product, at most one addition inside G^T G, N - 1 sequential additions -- N <= 3
    gives (1 + 2 + 1) + (1 + 1 + 2) = 8 u.  Against the row-by-row sum in exact rationals, rounded once, N <= 32 gives
    (1 + 5 + 1) + 1 = 8 u."""
    rng = np.random.default_rng(3)
    clouds = [(rng.standard_normal((n, 3)) * [1.0, 20.0, 0.1] + [3.0, -40.0, 0.5], eval_ref.information_rows) for n in (1, 2, 3)]
    clouds += [(rng.uniform(-2, 2, (n, 3)) + off, eval_ref.information_rows_exact) for n, off in ((17, 1e3), (32, 0.0), (31, -1e6))]
    for P, reference in clouds:
        ev, t = _evaluation_of(P)
        L, want, mag = ev.information, reference(P), _entry_magnitudes(t, len(P))
        assert (np.abs(L - want) <= 8 * U * mag).all()
        assert (L[mag == 0] == 0).all()
        assert np.array_equal(L, L.T)
        assert np.array_equal(L[3:6, 3:6], len(P) * np.eye(3))


def test_information_is_symmetric_and_positive_semidefinite_on_a_random_cloud():
    rng = np.random.default_rng(4)
    P = rng.standard_normal((300, 3)) * [1.0, 20.0, 0.1] + [3.0, -40.0, 0.5]
    ev, _ = _evaluation_of(P)
    L = ev.information
    assert np.array_equal(L, L.T)
    # (eigvalsh is backward stable: its eigenvalues are off by a few u |L|)
    assert np.linalg.eigvalsh(L).min() >= -64 * U * np.abs(L).sum()
    v = rng.standard_normal((50, 6))
    assert (np.einsum("ki,ij,kj->k", v, L, v) >= -64 * U * np.abs(L).sum() * (v * v).sum(axis=1)).all()


def test_evaluation_is_immutable_and_its_figures():
    from simpleicp_amd import Evaluation
    P = np.array([[1.0, 2.0, 3.0], [3.0, 2.0, 1.0]])
    ev, _ = _evaluation_of(P)
    assert ev.n_queries == 5 and ev.n_inliers == 2 and ev.fitness == 0.4
    assert ev.inlier_rmse == 0.5 and np.array_equal(ev.centroid, [2.0, 2.0, 2.0])
    with pytest.raises(Exception):
        ev.n_inliers = 3
    none = Evaluation(7, 0, 0.0, (0.0, 0.0, 0.0), (0.0,) * 6)
    assert none.fitness == 0.0 and none.inlier_rmse == 0.0 and not none.information.any() and np.isnan(none.centroid).all()


# ---- run()'s host plumbing on the stand-in ----
def _run_logged(icp, **kw):
    records = []
    handler = logging.Handler()
    handler.emit = lambda r: records.append(r.getMessage())
    log = logging.getLogger("simpleicp_amd")
    log.addHandler(handler)
    old = log.level
    log.setLevel(logging.INFO)
    try:
        out = icp.run(**kw)
    finally:
        log.removeHandler(handler)
        log.setLevel(old)
    return out, records


def _bunny(clouds, n=4000):
    from simpleicp_amd import PointCloud
    X1, X2 = clouds("bunny_part1")[:n], clouds("bunny_part2")[:n]
    return PointCloud(X1, columns=["x", "y", "z"]), PointCloud(X2.copy(), columns=["x", "y", "z"])


def test_run_evaluates_once_after_the_last_iteration_with_the_returned_H(ectx, clouds, monkeypatch):
    from simpleicp_amd import SimpleICP, _lib, backend
    pc_fix, pc_mov = _bunny(clouds)
    X1, X2 = pc_fix.X, pc_mov.X
    icp = SimpleICP(verbose=False)
    icp.add_point_clouds(pc_fix, pc_mov)
    icp.evaluate_distance = 0.5
    (H, X, rbp, res), records = _run_logged(icp, correspondences=300, max_iterations=3)
    assert ectx.calls.count("evaluate") == 1
    at = ectx.calls.index("evaluate")
    assert "icp_run" in ectx.calls[:at] and ectx.calls[at + 1:] == ["transform"]       # after the loop, before the final transform
    q, s, He, d, rows = ectx.eval_args
    assert (q, s, d, rows) == (_lib.FIX, _lib.MOV, 0.5, None) and np.array_equal(He, H)
    want = eval_ref.evaluate(X1, X2, H, 0.5)
    ev = icp.evaluation
    assert ev is icp.last_run_info["evaluation"]
    assert (ev.n_queries, ev.n_inliers) == (len(X1), want["n_inliers"]) and 0 < ev.n_inliers < len(X1)
    assert np.array([ev.sum_d2, *ev.sum_p, *ev.sum_pp]).tobytes() == want["sums"].tobytes()
    assert sum("fitness" in m for m in records) == 1
    # the same run without it: the parent's calls, the same bits, no evaluation
    plain = oracle_backend.OracleContext()
    monkeypatch.setattr(backend, "get_context", lambda: plain)
    pc_fix2, pc_mov2 = _bunny(clouds)
    icp2 = SimpleICP(verbose=False)
    icp2.add_point_clouds(pc_fix2, pc_mov2)
    (H2, X_2, rbp2, res2), records2 = _run_logged(icp2, correspondences=300, max_iterations=3)
    assert plain.calls == [c for c in ectx.calls if c != "evaluate"]
    assert H2.tobytes() == H.tobytes() and res2.tobytes() == res.tobytes() and X_2.tobytes() == X.tobytes()
    assert icp2.evaluation is None and "evaluation" not in icp2.last_run_info
    assert [m for m in records2 if not m.startswith("Finished")] == [m for m in records if "fitness" not in m and not m.startswith("Finished")]


def test_off_calls_nothing_and_a_backend_without_the_entry_point(monkeypatch, clouds):
    from simpleicp_amd import SimpleICP, _lib
    ctx = oracle_backend.install(monkeypatch)
    assert not hasattr(ctx, "evaluate")
    pc_fix, pc_mov = _bunny(clouds, 3000)
    icp = SimpleICP(verbose=False)
    icp.add_point_clouds(pc_fix, pc_mov)
    icp.evaluate_distance = 0.25
    with pytest.raises(_lib.BackendError, match="evaluation"):
        icp.run(correspondences=200, max_iterations=2)
    assert ctx.calls == []                                         # refused before the uploads
    icp.evaluate_distance = None
    H, _, _, _ = icp.run(correspondences=200, max_iterations=2)
    assert np.isfinite(H).all() and icp.evaluation is None


def test_evaluate_registration_on_the_stand_in(ectx, clouds):
    """both directions, arrays and PointClouds, inputs untouched; of="movable" hands the library the rigid inverse"""
    import simpleicp_amd
    from simpleicp_amd import PointCloud, _lib
    X1, X2 = clouds("bunny_part1")[:1500], clouds("bunny_part2")[:1200]
    a, t = 0.05, np.array([0.1, -0.2, 0.3])
    H = np.eye(4)
    H[:3, :3] = [[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]]
    H[:3, 3] = t
    keep1, keep2 = X1.copy(), X2.copy()
    ev = simpleicp_amd.evaluate_registration(X1, PointCloud(X2, columns=["x", "y", "z"]), H, 2.0)
    want = eval_ref.evaluate(X1, X2, H, 2.0)
    assert (ev.n_queries, ev.n_inliers) == (1500, want["n_inliers"]) and 0 < ev.n_inliers < 1500
    assert np.array([ev.sum_d2, *ev.sum_p, *ev.sum_pp]).tobytes() == want["sums"].tobytes()
    assert ectx.calls == ["upload", "upload", "evaluate"]
    ev = simpleicp_amd.evaluate_registration(X1, X2, H, 2.0, of="movable")
    Hi = np.eye(4)
    Hi[:3, :3] = H[:3, :3].T
    Hi[:3, 3] = -(H[:3, :3].T @ t)
    assert ectx.eval_args[:2] == (_lib.MOV, _lib.FIX) and np.array_equal(ectx.eval_args[2], Hi)
    want = eval_ref.evaluate(X2, X1, Hi, 2.0)
    assert (ev.n_queries, ev.n_inliers) == (1200, want["n_inliers"])
    assert np.array([ev.sum_d2, *ev.sum_p, *ev.sum_pp]).tobytes() == want["sums"].tobytes()
    assert np.array_equal(X1, keep1) and np.array_equal(X2, keep2)


def test_a_distributed_job_is_refused_before_any_backend_call(monkeypatch):
    from simpleicp_amd import PointCloud, SimpleICP, SimpleICPException, backend, dist

    def no_backend(*a, **k):
        raise AssertionError("the backend was used")

    class NoDevice:
        def __getattr__(self, name):
            if name.startswith("__"):
                raise AttributeError(name)
            return no_backend
    monkeypatch.setattr(dist, "is_distributed", lambda: True)
    monkeypatch.setattr(backend, "get_context", lambda: NoDevice())
    X = np.random.default_rng(0).standard_normal((50, 3))
    icp = SimpleICP(verbose=False)
    icp.add_point_clouds(PointCloud(X, columns=["x", "y", "z"]), PointCloud(X, columns=["x", "y", "z"]))
    icp.evaluate_distance = 0.5
    with pytest.raises(SimpleICPException, match="does not run in a torch.distributed job"):
        icp.run()
