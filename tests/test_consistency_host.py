"""Match consistency (contract (C)), the parts that need no GPU: the companion header and the binding, the
refusals that come before any device work, the numpy reference (tests/consistency_ref.py) on graphs checked by hand, its symmetry,
the recovery of the right matches under 90 to 98 % wrong ones, and the plumbing of consistent_matches and
register_global(prune=...) on a stand-in context."""
import ctypes as C
import inspect
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import consistency_ref
import oracle_backend
import robust_ref
from test_robust_host import RobustOracleContext, noisy_copy, pose_error, surface_pair, u64   # noqa: F401  (surface_pair: a fixture)

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "simpleicp_hip_consistency.h"

# The reference's robust fit (0.01, 64 rounds, divisor 1.4, identity start, automatic scale) on the rows the reference's pruning
# (tolerance 0.01, min_length 0.1) keeps, measured on the CPU (x86-64, numpy / OpenBLAS): (65 rows, 90 % wrong, seed 1) 0.0257
# degrees and 7.798e-4; (2 000 rows, 98 % wrong, seed 0) 0.0487 degrees and 4.125e-4.  DESIGN.md section 21.  The bounds are 10 x
# the largest: room for other libm and BLAS builds (section 20's margin and reason).
RECOVERY_ANGLE_BOUND = 0.487
RECOVERY_SHIFT_BOUND = 7.798e-3
RECOVERY_INPUTS = ((400, 0.95), (65, 0.90), (2000, 0.98))


def recovery_case(m, wrong, seed):
    return noisy_copy(np.random.default_rng(1000 * seed + m), m, wrong=wrong, noise=0.002)


# ---- header, exports, binding ----
def test_header_names_are_exported_and_bound():
    from simpleicp_amd import _lib, build
    head = HEADER.read_text()
    text = re.sub(r"/\*.*?\*/", "", head, flags=re.S)
    assert sorted(set(re.findall(r"\b(sicp_\w+)\s*\(", text))) == sorted(_lib.CONSISTENCY_EXPORTS) == [
        "sicp_consistency_version", "sicp_match_consistency"]
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", str(so)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sicp_\w+)", out))
    assert set(_lib.CONSISTENCY_EXPORTS) <= exported
    others = (set(_lib.EXPORTS) | set(_lib.BATCH_EXPORTS) | set(_lib.DEVICE_EXPORTS) | set(_lib.NORMALS_EXPORTS) | set(_lib.VOXEL_EXPORTS)
              | set(_lib.EVAL_EXPORTS) | set(_lib.OUTLIER_EXPORTS) | set(_lib.CHAIN_EXPORTS) | set(_lib.FPFH_EXPORTS)
              | set(_lib.GLOBAL_EXPORTS) | set(_lib.POSEFIT_EXPORTS) | set(_lib.ROBUST_EXPORTS))
    assert not set(_lib.CONSISTENCY_EXPORTS) & others
    L = _lib.load()
    # the version triple: the header's, the library's, the binding's
    assert "#define SICP_CONSISTENCY_VERSION 1" in head
    assert L.sicp_consistency_version() == _lib.CONSISTENCY_VERSION == 1 and _lib.consistency_version() == 1
    assert f"#define SICP_CONSISTENCY_MAX_ROWS {_lib.CONSISTENCY_MAX_ROWS}" in head
    assert _lib.CONSISTENCY_MAX_ROWS == consistency_ref.MAX_ROWS == 32768
    assert C.sizeof(_lib.ConsistencyStats) == 56
    assert [n for n, _ in _lib.ConsistencyStats._fields_] == re.search(r"typedef struct sicp_consistency_stats \{\s*int64_t ([^;]+);", head)\
        .group(1).replace(" ", "").split(",")
    f = _lib.FEATURES["consistency"]
    assert f.exports == _lib.CONSISTENCY_EXPORTS and f.header == HEADER.name and f.version == 1
    assert len(f.argtypes["sicp_match_consistency"]) == 9
    # the main header, its version and the other companions are untouched
    assert L.sicp_abi_version() == _lib.ABI_VERSION == 7
    assert (L.sicp_global_version(), L.sicp_posefit_version(), L.sicp_robust_version(), L.sicp_fpfh_version()) == (1, 1, 1, 1)
    assert (_lib.BATCH_VERSION, _lib.DEVICE_VERSION, _lib.NORMALS_VERSION, _lib.VOXEL_VERSION, _lib.EVAL_VERSION, _lib.OUTLIER_VERSION,
            _lib.CHAIN_VERSION, _lib.FPFH_VERSION, _lib.GLOBAL_VERSION, _lib.POSEFIT_VERSION, _lib.ROBUST_VERSION) == (1,) * 11
    for other in (ROOT / "include").glob("simpleicp_hip*.h"):
        if other != HEADER:
            assert "consistency" not in other.read_text().lower()
    # the word the global test refuses in every companion but its own
    assert "ransac" not in head.lower()
    assert list(inspect.signature(_lib.Context.match_consistency).parameters)[1:] == [
        "src", "dst", "tolerance", "min_length", "m", "degree_ptr", "core_ptr"]
    assert any(p.name == "sicp_consistency.hip" for p in build.SOURCES) and any(p.name == HEADER.name for p in build.HEADERS)


def test_null_ctx_is_refused_not_dereferenced():
    from simpleicp_amd import _lib
    L = _lib.load()
    P = _lib._ptr
    X, deg, core, st = np.zeros((4, 3)), np.full(4, 7, np.int32), np.full(4, 7, np.int32), _lib.ConsistencyStats()
    assert L.sicp_match_consistency(None, P(X), P(X), 4, 0.01, 0.0, P(deg), P(core), C.byref(st)) == _lib.ERR_INVALID
    assert b"null ctx" in L.sicp_last_error() and np.all(deg == 7) and np.all(core == 7)


# ---- argument errors before the backend is touched ----
def test_python_argument_errors_come_before_the_backend(monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import _lib, backend

    def no_backend(*a, **k):
        raise AssertionError("the backend was called")
    monkeypatch.setattr(backend, "get_context", no_backend)
    assert "consistent_matches" in simpleicp_amd.__all__ and "ConsistencyResult" in simpleicp_amd.__all__
    cm, rg = simpleicp_amd.consistent_matches, simpleicp_amd.register_global
    sig = inspect.signature(cm).parameters
    assert list(sig) == ["src", "dst", "tolerance", "min_length"]
    assert all(p.kind == p.KEYWORD_ONLY for n, p in sig.items() if n not in ("src", "dst")) and sig["min_length"].default == 0.0
    X = np.random.default_rng(0).standard_normal((10, 3))
    with pytest.raises(TypeError):
        cm(X, X)                                                      # tolerance has no default
    for t in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tolerance"):
            cm(X, X, tolerance=t)
    for t in ("wide", None, True):
        with pytest.raises(TypeError, match="tolerance"):
            cm(X, X, tolerance=t)
    for l in (-1e-9, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="min_length"):
            cm(X, X, tolerance=0.1, min_length=l)
    for l in ("0", None, False):
        with pytest.raises(TypeError, match="min_length"):
            cm(X, X, tolerance=0.1, min_length=l)
    with pytest.raises(ValueError, match="same number"):
        cm(X, X[:9], tolerance=0.1)
    with pytest.raises(ValueError, match="at least 3"):
        cm(X[:2], X[:2], tolerance=0.1)
    with pytest.raises(ValueError, match=r"\(m, 3\)"):
        cm(X[:, :2], X[:, :2], tolerance=0.1)
    big = np.zeros((_lib.CONSISTENCY_MAX_ROWS + 1, 3))
    with pytest.raises(ValueError, match=r"32768.*thin the matches first"):
        cm(big, big, tolerance=0.1)
    # register_global: the keywords arrive through **ransac_kwargs, under both methods
    assert list(inspect.signature(rg).parameters)[-1] == "ransac_kwargs"
    for method in ({}, {"method": "ransac"}, {"method": "robust"}):
        for t in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="tolerance"):
                rg(X, X, max_distance=1.0, prune=t, **method)
        for t in ("wide", True):
            with pytest.raises(TypeError, match="tolerance"):
                rg(X, X, max_distance=1.0, prune=t, **method)
        with pytest.raises(ValueError, match="min_length"):
            rg(X, X, max_distance=1.0, prune=0.1, prune_min_length=-1.0, **method)
        with pytest.raises(TypeError, match="min_length"):
            rg(X, X, max_distance=1.0, prune=0.1, prune_min_length=None, **method)
        with pytest.raises(TypeError, match="prune_min_length without prune"):
            rg(X, X, max_distance=1.0, prune_min_length=0.1, **method)
        with pytest.raises(TypeError, match="prune_min_length without prune"):
            rg(X, X, max_distance=1.0, prune=None, prune_min_length=0.1, **method)
    # prune is accepted with both methods: what raises next is the other keywords' check
    with pytest.raises(ValueError, match="rounds"):
        rg(X, X, max_distance=1.0, method="robust", prune=0.1, rounds=0)
    with pytest.raises(ValueError, match="hypotheses"):
        rg(X, X, max_distance=1.0, prune=0.1, prune_min_length=0.2, hypotheses=0)


def test_a_distributed_job_is_refused(monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import backend, dist
    monkeypatch.setattr(backend, "get_context", lambda: (_ for _ in ()).throw(AssertionError("the backend was called")))
    monkeypatch.setattr(dist, "is_distributed", lambda: True)
    X = np.random.default_rng(0).standard_normal((10, 3))
    with pytest.raises(simpleicp_amd.SimpleICPException, match="does not run in a torch.distributed job"):
        simpleicp_amd.consistent_matches(X, X, tolerance=0.1)


# ---- the reference alone ----
def graph(m, edges):
    A = np.zeros((m, m), bool)
    for i, j in edges:
        A[i, j] = A[j, i] = True
    return A


def test_core_numbers_of_graphs_checked_by_hand():
    cn = consistency_ref.core_numbers
    # a triangle with a pendant row: the triangle is a 2-core, the pendant row has one partner
    A = graph(4, [(0, 1), (1, 2), (0, 2), (2, 3)])
    assert cn(A).tolist() == [2, 2, 2, 1] and consistency_ref.subrounds(A) == 2
    # two cliques (of 4 and of 5 rows) joined by one edge: the edge lifts nobody
    k4 = [(i, j) for i in range(4) for j in range(i)]
    k5 = [(4 + i, 4 + j) for i in range(5) for j in range(i)]
    A = graph(9, k4 + k5 + [(0, 4)])
    assert cn(A).tolist() == [3] * 4 + [4] * 5
    # an empty graph, a complete graph
    assert cn(np.zeros((6, 6), bool)).tolist() == [0] * 6 and consistency_ref.subrounds(np.zeros((6, 6), bool)) == 1
    A = graph(7, [(i, j) for i in range(7) for j in range(i)])
    assert cn(A).tolist() == [6] * 7 and consistency_ref.subrounds(A) == 1
    # a path: every row has core 1; a cycle with a chord: 2
    assert cn(graph(5, [(0, 1), (1, 2), (2, 3), (3, 4)])).tolist() == [1] * 5
    assert cn(graph(5, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 0), (0, 2)])).tolist() == [2] * 5
    # the definition itself, on a random graph: the rows with core >= k have at least k partners among themselves, and adding
    # any set of other rows breaks that for one of them (the peel order of the rest)
    rng = np.random.default_rng(3)
    U = rng.random((40, 40)) < 0.2
    A = np.triu(U, 1) | np.triu(U, 1).T
    core = cn(A)
    for k in range(1, int(core.max()) + 1):
        inside = core >= k
        assert np.all(A[np.ix_(inside, inside)].sum(axis=1) >= k)
        rest = ~inside
        while rest.any():                                              # no larger set qualifies: some row of it always falls short
            union = inside | rest
            short = rest & (A[:, union].sum(axis=1) < k)
            assert short.any()
            rest &= ~short
    # the record and the mask
    src = np.array([[0.0, 0, 0], [3, 0, 0], [0, 4, 0], [50, 50, 50], [np.nan, 0, 0]])
    dst = src.copy()
    dst[3] = [0, 0, 1]
    dst[4] = [1, 1, 1]
    degree, core, rec = consistency_ref.consistency(src, dst, 0.5, 0.0)
    assert degree.tolist() == [2, 2, 2, 0, 0] and core.tolist() == [2, 2, 2, 0, 0]
    assert rec == dict(n_rows=5, n_valid=4, n_edges=3, max_degree=2, max_core=2, n_max_core=3)
    assert consistency_ref.keep_mask(core, rec).tolist() == [True, True, True, False, False]
    degree, core, rec = consistency_ref.consistency(src, dst, 0.5, 100.0)
    assert not degree.any() and not core.any() and rec["n_max_core"] == 0 and not consistency_ref.keep_mask(core, rec).any()


def test_the_graph_is_symmetric_bit_for_bit():
    for m, wrong in ((65, 0.5), (300, 0.9)):
        src, dst, _ = noisy_copy(np.random.default_rng(m), m, wrong)
        src[5], dst[7, 1] = np.nan, np.inf
        full = consistency_ref.adjacency(src, dst, 0.01, 0.1, full=True)
        assert np.array_equal(full, full.T) and not full.diagonal().any() and not full[5].any() and not full[:, 7].any()
        assert np.array_equal(full, consistency_ref.adjacency(src, dst, 0.01, 0.1))
        # the lengths themselves, both ways round
        a = consistency_ref.lengths(src, slice(0, m), slice(0, m))
        assert np.array_equal(u64(np.nan_to_num(a)), u64(np.nan_to_num(a.T)))


def test_recovery_of_the_right_matches_on_the_reference():
    fits = {}
    for m, wrong in RECOVERY_INPUTS:
        for seed in range(3):
            src, dst, good = recovery_case(m, wrong, seed)
            degree, core, rec = consistency_ref.consistency(src, dst, 0.01, 0.1)
            keep = consistency_ref.keep_mask(core, rec)
            print(f"m {m}, wrong share {wrong}, seed {seed}: {int(good.sum())} right matches, {int(keep.sum())} kept, "
                  f"{int((keep & good).sum())} of them right, max core {rec['max_core']}")
            assert not (keep & ~good).any()                            # no wrong match is kept
            assert (keep & good).sum() >= 0.9 * good.sum()             # ... and at least 0.9 of the right ones are
            if (m, seed) in ((65, 1), (2000, 0)):
                fits[m] = (src, dst, keep)
    worst_angle = worst_shift = 0.0
    for m, (src, dst, keep) in fits.items():
        # on all rows the robust fit of these two does not recover the motion; on the kept rows it does
        P, inl, _, _ = robust_ref.robust(src[keep], dst[keep], None, 0.01, 64, 1.4, 0.0)
        angle, shift = pose_error(P[0])
        print(f"m {m}: the robust fit on the {int(keep.sum())} kept rows: {angle:.4f} degrees, |t - t_true| = {shift:.3e}, {inl[0]} inliers")
        worst_angle, worst_shift = max(worst_angle, angle), max(worst_shift, shift)
        assert inl[0] == keep.sum()
    assert worst_angle <= RECOVERY_ANGLE_BOUND and worst_shift <= RECOVERY_SHIFT_BOUND


# ---- the plumbing on a stand-in context ----
class ConsistencyOracleContext(RobustOracleContext):
    """The chain's entry points answered by the numpy references, and the pruning's."""

    def match_consistency(self, src, dst, tolerance, min_length, m=None, degree_ptr=None, core_ptr=None):
        assert degree_ptr is None and src.dtype == dst.dtype == np.float64
        self._log("match_consistency")
        self.consistency_args = (np.array(src), np.array(dst), tolerance, min_length)
        degree, core, rec = consistency_ref.consistency(src, dst, tolerance, min_length)
        return degree, core, dict(rec, n_subrounds=1)

    def ransac_triplets(self, src, dst, triples, max_distance, edge_ratio, **kw):
        self.ransac_rows = (np.array(src), np.array(dst))
        return super().ransac_triplets(src, dst, triples, max_distance, edge_ratio, **kw)


@pytest.fixture
def octx(monkeypatch):
    from simpleicp_amd import backend
    ctx = ConsistencyOracleContext()
    monkeypatch.setattr(backend, "get_context", lambda: ctx)
    return ctx


def test_consistent_matches(octx):
    import simpleicp_amd
    src, dst, good = recovery_case(65, 0.90, 1)
    res = simpleicp_amd.consistent_matches(src.astype(np.float32), dst, tolerance=0.01, min_length=0.1)
    s32 = src.astype(np.float32).astype(np.float64)
    assert octx.calls == ["match_consistency"] and np.array_equal(octx.consistency_args[0], s32)
    assert octx.consistency_args[2:] == (0.01, 0.1)
    degree, core, rec = consistency_ref.consistency(s32, dst, 0.01, 0.1)
    assert res.keep.dtype == bool and res.core.dtype == res.degree.dtype == np.int32
    assert np.array_equal(res.core, core) and np.array_equal(res.degree, degree) and res.stats == dict(rec, n_subrounds=1)
    assert np.array_equal(res.keep, core == rec["max_core"]) and res.keep.sum() == rec["n_max_core"] > 0
    # min_length defaults to 0.0; an empty graph keeps nobody
    res = simpleicp_amd.consistent_matches(src, dst + np.arange(65)[:, None] * 100.0, tolerance=1e-6)
    assert octx.consistency_args[2:] == (1e-6, 0.0) and res.stats["max_core"] == 0 and not res.keep.any() and res.keep.shape == (65,)
    from simpleicp_amd import _lib
    octx.__class__ = oracle_backend.OracleContext                     # a backend without the entry point
    with pytest.raises(_lib.BackendError, match="match consistency"):
        simpleicp_amd.consistent_matches(src, dst, tolerance=0.01)


def test_register_global_with_prune(octx, surface_pair):
    import simpleicp_amd
    fixed, movable, kw = surface_pair
    plain = simpleicp_amd.register_global(fixed, movable, hypotheses=50, seed=1, **kw)
    assert "match_consistency" not in octx.calls and plain.n_consistent is None
    all_src, all_dst = octx.ransac_rows
    chain = [c for c in octx.calls if c != "ransac_triplets"]
    # prune=None is the default, call for call and byte for byte
    octx.calls.clear()
    same = simpleicp_amd.register_global(fixed, movable, hypotheses=50, seed=1, prune=None, **kw)
    assert octx.calls == chain + ["ransac_triplets"] and same.H.tobytes() == plain.H.tobytes() and same.stats == plain.stats
    assert same.n_consistent is None
    # with prune the estimator sees the rows of the maximal core, in their order
    tol, ml = 0.02, 0.3
    degree, core, rec = consistency_ref.consistency(all_src, all_dst, tol, ml)
    keep = consistency_ref.keep_mask(core, rec)
    assert 3 <= keep.sum() < len(keep)
    octx.calls.clear()
    res = simpleicp_amd.register_global(fixed, movable, hypotheses=50, seed=1, prune=tol, prune_min_length=ml, **kw)
    assert octx.calls == chain + ["match_consistency", "ransac_triplets"]
    assert np.array_equal(octx.consistency_args[0], all_src) and np.array_equal(octx.consistency_args[1], all_dst)
    assert octx.consistency_args[2:] == (tol, ml)
    assert np.array_equal(octx.ransac_rows[0], all_src[keep]) and np.array_equal(octx.ransac_rows[1], all_dst[keep])
    assert res.n_matches == plain.n_matches == len(keep) and res.n_consistent == int(keep.sum())
    direct = simpleicp_amd.ransac_pose(all_src[keep], all_dst[keep], max_distance=kw["max_distance"], hypotheses=50, seed=1)
    assert res.stats == direct.stats and res.index == direct.index and res.inliers == direct.inliers
    assert (res.H is None and direct.H is None) or res.H.tobytes() == direct.H.tobytes()
    # the robust method behind the same pruning
    octx.calls.clear()
    rob = simpleicp_amd.register_global(fixed, movable, method="robust", rounds=30, prune=tol, prune_min_length=ml, **kw)
    assert octx.calls == chain + ["match_consistency", "pose_robust"]
    assert np.array_equal(octx.robust_args[0], all_src[keep]) and np.array_equal(octx.robust_args[1], all_dst[keep])
    P, inl, _, rrec = robust_ref.robust(all_src[keep], all_dst[keep], None, kw["max_distance"], 30, 1.4, 0.0)
    assert rob.stats == rrec and rob.n_consistent == int(keep.sum()) and rob.n_matches == len(keep) and rob.inliers == inl[0]
    assert np.array_equal(u64(rob.H[:3, :3].ravel()), u64(P[0, :9])) and np.array_equal(u64(rob.H[:3, 3]), u64(P[0, 9:]))
    # fewer than three rows left: the result without a pose that fewer than three matches give, and no estimator call
    for method, none in (({}, dict(n_hypotheses=0, n_void=0, n_pruned=0, best=-1, best_inliers=-1)),
                         ({"method": "robust"}, dict(n_poses=0, n_void=0, best=-1, best_inliers=-1))):
        octx.calls.clear()
        few = simpleicp_amd.register_global(fixed, movable, prune=1e-9, prune_min_length=1e6, **method, **kw)
        assert octx.calls == chain + ["match_consistency"]
        assert few.H is None and few.candidates == [] and few.stats == none and few.n_matches == len(keep) and few.n_consistent == 0
    # a backend without the entry point
    from simpleicp_amd import _lib
    octx.__class__ = RobustOracleContext
    with pytest.raises(_lib.BackendError, match="match consistency"):
        simpleicp_amd.register_global(fixed, movable, prune=tol, **kw)
