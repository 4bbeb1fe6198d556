"""Consistent normal orientation (contract (H)), the parts that need no GPU: the companion header and the
binding, what Context.orient hands to the C entry in both forms, the argument checks, the plumbing of orient_normals,
PointCloud.orient_normals and register_global(orient=) on a stand-in context that answers with tests/orient_ref.py -- and the
reference itself, held to things it shares no code with: scipy's minimum spanning tree, analytic outward normals."""
import ctypes as C
import inspect
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle_backend
import orient_ref

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "simpleicp_hip_orient.h"


# ---- header, exports, binding ----
def test_header_names_are_exported_and_bound():
    from simpleicp_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(sicp_\w+)\s*\(", text))) == sorted(_lib.ORIENT_EXPORTS) == ["sicp_orient", "sicp_orient_version"]
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", str(so)], capture_output=True, text=True, check=True).stdout
    assert set(_lib.ORIENT_EXPORTS) <= set(re.findall(r" T (sicp_\w+)", out))
    others = set(_lib.EXPORTS)
    for name, f in _lib.FEATURES.items():
        if name != "orient":
            others |= set(f.exports)
    assert not set(_lib.ORIENT_EXPORTS) & others
    f = _lib.FEATURES["orient"]
    assert f.exports == _lib.ORIENT_EXPORTS and f.header == HEADER.name and f.version == 1 and f.exports[0] == "sicp_orient_version"
    L = _lib.load()
    assert "#define SICP_ORIENT_VERSION 1" in HEADER.read_text()
    assert L.sicp_orient_version() == _lib.ORIENT_VERSION == 1 and _lib.orient_version() == 1
    assert C.sizeof(_lib.OrientStats) == 56 and [n for n, _ in _lib.OrientStats._fields_] == list(orient_ref.KEYS)
    assert issubclass(_lib.OrientStats, _lib._Stats) and type(_lib.OrientStats().as_dict()["rounds"]) is int
    # the contract has a letter of its own, and the header carries it
    assert "contract (H)" in HEADER.read_text() and "(nx_i * nx_j + ny_i * ny_j) + nz_i * nz_j" in HEADER.read_text()
    # the main header and its version are untouched
    assert L.sicp_abi_version() == _lib.ABI_VERSION == 7
    assert "orient" not in (ROOT / "include" / "simpleicp_hip.h").read_text()
    assert any(p.name == "sicp_orient.hip" for p in build.SOURCES) and any(p.name == HEADER.name for p in build.HEADERS)
    assert list(inspect.signature(_lib.Context.orient).parameters)[1:6] == ["slot", "normals", "k", "reference", "away"]
    # the switch is read where the others are
    assert 'getenv("SICP_ORIENT_CHUNK")' in (ROOT / "simpleicp_amd" / "csrc" / "sicp_api.cpp").read_text()


def test_header_is_plain_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    src = tmp_path / "probe.c"
    src.write_text('#include "simpleicp_hip_orient.h"\n'
                   "int probe(sicp_ctx *c, const float *nrm, const double *ref, float *out, uint8_t *flipped)\n{\n"
                   "    sicp_orient_stats a;\n"
                   "    int rc = sicp_orient_version() + sicp_orient(c, SICP_FIX, nrm, 16, ref, 1, out, flipped, &a);\n"
                   "    return rc + (int)(a.n_points + a.n_void + a.n_components + a.n_forest_edges + a.n_flipped + a.n_components_voted\n"
                   "                      + a.rounds) + SICP_ORIENT_VERSION;\n}\n")
    r = subprocess.run([cc, "-std=c99", "-pedantic", "-Werror", "-Wall", "-Wextra", f"-I{ROOT / 'include'}", "-c", str(src), "-o",
                        str(tmp_path / "probe.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_ctx_is_refused_not_dereferenced():
    from simpleicp_amd import _lib
    L = _lib.load()
    N, out, flipped = np.zeros((8, 3), np.float32), np.full((8, 3), 7.5, np.float32), np.full(8, 9, np.uint8)
    st = _lib.OrientStats()
    rc = L.sicp_orient(None, _lib.FIX, _lib._ptr(N), 4, None, 0, _lib._ptr(out), _lib._ptr(flipped), C.byref(st))
    assert rc == _lib.ERR_INVALID and b"null ctx" in L.sicp_last_error()
    assert np.all(out == 7.5) and np.all(flipped == 9)


# ---- what the binding hands to the C entry ----
class _Recorder:
    """Stands in for the loaded library: the version function answers with the binding's version, the entry notes its arguments."""

    def __init__(self):
        self.calls = []

    def sicp_orient_version(self):
        from simpleicp_amd import _lib
        return _lib.ORIENT_VERSION

    def sicp_cloud_size(self, h, slot, out):
        out._obj.value = 9
        return 0

    def sicp_orient(self, *args):
        self.calls.append(args)
        return 0


def _seen(a):
    if a is None:
        return None
    if isinstance(a, C.c_void_p):
        return ("ptr", a.value)
    if hasattr(a, "_obj"):
        return ("ref", a._obj)
    return (type(a), a)


def test_context_orient_records_its_arguments(monkeypatch):
    from simpleicp_amd import _lib
    L = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda: L)
    ctx = _lib.Context.__new__(_lib.Context)
    ctx._L, ctx._h, ctx._Q, ctx._bg_src = L, C.c_void_p(0x1234), 5, {}
    monkeypatch.setattr(_lib.Context, "size", lambda self, slot: 9)
    try:
        N = np.random.default_rng(0).standard_normal((9, 3))
        out, flipped, st = ctx.orient(_lib.FIX, N, np.int64(4))
        assert out.shape == (9, 3) and out.dtype == np.float32 and flipped.shape == (9,) and flipped.dtype == bool
        assert type(st) is _lib.OrientStats
        a = [_seen(v) for v in L.calls.pop()]
        assert a[0] == ("ptr", 0x1234) and a[1] == (int, _lib.FIX) and a[2][0] == "ptr" and a[3] == (int, 4) and a[4] is None
        assert a[5] == (int, 0) and a[6] == ("ptr", out.ctypes.data) and a[7][0] == "ptr" and a[8][0] == "ref" and a[8][1] is st
        out, flipped, st = ctx.orient(_lib.MOV, N.astype(np.float32), 16, reference=(1, 2, 3), away=True, want_flipped=False)
        a = [_seen(v) for v in L.calls.pop()]
        assert flipped is None and a[7] is None and a[1] == (int, _lib.MOV) and a[4][0] == "ptr" and a[5] == (int, 1)
        st = ctx.orient(_lib.FIX, N.astype(np.float32), 7, normals_ptr=0x7000, flipped_ptr=0x7100)
        assert type(st) is _lib.OrientStats
        a = [_seen(v) for v in L.calls.pop()]
        assert a[3:8] == [(int, 7), None, (int, 0), ("ptr", 0x7000), ("ptr", 0x7100)]
        st = ctx.orient(_lib.FIX, N.astype(np.float32), 7, normals_ptr=0x7000)
        a = [_seen(v) for v in L.calls.pop()]
        assert a[6:8] == [("ptr", 0x7000), None] and not L.calls
        for bad in (np.zeros((9, 2)), np.zeros((8, 3))):
            with pytest.raises(ValueError, match=r"\(n, 3\)"):
                ctx.orient(_lib.FIX, bad, 2)
    finally:
        ctx._h = C.c_void_p()                  # (nothing to destroy)


# ---- argument checks ----
def test_argument_errors_name_the_keyword_and_come_before_the_backend(monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import PointCloud, backend, features
    from simpleicp_amd.pointcloud import PointCloudException

    def no_backend(*a, **k):
        raise AssertionError("the backend was called")
    monkeypatch.setattr(backend, "get_context", no_backend)
    X = np.random.default_rng(0).standard_normal((50, 3))
    f = simpleicp_amd.orient_normals
    assert "orient_normals" in simpleicp_amd.__all__
    sig = inspect.signature(f).parameters
    assert list(sig) == ["X", "normals", "neighbors", "normal_neighbors", "viewpoint", "away_from", "return_flipped", "return_info"]
    assert {n: p.default for n, p in sig.items() if n != "X"} == dict(normals=None, neighbors=16, normal_neighbors=10, viewpoint=None,
                                                                       away_from=None, return_flipped=False, return_info=False)
    assert all(sig[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig)[2:])
    k, kn, ref, away = features.orient_arguments(8, 10, None, (1, 2, 3))
    assert (k, kn, away) == (8, 10, True) and ref.tolist() == [1.0, 2.0, 3.0]
    assert features.orient_arguments()[2:] == (None, False) and features.orient_arguments(viewpoint=[0, 0, 1])[3] is False
    for bad in (1, 129, 2.0, "many", True, None):
        with pytest.raises(ValueError, match="neighbors"):
            f(X, neighbors=bad)
    for bad in (1, 0.5, None):
        with pytest.raises(ValueError, match="normal_neighbors"):
            f(X, normal_neighbors=bad)
    for bad in ((1, 2), (np.nan, 0, 0), "up", (0, np.inf, 0)):
        with pytest.raises(ValueError, match="viewpoint"):
            f(X, viewpoint=bad)
        with pytest.raises(ValueError, match="away_from"):
            f(X, away_from=bad)
    with pytest.raises(ValueError, match="viewpoint and away_from"):
        f(X, viewpoint=(0, 0, 1), away_from=(0, 0, 0))
    with pytest.raises(ValueError, match="return_flipped"):
        f(X, return_flipped=1)
    with pytest.raises(ValueError, match="return_info"):
        f(X, return_info="yes")
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        f(np.zeros((50, 2)))
    with pytest.raises(ValueError, match="normals must have shape"):
        f(X, np.zeros((49, 3)))
    with pytest.raises(ValueError, match=r"neighbors \(16\) exceeds"):
        f(X[:10], np.zeros((10, 3)))
    with pytest.raises(ValueError, match=r"normal_neighbors \(10\) exceeds"):
        f(X[:8], neighbors=4)
    # an empty input: an empty result and an all-zero record, the library untouched
    out, flipped, info = f(np.zeros((0, 3)), return_flipped=True, return_info=True)
    assert out.shape == (0, 3) and out.dtype == np.float32 and flipped.shape == (0,) and flipped.dtype == bool
    assert info == dict.fromkeys(orient_ref.KEYS, 0) and tuple(info) == orient_ref.KEYS
    pc = PointCloud(X, columns=["x", "y", "z"])
    with pytest.raises(PointCloudException, match="needs the normals"):
        pc.orient_normals()
    for c in ("nx", "ny", "nz"):
        pc[c] = 1.0
    with pytest.raises(PointCloudException, match="neighbors"):
        pc.orient_normals(neighbors=1)
    with pytest.raises(TypeError, match="orient"):
        simpleicp_amd.register_global(X, X, max_distance=1.0, orient=2.5)
    with pytest.raises(TypeError, match="orient"):
        simpleicp_amd.register_global(X, X, max_distance=1.0, orient=dict(viewpoint=(0, 0, 0)))
    with pytest.raises(ValueError, match="neighbors"):
        simpleicp_amd.register_global(X, X, max_distance=1.0, orient=1)


def test_a_distributed_job_is_refused(monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import backend, dist
    from simpleicp_amd.icp import SimpleICPException
    monkeypatch.setattr(dist, "is_distributed", lambda: True)
    monkeypatch.setattr(backend, "get_context", lambda: (_ for _ in ()).throw(AssertionError("the backend was called")))
    with pytest.raises(SimpleICPException, match="orient_normals does not run in a torch.distributed job"):
        simpleicp_amd.orient_normals(np.zeros((20, 3)), np.ones((20, 3)))


# ---- the plumbing on a stand-in context ----
class OrientOracleContext(oracle_backend.OracleContext):
    """The oracle backend, and the orient entry answered by the reference (host form only)."""

    def __init__(self):
        super().__init__()
        self.seen = []

    def orient(self, slot, normals, k, reference=None, away=False, normals_ptr=None, flipped_ptr=None, want_flipped=True):
        assert normals_ptr is None and flipped_ptr is None and type(k) is int and normals.dtype == np.float32
        self._log("orient")
        self.seen.append((slot, k, None if reference is None else np.array(reference), bool(away)))
        kw = {} if reference is None else ({"away_from": reference} if away else {"viewpoint": reference})
        ref = orient_ref.orient(self.download(slot), normals, k, **kw)
        return ref["normals"], ref["flipped"], orient_ref.record(ref)


@pytest.fixture
def octx(monkeypatch):
    from simpleicp_amd import backend
    ctx = OrientOracleContext()
    monkeypatch.setattr(backend, "get_context", lambda: ctx)
    return ctx


def test_orient_normals_on_host_clouds(octx, monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import PointCloud, _lib, backend
    X, T = orient_ref.sphere(1, 400)
    N, _ = orient_ref.coin(2, T)
    want = orient_ref.orient(X, N, 16)
    got = simpleicp_amd.orient_normals(X, N)
    assert octx.calls[-1] == "orient" and octx.seen[-1][:2] == (_lib.FIX, 16) and octx.seen[-1][2] is None
    assert got.tobytes() == want["normals"].tobytes() and got.dtype == np.float32
    out, flipped, info = simpleicp_amd.orient_normals(X, N.astype(np.float64), neighbors=8, away_from=(0, 0, 0), return_flipped=True,
                                                       return_info=True)
    want = orient_ref.orient(X, N, 8, away_from=(0.0, 0.0, 0.0))
    assert octx.seen[-1][1] == 8 and octx.seen[-1][3] is True and octx.seen[-1][2].tolist() == [0.0, 0.0, 0.0]
    assert out.tobytes() == want["normals"].tobytes() and np.array_equal(flipped, want["flipped"]) and info == orient_ref.record(want)
    assert tuple(info) == orient_ref.KEYS and ((out.astype(np.float64) * T).sum(axis=1) > 0).all()
    out, info = simpleicp_amd.orient_normals(X, N, viewpoint=(0, 0, 0), return_info=True)
    assert octx.seen[-1][3] is False and ((out.astype(np.float64) * T).sum(axis=1) < 0).all()
    # normals=None: the library's own from normal_neighbors points, exactly as fpfh_features chooses them
    own = simpleicp_amd.orient_normals(X, normal_neighbors=12, away_from=(0, 0, 0))
    assert "estimate_normals" in octx.calls and ((own.astype(np.float64) * T).sum(axis=1) > 0).mean() > 0.99
    # a PointCloud's own columns, and PointCloud.orient_normals rewriting them
    pc = PointCloud(X, columns=["x", "y", "z"])
    for j, c in enumerate(("nx", "ny", "nz")):
        pc[c] = N[:, j].astype(np.float64)
    before = len(octx.calls)
    got = simpleicp_amd.orient_normals(pc, neighbors=8, away_from=(0, 0, 0))
    assert got.tobytes() == want["normals"].tobytes() and "estimate_normals" not in octx.calls[before:]
    pc.orient_normals(neighbors=8, away_from=(0, 0, 0))
    cols = np.stack([pc[c].to_numpy() for c in ("nx", "ny", "nz")], axis=1)
    assert cols.astype(np.float32).tobytes() == want["normals"].tobytes() and pc.last_orient_stats == orient_ref.record(want)
    plain = oracle_backend.OracleContext()                                     # a backend without the entry says so
    monkeypatch.setattr(backend, "get_context", lambda: plain)
    with pytest.raises(_lib.BackendError, match="normal orientation"):
        simpleicp_amd.orient_normals(X, N)


# ---- the reference, held to things it shares no code with ----
def _scipy_forest(n, lo, hi, order):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import minimum_spanning_tree
    rank = np.empty(len(lo), np.int64)
    rank[order] = np.arange(1, len(lo) + 1)                                    # distinct positive integers: no "zero means no edge"
    T = minimum_spanning_tree(coo_matrix((rank.astype(np.float64), (lo, hi)), shape=(n, n)).tocsr()).tocoo()
    pairs = np.column_stack([np.minimum(T.row, T.col), np.maximum(T.row, T.col)]).astype(np.int64)
    return pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]


def _cases():
    for name, shape in (("sphere", orient_ref.sphere), ("torus", orient_ref.torus)):
        X, T = shape(40, 2000)
        yield name, X, T, orient_ref.coin(41, T)[0], 16
    A, TA = orient_ref.sphere(42, 2000)
    B, TB = orient_ref.sphere(43, 2000, centre=(100.0, 0.0, 0.0))
    yield "two spheres", np.vstack([A, B]), np.vstack([TA, TB]), orient_ref.coin(44, np.vstack([TA, TB]))[0], 8
    X, T = orient_ref.surface(45, 1500)
    X[np.arange(0, 300)] = X[np.arange(300, 600)]                              # duplicates, quantised normals: ties
    yield "ties", X, T, orient_ref.coin(46, np.round(T * 2.0) / 2.0)[0], 10


@pytest.fixture(scope="module")
def cases():
    return {name: (X, T, N, k, orient_ref.lists(X, k)) for name, X, T, N, k in _cases()}


@pytest.mark.parametrize("name", ["sphere", "torus", "two spheres", "ties"])
def test_the_forest_is_scipys_minimum_spanning_tree(cases, name):
    X, T, N, k, idx = cases[name]
    ref = orient_ref.orient(X, N, k, idx=idx)
    lo, hi, s = orient_ref.graph(idx, N.astype(np.float64))
    assert len(np.unique(lo * len(X) + hi)) == len(lo) and (lo < hi).all()     # every edge once
    order = orient_ref.total_order(lo, hi, s)
    c = np.abs(s)[order]
    assert (np.diff(c) <= 0).all()                                              # larger c first
    tie = np.diff(c) == 0
    assert (np.diff(lo[order])[tie] >= 0).all()
    assert np.array_equal(ref["forest"], _scipy_forest(len(X), lo, hi, order))
    assert ref["rounds"] <= int(np.ceil(np.log2(len(X)))) and ref["n_forest_edges"] == len(X) - ref["n_components"]


def _side(ref, T):
    return np.sign((ref["normals"].astype(np.float64) * T).sum(axis=1))


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_every_component_ends_on_one_side_and_the_vote_picks_it(cases, name):
    X, T, N, k, idx = cases[name]
    ref = orient_ref.orient(X, N, k, idx=idx)
    side = _side(ref, T)
    for a in np.unique(ref["component"]):
        assert len(np.unique(side[ref["component"] == a])) == 1
    assert (_side(orient_ref.orient(X, N, k, away_from=(0.0, 0.0, 0.0), idx=idx), T) == 1).all()
    assert (_side(orient_ref.orient(X, N, k, viewpoint=(0.0, 0.0, 0.0), idx=idx), T) == -1).all()
    # the library's own normals, through the oracle: unit eigenvectors of arbitrary sign, a little off the analytic ones
    from oracle import orc
    own = np.asarray(orc.normals(X, orc.knn(X, X, k=10)[0])[0], dtype=np.float32)
    own = orient_ref.coin(50, own.astype(np.float64))[0]
    ref = orient_ref.orient(X, own, k, away_from=(0.0, 0.0, 0.0), idx=idx)
    side = _side(ref, T)
    for a in np.unique(ref["component"]):
        assert len(np.unique(side[ref["component"] == a])) == 1
    assert (side == 1).all()


def test_two_spheres_a_hundred_radii_apart_are_two_components(cases):
    X, T, N, k, idx = cases["two spheres"]
    ref = orient_ref.orient(X, N, k, idx=idx)
    assert ref["n_components"] == 2 and sorted(np.unique(ref["component"]).tolist()) == [0, 2000]
    side = _side(ref, T)
    assert len(np.unique(side[:2000])) == 1 and len(np.unique(side[2000:])) == 1
    assert not ref["flipped"][0] and not ref["flipped"][2000]                  # the anchors keep their signs


def test_vote_arithmetic_ties_and_void_points():
    # four points in a row, normals up; seen from the side at their own height every t is 0: a tie, nothing turns
    X = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0], [3.0, 0, 0]])
    N = np.array([[0, 0, 1.0], [0, 0, -1.0], [0, 0, 1.0], [0, 0, 1.0]], np.float32)
    for kw in ({"viewpoint": (9.0, 0.0, 0.0)}, {"away_from": (9.0, 0.0, 0.0)}):
        ref = orient_ref.orient(X, N, 2, **kw)
        assert ref["flipped"].tolist() == [False, True, False, False] and ref["n_components_voted"] == 0
    # two up, two down after the tree: pos == neg, a tie again
    X2 = np.array([[0.0, 0, 1], [1.0, 0, 1], [2.0, 0, -1], [3.0, 0, -1]])
    up = np.tile(np.array([0, 0, 1.0], np.float32), (4, 1))
    for kw in ({"viewpoint": (1.5, 0.0, 0.0)}, {"away_from": (1.5, 0.0, 0.0)}):
        ref = orient_ref.orient(X2, up, 3, **kw)
        assert not ref["flipped"].any() and ref["n_components_voted"] == 0 and ref["n_components"] == 1
    # three against one: the majority decides for all four, both senses
    X3 = np.array([[0.0, 0, 1], [1.0, 0, 1], [2.0, 0, 1], [3.0, 0, -1]])
    ref = orient_ref.orient(X3, up, 3, viewpoint=(1.5, 0.0, 0.0))
    assert ref["flipped"].all() and ref["n_components_voted"] == 1 and ref["n_flipped"] == 4
    ref = orient_ref.orient(X3, up, 3, away_from=(1.5, 0.0, 0.0))
    assert not ref["flipped"].any() and ref["n_components_voted"] == 0
    # void points neither vote nor flip, and are components of their own
    N3 = up.copy()
    N3[1] = (np.nan, 0, 1)
    N3[2] = (0, 0, 0)
    ref = orient_ref.orient(X2, N3, 4, viewpoint=(0.0, 0.0, -9.0))
    assert ref["n_void"] == 2 and ref["n_components"] == 3 and ref["flipped"].tolist() == [True, False, False, True]
    assert ref["normals"][1:3].tobytes() == N3[1:3].tobytes() and ref["n_components_voted"] == 1
    # -0.0 and +0.0 agree
    Z = np.array([[1.0, 0, 0], [-0.0, -1.0, -1.0]], np.float32)
    ref = orient_ref.orient(X[:2], Z, 2)
    assert not ref["flipped"].any() and np.signbit(orient_ref.graph(orient_ref.lists(X[:2], 2), Z.astype(np.float64))[2][0])
