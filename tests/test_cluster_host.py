"""DBSCAN labels (contract (U)), the parts that need no GPU: the companion header and the binding, the
reference (tests/cluster_ref.py) against sklearn and on hand cases, what Context.cluster hands to the C entry in both forms, and
the plumbing of cluster_labels, PointCloud.select_largest_cluster and select_clusters on a stand-in context."""
import ctypes as C
import inspect
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import cluster_ref
import oracle_backend

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "simpleicp_hip_cluster.h"

# (seed, n, radius, min_points) of the clouds held against sklearn: cluster_ref.blobs
SKLEARN_CASES = [(1, 60, 0.5, 4), (2, 300, 0.4, 5), (3, 700, 0.35, 8), (4, 1200, 0.3, 10), (5, 1800, 0.3, 12), (6, 1800, 0.22, 6),
                 (7, 1000, 0.45, 20), (8, 500, 0.3, 3)]


# ---- header, exports, binding ----
def test_header_names_are_exported_and_bound():
    from simpleicp_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(sicp_\w+)\s*\(", text))) == sorted(_lib.CLUSTER_EXPORTS) == ["sicp_cluster", "sicp_cluster_version"]
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", str(so)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sicp_\w+)", out))
    assert set(_lib.CLUSTER_EXPORTS) <= exported
    others = set(_lib.EXPORTS)
    for name, f in _lib.FEATURES.items():
        if name != "cluster":
            others |= set(f.exports)
    assert not set(_lib.CLUSTER_EXPORTS) & others
    f = _lib.FEATURES["cluster"]
    assert f.exports == _lib.CLUSTER_EXPORTS and f.header == HEADER.name and f.version == 1 and f.exports[0] == "sicp_cluster_version"
    L = _lib.load()
    assert "#define SICP_CLUSTER_VERSION 1" in HEADER.read_text()
    assert L.sicp_cluster_version() == _lib.CLUSTER_VERSION == 1 and _lib.cluster_version() == 1
    assert C.sizeof(_lib.ClusterStats) == 56 and [n for n, _ in _lib.ClusterStats._fields_] == list(cluster_ref.KEYS)
    # the main header and its version are untouched, the outlier companion keeps its version
    assert L.sicp_abi_version() == _lib.ABI_VERSION == 7 and _lib.OUTLIER_VERSION == 1
    assert "cluster" not in (ROOT / "include" / "simpleicp_hip.h").read_text().lower()
    assert list(inspect.signature(_lib.Context.cluster).parameters)[1:] == ["slot", "radius", "min_points", "labels_ptr", "core_ptr"]
    assert any(p.name == "sicp_cluster.hip" for p in build.SOURCES) and any(p.name == HEADER.name for p in build.HEADERS)
    # one text of the core test: the unit launches the radius filter's kernel and defines no counting kernel of its own
    unit = (ROOT / "simpleicp_amd" / "csrc" / "sicp_cluster.hip").read_text()
    assert "ball_count_enqueue(" in unit and not re.search(r"\bvoid\s+k_ball_count\b", unit)
    assert len(re.findall(r"\bvoid\s+k_ball_count\b", (ROOT / "simpleicp_amd" / "csrc" / "sicp_outlier.hip").read_text())) == 1


def test_header_is_plain_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    src = tmp_path / "probe.c"
    src.write_text('#include "simpleicp_hip_cluster.h"\n'
                   "int probe(sicp_ctx *c, int32_t *labels, uint8_t *core)\n{\n"
                   "    sicp_cluster_stats st;\n"
                   "    int rc = sicp_cluster_version() + sicp_cluster(c, SICP_FIX, 0.5, 10, labels, core, &st);\n"
                   "    return rc + (int)(st.n_points + st.n_core + st.n_border + st.n_noise + st.n_clusters + st.largest_label + st.largest_size)\n"
                   "           + SICP_CLUSTER_VERSION;\n}\n")
    r = subprocess.run([cc, "-std=c99", "-pedantic", "-Werror", "-Wall", "-Wextra", f"-I{ROOT / 'include'}", "-c", str(src), "-o",
                        str(tmp_path / "probe.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_ctx_is_refused_not_dereferenced():
    from simpleicp_amd import _lib
    L = _lib.load()
    st = _lib.ClusterStats()
    labels = np.full(8, 7, np.int32)
    rc = L.sicp_cluster(None, 0, 1.0, 3, _lib._ptr(labels), None, C.byref(st))
    assert rc == _lib.ERR_INVALID and b"null ctx" in L.sicp_last_error()
    assert np.all(labels == 7)


# ---- the reference against sklearn ----
def test_the_reference_is_sklearns_dbscan():
    sk = pytest.importorskip("sklearn.cluster", reason="sklearn is not installed: the reference stands on its hand cases alone")
    most_border = 0
    for seed, n, r, mp in SKLEARN_CASES:
        X = cluster_ref.blobs(seed, n)
        ref = cluster_ref.cluster(X, r, mp)
        assert ref["n_core"] > 0 and ref["n_border"] > 0 and ref["n_noise"] > 0, (seed, cluster_ref.record(ref))
        most_border = max(most_border, ref["n_border"])
        want = sk.DBSCAN(eps=r, min_samples=mp).fit(X)
        assert np.array_equal(ref["labels"], want.labels_), seed
        assert np.array_equal(np.flatnonzero(ref["core"]), want.core_sample_indices_)
        print(seed, cluster_ref.record(ref))
    assert most_border > 100


def test_both_roads_of_the_reference_agree():
    rng = np.random.default_rng(9)
    X = rng.integers(0, 25, (1500, 3)).astype(np.float64)
    for r, mp in ((1.25, 3), (1.5, 4), (2.3, 9)):
        a, b = cluster_ref.cluster(X, r, mp), cluster_ref.cluster_pairs(X, r, mp)
        assert np.array_equal(a["labels"], b["labels"]) and np.array_equal(a["core"], b["core"])
        assert cluster_ref.record(a) == cluster_ref.record(b)
    assert a["n_clusters"] >= 1 and a["n_core"] > 0


# ---- the reference by hand ----
def rec(**kw):
    return kw


def test_hand_cases():
    one = np.zeros((1, 3))
    r = cluster_ref.cluster(one, 1.0, 1)
    assert r["labels"].tolist() == [0] and r["core"].tolist() == [True]
    assert cluster_ref.record(r) == rec(n_points=1, n_core=1, n_border=0, n_noise=0, n_clusters=1, largest_label=0, largest_size=1)
    r = cluster_ref.cluster(one, 1.0, 2)
    assert r["labels"].tolist() == [-1] and not r["core"].any()
    assert cluster_ref.record(r) == rec(n_points=1, n_core=0, n_border=0, n_noise=1, n_clusters=0, largest_label=-1, largest_size=0)
    # d2 == r * r is no neighbour
    two = np.array([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0]])
    assert cluster_ref.cluster(two, 5.0, 2)["labels"].tolist() == [-1, -1]
    assert cluster_ref.cluster(two, 5.0, 1)["labels"].tolist() == [0, 1]
    assert cluster_ref.cluster(two, np.nextafter(5.0, 6.0), 2)["labels"].tolist() == [0, 0]
    # the bridge: the point at 4 sees both clusters and takes the smaller label, in either order
    B = cluster_ref.bridge()
    r = cluster_ref.cluster(B, 2.1, 5)
    assert r["labels"].tolist() == [0] * 5 + [0] + [1] * 5 and r["core"].tolist() == [True] * 5 + [False] + [True] * 5
    assert cluster_ref.record(r) == rec(n_points=11, n_core=10, n_border=1, n_noise=0, n_clusters=2, largest_label=0, largest_size=6)
    r = cluster_ref.cluster(B[::-1], 2.1, 5)
    assert r["labels"].tolist() == [0] * 5 + [0] + [1] * 5                   # (the clusters have swapped their labels)
    # 64 identical points
    r = cluster_ref.cluster(np.full((64, 3), 2.5), 1e-3, 64)
    assert np.all(r["labels"] == 0) and r["core"].all() and r["largest_size"] == 64
    assert cluster_ref.cluster(np.full((64, 3), 2.5), 1e-3, 65)["n_noise"] == 64
    # min_points = 1: every point is core, an isolated point a cluster of its own
    X = np.array([[0.0, 0, 0], [10.0, 0, 0], [0.5, 0, 0], [20.0, 0, 0], [10.4, 0, 0]])
    r = cluster_ref.cluster(X, 1.0, 1)
    assert r["labels"].tolist() == [0, 1, 0, 2, 1] and r["core"].all() and r["n_clusters"] == 3 and r["largest_label"] == 0
    # min_points > n
    r = cluster_ref.cluster(X, 100.0, 6)
    assert np.all(r["labels"] == -1) and r["n_clusters"] == 0 and r["largest_label"] == -1 and r["largest_size"] == 0
    # a border point that sees only the higher-labelled cluster
    X = np.array([[0.0, 0, 0], [0.1, 0, 0], [0.2, 0, 0], [5.0, 0, 0], [5.1, 0, 0], [5.2, 0, 0], [5.9, 0, 0]])
    r = cluster_ref.cluster(X, 0.75, 3)
    assert r["labels"].tolist() == [0, 0, 0, 1, 1, 1, 1] and r["core"].tolist() == [True] * 6 + [False]


def test_the_lattice_clouds_are_what_the_gpu_tests_expect():
    S = cluster_ref.serpentine()
    r = cluster_ref.cluster_pairs(S, 1.25, 3)
    assert cluster_ref.record(r) == rec(n_points=100_200, n_core=100_198, n_border=2, n_noise=0, n_clusters=1, largest_label=0,
                                        largest_size=100_200)
    P = cluster_ref.patches()
    r = cluster_ref.cluster_pairs(P, 1.25, 3)
    assert r["n_clusters"] == 1000 and r["n_noise"] == len(P) - 100_000 > 100 and r["largest_size"] == 100 and r["largest_label"] == 0
    assert r["n_clusters"] > 1024 // 4                                       # (roots in more than one block of the ranking scan)


# ---- what the binding hands to the C entry ----
class _Recorder:
    """Stands in for the loaded library: the version functions answer with the binding's versions, sicp_cluster notes its arguments."""

    def __init__(self):
        self.calls = []

    def sicp_cluster_version(self):
        from simpleicp_amd import _lib
        return _lib.CLUSTER_VERSION

    def sicp_cluster(self, *args):
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


def test_context_cluster_records_its_arguments(monkeypatch):
    from simpleicp_amd import _lib
    L = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda: L)
    ctx = _lib.Context.__new__(_lib.Context)
    ctx._L, ctx._h, ctx._Q, ctx._bg_src = L, C.c_void_p(0x1234), 5, {}
    ctx.size = lambda slot: 5
    try:
        labels, core, st = ctx.cluster(_lib.FIX, 1, np.int64(3))
        assert labels.dtype == np.int32 and labels.shape == (5,) and core.dtype == np.bool_ and core.shape == (5,)
        assert type(st) is _lib.ClusterStats and len(L.calls) == 1
        a = [_seen(v) for v in L.calls.pop()]
        assert a[:4] == [("ptr", 0x1234), (int, _lib.FIX), (float, 1.0), (int, 3)]
        assert a[4] == ("ptr", labels.ctypes.data) and a[5] == ("ptr", core.ctypes.data) and a[6][0] == "ref" and a[6][1] is st
        st = ctx.cluster(_lib.MOV, 0.25, 10, labels_ptr=0x7000)
        assert type(st) is _lib.ClusterStats
        a = [_seen(v) for v in L.calls.pop()]
        assert a[:6] == [("ptr", 0x1234), (int, _lib.MOV), (float, 0.25), (int, 10), ("ptr", 0x7000), None] and a[6][1] is st
        st = ctx.cluster(_lib.FIX, 0.25, 10, labels_ptr=0x7000, core_ptr=0x7100)
        a = [_seen(v) for v in L.calls.pop()]
        assert a[4:6] == [("ptr", 0x7000), ("ptr", 0x7100)] and not L.calls
    finally:
        ctx._h = C.c_void_p()                  # (nothing to destroy)


# ---- the plumbing on a stand-in context ----
class ClusterOracleContext(oracle_backend.OracleContext):
    """The clouds' entry points of the oracle backend, and cluster answered by the reference."""

    def cluster(self, slot, radius, min_points, labels_ptr=None, core_ptr=None):
        assert labels_ptr is None and core_ptr is None
        self._log("cluster")
        self.cluster_args = (radius, min_points)
        self.cluster_cloud = self.cloud[slot][0].copy()
        r = cluster_ref.cluster(self.cloud[slot][0], radius, min_points)
        return r["labels"], r["core"], cluster_ref.record(r)


@pytest.fixture
def octx(monkeypatch):
    from simpleicp_amd import backend
    ctx = ClusterOracleContext()
    monkeypatch.setattr(backend, "get_context", lambda: ctx)
    return ctx


def test_argument_errors_come_before_the_backend(monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import PointCloud, backend
    from simpleicp_amd.pointcloud import PointCloudException

    def no_backend(*a, **k):
        raise AssertionError("the backend was called")
    monkeypatch.setattr(backend, "get_context", no_backend)
    X = np.random.default_rng(0).standard_normal((50, 3))
    f = simpleicp_amd.cluster_labels
    assert "cluster_labels" in simpleicp_amd.__all__
    sig = inspect.signature(f).parameters
    assert list(sig) == ["X", "radius", "min_points", "return_core", "return_info"]
    assert {n: p.default for n, p in sig.items() if n not in ("X", "radius")} == dict(min_points=10, return_core=False, return_info=False)
    for r in (0.0, -1.0, float("nan"), float("inf"), "wide", True, None, [1.0]):
        with pytest.raises(ValueError, match="radius"):
            f(X, r)
    for m in (0, -1, 2.5, 10.0, "ten", True, None):
        with pytest.raises(ValueError, match="min_points"):
            f(X, 1.0, m)
    with pytest.raises(ValueError, match="return_core"):
        f(X, 1.0, return_core=1)
    with pytest.raises(ValueError, match="return_info"):
        f(X, 1.0, return_info="yes")
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        f(np.zeros((50, 2)), 1.0)
    # an empty cloud has an empty answer, an all-zero record, and needs no backend
    e = f(np.zeros((0, 3)), 1.0)
    assert e.shape == (0,) and e.dtype == np.int32
    e, c, st = f(np.zeros((0, 3)), 1.0, return_core=True, return_info=True)
    assert e.shape == (0,) and c.shape == (0,) and c.dtype == bool and st == dict.fromkeys(cluster_ref.KEYS, 0)
    pc = PointCloud(X, columns=["x", "y", "z"])
    for call in (pc.select_largest_cluster, pc.select_clusters):
        with pytest.raises(PointCloudException, match="radius"):
            call(0.0)
        with pytest.raises(PointCloudException, match="min_points"):
            call(1.0, 0)
    for bad in (0, -2, 1.5, True, "3"):
        with pytest.raises(PointCloudException, match="min_size"):
            pc.select_clusters(1.0, 3, bad)
    pc.unselect_all_points()                       # nothing selected: nothing to do, no backend
    pc.select_largest_cluster(1.0)
    pc.select_clusters(1.0)
    assert pc.num_selected_points == 0 and pc.last_cluster_stats is None
    assert list(inspect.signature(PointCloud.select_largest_cluster).parameters)[1:3] == ["radius", "min_points"]
    assert list(inspect.signature(PointCloud.select_clusters).parameters)[1:4] == ["radius", "min_points", "min_size"]


def test_a_distributed_job_is_refused(monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import backend, dist
    from simpleicp_amd.icp import SimpleICPException
    monkeypatch.setattr(dist, "is_distributed", lambda: True)
    monkeypatch.setattr(backend, "get_context", lambda: (_ for _ in ()).throw(AssertionError("the backend was called")))
    with pytest.raises(SimpleICPException, match="cluster_labels does not run in a torch.distributed job"):
        simpleicp_amd.cluster_labels(np.random.default_rng(0).standard_normal((50, 3)), 1.0)


def test_cluster_labels_and_the_selectors_on_host_clouds(octx, monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import PointCloud, _lib, backend
    X = cluster_ref.blobs(21, 600)
    ref = cluster_ref.cluster(X, 0.4, 6)
    assert ref["n_clusters"] >= 2 and ref["n_border"] > 0 and ref["n_noise"] > 0
    labels = simpleicp_amd.cluster_labels(X, 0.4, 6)
    assert octx.calls == ["upload", "cluster"] and labels.dtype == np.int32 and np.array_equal(labels, ref["labels"])
    assert octx.cluster_args == (0.4, 6) and type(octx.cluster_args[0]) is float and type(octx.cluster_args[1]) is int
    labels, core = simpleicp_amd.cluster_labels(X, 0.4, min_points=np.int64(6), return_core=True)
    assert np.array_equal(labels, ref["labels"]) and core.dtype == bool and np.array_equal(core, ref["core"])
    labels, info = simpleicp_amd.cluster_labels(X, 0.4, 6, return_info=True)
    assert info == cluster_ref.record(ref) and isinstance(info, dict)
    labels, core, info = simpleicp_amd.cluster_labels(X.astype(np.float32), 0.4, 6, return_core=True, return_info=True)
    wide = cluster_ref.cluster(X.astype(np.float32).astype(np.float64), 0.4, 6)                 # float32 is widened exactly
    assert np.array_equal(labels, wide["labels"]) and np.array_equal(core, wide["core"]) and info == cluster_ref.record(wide)
    assert simpleicp_amd.cluster_labels(X, 0.4)[0] == cluster_ref.cluster(X, 0.4, 10)["labels"][0] and octx.cluster_args == (0.4, 10)
    # a PointCloud: all its points, whatever is selected
    pc = PointCloud(X, columns=["x", "y", "z"])
    pc.select_n_points(300)
    sel = pc.idx_selected
    assert np.array_equal(simpleicp_amd.cluster_labels(pc, 0.4, 6), ref["labels"]) and np.array_equal(pc.idx_selected, sel)
    # the selectors cluster the SELECTED points as a cloud of their own
    alone = cluster_ref.cluster(X[sel], 0.55, 4)
    assert alone["n_clusters"] >= 2 and alone["n_noise"] > 0
    octx.calls.clear()
    pc.select_largest_cluster(0.55, 4, _ctx=octx)
    assert octx.calls == ["upload", "cluster"] and np.array_equal(octx.cluster_cloud, X[sel]) and octx.cluster_args == (0.55, 4)
    assert np.array_equal(pc.idx_selected, sel[alone["labels"] == alone["largest_label"]])
    assert pc.num_selected_points == alone["largest_size"] and pc.last_cluster_stats == cluster_ref.record(alone)
    whole = cluster_ref.cluster(X, 0.55, 4)                                    # (not the whole cloud's clusters)
    assert not np.array_equal(np.flatnonzero(whole["labels"] == whole["largest_label"]), pc.idx_selected)
    # select_clusters(min_size=): composition with select_in_range-style narrowing before and select_n_points after
    pc.select_all_points()
    pc.select_by_indices(np.flatnonzero(X[:, 0] < 4.0))
    sel = pc.idx_selected
    alone = cluster_ref.cluster(X[sel], 0.45, 5)
    sizes = np.bincount(alone["labels"][alone["labels"] >= 0])
    assert len(sizes) >= 2 and sizes.min() < sizes.max()
    cut = int(sizes.min()) + 1
    pc.select_clusters(0.45, 5, min_size=cut, _ctx=octx)
    want = sel[(alone["labels"] >= 0) & (sizes[np.maximum(alone["labels"], 0)] >= cut)]
    assert np.array_equal(pc.idx_selected, want) and 0 < len(want) < int((alone["labels"] >= 0).sum())
    assert pc.last_cluster_stats == cluster_ref.record(alone)
    pc.select_n_points(50)
    assert pc.num_selected_points <= 50 and set(pc.idx_selected) <= set(want)
    pc.select_all_points()
    pc.select_clusters(0.45, 5, _ctx=octx)                                     # min_size = 1: everything but the noise
    all_ = cluster_ref.cluster(X, 0.45, 5)
    assert np.array_equal(pc.idx_selected, np.flatnonzero(all_["labels"] >= 0))
    pc.select_largest_cluster(1e-6, 2, _ctx=octx)                              # no cluster at all: nothing stays
    assert pc.num_selected_points == 0 and pc.last_cluster_stats["n_clusters"] == 0 and pc.last_cluster_stats["largest_label"] == -1
    monkeypatch.setattr(backend, "get_context", lambda: oracle_backend.OracleContext())      # a backend without the entry point
    with pytest.raises(_lib.BackendError, match="clustering"):
        simpleicp_amd.cluster_labels(X, 0.4, 6)
