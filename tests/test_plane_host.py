"""Planes of a cloud (contracts (P) and (Q)), the parts that need no GPU: the companion header and the
binding, what Context.plane_triplets / plane_refit hand to the C entries, the argument checks and the triple drawing, the plumbing
of segment_plane, segment_planes and PointCloud.select_plane on a stand-in context that answers with tests/plane_ref.py, and the
reference itself on constructed scenes."""
import ctypes as C
import inspect
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle_backend
import plane_ref
import voxel_ref

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "simpleicp_hip_plane.h"
MD = 0.05


# ---- header, exports, binding ----
def test_header_names_are_exported_and_bound():
    from simpleicp_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(sicp_\w+)\s*\(", text))) == sorted(_lib.PLANE_EXPORTS) \
        == ["sicp_plane_refit", "sicp_plane_triplets", "sicp_plane_version"]
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", str(so)], capture_output=True, text=True, check=True).stdout
    assert set(_lib.PLANE_EXPORTS) <= set(re.findall(r" T (sicp_\w+)", out))
    others = set(_lib.EXPORTS)
    for name, f in _lib.FEATURES.items():
        if name != "plane":
            others |= set(f.exports)
    assert not set(_lib.PLANE_EXPORTS) & others
    f = _lib.FEATURES["plane"]
    assert f.exports == _lib.PLANE_EXPORTS and f.header == HEADER.name and f.version == 1 and f.exports[0] == "sicp_plane_version"
    L = _lib.load()
    assert "#define SICP_PLANE_VERSION 1" in HEADER.read_text() and "#define SICP_PLANE_MAX_ROUNDS 16" in HEADER.read_text()
    assert L.sicp_plane_version() == _lib.PLANE_VERSION == 1 and _lib.plane_version() == 1
    assert _lib.PLANE_MAX_ROUNDS == plane_ref.MAX_ROUNDS == 16
    assert C.sizeof(_lib.PlaneStats) == 48 and [n for n, _ in _lib.PlaneStats._fields_] == list(plane_ref.KEYS)
    assert C.sizeof(_lib.PlaneRefitStats) == 40 and [n for n, _ in _lib.PlaneRefitStats._fields_] == list(plane_ref.REFIT_KEYS)
    assert issubclass(_lib.PlaneStats, _lib._Stats) and issubclass(_lib.PlaneRefitStats, _lib._Stats)
    # the main header and its version are untouched
    assert L.sicp_abi_version() == _lib.ABI_VERSION == 7
    assert "plane_triplets" not in (ROOT / "include" / "simpleicp_hip.h").read_text()
    assert any(p.name == "sicp_plane.hip" for p in build.SOURCES) and any(p.name == HEADER.name for p in build.HEADERS)
    assert list(inspect.signature(_lib.Context.plane_triplets).parameters)[1:5] == ["X", "triples", "max_distance", "mask"]
    assert list(inspect.signature(_lib.Context.plane_refit).parameters)[1:6] == ["X", "planes", "max_distance", "rounds", "mask"]


def test_header_is_plain_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    src = tmp_path / "probe.c"
    src.write_text('#include "simpleicp_hip_plane.h"\n'
                   "int probe(sicp_ctx *c, const double *X, const uint8_t *mask, const int32_t *tri, double *planes, int32_t *inl, uint8_t *keep)\n{\n"
                   "    sicp_plane_stats a;\n    sicp_plane_refit_stats b;\n"
                   "    int rc = sicp_plane_version() + sicp_plane_triplets(c, X, 100, mask, tri, 8, 0.05, planes, inl, &a)\n"
                   "             + sicp_plane_refit(c, X, 100, mask, planes, 1, 0.05, SICP_PLANE_MAX_ROUNDS, planes, inl, keep, &b);\n"
                   "    return rc + (int)(a.n_points + a.n_candidates + a.n_hypotheses + a.n_void + a.best + a.best_inliers)\n"
                   "           + (int)(b.n_planes + b.n_void + b.n_improved + b.best + b.best_inliers) + SICP_PLANE_VERSION;\n}\n")
    r = subprocess.run([cc, "-std=c99", "-pedantic", "-Werror", "-Wall", "-Wextra", f"-I{ROOT / 'include'}", "-c", str(src), "-o",
                        str(tmp_path / "probe.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_ctx_is_refused_not_dereferenced():
    from simpleicp_amd import _lib
    L = _lib.load()
    X, tri, inl, P = np.zeros((8, 3)), np.zeros((2, 3), np.int32), np.full(2, 7, np.int32), np.full((2, 4), 5.0)
    st, st2 = _lib.PlaneStats(), _lib.PlaneRefitStats()
    rc = L.sicp_plane_triplets(None, _lib._ptr(X), 8, None, _lib._ptr(tri), 2, 0.1, _lib._ptr(P), _lib._ptr(inl), C.byref(st))
    assert rc == _lib.ERR_INVALID and b"null ctx" in L.sicp_last_error()
    rc = L.sicp_plane_refit(None, _lib._ptr(X), 8, None, _lib._ptr(P), 2, 0.1, 3, _lib._ptr(P), _lib._ptr(inl), None, C.byref(st2))
    assert rc == _lib.ERR_INVALID and b"null ctx" in L.sicp_last_error()
    assert np.all(inl == 7) and np.all(P == 5.0)


# ---- what the binding hands to the C entries ----
class _Recorder:
    """Stands in for the loaded library: the version function answers with the binding's version, the entries note their arguments."""

    def __init__(self):
        self.calls = []

    def sicp_plane_version(self):
        from simpleicp_amd import _lib
        return _lib.PLANE_VERSION

    def sicp_plane_triplets(self, *args):
        self.calls.append(("triplets",) + args)
        return 0

    def sicp_plane_refit(self, *args):
        self.calls.append(("refit",) + args)
        return 0


def _seen(a):
    if a is None:
        return None
    if isinstance(a, C.c_void_p):
        return ("ptr", a.value)
    if hasattr(a, "_obj"):
        return ("ref", a._obj)
    return (type(a), a)


def test_context_plane_calls_record_their_arguments(monkeypatch):
    from simpleicp_amd import _lib
    L = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda: L)
    ctx = _lib.Context.__new__(_lib.Context)
    ctx._L, ctx._h, ctx._Q, ctx._bg_src = L, C.c_void_p(0x1234), 5, {}
    try:
        X = np.random.default_rng(0).standard_normal((9, 3))
        tri = np.array([[0, 1, 2], [3, 4, 5]])
        mask = np.array([1, 0, 2, 1, 1, 0, 1, 1, 1])
        planes, inl, st = ctx.plane_triplets(X, tri, 1, mask=mask)
        assert planes.shape == (2, 4) and planes.dtype == np.float64 and inl.shape == (2,) and inl.dtype == np.int32
        assert type(st) is _lib.PlaneStats and len(L.calls) == 1
        a = [_seen(v) for v in L.calls.pop()[1:]]
        assert a[0] == ("ptr", 0x1234) and a[2] == (int, 9) and a[5] == (int, 2) and a[6] == (float, 1.0)
        assert a[1][0] == a[3][0] == a[4][0] == "ptr" and a[7] == ("ptr", planes.ctypes.data) and a[8] == ("ptr", inl.ctypes.data)
        assert a[9][0] == "ref" and a[9][1] is st
        planes, inl, st = ctx.plane_triplets(X, tri, 0.5, want_planes=False)
        a = [_seen(v) for v in L.calls.pop()[1:]]
        assert planes is None and a[3] is None and a[7] is None
        st = ctx.plane_triplets(0x5000, 0x6000, 0.25, mask=0x5800, n=100, h=7, planes_ptr=0x7000, inliers_ptr=0x7100)
        assert type(st) is _lib.PlaneStats
        a = [_seen(v) for v in L.calls.pop()[1:]]
        assert a[:9] == [("ptr", 0x1234), ("ptr", 0x5000), (int, 100), ("ptr", 0x5800), ("ptr", 0x6000), (int, 7), (float, 0.25),
                         ("ptr", 0x7000), ("ptr", 0x7100)]
        out, cnt, keep, st = ctx.plane_refit(X, [[0, 0, 1, 0]], 0.5, np.int64(3), mask=mask, want_keep=True)
        assert out.shape == (1, 4) and cnt.shape == (1,) and keep.shape == (9,) and keep.dtype == np.bool_ and type(st) is _lib.PlaneRefitStats
        a = [_seen(v) for v in L.calls.pop()[1:]]
        assert a[2] == (int, 9) and a[5] == (int, 1) and a[6] == (float, 0.5) and a[7] == (int, 3) and a[8] == ("ptr", out.ctypes.data)
        assert a[9] == ("ptr", cnt.ctypes.data) and a[10][0] == "ptr" and a[11][1] is st
        assert ctx.plane_refit(X, np.zeros((2, 4)), 0.5, 1)[2] is None
        assert _seen(L.calls.pop()[11]) is None
        st = ctx.plane_refit(0x5000, 0x6000, 0.25, 2, n=100, b=1, planes_ptr=0x7000, inliers_ptr=0x7100, keep_ptr=0x7200)
        a = [_seen(v) for v in L.calls.pop()[1:]]
        assert a[:11] == [("ptr", 0x1234), ("ptr", 0x5000), (int, 100), None, ("ptr", 0x6000), (int, 1), (float, 0.25), (int, 2),
                          ("ptr", 0x7000), ("ptr", 0x7100), ("ptr", 0x7200)] and not L.calls
        for bad in (np.zeros((9, 2)), np.zeros(9)):
            with pytest.raises(ValueError, match=r"\(n, 3\)"):
                ctx.plane_triplets(bad, tri, 0.5)
        with pytest.raises(ValueError, match="mask"):
            ctx.plane_triplets(X, tri, 0.5, mask=np.ones(8))
        with pytest.raises(ValueError, match="triples"):
            ctx.plane_triplets(X, np.zeros((2, 2), int), 0.5)
        with pytest.raises(ValueError, match="planes"):
            ctx.plane_refit(X, np.zeros((2, 3)), 0.5, 1)
    finally:
        ctx._h = C.c_void_p()                  # (nothing to destroy)


# ---- argument checks ----
def test_argument_errors_come_before_the_backend(monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import PointCloud, backend, features
    from simpleicp_amd.pointcloud import PointCloudException

    def no_backend(*a, **k):
        raise AssertionError("the backend was called")
    monkeypatch.setattr(backend, "get_context", no_backend)
    X = np.random.default_rng(0).standard_normal((50, 3))
    f, g = simpleicp_amd.segment_plane, simpleicp_amd.segment_planes
    for name in ("segment_plane", "segment_planes", "PlaneResult"):
        assert name in simpleicp_amd.__all__
    sig = inspect.signature(f).parameters
    assert list(sig) == ["X", "max_distance", "hypotheses", "seed", "triples", "refine", "mask", "return_info"]
    assert {n: p.default for n, p in sig.items() if n not in ("X", "max_distance")} == dict(
        hypotheses=1024, seed=0, triples=None, refine=3, mask=None, return_info=False)
    sig = inspect.signature(g).parameters
    assert sig["min_inliers"].default is inspect.Parameter.empty and sig["max_planes"].default == 4
    assert features.plane_arguments(1, 8, 3, [[0, 1, 2]], 2)[:3] == (1.0, 8, 3)
    for d in ("wide", True, None, [1.0]):
        with pytest.raises(TypeError, match="max_distance"):
            f(X, d)
    for d in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_distance"):
            f(X, d)
    for h in (2.5, "many", True, None):
        with pytest.raises(TypeError, match="hypotheses"):
            f(X, MD, hypotheses=h)
    for h in (0, -1, 2**31):
        with pytest.raises(ValueError, match="hypotheses"):
            f(X, MD, hypotheses=h)
    with pytest.raises(TypeError, match="seed"):
        f(X, MD, seed=1.5)
    for s in (-1, [], [1, -2]):
        with pytest.raises(ValueError, match="seed"):
            f(X, MD, seed=s)
    with pytest.raises(TypeError, match="triples"):
        f(X, MD, triples=np.zeros((4, 3)))
    for t in (np.zeros((4, 2), int), np.zeros((0, 3), int), np.zeros(3, int), np.array([[0, 1, 2**31]])):
        with pytest.raises(ValueError, match="triples"):
            f(X, MD, triples=t)
    with pytest.raises(TypeError, match="refine"):
        f(X, MD, refine=1.0)
    for r in (0, -1, 17):                                                      # refine = 0: the refit forms the mask, there is no skipping it
        with pytest.raises(ValueError, match="refine"):
            f(X, MD, refine=r)
    with pytest.raises(TypeError, match="return_info"):
        f(X, MD, return_info=1)
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        f(np.zeros((50, 2)), MD)
    for m in (np.ones(49, bool), np.ones(50), "all"):
        with pytest.raises(TypeError, match="mask"):
            f(X, MD, mask=m)
    with pytest.raises(ValueError, match="at least 3 candidate rows"):
        f(X[:2], MD)
    two = np.zeros(50, bool)
    two[:2] = True
    with pytest.raises(ValueError, match="at least 3 candidate rows"):
        f(X, MD, mask=two)
    with pytest.raises(TypeError, match="min_inliers"):
        g(X, MD)
    with pytest.raises(ValueError, match="min_inliers"):
        g(X, MD, min_inliers=0)
    with pytest.raises(ValueError, match="max_planes"):
        g(X, MD, min_inliers=10, max_planes=0)
    with pytest.raises(TypeError, match="seed"):
        g(X, MD, min_inliers=10, seed=[1, 2])
    pc = PointCloud(X, columns=["x", "y", "z"])
    with pytest.raises(PointCloudException, match="max_distance"):
        pc.select_plane(0.0)
    with pytest.raises(PointCloudException, match="refine"):
        pc.select_plane(MD, refine=0)
    with pytest.raises(PointCloudException, match="invert"):
        pc.select_plane(MD, invert=1)
    with pytest.raises(PointCloudException, match="no keyword 'mask'"):
        pc.select_plane(MD, mask=two)
    pc.select_by_indices([3, 4])
    with pytest.raises(PointCloudException, match="at least 3 candidate rows"):
        pc.select_plane(MD)
    pc.unselect_all_points()                       # nothing selected: nothing to do, no backend
    pc.select_plane(MD)
    assert pc.num_selected_points == 0 and pc.last_plane is None


def test_a_distributed_job_is_refused(monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import backend, dist
    from simpleicp_amd.icp import SimpleICPException
    monkeypatch.setattr(dist, "is_distributed", lambda: True)
    monkeypatch.setattr(backend, "get_context", lambda: (_ for _ in ()).throw(AssertionError("the backend was called")))
    X = np.random.default_rng(0).standard_normal((50, 3))
    with pytest.raises(SimpleICPException, match="segment_plane does not run in a torch.distributed job"):
        simpleicp_amd.segment_plane(X, MD)
    with pytest.raises(SimpleICPException, match="segment_planes does not run in a torch.distributed job"):
        simpleicp_amd.segment_planes(X, MD, min_inliers=5)


# ---- the triples ----
def test_triples_with_and_without_a_mask():
    from simpleicp_amd import features
    a = features.plane_triples(500, None, 64, 7)
    assert a.dtype == np.int32 and a.shape == (64, 3) and a.flags.c_contiguous
    assert np.array_equal(a, np.random.default_rng(7).integers(0, 500, (64, 3), dtype=np.int32))
    assert np.array_equal(a, features.plane_triples(500, None, 64, 7)) and not np.array_equal(a, features.plane_triples(500, None, 64, 8))
    mask = np.random.default_rng(1).random(500) < 0.3
    rows = np.flatnonzero(mask)
    b = features.plane_triples(500, mask, 64, 7)
    assert b.dtype == np.int32 and b.shape == (64, 3) and mask[b].all()       # mapped triples name only candidate rows
    assert np.array_equal(b, rows[np.random.default_rng(7).integers(0, len(rows), (64, 3), dtype=np.int32)])
    assert np.array_equal(b, features.plane_triples(500, mask, 64, 7))
    for seed in (7, [7, 2]):
        for m in (None, mask):
            assert np.array_equal(features.plane_triples(500, m, 64, seed), plane_ref.draw_triples(500, m, 64, seed))
    assert not np.array_equal(features.plane_triples(500, mask, 64, [7, 0]), features.plane_triples(500, mask, 64, [7, 1]))


# ---- the plumbing on a stand-in context ----
class PlaneOracleContext(oracle_backend.OracleContext):
    """The oracle backend, and the two plane entries answered by the reference (host forms only)."""

    def __init__(self):
        super().__init__()
        self.triples, self.masks, self.refits = [], [], []

    def plane_triplets(self, X, triples, max_distance, mask=None, n=None, h=None, planes_ptr=None, inliers_ptr=None, want_planes=True):
        assert planes_ptr is None and inliers_ptr is None and n is None and h is None
        self._log("plane_triplets")
        assert type(max_distance) is float and triples.dtype == np.int32
        self.triples.append(triples.copy())
        self.masks.append(None if mask is None else mask.copy())
        return plane_ref.triplets(X, mask, triples, max_distance)

    def plane_refit(self, X, planes, max_distance, rounds, mask=None, n=None, b=None, planes_ptr=None, inliers_ptr=None, keep_ptr=None,
                    want_keep=False):
        assert planes_ptr is None and inliers_ptr is None and keep_ptr is None and want_keep and planes.shape == (1, 4)
        self._log("plane_refit")
        self.refits.append((planes.copy(), rounds))
        return plane_ref.refit(X, mask, planes, max_distance, rounds, want_keep=True)


@pytest.fixture
def octx(monkeypatch):
    from simpleicp_amd import backend
    ctx = PlaneOracleContext()
    monkeypatch.setattr(backend, "get_context", lambda: ctx)
    return ctx


@pytest.fixture(scope="module")
def two_planes():
    return plane_ref.two_plane_scene()


def test_segment_plane_on_host_clouds(octx, two_planes, monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import PointCloud, _lib, backend
    X = two_planes
    want = plane_ref.segment_plane(X, MD, hypotheses=256, seed=3)
    res = simpleicp_amd.segment_plane(X, MD, hypotheses=256, seed=3)
    assert octx.calls == ["plane_triplets", "plane_refit"] and isinstance(res, simpleicp_amd.PlaneResult)
    assert res.plane.shape == (4,) and res.plane.dtype == np.float64 and res.plane.tobytes() == want[0].tobytes()
    assert res.inliers.dtype == bool and np.array_equal(res.inliers, want[1]) and res.n_inliers == want[2] == int(want[1].sum())
    assert res.info is None and octx.refits[-1][1] == 3 and np.array_equal(octx.triples[-1], plane_ref.draw_triples(len(X), None, 256, 3))
    assert abs(np.linalg.norm(res.plane[:3]) - 1.0) < 1e-15
    res = simpleicp_amd.segment_plane(X, MD, hypotheses=256, seed=3, refine=1, return_info=True)
    assert octx.refits[-1][1] == 1 and tuple(res.info) == ("hypotheses", "refit")
    assert tuple(res.info["hypotheses"]) == plane_ref.KEYS and tuple(res.info["refit"]) == plane_ref.REFIT_KEYS
    best = res.info["hypotheses"]["best"]
    assert res.n_inliers >= res.info["hypotheses"]["best_inliers"] and octx.refits[-1][0].tobytes() == plane_ref.triplets(
        X, None, octx.triples[-1], MD)[0][best:best + 1].tobytes()
    # float32 is widened exactly; a PointCloud gives all its points; the caller's triples go through as they are
    wide = X.astype(np.float32).astype(np.float64)
    assert simpleicp_amd.segment_plane(X.astype(np.float32), MD, hypotheses=64).plane.tobytes() == plane_ref.segment_plane(
        wide, MD, hypotheses=64)[0].tobytes()
    pc = PointCloud(X, columns=["x", "y", "z"])
    pc.select_n_points(300)
    assert np.array_equal(simpleicp_amd.segment_plane(pc, MD, hypotheses=256, seed=3).inliers, want[1]) and pc.num_selected_points <= 300
    tri = np.array([[5, 900, 17], [4, 4, 2], [100, 200, 300]])
    simpleicp_amd.segment_plane(X, MD, triples=tri)
    assert np.array_equal(octx.triples[-1], tri) and octx.triples[-1].dtype == np.int32
    # a mask: only candidate rows count and define planes
    mask = np.random.default_rng(5).random(len(X)) < 0.5
    want = plane_ref.segment_plane(X, MD, hypotheses=256, seed=4, mask=mask)
    res = simpleicp_amd.segment_plane(X, MD, hypotheses=256, seed=4, mask=mask.astype(np.uint8) * 3)
    assert res.plane.tobytes() == want[0].tobytes() and np.array_equal(res.inliers, want[1]) and not (res.inliers & ~mask).any()
    assert mask[octx.triples[-1]].all() and octx.masks[-1].dtype == bool and np.array_equal(octx.masks[-1], mask)
    # no valid hypothesis
    with pytest.raises(ValueError, match="no hypothesis is valid"):
        simpleicp_amd.segment_plane(X, MD, triples=[[1, 1, 2], [0, 5, len(X)]])
    line = np.column_stack([np.arange(10.0)] * 3)
    with pytest.raises(ValueError, match="no hypothesis is valid"):
        simpleicp_amd.segment_plane(line, MD, hypotheses=16)
    monkeypatch.setattr(backend, "get_context", lambda: oracle_backend.OracleContext())      # a backend without the entry points
    with pytest.raises(_lib.BackendError, match="plane segmentation"):
        simpleicp_amd.segment_plane(X, MD)


def test_segment_planes_peels_in_order(octx, two_planes):
    import simpleicp_amd
    X = two_planes
    labels, planes = simpleicp_amd.segment_planes(X, MD, min_inliers=150, hypotheses=256, seed=9)
    want = plane_ref.segment_planes(X, MD, 4, 150, hypotheses=256, seed=9)
    assert labels.dtype == np.int32 and np.array_equal(labels, want[0]) and planes.tobytes() == want[1].tobytes() and planes.shape == (2, 4)
    sizes = np.bincount(labels[labels >= 0])
    assert sizes.tolist() == sorted(sizes, reverse=True) and sizes[1] >= 150                   # in the order of extraction
    # round j: the rows no plane has taken, triples from [seed, j]; the third round finds less than min_inliers and stops
    assert octx.calls == ["plane_triplets", "plane_refit"] * 3
    left = np.ones(len(X), bool)
    for j in range(3):
        assert np.array_equal(octx.masks[j], left)
        assert np.array_equal(octx.triples[j], plane_ref.draw_triples(len(X), left, 256, [9, j]))
        left = left & (labels != j)
    # the stop rules: max_planes, min_inliers
    one = simpleicp_amd.segment_planes(X, MD, min_inliers=150, max_planes=1, hypotheses=256, seed=9)
    assert np.array_equal(one[0], np.where(labels == 0, 0, -1)) and one[1].tobytes() == planes[:1].tobytes()
    big = simpleicp_amd.segment_planes(X, MD, min_inliers=int(sizes[1]) + 1, hypotheses=256, seed=9)
    assert np.array_equal(big[0], one[0]) and big[1].shape == (1, 4)
    none = simpleicp_amd.segment_planes(X, MD, min_inliers=len(X), hypotheses=256, seed=9)
    assert (none[0] == -1).all() and none[1].shape == (0, 4)
    other = simpleicp_amd.segment_planes(X, MD, min_inliers=150, hypotheses=256, seed=10)
    assert np.array_equal(other[0], plane_ref.segment_planes(X, MD, 4, 150, hypotheses=256, seed=10)[0])


def test_select_plane_and_its_complement(octx, two_planes):
    from simpleicp_amd import PointCloud
    X = two_planes
    pc = PointCloud(X, columns=["x", "y", "z"])
    pc.select_by_indices(np.flatnonzero(np.random.default_rng(2).random(len(X)) < 0.6))
    sel = pc.idx_selected
    mask = np.zeros(len(X), bool)
    mask[sel] = True
    want = plane_ref.segment_plane(X, MD, hypotheses=256, seed=5, mask=mask)
    pc.select_plane(MD, hypotheses=256, seed=5, _ctx=octx)
    on = pc.idx_selected
    assert octx.calls == ["plane_triplets", "plane_refit"] and np.array_equal(octx.masks[-1], mask)        # the selection is the mask
    assert np.array_equal(on, np.flatnonzero(want[1])) and set(on) <= set(sel) and pc.last_plane.n_inliers == len(on) == want[2]
    assert pc.last_plane.plane.tobytes() == want[0].tobytes() and tuple(pc.last_plane.info) == ("hypotheses", "refit")
    pc.select_all_points()
    pc.select_by_indices(sel)                                                  # (it narrows: from all points again)
    pc.select_plane(MD, invert=True, hypotheses=256, seed=5, _ctx=octx)
    off = pc.idx_selected
    assert len(on) and len(off) and not set(on) & set(off) and np.array_equal(np.sort(np.concatenate([on, off])), sel)
    pc.select_n_points(50)                                                     # composes with the other selectors
    assert pc.num_selected_points <= 50 and set(pc.idx_selected) <= set(off)


# ---- the reference on constructed scenes ----
def min_width(P2):
    """A lower bound of the smallest width of the planar point set P2 (k, 2) over all directions: the smallest over 3 600 sampled
    directions, less what the width can change between two samples (it is Lipschitz in the angle with the set's diameter)."""
    ang = np.linspace(0.0, np.pi, 3600, endpoint=False)
    proj = P2 @ np.stack([np.cos(ang), np.sin(ang)])
    diameter = 2.0 * np.linalg.norm(P2 - P2.mean(axis=0), axis=1).max()
    return float((proj.max(axis=0) - proj.min(axis=0)).min()) - diameter * (np.pi / 3600)


@pytest.mark.parametrize("seed,normal,offset", [(1, (0.2, -0.3, 1.0), 1.5), (2, (1.0, 0.0, 0.0), -3.0), (3, (-0.5, 0.5, 0.1), 0.0)])
def test_the_reference_recovers_a_noisy_plane_in_clutter(seed, normal, offset):
    X, on, nrm, d = plane_ref.plane_scene(seed, 1500, 1000, normal=normal, offset=offset, noise=MD / 4)
    assert np.abs(X[on] @ nrm - d).max() <= MD / 4 * (1 + 1e-12)
    plane, keep, count = plane_ref.segment_plane(X, MD)                       # the default arguments: 1 024 hypotheses, seed 0, 3 rounds
    assert keep[on].all() and count == int(keep.sum())                        # every plane point is recovered
    assert abs(np.linalg.norm(plane[:3]) - 1.0) < 1e-15
    # The angle.  Every plane point p is within MD of the output plane (it is an inlier) and within e = MD / 4 of the true one.
    # Write the output normal n' = cos(t) n + sin(t) u with u a unit vector in the true plane.  For two plane points p, q:
    # n'.(p - q) = sin(t) u.(p - q) + cos(t) n.(p - q), where |n'.(p - q)| < 2 MD and |n.(p - q)| <= 2 e.  So
    # sin(t) |u.(p - q)| < 2 MD + 2 e for every pair, and with the pair that spans the set's width in direction u:
    # sin(t) < (2 MD + 2 e) / width(u) <= (2 MD + 2 e) / (smallest width of the plane points over all in-plane directions).
    e1 = np.cross(nrm, [1.0, 0.0, 0.0]) if abs(nrm[0]) < 0.9 else np.cross(nrm, [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(nrm, e1)
    width = min_width(np.column_stack([X[on] @ e1, X[on] @ e2]))
    assert width > 15.0
    bound = (2 * MD + 2 * MD / 4) / width
    sin_t = np.linalg.norm(np.cross(plane[:3], nrm))
    assert sin_t < bound and bound < 0.01
    # ... and the clutter it took lies within MD of it
    assert np.abs(X[keep] @ plane[:3] + plane[3]).max() < MD


def test_the_ground_is_the_first_plane_of_the_terrestrial_scan():
    X = voxel_ref.terrestrial_scan(3000) + np.array([0.0, 0.0, 1.8])          # back from the scanner's frame: the ground is z = 0
    ground = np.abs(X[:, 2]) < 0.02
    assert 0.3 * len(X) < ground.sum() < 0.9 * len(X)
    labels, planes = plane_ref.segment_planes(X, MD, 2, 200, hypotheses=256, seed=0)
    assert len(planes) >= 1 and abs(abs(planes[0][2]) - 1.0) < 1e-4 and abs(planes[0][3]) < 0.01
    assert (labels[ground] == 0).all() and (labels == 0).sum() < ground.sum() + 0.02 * len(X)


def test_reference_hand_cases():
    X = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.3, 0.3, 0.5], [0.3, 0.3, -0.5], [2.0, 2.0, 0.25]])
    P, inl, rec = plane_ref.triplets(X, None, [[0, 1, 2], [0, 2, 1], [0, 0, 1], [0, 1, 6]], 0.5)
    assert np.array_equal(P[:2, :3], [[0, 0, 1], [0, 0, -1]]) and inl.tolist() == [4, 4, -1, -1]
    assert rec == dict(n_points=6, n_candidates=6, n_hypotheses=4, n_void=2, best=0, best_inliers=4)
    assert plane_ref.triplets(X, None, [[0, 1, 2]], np.nextafter(0.5, 1.0))[1].tolist() == [6]
    assert plane_ref.triplets(X, [1, 1, 0, 1, 1, 1], [[0, 1, 2]], 0.5)[2] == dict(
        n_points=6, n_candidates=5, n_hypotheses=1, n_void=1, best=-1, best_inliers=-1)
    a, v = plane_ref.jacobi3([[2.0, 1.0, 0.0], [1.0, 2.0, 0.0], [0.0, 0.0, 5.0]])
    assert np.allclose(np.sort(np.diag(a)), [1.0, 3.0, 5.0]) and np.allclose(v @ np.diag(np.diag(a)) @ v.T, [[2, 1, 0], [1, 2, 0], [0, 0, 5]])
    Y, Q = plane_ref.tilting_scene()
    out, cnt, keep, rec = plane_ref.refit(Y, None, Q, 0.1, 5, want_keep=True)
    assert out.tobytes() == Q.tobytes() and cnt.tolist() == [420] and keep.all() and rec["n_improved"] == 0
    out, cnt, keep, rec = plane_ref.refit(Y, None, [[0.0, np.inf, 1.0, 0.0]], 0.1, 5, want_keep=True)
    assert cnt.tolist() == [-1] and not keep.any() and rec == dict(n_planes=1, n_void=1, n_improved=0, best=-1, best_inliers=-1)
