"""Farthest point sampling (contract (S)), the parts that need no GPU: the companion header and the binding,
what Context.farthest hands to the C entry in both forms, the argument checks, the plumbing of farthest_points and
PointCloud.select_farthest on a stand-in context that answers with tests/farthest_ref.py, and the reference itself on
constructed inputs."""
import ctypes as C
import inspect
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import farthest_ref
import oracle_backend

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "simpleicp_hip_farthest.h"


# ---- header, exports, binding ----
def test_header_names_are_exported_and_bound():
    from simpleicp_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(sicp_\w+)\s*\(", text))) == sorted(_lib.FARTHEST_EXPORTS) == ["sicp_farthest", "sicp_farthest_version"]
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", str(so)], capture_output=True, text=True, check=True).stdout
    assert set(_lib.FARTHEST_EXPORTS) <= set(re.findall(r" T (sicp_\w+)", out))
    others = set(_lib.EXPORTS)
    for name, f in _lib.FEATURES.items():
        if name != "farthest":
            others |= set(f.exports)
    assert not set(_lib.FARTHEST_EXPORTS) & others
    f = _lib.FEATURES["farthest"]
    assert f.exports == _lib.FARTHEST_EXPORTS and f.header == HEADER.name and f.version == 1 and f.exports[0] == "sicp_farthest_version"
    L = _lib.load()
    assert "#define SICP_FARTHEST_VERSION 1" in HEADER.read_text() and "#define SICP_FARTHEST_ONE_LIMIT 12288" in HEADER.read_text()
    assert L.sicp_farthest_version() == _lib.FARTHEST_VERSION == 1 and _lib.farthest_version() == 1 and _lib.FARTHEST_ONE_LIMIT == 12288
    assert C.sizeof(_lib.FarthestStats) == 32 and [n for n, _ in _lib.FarthestStats._fields_] == list(farthest_ref.KEYS)
    assert issubclass(_lib.FarthestStats, _lib._Stats) and type(_lib.FarthestStats().as_dict()["cover_d2"]) is float
    # the contract has a letter of its own, and the header carries it
    assert "contract (S)" in HEADER.read_text() and "fma(dz, dz, fma(dy, dy, dx * dx))" in HEADER.read_text()
    # the main header and its version are untouched
    assert L.sicp_abi_version() == _lib.ABI_VERSION == 7
    assert "farthest" not in (ROOT / "include" / "simpleicp_hip.h").read_text()
    assert any(p.name == "sicp_farthest.hip" for p in build.SOURCES) and any(p.name == HEADER.name for p in build.HEADERS)
    assert list(inspect.signature(_lib.Context.farthest).parameters)[1:5] == ["X", "count", "start", "mask"]
    # the switches are read where the others are
    api = (ROOT / "simpleicp_amd" / "csrc" / "sicp_api.cpp").read_text()
    assert 'getenv("SICP_FARTHEST_ONE_MAX")' in api and 'getenv("SICP_FARTHEST_SPAN")' in api


def test_header_is_plain_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    src = tmp_path / "probe.c"
    src.write_text('#include "simpleicp_hip_farthest.h"\n'
                   "int probe(sicp_ctx *c, const double *X, const uint8_t *mask, int64_t *idx, double *d2)\n{\n"
                   "    sicp_farthest_stats a;\n"
                   "    int rc = sicp_farthest_version() + sicp_farthest(c, X, mask, 100, 8, -1, idx, d2, &a);\n"
                   "    return rc + (int)(a.n_points + a.n_candidates + a.n_selected) + (a.cover_d2 > 0.0) + SICP_FARTHEST_VERSION\n"
                   "           + SICP_FARTHEST_ONE_LIMIT;\n}\n")
    r = subprocess.run([cc, "-std=c99", "-pedantic", "-Werror", "-Wall", "-Wextra", f"-I{ROOT / 'include'}", "-c", str(src), "-o",
                        str(tmp_path / "probe.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_ctx_is_refused_not_dereferenced():
    from simpleicp_amd import _lib
    L = _lib.load()
    X, idx, d2 = np.zeros((8, 3)), np.full(4, 7, np.int64), np.full(4, 5.0)
    st = _lib.FarthestStats()
    rc = L.sicp_farthest(None, _lib._ptr(X), None, 8, 4, -1, _lib._ptr(idx), _lib._ptr(d2), C.byref(st))
    assert rc == _lib.ERR_INVALID and b"null ctx" in L.sicp_last_error()
    assert np.all(idx == 7) and np.all(d2 == 5.0)


# ---- what the binding hands to the C entry ----
class _Recorder:
    """Stands in for the loaded library: the version function answers with the binding's version, the entry notes its arguments."""

    def __init__(self):
        self.calls = []

    def sicp_farthest_version(self):
        from simpleicp_amd import _lib
        return _lib.FARTHEST_VERSION

    def sicp_farthest(self, *args):
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


def test_context_farthest_records_its_arguments(monkeypatch):
    from simpleicp_amd import _lib
    L = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda: L)
    ctx = _lib.Context.__new__(_lib.Context)
    ctx._L, ctx._h, ctx._Q, ctx._bg_src = L, C.c_void_p(0x1234), 5, {}
    try:
        X = np.random.default_rng(0).standard_normal((9, 3))
        mask = np.array([1, 0, 2, 1, 1, 0, 1, 1, 1])
        idx, d2, st = ctx.farthest(X, np.int64(4), mask=mask)
        assert idx.shape == (4,) and idx.dtype == np.int64 and d2.shape == (4,) and d2.dtype == np.float64 and type(st) is _lib.FarthestStats
        a = [_seen(v) for v in L.calls.pop()]
        assert a[0] == ("ptr", 0x1234) and a[1][0] == a[2][0] == "ptr" and a[3:6] == [(int, 9), (int, 4), (int, -1)]
        assert a[6] == ("ptr", idx.ctypes.data) and a[7] == ("ptr", d2.ctypes.data) and a[8][0] == "ref" and a[8][1] is st
        idx, d2, st = ctx.farthest(X, 3, 8, want_d2=False)
        a = [_seen(v) for v in L.calls.pop()]
        assert d2 is None and a[2] is None and a[7] is None and a[3:6] == [(int, 9), (int, 3), (int, 8)]
        st = ctx.farthest(0x5000, 7, 2, mask=0x5800, n=100, idx_ptr=0x7000, d2_ptr=0x7100)
        assert type(st) is _lib.FarthestStats
        a = [_seen(v) for v in L.calls.pop()]
        assert a[:8] == [("ptr", 0x1234), ("ptr", 0x5000), ("ptr", 0x5800), (int, 100), (int, 7), (int, 2), ("ptr", 0x7000), ("ptr", 0x7100)]
        st = ctx.farthest(0x5000, 7, n=100, idx_ptr=0x7000)
        a = [_seen(v) for v in L.calls.pop()]
        assert a[:8] == [("ptr", 0x1234), ("ptr", 0x5000), None, (int, 100), (int, 7), (int, -1), ("ptr", 0x7000), None] and not L.calls
        for bad in (np.zeros((9, 2)), np.zeros(9)):
            with pytest.raises(ValueError, match=r"\(n, 3\)"):
                ctx.farthest(bad, 2)
        with pytest.raises(ValueError, match="mask"):
            ctx.farthest(X, 2, mask=np.ones(8))
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
    f = simpleicp_amd.farthest_points
    assert "farthest_points" in simpleicp_amd.__all__
    sig = inspect.signature(f).parameters
    assert list(sig) == ["X", "count", "start", "mask", "return_distances", "return_info"]
    assert {n: p.default for n, p in sig.items() if n not in ("X", "count")} == dict(start=None, mask=None, return_distances=False,
                                                                                      return_info=False)
    assert all(sig[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("start", "mask", "return_distances", "return_info"))
    assert features.farthest_arguments(8) == (8, -1) and features.farthest_arguments(np.int32(8), 3) == (8, 3)
    for c in (2.5, "many", True, None):
        with pytest.raises(TypeError, match="count"):
            f(X, c)
    for c in (0, -1, 2**31):
        with pytest.raises(ValueError, match="count"):
            f(X, c)
    for s in (1.0, "first", False):
        with pytest.raises(TypeError, match="start"):
            f(X, 5, start=s)
    for s in (-1, 50, 2**31):
        with pytest.raises(ValueError, match="start"):
            f(X, 5, start=s)
    with pytest.raises(TypeError, match="return_distances"):
        f(X, 5, return_distances=1)
    with pytest.raises(TypeError, match="return_info"):
        f(X, 5, return_info="yes")
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        f(np.zeros((50, 2)), 5)
    with pytest.raises(ValueError, match="no rows"):
        f(np.zeros((0, 3)), 5)
    for m in (np.ones(49, bool), np.ones(50), "all"):
        with pytest.raises(TypeError, match="mask"):
            f(X, 5, mask=m)
    pc = PointCloud(X, columns=["x", "y", "z"])
    with pytest.raises(PointCloudException, match="count"):
        pc.select_farthest(0)
    with pytest.raises(PointCloudException, match="count"):
        pc.select_farthest(2.0)
    with pytest.raises(PointCloudException, match="start"):
        pc.select_farthest(5, start=50)
    pc.select_by_indices([3, 4])
    with pytest.raises(PointCloudException, match="start must be a selected point"):
        pc.select_farthest(2, start=5)
    pc.unselect_all_points()                       # nothing selected: nothing to do, no backend
    pc.select_farthest(5)
    assert pc.num_selected_points == 0 and pc.last_farthest is None


def test_a_distributed_job_is_refused(monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import backend, dist
    from simpleicp_amd.icp import SimpleICPException
    monkeypatch.setattr(dist, "is_distributed", lambda: True)
    monkeypatch.setattr(backend, "get_context", lambda: (_ for _ in ()).throw(AssertionError("the backend was called")))
    with pytest.raises(SimpleICPException, match="farthest_points does not run in a torch.distributed job"):
        simpleicp_amd.farthest_points(np.zeros((5, 3)), 2)


# ---- the plumbing on a stand-in context ----
class FarthestOracleContext(oracle_backend.OracleContext):
    """The oracle backend, and the farthest entry answered by the reference (host form only)."""

    def __init__(self):
        super().__init__()
        self.seen = []

    def farthest(self, X, count, start=-1, mask=None, n=None, idx_ptr=None, d2_ptr=None, want_d2=True):
        assert n is None and idx_ptr is None and d2_ptr is None and type(count) is int and type(start) is int
        assert X.dtype == np.float64 and X.flags.c_contiguous and (mask is None or mask.dtype == bool)
        self._log("farthest")
        self.seen.append((count, start, None if mask is None else mask.copy(), want_d2))
        idx, d2, rec = farthest_ref.farthest(X, mask, count, start)
        return idx, (d2 if want_d2 else None), rec


@pytest.fixture
def octx(monkeypatch):
    from simpleicp_amd import backend
    ctx = FarthestOracleContext()
    monkeypatch.setattr(backend, "get_context", lambda: ctx)
    return ctx


def test_farthest_points_on_host_clouds(octx, monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import PointCloud, _lib, backend
    X = farthest_ref.cloud(1, 400)
    want = farthest_ref.farthest(X, None, 32)
    got = simpleicp_amd.farthest_points(X, 32)
    assert octx.calls == ["farthest"] and octx.seen[-1][:2] == (32, -1) and octx.seen[-1][3] is False
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, want[0]) and got[0] == 0
    idx, d2 = simpleicp_amd.farthest_points(X, 32, start=17, return_distances=True)
    want = farthest_ref.farthest(X, None, 32, 17)
    assert octx.seen[-1][1] == 17 and octx.seen[-1][3] is True and idx[0] == 17
    assert np.array_equal(idx, want[0]) and d2.tobytes() == want[1].tobytes() and d2[0] == np.inf
    idx, info = simpleicp_amd.farthest_points(X, 32, return_info=True)
    assert tuple(info) == farthest_ref.KEYS and info == farthest_ref.farthest(X, None, 32)[2] and info["n_selected"] == 32
    idx, d2, info = simpleicp_amd.farthest_points(X, 8, return_distances=True, return_info=True)
    assert len(idx) == len(d2) == 8 and info["cover_d2"] <= d2[-1]
    # float32 is widened exactly; a PointCloud gives all its points
    wide = X.astype(np.float32).astype(np.float64)
    assert np.array_equal(simpleicp_amd.farthest_points(X.astype(np.float32), 16), farthest_ref.farthest(wide, None, 16)[0])
    pc = PointCloud(X, columns=["x", "y", "z"])
    pc.select_n_points(30)
    assert np.array_equal(simpleicp_amd.farthest_points(pc, 32), farthest_ref.farthest(X, None, 32)[0]) and pc.num_selected_points <= 30
    # a mask: only candidate rows are picked; the bytes 0 / 1 / 3 arrive as bool
    mask = np.random.default_rng(5).random(len(X)) < 0.5
    got = simpleicp_amd.farthest_points(X, 20, mask=mask.astype(np.uint8) * 3)
    assert np.array_equal(got, farthest_ref.farthest(X, mask, 20)[0]) and mask[got].all() and np.array_equal(octx.seen[-1][2], mask)
    assert got[0] == np.flatnonzero(mask)[0]
    # not padded: duplicates end the selection early, a count above n is n, a start that is no candidate selects nothing
    R = farthest_ref.repeated(7, 5)
    idx, d2, info = simpleicp_amd.farthest_points(R, 30, return_distances=True, return_info=True)
    assert len(idx) == len(d2) == 7 and info["n_selected"] == 7 and info["cover_d2"] == 0.0 and octx.seen[-1][0] == 30
    assert len(simpleicp_amd.farthest_points(X[:10], 500)) == 10 and octx.seen[-1][0] == 10
    off = mask.copy()
    off[3] = False
    idx, info = simpleicp_amd.farthest_points(X, 20, start=3, mask=off, return_info=True)
    assert len(idx) == 0 and idx.dtype == np.int64 and info["n_selected"] == 0
    monkeypatch.setattr(backend, "get_context", lambda: oracle_backend.OracleContext())      # a backend without the entry point
    with pytest.raises(_lib.BackendError, match="farthest point sampling"):
        simpleicp_amd.farthest_points(X, 5)


def test_select_farthest_narrows_the_selection(octx):
    from simpleicp_amd import PointCloud
    X = farthest_ref.cloud(2, 300)
    pc = PointCloud(X, columns=["x", "y", "z"])
    sel = np.flatnonzero(np.random.default_rng(2).random(len(X)) < 0.6)
    pc.select_by_indices(sel)
    mask = np.zeros(len(X), bool)
    mask[sel] = True
    want = farthest_ref.farthest(X, mask, 25)
    pc.select_farthest(25, _ctx=octx)
    assert octx.calls == ["farthest"] and np.array_equal(octx.seen[-1][2], mask) and octx.seen[-1][:2] == (25, -1)   # the selection is the mask
    assert np.array_equal(pc.idx_selected, np.sort(want[0])) and set(pc.idx_selected) <= set(sel) and pc.num_selected_points == 25
    idx, d2, rec = pc.last_farthest
    assert np.array_equal(idx, want[0]) and d2.tobytes() == want[1].tobytes() and rec == want[2] and idx[0] == sel[0]
    # with a prior selection and a start: a row of the cloud, which must be selected; it narrows again
    start = int(pc.idx_selected[7])
    now = np.zeros(len(X), bool)
    now[pc.idx_selected] = True
    want = farthest_ref.farthest(X, now, 10, start)
    pc.select_farthest(10, start=start, _ctx=octx)
    assert octx.seen[-1][:2] == (10, start) and np.array_equal(octx.seen[-1][2], now)
    assert np.array_equal(pc.last_farthest[0], want[0]) and pc.last_farthest[0][0] == start and pc.num_selected_points == 10
    pc.select_n_points(4)                                                      # composes with the other selectors
    assert pc.num_selected_points <= 4 and set(pc.idx_selected) <= set(want[0])
    pc.select_farthest(100, _ctx=octx)                                         # more than are selected: they all stay
    assert pc.num_selected_points <= 4 and octx.seen[-1][0] == 100


# ---- the reference alone on constructed inputs ----
@pytest.mark.parametrize("seed,n,m", [(1, 500, 500), (2, 777, 64), (3, 64, 64)])
def test_distances_never_increase(seed, n, m):
    idx, d2, rec = farthest_ref.farthest(farthest_ref.cloud(seed, n), None, m)
    assert rec["n_selected"] == m and d2[0] == np.inf
    assert (d2[2:] <= d2[1:-1]).all()                   # exactly: m_i only ever decreases, and D_t is a maximum over them
    assert rec["cover_d2"] <= d2[-1] and (rec["cover_d2"] == 0.0) == (m == n)


def test_a_prefix_of_a_run_is_the_run():
    X = farthest_ref.cloud(4, 600)
    mask = np.random.default_rng(4).random(600) < 0.7
    idx, d2, rec = farthest_ref.farthest(X, mask, 200, 11 if mask[11] else int(np.flatnonzero(mask)[3]))
    for k in (1, 2, 3, 64, 199):
        a, b, r = farthest_ref.farthest(X, mask, k, int(idx[0]))
        assert np.array_equal(a, idx[:k]) and b.tobytes() == d2[:k].tobytes() and r["n_selected"] == k
        assert r["cover_d2"] == d2[k]                   # the covering radius at k picks is the next pick's distance


def test_lattice_ties_go_to_the_lowest_index():
    X = farthest_ref.lattice(4)                         # 64 rows, x fastest
    idx, d2, rec = farthest_ref.farthest(X, None, 64)
    assert idx[:2].tolist() == [0, 63] and d2[:2].tolist() == [np.inf, 27.0]      # the corner opposite row 0, alone at 27
    assert rec["n_selected"] == 64 and sorted(idx) == list(range(64)) and rec["cover_d2"] == 0.0
    # every pick is the lowest index among the rows that are as far as it is
    mi, tied = np.full(64, np.inf), 0
    for t in range(63):
        mi = np.minimum(mi, ((X - X[idx[t]]) ** 2).sum(axis=1))       # (exact: small integers)
        assert idx[t + 1] == np.flatnonzero(mi == mi.max())[0] and d2[t + 1] == mi.max()
        tied += int((mi == mi.max()).sum() > 1)
    assert tied > 20                                    # (the case is about ties: most picks have one)


@pytest.mark.parametrize("p,times,count", [(7, 5, 35), (7, 5, 8), (1, 9, 9), (12, 2, 24)])
def test_repeated_points_select_each_once(p, times, count):
    X = farthest_ref.repeated(p, times, seed=p)
    idx, d2, rec = farthest_ref.farthest(X, None, count)
    assert rec["n_selected"] == p and rec["cover_d2"] == 0.0 and rec["n_candidates"] == p * times
    assert (idx[p:] == -1).all() and d2[p:].tobytes() == np.zeros(count - p).tobytes()
    assert len({X[i].tobytes() for i in idx[:p]}) == p  # p distinct positions, each once


def test_every_pick_is_a_candidate_and_picks_are_distinct():
    X = farthest_ref.cloud(6, 400)
    X[[5, 50, 300]] = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]]
    mask = (np.random.default_rng(6).random(400) < 0.5).astype(np.uint8) * 7
    mask[[5, 50, 300]] = 1
    cand = farthest_ref.candidates(X, mask)
    assert not cand[[5, 50, 300]].any() and cand.sum() == (mask != 0).sum() - 3
    idx, d2, rec = farthest_ref.farthest(X, mask, 400)
    k = rec["n_selected"]
    assert k == rec["n_candidates"] == cand.sum() and cand[idx[:k]].all() and len(set(idx[:k])) == k and (idx[k:] == -1).all()
    assert idx[0] == np.flatnonzero(cand)[0] and np.isfinite(d2[1:k]).all() and (d2[1:k] > 0).all()
    # start that is no candidate, and a cloud without one: nothing is selected
    for start in (5, int(np.flatnonzero(mask == 0)[0])):
        idx, d2, rec = farthest_ref.farthest(X, mask, 10, start)
        assert rec == dict(n_points=400, n_candidates=int(cand.sum()), n_selected=0, cover_d2=0.0) and (idx == -1).all() and not d2.any()
    idx, d2, rec = farthest_ref.farthest(X, np.zeros(400, np.uint8), 10)
    assert rec["n_candidates"] == 0 and rec["n_selected"] == 0 and (idx == -1).all()
    # rows 1e200 apart: d2 overflows to +inf, the ties at +inf go to the lowest index, and cover_d2 may be +inf
    far = np.array([[0.0, 0, 0], [1e200, 0, 0], [0, 1e200, 0], [1.0, 0, 0], [0, 0, -1e200]])
    idx, d2, rec = farthest_ref.farthest(far, None, 3)
    assert idx.tolist() == [0, 1, 2] and d2.tolist() == [np.inf, np.inf, np.inf] and rec["cover_d2"] == np.inf
