"""Outlier removal (contract (O)), the parts that need no GPU: the reference's own properties
(tests/outlier_ref.py), the companion header and the binding, the refusals that come before any device work, and the host plumbing
of run() / run_batch on the stand-in backend of tests/oracle_backend.py."""
import inspect
import logging
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle_backend
import outlier_ref
from tests.helpers import batch_oracle

ROOT = Path(__file__).resolve().parent.parent


class _OutlierAnswers:
    """The one new entry point of the pipeline, answered by the numpy reference."""

    def outlier_statistical(self, slot, k, std_ratio, rows=None, mask_ptr=None, keep_ptr=None, mean_ptr=None):
        assert mask_ptr is None and keep_ptr is None and mean_ptr is None
        self._log("outlier_statistical")
        self.outlier_args = (int(k), float(std_ratio), None if rows is None else np.array(rows))
        r = outlier_ref.statistical(self.cloud[slot][0], k, std_ratio, rows=rows)
        return r["keep"], r["d"], {key: r[key] for key in ("n_candidates", "n_kept", "mean", "std", "threshold")}


class OutlierOracleContext(_OutlierAnswers, oracle_backend.OracleContext):
    def voxel_select(self, slot, voxel_size, origin=None, rows=None, keep_ptr=None):
        import voxel_ref
        self._log("voxel_select")
        return voxel_ref.keep(self.cloud[slot][0], voxel_size, (0.0, 0.0, 0.0) if origin is None else tuple(origin), rows=rows)


class OutlierBatchContext(_OutlierAnswers, batch_oracle.BatchOracleContext):
    pass


@pytest.fixture
def octx(monkeypatch):
    from simpleicp_amd import backend
    ctx = OutlierOracleContext()
    monkeypatch.setattr(backend, "get_context", lambda: ctx)
    return ctx


def _cloud_with_strays(n=3000, strays=30, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 10.0, (n, 3))
    far = rng.uniform(0.0, 10.0, (strays, 3)) + 15.0                     # a thin cloud of its own, well off the dense one
    return np.ascontiguousarray(np.vstack([X, far])), np.arange(n, n + strays)


# ---- the reference ----
def test_reference_drops_planted_points_and_is_monotone_in_the_ratio():
    X, far = _cloud_with_strays()
    d2 = outlier_ref.neighbour_d2(X, 20)
    assert np.all(d2[:, 0] == 0.0) and np.all(np.diff(d2, axis=1) >= 0)
    r = outlier_ref.statistical(X, 20, 2.0, d2=d2)
    assert not r["keep"][far].any() and r["keep"][:3000].mean() > 0.95
    assert r["n_candidates"] == len(X) and r["n_kept"] == int(r["keep"].sum())
    assert r["threshold"] == r["mean"] + 2.0 * r["std"]
    kept = [outlier_ref.statistical(X, 20, ratio, d2=d2)["keep"] for ratio in (-0.5, 0.0, 1.0, 2.0, 10.0)]
    for a, b in zip(kept, kept[1:]):
        assert not (a & ~b).any() and b.sum() >= a.sum()              # a larger ratio never drops what a smaller one kept
    # a smaller k reads a prefix of the same ranked distances
    assert np.array_equal(outlier_ref.statistical(X, 8, 2.0, d2=d2)["d"], outlier_ref.statistical(X, 8, 2.0)["d"])
    # rows (any order, repeats) and masks: verdicts per entry / per point, statistics over the candidates alone
    rows = np.random.default_rng(1).integers(0, len(X), 500)
    rr = outlier_ref.statistical(X, 20, 2.0, rows=rows, d2=d2)
    assert len(rr["keep"]) == 500 and np.array_equal(rr["d"], r["d"][rows]) and rr["n_candidates"] == 500
    mask = np.zeros(len(X), np.uint8)
    mask[np.unique(rows)] = 1
    rm = outlier_ref.statistical(X, 20, 2.0, mask=mask, d2=d2)
    assert rm["n_candidates"] == len(np.unique(rows)) and not rm["keep"][mask == 0].any() and np.all(rm["d"][mask == 0] == 0.0)
    z = outlier_ref.statistical(X, 20, 2.0, mask=np.zeros(len(X), np.uint8), d2=d2)
    assert (z["n_kept"], z["mean"], z["std"], z["threshold"]) == (0, 0.0, 0.0, 0.0) and not z["keep"].any()
    one = outlier_ref.statistical(X, 20, 2.0, rows=[5], d2=d2)
    assert one["std"] == 0.0 and one["threshold"] == one["mean"] and one["keep"].all()


def test_reference_keeps_duplicates_and_ignores_tie_picks():
    rng = np.random.default_rng(9)
    X = rng.uniform(0, 1, (400, 3))
    X[10:15] = X[3]                                                # point 3 has five exact duplicates
    r = outlier_ref.statistical(X, 6, 0.0)
    assert r["d"][3] == 0.0 and r["keep"][3] and r["keep"][10:15].all()         # k - 1 duplicates: no outlier (Open3D drops d == 0)
    # a lattice: whichever of the equidistant points takes the last rank, its distance -- and so the mean -- is the same
    g = np.arange(5, dtype=np.float64)
    L = np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))
    idx, d2 = outlier_ref.orc.knn(L, L, k=5)
    centre = 62                                                     # (2, 2, 2): six neighbours at distance 1, four of them ranked
    assert list(d2[centre]) == [0.0, 1.0, 1.0, 1.0, 1.0]
    # another tie pick: every point's ranks 1 .. 4 taken by OTHER equidistant points where there are any (the ties reversed, as a
    # search that walks the cloud backwards would pick them), the distances gathered again from the coordinates
    full_idx, full_d2 = outlier_ref.orc.knn(L, L, k=len(L))
    other_idx = idx.copy()
    for i in range(len(L)):
        for lo in range(1, 5):
            if lo > 1 and d2[i, lo] == d2[i, lo - 1]:
                continue
            tied = full_idx[i][full_d2[i] == d2[i, lo]]             # all points at this distance, ascending index
            hi = lo + int(np.count_nonzero(d2[i, lo:] == d2[i, lo]))
            other_idx[i, lo:hi] = tied[::-1][:hi - lo]
    assert (other_idx != idx).any(axis=1).mean() > 0.9 and set(other_idx[centre][1:]) != set(idx[centre][1:])
    other = ((L[other_idx] - L[:, None, :]) ** 2).sum(axis=2)
    assert np.array_equal(np.sort(other, axis=1), other)           # still a ranked neighbour set
    assert np.array_equal(outlier_ref.mean_distance(other), outlier_ref.mean_distance(d2))
    all_equal = outlier_ref.statistical(np.ascontiguousarray(L[[0, 4, 20, 24, 100, 104, 120, 124]]), 2, 0.0)
    assert all_equal["std"] == 0.0 and all_equal["keep"].all()     # equal mean distances: <= keeps them (Open3D's < drops them)


def test_reference_radius():
    rng = np.random.default_rng(2)
    X = rng.uniform(0, 1, (300, 3))
    D2 = outlier_ref.all_d2(X)
    r = outlier_ref.radius(X, 0.15, 5, D2=D2)
    brute = np.array([np.count_nonzero(((X - p) ** 2).sum(1) < 0.15 * 0.15) for p in X])
    assert np.abs(brute - np.minimum(brute, 6)).max() > 0 and np.array_equal(r["count"], np.minimum(brute, 6))
    assert np.array_equal(r["keep"], brute > 5)
    assert outlier_ref.radius(X, 1e-9, 0, D2=D2)["keep"].all() and not outlier_ref.radius(X, 1e-9, 1, D2=D2)["keep"].any()
    assert outlier_ref.radius(X, 10.0, 299, D2=D2)["keep"].all() and not outlier_ref.radius(X, 10.0, 300, D2=D2)["keep"].any()


# ---- header, exports, binding ----
def _header_functions():
    text = (ROOT / "include" / "simpleicp_hip_outlier.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sicp_\w+)\s*\(", text)))


def test_header_names_are_exported_and_bound():
    import ctypes as C
    from simpleicp_amd import _lib, build
    assert _header_functions() == sorted(_lib.OUTLIER_EXPORTS)
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", str(so)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sicp_\w+)", out))
    assert set(_lib.OUTLIER_EXPORTS) <= exported
    others = (set(_lib.EXPORTS) | set(_lib.BATCH_EXPORTS) | set(_lib.DEVICE_EXPORTS) | set(_lib.NORMALS_EXPORTS) | set(_lib.VOXEL_EXPORTS)
              | set(_lib.EVAL_EXPORTS))
    assert not set(_lib.OUTLIER_EXPORTS) & others
    L = _lib.load()
    assert L.sicp_outlier_version() == _lib.OUTLIER_VERSION == 1 and _lib.outlier_version() == 1
    header = (ROOT / "include" / "simpleicp_hip_outlier.h").read_text()
    assert "#define SICP_OUTLIER_VERSION 1" in header
    assert f"#define SICP_OUTLIER_MAX_K {_lib.OUTLIER_MAX_K}" in header
    assert f"#define SICP_OUTLIER_MAX_BOX_CELLS {_lib.OUTLIER_MAX_BOX_CELLS}" in header
    assert C.sizeof(_lib.OutlierStats) == 40
    # the main header and its version are untouched, the other companions keep theirs
    assert L.sicp_abi_version() == _lib.ABI_VERSION == 7
    assert "outlier" not in (ROOT / "include" / "simpleicp_hip.h").read_text()
    assert (_lib.BATCH_VERSION, _lib.DEVICE_VERSION, _lib.NORMALS_VERSION, _lib.VOXEL_VERSION, _lib.EVAL_VERSION) == (1, 1, 1, 1, 1)
    for name in ("outlier_statistical", "outlier_radius", "outlier_radius_cells"):
        assert callable(getattr(_lib.Context, name))
    assert list(inspect.signature(_lib.Context.outlier_statistical).parameters)[1:] == [
        "slot", "k", "std_ratio", "rows", "mask_ptr", "keep_ptr", "mean_ptr"]


def test_null_arguments_are_refused_not_dereferenced():
    """no ctx, so nothing may be touched"""
    import ctypes as C
    from simpleicp_amd import _lib
    L = _lib.load()
    kept, st = C.c_int64(), _lib.OutlierStats()
    buf = np.zeros(4, np.uint8)
    assert L.sicp_outlier_statistical(None, 0, None, 0, None, 5, 2.0, _lib._ptr(buf), None, C.byref(st)) == _lib.ERR_INVALID
    assert b"null ctx" in L.sicp_last_error()
    assert L.sicp_outlier_radius(None, 0, None, 0, None, 1.0, 1, _lib._ptr(buf), None, C.byref(kept)) == _lib.ERR_INVALID
    assert b"null ctx" in L.sicp_last_error()
    assert L.sicp_outlier_radius_cells(None, 0, 1.0, _lib._ptr(np.zeros(4, np.int64))) == _lib.ERR_INVALID


# ---- refusals before any device work ----
def _no_backend(monkeypatch):
    from simpleicp_amd import backend

    def no_backend(*a, **k):
        raise AssertionError("the backend was called")
    monkeypatch.setattr(backend, "get_context", no_backend)
    monkeypatch.setattr(backend, "get_batch_contexts", no_backend)


@pytest.mark.parametrize("k", [1, 0, -3, 129, 2.5, 20.0, "many", True, [20]])
def test_bad_neighbors_are_refused_before_any_backend_call(k, monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import PointCloud, PointCloudException, SimpleICP, SimpleICPException
    _no_backend(monkeypatch)
    X = np.random.default_rng(0).standard_normal((50, 3))
    icp = SimpleICP(verbose=False)
    icp.add_point_clouds(PointCloud(X, columns=["x", "y", "z"]), PointCloud(X, columns=["x", "y", "z"]))
    icp.outlier_neighbors = k
    with pytest.raises(SimpleICPException, match="outlier_neighbors"):
        icp.run()
    with pytest.raises(SimpleICPException, match="outlier_neighbors"):
        simpleicp_amd.run_batch([(X, X)], outlier_neighbors=k)
    with pytest.raises(SimpleICPException, match="outlier_neighbors"):
        simpleicp_amd.run_batch([(X, X)], per_pair=[{"outlier_neighbors": k}])
    with pytest.raises(SimpleICPException, match="outlier_neighbors"):
        simpleicp_amd.run_tensors(X, X, outlier_neighbors=k)
    with pytest.raises(ValueError, match="neighbors"):
        simpleicp_amd.outlier_keep(X, neighbors=k)
    with pytest.raises((PointCloudException, TypeError), match="neighbors|int"):
        PointCloud(X, columns=["x", "y", "z"]).select_statistical_inliers(k)


@pytest.mark.parametrize("ratio", [float("nan"), float("inf"), -float("inf"), "two", None, [2.0]])
def test_bad_std_ratio_is_refused_before_any_backend_call(ratio, monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import PointCloud, PointCloudException, SimpleICP, SimpleICPException
    _no_backend(monkeypatch)
    X = np.random.default_rng(0).standard_normal((50, 3))
    icp = SimpleICP(verbose=False)
    icp.add_point_clouds(PointCloud(X, columns=["x", "y", "z"]), PointCloud(X, columns=["x", "y", "z"]))
    icp.outlier_neighbors, icp.outlier_std_ratio = 20, ratio
    with pytest.raises(SimpleICPException, match="outlier_std_ratio"):
        icp.run()
    with pytest.raises(SimpleICPException, match="outlier_std_ratio"):
        simpleicp_amd.run_batch([(X, X)], outlier_neighbors=20, outlier_std_ratio=ratio)
    with pytest.raises(SimpleICPException, match="outlier_std_ratio"):
        simpleicp_amd.run_tensors(X, X, outlier_neighbors=20, outlier_std_ratio=ratio)
    with pytest.raises(ValueError, match="std_ratio"):
        simpleicp_amd.outlier_keep(X, neighbors=20, std_ratio=ratio)
    with pytest.raises(PointCloudException, match="std_ratio"):
        PointCloud(X, columns=["x", "y", "z"]).select_statistical_inliers(20, ratio)


def test_outlier_keep_and_radius_arguments(monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import PointCloud, PointCloudException
    _no_backend(monkeypatch)
    X = np.random.default_rng(0).standard_normal((50, 3))
    assert list(inspect.signature(simpleicp_amd.outlier_keep).parameters) == ["X", "neighbors", "std_ratio", "radius", "min_points", "mask"]
    assert all(p.kind is p.KEYWORD_ONLY for n, p in inspect.signature(simpleicp_amd.outlier_keep).parameters.items() if n != "X")
    assert "outlier_keep" in simpleicp_amd.__all__
    with pytest.raises(ValueError, match="exactly one"):
        simpleicp_amd.outlier_keep(X)
    with pytest.raises(ValueError, match="exactly one"):
        simpleicp_amd.outlier_keep(X, neighbors=20, radius=0.5, min_points=3)
    with pytest.raises(ValueError, match="min_points"):
        simpleicp_amd.outlier_keep(X, neighbors=20, min_points=3)
    for r in (0.0, -1.0, float("nan"), float("inf"), "wide"):
        with pytest.raises(ValueError, match="radius"):
            simpleicp_amd.outlier_keep(X, radius=r, min_points=3)
        with pytest.raises(PointCloudException, match="radius"):
            PointCloud(X, columns=["x", "y", "z"]).select_radius_inliers(r, 3)
    for mp in (-1, 2.5, None, "few"):
        with pytest.raises(ValueError, match="min_points"):
            simpleicp_amd.outlier_keep(X, radius=0.5, min_points=mp)
    for mp in (-1, 2.5, "few"):
        with pytest.raises(PointCloudException, match="min_points"):
            PointCloud(X, columns=["x", "y", "z"]).select_radius_inliers(0.5, mp)
    with pytest.raises(TypeError, match="torch.Tensor"):           # accepted: refused for the cloud, not for the keywords
        simpleicp_amd.outlier_keep(X, neighbors=20)
    with pytest.raises(TypeError, match="torch.Tensor"):
        simpleicp_amd.outlier_keep(X, radius=0.5, min_points=0)


def test_keywords_accepted_and_misspelt_ones_refused(monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import SimpleICP, backend, batch

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached
    monkeypatch.setattr(backend, "get_batch_contexts", stop)
    X = np.random.default_rng(0).standard_normal((50, 3))
    names = {"outlier_neighbors", "outlier_std_ratio"}
    for fn in (simpleicp_amd.run_batch, simpleicp_amd.run_tensors):
        assert names <= set(inspect.signature(fn).parameters)
    assert names <= set(batch._EXTRA_DEFAULTS) and not names & set(batch._RUN_DEFAULTS)
    assert SimpleICP.outlier_neighbors is None and SimpleICP(verbose=False).outlier_neighbors is None and SimpleICP.outlier_std_ratio == 2.0
    assert not names & set(inspect.signature(SimpleICP.run).parameters)            # run()'s signature is the reference's
    with pytest.raises(Reached):
        simpleicp_amd.run_batch([(X, X)], outlier_neighbors=20, outlier_std_ratio=-0.5)
    with pytest.raises(Reached):
        simpleicp_amd.run_batch([(X, X)], per_pair=[{"outlier_neighbors": 8, "outlier_std_ratio": 1}])
    with pytest.raises(TypeError, match="outlier_neighbours"):
        simpleicp_amd.run_batch([(X, X)], outlier_neighbours=20)
    with pytest.raises(TypeError, match="outlier_neighbours"):
        simpleicp_amd.run_tensors(X, X, outlier_neighbours=20)
    with pytest.raises(TypeError, match="torch.Tensor"):
        simpleicp_amd.run_tensors(X, X, outlier_neighbors=20)


def test_more_neighbors_than_fixed_points_is_refused_before_any_backend_call(monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import PointCloud, SimpleICP, SimpleICPException, backend
    from simpleicp_amd.icp import _check_outlier_size
    _no_backend(monkeypatch)
    X = np.random.default_rng(0).standard_normal((15, 3))
    icp = SimpleICP(verbose=False)
    icp.add_point_clouds(PointCloud(X, columns=["x", "y", "z"]), PointCloud(X, columns=["x", "y", "z"]))
    icp.outlier_neighbors = 16
    with pytest.raises(SimpleICPException, match=r"outlier_neighbors \(16\) exceeds the number of points of the fixed point cloud \(15\)"):
        icp.run()
    _check_outlier_size((15, 2.0), 15)
    _check_outlier_size(None, 1)
    # run_batch reports it as the pair's error, like everything run() would raise for that pair
    class Untouched:                                               # a pool context nothing may call
        def __getattr__(self, name):
            raise AssertionError("the backend was called")
    monkeypatch.setattr(backend, "get_batch_contexts", lambda n: [Untouched() for _ in range(n)])
    out = simpleicp_amd.run_batch([(X, X)], outlier_neighbors=16)
    assert isinstance(out[0].error, SimpleICPException) and "exceeds the number of points" in str(out[0].error)


def test_cli_options():
    from simpleicp_amd import cli
    ap = cli.build_parser()
    a = ap.parse_args(["-f", "a", "-m", "b"])
    assert a.outlier_neighbors is None and a.outlier_std_ratio == 2.0
    a = ap.parse_args(["-f", "a", "-m", "b", "--outlier-neighbors", "20", "--outlier-std-ratio", "1.5"])
    assert a.outlier_neighbors == 20 and a.outlier_std_ratio == 1.5


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


def _bunny(clouds, n=5000, strays=40):
    """the bunny's first points with a few strays planted among the fixed cloud's rows"""
    from simpleicp_amd import PointCloud
    X1, X2 = clouds("bunny_part1")[:n].copy(), clouds("bunny_part2")[:n].copy()
    rng = np.random.default_rng(11)
    at = rng.choice(n, strays, replace=False)
    X1[at] += rng.uniform(2.0, 3.0, (strays, 3)) * rng.choice([-1.0, 1.0], (strays, 3))
    return PointCloud(X1, columns=["x", "y", "z"]), PointCloud(X2, columns=["x", "y", "z"]), at


@pytest.mark.parametrize("overlap,voxel", [(np.inf, None), (3.0, None), (3.0, 0.02)])
def test_run_filters_between_the_overlap_pass_and_the_voxel_step(octx, clouds, overlap, voxel):
    import voxel_ref
    from simpleicp_amd import SimpleICP, _lib
    pc_fix, pc_mov, strays = _bunny(clouds)
    X1, X2 = pc_fix.X, pc_mov.X
    k, ratio, Q = 12, 1.5, 300
    icp = SimpleICP(verbose=False)
    icp.add_point_clouds(pc_fix, pc_mov)
    icp.outlier_neighbors, icp.outlier_std_ratio, icp.voxel_size = k, ratio, voxel
    (H, X, rbp, res), records = _run_logged(icp, correspondences=Q, max_iterations=3, max_overlap_distance=overlap)
    rows = np.arange(len(X1))
    if np.isfinite(overlap):
        side = oracle_backend.OracleContext()
        side.upload(_lib.FIX, X1)
        side.upload(_lib.MOV, X2)
        rows = rows[side.select_in_range(_lib.FIX, _lib.MOV, None, np.eye(4), overlap)]
        assert 0 < len(rows) < len(X1)
    ref = outlier_ref.statistical(X1, k, ratio, rows=None if len(rows) == len(X1) else rows)
    inl = rows[ref["keep"]]
    assert 0 < len(inl) < len(rows) and np.isin(strays, inl).mean() < 0.2      # (a displaced point may land next to another part of the model)
    if voxel is not None:
        inl = voxel_ref.kept_rows(X1, voxel, rows=inl)
    assert Q < len(inl)
    want = np.unique(inl[np.round(np.linspace(0, len(inl) - 1, Q)).astype(int)])
    assert np.array_equal(pc_fix.idx_selected, want) and np.array_equal(octx._sel, want)
    assert octx.outlier_args[:2] == (k, ratio)
    assert (octx.outlier_args[2] is None) == (len(rows) == len(X1))
    # the step's place among the calls and among the log lines; its statistics
    calls = [n for n in octx.calls if n in ("select_in_range", "outlier_statistical", "voxel_select", "estimate_normals", "icp_setup")]
    assert calls == ((["select_in_range"] if np.isfinite(overlap) else []) + ["outlier_statistical"]
                     + (["voxel_select"] if voxel is not None else []) + ["estimate_normals", "icp_setup"])
    lines = [m for m in records if m.startswith("Remove statistical outliers ...")]
    assert len(lines) == 1 and f"kept {ref['n_kept']} of {ref['n_candidates']} points" in lines[0]
    at = records.index(lines[0])
    assert records[at + 1] == ("Keep one point per voxel ..." if voxel is not None else "Select points for correspondences in fixed point cloud ...")
    if np.isfinite(overlap):
        assert records[at - 1] == "Consider partial overlap of point clouds ..."
    st = icp.last_run_info["outlier"]
    assert st == {key: ref[key] for key in ("n_candidates", "n_kept", "mean", "std", "threshold")}


def test_off_is_untouched(octx, clouds):
    from simpleicp_amd import SimpleICP
    pc_fix, pc_mov, _ = _bunny(clouds, 3000)
    icp = SimpleICP(verbose=False)
    icp.add_point_clouds(pc_fix, pc_mov)
    assert icp.outlier_neighbors is None
    (H, X, rbp, res), records = _run_logged(icp, correspondences=200, max_iterations=2)
    assert "outlier_statistical" not in octx.calls and not any("outlier" in m.lower() for m in records)
    assert "outlier" not in icp.last_run_info and np.isfinite(H).all()
    plain = oracle_backend.OracleContext()
    from simpleicp_amd import backend
    import simpleicp_amd
    pc_a, pc_b, _ = _bunny(clouds, 3000)
    icp2 = SimpleICP(verbose=False)
    icp2.add_point_clouds(pc_a, pc_b)
    old = backend.get_context
    backend.get_context = lambda: plain
    try:
        H2 = icp2.run(correspondences=200, max_iterations=2)[0]
    finally:
        backend.get_context = old
    assert np.array_equal(H, H2) and simpleicp_amd is not None


def test_backend_without_the_entry_point(monkeypatch, clouds):
    """the plain stand-in has no outlier_statistical: asked for, BackendError; not asked for, never touched"""
    from simpleicp_amd import SimpleICP, _lib
    ctx = oracle_backend.install(monkeypatch)
    assert not hasattr(ctx, "outlier_statistical")
    pc_fix, pc_mov, _ = _bunny(clouds, 3000)
    icp = SimpleICP(verbose=False)
    icp.add_point_clouds(pc_fix, pc_mov)
    icp.outlier_neighbors = 10
    with pytest.raises(_lib.BackendError, match="outlier"):
        icp.run(correspondences=200, max_iterations=2)
    icp.outlier_neighbors = None
    H, _, _, _ = icp.run(correspondences=200, max_iterations=2)
    assert np.isfinite(H).all()


def test_select_inliers_compose_with_the_other_selections(octx, clouds):
    from simpleicp_amd import PointCloud
    pc, _, strays = _bunny(clouds)
    X = pc.X
    pc.select_by_indices(np.arange(500, 4500))
    pc.select_statistical_inliers(12, 1.5)
    ref = outlier_ref.statistical(X, 12, 1.5, rows=np.arange(500, 4500))
    want = np.arange(500, 4500)[ref["keep"]]
    assert np.array_equal(pc.idx_selected, want) and 0 < len(want) < 4000
    assert pc.last_outlier_stats == {key: ref[key] for key in ("n_candidates", "n_kept", "mean", "std", "threshold")}
    pc.select_n_points(50)
    assert np.array_equal(pc.idx_selected, np.unique(want[np.round(np.linspace(0, len(want) - 1, 50)).astype(int)]))
    pc.unselect_all_points()
    pc.select_statistical_inliers(12, 1.5)                      # nothing selected: nothing to do
    assert pc.num_selected_points == 0


def test_run_batch_members_take_the_step_call_wide_and_per_pair(monkeypatch, clouds):
    import simpleicp_amd
    from simpleicp_amd import backend
    backend.reset_batch_contexts()
    made = []

    def factory(device):
        made.append(OutlierBatchContext())
        return made[-1]
    monkeypatch.setattr(backend, "batch_context_factory", factory)
    try:
        pc_fix, pc_mov, strays = _bunny(clouds, 3000)
        X1, X2 = pc_fix.X, pc_mov.X
        out = simpleicp_amd.run_batch([(X1, X2), (X1, X2), (X1, X2)], per_pair=[None, {"outlier_neighbors": None}, {"outlier_std_ratio": 0.5}],
                                      outlier_neighbors=12, correspondences=200, max_iterations=2)
        assert [o.error for o in out] == [None, None, None] and [o.path for o in out] == ["batched"] * 3
        ref = [outlier_ref.statistical(X1, 12, ratio) for ratio in (2.0, 0.5)]
        keys = ("n_candidates", "n_kept", "mean", "std", "threshold")
        assert out[0].outlier == {key: ref[0][key] for key in keys} and out[1].outlier is None
        assert out[2].outlier == {key: ref[1][key] for key in keys} and ref[1]["n_kept"] < ref[0]["n_kept"]
        assert ["outlier_statistical" in c.calls for c in made[:3]] == [True, False, True]
        for c, r in ((made[0], ref[0]), (made[2], ref[1])):
            inl = np.flatnonzero(r["keep"])
            assert np.array_equal(c._sel, np.unique(inl[np.round(np.linspace(0, len(inl) - 1, 200)).astype(int)]))
        assert not np.array_equal(out[0].H, out[1].H)
    finally:
        backend.reset_batch_contexts()


def test_a_distributed_job_is_refused_before_any_backend_call(monkeypatch):
    import simpleicp_amd
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
    icp.outlier_neighbors = 20
    with pytest.raises(SimpleICPException, match="does not run in a torch.distributed job"):
        icp.run()
    with pytest.raises(SimpleICPException, match="does not run in a torch.distributed job"):
        simpleicp_amd.outlier_keep(X, neighbors=20)
    with pytest.raises(SimpleICPException, match="does not run in a torch.distributed job"):
        simpleicp_amd.run_tensors(X, X, outlier_neighbors=20)
