"""Voxel selection (contract (V)), the parts that need no GPU: the reference's own properties
(tests/voxel_ref.py), the companion header and the binding, the refusals that come before any device work, and run()'s host plumbing
on the stand-in backend of tests/oracle_backend.py."""
import inspect
import logging
import re
import subprocess
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

import oracle_backend
import voxel_ref
from conftest import load_golden

ROOT = Path(__file__).resolve().parent.parent


class VoxelOracleContext(oracle_backend.OracleContext):
    """The stand-in with the one new entry point, answered by the numpy reference."""

    def voxel_select(self, slot, voxel_size, origin=None, rows=None, keep_ptr=None):
        assert keep_ptr is None
        self._log("voxel_select")
        self.voxel_args = (float(voxel_size), tuple(origin) if origin is not None else (0.0, 0.0, 0.0), None if rows is None else np.array(rows))
        return voxel_ref.keep(self.cloud[slot][0], voxel_size, self.voxel_args[1], rows=rows)


@pytest.fixture
def vctx(monkeypatch):
    from simpleicp_amd import backend
    ctx = VoxelOracleContext()
    monkeypatch.setattr(backend, "get_context", lambda: ctx)
    return ctx


# ---- the reference ----
def test_reference_properties():
    rng = np.random.default_rng(5)
    X = rng.uniform(-3, 3, (5000, 3))
    X[100:110] = X[7]                                              # exact duplicates
    X[200] = [0.5, -0.0, 1.0]                                      # on lattice planes, a negative zero
    c = 0.5
    k = voxel_ref.keep(X, c)
    V = voxel_ref.voxels(X, c)
    # exactly one kept point per occupied voxel, and it is the first of its voxel
    uniq, first, inv = np.unique(V + 0.0, axis=0, return_index=True, return_inverse=True)
    assert k.sum() == len(uniq) and np.array_equal(np.flatnonzero(k), np.sort(first))
    assert k[7] and not k[100:110].any()
    # the packed comparison is the axis=0 comparison
    assert np.array_equal(np.sort(voxel_ref._first_of_each(V)), np.sort(first))
    far = X.copy()
    far[0, 0] = 1e9                                                # wider than 2^21 cells: the axis=0 road
    assert voxel_ref.keep(far, c).sum() == len(np.unique(voxel_ref.voxels(far, c) + 0.0, axis=0))
    # rows in any order: the verdict belongs to the entry, the winner is the lowest point index
    rows = rng.permutation(len(X))[:3000]
    kr = voxel_ref.keep(X, c, rows=rows)
    assert np.array_equal(np.sort(rows[kr]), np.sort(rows)[voxel_ref.keep(X[np.sort(rows)], c)])
    assert np.array_equal(voxel_ref.kept_rows(X, c, rows=rows), np.sort(rows[kr]))
    # a mask: the same candidates, verdicts per point
    mask = np.zeros(len(X), np.uint8)
    mask[rows] = 1
    assert np.array_equal(np.flatnonzero(voxel_ref.keep(X, c, mask=mask)), np.sort(rows[kr]))
    assert not voxel_ref.keep(X, c, mask=np.zeros(len(X), np.uint8)).any()
    # an origin moves the lattice; a cell larger than the cloud keeps point 0 alone
    assert not np.array_equal(voxel_ref.keep(X, c, (0.25, 0.1, 0.0)), k)
    big = voxel_ref.keep(X, 100.0, (-50.0, -50.0, -50.0))
    assert big.sum() == 1 and big[0]


# ---- header, exports, binding ----
def _header_functions():
    text = (ROOT / "include" / "simpleicp_hip_voxel.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sicp_\w+)\s*\(", text)))


def test_header_names_are_exported_and_bound():
    from simpleicp_amd import _lib, build
    assert _header_functions() == sorted(_lib.VOXEL_EXPORTS)
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", str(so)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sicp_\w+)", out))
    assert set(_lib.VOXEL_EXPORTS) <= exported
    others = set(_lib.EXPORTS) | set(_lib.BATCH_EXPORTS) | set(_lib.DEVICE_EXPORTS) | set(_lib.NORMALS_EXPORTS)
    assert not set(_lib.VOXEL_EXPORTS) & others
    L = _lib.load()
    for name in _lib.VOXEL_EXPORTS:
        assert hasattr(L, name)
    assert L.sicp_voxel_version() == _lib.VOXEL_VERSION == 1 and _lib.voxel_version() == 1
    assert "#define SICP_VOXEL_VERSION 1" in (ROOT / "include" / "simpleicp_hip_voxel.h").read_text()
    # the main header and its version are untouched, the other companions keep theirs
    assert L.sicp_abi_version() == _lib.ABI_VERSION == 7
    assert "voxel" not in (ROOT / "include" / "simpleicp_hip.h").read_text()
    assert (_lib.BATCH_VERSION, _lib.DEVICE_VERSION, _lib.NORMALS_VERSION) == (1, 1, 1)
    for name in ("voxel_select", "voxel_select_masked"):
        assert callable(getattr(_lib.Context, name))


def test_null_arguments_are_refused_not_dereferenced():
    """the NULL-argument probe of the other entries: no ctx, so nothing may be touched"""
    import ctypes as C
    from simpleicp_amd import _lib
    L = _lib.load()
    kept = C.c_int64()
    buf = np.zeros(4, np.uint8)
    assert L.sicp_voxel_select(None, 0, None, 0, 1.0, None, _lib._ptr(buf), C.byref(kept)) == _lib.ERR_INVALID
    assert L.sicp_voxel_select_masked(None, 0, _lib._ptr(buf), 4, 1.0, None, _lib._ptr(buf), C.byref(kept)) == _lib.ERR_INVALID
    assert b"null ctx" in L.sicp_last_error()


# ---- refusals before any device work ----
BAD_SIZES = [0.0, -1.0, float("nan"), float("inf"), "wide", {}, [1.0, 2.0]]


@pytest.mark.parametrize("size", BAD_SIZES)
def test_bad_voxel_size_is_refused_before_any_backend_call(size, monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import PointCloud, PointCloudException, SimpleICP, SimpleICPException, backend

    def no_backend(*a, **k):
        raise AssertionError("the backend was called")
    monkeypatch.setattr(backend, "get_context", no_backend)
    monkeypatch.setattr(backend, "get_batch_contexts", no_backend)
    X = np.random.default_rng(0).standard_normal((50, 3))
    icp = SimpleICP(verbose=False)
    icp.add_point_clouds(PointCloud(X, columns=["x", "y", "z"]), PointCloud(X, columns=["x", "y", "z"]))
    icp.voxel_size = size
    with pytest.raises(SimpleICPException, match="voxel_size"):
        icp.run()
    with pytest.raises(SimpleICPException, match="voxel_size"):
        simpleicp_amd.run_batch([(X, X)], voxel_size=size)
    with pytest.raises(SimpleICPException, match="voxel_size"):
        simpleicp_amd.run_batch([(X, X)], per_pair=[{"voxel_size": size}])
    with pytest.raises(SimpleICPException, match="voxel_size"):
        simpleicp_amd.run_tensors(X, X, voxel_size=size)
    with pytest.raises(SimpleICPException, match="voxel_size"):
        simpleicp_amd.voxel_keep(X, size)
    with pytest.raises(PointCloudException, match="voxel_size"):
        PointCloud(X, columns=["x", "y", "z"]).select_voxels(size)


@pytest.mark.parametrize("origin", [(0.0, float("nan"), 0.0), (float("inf"), 0.0, 0.0), (0.0, 0.0), "abc", 5.0])
def test_bad_origin_is_refused_before_any_backend_call(origin, monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import PointCloud, PointCloudException, SimpleICP, SimpleICPException, backend

    def no_backend(*a, **k):
        raise AssertionError("the backend was called")
    monkeypatch.setattr(backend, "get_context", no_backend)
    monkeypatch.setattr(backend, "get_batch_contexts", no_backend)
    X = np.random.default_rng(0).standard_normal((50, 3))
    icp = SimpleICP(verbose=False)
    icp.add_point_clouds(PointCloud(X, columns=["x", "y", "z"]), PointCloud(X, columns=["x", "y", "z"]))
    icp.voxel_size, icp.voxel_origin = 0.5, origin
    with pytest.raises(SimpleICPException, match="voxel_origin"):
        icp.run()
    with pytest.raises(SimpleICPException, match="voxel_origin"):
        simpleicp_amd.run_batch([(X, X)], voxel_size=0.5, voxel_origin=origin)
    with pytest.raises(SimpleICPException, match="voxel_origin"):
        simpleicp_amd.run_tensors(X, X, voxel_size=0.5, voxel_origin=origin)
    with pytest.raises(SimpleICPException, match="voxel_origin"):
        simpleicp_amd.voxel_keep(X, 0.5, origin)
    with pytest.raises(PointCloudException, match="voxel_origin"):
        PointCloud(X, columns=["x", "y", "z"]).select_voxels(0.5, origin)


def test_keywords_accepted_and_misspelt_ones_refused(monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import SimpleICP, backend, batch

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached
    monkeypatch.setattr(backend, "get_batch_contexts", stop)
    X = np.random.default_rng(0).standard_normal((50, 3))
    for fn in (simpleicp_amd.run_batch, simpleicp_amd.run_tensors):
        assert {"voxel_size", "voxel_origin"} <= set(inspect.signature(fn).parameters)
    assert {"voxel_size", "voxel_origin"} <= set(batch._EXTRA_DEFAULTS) and not {"voxel_size", "voxel_origin"} & set(batch._RUN_DEFAULTS)
    assert list(inspect.signature(simpleicp_amd.voxel_keep).parameters) == ["X", "voxel_size", "origin", "mask"]
    assert SimpleICP.voxel_size is None and SimpleICP(verbose=False).voxel_size is None
    assert tuple(SimpleICP.voxel_origin) == (0.0, 0.0, 0.0)
    assert "voxel_size" not in inspect.signature(SimpleICP.run).parameters          # run()'s signature is the reference's
    with pytest.raises(Reached):                                   # accepted: the call gets as far as the device
        simpleicp_amd.run_batch([(X, X)], voxel_size=0.5, voxel_origin=(0.1, 0.2, 0.3))
    with pytest.raises(Reached):
        simpleicp_amd.run_batch([(X, X)], per_pair=[{"voxel_size": 2, "voxel_origin": (1, 1, 1)}])
    with pytest.raises(TypeError, match="voxel_sise"):
        simpleicp_amd.run_batch([(X, X)], voxel_sise=0.5)
    with pytest.raises(TypeError, match="voxel_sise"):
        simpleicp_amd.run_batch([(X, X)], per_pair=[{"voxel_sise": 0.5}])
    with pytest.raises(TypeError, match="voxel_sise"):
        simpleicp_amd.run_tensors(X, X, voxel_sise=0.5)
    with pytest.raises(TypeError, match="torch.Tensor"):           # accepted: refused for the clouds, not for the keyword
        simpleicp_amd.run_tensors(X, X, voxel_size=0.5)
    with pytest.raises(TypeError, match="torch.Tensor"):
        simpleicp_amd.voxel_keep(X, 0.5)


def test_cli_option():
    from simpleicp_amd import cli
    ap = cli.build_parser()
    assert ap.parse_args(["-f", "a", "-m", "b"]).voxel_size is None
    assert ap.parse_args(["-f", "a", "-m", "b", "--voxel-size", "0.25"]).voxel_size == 0.25


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


def _bunny(clouds, n=6000):
    from simpleicp_amd import PointCloud
    X1, X2 = clouds("bunny_part1")[:n], clouds("bunny_part2")[:n]
    return PointCloud(X1, columns=["x", "y", "z"]), PointCloud(X2.copy(), columns=["x", "y", "z"])


@pytest.mark.parametrize("overlap", [np.inf, 3.0])
def test_run_thins_between_the_overlap_pass_and_select_n_points(vctx, clouds, overlap):
    from simpleicp_amd import SimpleICP, _lib
    pc_fix, pc_mov = _bunny(clouds)
    X1, X2 = pc_fix.X, pc_mov.X
    c, o, Q = 0.25, (0.1, -0.2, 0.05), 300
    icp = SimpleICP(verbose=False)
    icp.add_point_clouds(pc_fix, pc_mov)
    icp.voxel_size, icp.voxel_origin = c, o
    (H, X, rbp, res), records = _run_logged(icp, correspondences=Q, max_iterations=3, max_overlap_distance=overlap)
    # what the selection must be: select_n_points applied to the voxel-thinned in-range rows
    rows = np.arange(len(X1))
    if np.isfinite(overlap):
        side = oracle_backend.OracleContext()
        side.upload(_lib.FIX, X1)
        side.upload(_lib.MOV, X2)
        rows = rows[side.select_in_range(_lib.FIX, _lib.MOV, None, np.eye(4), overlap)]
        assert 0 < len(rows) < len(X1)
    thin = voxel_ref.kept_rows(X1, c, o, rows=rows)
    assert Q < len(thin) < len(rows)
    want = np.unique(thin[np.round(np.linspace(0, len(thin) - 1, Q)).astype(int)])
    assert np.array_equal(pc_fix.idx_selected, want)
    assert np.array_equal(vctx._sel, want)
    assert vctx.voxel_args[0] == c and vctx.voxel_args[1] == o
    # the step's place among the calls and among the log lines
    calls = [n for n in vctx.calls if n in ("select_in_range", "voxel_select", "estimate_normals", "icp_setup")]
    assert calls == (["select_in_range"] if np.isfinite(overlap) else []) + ["voxel_select", "estimate_normals", "icp_setup"]
    assert records.count("Keep one point per voxel ...") == 1
    at = records.index("Keep one point per voxel ...")
    assert records[at + 1] == "Select points for correspondences in fixed point cloud ..."
    if np.isfinite(overlap):
        assert records[at - 1] == "Consider partial overlap of point clouds ..."


def test_off_is_todays_run(vctx, clouds):
    """voxel_size = None: the recorded result of the fixture, its log lines, and the new entry point is never touched"""
    from simpleicp_amd import PointCloud, SimpleICP
    g, files, kw = load_golden("bunny")
    pc_fix = PointCloud(clouds(files[0]), columns=["x", "y", "z"])
    pc_mov = PointCloud(clouds(files[1]).copy(), columns=["x", "y", "z"])
    sel = g["sel_idx"]
    for j, c in enumerate(("nx", "ny", "nz", "planarity")):
        v = np.full(len(pc_fix), np.nan, np.float32)
        v[sel] = g["planarity"] if c == "planarity" else g["normals"][:, j]
        pc_fix[c] = pd.arrays.SparseArray(v)
    icp = SimpleICP(verbose=False)
    icp.add_point_clouds(pc_fix, pc_mov)
    assert icp.voxel_size is None
    (H, X, rbp, res), records = _run_logged(icp, **kw)
    assert np.abs(H - g["H"]).max() < 1e-7
    assert icp.last_run_info["iterations"] == int(g["iterations"])
    assert np.array_equal(pc_fix.idx_selected, sel)
    assert "voxel_select" not in vctx.calls and not any("voxel" in m for m in records)
    theirs = [m for m in str(g["log"]).splitlines() if not m.startswith(("Finished in", "Estimate normals"))]
    mine = [m for m in records if not m.startswith("Finished in")]
    assert [m for m in mine if "|" not in m and "[" not in m] == [m for m in theirs if "|" not in m and "[" not in m]


def test_backend_without_the_entry_point(monkeypatch, clouds):
    """the plain stand-in has no voxel_select: asked for, BackendError; not asked for, never touched"""
    from simpleicp_amd import SimpleICP, _lib
    ctx = oracle_backend.install(monkeypatch)
    assert not hasattr(ctx, "voxel_select")
    pc_fix, pc_mov = _bunny(clouds, 3000)
    icp = SimpleICP(verbose=False)
    icp.add_point_clouds(pc_fix, pc_mov)
    icp.voxel_size = 0.25
    with pytest.raises(_lib.BackendError, match="voxel"):
        icp.run(correspondences=200, max_iterations=2)
    icp.voxel_size = None
    H, _, _, _ = icp.run(correspondences=200, max_iterations=2)
    assert np.isfinite(H).all()


def test_select_voxels_composes_with_the_other_selections(vctx, clouds):
    from simpleicp_amd import PointCloud
    X = clouds("bunny_part1")[:5000]
    pc = PointCloud(X, columns=["x", "y", "z"])
    pc.select_by_indices(np.arange(500, 4500))
    pc.select_voxels(0.3, origin=(0.0, 0.1, 0.0))
    want = voxel_ref.kept_rows(X, 0.3, (0.0, 0.1, 0.0), rows=np.arange(500, 4500))
    assert np.array_equal(pc.idx_selected, want) and 0 < len(want) < 4000
    pc.select_n_points(50)
    assert np.array_equal(pc.idx_selected, np.unique(want[np.round(np.linspace(0, len(want) - 1, 50)).astype(int)]))
    pc.select_voxels(100.0, origin=(-50.0, -50.0, -50.0))                 # one voxel holds the whole cloud: its lowest selected index stays
    assert list(pc.idx_selected) == [pc.idx_selected.min()] and len(pc.idx_selected) == 1
    pc.unselect_all_points()
    pc.select_voxels(0.3)                                       # nothing selected: nothing to do, no backend call needed
    assert pc.num_selected_points == 0


def test_a_distributed_job_is_refused_before_any_backend_call(monkeypatch):
    """run() with voxel_size and voxel_keep in a torch.distributed job: SimpleICPException, worded like run_tensors' refusal"""
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
    icp.voxel_size = 0.5
    with pytest.raises(SimpleICPException, match="does not run in a torch.distributed job"):
        icp.run()
    with pytest.raises(SimpleICPException, match="does not run in a torch.distributed job"):
        simpleicp_amd.voxel_keep(X, 0.5)
    with pytest.raises(SimpleICPException, match="does not run in a torch.distributed job"):
        simpleicp_amd.run_tensors(X, X, voxel_size=0.5)
