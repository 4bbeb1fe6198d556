"""run_batch and the batch ABI without a GPU: exported symbols, the NULL probe, run_batch's host logic on stand-in contexts
(tests/helpers/batch_oracle.py), and the upload_start fix.  (The GPU side: tests/test_gpu_batch.py.)"""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import simpleicp_amd
from simpleicp_amd import PointCloud, SimpleICP, SimpleICPException, _lib, backend, run_batch
from tests.helpers import batch_oracle

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture
def stand_in(monkeypatch):
    """Stand-in contexts for run_batch's pool and SimpleICP.run; the pool is emptied again when the test ends."""
    ctx = batch_oracle.install(monkeypatch)
    yield ctx
    backend.reset_batch_contexts()


def surface_pair(n, seed, shift=(0.3, -0.2, 0.1), yaw=0.02):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-15, 15, (n, 2))
    z = 2 * np.sin(xy[:, 0] / 4) * np.cos(xy[:, 1] / 6) + rng.normal(0, 0.005, n)
    Xf = np.column_stack((xy, z))
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    Xm = (Xf + rng.normal(0, 0.005, Xf.shape)) @ R.T + np.array(shift)
    return Xf, Xm


def batch_header_functions():
    txt = (ROOT / "include" / "simpleicp_hip_batch.h").read_text()
    return sorted(set(re.findall(r"^int\s+(sicp_\w+)\s*\(", txt, flags=re.M)))


def test_batch_header_symbols_exported_and_versioned():
    assert batch_header_functions() == sorted(_lib.BATCH_EXPORTS)
    L = _lib.load()
    for name in _lib.BATCH_EXPORTS:
        assert hasattr(L, name), name
    assert L.sicp_batch_version() == _lib.BATCH_VERSION == 1
    assert _lib.batch_version() == 1
    assert not set(_lib.BATCH_EXPORTS) & set(_lib.EXPORTS)          # the main ABI's list stays as it is


def test_batch_null_probe_in_child():
    code = (
        "import ctypes as C\n"
        "from simpleicp_amd import _lib\n"
        "L = _lib.load()\n"
        "fb = C.c_int64(7)\n"
        "print(L.sicp_icp_run_batch(None, 0, C.byref(fb)), fb.value, L.sicp_last_error().decode())\n"
        "arr = (_lib.BatchMember * 2)()\n"
        "print(L.sicp_icp_run_batch(arr, 2, None), L.sicp_last_error().decode())\n"
        "print(L.sicp_ctx_lean(None), L.sicp_last_error().decode())\n"
    )
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[0].startswith(f"{_lib.ERR_INVALID} 0 ") and "empty batch" in lines[0]
    assert lines[1].startswith(f"{_lib.ERR_INVALID} ") and "null ctx" in lines[1]
    assert lines[2].startswith(f"{_lib.ERR_INVALID} ") and "null ctx" in lines[2]


def test_missing_batch_symbols_raise_backend_error(monkeypatch):
    class NoBatch:
        pass
    monkeypatch.setattr(_lib, "load", lambda: NoBatch())
    with pytest.raises(_lib.BackendError, match="no batch entry points"):
        _lib.batch_version()


def test_run_batch_is_exported():
    assert simpleicp_amd.run_batch is run_batch
    assert "run_batch" in simpleicp_amd.__all__


def lone_run(Xf, Xm, **kw):
    pc1, pc2 = PointCloud(Xf, columns=["x", "y", "z"]), PointCloud(Xm, columns=["x", "y", "z"])
    icp = SimpleICP(verbose=False)
    icp.add_point_clouds(pc1, pc2)
    return icp.run(**kw)


def assert_same(res, ref):
    H, X, rbp, resid = ref
    assert res.error is None
    assert np.array_equal(res.H, H)
    assert np.array_equal(res.X_mov_transformed, X)
    assert np.array_equal(res.residuals, resid)
    for name in ("alpha1", "alpha2", "alpha3", "tx", "ty", "tz"):
        a, b = getattr(res.rbp, name), getattr(rbp, name)
        assert a.estimated_value == b.estimated_value
        assert a.initial_value == b.initial_value
        assert np.array_equal(a.estimated_uncertainty, b.estimated_uncertainty, equal_nan=True)
    h, x, r, d = res                                            # unpacks like run()'s 4-tuple
    assert h is res.H and d is res.residuals


def test_run_batch_equals_run_on_fresh_copies_with_per_pair(stand_in):
    pairs = [surface_pair(3000, s, shift=(0.2 * s, -0.1, 0.05)) for s in range(3)]
    per = [None, {"rbp_observed_values": (0, 0, 1.0, 0, 0, 0), "rbp_observation_weights": (0, 0, 0, 0, 0, 0)},
           {"max_iterations": 2, "correspondences": 400}]
    out = run_batch(pairs, per_pair=per, correspondences=800, neighbors=8)
    assert len(out) == 3
    for (Xf, Xm), p, res in zip(pairs, per, out):
        kw = {"correspondences": 800, "neighbors": 8, **(p or {})}
        assert_same(res, lone_run(Xf, Xm, **kw))
    assert out[2].iterations == 2                                  # per_pair's max_iterations applied
    assert out[0].iterations > 2


def test_run_batch_leaves_inputs_unmodified(stand_in):
    Xf, Xm = surface_pair(2000, 5)
    pc1, pc2 = PointCloud(Xf, columns=["x", "y", "z"]), PointCloud(Xm, columns=["x", "y", "z"])
    c1, c2 = pc1.copy(deep=True), pc2.copy(deep=True)
    res = run_batch([(pc1, pc2)], correspondences=500, max_overlap_distance=5.0)
    assert res[0].error is None
    assert list(pc1.columns) == list(c1.columns) and list(pc2.columns) == list(c2.columns)
    assert pc1.equals(c1) and pc2.equals(c2)


def test_run_batch_errors_are_per_pair_with_runs_message(stand_in):
    good = surface_pair(2000, 1)
    Xf, Xm = surface_pair(2000, 2)
    far = (Xf, Xm + np.array([1000.0, 0, 0]))
    per = [None, {"max_overlap_distance": 1.0}, {"min_planarity": 1.0}, None]
    out = run_batch([good, far, good, good], per_pair=per, correspondences=500)
    for i, kw in ((1, {"max_overlap_distance": 1.0}), (2, {"min_planarity": 1.0})):
        X1, X2 = (far if i == 1 else good)
        with pytest.raises(SimpleICPException) as ei:
            lone_run(X1, X2, correspondences=500, **kw)
        assert isinstance(out[i].error, SimpleICPException)
        assert str(out[i].error) == str(ei.value)
        assert out[i].H is None
    ref = lone_run(*good, correspondences=500)
    assert_same(out[0], ref)
    assert_same(out[3], ref)


def test_run_batch_refuses_debug_dirpath(stand_in, tmp_path):
    with pytest.raises(SimpleICPException, match="debug_dirpath"):
        run_batch([surface_pair(500, 0)], debug_dirpath=str(tmp_path))
    with pytest.raises(SimpleICPException, match="debug_dirpath"):
        run_batch([surface_pair(500, 0)] * 2, per_pair=[None, {"debug_dirpath": str(tmp_path)}])


def test_batch_pool_is_reused_and_reset(stand_in):
    a = backend.get_batch_contexts(3)
    b = backend.get_batch_contexts(2)
    assert b == a[:2]
    backend.reset_batch_contexts()
    assert backend.get_batch_contexts(1)[0] is not a[0]
    backend.reset_batch_contexts()


def test_upload_start_keeps_previous_source_alive_during_call():
    """the slot's previous source must still be referenced while sicp_cloud_upload_start runs (the C call joins the
    helper that may still be reading it).  A stub stands in for the C function and looks at what the Context holds."""
    ctx = _lib.Context.__new__(_lib.Context)
    ctx._h = C.c_void_p()
    ctx._bg_src = {}
    seen = []

    class StubLib:
        def sicp_cloud_upload_start(self, h, slot, xyz, x, y, z, n, base):
            held = ctx._bg_src.get(slot)
            seen.append(None if held is None else [a.ctypes.data for a in held])
            return _lib.OK

    ctx._L = StubLib()
    first = np.arange(30, dtype=np.float32).reshape(10, 3)        # float32: _f64 makes a temporary the helper reads
    ctx.upload_start(_lib.MOV, xyz=first)
    first_src = ctx._bg_src[_lib.MOV]
    ptr_first = first_src[0].ctypes.data
    del first_src
    ctx.upload_start(_lib.MOV, xyz=np.ones((7, 3), np.float32))
    assert seen[0] is None
    assert seen[1] == [ptr_first]                                 # the first call's temporary was alive during the second call
    assert ctx._bg_src[_lib.MOV][0].shape == (7, 3)
    ctx._h = C.c_void_p()


def test_run_batch_non_finite_pair_is_its_own_error(stand_in):
    good = surface_pair(2000, 1)
    Xf, Xm = surface_pair(2000, 2)
    Xm[5, 0] = np.nan
    out = run_batch([good, (Xf, Xm), good], correspondences=500)
    with pytest.raises(Exception) as ei:
        lone_run(Xf, Xm, correspondences=500)
    assert type(out[1].error) is type(ei.value) and str(out[1].error) == str(ei.value)
    ref = lone_run(*good, correspondences=500)
    assert_same(out[0], ref)
    assert_same(out[2], ref)


def test_run_batch_takes_runs_keywords_and_defaults():
    import inspect
    from simpleicp_amd import batch
    sig = inspect.signature(SimpleICP.run).parameters
    assert batch._RUN_DEFAULTS == {k: v.default for k, v in sig.items() if k != "self"}
    with pytest.raises(TypeError, match="unexpected keyword"):
        run_batch([surface_pair(100, 0)], no_such_argument=1)
