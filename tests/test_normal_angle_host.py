"""Rejection by the angle between normals, the parts that need no GPU: the properties of the reference's restatement of contract
(N) (tests/normal_angle_ref.py) and the new surface -- the companion header, the binding, the Python keywords."""
import inspect
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import normal_angle_ref as ref

ROOT = Path(__file__).resolve().parent.parent


def _data(n=4000, seed=3):
    rng = np.random.default_rng(seed)
    n1 = rng.standard_normal((n, 3)).astype(np.float32)
    n1 /= np.linalg.norm(n1, axis=1, keepdims=True)
    n2 = (n1 + 0.5 * rng.standard_normal((n, 3))).astype(np.float32)
    n2 /= np.linalg.norm(n2, axis=1, keepdims=True)
    return n1, n2


def _rot(a, b, c):
    from oracle import orc
    return orc.params_to_H(np.array([a, b, c, 0.5, -2.0, 7.0]))


def test_restatement_properties():
    n1, n2 = _data()
    H = _rot(0.3, -0.2, 0.7)
    cos_max = math.cos(math.radians(30.0))
    c = ref.cos_of(n1, n2, H)
    assert np.abs(np.abs(c) - cos_max).min() > 1e-12               # the threshold case is excluded by construction
    keep = ref.verdict(n1, n2, H, cos_max)
    assert 0 < keep.sum() < len(keep)
    # identical normals keep at any cos_max <= 1 (up to the rounding of a float32 unit vector's length: compare with its own |c|)
    same = ref.cos_of(n1, n1, np.eye(4))
    assert np.all(np.abs(same - 1.0) < 1e-6) and ref.verdict(n1, n1, np.eye(4), 1.0 - 1e-6).all()
    unit = np.eye(3, dtype=np.float32)
    assert ref.verdict(unit, unit, np.eye(4), 1.0).all()
    # normals are unoriented: flipping either changes no verdict
    assert np.array_equal(ref.verdict(-n1, n2, H, cos_max), keep) and np.array_equal(ref.verdict(n1, -n2, H, cos_max), keep)
    # a NaN component fails
    bad = n2.copy()
    bad[::7, 1] = np.nan
    assert not ref.verdict(n1, bad, H, cos_max)[::7].any()
    bad1 = n1.copy()
    bad1[::5, 2] = np.nan
    assert not ref.verdict(bad1, n2, H, cos_max)[::5].any()
    # invariance under a common rotation G of n1 and H (n1 -> G n1, H -> G H), the threshold case being excluded above
    G = _rot(-0.4, 0.9, 0.1)
    n1g = (G[:3, :3] @ n1.astype(np.float64).T).T
    cg = (n1g * (((G @ H)[:3, :3]) @ n2.astype(np.float64).T).T).sum(axis=1)
    assert np.abs(cg - c).max() < 1e-12
    assert np.array_equal(np.abs(cg) >= cos_max, keep)


def test_stub_stays_and_signatures_are_the_references():
    from simpleicp_amd import SimpleICP
    from simpleicp_amd.corrpts import CorrPts
    with pytest.raises(NotImplementedError):
        CorrPts(None, None).reject_wrt_to_angle_between_normals()
    assert list(inspect.signature(CorrPts.reject_wrt_to_angle_between_normals).parameters) == ["self"]
    assert list(inspect.signature(CorrPts.reject_wrt_normal_angle).parameters)[:2] == ["self", "max_angle"]
    names = list(inspect.signature(SimpleICP.run).parameters)
    assert names == ["self", "correspondences", "neighbors", "min_planarity", "max_overlap_distance", "min_change", "max_iterations",
                     "distance_weights", "rbp_observed_values", "rbp_observation_weights", "debug_dirpath"]
    assert SimpleICP.max_normal_angle is None and SimpleICP(verbose=False).max_normal_angle is None
    assert list(inspect.signature(SimpleICP.__init__).parameters) == ["self", "verbose"]


def _header_functions():
    text = (ROOT / "include" / "simpleicp_hip_normals.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sicp_\w+)\s*\(", text)))


def test_header_names_are_exported_and_bound():
    from simpleicp_amd import _lib, build
    assert _header_functions() == sorted(_lib.NORMALS_EXPORTS)
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", str(so)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sicp_\w+)", out))
    assert set(_lib.NORMALS_EXPORTS) <= exported
    assert not set(_lib.NORMALS_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.BATCH_EXPORTS) | set(_lib.DEVICE_EXPORTS))
    L = _lib.load()
    for name in _lib.NORMALS_EXPORTS:
        assert hasattr(L, name)
    assert L.sicp_normals_version() == _lib.NORMALS_VERSION == 1
    assert "#define SICP_NORMALS_VERSION 1" in (ROOT / "include" / "simpleicp_hip_normals.h").read_text()
    # the main header and its version are untouched
    assert "normal_angle" not in (ROOT / "include" / "simpleicp_hip.h").read_text()
    for name in ("set_normals", "normal_angle_set", "corr_reject_normal_angle", "normal_angle_info", "normal_cache"):
        assert callable(getattr(_lib.Context, name))


@pytest.mark.parametrize("angle", [0.0, -5.0, 90.5, float("nan"), "wide"])
def test_angle_out_of_range_is_refused_before_any_backend_call(angle, monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import PointCloud, SimpleICP, SimpleICPException, backend

    def no_backend(*a, **k):
        raise AssertionError("the backend was called")
    monkeypatch.setattr(backend, "get_context", no_backend)
    monkeypatch.setattr(backend, "get_batch_contexts", no_backend)
    X = np.random.default_rng(0).standard_normal((50, 3))
    icp = SimpleICP(verbose=False)
    icp.add_point_clouds(PointCloud(X, columns=["x", "y", "z"]), PointCloud(X, columns=["x", "y", "z"]))
    icp.max_normal_angle = angle
    with pytest.raises(SimpleICPException, match="max_normal_angle"):
        icp.run()
    with pytest.raises(SimpleICPException, match="max_normal_angle"):
        simpleicp_amd.run_batch([(X, X)], max_normal_angle=angle)
    with pytest.raises(SimpleICPException, match="max_normal_angle"):
        simpleicp_amd.run_batch([(X, X)], per_pair=[{"max_normal_angle": angle}])
    with pytest.raises(SimpleICPException, match="max_normal_angle"):
        simpleicp_amd.run_tensors(X, X, max_normal_angle=angle)


def test_keywords_accepted_and_misspelt_ones_refused(monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import backend, batch

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached
    monkeypatch.setattr(backend, "get_batch_contexts", stop)
    X = np.random.default_rng(0).standard_normal((50, 3))
    assert "max_normal_angle" in inspect.signature(simpleicp_amd.run_batch).parameters
    assert "max_normal_angle" in inspect.signature(simpleicp_amd.run_tensors).parameters
    assert "max_normal_angle" not in batch._RUN_DEFAULTS
    with pytest.raises(Reached):                                   # accepted: the call gets as far as the device
        simpleicp_amd.run_batch([(X, X)], max_normal_angle=30.0)
    with pytest.raises(Reached):
        simpleicp_amd.run_batch([(X, X)], per_pair=[{"max_normal_angle": 45}])
    with pytest.raises(TypeError, match="max_normal_angel"):
        simpleicp_amd.run_batch([(X, X)], max_normal_angel=30.0)
    with pytest.raises(TypeError, match="max_normal_angel"):
        simpleicp_amd.run_batch([(X, X)], per_pair=[{"max_normal_angel": 30.0}])
    with pytest.raises(TypeError, match="max_normal_angel"):
        simpleicp_amd.run_tensors(X, X, max_normal_angel=30.0)
    with pytest.raises(TypeError, match="torch.Tensor"):           # accepted: refused for the clouds, not for the keyword
        simpleicp_amd.run_tensors(X, X, max_normal_angle=30.0)
