"""What the binding hands to the C entry points, argument by argument: every operator method of Context in its array form and in
its pointer form, against a library whose exports only record.  No device, no shared library: the marshalling alone."""
import ctypes as C
import math
import struct

import numpy as np
import pytest

from simpleicp_amd import _lib

HANDLE, N = 0x1234, 5
FIX = _lib.FIX


class _Recorder:
    """Stands in for the loaded library: the version functions answer with the binding's versions, every other export notes its
    positional arguments and returns OK."""

    def __init__(self):
        self.calls = []
        self.versions = {"sicp_abi_version": _lib.ABI_VERSION, "sicp_batch_version": _lib.BATCH_VERSION}
        self.versions.update({f.exports[0]: f.version for f in _lib.FEATURES.values() if f.version is not None})

    def __getattr__(self, name):
        if not name.startswith("sicp_"):
            raise AttributeError(name)
        if name in self.versions:
            return lambda: self.versions[name]

        def export(*args):
            self.calls.append((name, args))
            return _lib.OK
        return export


class _Tensor:
    """As much of a device tensor as the binding looks at."""

    def __init__(self, shape, address):
        self.shape, self._address = shape, address

    def data_ptr(self):
        return self._address


@pytest.fixture
def bound(monkeypatch):
    L = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda: L)
    ctx = _lib.Context.__new__(_lib.Context)
    ctx._L, ctx._h, ctx._Q, ctx._bg_src = L, C.c_void_p(HANDLE), N, {}
    ctx.size = lambda slot: N
    yield ctx, L.calls
    ctx._h = C.c_void_p()                      # (nothing to destroy)


def P(a):
    """A pointer argument: to this address, or to this array's buffer."""
    return ("ptr", a if isinstance(a, int) else a.ctypes.data)


def I(v):
    return (int, v)


def F(v):
    return (float, v)


ANY = ("ptr", "anywhere")


def _seen(a):
    if a is None:
        return None
    if isinstance(a, C.c_void_p):
        return ("ptr", a.value)
    if hasattr(a, "_obj"):                     # (what C.byref returns)
        return ("ref", a._obj)
    return (type(a), a)


def the_call(calls, name, expected):
    """The one call recorded since the last look: its entry, its argument count, and every argument after the context handle --
    None, P / I / F, ANY (some non-null pointer), a ctypes class (a reference to one of those) or a ctypes object (to that one)."""
    assert len(calls) == 1, calls
    got, args = calls.pop()
    assert got == name
    assert len(args) == len(expected) + 1, (len(args), name)
    assert _seen(args[0]) == ("ptr", HANDLE)
    for i, (a, e) in enumerate(zip(args[1:], expected), 1):
        g = _seen(a)
        if isinstance(e, type):
            assert g[0] == "ref" and type(g[1]) is e, (name, i, g)
        elif e is ANY:
            assert g[0] == "ptr" and g[1], (name, i, g)
        elif isinstance(e, (C.Structure, C._SimpleCData)):
            assert g[0] == "ref" and g[1] is e, (name, i, g)
        else:
            assert g == e, (name, i, g, e)
    return args


ROWS = np.array([4, 0, 2], np.int64)
ORIGIN = np.array([0.5, -1.0, 2.0])
SRC = np.arange(15, dtype=np.float64).reshape(N, 3)
DST = SRC + 1.0
POSE = np.array([[1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0.5, 0.25, 0.125]])
TRIPLES = np.array([[0, 1, 2], [2, 3, 4], [4, 0, 1]], np.int32)


# ---- the ten operators ----
def test_voxel_select(bound):
    ctx, calls = bound
    keep = ctx.voxel_select(FIX, 1)
    assert keep.dtype == np.bool_ and keep.shape == (N,)
    the_call(calls, "sicp_voxel_select", [I(FIX), None, I(N), F(1.0), None, P(keep), C.c_int64])
    keep = ctx.voxel_select(FIX, 0.5, origin=ORIGIN, rows=ROWS)
    assert keep.shape == (3,)
    the_call(calls, "sicp_voxel_select", [I(FIX), P(ROWS), I(3), F(0.5), P(ORIGIN), P(keep), C.c_int64])
    assert ctx.voxel_select(FIX, np.float32(0.5), origin=ORIGIN, keep_ptr=0x7000) == 0
    the_call(calls, "sicp_voxel_select", [I(FIX), None, I(N), F(0.5), P(ORIGIN), P(0x7000), C.c_int64])
    assert ctx.voxel_select(FIX, 0.5, rows=ROWS, keep_ptr=0x7000) == 0
    the_call(calls, "sicp_voxel_select", [I(FIX), P(ROWS), I(3), F(0.5), None, P(0x7000), C.c_int64])


def test_outlier_statistical(bound):
    ctx, calls = bound
    keep, d, st = ctx.outlier_statistical(FIX, np.int64(2), 2)
    assert keep.dtype == np.bool_ and keep.shape == (N,) and d.dtype == np.float64 and d.shape == (N,)
    assert type(st) is _lib.OutlierStats
    the_call(calls, "sicp_outlier_statistical", [I(FIX), None, I(N), None, I(2), F(2.0), P(keep), P(d), st])
    keep, d, st = ctx.outlier_statistical(FIX, 2, 1.5, rows=ROWS)
    assert keep.shape == (3,) and d.shape == (3,)
    the_call(calls, "sicp_outlier_statistical", [I(FIX), P(ROWS), I(3), None, I(2), F(1.5), P(keep), P(d), st])
    st = ctx.outlier_statistical(FIX, 2, 1.5, mask_ptr=0x5000, keep_ptr=0x5000)
    assert type(st) is _lib.OutlierStats
    the_call(calls, "sicp_outlier_statistical", [I(FIX), None, I(N), P(0x5000), I(2), F(1.5), P(0x5000), None, st])
    st = ctx.outlier_statistical(FIX, 2, 1.5, rows=ROWS, keep_ptr=0x7000, mean_ptr=0x7100)
    the_call(calls, "sicp_outlier_statistical", [I(FIX), P(ROWS), I(3), None, I(2), F(1.5), P(0x7000), P(0x7100), st])


def test_outlier_radius(bound):
    ctx, calls = bound
    keep, cnt, kept = ctx.outlier_radius(FIX, 1, np.int64(3))
    assert keep.dtype == np.bool_ and keep.shape == (N,) and cnt.dtype == np.uint32 and cnt.shape == (N,) and kept == 0
    the_call(calls, "sicp_outlier_radius", [I(FIX), None, I(N), None, F(1.0), I(3), P(keep), P(cnt), C.c_int64])
    keep, cnt, kept = ctx.outlier_radius(FIX, 0.25, 3, rows=ROWS)
    assert keep.shape == (3,) and cnt.shape == (3,)
    the_call(calls, "sicp_outlier_radius", [I(FIX), P(ROWS), I(3), None, F(0.25), I(3), P(keep), P(cnt), C.c_int64])
    assert ctx.outlier_radius(FIX, 0.25, 3, mask_ptr=0x5000, keep_ptr=0x7000) == 0
    the_call(calls, "sicp_outlier_radius", [I(FIX), None, I(N), P(0x5000), F(0.25), I(3), P(0x7000), None, C.c_int64])
    assert ctx.outlier_radius(FIX, 0.25, 3, rows=ROWS, keep_ptr=0x7000, count_ptr=0x7100) == 0
    the_call(calls, "sicp_outlier_radius", [I(FIX), P(ROWS), I(3), None, F(0.25), I(3), P(0x7000), P(0x7100), C.c_int64])


def test_fpfh(bound):
    ctx, calls = bound
    normals = np.ones((N, 3), np.float32)
    view = np.array([0.0, 0.0, 9.0])
    out, cnt, st = ctx.fpfh(FIX, normals, np.int64(2))
    assert out.dtype == np.float32 and out.shape == (N, 33) and cnt is None and type(st) is _lib.FpfhStats
    the_call(calls, "sicp_fpfh", [I(FIX), P(normals), I(2), F(math.inf), None, P(out), None, st])
    out, cnt, st = ctx.fpfh(FIX, normals, 2, 1, view, want_counts=True)
    assert cnt.dtype == np.uint16 and cnt.shape == (N, 34)
    the_call(calls, "sicp_fpfh", [I(FIX), P(normals), I(2), F(1.0), P(view), P(out), P(cnt), st])
    device_normals = _Tensor((N, 3), 0x9000)
    st = ctx.fpfh(FIX, device_normals, 2, 0.5, fpfh_ptr=0x7000)
    assert type(st) is _lib.FpfhStats
    the_call(calls, "sicp_fpfh", [I(FIX), P(0x9000), I(2), F(0.5), None, P(0x7000), None, st])
    st = ctx.fpfh(FIX, device_normals, 2, 0.5, view, fpfh_ptr=0x7000, counts_ptr=0x7100)
    the_call(calls, "sicp_fpfh", [I(FIX), P(0x9000), I(2), F(0.5), P(view), P(0x7000), P(0x7100), st])
    with pytest.raises(ValueError, match="normals must have shape"):
        ctx.fpfh(FIX, normals[:4], 2)
    assert not calls


def test_keypoints(bound):
    ctx, calls = bound
    keep, sal, eig, st = ctx.keypoints(FIX, np.int64(2))
    assert keep.dtype == np.bool_ and keep.shape == (N,) and sal is None and eig is None and type(st) is _lib.KeypointStats
    the_call(calls, "sicp_keypoints", [I(FIX), I(2), F(math.inf), I(2), F(math.inf), F(0.975), F(0.975), I(5), P(keep), None, None, st])
    keep, sal, eig, st = ctx.keypoints(FIX, 2, 1, 3, 2, 1, 0.5, np.int64(4), want_saliency=True)
    assert sal.dtype == np.float64 and sal.shape == (N,) and eig.dtype == np.float64 and eig.shape == (N, 3)
    the_call(calls, "sicp_keypoints", [I(FIX), I(2), F(1.0), I(3), F(2.0), F(1.0), F(0.5), I(4), P(keep), P(sal), P(eig), st])
    st = ctx.keypoints(FIX, 2, 1.0, None, 2.0, keep_ptr=0x7000)
    assert type(st) is _lib.KeypointStats
    the_call(calls, "sicp_keypoints", [I(FIX), I(2), F(1.0), I(2), F(2.0), F(0.975), F(0.975), I(5), P(0x7000), None, None, st])
    st = ctx.keypoints(FIX, 2, 1.0, 3, 2.0, keep_ptr=0x7000, saliency_ptr=0x7100, eig_ptr=0x7200)
    the_call(calls, "sicp_keypoints", [I(FIX), I(2), F(1.0), I(3), F(2.0), F(0.975), F(0.975), I(5), P(0x7000), P(0x7100), P(0x7200), st])
    st = ctx.keypoints(FIX, 2, keep_ptr=0x7000, eig_ptr=0x7200)
    the_call(calls, "sicp_keypoints", [I(FIX), I(2), F(math.inf), I(2), F(math.inf), F(0.975), F(0.975), I(5), P(0x7000), None, P(0x7200), st])


def test_feature_match(bound):
    ctx, calls = bound
    q, t = np.ones((N, 4), np.float32), np.zeros((3, 4), np.float32)
    idx, d2, st = ctx.feature_match(q, t)
    assert idx.dtype == np.int32 and idx.shape == (N,) and d2.dtype == np.float32 and d2.shape == (N,) and type(st) is _lib.MatchStats
    the_call(calls, "sicp_feature_match", [P(q), I(N), P(t), I(3), I(4), P(idx), P(d2), st])
    idx, d2, st = ctx.feature_match(q, t, want_d2=False)
    assert d2 is None
    the_call(calls, "sicp_feature_match", [P(q), I(N), P(t), I(3), I(4), P(idx), None, st])
    st = ctx.feature_match(0x1000, 0x2000, np.int64(N), 3, 4, idx_ptr=0x7000)
    assert type(st) is _lib.MatchStats
    the_call(calls, "sicp_feature_match", [P(0x1000), I(N), P(0x2000), I(3), I(4), P(0x7000), None, st])
    st = ctx.feature_match(0x1000, 0x2000, N, 3, 4, idx_ptr=0x7000, d2_ptr=0x7100)
    the_call(calls, "sicp_feature_match", [P(0x1000), I(N), P(0x2000), I(3), I(4), P(0x7000), P(0x7100), st])
    with pytest.raises(ValueError, match=r"query and target must be \(nq, dim\) and \(nt, dim\)"):
        ctx.feature_match(q, t[:, :3])
    assert not calls


def test_ransac_triplets(bound):
    ctx, calls = bound
    poses, inl, st = ctx.ransac_triplets(SRC, DST, TRIPLES, 1, 0.9)
    assert poses.dtype == np.float64 and poses.shape == (3, 12) and inl.dtype == np.int32 and inl.shape == (3,)
    assert type(st) is _lib.RansacStats
    the_call(calls, "sicp_ransac_triplets", [P(SRC), P(DST), I(N), P(TRIPLES), I(3), F(1.0), F(0.9), P(poses), P(inl), st])
    poses, inl, st = ctx.ransac_triplets(SRC, DST, TRIPLES, 0.5, 1, want_poses=False)
    assert poses is None
    the_call(calls, "sicp_ransac_triplets", [P(SRC), P(DST), I(N), P(TRIPLES), I(3), F(0.5), F(1.0), None, P(inl), st])
    st = ctx.ransac_triplets(0x1000, 0x2000, 0x3000, 0.5, 0.9, m=np.int64(N), h=3, inliers_ptr=0x7000)
    assert type(st) is _lib.RansacStats
    the_call(calls, "sicp_ransac_triplets", [P(0x1000), P(0x2000), I(N), P(0x3000), I(3), F(0.5), F(0.9), None, P(0x7000), st])
    st = ctx.ransac_triplets(0x1000, 0x2000, 0x3000, 0.5, 0.9, m=N, h=3, poses_ptr=0x7100, inliers_ptr=0x7000)
    the_call(calls, "sicp_ransac_triplets", [P(0x1000), P(0x2000), I(N), P(0x3000), I(3), F(0.5), F(0.9), P(0x7100), P(0x7000), st])
    with pytest.raises(ValueError, match=r"src and dst must be \(m, 3\), triples \(h, 3\)"):
        ctx.ransac_triplets(SRC, DST[:4], TRIPLES, 0.5, 0.9)
    assert not calls


def test_pose_refit(bound):
    ctx, calls = bound
    out, inl, st = ctx.pose_refit(SRC, DST, None, 1, np.int64(3))
    assert out.dtype == np.float64 and out.shape == (1, 12) and inl.dtype == np.int32 and inl.shape == (1,)
    assert type(st) is _lib.PosefitStats
    the_call(calls, "sicp_pose_refit", [P(SRC), P(DST), I(N), None, I(1), F(1.0), I(3), P(out), P(inl), st])
    out, inl, st = ctx.pose_refit(SRC, DST, POSE, math.inf, 3)
    the_call(calls, "sicp_pose_refit", [P(SRC), P(DST), I(N), P(POSE), I(1), F(math.inf), I(3), P(out), P(inl), st])
    st = ctx.pose_refit(0x1000, 0x2000, None, 0.5, 3, m=np.int64(N), b=np.int64(1), poses_ptr=0x7100, inliers_ptr=0x7000)
    assert type(st) is _lib.PosefitStats
    the_call(calls, "sicp_pose_refit", [P(0x1000), P(0x2000), I(N), None, I(1), F(0.5), I(3), P(0x7100), P(0x7000), st])
    st = ctx.pose_refit(0x1000, 0x2000, 0x3000, 0.5, 3, m=N, b=1, poses_ptr=0x7100, inliers_ptr=0x7000)
    the_call(calls, "sicp_pose_refit", [P(0x1000), P(0x2000), I(N), P(0x3000), I(1), F(0.5), I(3), P(0x7100), P(0x7000), st])
    with pytest.raises(ValueError, match=r"src and dst must be \(m, 3\), poses \(b, 12\) or None"):
        ctx.pose_refit(SRC, DST, POSE[:, :11], 0.5, 3)
    assert not calls


def test_pose_robust(bound):
    ctx, calls = bound
    out, inl, scales, st = ctx.pose_robust(SRC, DST, None, 1, np.int64(8), 2)
    assert out.dtype == np.float64 and out.shape == (1, 12) and inl.dtype == np.int32 and inl.shape == (1,)
    assert scales.dtype == np.float64 and scales.shape == (1,) and type(st) is _lib.RobustStats
    the_call(calls, "sicp_pose_robust", [P(SRC), P(DST), I(N), None, I(1), F(1.0), I(8), F(2.0), F(0.0), P(out), P(inl), P(scales), st])
    out, inl, scales, st = ctx.pose_robust(SRC, DST, POSE, 0.5, 8, 1.4, 4)
    the_call(calls, "sicp_pose_robust", [P(SRC), P(DST), I(N), P(POSE), I(1), F(0.5), I(8), F(1.4), F(4.0), P(out), P(inl), P(scales), st])
    st = ctx.pose_robust(0x1000, 0x2000, None, 0.5, 8, 1.4, m=np.int64(N), b=np.int64(1), poses_ptr=0x7100, inliers_ptr=0x7000,
                         scales_ptr=0x7200)
    assert type(st) is _lib.RobustStats
    the_call(calls, "sicp_pose_robust", [P(0x1000), P(0x2000), I(N), None, I(1), F(0.5), I(8), F(1.4), F(0.0), P(0x7100), P(0x7000),
                                         P(0x7200), st])
    st = ctx.pose_robust(0x1000, 0x2000, 0x3000, 0.5, 8, 1.4, 4.0, m=N, b=1, poses_ptr=0x7100, inliers_ptr=0x7000, scales_ptr=0x7200)
    the_call(calls, "sicp_pose_robust", [P(0x1000), P(0x2000), I(N), P(0x3000), I(1), F(0.5), I(8), F(1.4), F(4.0), P(0x7100), P(0x7000),
                                         P(0x7200), st])


def test_match_consistency(bound):
    ctx, calls = bound
    degree, core, st = ctx.match_consistency(SRC, DST, 1, 0)
    assert degree.dtype == np.int32 and degree.shape == (N,) and core.dtype == np.int32 and core.shape == (N,)
    assert degree.ctypes.data != core.ctypes.data and type(st) is _lib.ConsistencyStats
    the_call(calls, "sicp_match_consistency", [P(SRC), P(DST), I(N), F(1.0), F(0.0), P(degree), P(core), st])
    st = ctx.match_consistency(0x1000, 0x2000, 0.5, 0.25, m=np.int64(N), degree_ptr=0x7000, core_ptr=0x7100)
    assert type(st) is _lib.ConsistencyStats
    the_call(calls, "sicp_match_consistency", [P(0x1000), P(0x2000), I(N), F(0.5), F(0.25), P(0x7000), P(0x7100), st])
    with pytest.raises(ValueError, match=r"src and dst must be \(m, 3\)"):
        ctx.match_consistency(SRC[:, :2], DST, 0.5, 0.25)
    assert not calls


# ---- the clouds' columns ----
def test_set_planarity(bound):
    ctx, calls = bound
    ctx.set_planarity(FIX)
    the_call(calls, "sicp_cloud_set_planarity", [I(FIX), None, None, I(0), I(0)])
    dense = np.linspace(0, 1, N).astype(np.float32)
    ctx.set_planarity(FIX, dense)
    the_call(calls, "sicp_cloud_set_planarity", [I(FIX), None, P(dense), I(N), I(N)])
    part = dense[:3].copy()
    ctx.set_planarity(FIX, part, rows=ROWS)
    the_call(calls, "sicp_cloud_set_planarity", [I(FIX), P(ROWS), P(part), I(3), I(N)])
    ctx.set_planarity(FIX, part, rows=ROWS, n_global=np.int64(9))
    the_call(calls, "sicp_cloud_set_planarity", [I(FIX), P(ROWS), P(part), I(3), I(9)])
    ctx.set_planarity(FIX, np.empty(0, np.float32))
    the_call(calls, "sicp_cloud_set_planarity", [I(FIX), None, ANY, I(0), I(0)])
    with pytest.raises(ValueError, match="rows and planarity must have the same length"):
        ctx.set_planarity(FIX, dense, rows=ROWS)
    assert not calls


def test_set_normals(bound):
    ctx, calls = bound
    ctx.set_normals(_lib.MOV)
    the_call(calls, "sicp_cloud_set_normals", [I(_lib.MOV), None, None, I(0), I(0)])
    dense = np.ones((N, 3), np.float32)
    ctx.set_normals(_lib.MOV, dense)
    the_call(calls, "sicp_cloud_set_normals", [I(_lib.MOV), None, P(dense), I(N), I(N)])
    part = dense[:3].copy()
    ctx.set_normals(_lib.MOV, part, rows=ROWS)
    the_call(calls, "sicp_cloud_set_normals", [I(_lib.MOV), P(ROWS), P(part), I(3), I(N)])
    ctx.set_normals(_lib.MOV, part.reshape(9), rows=ROWS, n_global=9)
    the_call(calls, "sicp_cloud_set_normals", [I(_lib.MOV), P(ROWS), P(part), I(3), I(9)])
    ctx.set_normals(_lib.MOV, np.empty((0, 3), np.float32))
    the_call(calls, "sicp_cloud_set_normals", [I(_lib.MOV), None, ANY, I(0), I(0)])
    with pytest.raises(ValueError, match="rows and normals must have the same length"):
        ctx.set_normals(_lib.MOV, dense, rows=ROWS)
    assert not calls


# ---- the iteration's parameters ----
X = [0.01, -0.02, 0.03, 0.2, -0.1, 0.05]
OBS = [0.0, 0.0, 0.5, 1.0, 2.0, 3.0]
WEIGHT = [0.0, 1.0, 0.0, 4.0, 0.0, 9.0]


def _params_bytes(min_planarity, distance_weight, max_lm_steps):
    return struct.pack("=18d2dq", *X, *OBS, *WEIGHT, min_planarity, distance_weight, max_lm_steps)


@pytest.mark.parametrize("weight, packed", [(2.5, 2.5), (None, -1.0)])
def test_iter_params_bytes(bound, weight, packed):
    ctx, calls = bound
    want = _params_bytes(0.4, packed, 7)
    assert C.sizeof(_lib.IterParams) == len(want) == 168
    made = ctx._params(np.array(X), OBS, tuple(WEIGHT), 0.4, weight, np.int64(7))
    assert type(made) is _lib.IterParams and bytes(made) == want
    assert bytes(_lib.Context._params(X, OBS, WEIGHT, distance_weight=weight)) == _params_bytes(0.3, packed, 0)

    R = ctx.icp_iterate(np.array(X), OBS, WEIGHT, 0.4, weight, np.int64(7))
    assert type(R) is _lib.IterResult
    args = the_call(calls, "sicp_icp_iterate", [_lib.IterParams, R])
    assert bytes(args[1]._obj) == want

    assert ctx.icp_run(np.array(X), OBS, WEIGHT, 0.4, weight, np.int64(3), 2, np.int64(7)) == []
    name, args = calls.pop()
    assert name == "sicp_icp_run" and len(args) == 6 and not calls
    assert _seen(args[0]) == ("ptr", HANDLE) and bytes(args[1]._obj) == want
    assert _seen(args[2]) == I(3) and _seen(args[3]) == F(2.0)
    assert isinstance(args[4], C.Array) and args[4]._type_ is _lib.IterResult and len(args[4]) == 3
    assert type(args[5]._obj) is C.c_int64


# ---- the records ----
def test_stats_records_as_dicts():
    sizes = {_lib.OutlierStats: 40, _lib.FpfhStats: 32, _lib.MatchStats: 24, _lib.RansacStats: 40, _lib.PosefitStats: 40,
             _lib.RobustStats: 32, _lib.ConsistencyStats: 56, _lib.KeypointStats: 48}
    for cls, size in sizes.items():
        assert C.sizeof(cls) == size and issubclass(cls, C.Structure)
        st = cls(*range(1, len(cls._fields_) + 1))
        d = st.as_dict()
        assert list(d) == [name for name, _ in cls._fields_]
        for i, (name, kind) in enumerate(cls._fields_, 1):
            assert type(d[name]) is (float if kind is C.c_double else int) and d[name] == i
