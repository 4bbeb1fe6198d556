"""Robust pose fit (contract (G)), the parts that need no GPU: the companion header and the binding, the
refusals that come before any device work, the numpy reference (tests/robust_ref.py) and its properties -- the plain fit as a
special case, the schedule of the scale, NaN rows, the recovery of a motion under 80 % wrong matches --, and the plumbing of
robust_pose and register_global(method="robust") on a stand-in context."""
import ctypes as C
import inspect
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import fpfh_ref
import global_ref
import oracle_backend
import posefit_ref
import robust_ref

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "simpleicp_hip_robust.h"

# The largest rotation and translation error of the reference over recovery_cases() (m = 400, 80 % wrong matches, noise 0.002,
# max_distance 0.01, 64 rounds, divisor 1.4, identity start, automatic scale), measured on the CPU (x86-64, numpy / OpenBLAS):
# 0.0434 degrees (seed 4) and 6.114e-4 (seed 1); the inliers are the 80 true matches in every case.  DESIGN.md section 20.  The
# bounds are 10 x those: room for other libm and BLAS builds.
RECOVERY_ANGLE_BOUND = 0.434
RECOVERY_SHIFT_BOUND = 6.114e-3


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def rotation(axis, angle):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


R_TRUE, T_TRUE = rotation([1.0, 2.0, 3.0], 0.7), np.array([0.3, -0.2, 0.1])


def noisy_copy(rng, m, wrong=0.4, noise=0.002):
    """test_posefit_host's noisy rigid copy, and the mask of the rows that stayed matches."""
    src = rng.uniform(-1, 1, (m, 3))
    dst = src @ R_TRUE.T + T_TRUE + rng.normal(0, noise, (m, 3))
    bad = rng.choice(m, int(wrong * m), replace=False)
    dst[bad] = rng.uniform(-1, 1, (len(bad), 3))
    good = np.ones(m, bool)
    good[bad] = False
    return src, dst, good


def recovery_cases():
    return [(seed,) + noisy_copy(np.random.default_rng(1000 * seed + 400), 400, wrong=0.8, noise=0.002) for seed in range(5)]


def pose_error(pose):
    dR = pose[:9].reshape(3, 3) @ R_TRUE.T
    return np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1))), np.linalg.norm(pose[9:] - T_TRUE)


# ---- header, exports, binding ----
def test_header_names_are_exported_and_bound():
    from simpleicp_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(sicp_\w+)\s*\(", text))) == sorted(_lib.ROBUST_EXPORTS) == ["sicp_pose_robust", "sicp_robust_version"]
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", str(so)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sicp_\w+)", out))
    assert set(_lib.ROBUST_EXPORTS) <= exported
    others = (set(_lib.EXPORTS) | set(_lib.BATCH_EXPORTS) | set(_lib.DEVICE_EXPORTS) | set(_lib.NORMALS_EXPORTS) | set(_lib.VOXEL_EXPORTS)
              | set(_lib.EVAL_EXPORTS) | set(_lib.OUTLIER_EXPORTS) | set(_lib.CHAIN_EXPORTS) | set(_lib.FPFH_EXPORTS)
              | set(_lib.GLOBAL_EXPORTS) | set(_lib.POSEFIT_EXPORTS))
    assert not set(_lib.ROBUST_EXPORTS) & others
    L = _lib.load()
    head = HEADER.read_text()
    # the version triple: the header's, the library's, the binding's
    assert "#define SICP_ROBUST_VERSION 1" in head
    assert L.sicp_robust_version() == _lib.ROBUST_VERSION == 1 and _lib.robust_version() == 1
    assert f"#define SICP_ROBUST_MAX_ROUNDS {_lib.ROBUST_MAX_ROUNDS}" in head and _lib.ROBUST_MAX_ROUNDS == robust_ref.MAX_ROUNDS == 256
    assert C.sizeof(_lib.RobustStats) == 32
    assert _lib.FEATURES["robust"].exports == _lib.ROBUST_EXPORTS and _lib.FEATURES["robust"].header == HEADER.name
    # the main header, its version and the other companions are untouched
    assert L.sicp_abi_version() == _lib.ABI_VERSION == 7 and L.sicp_global_version() == _lib.GLOBAL_VERSION == 1
    assert L.sicp_posefit_version() == _lib.POSEFIT_VERSION == 1 and L.sicp_fpfh_version() == _lib.FPFH_VERSION == 1
    assert "#define SICP_POSEFIT_VERSION 1" in (ROOT / "include" / "simpleicp_hip_posefit.h").read_text()
    assert "#define SICP_GLOBAL_VERSION 1" in (ROOT / "include" / "simpleicp_hip_global.h").read_text()
    for other in ("simpleicp_hip.h", "simpleicp_hip_posefit.h", "simpleicp_hip_global.h"):
        assert "robust" not in (ROOT / "include" / other).read_text().lower()
    assert list(inspect.signature(_lib.Context.pose_robust).parameters)[1:] == [
        "src", "dst", "poses", "max_distance", "rounds", "divisor", "start_scale", "m", "b", "poses_ptr", "inliers_ptr", "scales_ptr"]
    assert any(p.name == "sicp_robust.hip" for p in build.SOURCES) and any(p.name == HEADER.name for p in build.HEADERS)
    assert any(p.name == "sicp_horn.h" for p in build.HEADERS)


def test_null_ctx_is_refused_not_dereferenced():
    from simpleicp_amd import _lib
    L = _lib.load()
    P = _lib._ptr
    X, pose, out, inl, sc, st = (np.zeros((4, 3)), np.zeros((1, 12)), np.full((1, 12), 7.0), np.full(1, 7, np.int32), np.full(1, 7.0),
                                 _lib.RobustStats())
    assert L.sicp_pose_robust(None, P(X), P(X), 4, P(pose), 1, 1.0, 1, 1.4, 0.0, P(out), P(inl), P(sc), C.byref(st)) == _lib.ERR_INVALID
    assert b"null ctx" in L.sicp_last_error() and np.all(inl == 7) and np.all(out == 7.0) and np.all(sc == 7.0)


# ---- argument errors before the backend is touched ----
def test_python_argument_errors_come_before_the_backend(monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import backend

    def no_backend(*a, **k):
        raise AssertionError("the backend was called")
    monkeypatch.setattr(backend, "get_context", no_backend)
    assert "robust_pose" in simpleicp_amd.__all__
    rp, rg = simpleicp_amd.robust_pose, simpleicp_amd.register_global
    sig = inspect.signature(rp).parameters
    assert list(sig) == ["src", "dst", "max_distance", "H", "rounds", "divisor", "start_scale"]
    assert all(p.kind == p.KEYWORD_ONLY for n, p in sig.items() if n not in ("src", "dst"))
    assert (sig["H"].default, sig["rounds"].default, sig["divisor"].default, sig["start_scale"].default) == (None, 64, 1.4, None)
    X = np.random.default_rng(0).standard_normal((10, 3))
    with pytest.raises(TypeError):
        rp(X, X)                                                      # max_distance has no default
    for d in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_distance"):
            rp(X, X, max_distance=d)
    for d in ("far", None, True):
        with pytest.raises(TypeError, match="max_distance"):
            rp(X, X, max_distance=d)
    for r in (0, -1, 257):
        with pytest.raises(ValueError, match="rounds"):
            rp(X, X, max_distance=1.0, rounds=r)
    with pytest.raises(TypeError, match="rounds"):
        rp(X, X, max_distance=1.0, rounds=2.0)
    for q in (1.0, 0.5, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="divisor"):
            rp(X, X, max_distance=1.0, divisor=q)
    with pytest.raises(TypeError, match="divisor"):
        rp(X, X, max_distance=1.0, divisor="2")
    for s in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="start_scale"):
            rp(X, X, max_distance=1.0, start_scale=s)
    with pytest.raises(TypeError, match="start_scale"):
        rp(X, X, max_distance=1.0, start_scale=True)
    for bad in (np.eye(3), np.zeros((0, 4, 4)), np.zeros((2, 2, 4, 4)), np.zeros(16)):
        with pytest.raises(ValueError, match="H must"):
            rp(X, X, max_distance=1.0, H=bad)
    with pytest.raises(ValueError, match="same number"):
        rp(X, X[:9], max_distance=1.0)
    with pytest.raises(ValueError, match="at least 3"):
        rp(X[:2], X[:2], max_distance=1.0)
    with pytest.raises(ValueError, match=r"\(m, 3\)"):
        rp(X[:, :2], X[:, :2], max_distance=1.0)
    # register_global: the method, and the keywords that belong to it
    assert list(inspect.signature(rg).parameters)[-1] == "ransac_kwargs"
    with pytest.raises(ValueError, match="method"):
        rg(X, X, max_distance=1.0, method="gnc")
    with pytest.raises(TypeError, match="method"):
        rg(X, X, max_distance=1.0, method=1)
    for name, value in (("hypotheses", 10), ("edge_ratio", 0.9), ("seed", 1), ("triples", None), ("top", 2), ("refine", 1)):
        with pytest.raises(TypeError, match=f"unexpected keyword argument '{name}'"):
            rg(X, X, max_distance=1.0, method="robust", **{name: value})
    for name, value in (("rounds", 10), ("divisor", 2.0), ("start_scale", 1.0)):
        for method in ({}, {"method": "ransac"}):
            with pytest.raises(TypeError, match=f"unexpected keyword argument '{name}'"):
                rg(X, X, max_distance=1.0, **method, **{name: value})
    with pytest.raises(ValueError, match="rounds"):
        rg(X, X, max_distance=1.0, method="robust", rounds=0)
    with pytest.raises(ValueError, match="divisor"):
        rg(X, X, max_distance=1.0, method="robust", divisor=1.0)
    with pytest.raises(ValueError, match="start_scale"):
        rg(X, X, max_distance=1.0, method="robust", start_scale=-1.0)
    with pytest.raises(ValueError, match="max_distance"):
        rg(X, X, max_distance=float("inf"), method="robust")


def test_a_distributed_job_is_refused(monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import backend, dist
    monkeypatch.setattr(backend, "get_context", lambda: (_ for _ in ()).throw(AssertionError("the backend was called")))
    monkeypatch.setattr(dist, "is_distributed", lambda: True)
    X = np.random.default_rng(0).standard_normal((10, 3))
    for call in (lambda: simpleicp_amd.robust_pose(X, X, max_distance=1.0),
                 lambda: simpleicp_amd.robust_pose(X, X, max_distance=1.0, H=np.eye(4)),
                 lambda: simpleicp_amd.register_global(X, X, max_distance=1.0, method="robust")):
        with pytest.raises(simpleicp_amd.SimpleICPException, match="does not run in a torch.distributed job"):
            call()


# ---- the reference alone ----
def test_one_round_at_a_huge_scale_is_the_plain_fit():
    """start_scale = 1e30: s + d2 == s for every d2 below 7e13, so u = 1.0, w = 1.0, W = n exactly, and every expression of the
    round is the plain fit's of contract (L)."""
    for m, wrong in ((3, 0.0), (65, 0.4), (1000, 0.4)):
        src, dst, _ = noisy_copy(np.random.default_rng(m), m, wrong)
        d2, counts = robust_ref.residuals(np.eye(3), np.zeros(3), src, dst)
        assert np.all(robust_ref.weights(d2, counts, np.float64(1e30)) == 1.0)
        P, inl, scales, rec = robust_ref.robust(src, dst, None, 0.01, 1, 1.4, 1e30)
        fP, _, _ = posefit_ref.refit(src, dst, None, np.inf, 1)
        assert np.array_equal(u64(P), u64(fP)) and scales[0] == np.float64(1e30) / np.float64(1.4)
        md2 = np.float64(0.01) * np.float64(0.01)
        assert inl[0] == int(posefit_ref.inlier_mask(P[0, :9].reshape(3, 3), P[0, 9:], src, dst, md2).sum())
        assert rec == dict(n_poses=1, n_void=0, best=0, best_inliers=int(inl[0]))


def test_the_scale_never_goes_below_md2_and_arrives_on_time():
    src, dst, _ = noisy_copy(np.random.default_rng(5), 200, 0.5)
    md2 = np.float64(0.01) * np.float64(0.01)
    for start, divisor in ((1.0, 1.4), (1.0, 2.0), (3.7e-3, 1.1), (5e-5, 1.4)):
        # the rounds the scale needs: divide as the contract divides until the clamp bites
        s, need = np.float64(max(start, md2)), 0
        while s > md2:
            s = max(s / np.float64(divisor), md2)
            need += 1
        for rounds in sorted({1, max(need - 1, 1), need, need + 3} - {0}):
            trace = []
            _, _, scales, _ = robust_ref.robust(src, dst, None, 0.01, rounds, divisor, start, trace=trace)
            used = [s for _, _, s in trace]
            assert len(used) == rounds and all(s >= md2 for s in used) and scales[0] >= md2
            assert all(a > b or a == b == md2 for a, b in zip(used, used[1:]))
            assert (scales[0] == md2) == (rounds >= need), (start, divisor, rounds, need, scales[0])
    # the automatic start: twice the largest squared residual under the start
    trace = []
    robust_ref.robust(src, dst, None, 0.01, 2, 1.4, 0.0, trace=trace)
    d2, counts = robust_ref.residuals(np.eye(3), np.zeros(3), src, dst)
    assert trace[0][2] == 2.0 * d2[counts].max() and trace[1][2] == trace[0][2] / np.float64(1.4)
    # ... clamped from below when every residual is tiny
    P, _, scales, _ = robust_ref.robust(src, src.copy(), None, 0.01, 3, 1.4, 0.0)
    assert scales[0] == md2 and np.array_equal(P[0], np.concatenate([np.eye(3).ravel(), np.zeros(3)]))


def test_a_nan_row_changes_nothing_but_its_own_weight():
    src, dst, _ = noisy_copy(np.random.default_rng(6), 129, 0.5)
    poses = np.stack([np.concatenate([np.eye(3).ravel(), np.zeros(3)]), np.concatenate([R_TRUE.ravel(), T_TRUE])])
    base = robust_ref.robust(src, dst, poses, 0.01, 8, 1.4, 4.0)
    for row, (arr, col, value) in ((0, ("s", 1, np.nan)), (64, ("d", 2, np.inf)), (128, ("s", 0, -np.inf))):
        # whichever coordinate is not finite, and how: the row's terms are +0.0, so the results are those of the same row spoilt
        # in another way
        s2, d2 = src.copy(), dst.copy()
        (s2 if arr == "s" else d2)[row, col] = value
        s3, d3 = src.copy(), dst.copy()
        d3[row] = np.nan
        a, b = robust_ref.robust(s2, d2, poses, 0.01, 8, 1.4, 4.0), robust_ref.robust(s3, d3, poses, 0.01, 8, 1.4, 4.0)
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
        assert np.isfinite(a[0]).all() and np.all(a[1] >= 0)
        # and the other rows' weights are what they were
        r2, c2 = robust_ref.residuals(np.eye(3), np.zeros(3), s2, d2)
        r0, c0 = robust_ref.residuals(np.eye(3), np.zeros(3), src, dst)
        w2, w0 = robust_ref.weights(r2, c2, np.float64(4.0)), robust_ref.weights(r0, c0, np.float64(4.0))
        keep = np.arange(129) != row
        assert w2[row] == 0.0 and not np.signbit(w2[row]) and np.array_equal(u64(w2[keep]), u64(w0[keep]))
        # the automatic scale passes the row over as well
        t2, t0 = [], []
        robust_ref.robust(s2, d2, None, 0.01, 1, 1.4, 0.0, trace=t2)
        robust_ref.robust(np.delete(src, row, 0), np.delete(dst, row, 0), None, 0.01, 1, 1.4, 0.0, trace=t0)
        assert t2[0][2] == t0[0][2]
    assert np.isfinite(base[0]).all()
    # void poses, and a set without a row that counts
    void = poses.copy()
    void[0, 3] = np.nan
    P, inl, scales, rec = robust_ref.robust(src, dst, void, 0.01, 3, 1.4, 0.0)
    assert inl[0] == -1 and not P[0].any() and scales[0] == 0.0 and inl[1] >= 0 and rec["n_void"] == 1 and rec["best"] == 1
    P, inl, scales, rec = robust_ref.robust(np.full((5, 3), np.nan), dst[:5], None, 0.01, 3, 1.4, 0.0)
    assert inl[0] == -1 and not P.any() and rec == dict(n_poses=1, n_void=1, best=-1, best_inliers=-1)
    # ... with a given scale there is a start: no round yields anything, the identity stays with no inlier
    P, inl, scales, rec = robust_ref.robust(np.full((5, 3), np.nan), dst[:5], None, 0.01, 3, 1.4, 2.0)
    assert inl[0] == 0 and np.array_equal(P[0], np.concatenate([np.eye(3).ravel(), np.zeros(3)])) and scales[0] == 2.0
    assert rec == dict(n_poses=1, n_void=0, best=0, best_inliers=0)


def test_recovery_under_80_percent_wrong_matches():
    worst_angle = worst_shift = 0.0
    for seed, src, dst, good in recovery_cases():
        P, inl, scales, _ = robust_ref.robust(src, dst, None, 0.01, 64, 1.4, 0.0)
        angle, shift = pose_error(P[0])
        print(f"seed {seed}: {angle:.4f} degrees, |t - t_true| = {shift:.3e}, inliers {inl[0]} of {int(good.sum())} true matches, "
              f"final scale {scales[0]:.3e}")
        worst_angle, worst_shift = max(worst_angle, angle), max(worst_shift, shift)
        assert scales[0] == np.float64(0.01) * np.float64(0.01)
        assert int(inl[0]) == int(good.sum()) == 80                  # (noise of 0.002 a coordinate: no true match is 0.01 away)
    print(f"largest: {worst_angle:.4f} degrees, {worst_shift:.3e}")
    assert worst_angle <= RECOVERY_ANGLE_BOUND and worst_shift <= RECOVERY_SHIFT_BOUND


# ---- the plumbing on a stand-in context ----
class ChainOracleContext(oracle_backend.OracleContext):
    """The entry points of the chain, answered by the numpy references."""

    def fpfh(self, slot, normals, k, radius=np.inf, viewpoint=None, fpfh_ptr=None, counts_ptr=None, want_counts=False):
        self._log("fpfh")
        return fpfh_ref.fpfh(self.cloud[slot][0], normals, k, radius, viewpoint)["fpfh"], None, {}

    def feature_match(self, query, target, nq=None, nt=None, dim=None, idx_ptr=None, d2_ptr=None, want_d2=True):
        self._log("feature_match")
        return global_ref.match(query, target)

    def ransac_triplets(self, src, dst, triples, max_distance, edge_ratio, m=None, h=None, poses_ptr=None, inliers_ptr=None,
                        want_poses=True):
        self._log("ransac_triplets")
        return global_ref.ransac(src, dst, triples, max_distance, edge_ratio)


class RobustOracleContext(ChainOracleContext):
    """... and the robust fit's."""

    def pose_robust(self, src, dst, poses, max_distance, rounds, divisor, start_scale=0.0, m=None, b=None, poses_ptr=None,
                    inliers_ptr=None, scales_ptr=None):
        assert inliers_ptr is None and src.dtype == dst.dtype == np.float64
        self._log("pose_robust")
        self.robust_args = (np.array(src), np.array(dst), None if poses is None else np.array(poses), max_distance, rounds, divisor,
                            start_scale)
        return robust_ref.robust(src, dst, poses, max_distance, rounds, divisor, start_scale)


@pytest.fixture
def octx(monkeypatch):
    from simpleicp_amd import backend
    ctx = RobustOracleContext()
    monkeypatch.setattr(backend, "get_context", lambda: ctx)
    return ctx


def test_robust_pose(octx):
    import simpleicp_amd
    rng = np.random.default_rng(4)
    src, dst, _ = noisy_copy(rng, 120, 0.5)
    H, n = simpleicp_amd.robust_pose(src.astype(np.float32), dst, max_distance=0.01)
    s32 = src.astype(np.float32).astype(np.float64)
    assert octx.calls == ["pose_robust"] and np.array_equal(octx.robust_args[0], s32) and octx.robust_args[2] is None
    assert octx.robust_args[3:] == (0.01, 64, 1.4, 0.0)
    P, inl, _, _ = robust_ref.robust(s32, dst, None, 0.01, 64, 1.4, 0.0)
    assert H.shape == (4, 4) and isinstance(n, int) and n == inl[0] > 0
    assert np.array_equal(u64(H[:3, :3].ravel()), u64(P[0, :9])) and np.array_equal(u64(H[:3, 3]), u64(P[0, 9:]))
    assert np.array_equal(H[3], [0, 0, 0, 1])
    # one pose and a stack; the keywords arrive as given; a void pose comes back as zeros with -1
    Hs = np.tile(np.eye(4), (3, 1, 1))
    Hs[1, :3, :3], Hs[1, :3, 3] = R_TRUE, T_TRUE
    Hs[2, 1, 1] = np.nan
    out, n = simpleicp_amd.robust_pose(src, dst, max_distance=0.02, H=Hs, rounds=5, divisor=2.0, start_scale=3.0)
    assert octx.robust_args[3:] == (0.02, 5, 2.0, 3.0) and octx.robust_args[2].shape == (3, 12)
    assert np.array_equal(octx.robust_args[2][1], np.concatenate([R_TRUE.ravel(), T_TRUE]))
    rP, rn, _, _ = robust_ref.robust(src, dst, octx.robust_args[2], 0.02, 5, 2.0, 3.0)
    assert out.shape == (3, 4, 4) and n.dtype == np.int64 and np.array_equal(n, rn) and n[2] == -1 and not out[2].any()
    for k in (0, 1):
        assert np.array_equal(u64(out[k, :3, :3].ravel()), u64(rP[k, :9])) and np.array_equal(u64(out[k, :3, 3]), u64(rP[k, 9:]))
        assert np.array_equal(out[k, 3], [0, 0, 0, 1])
    one, n1 = simpleicp_amd.robust_pose(src, dst, max_distance=0.02, H=Hs[1], rounds=5, divisor=2.0, start_scale=3.0)
    assert one.shape == (4, 4) and isinstance(n1, int) and n1 == n[1] and np.array_equal(u64(one), u64(out[1]))
    nowhere = np.full_like(src, np.nan)
    H, n = simpleicp_amd.robust_pose(nowhere, dst, max_distance=0.02)
    assert n == -1 and H.shape == (4, 4) and not H.any()
    from simpleicp_amd import _lib
    octx.__class__ = oracle_backend.OracleContext                     # a backend without the entry point
    with pytest.raises(_lib.BackendError, match="robust pose"):
        simpleicp_amd.robust_pose(src, dst, max_distance=0.02)


@pytest.fixture(scope="module")
def surface_pair():
    """test_posefit_host's pair of samples of one surface."""
    rng = np.random.default_rng(8)
    g = np.linspace(-1, 1, 14)
    u, v = [a.ravel() for a in np.meshgrid(g, g)]
    fixed = np.column_stack([u, v, 0.3 * np.sin(3 * u) * np.cos(2 * v) + 0.2 * u * v]) + rng.normal(0, 1e-3, (196, 3))
    c, s = np.cos(0.5), np.sin(0.5)
    R, t = np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), np.array([0.5, 0.1, -0.4])
    movable = (fixed - t) @ R + rng.normal(0, 2e-3, (196, 3))
    kw = dict(max_distance=0.003, neighbors=12, normal_neighbors=8, viewpoint_fixed=(0, 0, 9),
              viewpoint_movable=tuple(R.T @ (np.array([0, 0, 9.0]) - t)))
    return fixed, movable, kw


def test_register_global_with_the_robust_method(octx, surface_pair):
    import simpleicp_amd
    fixed, movable, kw = surface_pair
    plain = simpleicp_amd.register_global(fixed, movable, hypotheses=50, seed=1, **kw)
    chain = [c for c in octx.calls if c != "ransac_triplets"]
    assert octx.calls[-1] == "ransac_triplets" and "pose_robust" not in octx.calls
    # method="ransac" is the default, call for call and byte for byte
    octx.calls.clear()
    same = simpleicp_amd.register_global(fixed, movable, hypotheses=50, seed=1, method="ransac", **kw)
    assert octx.calls == chain + ["ransac_triplets"] and same.stats == plain.stats and len(same.candidates) == len(plain.candidates) == 1
    assert same.H.tobytes() == plain.H.tobytes() and (same.inliers, same.index) == (plain.inliers, plain.index)
    octx.calls.clear()
    res = simpleicp_amd.register_global(fixed, movable, method="robust", rounds=30, divisor=1.5, **kw)
    assert octx.calls == chain + ["pose_robust"]
    src, dst, start = octx.robust_args[:3]
    assert start is None and octx.robust_args[3:] == (0.003, 30, 1.5, 0.0) and len(src) == len(dst) == res.n_matches == plain.n_matches
    assert set(map(bytes, src)) <= set(map(bytes, np.asarray(movable, np.float64))) and set(map(bytes, dst)) <= set(map(bytes, fixed))
    P, inl, _, rec = robust_ref.robust(src, dst, None, 0.003, 30, 1.5, 0.0)
    assert res.stats == rec and res.refined is None and len(res.candidates) == 1
    assert res.inliers == inl[0] and res.index == -1 and res.H is res.candidates[0][0]
    assert np.array_equal(u64(res.H[:3, :3].ravel()), u64(P[0, :9])) and np.array_equal(u64(res.H[:3, 3]), u64(P[0, 9:]))
    # a void fit: no candidate, the record says so
    octx.pose_robust = lambda s, d, p, *a, **k: (np.zeros((1, 12)), np.array([-1], np.int32), np.zeros(1),
                                                 dict(n_poses=1, n_void=1, best=-1, best_inliers=-1))
    res = simpleicp_amd.register_global(fixed, movable, method="robust", **kw)
    assert res.H is None and res.inliers == -1 and res.candidates == [] and res.stats["n_void"] == 1
    # fewer than three matches: the robust record, empty, and no fit
    octx.calls.clear()
    octx.feature_match = lambda q, t, **k: (np.full(len(q), -1, np.int32), np.full(len(q), np.inf, np.float32), {})
    few = simpleicp_amd.register_global(fixed, movable, method="robust", **kw)
    assert few.n_matches == 0 and few.stats == dict(n_poses=0, n_void=0, best=-1, best_inliers=-1) and few.H is None
    # a backend without the entry point
    from simpleicp_amd import _lib
    del octx.feature_match, octx.pose_robust
    octx.__class__ = ChainOracleContext
    with pytest.raises(_lib.BackendError, match="robust pose"):
        simpleicp_amd.register_global(fixed, movable, method="robust", **kw)
