"""Least-squares pose refit (contract (L)), the parts that need no GPU: the companion header and the binding,
the refusals that come before any device work, the numpy reference (tests/posefit_ref.py) against textbook Kabsch, its
properties, and the plumbing of fit_pose, refine_pose and register_global(refine=) on a stand-in context."""
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

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "simpleicp_hip_posefit.h"

# The largest |R - R_svd| and |t - t_svd| of the reference against np.linalg.svd Kabsch over kabsch_cases(), measured on the CPU
# (x86-64, numpy / OpenBLAS): 3.9e-15 and 4.8e-16, both on the noisy copy of 65 rows; DESIGN.md section 19.  The bounds are 100 x
# those: room for other LAPACK builds.
KABSCH_R_BOUND = 3.9e-13
KABSCH_T_BOUND = 4.8e-14


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def rotation(axis, angle):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


R_TRUE, T_TRUE = rotation([1.0, 2.0, 3.0], 0.7), np.array([0.3, -0.2, 0.1])


def noisy_copy(rng, m, wrong=0.4, noise=0.002):
    """test_gpu_global's noisy rigid copy, and the mask of the rows that stayed matches."""
    src = rng.uniform(-1, 1, (m, 3))
    dst = src @ R_TRUE.T + T_TRUE + rng.normal(0, noise, (m, 3))
    bad = rng.choice(m, int(wrong * m), replace=False)
    dst[bad] = rng.uniform(-1, 1, (len(bad), 3))
    good = np.ones(m, bool)
    good[bad] = False
    return src, dst, good


def perturbed(rng, b, degrees=3.0, shift=0.01):
    """(b, 12) poses: the true motion off by a few degrees and a little shift."""
    out = np.empty((b, 12))
    for k in range(b):
        R = rotation(rng.standard_normal(3), np.radians(degrees) * rng.uniform(0.2, 1.0)) @ R_TRUE
        out[k, :9], out[k, 9:] = R.ravel(), T_TRUE + rng.normal(0, shift, 3)
    return out


def kabsch_cases():
    """(name, src, dst, mask): the inlier sets the reference and Kabsch both fit."""
    cases = []
    for m in (3, 65, 1000):
        for noise in (0.0, 0.002):
            src, dst, good = noisy_copy(np.random.default_rng(10 * m + int(noise > 0)), m, 0.4 if m > 3 else 0.0, noise)
            cases.append((f"copy m={m} noise={noise}", src, dst, good))
    rng = np.random.default_rng(77)
    flat = np.column_stack([rng.uniform(-1, 1, (200, 2)), np.zeros(200)])
    cases.append(("planar", flat, flat @ R_TRUE.T + T_TRUE + rng.normal(0, 0.002, (200, 3)), np.ones(200, bool)))
    src = rng.uniform(-1, 1, (150, 3)) * (1.0, 0.7, 0.4)
    cases.append(("reflection", src, src * (1.0, 1.0, -1.0) + rng.normal(0, 0.002, (150, 3)), np.ones(150, bool)))
    return cases


# ---- header, exports, binding ----
def test_header_names_are_exported_and_bound():
    from simpleicp_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(sicp_\w+)\s*\(", text))) == sorted(_lib.POSEFIT_EXPORTS) == ["sicp_pose_refit", "sicp_posefit_version"]
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", str(so)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sicp_\w+)", out))
    assert set(_lib.POSEFIT_EXPORTS) <= exported
    others = (set(_lib.EXPORTS) | set(_lib.BATCH_EXPORTS) | set(_lib.DEVICE_EXPORTS) | set(_lib.NORMALS_EXPORTS) | set(_lib.VOXEL_EXPORTS)
              | set(_lib.EVAL_EXPORTS) | set(_lib.OUTLIER_EXPORTS) | set(_lib.CHAIN_EXPORTS) | set(_lib.FPFH_EXPORTS)
              | set(_lib.GLOBAL_EXPORTS))
    assert not set(_lib.POSEFIT_EXPORTS) & others
    L = _lib.load()
    head = HEADER.read_text()
    # the version triple: the header's, the library's, the binding's
    assert "#define SICP_POSEFIT_VERSION 1" in head
    assert L.sicp_posefit_version() == _lib.POSEFIT_VERSION == 1 and _lib.posefit_version() == 1
    assert f"#define SICP_POSEFIT_MAX_ROUNDS {_lib.POSEFIT_MAX_ROUNDS}" in head and _lib.POSEFIT_MAX_ROUNDS == 64
    assert f"#define SICP_POSEFIT_SWEEPS {_lib.POSEFIT_SWEEPS}" in head and _lib.POSEFIT_SWEEPS == posefit_ref.SWEEPS
    assert C.sizeof(_lib.PosefitStats) == 40
    assert _lib.FEATURES["posefit"].exports == _lib.POSEFIT_EXPORTS and _lib.FEATURES["posefit"].header == HEADER.name
    # the main header, its version and the other companions are untouched; the word stays where test_global_host.py wants it
    assert L.sicp_abi_version() == _lib.ABI_VERSION == 7 and L.sicp_global_version() == _lib.GLOBAL_VERSION == 1
    assert "ransac" not in head.lower()
    main = (ROOT / "include" / "simpleicp_hip.h").read_text().lower()
    assert "pose_refit" not in main and "posefit" not in main
    assert list(inspect.signature(_lib.Context.pose_refit).parameters)[1:] == [
        "src", "dst", "poses", "max_distance", "rounds", "m", "b", "poses_ptr", "inliers_ptr"]
    assert any(p.name == "sicp_posefit.hip" for p in build.SOURCES) and any(p.name == HEADER.name for p in build.HEADERS)


def test_null_ctx_is_refused_not_dereferenced():
    from simpleicp_amd import _lib
    L = _lib.load()
    P = _lib._ptr
    X, pose, out, inl, st = np.zeros((4, 3)), np.zeros((1, 12)), np.full((1, 12), 7.0), np.full(1, 7, np.int32), _lib.PosefitStats()
    assert L.sicp_pose_refit(None, P(X), P(X), 4, P(pose), 1, 1.0, 1, P(out), P(inl), C.byref(st)) == _lib.ERR_INVALID
    assert b"null ctx" in L.sicp_last_error() and np.all(inl == 7) and np.all(out == 7.0)


# ---- argument errors before the backend is touched ----
def test_python_argument_errors_come_before_the_backend(monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import backend

    def no_backend(*a, **k):
        raise AssertionError("the backend was called")
    monkeypatch.setattr(backend, "get_context", no_backend)
    for name in ("fit_pose", "refine_pose"):
        assert name in simpleicp_amd.__all__
    fp, rf, rg = simpleicp_amd.fit_pose, simpleicp_amd.refine_pose, simpleicp_amd.register_global
    assert list(inspect.signature(fp).parameters) == ["src", "dst"]
    assert list(inspect.signature(rf).parameters) == ["src", "dst", "H", "max_distance", "rounds"]
    assert all(p.kind == p.KEYWORD_ONLY for n, p in inspect.signature(rf).parameters.items() if n in ("max_distance", "rounds"))
    X, H = np.random.default_rng(0).standard_normal((10, 3)), np.eye(4)
    with pytest.raises(ValueError, match="same number"):
        fp(X, X[:9])
    with pytest.raises(ValueError, match="at least 3"):
        fp(X[:2], X[:2])
    with pytest.raises(ValueError, match=r"\(m, 3\)"):
        fp(X[:, :2], X[:, :2])
    for d in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_distance"):
            rf(X, X, H, max_distance=d)
    for d in ("far", None, True):
        with pytest.raises(TypeError, match="max_distance"):
            rf(X, X, H, max_distance=d)
    with pytest.raises(TypeError):
        rf(X, X, H)                                                   # max_distance has no default
    for r in (0, -1, 65):
        with pytest.raises(ValueError, match="rounds"):
            rf(X, X, H, max_distance=1.0, rounds=r)
    with pytest.raises(TypeError, match="rounds"):
        rf(X, X, H, max_distance=1.0, rounds=2.0)
    for bad in (np.eye(3), np.zeros((0, 4, 4)), np.zeros((2, 2, 4, 4)), np.zeros(16)):
        with pytest.raises(ValueError, match="H must"):
            rf(X, X, bad, max_distance=1.0)
    with pytest.raises(ValueError, match="same number"):
        rf(X, X[:9], H, max_distance=1.0)
    with pytest.raises(ValueError, match="at least 3"):
        rf(X[:2], X[:2], H, max_distance=1.0)
    for r in (-1, 65):
        with pytest.raises(ValueError, match="refine"):
            rg(X, X, max_distance=1.0, refine=r)
    for r in (1.0, True, "2"):
        with pytest.raises(TypeError, match="refine"):
            rg(X, X, max_distance=1.0, refine=r)
    with pytest.raises(TypeError, match="unexpected keyword"):
        rg(X, X, max_distance=1.0, refines=1)


def test_a_distributed_job_is_refused(monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import backend, dist
    monkeypatch.setattr(backend, "get_context", lambda: (_ for _ in ()).throw(AssertionError("the backend was called")))
    monkeypatch.setattr(dist, "is_distributed", lambda: True)
    X = np.random.default_rng(0).standard_normal((10, 3))
    for call in (lambda: simpleicp_amd.fit_pose(X, X), lambda: simpleicp_amd.refine_pose(X, X, np.eye(4), max_distance=1.0),
                 lambda: simpleicp_amd.register_global(X, X, max_distance=1.0, refine=2)):
        with pytest.raises(simpleicp_amd.SimpleICPException, match="does not run in a torch.distributed job"):
            call()


# ---- the reference alone ----
def test_reference_against_textbook_kabsch():
    worst_R = worst_t = 0.0
    for name, src, dst, mask in kabsch_cases():
        R, t = posefit_ref.fit_masked(src, dst, mask)
        Rs, ts = posefit_ref.kabsch(src[mask], dst[mask])
        dR, dt = np.abs(R - Rs).max(), np.abs(t - ts).max()
        print(f"{name}: |R - R_svd| = {dR:.3e}, |t - t_svd| = {dt:.3e}, det R = {np.linalg.det(R):.17g}")
        worst_R, worst_t = max(worst_R, dR), max(worst_t, dt)
        assert abs(np.linalg.det(R) - 1.0) < 1e-14 and np.abs(R @ R.T - np.eye(3)).max() < 1e-14
    print(f"largest: |R - R_svd| = {worst_R:.3e}, |t - t_svd| = {worst_t:.3e}")
    assert worst_R <= KABSCH_R_BOUND and worst_t <= KABSCH_T_BOUND


def test_reference_known_answers():
    # noise-free matches: the true motion comes back to rounding, every row an inlier at a tiny distance
    src, dst, _ = noisy_copy(np.random.default_rng(1), 50, 0.0, 0.0)
    P, inl, rec = posefit_ref.refit(src, dst, None, np.inf, 1)
    assert np.abs(P[0, :9].reshape(3, 3) - R_TRUE).max() < 1e-14 and np.abs(P[0, 9:] - T_TRUE).max() < 1e-14
    assert inl.tolist() == [50] and rec == dict(n_poses=1, n_void=0, n_improved=1, best=0, best_inliers=50)
    # fewer than three finite rows: no pose
    bad = src.copy()
    bad[2:, 0] = np.nan
    P, inl, rec = posefit_ref.refit(bad, dst, None, np.inf, 1)
    assert inl.tolist() == [-1] and not P.any() and rec == dict(n_poses=1, n_void=0, n_improved=0, best=-1, best_inliers=-1)
    # a void pose, a pose without inliers (it stays, with its count), a good one; ties in the record go to the lower index
    good = np.concatenate([R_TRUE.ravel(), T_TRUE])
    void = good.copy()
    void[4] = np.inf
    off = np.concatenate([np.eye(3).ravel(), [50.0, 0.0, 0.0]])
    P, inl, rec = posefit_ref.refit(src, dst, np.stack([void, off, np.zeros(12), good, good]), 0.01, 3)
    assert inl.tolist() == [-1, 0, 0, 50, 50] and not P[0].any() and np.array_equal(u64(P[1]), u64(off)) and not P[2].any()
    assert np.array_equal(u64(P[3]), u64(good)) and rec == dict(n_poses=5, n_void=1, n_improved=0, best=3, best_inliers=50)
    # georeferenced rows -- coordinates of 1e6, an extent of 100 -- lose nothing to cancellation: the rows themselves are good to
    # 1.2e-10 (half an ulp at 1e6) over lever arms of tens, a few 1e-12 rad; sums of uncentred products would be off by
    # 1e12 * 2.2e-16 = 2e-4.  1e-9 tells the two apart.
    far = np.random.default_rng(3).uniform(-50, 50, (500, 3)) + 1e6
    P, inl, _ = posefit_ref.refit(far, far @ R_TRUE.T + T_TRUE, None, np.inf, 1)
    assert inl[0] == 500 and np.abs(P[0, :9].reshape(3, 3) - R_TRUE).max() < 1e-9
    # q and -q are the same rotation, bit for bit
    quat = np.array([0.3, -0.5, 0.1, 0.8])
    assert np.array_equal(u64(posefit_ref.rotation(quat)), u64(posefit_ref.rotation(-quat)))


def test_the_sweep_count_is_one_past_convergence():
    """on these inputs the quaternion's bits are final after at most five sweeps; SWEEPS is that plus one."""
    need = 0
    for name, src, dst, mask in kabsch_cases():
        quats = [posefit_ref.fit_masked(src, dst, mask, sweeps=s, want_quat=True) for s in range(1, posefit_ref.SWEEPS + 4)]
        settled = next(s for s in range(1, len(quats)) if all(np.array_equal(u64(quats[s - 1]), u64(q)) for q in quats[s:]))
        print(f"{name}: the quaternion is final after {settled} sweeps")
        need = max(need, settled)
    assert need + 1 == posefit_ref.SWEEPS


def test_inliers_never_drop():
    for seed, (m, b, rounds, dist) in enumerate([(65, 20, 1, 0.02), (300, 40, 3, 0.02), (300, 20, 5, 0.005), (1000, 10, 2, np.inf)]):
        rng = np.random.default_rng(seed)
        src, dst, _ = noisy_copy(rng, m)
        poses = perturbed(rng, b, degrees=1.0, shift=0.004)
        with np.errstate(all="ignore"):
            before = global_ref.count_inliers(poses[:, :9].reshape(-1, 3, 3), poses[:, 9:], src, dst, dist) if np.isfinite(dist) else \
                np.full(b, m)
        P, inl, rec = posefit_ref.refit(src, dst, poses, dist, rounds)
        assert np.all(inl >= before) and rec["n_improved"] == int((inl > before).sum()) and rec["best_inliers"] == inl.max()
        same = inl == before
        assert np.array_equal(u64(P[same]), u64(poses[same]))           # (a pose that was not beaten leaves as it came)
        if np.isfinite(dist):
            assert rec["n_improved"] > 0
            after = global_ref.count_inliers(P[:, :9].reshape(-1, 3, 3), P[:, 9:], src, dst, dist)
            assert np.array_equal(after, inl)


# ---- the plumbing on a stand-in context ----
class PosefitOracleContext(oracle_backend.OracleContext):
    """The entry points of the chain and of the refit, answered by the numpy references."""

    def fpfh(self, slot, normals, k, radius=np.inf, viewpoint=None, fpfh_ptr=None, counts_ptr=None, want_counts=False):
        self._log("fpfh")
        return fpfh_ref.fpfh(self.cloud[slot][0], normals, k, radius, viewpoint)["fpfh"], None, {}

    def feature_match(self, query, target, nq=None, nt=None, dim=None, idx_ptr=None, d2_ptr=None, want_d2=True):
        self._log("feature_match")
        return global_ref.match(query, target)

    def ransac_triplets(self, src, dst, triples, max_distance, edge_ratio, m=None, h=None, poses_ptr=None, inliers_ptr=None,
                        want_poses=True):
        assert inliers_ptr is None
        self._log("ransac_triplets")
        self.ransac_args = (np.array(src), np.array(dst), np.array(triples), max_distance, edge_ratio)
        return global_ref.ransac(src, dst, triples, max_distance, edge_ratio)

    def pose_refit(self, src, dst, poses, max_distance, rounds, m=None, b=None, poses_ptr=None, inliers_ptr=None):
        assert inliers_ptr is None and src.dtype == dst.dtype == np.float64
        self._log("pose_refit")
        self.refit_args = (np.array(src), np.array(dst), None if poses is None else np.array(poses), max_distance, rounds)
        return posefit_ref.refit(src, dst, poses, max_distance, rounds)


@pytest.fixture
def octx(monkeypatch):
    from simpleicp_amd import backend
    ctx = PosefitOracleContext()
    monkeypatch.setattr(backend, "get_context", lambda: ctx)
    return ctx


def test_fit_pose_and_refine_pose(octx):
    import simpleicp_amd
    rng = np.random.default_rng(4)
    src, dst, _ = noisy_copy(rng, 120, 0.3)
    H = simpleicp_amd.fit_pose(src.astype(np.float32), dst)
    s32 = src.astype(np.float32).astype(np.float64)
    assert octx.calls == ["pose_refit"] and np.array_equal(octx.refit_args[0], s32) and octx.refit_args[2] is None
    assert octx.refit_args[3:] == (np.inf, 1)
    P, inl, _ = posefit_ref.refit(s32, dst, None, np.inf, 1)
    assert H.shape == (4, 4) and np.array_equal(u64(H[:3, :3].ravel()), u64(P[0, :9])) and np.array_equal(u64(H[:3, 3]), u64(P[0, 9:]))
    assert np.array_equal(H[3], [0, 0, 0, 1])
    nowhere = src.copy()
    nowhere[1:] = np.nan
    assert simpleicp_amd.fit_pose(nowhere, dst) is None
    # one pose and a stack; rounds and the distance arrive as given; a void pose comes back as zeros with -1
    poses = perturbed(rng, 4)
    Hs = np.tile(np.eye(4), (4, 1, 1))
    Hs[:, :3, :3], Hs[:, :3, 3] = poses[:, :9].reshape(-1, 3, 3), poses[:, 9:]
    Hs[2, 1, 1] = np.nan
    out, n = simpleicp_amd.refine_pose(src, dst, Hs, max_distance=0.02, rounds=2)
    assert octx.refit_args[3:] == (0.02, 2) and octx.refit_args[2].shape == (4, 12)
    rP, rn, _ = posefit_ref.refit(src, dst, octx.refit_args[2], 0.02, 2)
    assert out.shape == (4, 4, 4) and n.dtype == np.int64 and np.array_equal(n, rn) and n[2] == -1 and not out[2].any()
    for k in (0, 1, 3):
        assert np.array_equal(u64(out[k, :3, :3].ravel()), u64(rP[k, :9])) and np.array_equal(u64(out[k, :3, 3]), u64(rP[k, 9:]))
        assert np.array_equal(out[k, 3], [0, 0, 0, 1])
    one, n1 = simpleicp_amd.refine_pose(src, dst, Hs[0], max_distance=0.02, rounds=2)
    assert one.shape == (4, 4) and isinstance(n1, int) and n1 == n[0] and np.array_equal(u64(one), u64(out[0]))
    assert simpleicp_amd.refine_pose(src, dst, Hs[0], max_distance=np.inf)[1] == 120 and octx.refit_args[3:] == (np.inf, 3)
    from simpleicp_amd import _lib, backend
    octx.__class__ = oracle_backend.OracleContext                     # a backend without the entry point
    with pytest.raises(_lib.BackendError, match="pose refit"):
        simpleicp_amd.fit_pose(src, dst)


@pytest.fixture(scope="module")
def surface_pair():
    rng = np.random.default_rng(8)
    g = np.linspace(-1, 1, 14)
    u, v = [a.ravel() for a in np.meshgrid(g, g)]
    fixed = np.column_stack([u, v, 0.3 * np.sin(3 * u) * np.cos(2 * v) + 0.2 * u * v]) + rng.normal(0, 1e-3, (196, 3))
    c, s = np.cos(0.5), np.sin(0.5)
    R, t = np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), np.array([0.5, 0.1, -0.4])
    movable = (fixed - t) @ R + rng.normal(0, 2e-3, (196, 3))       # (noise of its own: a triple's pose is no longer exact)
    kw = dict(max_distance=0.003, neighbors=12, normal_neighbors=8, viewpoint_fixed=(0, 0, 9),
              viewpoint_movable=tuple(R.T @ (np.array([0, 0, 9.0]) - t)), hypotheses=200, seed=1, top=5)
    return fixed, movable, kw


def test_refine_0_changes_nothing(octx, surface_pair):
    import simpleicp_amd
    fixed, movable, kw = surface_pair
    plain = simpleicp_amd.register_global(fixed, movable, **kw)
    calls = list(octx.calls)
    octx.calls.clear()
    zero = simpleicp_amd.register_global(fixed, movable, refine=0, **kw)
    assert octx.calls == calls and "pose_refit" not in calls and plain.refined is None and zero.refined is None
    assert zero.stats == plain.stats and zero.n_matches == plain.n_matches and len(zero.candidates) == len(plain.candidates) > 1
    for (Ha, na, ka), (Hb, nb, kb) in zip(plain.candidates, zero.candidates):
        assert Ha.tobytes() == Hb.tobytes() and (na, ka) == (nb, kb)
    # ransac_pose itself: what contract (R) says, byte for byte, and no refit
    src, dst, tri = octx.ransac_args[:3]
    octx.calls.clear()
    res = simpleicp_amd.ransac_pose(src, dst, max_distance=0.003, triples=tri, top=5)
    assert octx.calls == ["ransac_triplets"] and res.refined is None
    P, inl, rec = global_ref.ransac(src, dst, tri, 0.003, 0.9)
    order = sorted(np.flatnonzero(inl >= 0), key=lambda k: (-inl[k], k))[:5]
    assert res.stats == rec and [c[2] for c in res.candidates] == order
    for (H, n, k), (Hb, nb, kb) in zip(res.candidates, plain.candidates):
        assert H.tobytes() == Hb.tobytes() and (n, k) == (nb, kb) and np.array_equal(u64(H[:3, :3].ravel()), u64(P[k, :9]))


def test_refine_2_reorders_the_candidates(octx, surface_pair):
    import simpleicp_amd
    fixed, movable, kw = surface_pair
    plain = simpleicp_amd.register_global(fixed, movable, **kw)
    octx.calls.clear()
    res = simpleicp_amd.register_global(fixed, movable, refine=2, **kw)
    assert octx.calls[-2:] == ["ransac_triplets", "pose_refit"] and octx.calls.count("pose_refit") == 1
    src, dst = octx.ransac_args[:2]
    poses = np.array([np.concatenate([H[:3, :3].ravel(), H[:3, 3]]) for H, _, _ in plain.candidates])
    assert np.array_equal(octx.refit_args[0], src) and np.array_equal(octx.refit_args[1], dst)
    assert np.array_equal(u64(octx.refit_args[2]), u64(poses)) and octx.refit_args[3:] == (0.003, 2)
    rP, rn, rec = posefit_ref.refit(src, dst, poses, 0.003, 2)
    index = np.array([k for _, _, k in plain.candidates])
    before = np.array([n for _, n, _ in plain.candidates])
    assert np.all(rn >= before) and rec["n_improved"] > 0
    order = np.lexsort((index, -rn.astype(np.int64)))
    print(f"counts {before.tolist()} -> {rn.tolist()}, order {index.tolist()} -> {index[order].tolist()}")
    assert order.tolist() != list(range(len(order)))                  # (the refit changes the ranking on this pair)
    assert res.stats == plain.stats and res.n_matches == plain.n_matches and res.refined == rec
    assert [c[2] for c in res.candidates] == index[order].tolist() and [c[1] for c in res.candidates] == rn[order].tolist()
    for (H, _, _), j in zip(res.candidates, order):
        assert np.array_equal(u64(H[:3, :3].ravel()), u64(rP[j, :9])) and np.array_equal(u64(H[:3, 3]), u64(rP[j, 9:]))
    assert res.H is res.candidates[0][0] and res.inliers == rn.max() and res.index == index[order][0]
    # the order is by (-inliers, index) whatever the refit returns: equal counts fall back on the triple's row
    octx.pose_refit = lambda s, d, p, md, r, **k: (p, np.array([7, 9, 7, 9, 7], np.int32)[:len(p)], dict(rec))
    tied = simpleicp_amd.register_global(fixed, movable, refine=1, **kw)
    want = sorted(range(len(index)), key=lambda j: (-[7, 9, 7, 9, 7][j], index[j]))
    assert [c[2] for c in tied.candidates] == index[want].tolist()
