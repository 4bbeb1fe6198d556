"""ISS keypoints (contract (I)), the parts that need no GPU: the companion header and the binding, the refusals
that come before any device work, the reference (tests/iss_ref.py) pinned to the oracle and on known answers, its repeatability
on the bundled bunny pair, and the plumbing of keypoint_keep, PointCloud.select_keypoints and register_global(keypoints=...) on a
stand-in context."""
import ctypes as C
import inspect
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import eval_ref
import iss_ref
import oracle_backend
from oracle import orc
from test_robust_host import RobustOracleContext, surface_pair   # noqa: F401  (surface_pair: a fixture)

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "simpleicp_hip_keypoints.h"

# Repeatability on the bunny pair of tests/test_gpu_global.py (1 500 points a cloud, max_distance 10 000) at neighbors=32,
# nms_neighbors=6, the other keywords at their defaults, measured with tests/iss_ref.py on the CPU (x86-64, numpy): 165 fixed and
# 149 movable keypoints, 131 of the 149 (0.879) with a fixed keypoint within max_distance under the true motion.  DESIGN.md
# section 22.  The test asserts half of the measured share: room for other libm and BLAS builds.
BUNNY_KEYWORDS = dict(neighbors=32, nms_neighbors=6)
BUNNY_MEASURED_SHARE = 0.879
EXTENT = 263_800.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def record(r):
    return {key: r[key] for key in iss_ref.KEYS}


def lattice(n, dims=3):
    g = np.arange(n, dtype=np.float64)
    return np.ascontiguousarray(np.stack(np.meshgrid(*([g] * dims), indexing="ij"), -1).reshape(-1, dims))


# ---- header, exports, binding ----
def test_header_names_are_exported_and_bound():
    from simpleicp_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(sicp_\w+)\s*\(", text))) == sorted(_lib.KEYPOINTS_EXPORTS) == ["sicp_keypoints", "sicp_keypoints_version"]
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", str(so)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sicp_\w+)", out))
    assert set(_lib.KEYPOINTS_EXPORTS) <= exported
    others = set(_lib.EXPORTS)
    for name, f in _lib.FEATURES.items():
        if name != "keypoints":
            others |= set(f.exports)
    assert not set(_lib.KEYPOINTS_EXPORTS) & others and _lib.FEATURES["keypoints"].exports == _lib.KEYPOINTS_EXPORTS
    L = _lib.load()
    # the version triple: the header's, the library's, the binding's
    assert "#define SICP_KEYPOINTS_VERSION 1" in HEADER.read_text()
    assert L.sicp_keypoints_version() == _lib.KEYPOINTS_VERSION == 1 and _lib.keypoints_version() == 1
    assert f"#define SICP_KEYPOINT_MAX_K {_lib.KEYPOINTS_MAX_K}" in HEADER.read_text() and _lib.KEYPOINTS_MAX_K == _lib.OUTLIER_MAX_K
    assert C.sizeof(_lib.KeypointStats) == 48 and [n for n, _ in _lib.KeypointStats._fields_] == list(iss_ref.KEYS)
    # the main header and its version are untouched, the other companions keep theirs
    assert L.sicp_abi_version() == _lib.ABI_VERSION == 7
    assert "keypoint" not in (ROOT / "include" / "simpleicp_hip.h").read_text().lower()
    assert (_lib.BATCH_VERSION, _lib.DEVICE_VERSION, _lib.NORMALS_VERSION, _lib.VOXEL_VERSION, _lib.EVAL_VERSION, _lib.OUTLIER_VERSION,
            _lib.CHAIN_VERSION, _lib.FPFH_VERSION, _lib.GLOBAL_VERSION, _lib.POSEFIT_VERSION, _lib.ROBUST_VERSION,
            _lib.CONSISTENCY_VERSION) == (1,) * 12
    assert list(inspect.signature(_lib.Context.keypoints).parameters)[1:] == [
        "slot", "k_s", "salient_radius", "k_n", "nms_radius", "gamma21", "gamma32", "min_neighbors", "keep_ptr", "saliency_ptr", "eig_ptr",
        "want_saliency"]
    assert any(p.name == "sicp_keypoints.hip" for p in build.SOURCES) and any(p.name == "simpleicp_hip_keypoints.h" for p in build.HEADERS)
    # one text of the eigen-solve: the unit includes the normals' header and defines no jacobi of its own
    unit = (ROOT / "simpleicp_amd" / "csrc" / "sicp_keypoints.hip").read_text()
    assert '#include "sicp_normals.h"' in unit and not re.search(r"\bvoid\s+jacobi", unit)


def test_null_ctx_is_refused_not_dereferenced():
    from simpleicp_amd import _lib
    L = _lib.load()
    st = _lib.KeypointStats()
    keep = np.zeros(8, np.uint8)
    rc = L.sicp_keypoints(None, 0, 4, 1.0, 4, 1.0, 0.975, 0.975, 5, _lib._ptr(keep), None, None, C.byref(st))
    assert rc == _lib.ERR_INVALID and b"null ctx" in L.sicp_last_error()
    assert not keep.any()


# ---- argument errors before the backend is touched ----
def test_python_argument_errors_come_before_the_backend(monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import PointCloud, backend
    from simpleicp_amd.pointcloud import PointCloudException

    def no_backend(*a, **k):
        raise AssertionError("the backend was called")
    monkeypatch.setattr(backend, "get_context", no_backend)
    X = np.random.default_rng(0).standard_normal((50, 3))
    f = simpleicp_amd.keypoint_keep
    assert "keypoint_keep" in simpleicp_amd.__all__
    sig = inspect.signature(f).parameters
    assert list(sig) == ["X", "neighbors", "salient_radius", "nms_neighbors", "nms_radius", "gamma21", "gamma32", "min_neighbors",
                         "return_saliency"]
    assert all(p.kind is p.KEYWORD_ONLY for n, p in sig.items() if n != "X")
    assert {n: p.default for n, p in sig.items() if n != "X"} == dict(iss_ref.DEFAULTS, return_saliency=False)
    for name in ("neighbors", "nms_neighbors"):
        for k in (1, 0, -3, 129):
            with pytest.raises(ValueError, match=name):
                f(X, **{name: k})
        for k in (2.5, 20.0, "many", True, [20]):
            with pytest.raises(TypeError, match=name):
                f(X, **{name: k})
        with pytest.raises(ValueError, match=name + r" .* exceeds"):
            f(X, **{"neighbors": 8, name: 51})
    with pytest.raises(TypeError, match="neighbors"):
        f(X, neighbors=None)
    for name in ("salient_radius", "nms_radius"):
        for r in (0.0, -1.0, float("nan"), -float("inf")):
            with pytest.raises(ValueError, match=name):
                f(X, **{name: r})
        for r in ("wide", True, [1.0]):
            with pytest.raises(TypeError, match=name):
                f(X, **{name: r})
    for name in ("gamma21", "gamma32"):
        for g in (0.0, -0.5, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=name):
                f(X, **{name: g})
        for g in ("most", None, False):
            with pytest.raises(TypeError, match=name):
                f(X, **{name: g})
    for m in (0, -1):
        with pytest.raises(ValueError, match="min_neighbors"):
            f(X, min_neighbors=m)
    for m in (5.0, "five", True, None):
        with pytest.raises(TypeError, match="min_neighbors"):
            f(X, min_neighbors=m)
    with pytest.raises(TypeError, match="return_saliency"):
        f(X, return_saliency=1)
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        f(np.zeros((50, 2)))
    pc = PointCloud(X, columns=["x", "y", "z"])
    with pytest.raises(PointCloudException, match="neighbors"):
        pc.select_keypoints(1)
    with pytest.raises(PointCloudException, match="exceeds"):
        pc.select_keypoints(51)
    # an empty cloud has an empty answer and needs no backend
    e = f(np.zeros((0, 3)))
    assert e.shape == (0,) and e.dtype == bool
    e, s, w, st = f(np.zeros((0, 3)), return_saliency=True)
    assert e.shape == (0,) and s.shape == (0,) and w.shape == (0, 3) and st == dict.fromkeys(iss_ref.KEYS, 0)
    # register_global: the keyword's own errors, under both methods
    for method in ({}, {"method": "robust"}):
        for bad in (False, 1, "yes", [32]):
            with pytest.raises(TypeError, match="keypoints"):
                simpleicp_amd.register_global(X, X, max_distance=1.0, keypoints=bad, **method)
        with pytest.raises(TypeError, match="radius"):
            simpleicp_amd.register_global(X, X, max_distance=1.0, keypoints=dict(radius=1.0), **method)
        with pytest.raises(TypeError, match="return_saliency"):
            simpleicp_amd.register_global(X, X, max_distance=1.0, keypoints=dict(return_saliency=True), **method)
        with pytest.raises(ValueError, match="gamma21"):
            simpleicp_amd.register_global(X, X, max_distance=1.0, keypoints=dict(gamma21=0.0), **method)


def test_a_distributed_job_is_refused(monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import backend, dist
    from simpleicp_amd.icp import SimpleICPException
    monkeypatch.setattr(dist, "is_distributed", lambda: True)
    monkeypatch.setattr(backend, "get_context", lambda: (_ for _ in ()).throw(AssertionError("the backend was called")))
    with pytest.raises(SimpleICPException, match="keypoint_keep does not run in a torch.distributed job"):
        simpleicp_amd.keypoint_keep(np.random.default_rng(0).standard_normal((50, 3)))


# ---- the reference pinned to the oracle ----
def test_the_tree_over_rows_is_eval_refs_tree():
    rng = np.random.default_rng(3)
    for k in (2, 3, 8, 27, 64, 65, 128):
        t = rng.standard_normal((20, k)) * 10.0 ** rng.integers(-8, 8, (20, k))
        assert np.array_equal(bits(iss_ref.tree_rows(t)), bits([eval_ref.tree_sum(row) for row in t]))


def test_jacobi3_reproduces_the_oracles_planarity_bit_for_bit():
    # 500 seeded neighbourhoods of 8 points with small integer coordinates: the mean (a division by 8), the differences, their
    # products and the sums are exact, so the covariance orc_normals forms with fma is the one numpy forms without; the one
    # rounded operation is the multiplication by 1.0 / 7.0
    rng = np.random.default_rng(500)
    P = rng.integers(-50, 50, (500, 8, 3)).astype(np.float64)
    mean = P.sum(axis=1) / 8.0
    d = P - mean[:, None, :]
    inv = 1.0 / 7.0
    C6 = np.stack([(d[:, :, a] * d[:, :, b]).sum(axis=1) * inv for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))], axis=1)
    w = iss_ref.jacobi3(C6)
    e1, e2, e3 = iss_ref.sorted3(w)
    _, pl = orc.normals(P.reshape(-1, 3), np.arange(4000, dtype=np.int64).reshape(500, 8))
    assert np.array_equal(((e2 - e3) / e1).astype(np.float32).view(np.uint32), pl.view(np.uint32))
    # ... and they are the eigenvalues
    full = np.zeros((500, 3, 3))
    for c, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        full[:, a, b] = full[:, b, a] = C6[:, c]
    lam = np.linalg.eigvalsh(full)
    assert np.all(np.abs(np.stack([e3, e2, e1], axis=1) - lam) <= 1e-12 * lam[:, 2:3])


# ---- known answers on the reference alone ----
def test_flat_and_collinear_sets_have_no_salient_point():
    flat = np.column_stack([lattice(8, 2), np.zeros(64)])
    r = iss_ref.keypoints(flat, neighbors=9, min_neighbors=3)
    assert np.all(r["eig"][:, 2] == 0.0) and r["n_salient"] == 0 and r["n_keypoints"] == 0 and not r["keep"].any()
    assert not r["saliency"].any() and r["n_small"] == 0
    line = np.column_stack([np.arange(40.0), 2.0 * np.arange(40.0), np.zeros(40)])
    r = iss_ref.keypoints(line, neighbors=5, min_neighbors=3)
    assert r["n_salient"] == 0 and not r["keep"].any()


def test_the_interior_of_an_integer_lattice_is_a_ball():
    X = lattice(6)
    inner = np.flatnonzero(((X > 0) & (X < 5)).all(axis=1))
    idx, d2 = orc.knn(X, X[inner], k=27)
    assert len(inner) == 64 and np.array_equal(np.sort(d2, axis=1)[0], [0.0] + [1.0] * 6 + [2.0] * 12 + [3.0] * 8)
    for gamma in (1.0, 0.975, 0.5):
        r = iss_ref.keypoints(X, neighbors=27, gamma21=gamma, gamma32=gamma, min_neighbors=5)
        e = r["eig"][inner]
        assert np.all(e[:, 0] == e[:, 1]) and np.all(e[:, 1] == e[:, 2]) and np.all(e[:, 0] == 18.0 / 27.0)
        assert not r["saliency"][inner].any() and not r["keep"][inner].any()


def test_of_two_exact_duplicate_maxima_the_lower_index_stays():
    rng = np.random.default_rng(12)
    X = rng.uniform(0, 1, (300, 3))
    base = iss_ref.keypoints(X, neighbors=12, nms_neighbors=6)
    top = int(np.argmax(base["saliency"]))
    assert base["keep"][top]
    # an exact copy of every point: each pair of twins has the same support, hence the same saliency bits
    XX = np.concatenate([X, X])
    r = iss_ref.keypoints(XX, neighbors=24, nms_neighbors=12)
    assert np.array_equal(bits(r["saliency"][:300]), bits(r["saliency"][300:])) and r["n_salient"] > 0
    assert r["keep"][:300].any() and not r["keep"][300:].any()
    both = np.flatnonzero(r["saliency"][:300] > 0)
    assert set(np.flatnonzero(r["keep"])) <= set(both)


def test_a_radius_equal_to_a_neighbours_distance_is_strict():
    X = lattice(5)
    centre = 62
    r = iss_ref.keypoints(X, neighbors=40, salient_radius=2.0, min_neighbors=27)
    # the centre's 40 nearest: itself, 6 at d2 = 1, 12 at 2, 8 at 3, 6 at 4, ...: within 2.0, strictly: the first 27 -- the
    # 3 x 3 x 3 block, which the 27 points off the faces have whole
    assert r["n_small"] == 125 - 27 and r["n_clipped_salient"] == 0 and np.all(r["eig"][centre] == 18.0 / 27.0)
    r = iss_ref.keypoints(X, neighbors=40, salient_radius=np.nextafter(2.0, 3.0), min_neighbors=33)
    assert r["n_small"] == 124 and r["eig"][centre, 0] > 18.0 / 27.0
    r = iss_ref.keypoints(X, neighbors=7, salient_radius=1.0, min_neighbors=1)     # d2 = 1 < 1 * 1 fails: everybody is alone
    assert not r["eig"].any() and r["n_salient"] == 0 and r["n_small"] == 0
    r = iss_ref.keypoints(X, neighbors=7, salient_radius=1.2, min_neighbors=1)
    assert r["n_clipped_salient"] == 27            # the points off the faces: their seventh is still inside, k may hide an eighth


def test_translation_by_integers_leaves_every_bit():
    rng = np.random.default_rng(11)
    X = rng.integers(-20, 20, (400, 3)).astype(np.float64)
    # every support holds 16 points: sums of integers and their division by 16 are exact, so the centred differences are the same
    # numbers before and after (with another m the rounded mean, and with it every bit below, depends on where the cloud lies)
    kw = dict(neighbors=16, nms_neighbors=7, nms_radius=5.0)
    a = iss_ref.keypoints(X, **kw)
    b = iss_ref.keypoints(X + np.array([1000.0, -3000.0, 77.0]), **kw)
    assert np.array_equal(a["keep"], b["keep"]) and np.array_equal(bits(a["saliency"]), bits(b["saliency"]))
    assert np.array_equal(bits(a["eig"]), bits(b["eig"])) and record(a) == record(b) and a["n_keypoints"] > 0


def test_the_reference_takes_70_000_points_in_seconds():
    import time
    X = np.random.default_rng(70).uniform(-5, 5, (70_000, 3))
    t0 = time.perf_counter()
    r = iss_ref.keypoints(X, neighbors=8, min_neighbors=3)
    assert 0 < r["n_keypoints"] < r["n_salient"] <= 70_000
    print(f"70 000 points: {time.perf_counter() - t0:.1f} s, {record(r)}")


# ---- repeatability on the bunny pair ----
def bunny_pair():
    X = np.load(os.path.join(os.path.dirname(__file__), "golden", "data", "bunny_part1.npz"))["q"].astype(np.float64)
    perm = np.random.default_rng(1).permutation(len(X))
    A = np.ascontiguousarray(X[perm[:1500]])
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * K @ K
    t = np.array([0.05, -0.02, 0.1]) * EXTENT
    return A, np.ascontiguousarray(X[perm[1500:3000]] @ R.T + t), R, t


def test_keypoints_repeat_between_the_two_bunny_clouds():
    A, B, R, t = bunny_pair()
    ra, rb = iss_ref.keypoints(A, **BUNNY_KEYWORDS), iss_ref.keypoints(B, **BUNNY_KEYWORDS)
    assert 100 <= ra["n_keypoints"] <= 600 and 100 <= rb["n_keypoints"] <= 600
    back = (B[rb["keep"]] - t) @ R                                     # the movable keypoints under the true motion
    _, d2 = orc.knn(A[ra["keep"]], np.ascontiguousarray(back), k=1)
    share = float((d2[:, 0] < 10_000.0 ** 2).mean())
    print(f"{ra['n_keypoints']} fixed and {rb['n_keypoints']} movable keypoints, share repeated within max_distance: {share:.3f}")
    assert share >= 0.5 * BUNNY_MEASURED_SHARE


# ---- the plumbing on a stand-in context ----
class KeypointOracleContext(RobustOracleContext):
    """The chain's entry points answered by the numpy references, and the keypoints'."""

    def keypoints(self, slot, k_s, salient_radius=np.inf, k_n=None, nms_radius=np.inf, gamma21=0.975, gamma32=0.975, min_neighbors=5,
                  keep_ptr=None, saliency_ptr=None, eig_ptr=None, want_saliency=False):
        assert keep_ptr is None and saliency_ptr is None and eig_ptr is None
        self._log("keypoints")
        self.keypoint_args = (k_s, salient_radius, k_n, nms_radius, gamma21, gamma32, min_neighbors)
        r = iss_ref.keypoints(self.cloud[slot][0], k_s, salient_radius, k_n, nms_radius, gamma21, gamma32, min_neighbors)
        return r["keep"], (r["saliency"] if want_saliency else None), (r["eig"] if want_saliency else None), record(r)

    def ransac_triplets(self, src, dst, triples, max_distance, edge_ratio, **kw):
        self.ransac_rows = (np.array(src), np.array(dst))
        return super().ransac_triplets(src, dst, triples, max_distance, edge_ratio, **kw)


@pytest.fixture
def octx(monkeypatch):
    from simpleicp_amd import backend
    ctx = KeypointOracleContext()
    monkeypatch.setattr(backend, "get_context", lambda: ctx)
    return ctx


def test_keypoint_keep_and_select_keypoints_on_host_clouds(octx, monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import PointCloud, _lib, backend
    X = np.random.default_rng(4).uniform(0, 1, (300, 3))
    keep = simpleicp_amd.keypoint_keep(X, neighbors=12)
    ref = iss_ref.keypoints(X, neighbors=12)
    assert octx.calls == ["upload", "keypoints"] and keep.dtype == bool and np.array_equal(keep, ref["keep"]) and keep.any()
    assert octx.keypoint_args == (12, np.inf, 12, np.inf, 0.975, 0.975, 5)            # None: neighbors, +inf
    keep, sal, eig, st = simpleicp_amd.keypoint_keep(X.astype(np.float32), neighbors=12, salient_radius=0.3, nms_neighbors=6, nms_radius=0.2,
                                                     gamma21=0.9, gamma32=0.8, min_neighbors=4, return_saliency=True)
    assert octx.keypoint_args == (12, 0.3, 6, 0.2, 0.9, 0.8, 4)
    ref = iss_ref.keypoints(X.astype(np.float32).astype(np.float64), 12, 0.3, 6, 0.2, 0.9, 0.8, 4)
    assert np.array_equal(keep, ref["keep"]) and np.array_equal(bits(sal), bits(ref["saliency"])) and np.array_equal(bits(eig), bits(ref["eig"]))
    assert st == record(ref) and isinstance(st, dict)
    # a PointCloud: all its points, whatever is selected; select_keypoints narrows the selection to the WHOLE cloud's keypoints
    pc = PointCloud(X, columns=["x", "y", "z"])
    pc.select_n_points(100)
    sel = pc.idx_selected
    whole = iss_ref.keypoints(X, neighbors=12, nms_neighbors=6)
    assert np.array_equal(simpleicp_amd.keypoint_keep(pc, neighbors=12, nms_neighbors=6), whole["keep"])
    assert np.array_equal(pc.idx_selected, sel)
    pc.select_keypoints(12, nms_neighbors=6, _ctx=octx)
    assert np.array_equal(pc.idx_selected, sel[whole["keep"][sel]]) and 0 < len(pc.idx_selected) < len(sel)
    assert pc.last_keypoint_stats == record(whole)
    alone = iss_ref.keypoints(X[sel], neighbors=12, nms_neighbors=6)["keep"]          # (not the keypoints of the selection alone)
    assert not np.array_equal(sel[alone], pc.idx_selected)
    monkeypatch.setattr(backend, "get_context", lambda: oracle_backend.OracleContext())      # a backend without the entry point
    with pytest.raises(_lib.BackendError, match="ISS keypoints"):
        simpleicp_amd.keypoint_keep(X, neighbors=12)


def test_register_global_with_keypoints(octx, surface_pair):
    import simpleicp_amd
    import global_ref
    fixed, movable, kw = surface_pair
    plain = simpleicp_amd.register_global(fixed, movable, hypotheses=50, seed=1, **kw)
    assert "keypoints" not in octx.calls and plain.n_keypoints is None
    chain = list(octx.calls)
    # keypoints=None is the default, call for call and byte for byte
    octx.calls.clear()
    same = simpleicp_amd.register_global(fixed, movable, hypotheses=50, seed=1, keypoints=None, **kw)
    assert octx.calls == chain and same.H.tobytes() == plain.H.tobytes() and same.stats == plain.stats and same.n_keypoints is None
    assert (same.n_matches, same.inliers, same.index) == (plain.n_matches, plain.inliers, plain.index)
    # with keypoints the chain runs on the gathered rows
    kp = dict(neighbors=12, nms_neighbors=4, min_neighbors=3)
    kf, km = iss_ref.keypoints(fixed, **kp)["keep"], iss_ref.keypoints(movable, **kp)["keep"]
    assert kf.sum() >= 3 and km.sum() >= 3
    desc = {}
    for name, X, v in (("f", fixed, kw["viewpoint_fixed"]), ("m", movable, kw["viewpoint_movable"])):
        desc[name] = simpleicp_amd.fpfh_features(X, neighbors=kw["neighbors"], normal_neighbors=kw["normal_neighbors"], viewpoint=v)
    Ff, Fm = desc["f"][kf], desc["m"][km]
    idx = global_ref.mutual(global_ref.match(Fm, Ff)[0], global_ref.match(Ff, Fm)[0])
    good = idx >= 0
    for method, last in (({"hypotheses": 50, "seed": 1}, "ransac_triplets"), ({"method": "robust", "rounds": 30}, "pose_robust")):
        octx.calls.clear()
        res = simpleicp_amd.register_global(fixed, movable, keypoints=kp, **method, **kw)
        assert octx.calls.count("keypoints") == 2 and octx.calls.count("fpfh") == 2
        assert res.n_keypoints == (int(kf.sum()), int(km.sum())) and res.n_matches == int(good.sum())
        if res.n_matches >= 3:
            assert octx.calls[-1] == last
            rows = octx.ransac_rows if last == "ransac_triplets" else octx.robust_args[:2]
            assert np.array_equal(rows[0], movable[km][good]) and np.array_equal(rows[1], fixed[kf][idx[good]])
    assert res.n_matches >= 3                                          # (the rows above were checked)
    # keypoints=True: the defaults
    octx.calls.clear()
    res = simpleicp_amd.register_global(fixed, movable, hypotheses=50, seed=1, keypoints=True, **kw)
    assert octx.keypoint_args == (32, np.inf, 32, np.inf, 0.975, 0.975, 5)
    # fewer than three keypoints on a side: the result without a pose, and nothing after the keypoints is called
    for method, none in (({}, dict(n_hypotheses=0, n_void=0, n_pruned=0, best=-1, best_inliers=-1)),
                         ({"method": "robust"}, dict(n_poses=0, n_void=0, best=-1, best_inliers=-1))):
        octx.calls.clear()
        few = simpleicp_amd.register_global(fixed, movable, keypoints=dict(neighbors=12, gamma21=1e-6), **method, **kw)
        assert octx.calls[-1] == "keypoints" and "feature_match" not in octx.calls
        assert few.H is None and few.candidates == [] and few.stats == none and few.n_keypoints == (0, 0) and few.n_matches == 0
