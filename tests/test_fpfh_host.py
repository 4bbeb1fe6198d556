"""FPFH descriptors (contract (F)), the parts that need no GPU: the companion header and the binding, the
refusals that come before any device work, known answers of the reference alone (tests/fpfh_ref.py), and fpfh_features' host
plumbing on the stand-in backend of tests/oracle_backend.py."""
import ctypes as C
import inspect
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import fpfh_ref
import oracle_backend

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "simpleicp_hip_fpfh.h"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- header, exports, binding ----
def test_header_names_are_exported_and_bound():
    from simpleicp_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(sicp_\w+)\s*\(", text))) == sorted(_lib.FPFH_EXPORTS) == ["sicp_fpfh", "sicp_fpfh_version"]
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", str(so)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (sicp_\w+)", out))
    assert set(_lib.FPFH_EXPORTS) <= exported
    others = (set(_lib.EXPORTS) | set(_lib.BATCH_EXPORTS) | set(_lib.DEVICE_EXPORTS) | set(_lib.NORMALS_EXPORTS) | set(_lib.VOXEL_EXPORTS)
              | set(_lib.EVAL_EXPORTS) | set(_lib.OUTLIER_EXPORTS) | set(_lib.CHAIN_EXPORTS))
    assert not set(_lib.FPFH_EXPORTS) & others
    L = _lib.load()
    # the version triple: the header's, the library's, the binding's
    assert "#define SICP_FPFH_VERSION 1" in HEADER.read_text()
    assert L.sicp_fpfh_version() == _lib.FPFH_VERSION == 1 and _lib.fpfh_version() == 1
    assert f"#define SICP_FPFH_MAX_K {_lib.FPFH_MAX_K}" in HEADER.read_text() and _lib.FPFH_MAX_K == _lib.OUTLIER_MAX_K
    assert f"#define SICP_FPFH_BINS {_lib.FPFH_BINS}" in HEADER.read_text()
    assert C.sizeof(_lib.FpfhStats) == 32
    # the main header and its version are untouched, the other companions keep theirs
    assert L.sicp_abi_version() == _lib.ABI_VERSION == 7
    assert "fpfh" not in (ROOT / "include" / "simpleicp_hip.h").read_text().lower()
    assert (_lib.BATCH_VERSION, _lib.DEVICE_VERSION, _lib.NORMALS_VERSION, _lib.VOXEL_VERSION, _lib.EVAL_VERSION, _lib.OUTLIER_VERSION,
            _lib.CHAIN_VERSION) == (1,) * 7
    assert list(inspect.signature(_lib.Context.fpfh).parameters)[1:] == [
        "slot", "normals", "k", "radius", "viewpoint", "fpfh_ptr", "counts_ptr", "want_counts"]
    from simpleicp_amd import build as b
    assert any(p.name == "sicp_fpfh.hip" for p in b.SOURCES) and any(p.name == "simpleicp_hip_fpfh.h" for p in b.HEADERS)


def test_the_header_and_the_reference_hold_the_same_table():
    literals = re.findall(r"\{(-?0x[0-9a-f.]+p[-+]?\d+), (-?0x[0-9a-f.]+p[-+]?\d+)\}", HEADER.read_text())
    assert len(literals) == 10
    assert [(float.fromhex(c), float.fromhex(s)) for c, s in literals] == fpfh_ref.BORDERS
    # documentation, not contract: the entries are cos / sin of -pi + 2 pi j / 11 to within an ulp or two of libm's
    for j, (c, s) in enumerate(fpfh_ref.BORDERS, start=1):
        phi = -math.pi + 2.0 * math.pi * j / 11.0
        assert abs(c - math.cos(phi)) < 1e-15 and abs(s - math.sin(phi)) < 1e-15


def test_null_ctx_is_refused_not_dereferenced():
    from simpleicp_amd import _lib
    L = _lib.load()
    st = _lib.FpfhStats()
    nv, out = np.zeros((4, 3), np.float32), np.zeros((4, 33), np.float32)
    assert L.sicp_fpfh(None, 0, _lib._ptr(nv), 3, 1.0, None, _lib._ptr(out), None, C.byref(st)) == _lib.ERR_INVALID
    assert b"null ctx" in L.sicp_last_error()
    assert not out.any()


# ---- argument errors before the backend is touched ----
def _no_backend(monkeypatch):
    from simpleicp_amd import backend

    def no_backend(*a, **k):
        raise AssertionError("the backend was called")
    monkeypatch.setattr(backend, "get_context", no_backend)


def test_python_argument_errors_come_before_the_backend(monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import PointCloud
    _no_backend(monkeypatch)
    X = np.random.default_rng(0).standard_normal((50, 3))
    f = simpleicp_amd.fpfh_features
    assert "fpfh_features" in simpleicp_amd.__all__
    assert list(inspect.signature(f).parameters) == ["X", "normals", "neighbors", "radius", "normal_neighbors", "viewpoint", "return_counts"]
    assert all(p.kind is p.KEYWORD_ONLY for n, p in inspect.signature(f).parameters.items() if n not in ("X", "normals"))
    for k in (1, 0, -3, 129):
        with pytest.raises(ValueError, match="neighbors"):
            f(X, neighbors=k)
    for k in (2.5, 20.0, "many", True, [20], None):
        with pytest.raises(TypeError, match="neighbors"):
            f(X, neighbors=k)
    with pytest.raises(ValueError, match="neighbors .* exceeds"):
        f(X, neighbors=51)
    with pytest.raises(ValueError, match="normal_neighbors .* exceeds"):
        f(X, neighbors=8, normal_neighbors=51)
    for kn in (1, 0):
        with pytest.raises(ValueError, match="normal_neighbors"):
            f(X, normal_neighbors=kn)
    with pytest.raises(TypeError, match="normal_neighbors"):
        f(X, normal_neighbors=4.0)
    for r in (0.0, -1.0, float("nan"), -float("inf")):
        with pytest.raises(ValueError, match="radius"):
            f(X, radius=r)
    for r in ("wide", True, [1.0]):
        with pytest.raises(TypeError, match="radius"):
            f(X, radius=r)
    for v in ((0.0, 1.0), (0.0, 1.0, float("nan")), (0.0, 1.0, float("inf")), 3.0):
        with pytest.raises(ValueError, match="viewpoint"):
            f(X, viewpoint=v)
    with pytest.raises(TypeError, match="viewpoint"):
        f(X, viewpoint="here")
    with pytest.raises(ValueError, match="normals must have shape"):
        f(X, np.zeros((49, 3)))
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        f(np.zeros((50, 2)))
    with pytest.raises(ValueError, match="neighbors"):
        PointCloud(X, columns=["x", "y", "z"]).fpfh(1)
    # an empty cloud has an empty answer and needs no backend
    e = f(np.zeros((0, 3)))
    assert e.shape == (0, 33) and e.dtype == np.float32
    e, c = f(np.zeros((0, 3)), return_counts=True)
    assert e.shape == (0, 33) and c.shape == (0, 34) and c.dtype == np.uint16


# ---- known answers of the reference alone ----
def _lattice2(n=8):
    g = np.arange(n, dtype=np.float64)
    return np.ascontiguousarray(np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2))


def test_flat_patch_is_exactly_200_in_bins_5_16_27():
    P = _lattice2()
    X = np.column_stack([P, np.zeros(len(P))])
    N = np.tile(np.float32([0, 0, 1]), (len(X), 1))
    r = fpfh_ref.fpfh(X, N, 9)
    interior = np.flatnonzero(((P > 0) & (P < 7)).all(axis=1))
    want = np.zeros(33, np.float32)
    want[[5, 16, 27]] = 200.0
    assert len(interior) == 36 and np.array_equal(r["fpfh"][interior], np.tile(want, (36, 1)))
    assert np.array_equal(r["fpfh"], np.tile(want, (64, 1)))        # (the border points too: every pair of the patch is the same)
    assert np.all(r["counts"][:, 33] == 8) and np.all(r["counts"][:, [5, 16, 27]] == 8)
    assert (r["n_points"], r["n_pairs"], r["n_void_pairs"], r["n_empty"]) == (64, 64 * 8, 0, 0)
    void, b1, b2, b3, (f2, f3, a, b) = fpfh_ref.pair_feature(X[9], N[9], X[10], N[10], 1.0)
    assert not void and (f2, f3, a, b) == (0.0, 0.0, 0.0, 1.0) and (int(b1), int(b2), int(b3)) == (5, 16, 27)


def test_pair_feature_by_hand_and_under_a_swap_of_its_arguments():
    # p at the origin with normal z, q one step along x with a normal tilted towards -x by 3-4-5:
    # a1 = 0, a2 = -0.6: |a1| < |a2|, the roles swap: n1 = n_q, dp = (-1, 0, 0), f3 = 0.6
    # v = dp x n1 = (0*0.8 - 0*0, 0*(-0.6) - (-1)*0.8, 0) = (0, 0.8, 0), vn = 0.8, v = (0, 1, 0)
    # w = n1 x v = (0*0 - 0.8*1, 0.8*0 - (-0.6)*0, -0.6*1 - 0) = (-0.8, 0, -0.6); n2 = (0, 0, 1): f2 = 0, a = -0.6, b = 0.8
    p, n_p = np.zeros(3), np.float32([0, 0, 1])
    q, n_q = np.array([1.0, 0, 0]), np.float32([-0.6, 0, 0.8])
    void, b1, b2, b3, (f2, f3, a, b) = fpfh_ref.pair_feature(p, n_p, q, n_q, 1.0)
    nq = n_q.astype(np.float64)
    assert not void and f2 == 0.0 and f3 == -(nq[0] * 1.0 + 0.0 + 0.0) / 1.0 and abs(f3 - 0.6) < 1e-7
    assert abs(a + 0.6) < 1e-7 and abs(b - 0.8) < 1e-7
    # atan2(-0.6, 0.8) = -0.6435: above border 4 (-0.8568), below border 5 (-0.2856): sector 4; f2 = 0: 16; f3 = 0.6: 22 + floor(8.8)
    assert (int(b1), int(b2), int(b3)) == (4, 16, 30)
    assert int(b1) == int(math.floor(11 * (math.atan2(a, b) + math.pi) / (2 * math.pi)))
    # the same pair with its arguments swapped: dp changes sign, the test |a1| < |a2| picks the same source -- the same three bins
    rng = np.random.default_rng(5)
    P, Q = rng.standard_normal((500, 3)), rng.standard_normal((500, 3))
    NP, NQ = rng.standard_normal((500, 3)).astype(np.float32), rng.standard_normal((500, 3)).astype(np.float32)
    NP /= np.linalg.norm(NP, axis=1, keepdims=True)
    NQ /= np.linalg.norm(NQ, axis=1, keepdims=True)
    d = Q - P
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    one = fpfh_ref.pair_feature(P, NP, Q, NQ, d2)
    two = fpfh_ref.pair_feature(Q, NQ, P, NP, d2)
    assert not one[0].any() and all(np.array_equal(u, v) for u, v in zip(one[:4], two[:4]))
    assert len(np.unique(one[1])) == 11                               # every sector is met
    # void pairs: d2 == 0, a normal along dp (vn == 0), a non-finite normal
    assert fpfh_ref.pair_feature(p, n_p, p, n_q, 0.0)[0]
    assert fpfh_ref.pair_feature(p, np.float32([1, 0, 0]), q, np.float32([1, 0, 0]), 1.0)[0]
    assert fpfh_ref.pair_feature(p, np.float32([np.nan, 0, 1]), q, n_q, 1.0)[0]
    assert fpfh_ref.pair_feature(p, n_p, q, np.float32([0, np.inf, 1]), 1.0)[0]


def test_sector_table():
    # a direction exactly on border j, built from the table itself, has reached it: bin j
    for j, (c, s) in enumerate(fpfh_ref.BORDERS, start=1):
        assert int(fpfh_ref.sector(s, c)) == j
        assert int(fpfh_ref.sector(4.0 * s, 4.0 * c)) == j                        # (a power of two scales both products exactly)
    # just before a border the direction is still in the sector below it; the sectors agree with atan2 away from the borders
    th = np.linspace(-math.pi, math.pi, 20001)[1:-1]
    want = np.floor(11 * (th + math.pi) / (2 * math.pi)).astype(int)
    near = np.min(np.abs(th[:, None] - np.array([-math.pi + 2 * math.pi * j / 11 for j in range(1, 11)])[None, :]), axis=1) < 1e-9
    got = fpfh_ref.sector(np.sin(th), np.cos(th))
    assert np.array_equal(got[~near], want[~near]) and set(got) == set(range(11))
    # the chosen edge cases
    assert int(fpfh_ref.sector(0.0, -1.0)) == 0 and int(fpfh_ref.sector(-0.0, -1.0)) == 0         # +-pi: the first sector
    assert int(fpfh_ref.sector(0.0, 1.0)) == 5 and int(fpfh_ref.sector(-0.0, 1.0)) == 5           # angle 0
    assert int(fpfh_ref.sector(0.0, 0.0)) == 5 and int(fpfh_ref.sector(-0.0, -0.0)) == 5          # a = b = 0
    assert int(fpfh_ref.sector(np.nan, 1.0)) == 5 and int(fpfh_ref.sector(0.0, np.nan)) == 5
    assert int(fpfh_ref.sector(-1e-300, -1.0)) == 0 and int(fpfh_ref.sector(1e-300, -1.0)) == 10
    # the cosine bins
    assert [int(fpfh_ref.bin11(v)) for v in (-1.0, -0.82, 0.0, 0.99, 1.0, 1.5, -1.5, np.nan)] == [0, 0, 5, 10, 10, 10, 0, 0]


def test_translation_by_integers_leaves_every_bit():
    rng = np.random.default_rng(11)
    X = rng.integers(-20, 20, (400, 3)).astype(np.float64)
    N = rng.standard_normal((400, 3)).astype(np.float32)
    a = fpfh_ref.fpfh(X, N, 12, radius=9.0)
    b = fpfh_ref.fpfh(X + np.array([1000.0, -3000.0, 77.0]), N, 12, radius=9.0)
    assert np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["fpfh"].view(np.uint32), b["fpfh"].view(np.uint32))
    assert a["n_pairs"] == b["n_pairs"] > 0
    # the groups of a point with pairs sum to 200 up to rounding; rows= gives the same rows as the whole cloud
    full = a["fpfh"].astype(np.float64)
    has = a["counts"][:, 33] > 0
    assert np.allclose(full[has].reshape(-1, 3, 11).sum(axis=2), 200.0, atol=1e-3)
    some = np.array([7, 3, 399, 3])
    part = fpfh_ref.fpfh(X, N, 12, radius=9.0, rows=some)
    assert np.array_equal(part["counts"], a["counts"][some]) and np.array_equal(part["fpfh"], a["fpfh"][some])


# ---- fpfh_features on host clouds, on the stand-in backend ----
class FpfhOracleContext(oracle_backend.OracleContext):
    """The one new entry point, answered by the numpy reference."""

    def fpfh(self, slot, normals, k, radius=np.inf, viewpoint=None, fpfh_ptr=None, counts_ptr=None, want_counts=False):
        assert fpfh_ptr is None and counts_ptr is None
        self._log("fpfh")
        self.fpfh_args = (np.array(normals), int(k), float(radius), None if viewpoint is None else np.array(viewpoint))
        r = fpfh_ref.fpfh(self.cloud[slot][0], normals, k, radius, viewpoint)
        return r["fpfh"], (r["counts"] if want_counts else None), {key: r[key] for key in ("n_points", "n_pairs", "n_void_pairs", "n_empty")}


@pytest.fixture
def octx(monkeypatch):
    from simpleicp_amd import backend
    ctx = FpfhOracleContext()
    monkeypatch.setattr(backend, "get_context", lambda: ctx)
    return ctx


def test_fpfh_features_on_host_clouds(octx, monkeypatch):
    import simpleicp_amd
    from simpleicp_amd import PointCloud, _lib
    X = np.random.default_rng(4).uniform(0, 1, (300, 3))
    F = simpleicp_amd.fpfh_features(X, neighbors=12, normal_neighbors=8)
    assert octx.calls == ["upload", "estimate_normals", "fpfh"] and F.shape == (300, 33) and F.dtype == np.float32
    nv = octx.estimate_normals(_lib.FIX, np.arange(300), 8)[0]
    assert np.array_equal(octx.fpfh_args[0], nv) and octx.fpfh_args[1:3] == (12, math.inf) and octx.fpfh_args[3] is None
    # the same normals handed over: the same answer, and no estimate
    octx.calls.clear()
    F2, cnt = simpleicp_amd.fpfh_features(X, nv, neighbors=12, return_counts=True)
    assert octx.calls == ["upload", "fpfh"] and np.array_equal(F2, F) and cnt.shape == (300, 34)
    simpleicp_amd.fpfh_features(X, nv, neighbors=12, radius=0.25, viewpoint=(0, 0, 9))
    assert octx.fpfh_args[2] == 0.25 and np.array_equal(octx.fpfh_args[3], [0.0, 0.0, 9.0])
    # a PointCloud: all its points, its own normal columns where it has them
    pc = PointCloud(X, columns=["x", "y", "z"])
    pc.select_n_points(100)
    assert np.array_equal(pc.fpfh(12), simpleicp_amd.fpfh_features(X, neighbors=12))
    pc.estimate_normals(8, _ctx=octx)
    octx.calls.clear()
    Fp = pc.fpfh(12, radius=0.3)
    assert "estimate_normals" not in octx.calls
    own = octx.fpfh_args[0]
    sel = pc.idx_selected
    assert own.shape == (300, 3) and np.isnan(own[np.setdiff1d(np.arange(300), sel)]).all() and np.array_equal(own[sel], nv[sel])
    # no normal: no pairs of its own (S = 0), what is left is the neighbours' share, 100 per group -- or nothing
    sums = Fp[np.setdiff1d(np.arange(300), sel)].astype(np.float64).reshape(-1, 3, 11).sum(axis=2)
    assert np.all((np.abs(sums - 100.0) < 1e-3) | (sums == 0.0)) and (sums > 0).any()
    assert len(pc.idx_selected) == len(sel)                           # the selection is left alone
    from simpleicp_amd import backend
    monkeypatch.setattr(backend, "get_context", lambda: oracle_backend.OracleContext())      # a backend without the entry point
    with pytest.raises(_lib.BackendError, match="FPFH"):
        simpleicp_amd.fpfh_features(X, neighbors=12)
