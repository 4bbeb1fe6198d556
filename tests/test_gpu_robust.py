"""Robust pose fit on the GPU (contract (G)): the bits of the poses, the counts, the scales and the record
equal the numpy reference of tests/robust_ref.py -- at the wave, span and one-launch seams of the pair tree, on both paths of
sicp_pose_robust (SICP_ROBUST, read at sicp_ctx_create), with two levels of the second stage, more poses than the grids, void
poses, rows that are not finite, host and device memory --, the refusals, and the chain register_global(method="robust") on two
disjoint samples of the bundled bunny."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import fpfh_ref
import global_ref
import robust_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def forced(path):
    """A context of its own whose sicp_pose_robust takes `path` wherever it applies (SICP_ROBUST is read at sicp_ctx_create)."""
    from simpleicp_amd import _lib
    old = os.environ.get("SICP_ROBUST")
    os.environ["SICP_ROBUST"] = path
    try:
        return _lib.Context(0)
    finally:
        if old is None:
            del os.environ["SICP_ROBUST"]
        else:
            os.environ["SICP_ROBUST"] = old


@pytest.fixture(scope="module")
def paths():
    """The context as users get it, and one per forced path."""
    from simpleicp_amd import _lib
    ctxs = {"default": _lib.Context(0), "sweeps": forced("sweeps"), "one": forced("one")}
    yield ctxs
    for c in ctxs.values():
        c.close()


@pytest.fixture(scope="module")
def ctx(paths):
    return paths["default"]


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def rotation(axis, angle):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


R_TRUE, T_TRUE = rotation([1.0, 2.0, 3.0], 0.7), np.array([0.3, -0.2, 0.1])
IDENTITY = np.concatenate([np.eye(3).ravel(), np.zeros(3)])


def noisy_copy(rng, m, wrong=0.5, noise=0.002):
    src = rng.uniform(-1, 1, (m, 3))
    dst = src @ R_TRUE.T + T_TRUE + rng.normal(0, noise, (m, 3))
    bad = rng.choice(m, int(wrong * m), replace=False)
    dst[bad] = rng.uniform(-1, 1, (len(bad), 3))
    return src, dst


def starts(rng, b):
    """(b, 12) starts: the identity, then the true motion off by up to 20 degrees."""
    out = np.tile(IDENTITY, (b, 1))
    for k in range(1, b):
        R = rotation(rng.standard_normal(3), np.radians(20.0) * rng.uniform(0.2, 1.0)) @ R_TRUE
        out[k, :9], out[k, 9:] = R.ravel(), T_TRUE + rng.normal(0, 0.05, 3)
    return out


def same_bits(got, want, what=""):
    P, inl, scales, st = got
    rP, rinl, rscales, rec = want
    assert inl.dtype == np.int32 and np.array_equal(inl, rinl), what
    assert np.array_equal(u64(P), u64(rP)), what
    assert np.array_equal(u64(scales), u64(rscales)), what
    assert (st.as_dict() if hasattr(st, "as_dict") else st) == rec, what


def check(paths, src, dst, poses, max_distance, rounds, divisor=1.4, start_scale=0.0):
    """Every context against the reference (computed once): the default, and both forced paths."""
    want = robust_ref.robust(src, dst, poses, max_distance, rounds, divisor, start_scale)
    for name, c in paths.items():
        same_bits(c.pose_robust(src, dst, poses, max_distance, rounds, divisor, start_scale), want,
                  f"path {name}, m={len(src)}, rounds={rounds}, start_scale={start_scale}")
    return want


# ---- bit parity at the seams of the pair tree, on both paths ----
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("m", [3, 63, 64, 65, 1023, 1024, 1025, 4097, 16384, 16385])
def test_robust_equals_the_reference(paths, m, b):
    rng = np.random.default_rng(1000 * m + b)
    src, dst = noisy_copy(rng, m, wrong=0.5 if m > 3 else 0.0)
    poses = starts(rng, b) if b > 1 else None                         # (b == 1: the NULL start)
    for rounds in (1, 5, 40):
        for start_scale in (0.0, 1.5):
            P, inl, scales, rec = check(paths, src, dst, poses, 0.01, rounds, 1.4, start_scale)
            assert rec["n_void"] == 0 and np.isfinite(P).all() and np.all(inl >= 0)
    assert np.all(scales == np.float64(0.01) * np.float64(0.01))      # 40 rounds from 1.5 by 1.4: the scale is down at md2


def test_two_levels_of_the_second_stage(paths):
    """m = 2^20 + 1 025: 1 026 spans, so pt_fold runs two levels with seven and with nine terms."""
    m = 2**20 + 1025
    rng = np.random.default_rng(7)
    src, dst = noisy_copy(rng, m)
    poses = starts(rng, 2)
    want = robust_ref.robust(src, dst, poses, 0.01, 2, 1.4, 0.0)
    sd, dd = torch.tensor(src, device=DEV), torch.tensor(dst, device=DEV)
    for name in ("default", "one"):                                   # (beyond its bound a forced one-launch path is the sweeps path)
        P, inl, scales = np.empty((2, 12)), np.empty(2, np.int32), np.empty(2)
        st = paths[name].pose_robust(sd.data_ptr(), dd.data_ptr(), poses.ctypes.data, 0.01, 2, 1.4, 0.0, m=m, b=2, poses_ptr=P.ctypes.data,
                                     inliers_ptr=inl.ctypes.data, scales_ptr=scales.ctypes.data)
        same_bits((P, inl, scales, st), want, name)


def test_more_poses_than_the_grids(paths):
    """b = 32 768 + 3 over five rows: the poses' dimension of every grid strides.  Three distinct starts, repeated cyclically."""
    rng = np.random.default_rng(5)
    src, dst = noisy_copy(rng, 5, wrong=0.0)
    three = starts(rng, 3)
    b = 32768 + 3
    poses = np.ascontiguousarray(np.tile(three, (b // 3 + 1, 1))[:b])
    rP, rinl, rscales, _ = robust_ref.robust(src, dst, three, 0.01, 1, 1.4, 0.0)
    which = np.arange(b) % 3
    want = (rP[which], rinl[which], rscales[which],
            dict(n_poses=b, n_void=0, best=int(np.flatnonzero(rinl[which] == rinl.max())[0]), best_inliers=int(rinl.max())))
    for name, c in paths.items():
        same_bits(c.pose_robust(src, dst, poses, 0.01, 1, 1.4, 0.0), want, name)


def test_void_poses_and_rows_that_are_not_finite(paths):
    rng = np.random.default_rng(65)
    src, dst = noisy_copy(rng, 1100, wrong=0.3)
    good = starts(rng, 3)
    nan, inf = good[1].copy(), good[2].copy()
    nan[7], inf[11] = np.nan, -np.inf
    far = np.concatenate([np.eye(3).ravel(), [1e200, 0.0, 0.0]])      # d2 overflows for every row: no row counts
    poses = np.stack([good[0], nan, good[1], inf, far, good[2], np.zeros(12)])
    for start_scale in (0.0, 2.0):
        P, inl, scales, rec = check(paths, src, dst, poses, 0.01, 20, 1.4, start_scale)
        assert inl[1] == inl[3] == -1 and not P[[1, 3]].any() and not np.signbit(P[[1, 3]]).any() and not scales[[1, 3]].any()
        if start_scale == 0.0:
            assert inl[4] == -1 and not P[4].any() and rec["n_void"] == 3      # no row to take a scale from: void
        else:
            assert inl[4] == 0 and np.array_equal(u64(P[4]), u64(far)) and scales[4] == 2.0 and rec["n_void"] == 2
        assert rec["best_inliers"] == inl.max() > 300 and rec["best"] == int(np.argmax(inl))
    # nothing but void poses
    _, inl, _, rec = check(paths, src, dst, np.stack([nan, inf]), 0.01, 2)
    assert rec == dict(n_poses=2, n_void=2, best=-1, best_inliers=-1)
    # rows with NaN and infinities, at the seams of a wave and of a span
    bad_s, bad_d = src.copy(), dst.copy()
    bad_s[[0, 63, 64, 1023, 1024], [0, 1, 2, 0, 1]] = [np.nan, np.inf, np.nan, -np.inf, np.nan]
    bad_d[[5, 700, 1099], [1, 2, 0]] = [np.inf, np.nan, -np.inf]
    for start_scale in (0.0, 2.0):
        P, inl, _, _ = check(paths, bad_s, bad_d, good, 0.01, 20, 1.4, start_scale)
        assert np.isfinite(P).all() and np.all(inl > 300)
    check(paths, bad_s, bad_d, None, 0.01, 3)
    # every row invalid: void with the automatic scale; with a given one the start stays, without an inlier
    nowhere = np.full((70, 3), np.nan)
    P, inl, scales, rec = check(paths, nowhere, dst[:70], good, 0.01, 3)
    assert np.all(inl == -1) and not P.any() and not scales.any() and rec == dict(n_poses=3, n_void=3, best=-1, best_inliers=-1)
    P, inl, scales, rec = check(paths, nowhere, dst[:70], good, 0.01, 3, 1.4, 2.0)
    assert np.all(inl == 0) and np.array_equal(u64(P), u64(good)) and np.all(scales == 2.0) and rec["best"] == 0
    # every point the same: K is zero, the rotation the identity
    P, inl, _, _ = check(paths, np.ones((65, 3)), np.full((65, 3), 2.0), None, 0.01, 2)
    assert np.array_equal(P[0], np.concatenate([np.eye(3).ravel(), [1.0, 1.0, 1.0]])) and inl[0] == 65


def test_host_and_device_memory_give_the_same_bits(ctx):
    import simpleicp_amd
    from simpleicp_amd import _lib
    rng = np.random.default_rng(300)
    src, dst = noisy_copy(rng, 300)
    poses = starts(rng, 4)
    want = robust_ref.robust(src, dst, poses, 0.01, 7, 1.4, 0.0)
    sd, dd, pd_in = torch.tensor(src, device=DEV), torch.tensor(dst, device=DEV), torch.tensor(poses, device=DEV)
    L, P = _lib.load(), _lib._ptr
    for on_device in (False, True):
        po = torch.full((4, 12), -7.0, dtype=torch.float64, device=DEV) if on_device else np.full((4, 12), -7.0)
        io = torch.full((4,), -7, dtype=torch.int32, device=DEV) if on_device else np.full(4, -7, np.int32)
        so = torch.full((4,), -7.0, dtype=torch.float64, device=DEV) if on_device else np.full(4, -7.0)
        st = _lib.RobustStats()
        rc = L.sicp_pose_robust(ctx._h, P(sd if on_device else src), P(dst if on_device else dd), 300, P(pd_in if on_device else poses), 4,
                                0.01, 7, 1.4, 0.0, P(po), P(io), P(so), C.byref(st))
        assert rc == _lib.OK, L.sicp_last_error()
        got = [a.cpu().numpy() if on_device else a for a in (po, io, so)]
        same_bits((*got, st), want, f"outputs on the device: {on_device}")
    assert np.array_equal(u64(sd.cpu().numpy()), u64(src)) and np.array_equal(u64(pd_in.cpu().numpy()), u64(poses))
    # the Python road: arrays and CUDA tensors, float32 widened exactly, one pose, a stack and no pose
    Hs = np.tile(np.eye(4), (4, 1, 1))
    Hs[:, :3, :3], Hs[:, :3, 3] = poses[:, :9].reshape(-1, 3, 3), poses[:, 9:]
    s32 = src.astype(np.float32)
    rP, rn, _, _ = robust_ref.robust(s32.astype(np.float64), dst, poses, 0.01, 7, 1.4, 0.0)
    out_t, n_t = simpleicp_amd.robust_pose(torch.tensor(s32, device=DEV), torch.tensor(dst, device=DEV), max_distance=0.01, H=Hs, rounds=7)
    out_a, n_a = simpleicp_amd.robust_pose(s32, dst, max_distance=0.01, H=Hs, rounds=7)
    assert np.array_equal(u64(out_t), u64(out_a)) and np.array_equal(n_t, n_a) and np.array_equal(n_a, rn)
    assert np.array_equal(u64(out_a[:, :3, :3].reshape(4, 9)), u64(rP[:, :9])) and np.array_equal(u64(out_a[:, :3, 3]), u64(rP[:, 9:]))
    H0, n0 = simpleicp_amd.robust_pose(sd, dd, max_distance=0.01)
    H1, n1 = simpleicp_amd.robust_pose(src, dst, max_distance=0.01)
    fP, fn, _, _ = robust_ref.robust(src, dst, None, 0.01, 64, 1.4, 0.0)
    assert n0 == n1 == fn[0] and np.array_equal(u64(H0), u64(H1)) and np.array_equal(u64(H0[:3, :3].ravel()), u64(fP[0, :9]))
    assert np.array_equal(u64(H0[:3, 3]), u64(fP[0, 9:]))


def test_refusals_leave_the_context_usable(ctx):
    from simpleicp_amd import _lib
    L, P = _lib.load(), _lib._ptr
    rng = np.random.default_rng(2)
    src, dst = noisy_copy(rng, 20, wrong=0.0)
    poses = starts(rng, 2)
    out, inl, sc, st = np.full((2, 12), -7.0), np.full(2, -7, np.int32), np.full(2, -7.0), _lib.RobustStats()

    def raw(s=src, d=dst, m=20, p=poses, b=2, md=0.05, rounds=2, div=1.4, s0=0.0, po=out, io=inl, so=sc, stats=st):
        return L.sicp_pose_robust(ctx._h, P(s), P(d), m, P(p), b, md, rounds, div, s0, P(po), P(io), P(so),
                                  None if stats is None else C.byref(stats))

    def refused(rc, word):
        assert rc == _lib.ERR_INVALID and word in L.sicp_last_error().decode(), (rc, L.sicp_last_error())
        assert np.all(inl == -7) and np.all(out == -7.0) and np.all(sc == -7.0)

    refused(raw(s=None), "src")
    refused(raw(d=None), "dst")
    refused(raw(po=None), "poses_out")
    refused(raw(io=None), "inliers_out")
    refused(raw(so=None), "scales_out")
    refused(raw(stats=None), "out is null")
    refused(raw(p=None), "poses_in")                                  # NULL poses_in: b must be 1
    refused(raw(m=2), "m ")
    refused(raw(m=2**31), "m ")
    refused(raw(b=0), "b ")
    for r in (0, -1, 257):
        refused(raw(rounds=r), "rounds")
    for md in (0.0, -1.0, float("nan"), float("inf")):
        refused(raw(md=md), "max_distance")
    for div in (1.0, 0.5, -3.0, float("nan"), float("inf")):
        refused(raw(div=div), "divisor")
    for s0 in (-1.0, float("nan"), float("inf")):
        refused(raw(s0=s0), "start_scale")
    ctx.set_exchange(lambda *a: 0, 0, 1)
    try:
        refused(raw(), "not supported with an exchange")
    finally:
        ctx.set_exchange(None, 0, 1)
    assert raw(rounds=256) == _lib.OK
    same_bits((out, inl, sc, st), robust_ref.robust(src, dst, poses, 0.05, 256, 1.4, 0.0))


# ---- the chain on the bundled bunny (the fixtures of test_gpu_global.py) ----
EXTENT = 263_800.0


@pytest.fixture(scope="module")
def bunny_pair():
    X = np.load(os.path.join(os.path.dirname(__file__), "golden", "data", "bunny_part1.npz"))["q"].astype(np.float64)
    perm = np.random.default_rng(1).permutation(len(X))
    A = np.ascontiguousarray(X[perm[:1500]])
    R = rotation([1.0, 2.0, 3.0], 0.7)
    t = np.array([0.05, -0.02, 0.1]) * EXTENT
    B = np.ascontiguousarray(X[perm[1500:3000]] @ R.T + t)
    vA = A.mean(axis=0) + np.array([0.0, 0.0, 2_638_000.0])
    vB = R @ vA + t
    return A, B, vA, vB, R, t


@pytest.fixture(scope="module")
def bunny_reference(bunny_pair):
    """The references fed the library's own normals and descriptors: the matches."""
    import simpleicp_amd
    from simpleicp_amd import _lib, backend
    A, B, vA, vB, _, _ = bunny_pair
    F = {}
    for name, X, v in (("A", A, vA), ("B", B, vB)):
        F[name] = simpleicp_amd.fpfh_features(X, neighbors=32, normal_neighbors=10, viewpoint=tuple(v))
        nv = backend.get_context().estimate_normals(_lib.FIX, np.arange(len(X), dtype=np.int64), 10)[0]
        assert np.array_equal(u32(F[name]), u32(fpfh_ref.fpfh(X, nv, 32, viewpoint=v)["fpfh"]))
    idx = global_ref.mutual(global_ref.match(F["B"], F["A"])[0], global_ref.match(F["A"], F["B"])[0])
    keep = idx >= 0
    return np.ascontiguousarray(B[keep]), np.ascontiguousarray(A[idx[keep]]), int(keep.sum())


def pose_error(H, R, t):
    """(degrees, length) between H and the inverse of the motion (R, t) that made the movable cloud."""
    Rt, tt = R.T, -R.T @ t
    dR = H[:3, :3] @ Rt.T
    return np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1))), np.linalg.norm(H[:3, 3] - tt)


def test_robust_chain_on_the_bunny(bunny_pair, bunny_reference):
    """Recorded on one MI355X, 395 matches: the robust fit ends with 160 inliers, 0.50 degrees and 0.36 % of
    the extent from the truth; RANSAC with refine=3 on the same matches with 162 / 161 / 163 inliers, 0.21 / 0.53 / 2.27 degrees
    and 0.22 % / 0.18 % / 1.64 % (seeds 0 / 1 / 2).  A finding, not asserted: wrong descriptor matches are structured, and no
    ranking of the two methods is claimed.  Asserted: the chain is the reference's bit for bit, twice, on both roads."""
    import simpleicp_amd
    A, B, vA, vB, R, t = bunny_pair
    src, dst, n_matches = bunny_reference
    kw = dict(max_distance=10_000.0, viewpoint_fixed=tuple(vA), viewpoint_movable=tuple(vB))
    res = simpleicp_amd.register_global(torch.tensor(A, device=DEV), torch.tensor(B, device=DEV), method="robust", **kw)
    again = simpleicp_amd.register_global(torch.tensor(A, device=DEV), torch.tensor(B, device=DEV), method="robust", **kw)
    host = simpleicp_amd.register_global(A, B, method="robust", **kw)
    P, inl, scales, rec = robust_ref.robust(src, dst, None, 10_000.0, 64, 1.4, 0.0)
    assert res.n_matches == n_matches and res.stats == rec and res.refined is None and len(res.candidates) == 1
    assert res.inliers == inl[0] and res.index == -1
    assert np.array_equal(u64(res.H[:3, :3].ravel()), u64(P[0, :9])) and np.array_equal(u64(res.H[:3, 3]), u64(P[0, 9:]))
    for other in (again, host):
        assert np.array_equal(u64(other.H), u64(res.H)) and other.inliers == res.inliers and other.stats == res.stats
    angle, shift = pose_error(res.H, R, t)
    print(f"robust: {n_matches} matches, {res.inliers} inliers, rotation error {angle:.2f} deg, translation error "
          f"{shift / EXTENT:.4f} of the extent, final scale {scales[0]:.4g}")
    for seed in (0, 1, 2):
        ran = simpleicp_amd.register_global(A, B, hypotheses=1000, edge_ratio=0.9, seed=seed, top=4, refine=3, **kw)
        a, s = pose_error(ran.H, R, t)
        print(f"ransac seed {seed} + refine=3: {ran.inliers} inliers, rotation error {a:.2f} deg, translation error "
              f"{s / EXTENT:.4f} of the extent")
