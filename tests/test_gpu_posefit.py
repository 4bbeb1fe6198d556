"""Least-squares pose refit on the GPU (contract (L)): the bits of the poses, the counts and the record equal
the numpy reference of tests/posefit_ref.py -- the wave, tile and span seams of the pair tree, few and many poses, one and
three rounds, the plain fit, an unbounded distance, void poses and sets with nothing to fit, host and device memory --, the
refusals, and the chain register_global(refine=3) on two disjoint samples of the bundled bunny."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest
import torch

import fpfh_ref
import global_ref
import posefit_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ctx():
    from simpleicp_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def rotation(axis, angle):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


R_TRUE, T_TRUE = rotation([1.0, 2.0, 3.0], 0.7), np.array([0.3, -0.2, 0.1])


def noisy_copy(rng, m, wrong=0.4, noise=0.002):
    src = rng.uniform(-1, 1, (m, 3))
    dst = src @ R_TRUE.T + T_TRUE + rng.normal(0, noise, (m, 3))
    bad = rng.choice(m, int(wrong * m), replace=False)
    dst[bad] = rng.uniform(-1, 1, (len(bad), 3))
    return src, dst


def perturbed(rng, b, degrees=3.0, shift=0.01):
    """(b, 12) poses: the true motion off by a few degrees and a little shift."""
    out = np.empty((b, 12))
    for k in range(b):
        R = rotation(rng.standard_normal(3), np.radians(degrees) * rng.uniform(0.2, 1.0)) @ R_TRUE
        out[k, :9], out[k, 9:] = R.ravel(), T_TRUE + rng.normal(0, shift, 3)
    return out


def check(ctx, src, dst, poses, max_distance, rounds):
    P, inl, st = ctx.pose_refit(src, dst, poses, max_distance, rounds)
    rP, rinl, rec = posefit_ref.refit(src, dst, poses, max_distance, rounds)
    print(f"m={len(src)} b={len(rP)} rounds={rounds} max_distance={max_distance}: {st.as_dict()}")
    assert inl.dtype == np.int32 and np.array_equal(inl, rinl)
    assert np.array_equal(u64(P), u64(rP))
    assert st.as_dict() == rec
    return P, inl, rec


# ---- bit parity at the seams of the pair tree ----
@pytest.mark.parametrize("rounds", [1, 3])
@pytest.mark.parametrize("b", [1, 5, 70])
@pytest.mark.parametrize("m", [3, 64, 65, 256, 257, 1024, 1025, 2049])
def test_refit_equals_the_reference(ctx, m, b, rounds):
    rng = np.random.default_rng(1000 * m + 10 * b + rounds)
    src, dst = noisy_copy(rng, m, wrong=0.4 if m > 3 else 0.0)
    poses = perturbed(rng, b)
    before = global_ref.count_inliers(poses[:, :9].reshape(-1, 3, 3), poses[:, 9:], src, dst, 0.05)
    _, inl, rec = check(ctx, src, dst, poses, 0.05, rounds)
    assert np.all(inl >= before) and rec["n_improved"] == int((inl > before).sum())
    if m >= 64 and b >= 5:
        assert rec["n_improved"] > 0


def test_refit_masks_by_the_fused_sum(ctx):
    """A max_distance whose square lies between the fused d2 of contract (D) and the same sum rounded product by product, for a
    row under the first input pose: that row is in the mask of exactly one of the two, so the round's fit tells them apart."""
    rng = np.random.default_rng(78)
    src, dst = noisy_copy(rng, 2048, wrong=0.3)
    poses = perturbed(rng, 4, degrees=0.5, shift=0.002)
    fused, plain = global_ref.d2_fused_and_plain(poses[0, :9].reshape(3, 3), poses[0, 9:], src, dst)
    md = global_ref.threshold_between(fused, plain)
    assert md is not None and (fused < md * md).sum() != (plain < md * md).sum()
    for rounds in (1, 2):
        check(ctx, src, dst, poses, md, rounds)


def test_unbounded_distance_and_the_plain_fit(ctx):
    import simpleicp_amd
    rng = np.random.default_rng(1025)
    src, dst = noisy_copy(rng, 1025, wrong=0.0)
    poses = perturbed(rng, 5)
    _, inl, _ = check(ctx, src, dst, poses, np.inf, 2)
    assert np.all(inl == 1025)
    P, inl, rec = check(ctx, src, dst, None, np.inf, 1)
    assert inl[0] == 1025 and rec["n_improved"] == 1 and np.abs(P[0, :9].reshape(3, 3) - R_TRUE).max() < 1e-3
    check(ctx, src, dst, None, 0.004, 3)                              # a plain start, then rounds under a distance
    # NaN and infinite rows are no part of a plain fit, and of no mask
    bad_s, bad_d = src.copy(), dst.copy()
    bad_s[[0, 63, 64, 1024], [0, 1, 2, 0]] = np.nan
    bad_d[[5, 700], [1, 2]] = [np.inf, np.nan]
    P, inl, _ = check(ctx, bad_s, bad_d, None, np.inf, 1)
    assert inl[0] == 1025 - 6
    check(ctx, bad_s, bad_d, poses, 0.05, 2)
    # the Python road: arrays and CUDA tensors, float32 widened exactly
    H = simpleicp_amd.fit_pose(torch.tensor(bad_s, device=DEV), torch.tensor(bad_d, device=DEV))
    assert np.array_equal(u64(H[:3, :3].ravel()), u64(P[0, :9])) and np.array_equal(u64(H[:3, 3]), u64(P[0, 9:]))
    assert np.array_equal(u64(simpleicp_amd.fit_pose(bad_s, bad_d)), u64(H))
    s32 = torch.tensor(src.astype(np.float32), device=DEV)
    Hs = np.tile(np.eye(4), (5, 1, 1))
    Hs[:, :3, :3], Hs[:, :3, 3] = poses[:, :9].reshape(-1, 3, 3), poses[:, 9:]
    out, n = simpleicp_amd.refine_pose(s32, torch.tensor(dst, device=DEV), Hs, max_distance=0.05, rounds=2)
    rP, rn, _ = posefit_ref.refit(src.astype(np.float32).astype(np.float64), dst, poses, 0.05, 2)
    assert np.array_equal(n, rn) and np.array_equal(u64(out[:, :3, :3].reshape(5, 9)), u64(rP[:, :9]))
    assert np.array_equal(u64(out[:, :3, 3]), u64(rP[:, 9:]))
    out2, n2 = simpleicp_amd.refine_pose(src.astype(np.float32), dst, Hs, max_distance=0.05, rounds=2)
    assert np.array_equal(u64(out2), u64(out)) and np.array_equal(n2, n)


def test_void_poses_and_nothing_to_fit(ctx):
    rng = np.random.default_rng(65)
    src, dst = noisy_copy(rng, 65, wrong=0.2)
    good = perturbed(rng, 3)
    nan = good[0].copy()
    nan[7] = np.nan
    inf = good[1].copy()
    inf[11] = -np.inf
    far = np.concatenate([np.eye(3).ravel(), [40.0, 0.0, 0.0]])      # a finite pose without a single inlier
    poses = np.stack([np.zeros(12), nan, good[0], far, inf, good[2]])
    P, inl, rec = check(ctx, src, dst, poses, 0.05, 3)
    assert inl[1] == inl[4] == -1 and rec["n_void"] == 2 and not P[[1, 4]].any() and not np.signbit(P[[1, 4]]).any()
    assert inl[3] == 0 and np.array_equal(u64(P[3]), u64(far)) and inl[0] < 3 and not P[0].any()
    assert rec["best"] in (2, 5) and rec["best_inliers"] == inl.max() > 30
    # nothing but void poses
    _, inl, rec = check(ctx, src, dst, np.stack([nan, inf]), 0.05, 2)
    assert rec == dict(n_poses=2, n_void=2, n_improved=0, best=-1, best_inliers=-1)
    # two inliers: the round yields nothing, the pose stays
    two = src @ R_TRUE.T + T_TRUE
    two[2:] += 5.0
    P, inl, rec = check(ctx, src, two, np.concatenate([R_TRUE.ravel(), T_TRUE])[None], 0.05, 3)
    assert inl[0] == 2 and rec["n_improved"] == 0
    # all inliers on one line: a finite pose, whatever it is, the reference's
    line = np.zeros((65, 3))
    line[:, 0] = np.linspace(-1, 1, 65)
    P, inl, _ = check(ctx, line, line @ R_TRUE.T + T_TRUE, None, np.inf, 1)
    assert np.isfinite(P).all() and inl[0] == 65
    check(ctx, line, line @ R_TRUE.T + T_TRUE, good, 0.5, 3)
    # every point the same: K is zero, the rotation the identity
    P, inl, _ = check(ctx, np.ones((65, 3)), np.full((65, 3), 2.0), None, np.inf, 1)
    assert np.array_equal(P[0], np.concatenate([np.eye(3).ravel(), [1.0, 1.0, 1.0]])) and inl[0] == 65
    # NaN rows in src
    holes = src.copy()
    holes[::7, 1] = np.nan
    _, inl, _ = check(ctx, holes, dst, good, 0.05, 3)
    assert inl.max() <= 65 - 10
    # fewer than three finite rows: no pose at all
    holes[2:] = np.nan
    _, inl, rec = check(ctx, holes, dst, None, np.inf, 1)
    assert inl[0] == -1 and rec["best"] == -1


def test_host_and_device_memory_give_the_same_bits(ctx):
    from simpleicp_amd import _lib
    rng = np.random.default_rng(300)
    src, dst = noisy_copy(rng, 300)
    poses = perturbed(rng, 5)
    rP, rinl, rec = posefit_ref.refit(src, dst, poses, 0.05, 3)
    sd, dd, pd_in = torch.tensor(src, device=DEV), torch.tensor(dst, device=DEV), torch.tensor(poses, device=DEV)
    L, P = _lib.load(), _lib._ptr
    for s_dev, d_dev, in_dev, p_dev, i_dev in itertools.product((False, True), repeat=5):
        ph, ih = np.full((5, 12), -7.0), np.full(5, -7, np.int32)
        pd = torch.full((5, 12), -7.0, dtype=torch.float64, device=DEV)
        idv = torch.full((5,), -7, dtype=torch.int32, device=DEV)
        st = _lib.PosefitStats()
        rc = L.sicp_pose_refit(ctx._h, P(sd if s_dev else src), P(dd if d_dev else dst), 300, P(pd_in if in_dev else poses), 5, 0.05, 3,
                               P(pd if p_dev else ph), P(idv if i_dev else ih), C.byref(st))
        assert rc == _lib.OK, L.sicp_last_error()
        assert np.array_equal(idv.cpu().numpy() if i_dev else ih, rinl), (s_dev, d_dev, in_dev, p_dev, i_dev)
        assert np.array_equal(u64(pd.cpu().numpy() if p_dev else ph), u64(rP)) and st.as_dict() == rec
    # the pointer road of the binding; the inputs are left alone
    pd, idv = torch.empty((5, 12), dtype=torch.float64, device=DEV), torch.empty(5, dtype=torch.int32, device=DEV)
    st = ctx.pose_refit(sd.data_ptr(), dd.data_ptr(), pd_in.data_ptr(), 0.05, 3, m=300, b=5, poses_ptr=pd.data_ptr(),
                        inliers_ptr=idv.data_ptr())
    assert np.array_equal(u64(pd.cpu().numpy()), u64(rP)) and np.array_equal(idv.cpu().numpy(), rinl) and st.as_dict() == rec
    assert np.array_equal(u64(sd.cpu().numpy()), u64(src)) and np.array_equal(u64(pd_in.cpu().numpy()), u64(poses))


def test_refusals_leave_the_context_usable(ctx):
    from simpleicp_amd import _lib
    L, P = _lib.load(), _lib._ptr
    rng = np.random.default_rng(2)
    src, dst = noisy_copy(rng, 20, wrong=0.0)
    poses = perturbed(rng, 2)
    out, inl, st = np.full((2, 12), -7.0), np.full(2, -7, np.int32), _lib.PosefitStats()

    def raw(s=src, d=dst, m=20, p=poses, b=2, md=0.05, rounds=2, po=out, io=inl, stats=st):
        return L.sicp_pose_refit(ctx._h, P(s), P(d), m, P(p), b, md, rounds, P(po), P(io), None if stats is None else C.byref(stats))

    def refused(rc, word):
        assert rc == _lib.ERR_INVALID and word in L.sicp_last_error().decode(), (rc, L.sicp_last_error())
        assert np.all(inl == -7) and np.all(out == -7.0)

    refused(raw(s=None), "src")
    refused(raw(d=None), "dst")
    refused(raw(po=None), "poses_out")
    refused(raw(io=None), "inliers_out")
    refused(raw(stats=None), "out is null")
    refused(raw(p=None), "poses_in")                                  # NULL poses_in: b must be 1
    refused(raw(m=2), "m ")
    refused(raw(m=2**31), "m ")
    refused(raw(b=0), "b ")
    for r in (0, -1, 65):
        refused(raw(rounds=r), "rounds")
    for md in (0.0, -1.0, float("nan"), -float("inf")):
        refused(raw(md=md), "max_distance")
    ctx.set_exchange(lambda *a: 0, 0, 1)
    try:
        refused(raw(), "not supported with an exchange")
    finally:
        ctx.set_exchange(None, 0, 1)
    assert raw() == _lib.OK
    rP, rinl, rec = posefit_ref.refit(src, dst, poses, 0.05, 2)
    assert np.array_equal(u64(out), u64(rP)) and np.array_equal(inl, rinl) and st.as_dict() == rec


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
    """The references fed the library's own normals and descriptors: the matches, shared by the seeds."""
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


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_refined_chain_on_the_bunny(bunny_pair, bunny_reference, seed):
    """Recorded on one MI355X, the best candidate before -> after the refit: seed 0: 153 -> 162 inliers,
    3.31 -> 0.21 degrees, 2.29 % -> 0.22 % of the extent; seed 1: 160 -> 161, 2.18 -> 0.53 degrees, 0.49 % -> 0.18 %; seed 2: no
    candidate's refit beats the leader's 163 inliers, which leaves as it came (2.27 degrees, 1.64 %).  A finding, not asserted:
    the bar stays the unrefined chain's."""
    import simpleicp_amd
    A, B, vA, vB, R, t = bunny_pair
    src, dst, n_matches = bunny_reference
    kw = dict(max_distance=10_000.0, viewpoint_fixed=tuple(vA), viewpoint_movable=tuple(vB), hypotheses=1000, edge_ratio=0.9, seed=seed,
              top=4)
    res = simpleicp_amd.register_global(torch.tensor(A, device=DEV), torch.tensor(B, device=DEV), refine=3, **kw)
    tri = np.random.default_rng(seed).integers(0, n_matches, (1000, 3), dtype=np.int32)
    rP, rinl, rec = global_ref.ransac(src, dst, tri, 10_000.0, 0.9)
    rows = np.array(sorted(np.flatnonzero(rinl >= 0), key=lambda k: (-rinl[k], k))[:4])
    fP, finl, frec = posefit_ref.refit(src, dst, rP[rows], 10_000.0, 3)
    order = np.lexsort((rows, -finl.astype(np.int64)))
    print(f"seed {seed}: {n_matches} matches, {res.stats}, refit {res.refined}: counts {rinl[rows].tolist()} -> {finl.tolist()}")
    assert res.n_matches == n_matches and res.stats == rec and res.refined == frec
    assert [c[2] for c in res.candidates] == rows[order].tolist() and [c[1] for c in res.candidates] == finl[order].tolist()
    for (H, _, _), j in zip(res.candidates, order):
        assert np.array_equal(u64(H[:3, :3].ravel()), u64(fP[j, :9])) and np.array_equal(u64(H[:3, 3]), u64(fP[j, 9:]))
    assert np.all(finl >= rinl[rows])
    # the numpy road gives the same candidates
    host = simpleicp_amd.register_global(A, B, refine=3, **kw)
    assert [c[1:] for c in host.candidates] == [c[1:] for c in res.candidates] and host.refined == res.refined
    assert all(np.array_equal(u64(a[0]), u64(b[0])) for a, b in zip(host.candidates, res.candidates))
    H0 = np.eye(4)
    H0[:3, :3], H0[:3, 3] = rP[rec["best"], :9].reshape(3, 3), rP[rec["best"], 9:]
    a0, s0 = pose_error(H0, R, t)
    angle, shift = pose_error(res.H, R, t)
    print(f"seed {seed}: rotation error {a0:.2f} -> {angle:.2f} deg, translation error {s0 / EXTENT:.4f} -> {shift / EXTENT:.4f} of the "
          f"extent, inliers {rec['best_inliers']} -> {res.inliers}")
    assert angle < 10.0 and shift < 0.1 * EXTENT
