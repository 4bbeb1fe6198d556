"""ISS keypoints on the GPU (contract (I)): the keep bytes, the bits of saliency and eigenvalues and the whole
record equal the numpy reference of tests/iss_ref.py, on host and device outputs -- seeded clouds, the lane seams of k, k_s != k_n,
the radii and a radius that clips, chunk seams and a partly filled last wave, a cloud past the natural chunk, exact ties,
duplicates, a cloud without a salient point --, the refusals, keypoint_keep on tensors, and the chain
register_global(keypoints=...) on the bundled bunny."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import consistency_ref
import fpfh_ref
import global_ref
import iss_ref
import posefit_ref
import robust_ref
from oracle import orc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EXTENT = 263_800.0


@pytest.fixture(scope="module")
def ctx():
    from simpleicp_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def record(r):
    return {key: r[key] for key in iss_ref.KEYS}


def check(ctx, X, k_s, r_s=np.inf, k_n=None, r_n=np.inf, g21=0.975, g32=0.975, min_nb=5, device=True, upload=True, ref=None):
    """One call against the reference: outputs in host memory; device=True: also in device memory, and keep alone.  Returns the
    reference."""
    from simpleicp_amd import _lib
    X = np.ascontiguousarray(X, dtype=np.float64)
    n = len(X)
    if upload:
        ctx.upload(_lib.FIX, X)
    if ref is None:
        ref = iss_ref.keypoints(X, k_s, r_s, k_n, r_n, g21, g32, min_nb)
    keep, sal, eig, st = ctx.keypoints(_lib.FIX, k_s, r_s, k_n, r_n, g21, g32, min_nb, want_saliency=True)
    print(f"n={n} k_s={k_s} r_s={r_s} k_n={k_n} r_n={r_n}: {st.as_dict()}")
    assert keep.dtype == np.bool_ and keep.shape == (n,) and sal.shape == (n,) and eig.shape == (n, 3)
    assert np.array_equal(u64(eig), u64(ref["eig"]))
    assert np.array_equal(u64(sal), u64(ref["saliency"]))
    assert np.array_equal(keep, ref["keep"])
    assert st.as_dict() == record(ref)
    if device:
        kd = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
        sd = torch.full((n,), -1.0, dtype=torch.float64, device=DEV)
        ed = torch.full((n, 3), -1.0, dtype=torch.float64, device=DEV)
        st2 = ctx.keypoints(_lib.FIX, k_s, r_s, k_n, r_n, g21, g32, min_nb, keep_ptr=kd.data_ptr(), saliency_ptr=sd.data_ptr(),
                            eig_ptr=ed.data_ptr())
        assert st2.as_dict() == st.as_dict()
        assert np.array_equal(kd.cpu().numpy(), keep.view(np.uint8)) and np.array_equal(u64(sd.cpu().numpy()), u64(sal))
        assert np.array_equal(u64(ed.cpu().numpy()), u64(eig))
        kd.fill_(7)                                                    # the verdicts alone, to the device
        st3 = ctx.keypoints(_lib.FIX, k_s, r_s, k_n, r_n, g21, g32, min_nb, keep_ptr=kd.data_ptr())
        assert st3.as_dict() == st.as_dict() and np.array_equal(kd.cpu().numpy(), keep.view(np.uint8))
        only = ctx.keypoints(_lib.FIX, k_s, r_s, k_n, r_n, g21, g32, min_nb)
        assert only[1] is None and only[2] is None and np.array_equal(only[0], keep)
    return ref


def lattice(n, dims=3):
    g = np.arange(n, dtype=np.float64)
    return np.ascontiguousarray(np.stack(np.meshgrid(*([g] * dims), indexing="ij"), -1).reshape(-1, dims))


# ---- seeded clouds ----
def test_seeded_cloud(ctx):
    X = np.random.default_rng(2000).uniform(-1, 1, (2000, 3))
    ref = check(ctx, X, 32, k_n=8)
    assert 0 < ref["n_keypoints"] < ref["n_salient"] <= 2000 and ref["n_small"] == 0
    assert ref["n_clipped_salient"] == 0 and ref["n_clipped_nms"] == 0
    check(ctx, X, 32, upload=False, device=False)                      # k_n None: k_s


@pytest.mark.parametrize("k", [2, 64, 65, 128])
def test_lane_seams_of_k(ctx, k):
    """One rank a lane up to 64, two from 65 on; 300 points."""
    X = np.random.default_rng(300 + k).uniform(0, 1, (300, 3))
    ref = check(ctx, X, k, min_nb=2)
    assert ref["n_salient"] > 0       # (at k = 2 too: two points are a line, whose e2 and e3 are rounding residue, not exact zeros)
    check(ctx, X, 16, k_n=k, min_nb=2, upload=False, device=False)    # the same seams in pass 2


def test_k_s_differs_from_k_n(ctx):
    X = np.random.default_rng(77).uniform(0, 1, (1200, 3))
    a = check(ctx, X, 24, k_n=10)
    b = check(ctx, X, 10, k_n=70, upload=False)
    assert a["n_keypoints"] > 0 and b["n_keypoints"] > 0 and not np.array_equal(a["keep"], b["keep"])


# ---- the radii ----
def test_radii_finite_infinite_and_clipping(ctx):
    X = np.random.default_rng(17).uniform(0, 1, (1500, 3))
    X = np.vstack([X, [[50.0, 50.0, 50.0]]])                           # an isolated point: alone in its ball
    both = check(ctx, X, 20, 0.2, 12, 0.15)
    assert both["n_small"] >= 1 and not both["keep"][1500] and both["n_keypoints"] > 0
    assert both["eig"][1500].tolist() == [0.0, 0.0, 0.0]               # m = 1: the point is its own mean
    check(ctx, X, 20, 0.2, 12, np.inf, upload=False, device=False)
    check(ctx, X, 20, np.inf, 12, 0.15, upload=False, device=False)
    # balls that hold more than k points: the counters say so
    clip = check(ctx, X, 8, 0.3, 6, 0.3, upload=False)
    assert clip["n_clipped_salient"] > 0 and clip["n_clipped_nms"] > 0


def test_radius_equal_to_a_neighbour_distance_is_strict(ctx):
    X = lattice(5)
    ref = check(ctx, X, 40, 2.0, min_nb=27, device=False)
    assert ref["n_small"] == 125 - 27 and np.all(ref["eig"][62] == 18.0 / 27.0)
    check(ctx, X, 40, np.nextafter(2.0, 3.0), min_nb=27, upload=False, device=False)
    ref = check(ctx, X, 7, 1.0, min_nb=1, upload=False, device=False)  # d2 = 1 < 1 * 1 fails: everybody is alone
    assert not ref["eig"].any() and ref["n_salient"] == 0


# ---- chunk seams ----
@pytest.mark.parametrize("n", [256, 64 * 3 + 1])
def test_chunks_of_64_give_the_bytes_of_one(ctx, n):
    """Four chunks of 64; and 64 * 3 + 1 points: a last chunk of one point, a last wave partly filled."""
    from simpleicp_amd import _lib
    X = np.random.default_rng(n).uniform(0, 1, (n, 3))
    ref = check(ctx, X, 12, 0.4, 7, 0.3, device=False)
    assert ref["n_salient"] > 64                                       # pass 2 takes more than one chunk too
    old = os.environ.get("SICP_KEYPOINT_CHUNK")
    os.environ["SICP_KEYPOINT_CHUNK"] = "64"                           # (read at sicp_ctx_create)
    try:
        with _lib.Context(0) as other:
            check(other, X, 12, 0.4, 7, 0.3, ref=ref)
    finally:
        if old is None:
            del os.environ["SICP_KEYPOINT_CHUNK"]
        else:
            os.environ["SICP_KEYPOINT_CHUNK"] = old


def test_past_the_natural_chunk(ctx):
    """70 001 points at k = 8: knn_chunk's floor is 65 536, the second chunk holds 4 465 points and ends in a wave of 49."""
    X = np.random.default_rng(70).uniform(-5, 5, (70_001, 3))
    ref = check(ctx, X, 8, min_nb=3, device=False)
    assert ref["n_salient"] > 65_536 and 0 < ref["n_keypoints"] < ref["n_salient"]


# ---- exact ties, duplicates, nothing salient ----
def test_lattices_with_ties_at_the_last_rank(ctx):
    X = lattice(6)
    idx, d2 = orc.knn(X, X, k=9)
    assert (d2[:, 8] == d2[:, 7]).mean() > 0.5                         # the k-th rank is one of several equidistant points
    check(ctx, X, 9, k_n=8, min_nb=3)
    ref = check(ctx, X, 27, min_nb=5, upload=False, device=False)
    inner = np.flatnonzero(((X > 0) & (X < 5)).all(axis=1))
    assert np.all(ref["eig"][inner] == 18.0 / 27.0) and not ref["keep"][inner].any()


def test_exact_duplicates(ctx):
    rng = np.random.default_rng(12)
    X = rng.uniform(0, 1, (300, 3))
    XX = np.concatenate([X, X])                                        # every point twice: twins share their saliency bits
    ref = check(ctx, XX, 24, k_n=12)
    assert np.array_equal(u64(ref["saliency"][:300]), u64(ref["saliency"][300:]))
    assert ref["keep"][:300].any() and not ref["keep"][300:].any()     # the lower index stays
    X[10:15] = X[3]                                                    # five copies of one point, in a cloud without twins
    check(ctx, X, 8, k_n=6, min_nb=3)


def test_a_cloud_without_a_salient_point(ctx):
    flat = np.column_stack([lattice(8, 2), np.zeros(64)])
    ref = check(ctx, flat, 9, min_nb=3)
    assert ref["n_salient"] == 0 and not ref["keep"].any() and np.all(ref["eig"][:, 2] == 0.0)
    X = np.random.default_rng(5).uniform(0, 1, (400, 3))              # the context goes on
    assert check(ctx, X, 16, k_n=6)["n_keypoints"] > 0


# ---- refusals ----
def test_non_finite_coordinates_never_reach_the_operator(ctx):
    from simpleicp_amd import _lib
    L = _lib.load()
    X = np.random.default_rng(6).uniform(0, 1, (200, 3))
    keep, st = np.zeros(200, np.uint8), _lib.KeypointStats()
    for row, bad in ((0, np.nan), (199, np.nan), (0, np.inf), (199, -np.inf)):
        Y = X.copy()
        Y[row, 1] = bad
        with pytest.raises(_lib.BackendError, match="non-finite"):
            ctx.upload(_lib.FIX, Y)
        rc = L.sicp_keypoints(ctx._h, _lib.FIX, 8, 1.0, 8, 1.0, 0.975, 0.975, 5, _lib._ptr(keep), None, None, C.byref(st))
        assert rc == _lib.ERR_INVALID and "empty" in L.sicp_last_error().decode() and not keep.any()
    check(ctx, X, 8, k_n=6, device=False)


def test_refusals_leave_the_context_usable(ctx):
    from simpleicp_amd import _lib
    X = np.random.default_rng(31).uniform(0, 1, (100, 3))
    ctx.upload(_lib.FIX, X)
    L = _lib.load()
    keep, st = np.zeros(100, np.uint8), _lib.KeypointStats()
    sal = np.zeros(100)
    P = _lib._ptr

    def raw(k_s=8, r_s=1.0, k_n=8, r_n=1.0, g21=0.975, g32=0.975, mn=3, out=keep, stats=st, c=ctx, slot=_lib.FIX):
        return L.sicp_keypoints(c._h, slot, k_s, r_s, k_n, r_n, g21, g32, mn, P(out), P(sal), None, None if stats is None else C.byref(stats))

    def refused(rc, word):
        assert rc == _lib.ERR_INVALID and word in L.sicp_last_error().decode(), (rc, L.sicp_last_error())
        assert not keep.any() and not sal.any()
        assert raw() == _lib.OK and sal.any()                          # the next valid call works
        keep[:], sal[:] = 0, 0

    refused(raw(out=None), "keep_out")
    refused(raw(stats=None), "out is null")
    for k in (1, 0, -4, 129, 101):
        refused(raw(k_s=k), "k_s ")
        refused(raw(k_n=k), "k_n ")
    for r in (float("nan"), 0.0, -1.0, -float("inf")):
        refused(raw(r_s=r), "salient_radius")
        refused(raw(r_n=r), "nms_radius")
    for g in (float("nan"), 0.0, -1.0, float("inf")):
        refused(raw(g21=g), "gamma21")
        refused(raw(g32=g), "gamma32")
    for m in (0, -1):
        refused(raw(mn=m), "min_neighbors")
    with _lib.Context(0) as other:
        refused(raw(c=other, slot=_lib.MOV), "empty")
        other.upload(_lib.MOV, X, index_base=7)
        refused(raw(c=other, slot=_lib.MOV), "shard")
    ctx.set_exchange(lambda *a: 0, 0, 1)
    try:
        rc = raw()
        assert rc == _lib.ERR_INVALID and "not supported with an exchange" in L.sicp_last_error().decode()
    finally:
        ctx.set_exchange(None, 0, 1)
    assert raw(r_s=float("inf"), r_n=float("inf")) == _lib.OK          # +inf: no radius
    check(ctx, X, 8, 1.0, 8, 1.0, min_nb=3, upload=False)


# ---- through Python ----
def test_keypoint_keep_on_a_strided_float32_view():
    import simpleicp_amd
    rng = np.random.default_rng(41)
    T = torch.tensor(rng.uniform(-1, 1, (3000, 6)), dtype=torch.float32, device=DEV)
    V = T[:, 1:6:2]                                                    # columns 1, 3, 5: row stride 6, column stride 2
    assert not V.is_contiguous()
    kw = dict(neighbors=16, salient_radius=0.4, nms_neighbors=8, nms_radius=0.3)
    kd, sd, ed, std = simpleicp_amd.keypoint_keep(V, return_saliency=True, **kw)
    assert isinstance(kd, torch.Tensor) and kd.device == T.device and kd.dtype == torch.bool and tuple(kd.shape) == (3000,)
    assert sd.dtype == ed.dtype == torch.float64 and tuple(ed.shape) == (3000, 3)
    Xh = V.cpu().numpy().astype(np.float64)
    kh, sh, eh, sth = simpleicp_amd.keypoint_keep(Xh, return_saliency=True, **kw)
    ref = iss_ref.keypoints(Xh, **kw)
    for keep, sal, eig, st in ((kd.cpu().numpy(), sd.cpu().numpy(), ed.cpu().numpy(), std), (kh, sh, eh, sth)):
        assert np.array_equal(keep, ref["keep"]) and np.array_equal(u64(sal), u64(ref["saliency"])) and np.array_equal(u64(eig), u64(ref["eig"]))
        assert st == record(ref)
    assert torch.equal(simpleicp_amd.keypoint_keep(V, **kw), kd) and len(V[kd]) == ref["n_keypoints"] > 0
    e = simpleicp_amd.keypoint_keep(V[:0])
    assert isinstance(e, torch.Tensor) and tuple(e.shape) == (0,) and e.dtype == torch.bool and e.device == T.device
    from simpleicp_amd import PointCloud
    pc = PointCloud(Xh, columns=["x", "y", "z"])
    pc.select_n_points(1000)
    sel = pc.idx_selected
    pc.select_keypoints(**kw)
    assert np.array_equal(pc.idx_selected, sel[ref["keep"][sel]]) and pc.last_keypoint_stats == record(ref)


# ---- the chain on the bundled bunny ----
KEYPOINTS = dict(neighbors=32, nms_neighbors=6)
PRUNE = dict(prune=10_000.0, prune_min_length=20_000.0)


@pytest.fixture(scope="module")
def bunny_pair():
    X = np.load(os.path.join(os.path.dirname(__file__), "golden", "data", "bunny_part1.npz"))["q"].astype(np.float64)
    perm = np.random.default_rng(1).permutation(len(X))
    A = np.ascontiguousarray(X[perm[:1500]])
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * K @ K
    t = np.array([0.05, -0.02, 0.1]) * EXTENT
    B = np.ascontiguousarray(X[perm[1500:3000]] @ R.T + t)
    vA = A.mean(axis=0) + np.array([0.0, 0.0, 2_638_000.0])
    vB = R @ vA + t
    return A, B, vA, vB, R, t


@pytest.fixture(scope="module")
def bunny_reference(bunny_pair):
    """The reference chain up to the matches: iss_ref's keypoints, the descriptors (the library's, equal to fpfh_ref's on the
    library's normals) gathered at them, global_ref's mutual matches.  Returns (src, dst, n_matches, n_keypoints)."""
    import simpleicp_amd
    from simpleicp_amd import _lib, backend
    A, B, vA, vB, _, _ = bunny_pair
    F, keep = {}, {}
    for name, X, v in (("A", A, vA), ("B", B, vB)):
        F[name] = simpleicp_amd.fpfh_features(X, neighbors=32, normal_neighbors=10, viewpoint=tuple(v))
        nv = backend.get_context().estimate_normals(_lib.FIX, np.arange(len(X), dtype=np.int64), 10)[0]
        assert np.array_equal(u32(F[name]), u32(fpfh_ref.fpfh(X, nv, 32, viewpoint=v)["fpfh"]))
        keep[name] = iss_ref.keypoints(X, **KEYPOINTS)["keep"]
    FA, FB, KA, KB = F["A"][keep["A"]], F["B"][keep["B"]], A[keep["A"]], B[keep["B"]]
    idx = global_ref.mutual(global_ref.match(FB, FA)[0], global_ref.match(FA, FB)[0])
    good = idx >= 0
    return np.ascontiguousarray(KB[good]), np.ascontiguousarray(KA[idx[good]]), int(good.sum()), (int(keep["A"].sum()), int(keep["B"].sum()))


def pose_error(H, R, t):
    Rt, tt = R.T, -R.T @ t
    dR = H[:3, :3] @ Rt.T
    return np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1))), np.linalg.norm(H[:3, 3] - tt)


def test_chain_with_keypoints_on_the_bunny(bunny_pair, bunny_reference):
    """Asserted: register_global(keypoints=...) is the reference chain bit for bit -- iss_ref, the gather, global_ref and the
    existing references --, twice and on both roads, under method="ransac" with refine=3 and under method="robust" with prune;
    n_keypoints is the reference's.  The errors against the truth are printed, not asserted."""
    import simpleicp_amd
    A, B, vA, vB, R, t = bunny_pair
    src, dst, n_matches, n_keypoints = bunny_reference
    print(f"keypoints {n_keypoints}, {n_matches} matches")
    assert min(n_keypoints) >= 100 and n_matches >= 3
    kw = dict(max_distance=10_000.0, viewpoint_fixed=tuple(vA), viewpoint_movable=tuple(vB), keypoints=KEYPOINTS)
    At, Bt = torch.tensor(A, device=DEV), torch.tensor(B, device=DEV)
    # triples and the refit
    seed = 0
    rkw = dict(hypotheses=1000, edge_ratio=0.9, seed=seed, top=4, refine=3)
    tri = np.random.default_rng(seed).integers(0, n_matches, (1000, 3), dtype=np.int32)
    rP, rinl, rec = global_ref.ransac(src, dst, tri, 10_000.0, 0.9)
    rows = np.array(sorted(np.flatnonzero(rinl >= 0), key=lambda k: (-rinl[k], k))[:4])
    fP, finl, frec = posefit_ref.refit(src, dst, rP[rows], 10_000.0, 3)
    order = np.lexsort((rows, -finl.astype(np.int64)))
    res = simpleicp_amd.register_global(At, Bt, **rkw, **kw)
    assert res.n_keypoints == n_keypoints and res.n_matches == n_matches and res.stats == rec and res.refined == frec
    assert [c[2] for c in res.candidates] == rows[order].tolist() and [c[1] for c in res.candidates] == finl[order].tolist()
    for (H, _, _), j in zip(res.candidates, order):
        assert np.array_equal(u64(H[:3, :3].ravel()), u64(fP[j, :9])) and np.array_equal(u64(H[:3, 3]), u64(fP[j, 9:]))
    for other in (simpleicp_amd.register_global(At, Bt, **rkw, **kw), simpleicp_amd.register_global(A, B, **rkw, **kw)):
        assert [c[1:] for c in other.candidates] == [c[1:] for c in res.candidates] and other.refined == res.refined
        assert all(np.array_equal(u64(a[0]), u64(b[0])) for a, b in zip(other.candidates, res.candidates))
        assert (other.n_keypoints, other.n_matches, other.stats) == (res.n_keypoints, res.n_matches, res.stats)
    angle, shift = pose_error(res.H, R, t)
    print(f"keypoints, triples + refit: {res.inliers} inliers of {n_matches}, rotation error {angle:.2f} deg, translation error "
          f"{shift / EXTENT:.4f} of the extent")
    # the robust method behind the pruning
    degree, core, crec = consistency_ref.consistency(src, dst, PRUNE["prune"], PRUNE["prune_min_length"])
    ck = consistency_ref.keep_mask(core, crec)
    assert ck.sum() >= 3
    ks, kd = np.ascontiguousarray(src[ck]), np.ascontiguousarray(dst[ck])
    P, inl, _, rrec = robust_ref.robust(ks, kd, None, 10_000.0, 64, 1.4, 0.0)
    rob = simpleicp_amd.register_global(At, Bt, method="robust", **PRUNE, **kw)
    assert rob.n_keypoints == n_keypoints and rob.n_matches == n_matches and rob.n_consistent == int(ck.sum())
    assert rob.stats == rrec and rob.inliers == inl[0]
    assert np.array_equal(u64(rob.H[:3, :3].ravel()), u64(P[0, :9])) and np.array_equal(u64(rob.H[:3, 3]), u64(P[0, 9:]))
    for other in (simpleicp_amd.register_global(At, Bt, method="robust", **PRUNE, **kw),
                  simpleicp_amd.register_global(A, B, method="robust", **PRUNE, **kw)):
        assert np.array_equal(u64(other.H), u64(rob.H))
        assert (other.inliers, other.n_consistent, other.n_keypoints, other.stats) == (rob.inliers, rob.n_consistent, rob.n_keypoints, rob.stats)
    angle, shift = pose_error(rob.H, R, t)
    print(f"keypoints, pruned, robust: {rob.inliers} inliers of {rob.n_consistent}, rotation error {angle:.2f} deg, translation error "
          f"{shift / EXTENT:.4f} of the extent")
    # without the keyword: today's chain, no field
    plain = simpleicp_amd.register_global(A, B, method="robust", max_distance=10_000.0, viewpoint_fixed=tuple(vA), viewpoint_movable=tuple(vB))
    assert plain.n_keypoints is None and plain.n_matches > n_matches
    angle, shift = pose_error(plain.H, R, t)
    print(f"all points, robust: {plain.inliers} inliers of {plain.n_matches}, rotation error {angle:.2f} deg, translation error "
          f"{shift / EXTENT:.4f} of the extent")
