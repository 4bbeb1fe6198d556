"""Descriptor matching and RANSAC poses on the GPU (contracts (M) and (R)): indices, the bits of the
distances, inlier counts, the bits of the poses and the records equal the numpy references of tests/global_ref.py -- seeded
shapes, chunk seams, ties, NaN and overflow, void and pruned hypotheses, host and device memory --, the refusals, and the chain
fpfh_features -> match_features -> ransac_pose on two disjoint samples of the bundled bunny."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest
import torch

import fpfh_ref
import global_ref

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


# ---- matching (M) ----
def check_match(ctx, q, t):
    idx, d2, st = ctx.feature_match(q, t)
    ridx, rd2, rec = global_ref.match(q, t)
    print(f"nq={len(q)} nt={len(t)} dim={q.shape[1]}: {st.as_dict()}")
    assert idx.dtype == np.int32 and np.array_equal(idx, ridx)
    assert np.array_equal(u32(d2), u32(rd2))
    assert st.as_dict() == rec
    return idx, d2


@pytest.mark.parametrize("nq,nt,dim", [(1, 1, 1), (5, 1, 33), (300, 257, 33), (1000, 1500, 33), (130, 1000, 64), (64, 65, 2)])
def test_match_seeded_shapes(ctx, nq, nt, dim):
    rng = np.random.default_rng(1000 * nq + nt + dim)
    q = rng.uniform(0, 200, (nq, dim)).astype(np.float32)
    t = rng.uniform(0, 200, (nt, dim)).astype(np.float32)
    t[rng.integers(0, nt, max(nt // 10, 1))] = q[rng.integers(0, nq, max(nt // 10, 1))]          # exact hits, some of them repeated
    check_match(ctx, q, t)


@pytest.fixture(scope="module")
def fpfh_rows():
    """Real FPFH rows of a seeded cloud, in two halves."""
    import simpleicp_amd
    X = np.random.default_rng(77).uniform(-1, 1, (1400, 3))
    F = simpleicp_amd.fpfh_features(X, neighbors=16, normal_neighbors=10, viewpoint=(0, 0, 5))
    return np.ascontiguousarray(F[:600]), np.ascontiguousarray(F[600:])


def test_match_real_fpfh_rows(ctx, fpfh_rows):
    q, t = fpfh_rows
    idx, _ = check_match(ctx, q, t)
    assert len(np.unique(idx)) > 100


def test_match_tie_across_a_chunk_seam():
    from simpleicp_amd import _lib
    rng = np.random.default_rng(64)
    q = rng.uniform(0, 1, (70, 33)).astype(np.float32)
    t = rng.uniform(0, 1, (300, 33)).astype(np.float32)
    t[63] = t[64] = t[200] = q[5]
    t[130] = t[10] = q[6]                                             # the lower index lies two chunks before
    old = os.environ.get("SICP_MATCH_CHUNK")
    os.environ["SICP_MATCH_CHUNK"] = "64"                             # (read at sicp_ctx_create)
    try:
        with _lib.Context(0) as other:
            idx, d2 = check_match(other, q, t)
            assert idx[5] == 63 and d2[5] == 0 and idx[6] == 10
            dup = np.ascontiguousarray(np.tile(q[5], (300, 1)))       # every row ties: row 0 of the first chunk
            assert np.all(check_match(other, q[5:6], dup)[0] == 0)
    finally:
        if old is None:
            del os.environ["SICP_MATCH_CHUNK"]
        else:
            os.environ["SICP_MATCH_CHUNK"] = old


def test_match_nan_and_overflowing_rows_never_win(ctx):
    rng = np.random.default_rng(9)
    q = rng.uniform(0, 1, (200, 33)).astype(np.float32)
    t = rng.uniform(0, 1, (400, 33)).astype(np.float32)
    t[7] = np.nan
    t[100, 3] = np.nan
    t[200, 0] = 3e38                                                  # the square overflows
    t[201] = -3e38
    t[202, 32] = np.inf
    q[50] = np.nan                                                    # unmatched: every distance is NaN
    q[51, 32] = np.nan
    q[52, 0] = -3e38                                                  # every square overflows
    idx, d2 = check_match(ctx, q, t)
    assert idx[50] == idx[51] == idx[52] == -1 and np.isposinf(d2[[50, 51, 52]]).all()
    assert not set(idx.tolist()) & {7, 100, 200, 201, 202}
    only_bad = np.ascontiguousarray(t[[7, 200, 202]])
    idx, d2 = check_match(ctx, q, only_bad)
    assert np.all(idx == -1) and np.isposinf(d2).all()


def test_match_host_and_device_memory_give_the_same_bits(ctx):
    from simpleicp_amd import _lib
    rng = np.random.default_rng(21)
    q = rng.uniform(0, 1, (333, 33)).astype(np.float32)
    t = rng.uniform(0, 1, (777, 33)).astype(np.float32)
    ridx, rd2, rec = global_ref.match(q, t)
    qd, td = torch.tensor(q, device=DEV), torch.tensor(t, device=DEV)
    L, P = _lib.load(), _lib._ptr
    for q_dev, t_dev, i_dev, d_dev in itertools.product((False, True), repeat=4):
        ih, dh = np.full(333, -7, np.int32), np.full(333, -7, np.float32)
        idv, ddv = torch.full((333,), -7, dtype=torch.int32, device=DEV), torch.full((333,), -7.0, dtype=torch.float32, device=DEV)
        st = _lib.MatchStats()
        rc = L.sicp_feature_match(ctx._h, P(qd if q_dev else q), 333, P(td if t_dev else t), 777, 33, P(idv if i_dev else ih),
                                  P(ddv if d_dev else dh), C.byref(st))
        assert rc == _lib.OK, L.sicp_last_error()
        assert np.array_equal(idv.cpu().numpy() if i_dev else ih, ridx), (q_dev, t_dev, i_dev, d_dev)
        assert np.array_equal(u32(ddv.cpu().numpy() if d_dev else dh), u32(rd2)) and st.as_dict() == rec
    # d2_out NULL
    idx, d2, st = ctx.feature_match(q, t, want_d2=False)
    assert d2 is None and np.array_equal(idx, ridx)
    idv = torch.full((333,), -7, dtype=torch.int32, device=DEV)
    ctx.feature_match(qd.data_ptr(), td.data_ptr(), 333, 777, 33, idx_ptr=idv.data_ptr())
    assert np.array_equal(idv.cpu().numpy(), ridx)
    assert np.array_equal(u32(qd.cpu().numpy()), u32(q)) and np.array_equal(u32(td.cpu().numpy()), u32(t))        # inputs left alone


def test_match_features_mutual_against_the_reference(fpfh_rows):
    import simpleicp_amd
    q, t = fpfh_rows
    want = global_ref.mutual(global_ref.match(q, t)[0], global_ref.match(t, q)[0])
    got = simpleicp_amd.match_features(q, t, mutual=True)
    assert got.dtype == np.int64 and np.array_equal(got, want) and 0 < (want >= 0).sum() < len(q)
    gd, d2 = simpleicp_amd.match_features(torch.tensor(q, device=DEV), torch.tensor(t, device=DEV), mutual=True, return_distance=True)
    assert isinstance(gd, torch.Tensor) and gd.dtype == torch.int64 and gd.device.type == "cuda"
    assert np.array_equal(gd.cpu().numpy(), want) and np.array_equal(u32(d2.cpu().numpy()), u32(global_ref.match(q, t)[1]))
    V = torch.tensor(np.hstack([q, q]), device=DEV)[:, :33]           # a strided view
    assert not V.is_contiguous() and np.array_equal(simpleicp_amd.match_features(V, torch.tensor(t, device=DEV)).cpu().numpy(),
                                                    global_ref.match(q, t)[0])


def test_match_refusals_leave_the_context_usable(ctx):
    from simpleicp_amd import _lib
    L, P = _lib.load(), _lib._ptr
    q = np.random.default_rng(1).uniform(0, 1, (10, 33)).astype(np.float32)
    idx, st = np.full(10, -7, np.int32), _lib.MatchStats()

    def raw(query=q, nq=10, target=q, nt=10, dim=33, out=idx, stats=st):
        return L.sicp_feature_match(ctx._h, P(query), nq, P(target), nt, dim, P(out), None, None if stats is None else C.byref(stats))

    def refused(rc, word):
        assert rc == _lib.ERR_INVALID and word in L.sicp_last_error().decode(), (rc, L.sicp_last_error())
        assert np.all(idx == -7)

    refused(raw(query=None), "query")
    refused(raw(target=None), "target")
    refused(raw(out=None), "idx_out")
    refused(raw(stats=None), "out is null")
    refused(raw(nq=0), "nq")
    refused(raw(nt=0), "nt")
    refused(raw(nt=2**31), "nt")
    for d in (0, -1, 65):
        refused(raw(dim=d), "dim")
    ctx.set_exchange(lambda *a: 0, 0, 1)
    try:
        refused(raw(), "not supported with an exchange")
    finally:
        ctx.set_exchange(None, 0, 1)
    assert raw() == _lib.OK and np.array_equal(idx, np.arange(10))


# ---- RANSAC (R) ----
def check_ransac(ctx, src, dst, tri, max_distance, edge_ratio):
    P, inl, st = ctx.ransac_triplets(src, dst, tri, max_distance, edge_ratio)
    rP, rinl, rec = global_ref.ransac(src, dst, tri, max_distance, edge_ratio)
    print(f"m={len(src)} h={len(tri)} edge_ratio={edge_ratio}: {st.as_dict()}")
    assert inl.dtype == np.int32 and np.array_equal(inl, rinl)
    assert np.array_equal(u64(P), u64(rP))
    assert st.as_dict() == rec
    return P, inl, rec


def noisy_copy(rng, m, wrong=0.4, noise=0.002):
    src = rng.uniform(-1, 1, (m, 3))
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * K @ K
    dst = src @ R.T + np.array([0.3, -0.2, 0.1]) + rng.normal(0, noise, (m, 3))
    bad = rng.choice(m, int(wrong * m), replace=False)
    dst[bad] = rng.uniform(-1, 1, (len(bad), 3))
    return src, dst


@pytest.mark.parametrize("m,h", [(3, 1), (65, 257), (1000, 1000)])
def test_ransac_noisy_rigid_copy(ctx, m, h):
    rng = np.random.default_rng(m + h)
    src, dst = noisy_copy(rng, m, wrong=0.4 if m > 3 else 0.0)
    tri = rng.integers(0, m, (h, 3), dtype=np.int32) if m > 3 else np.array([[2, 0, 1]], np.int32)
    _, inl, rec = check_ransac(ctx, src, dst, tri, 0.02, 0.9)
    if m == 1000:
        assert rec["best_inliers"] > 400 and rec["n_pruned"] > 100 and rec["n_void"] > 0
    if m == 3:
        assert inl[0] == 3


def test_ransac_void_and_pruned_hypotheses(ctx):
    rng = np.random.default_rng(12)
    src, dst = noisy_copy(rng, 40, wrong=0.0, noise=0.0)
    src[10] = src[11]                                                 # coincident source points (their partners are not)
    dst[12] = dst[13] = (1.0, 2.0, 3.0)
    src[12] = src[13]                                                 # coincident on both sides: that pair prunes nothing
    src[20:23] = [[0, 0, 0], [1, 0, 0], [2, 0, 0]]                    # exactly collinear, on both sides
    dst[20:23] = [[0, 5, 0], [0, 6, 0], [0, 7, 0]]
    src[30, 1] = np.nan                                               # a NaN coordinate
    tri = np.array([[0, 1, 2], [1, 1, 2], [0, 2, 2], [5, 4, 5], [-1, 1, 2], [0, 40, 2], [0, 1, 2**31 - 1], [10, 11, 0], [12, 13, 0],
                    [20, 21, 22], [30, 1, 2], [1, 30, 2], [3, 4, 5], [0, 1, 2]], np.int32)
    P, inl, rec = check_ransac(ctx, src, dst, tri, 0.02, 0.0)
    # at edge_ratio 0 nothing is pruned: every degenerate triple reaches the pose and is void there
    assert inl[1:12].tolist() == [-1] * 11 and rec["n_pruned"] == 0 and rec["n_void"] == 11
    # a NaN coordinate outside the triple is simply no inlier: rows 10, 11 (moved), 30 (NaN) and 20..22 are not
    assert inl[0] == inl[12] == inl[13] == 40 - 2 - 1 - 3 - 1 and rec["best"] == 0
    assert not P[1:12].any() and not np.signbit(P[1:12]).any()
    # the same triples at 0.9: the triples with a coincident pair are pruned now (their other edges differ), a NaN still prunes nothing
    _, inl9, rec9 = check_ransac(ctx, src, dst, tri, 0.02, 0.9)
    assert inl9[7] == inl9[8] == -2 and inl9[9] == inl9[10] == inl9[11] == -1 and inl9[0] == inl[0]


def test_ransac_pruned_at_09_valid_at_0(ctx):
    rng = np.random.default_rng(90)
    src = rng.uniform(-1, 1, (80, 3))
    dst = src * rng.uniform(0.5, 2.0, (80, 1)) + 0.1                  # every match stretched by a factor of its own
    tri = rng.integers(0, 80, (300, 3), dtype=np.int32)
    _, inl9, rec9 = check_ransac(ctx, src, dst, tri, 0.3, 0.9)
    _, inl0, rec0 = check_ransac(ctx, src, dst, tri, 0.3, 0.0)
    assert rec9["n_pruned"] > 200 and rec0["n_pruned"] == 0 and rec0["n_void"] == rec9["n_void"]
    assert np.all(inl0[inl9 == -2] >= 0) and np.array_equal(inl0[inl9 >= 0], inl9[inl9 >= 0])
    _, inl1, _ = check_ransac(ctx, src, dst, tri, 0.3, 1.0)           # edge_ratio 1: only exactly congruent triangles pass
    assert np.all(inl1 < 0)


def test_ransac_ties_and_nothing_valid(ctx):
    rng = np.random.default_rng(5)
    src, dst = noisy_copy(rng, 200, wrong=0.3)
    tri = rng.integers(0, 200, (64, 3), dtype=np.int32)
    _, inl, rec = check_ransac(ctx, src, dst, tri, 0.02, 0.9)
    twice = np.ascontiguousarray(np.vstack([tri[:40], tri[rec["best"]][None], tri[40:], tri[rec["best"]][None]]))
    _, inl2, rec2 = check_ransac(ctx, src, dst, twice, 0.02, 0.9)
    assert rec2["best"] == min(rec["best"], 40) and rec2["best_inliers"] == rec["best_inliers"] and (inl2 == rec["best_inliers"]).sum() >= 3
    void = np.array([[0, 0, 1], [5, 5, 5], [-1, 2, 3], [1, 2, 200]], np.int32)
    _, inl, rec = check_ransac(ctx, src, dst, void, 0.02, 0.9)
    assert rec == dict(n_hypotheses=4, n_void=4, n_pruned=0, best=-1, best_inliers=-1)
    # nothing but pruned ones
    _, inl, rec = check_ransac(ctx, src, 3.0 * dst, tri[:7], 0.02, 0.9)
    assert rec["n_pruned"] + rec["n_void"] == 7 and rec["best"] == -1 and rec["best_inliers"] == -1
    # a valid pose without a single inlier is still the best
    _, inl, rec = check_ransac(ctx, src, 3.0 * dst, tri[:7], 1e-9, 0.0)
    assert rec["best_inliers"] >= 0 and rec["best"] == int(np.flatnonzero(inl == inl.max())[0])


def test_ransac_counts_by_the_fused_sum(ctx):
    """A max_distance whose square lies between the fused d2 of contract (D) and the same sum rounded product by product, for a
    row under hypothesis 0: the count of that hypothesis is the fused sum's, one apart from the other."""
    rng = np.random.default_rng(77)
    src, dst = noisy_copy(rng, 2048, wrong=0.3)
    tri = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11], [12, 13, 14], [15, 16, 17], [18, 19, 20], [21, 22, 23]], np.int32)
    verdict, R, t = global_ref.poses(src, dst, tri, 0.0)
    assert verdict[0] == 0
    fused, plain = global_ref.d2_fused_and_plain(R[0], t[0], src, dst)
    md = global_ref.threshold_between(fused, plain)
    assert md is not None and (fused < md * md).sum() != (plain < md * md).sum()
    _, inl, _ = check_ransac(ctx, src, dst, tri, md, 0.0)
    assert inl[0] == (fused < md * md).sum()


def test_ransac_host_and_device_memory_give_the_same_bits(ctx):
    from simpleicp_amd import _lib
    rng = np.random.default_rng(31)
    src, dst = noisy_copy(rng, 300)
    tri = rng.integers(0, 300, (200, 3), dtype=np.int32)
    rP, rinl, rec = global_ref.ransac(src, dst, tri, 0.02, 0.9)
    sd, dd, td = torch.tensor(src, device=DEV), torch.tensor(dst, device=DEV), torch.tensor(tri, device=DEV)
    L, P = _lib.load(), _lib._ptr
    for in_dev, tri_dev, p_dev, i_dev in itertools.product((False, True), repeat=4):
        ph, ih = np.full((200, 12), -7.0), np.full(200, -7, np.int32)
        pd = torch.full((200, 12), -7.0, dtype=torch.float64, device=DEV)
        idv = torch.full((200,), -7, dtype=torch.int32, device=DEV)
        st = _lib.RansacStats()
        rc = L.sicp_ransac_triplets(ctx._h, P(sd if in_dev else src), P(dd if in_dev else dst), 300, P(td if tri_dev else tri), 200, 0.02,
                                    0.9, P(pd if p_dev else ph), P(idv if i_dev else ih), C.byref(st))
        assert rc == _lib.OK, L.sicp_last_error()
        assert np.array_equal(idv.cpu().numpy() if i_dev else ih, rinl), (in_dev, tri_dev, p_dev, i_dev)
        assert np.array_equal(u64(pd.cpu().numpy() if p_dev else ph), u64(rP)) and st.as_dict() == rec
    # poses_out NULL
    poses, inl, st = ctx.ransac_triplets(src, dst, tri, 0.02, 0.9, want_poses=False)
    assert poses is None and np.array_equal(inl, rinl) and st.as_dict() == rec
    idv = torch.full((200,), -7, dtype=torch.int32, device=DEV)
    st = ctx.ransac_triplets(sd.data_ptr(), dd.data_ptr(), td.data_ptr(), 0.02, 0.9, m=300, h=200, inliers_ptr=idv.data_ptr())
    assert np.array_equal(idv.cpu().numpy(), rinl) and st.as_dict() == rec


def test_ransac_refusals_leave_the_context_usable(ctx):
    from simpleicp_amd import _lib
    L, P = _lib.load(), _lib._ptr
    rng = np.random.default_rng(2)
    src, dst = noisy_copy(rng, 20, wrong=0.0)
    tri = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    inl, st = np.full(2, -7, np.int32), _lib.RansacStats()

    def raw(s=src, d=dst, m=20, t=tri, h=2, md=0.02, er=0.9, out=inl, stats=st):
        return L.sicp_ransac_triplets(ctx._h, P(s), P(d), m, P(t), h, md, er, None, P(out), None if stats is None else C.byref(stats))

    def refused(rc, word):
        assert rc == _lib.ERR_INVALID and word in L.sicp_last_error().decode(), (rc, L.sicp_last_error())
        assert np.all(inl == -7)

    refused(raw(s=None), "src")
    refused(raw(d=None), "dst")
    refused(raw(t=None), "triples")
    refused(raw(out=None), "inliers_out")
    refused(raw(stats=None), "out is null")
    refused(raw(m=2), "m ")
    refused(raw(m=2**31), "m ")
    refused(raw(h=0), "h ")
    for md in (0.0, -1.0, float("nan"), float("inf")):
        refused(raw(md=md), "max_distance")
    for er in (-0.1, 1.5, float("nan")):
        refused(raw(er=er), "edge_ratio")
    ctx.set_exchange(lambda *a: 0, 0, 1)
    try:
        refused(raw(), "not supported with an exchange")
    finally:
        ctx.set_exchange(None, 0, 1)
    assert raw() == _lib.OK and np.all(inl == 20)


# ---- the chain on the bundled bunny ----
EXTENT = 263_800.0


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


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_chain_on_the_bunny(bunny_pair, bunny_reference, seed):
    import simpleicp_amd
    A, B, vA, vB, R, t = bunny_pair
    src, dst, n_matches = bunny_reference
    res = simpleicp_amd.register_global(torch.tensor(A, device=DEV), torch.tensor(B, device=DEV), max_distance=10_000.0,
                                        viewpoint_fixed=tuple(vA), viewpoint_movable=tuple(vB), hypotheses=1000, edge_ratio=0.9,
                                        seed=seed, top=4)
    tri = np.random.default_rng(seed).integers(0, n_matches, (1000, 3), dtype=np.int32)
    rP, rinl, rec = global_ref.ransac(src, dst, tri, 10_000.0, 0.9)
    print(f"seed {seed}: {n_matches} matches, {res.stats}")
    assert res.n_matches == n_matches and res.stats == rec and res.index == rec["best"] and res.inliers == rec["best_inliers"]
    order = sorted(np.flatnonzero(rinl >= 0), key=lambda k: (-rinl[k], k))[:4]
    assert [c[2] for c in res.candidates] == order
    for H, inl, k in res.candidates:
        assert np.array_equal(u64(H[:3, :3].ravel()), u64(rP[k, :9])) and np.array_equal(u64(H[:3, 3]), u64(rP[k, 9:])) and inl == rinl[k]
    # the pose maps movable (B) onto fixed (A): the inverse of the motion that made B
    Rt, tt = R.T, -R.T @ t
    dR = res.H[:3, :3] @ Rt.T
    angle = np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1)))
    shift = np.linalg.norm(res.H[:3, 3] - tt)
    print(f"seed {seed}: rotation error {angle:.2f} deg, translation error {shift / EXTENT:.4f} of the extent")
    assert angle < 10.0 and shift < 0.1 * EXTENT
