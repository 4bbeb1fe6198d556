"""Moving-least-squares smoothing on the GPU (contract (W)) against tests/denoise_ref.py: the bytes of the
points, the normals and the displacements and every field of the record -- max_displacement by its bit pattern -- for equality,
on every case.  Every call goes to the C entry with the outputs prefilled with a pattern, and the cloud is compared with its bytes
from before."""
import ctypes as C_
import math
import os
import struct
from contextlib import contextmanager
from functools import lru_cache

import numpy as np
import pytest

import denoise_ref
import iss_ref
import regions_ref
from oracle import orc

pytestmark = pytest.mark.gpu

FILL = -77.0
INF = math.inf


@pytest.fixture(scope="module")
def ctx():
    from simpleicp_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@contextmanager
def context_with(**env):
    """a context created with these switches in the environment (they are read at sicp_ctx_create)"""
    from simpleicp_amd import _lib
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        c = _lib.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    try:
        yield c
    finally:
        c.close()


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits(v):
    return struct.pack("<d", float(v))


def record(ref):
    return {key: ref[key] for key in denoise_ref.KEYS}


def same_record(st, ref):
    assert {k: v for k, v in st.items() if k != "max_displacement"} == {k: v for k, v in record(ref).items() if k != "max_displacement"}
    assert bits(st["max_displacement"]) == bits(ref["max_displacement"]), (st["max_displacement"], ref["max_displacement"])


def call(ctx, X, k, radius=INF, bandwidth=INF, strength=1.0, min_nb=3, upload=True, normals=True, displacement=True):
    """sicp_denoise on X in the fixed slot, host outputs: (points, normals or None, displacement or None, record as a dict)"""
    from simpleicp_amd import _lib
    before = X.tobytes()
    if upload:
        ctx.upload(_lib.FIX, X)
    n = len(X)
    P = np.full((n, 3), FILL)
    N = np.full((n, 3), FILL, np.float32) if normals else None
    G = np.full(n, FILL) if displacement else None
    st = _lib.DenoiseStats()
    ctx._chk(ctx._L.sicp_denoise(ctx._h, _lib.FIX, int(k), float(radius), float(bandwidth), float(strength), int(min_nb), _lib._ptr(P),
                                 _lib._ptr(N), _lib._ptr(G), C_.byref(st)))
    assert X.tobytes() == before
    return P, N, G, st.as_dict()


def same_outputs(P, N, G, st, ref):
    assert np.array_equal(u64(P), u64(ref["points"]))
    assert N is None or np.array_equal(u32(N), u32(ref["normals"]))
    assert G is None or np.array_equal(u64(G), u64(ref["displacement"]))
    same_record(st, ref)


def check(ctx, X, k, radius=INF, bandwidth=INF, strength=1.0, min_nb=3, upload=True, ref=None):
    X = np.ascontiguousarray(X, dtype=np.float64)
    if ref is None:
        ref = denoise_ref.denoise(X, k, None if radius == INF else radius, None if bandwidth == INF else bandwidth, strength, min_nb)
    same_outputs(*call(ctx, X, k, radius, bandwidth, strength, min_nb, upload=upload), ref)
    return ref


# ---- hand cases ----
def test_two_points(ctx):
    ref = check(ctx, np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 2.0]]), 2, min_nb=2)
    assert ref["n_small"] == 0 and ref["n_points"] == 2
    ref = check(ctx, np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 2.0]]), 2, min_nb=3, upload=False)
    assert ref["n_small"] == 2 and not ref["normals"].any()


def test_sixty_four_identical_points(ctx):
    X = np.tile([0.25, -3.0, 7.5], (64, 1))
    ref = check(ctx, X, 16)
    assert np.array_equal(ref["normals"], np.tile(np.float32([0, 0, 1]), (64, 1))) and not ref["displacement"].any()
    assert ref["n_moved"] == 0 and bits(ref["max_displacement"]) == bits(0.0) and np.array_equal(u64(ref["points"]), u64(X))


def test_collinear_points(ctx):
    t = np.random.default_rng(3).uniform(0, 1, 200)
    X = np.ascontiguousarray(np.outer(t, [1.0, 2.0, -0.5]) + [3.0, 1.0, 2.0])
    check(ctx, X, 8)
    check(ctx, np.column_stack([np.arange(100.0), np.zeros(100), np.zeros(100)]), 5)


def test_a_lattice_plane_does_not_move(ctx):
    g = np.arange(12.0)
    X = np.column_stack([np.repeat(g, 12), np.tile(g, 12), np.zeros(144)])
    ref = check(ctx, X, 9)
    assert ref["n_moved"] == 0 and np.array_equal(u64(ref["points"]), u64(X))


def test_exact_duplicates_that_outrank_the_point_itself(ctx):
    rng = np.random.default_rng(12)
    X = rng.uniform(0, 1, (300, 3))
    XX = np.ascontiguousarray(np.concatenate([X, X]))                  # every point twice: the twin with the lower index is rank 0 of both
    idx = orc.knn(XX, XX, k=2)[0]
    assert (idx[300:, 0] == np.arange(300)).all()
    ref = check(ctx, XX, 12)
    assert np.array_equal(u64(ref["points"][:300]), u64(ref["points"][300:]))
    X[10:15] = X[3]                                                    # five copies of one point, in a cloud without twins
    check(ctx, X, 8)


# ---- seams ----
@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257, 1025])
def test_wave_and_block_seams_and_the_padding_of_k(ctx, n):
    """n across the wave and block seams; k across the padding of K and the two-ranks-a-lane path above 64; k = n."""
    from simpleicp_amd import _lib
    X = np.ascontiguousarray(np.random.default_rng(n).uniform(0, 1, (n, 3)) * [1.0, 1.0, 0.1])
    ctx.upload(_lib.FIX, X)
    knn = orc.knn(X, X, k=min(n, 128))
    ks = sorted({k for k in (2, 3, 16, 17, 33, 64, 65, 128, n) if k <= min(n, 128)})
    assert n > 128 or n in ks
    for k in ks:
        same_outputs(*call(ctx, X, k, upload=False), denoise_ref.denoise(X, k, knn=knn))
    b = float(np.sqrt(knn[1][:, ks[-1] - 1].mean()))
    same_outputs(*call(ctx, X, ks[-1], bandwidth=b, upload=False), denoise_ref.denoise(X, ks[-1], bandwidth=b, knn=knn))


@pytest.fixture(scope="module")
def two_thousand():
    X = regions_ref.noisy_box(78, 2100)
    d2 = orc.knn(X, X, k=12)[1]
    kw = dict(radius=float(np.sqrt(np.quantile(d2[:, -1], 0.7))), bandwidth=float(np.sqrt(np.quantile(d2[:, -1], 0.9))), min_nb=9)
    return X, kw, denoise_ref.denoise(X, 12, kw["radius"], kw["bandwidth"], 1.0, kw["min_nb"])


def test_the_two_thousand_are_a_real_case(two_thousand):
    ref = two_thousand[2]
    assert 0 < ref["n_small"] < 2100 and 0 < ref["n_clipped"] < 2100 and ref["n_moved"] == 2100 - ref["n_small"]
    assert ref["max_displacement"] > 0.004


@pytest.mark.parametrize("chunk", [None, 64, 1000])
def test_chunks_give_the_bytes_of_one(two_thousand, chunk):
    X, kw, ref = two_thousand
    with context_with(**({} if chunk is None else {"SICP_DENOISE_CHUNK": chunk})) as c:
        check(c, X, 12, ref=ref, **kw)


# ---- radius, bandwidth, min_neighbors, strength ----
def lattice(n):
    g = np.arange(n, dtype=np.float64)
    return np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))


def test_a_distance_of_exactly_the_radius_does_not_count(ctx):
    X = lattice(5)
    X[:, 2] += 0.125 * ((X[:, 0] + X[:, 1]) % 2)                      # (dyadic: the distances stay exact; the planes are not the lattice's)
    d2 = orc.knn(X, X, k=40)[1]
    assert (d2 == 4.0).any()
    at = check(ctx, X, 40, radius=2.0, min_nb=5)
    past = check(ctx, X, 40, radius=float(np.nextafter(2.0, 3.0)), min_nb=5, upload=False)
    assert not np.array_equal(u64(at["points"]), u64(past["points"]))
    clip = check(ctx, X, 7, radius=2.0, upload=False)                  # balls that hold more than k points
    assert clip["n_clipped"] > 0 and at["n_clipped"] == 0
    assert check(ctx, X, 7, upload=False)["n_clipped"] == 0           # +inf: never clipped


def test_bandwidth_with_t_exactly_zero_and_below(ctx):
    A = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 0.25)])
    A[:, 2] += np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0625, 0.0, 0.03125])
    B = np.ascontiguousarray(np.vstack([A, [[3.0, 0.0, 0.0]]]))
    d2 = orc.knn(B, B, k=9)[1]
    assert (d2[:8, 8] == 4.0).sum() == 1 and (d2[:8, 8] > 4.0).sum() == 7
    with_far = check(ctx, B, 9, bandwidth=2.0)
    without = check(ctx, np.ascontiguousarray(A), 8, bandwidth=2.0)
    assert np.array_equal(u64(with_far["points"][:8]), u64(without["points"])) and without["n_moved"] > 0
    X = np.random.default_rng(21).uniform(0, 1, (500, 3))
    check(ctx, X, 20, bandwidth=0.15)                                  # many ranks beyond the bandwidth
    check(ctx, X, 20, radius=0.2, bandwidth=0.15, upload=False)
    check(ctx, X, 20, radius=0.1, bandwidth=0.15, upload=False)


def test_min_neighbors_at_m_and_above(ctx):
    X = np.random.default_rng(9).uniform(0, 1, (300, 3))
    r = 0.17
    m = (orc.knn(X, X, k=12)[1] < r * r).sum(axis=1)
    target = int(np.median(m))
    assert 4 <= target < 12
    at = check(ctx, X, 12, radius=r, min_nb=target)
    above = check(ctx, X, 12, radius=r, min_nb=target + 1, upload=False)
    assert at["n_small"] == (m < target).sum() and above["n_small"] == (m <= target).sum() > at["n_small"]
    just = np.flatnonzero(m == target)
    assert at["displacement"][just].any() and not above["displacement"][just].any() and not above["normals"][just].any()
    assert np.array_equal(u64(above["points"][just]), u64(X[just]))


@pytest.mark.parametrize("strength", [0.0, 0.5, 1.0])
def test_strength(ctx, strength):
    X = regions_ref.noisy_can(5, 700)
    ref = check(ctx, X, 14, strength=strength)
    if strength == 0.0:
        assert np.array_equal(u64(ref["points"]), u64(X)) and ref["n_moved"] == 0 and ref["normals"].any()


# ---- seeded clouds ----
RANDOM_SEEDS = list(range(800, 830))


@lru_cache(maxsize=None)
def random_case(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1500, 2501))
    X = (regions_ref.noisy_box, regions_ref.noisy_can)[seed % 2](seed, n)
    k = int(rng.integers(6, 41))
    d2 = orc.knn(X, X, k=k)[1]
    kw = dict(strength=float(rng.choice([1.0, 1.0, 0.75])), min_nb=int(rng.integers(1, 7)))
    if (seed // 2) % 2 == 0:
        kw["radius"] = float(np.sqrt(np.quantile(d2[:, -1], 0.7)))
    if (seed // 4) % 2 == 0:
        kw["bandwidth"] = float(np.sqrt(np.quantile(d2[:, -1], rng.uniform(0.5, 1.0))))
    return X, k, kw


@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_seeded_noisy_boxes_and_cans(ctx, seed):
    X, k, kw = random_case(seed)
    ref = check(ctx, X, k, **kw)
    assert ref["n_moved"] > 0.9 * (len(X) - ref["n_small"])


def test_georeferenced_offsets(ctx):
    X = regions_ref.noisy_box(31, 1500) + np.array([5e5, -5e5, 5e5])
    ref = check(ctx, X, 16)
    local = denoise_ref.denoise(X - np.array([5e5, -5e5, 5e5]), 16)
    assert np.abs(ref["displacement"] - local["displacement"]).max() < 1e-6    # (the centred sums keep the offset out of the plane)
    check(ctx, X, 16, radius=0.08, bandwidth=0.1, upload=False)


# ---- roads ----
def test_host_and_device_outputs_with_the_nullable_ones_null_and_given(ctx, two_thousand):
    import torch
    from simpleicp_amd import _lib
    X, kw, ref = two_thousand
    a = (12, kw["radius"], kw["bandwidth"], 1.0, kw["min_nb"])
    for normals in (False, True):
        for displacement in (False, True):
            same_outputs(*call(ctx, X, *a, normals=normals, displacement=displacement), ref)
    dev = torch.device("cuda", 0)
    for normals in (False, True):
        for displacement in (False, True):
            P = torch.full((2100, 3), FILL, dtype=torch.float64, device=dev)
            N = torch.full((2100, 3), FILL, dtype=torch.float32, device=dev) if normals else None
            G = torch.full((2100,), FILL, dtype=torch.float64, device=dev) if displacement else None
            torch.cuda.synchronize()
            st = ctx.denoise(_lib.FIX, *a, points_ptr=P.data_ptr(), normals_ptr=None if N is None else N.data_ptr(),
                             displacement_ptr=None if G is None else G.data_ptr())
            same_outputs(P.cpu().numpy(), None if N is None else N.cpu().numpy(), None if G is None else G.cpu().numpy(), st.as_dict(), ref)
    # mixed: device points, host displacement; and the binding's host form
    P = torch.full((2100, 3), FILL, dtype=torch.float64, device=dev)
    G = np.full(2100, FILL)
    torch.cuda.synchronize()
    st = ctx.denoise(_lib.FIX, *a, points_ptr=P.data_ptr(), displacement_ptr=G.ctypes.data)
    same_outputs(P.cpu().numpy(), None, G, st.as_dict(), ref)
    pts, nrm, disp, st = ctx.denoise(_lib.FIX, *a)
    assert nrm is None and disp is None and pts.shape == (2100, 3)
    same_outputs(pts, None, None, st.as_dict(), ref)
    same_outputs(*ctx.denoise(_lib.FIX, *a, want_normals=True, want_displacement=True)[:3], st.as_dict(), ref)


def test_a_strided_float32_tensor_and_three_rounds_through_denoise_points(two_thousand):
    import torch
    import simpleicp_amd
    X, kw, _ = two_thousand
    X32 = X.astype(np.float32)
    X64 = X32.astype(np.float64)
    want = dict(neighbors=12, radius=kw["radius"], bandwidth=kw["bandwidth"], min_neighbors=kw["min_nb"])
    ref = denoise_ref.denoise(X64, **want)
    wide = torch.zeros((2100, 7), dtype=torch.float32, device="cuda:0")
    wide[:, 1:6:2] = torch.from_numpy(X32).to("cuda:0")
    view = wide[:, 1:6:2]
    assert not view.is_contiguous()
    P, N, G, info = simpleicp_amd.denoise_points(view, return_normals=True, return_displacement=True, return_info=True, **want)
    assert P.is_cuda and P.dtype == torch.float64 and N.dtype == torch.float32 and G.dtype == torch.float64 and tuple(P.shape) == (2100, 3)
    assert info.pop("rounds") == 1
    same_outputs(P.cpu().numpy(), N.cpu().numpy(), G.cpu().numpy(), info, ref)
    assert view.cpu().numpy().tobytes() == X32.tobytes()
    alone = simpleicp_amd.denoise_points(view, **want)
    assert isinstance(alone, torch.Tensor) and torch.equal(alone, P)
    host = simpleicp_amd.denoise_points(X32, return_displacement=True, **want)
    assert isinstance(host[0], np.ndarray) and host[0].dtype == np.float64
    assert np.array_equal(u64(host[0]), u64(ref["points"])) and np.array_equal(u64(host[1]), u64(ref["displacement"]))
    # three rounds against three reference rounds, on both roads and through a PointCloud
    ref3 = denoise_ref.denoise_rounds(X64, rounds=3, **want)
    for src in (view, X64, simpleicp_amd.PointCloud(X64, columns=["x", "y", "z"])):
        P, N, G, info = simpleicp_amd.denoise_points(src, rounds=3, return_normals=True, return_displacement=True, return_info=True, **want)
        assert info.pop("rounds") == 3
        if isinstance(P, torch.Tensor):
            P, N, G = P.cpu().numpy(), N.cpu().numpy(), G.cpu().numpy()
        same_outputs(P, N, G, info, ref3)
    assert not np.array_equal(u64(ref3["points"]), u64(ref["points"]))
    empty = simpleicp_amd.denoise_points(torch.zeros((0, 3), device="cuda:0"), return_normals=True, return_info=True)
    assert empty[0].shape == (0, 3) and empty[0].dtype == torch.float64 and empty[0].is_cuda and empty[1].shape == (0, 3)
    assert empty[2] == dict(n_points=0, n_small=0, n_moved=0, n_clipped=0, max_displacement=0.0, rounds=1)
    with pytest.raises(ValueError, match="neighbors"):
        simpleicp_amd.denoise_points(view[:5], neighbors=6)


def test_the_same_bytes_again_and_behind_other_calls(ctx, two_thousand):
    from simpleicp_amd import _lib
    X, kw, ref = two_thousand
    a = (12, kw["radius"], kw["bandwidth"], 1.0, kw["min_nb"])
    first = call(ctx, X, *a)
    same_outputs(*first, ref)
    again = call(ctx, X, *a, upload=False)
    ctx.keypoints(_lib.FIX, 16, want_saliency=True)
    third = call(ctx, X, *a, upload=False)
    N = orc.normals(X, orc.knn(X, X, k=10)[0])[0]
    ctx.regions(_lib.FIX, N, 12, 0.98)
    fourth = call(ctx, X, *a, upload=False)
    ctx.upload(_lib.MOV, X + np.array([0.01, -0.02, 0.015]))
    Q = np.arange(0, 2100, 2, dtype=np.int64)
    nv, pl = ctx.estimate_normals(_lib.FIX, Q, 10)
    ctx.icp_setup(Q, nv, pl)
    ctx.icp_run(np.zeros(6), np.zeros(6), np.zeros(6), 0.0, None, 5, 0.0, 0)
    fifth = call(ctx, X, *a, upload=False)
    for x in (again, third, fourth, fifth):
        assert all(p.tobytes() == q.tobytes() for p, q in zip(x[:3], first[:3])) and x[3] == first[3]


def test_keypoints_and_regions_are_what_their_references_say_behind_a_denoise_call(ctx):
    """sicp_denoise stages its host outputs in the keypoints' and the orientation's buffers and counts in the shared counter
    words: both operators are held to their own references behind a call that used them."""
    from simpleicp_amd import _lib
    X = regions_ref.noisy_box(55, 1500)
    ctx.upload(_lib.FIX, X)
    call(ctx, X, 16, upload=False)
    ref = iss_ref.keypoints(X, 24, nms_neighbors=8)
    keep, sal, eig, st = ctx.keypoints(_lib.FIX, 24, k_n=8, want_saliency=True)
    assert np.array_equal(keep, ref["keep"]) and np.array_equal(u64(sal), u64(ref["saliency"])) and np.array_equal(u64(eig), u64(ref["eig"]))
    assert st.as_dict() == {key: ref[key] for key in iss_ref.KEYS}
    call(ctx, X, 16, upload=False)
    N, pl = orc.normals(X, orc.knn(X, X, k=10)[0])
    cm = math.cos(math.radians(10.0))
    rref = regions_ref.regions(X, N, 12, cm, seeds=pl >= 0.6, min_size=20)
    labels, st = ctx.regions(_lib.FIX, N, 12, cm, seeds=pl >= 0.6, min_size=20)
    assert np.array_equal(labels, rref["labels"]) and st.as_dict() == regions_ref.record(rref)


def test_pointcloud_denoise_on_the_bunny():
    from simpleicp_amd import PointCloud
    d = os.path.join(os.path.dirname(__file__), "golden", "data")
    B = np.ascontiguousarray(np.load(os.path.join(d, "bunny_part1.npz"))["q"].astype(np.float64)[::4])
    pc = PointCloud(B, columns=["x", "y", "z"])
    pc["nx"] = 0.5
    pc.select_in_range(B[len(B) // 2][None, :], float(np.ptp(B, axis=0).max()) / 3.0)
    cur = pc.idx_selected
    assert 100 < len(cur) < len(B)
    ref = denoise_ref.denoise_rounds(np.ascontiguousarray(B[cur]), rounds=2, neighbors=12, strength=0.5)
    pc.denoise(neighbors=12, strength=0.5, rounds=2)
    want = B.copy()
    want[cur] = ref["points"]
    assert np.array_equal(u64(pc.X), u64(want)) and np.array_equal(pc.idx_selected, cur) and (pc["nx"] == 0.5).all()
    info = dict(pc.last_denoise_stats)
    assert info.pop("rounds") == 2
    same_record(info, ref)
    assert ref["n_moved"] > 0 and not np.array_equal(u64(want[cur]), u64(B[cur]))


# ---- refusals ----
def test_refusals_name_the_argument_and_leave_the_outputs(ctx, two_thousand):
    from simpleicp_amd import _lib
    X, kw, ref = two_thousand
    ctx.upload(_lib.FIX, X)
    L, F = ctx._L, _lib.FIX
    P, N, G, st = np.full((2100, 3), FILL), np.full((2100, 3), FILL, np.float32), np.full(2100, FILL), _lib.DenoiseStats()

    def refused(c, slot, k, radius, bandwidth, strength, min_nb, pp, sp, word):
        assert L.sicp_denoise(c._h, slot, k, radius, bandwidth, strength, min_nb, pp, _lib._ptr(N), _lib._ptr(G), sp) == _lib.ERR_INVALID
        assert word.encode() in L.sicp_last_error(), L.sicp_last_error()
        assert np.all(P == FILL) and np.all(N == FILL) and np.all(G == FILL)

    pp, sp = _lib._ptr(P), C_.byref(st)
    refused(ctx, F, 12, INF, INF, 1.0, 3, None, sp, "points_out is null")
    refused(ctx, F, 12, INF, INF, 1.0, 3, pp, None, "out is null")
    for bad in (1, 0, -3):
        refused(ctx, F, bad, INF, INF, 1.0, 3, pp, sp, "k must be >= 2")
    refused(ctx, F, _lib.KEYPOINTS_MAX_K + 1, INF, INF, 1.0, 3, pp, sp, "k must be <=")
    for bad in (0.0, -1.0, math.nan, -INF):
        refused(ctx, F, 12, bad, INF, 1.0, 3, pp, sp, "radius must be > 0")
        refused(ctx, F, 12, INF, bad, 1.0, 3, pp, sp, "bandwidth must be > 0")
    for bad in (math.nan, INF, -INF, -1e-9, 1.0000001):
        refused(ctx, F, 12, INF, INF, bad, 3, pp, sp, "strength must be")
    for bad in (0, -5):
        refused(ctx, F, 12, INF, INF, 1.0, bad, pp, sp, "min_neighbors must be >= 1")
    refused(ctx, 2, 12, INF, INF, 1.0, 3, pp, sp, "slot")
    with _lib.Context(0) as other:
        refused(other, _lib.MOV, 12, INF, INF, 1.0, 3, pp, sp, "empty")
        other.upload(_lib.MOV, X[:10])
        refused(other, _lib.MOV, 11, INF, INF, 1.0, 3, pp, sp, "exceeds the number of points")
        other.upload(_lib.MOV, X, index_base=7)
        refused(other, _lib.MOV, 12, INF, INF, 1.0, 3, pp, sp, "shard")
    ctx.set_exchange(lambda *a: 0, 0, 1)
    try:
        refused(ctx, F, 12, INF, INF, 1.0, 3, pp, sp, "not supported with an exchange")
    finally:
        ctx.set_exchange(None, 0, 1)
    assert L.sicp_denoise(None, F, 12, INF, INF, 1.0, 3, pp, None, None, sp) == _lib.ERR_INVALID and b"null ctx" in L.sicp_last_error()
    with pytest.raises(_lib.BackendError, match="k must be"):
        ctx.denoise(F, 1)
    check(ctx, X, 12, ref=ref, **kw)                                           # and the context still works
