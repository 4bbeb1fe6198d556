"""Consistent normal orientation on the GPU (contract (H)) against tests/orient_ref.py: normals, flipped bytes
and every field of the record for equality, on every case -- the order of the edges is total, so there is no degenerate case to
leave out.  Every call goes to the C entry with outputs prefilled with a pattern, and the cloud is compared with its bytes from
before."""
import ctypes as C_
import math
import os
from contextlib import contextmanager
from functools import lru_cache

import numpy as np
import pytest

import orient_ref

pytestmark = pytest.mark.gpu

FLIP_FILL = 0xAB


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


def call(ctx, X, N, k, viewpoint=None, away_from=None, want_flipped=True, upload=True):
    """sicp_orient on X in the fixed slot: (normals, flipped or None, record as a dict)"""
    from simpleicp_amd import _lib
    before = X.tobytes()
    if upload:
        ctx.upload(_lib.FIX, X)
    n = len(X)
    N = np.ascontiguousarray(N, dtype=np.float32)
    given = N.tobytes()
    out = np.full((n, 3), 7.5, np.float32)
    flipped = np.full(n, FLIP_FILL, np.uint8) if want_flipped else None
    ref = viewpoint if viewpoint is not None else away_from
    ref = None if ref is None else np.ascontiguousarray(ref, dtype=np.float64)
    st = _lib.OrientStats()
    ctx._chk(ctx._L.sicp_orient(ctx._h, _lib.FIX, _lib._ptr(N), int(k), _lib._ptr(ref), 1 if away_from is not None else 0, _lib._ptr(out),
                                _lib._ptr(flipped), C_.byref(st)))
    assert X.tobytes() == before and N.tobytes() == given
    assert flipped is None or set(np.unique(flipped)) <= {0, 1}
    return out, (None if flipped is None else flipped.view(np.bool_)), st.as_dict()


def check(ctx, X, N, k, ref, **kw):
    out, flipped, st = call(ctx, X, N, k, **kw)
    assert np.array_equal(flipped, ref["flipped"])
    assert out.tobytes() == ref["normals"].tobytes()
    assert st == orient_ref.record(ref)
    assert st["n_forest_edges"] == st["n_points"] - st["n_components"]
    assert st["rounds"] <= math.ceil(math.log2(max(len(X), 2))) + 1
    return out, flipped, st


def check_all_roads(ctx, X, N, k):
    """without a reference, towards one and away from one"""
    centre = (X.min(axis=0) + X.max(axis=0)) * 0.5
    idx = orient_ref.lists(X, k)
    for kw in ({}, {"viewpoint": centre}, {"away_from": centre}):
        check(ctx, X, N, k, orient_ref.orient(X, N, k, idx=idx, **kw), **kw)


# ---- hand cases ----
def test_two_points_and_refused_one(ctx):
    from simpleicp_amd import _lib
    X = np.array([[0.0, 0, 0], [1.0, 0, 0]])
    N = np.array([[0.0, 0, 1], [0.0, 0, -1]], np.float32)
    out, f, st = check(ctx, X, N, 2, orient_ref.orient(X, N, 2))
    assert f.tolist() == [False, True] and st["n_components"] == 1 and st["rounds"] == 1
    out, f, st = check(ctx, X, N, 2, orient_ref.orient(X, N, 2, viewpoint=(0.0, 0, -5)), viewpoint=(0.0, 0, -5))
    assert f.tolist() == [True, False] and st["n_components_voted"] == 1
    one = np.zeros((1, 3))                                                     # n = 1: no k with 2 <= k <= n
    ctx.upload(_lib.FIX, one)
    with pytest.raises(_lib.BackendError, match="exceeds the number of points"):
        ctx.orient(_lib.FIX, np.array([[0.0, 0, 1]], np.float32), 2)


def test_identical_normals_tie_every_weight(ctx):
    X, _ = orient_ref.sphere(3, 300)
    N = np.tile(np.array([0.6, 0.0, 0.8], np.float32), (300, 1))
    N[::3] *= -1
    ref = orient_ref.orient(X, N, 6)
    out, f, st = check(ctx, X, N, 6, ref)
    negated = np.arange(300) % 3 == 0
    assert np.array_equal(f, negated ^ negated[ref["component"]])             # whatever the forest: the anchor's side wins
    check_all_roads(ctx, X, N, 6)


def test_axis_aligned_normals_with_zero_and_negative_zero_dots(ctx):
    rng = np.random.default_rng(4)
    X = rng.uniform(0, 1, (200, 3))
    axes = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [-0.0, -1.0, -1.0], [0, 0, 1.0], [-1.0, 0, 0], [-0.0, -2.0, 0.0]], np.float32)
    N = axes[rng.integers(0, len(axes), 200)]
    lo, hi, s = orient_ref.graph(orient_ref.lists(X, 5), N.astype(np.float64))
    assert (s == 0.0).any() and np.signbit(s[s == 0.0]).any() and (~np.signbit(s[s == 0.0])).any()
    check_all_roads(ctx, X, N, 5)


def test_void_normals_stand_alone_and_never_flip(ctx):
    X, T = orient_ref.sphere(5, 400)
    N, _ = orient_ref.coin(6, T)
    N[7] = (np.nan, 0.0, 1.0)
    N[8] = (0.0, 0.0, 0.0)
    N[9] = (np.inf, 1.0, 0.0)
    N[10] = (-0.0, 0.0, -0.0)
    centre = np.zeros(3)
    for kw in ({}, {"viewpoint": centre}, {"away_from": centre}):
        ref = orient_ref.orient(X, N, 8, **kw)
        assert ref["n_void"] == 4 and ref["n_components"] >= 5
        out, f, st = check(ctx, X, N, 8, ref, **kw)
        assert not f[7:11].any() and out[7:11].tobytes() == N[7:11].tobytes()


def test_sixty_four_identical_points(ctx):
    X = np.full((64, 3), 2.5)
    N, _ = orient_ref.coin(7, np.tile(np.array([0.0, 1.0, 0.0]), (64, 1)))
    for k in (2, 16, 64):
        check_all_roads(ctx, X, N, k)


def test_k_two_and_k_n(ctx):
    X, T = orient_ref.torus(8, 90)
    N, _ = orient_ref.coin(9, T)
    check_all_roads(ctx, X, N, 2)
    check_all_roads(ctx, X, N, 90)


def test_two_far_patches_keep_their_anchors(ctx):
    A, TA = orient_ref.sphere(10, 150)
    B, TB = orient_ref.sphere(11, 150, centre=(200.0, 0.0, 0.0))
    p = np.random.default_rng(12).permutation(300)
    X = np.ascontiguousarray(np.vstack([A, B])[p])
    N, _ = orient_ref.coin(13, np.vstack([TA, TB])[p])
    ref = orient_ref.orient(X, N, 8)
    assert ref["n_components"] == 2
    out, f, st = check(ctx, X, N, 8, ref)
    for a in np.unique(ref["component"]):
        assert not f[a] and a == np.flatnonzero(ref["component"] == a)[0]     # the lowest index of each keeps its sign
    check_all_roads(ctx, X, N, 8)


# ---- group, wave and block seams ----
@pytest.mark.parametrize("n", [15, 16, 17, 63, 64, 65, 255, 257, 1025, 4097])
def test_wave_and_block_seams(ctx, n):
    X, T = orient_ref.surface(100 + n, n)
    N, _ = orient_ref.coin(200 + n, T)
    ref = orient_ref.orient(X, N, 8, away_from=(0.0, 0.0, -10.0))
    check(ctx, X, N, 8, ref, away_from=(0.0, 0.0, -10.0))


@pytest.mark.parametrize("k", [2, 3, 16, 17, 33])
def test_list_lengths(ctx, k):
    X, T = orient_ref.surface(300 + k, 700)
    N, _ = orient_ref.coin(400 + k, T)
    check_all_roads(ctx, X, N, k)


# ---- one long path ----
@pytest.mark.parametrize("order", ["shuffled", "ascending", "descending"])
def test_one_long_path(ctx, order):
    """100 200 lattice points on a line at k = 3, the true normals all (0, 0, 1): every weight ties, so the order falls to the
    indices -- given ascending, every point's first edge goes to its predecessor and one round hooks a chain as long as the
    cloud.  Whatever the forest, every edge disagrees iff the coins of its ends differ, so a point is flipped iff its coin
    differs from the coin of point 0, the anchor."""
    n = 100_200
    pos = np.arange(n, dtype=np.float64)
    if order == "shuffled":
        pos = pos[np.random.default_rng(31).permutation(n)]
    elif order == "descending":
        pos = pos[::-1]
    X = np.ascontiguousarray(np.column_stack([pos, np.zeros(n), np.zeros(n)]))
    N, coin = orient_ref.coin(32, np.tile(np.array([0.0, 0.0, 1.0]), (n, 1)))
    out, f, st = call(ctx, X, N, 3)
    want = coin ^ coin[0]
    assert np.array_equal(f, want) and out.tobytes() == np.where(want[:, None], -N, N).tobytes()
    assert st["rounds"] <= math.ceil(math.log2(n)) + 1
    st.pop("rounds")
    assert st == dict(n_points=n, n_void=0, n_components=1, n_forest_edges=n - 1, n_flipped=int(want.sum()), n_components_voted=0)
    out, f, st = call(ctx, X, N, 3, viewpoint=(0.0, 0.0, -1.0), upload=False)  # every point looks down then
    assert np.array_equal(f, ~coin) and st["n_components_voted"] == int(not coin[0])


# ---- a thousand small patches ----
def test_a_thousand_patches_count_over_more_than_one_block(ctx):
    X, N = orient_ref.patches()
    ref = orient_ref.orient(X, N, 3)
    assert ref["n_components"] == 1000
    check(ctx, X, N, 3, ref)
    far = (0.0, 0.0, 1e4)
    ref = orient_ref.orient(X, N, 3, viewpoint=far)
    assert 300 < ref["n_components_voted"] < 700
    out, f, st = check(ctx, X, N, 3, ref, viewpoint=far)
    assert (out[:, 2] > 0).all()


# ---- lists across chunks, cell order ----
@pytest.fixture(scope="module")
def two_thousand():
    X, T = orient_ref.torus(77, 2000)
    N, _ = orient_ref.coin(78, T + np.random.default_rng(79).normal(0, 0.05, T.shape))
    return X, N, orient_ref.orient(X, N, 12, away_from=(0.0, 0.0, 0.0))


@pytest.mark.parametrize("chunk", [None, 64, 1000])
def test_lists_cross_chunk_boundaries(two_thousand, chunk):
    X, N, ref = two_thousand
    with context_with(**({} if chunk is None else {"SICP_ORIENT_CHUNK": chunk})) as c:
        check(c, X, N, 12, ref, away_from=(0.0, 0.0, 0.0))


def test_cell_order_changes_no_byte(two_thousand):
    X, N, ref = two_thousand
    got = []
    for q in (1, 0):
        with context_with(SICP_ORDER_MIN_Q=q, SICP_ORIENT_CHUNK=700) as c:
            got.append(check(c, X, N, 12, ref, away_from=(0.0, 0.0, 0.0)))
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1].tobytes() == got[1][1].tobytes() and got[0][2] == got[1][2]


# ---- seeded random ----
RANDOM_SEEDS = list(range(500, 530))


@lru_cache(maxsize=None)
def random_case(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(50, 3001))
    shape = (orient_ref.sphere, orient_ref.torus, orient_ref.surface)[seed % 3]
    X, T = shape(seed, n)
    X = X + rng.normal(0, 0.01, X.shape)
    N = T + rng.normal(0, 0.1, T.shape)
    if seed % 4 == 0:                              # duplicated points, normals quantised to few values: ties are common
        X[rng.integers(0, n, n // 5)] = X[rng.integers(0, n, n // 5)]
        N = np.round(N * 2.0) / 2.0
    N = orient_ref.coin(seed + 1000, N)[0]
    k = int(rng.integers(2, min(n, 24) + 1))
    centre = (X.min(axis=0) + X.max(axis=0)) * 0.5
    kw = ({}, {"viewpoint": centre}, {"away_from": centre})[(seed // 3) % 3]
    return np.ascontiguousarray(X), N, k, kw, orient_ref.orient(X, N, k, **kw)


@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_seeded_random_clouds(ctx, seed):
    X, N, k, kw, ref = random_case(seed)
    check(ctx, X, N, k, ref, **kw)


# ---- roads ----
def test_device_outputs_aliasing_and_a_null_flipped(ctx, two_thousand):
    import torch
    from simpleicp_amd import _lib
    X, N, ref = two_thousand
    ctx.upload(_lib.FIX, X)
    dev = torch.device("cuda", 0)
    out = torch.full((2000, 3), 7.5, dtype=torch.float32, device=dev)
    flipped = torch.full((2000,), FLIP_FILL, dtype=torch.uint8, device=dev)
    nd = torch.from_numpy(N).to(dev)
    torch.cuda.synchronize()
    st = ctx.orient(_lib.FIX, nd, 12, reference=(0.0, 0.0, 0.0), away=True, normals_ptr=out.data_ptr(), flipped_ptr=flipped.data_ptr())
    assert out.cpu().numpy().tobytes() == ref["normals"].tobytes() and np.array_equal(flipped.cpu().numpy().astype(bool), ref["flipped"])
    assert st.as_dict() == orient_ref.record(ref) and nd.cpu().numpy().tobytes() == N.tobytes()
    # normals_out aliasing the input, on the device and on the host; flipped_out NULL
    st = ctx.orient(_lib.FIX, nd, 12, reference=(0.0, 0.0, 0.0), away=True, normals_ptr=nd.data_ptr())
    assert nd.cpu().numpy().tobytes() == ref["normals"].tobytes() and st.as_dict() == orient_ref.record(ref)
    mine = N.copy()
    st = ctx.orient(_lib.FIX, mine, 12, reference=(0.0, 0.0, 0.0), away=True, normals_ptr=mine.ctypes.data)
    assert mine.tobytes() == ref["normals"].tobytes() and st.as_dict() == orient_ref.record(ref)
    o, f, st = call(ctx, X, N, 12, away_from=(0.0, 0.0, 0.0), want_flipped=False, upload=False)
    assert f is None and o.tobytes() == ref["normals"].tobytes() and st == orient_ref.record(ref)
    # a host normals_out with a device flipped_out, and the binding's host form
    host = np.full((2000, 3), 7.5, np.float32)
    flipped.fill_(FLIP_FILL)
    torch.cuda.synchronize()
    st = ctx.orient(_lib.FIX, N, 12, reference=(0.0, 0.0, 0.0), away=True, normals_ptr=host.ctypes.data, flipped_ptr=flipped.data_ptr())
    assert host.tobytes() == ref["normals"].tobytes() and np.array_equal(flipped.cpu().numpy().astype(bool), ref["flipped"])
    o, f, st = ctx.orient(_lib.FIX, N, 12, reference=(0.0, 0.0, 0.0), away=True)
    assert o.tobytes() == ref["normals"].tobytes() and np.array_equal(f, ref["flipped"]) and st.as_dict() == orient_ref.record(ref)


def test_a_strided_float32_tensor_through_orient_normals(two_thousand):
    import torch
    import simpleicp_amd
    X, N, _ = two_thousand
    X32 = X.astype(np.float32)
    ref = orient_ref.orient(X32.astype(np.float64), N, 12, away_from=(0.0, 0.0, 0.0))
    wide = torch.zeros((2000, 7), dtype=torch.float32, device="cuda:0")
    wide[:, 1:6:2] = torch.from_numpy(X32).to("cuda:0")
    view = wide[:, 1:6:2]
    nwide = torch.zeros((2000, 5), dtype=torch.float32, device="cuda:0")
    nwide[:, 1:4] = torch.from_numpy(N).to("cuda:0")
    assert not view.is_contiguous() and not nwide[:, 1:4].is_contiguous()
    out, flipped, info = simpleicp_amd.orient_normals(view, nwide[:, 1:4], neighbors=12, away_from=(0.0, 0.0, 0.0), return_flipped=True,
                                                       return_info=True)
    assert out.is_cuda and out.dtype == torch.float32 and flipped.dtype == torch.bool and flipped.is_cuda
    assert out.cpu().numpy().tobytes() == ref["normals"].tobytes() and np.array_equal(flipped.cpu().numpy(), ref["flipped"])
    assert info == orient_ref.record(ref) and nwide[:, 1:4].cpu().numpy().tobytes() == N.tobytes()
    host = simpleicp_amd.orient_normals(X32, N, neighbors=12, away_from=(0.0, 0.0, 0.0))
    assert isinstance(host, np.ndarray) and host.tobytes() == ref["normals"].tobytes()
    # the library's own normals, on both roads: the same bytes, one component turned outwards
    own_dev, info = simpleicp_amd.orient_normals(view, neighbors=12, away_from=(0.0, 0.0, 0.0), return_info=True)
    own_host = simpleicp_amd.orient_normals(X32, neighbors=12, away_from=(0.0, 0.0, 0.0))
    assert own_dev.cpu().numpy().tobytes() == own_host.tobytes() and info["n_components"] == 1
    T = orient_ref.torus(77, 2000)[1]
    assert ((own_host.astype(np.float64) * T).sum(axis=1) > 0).mean() > 0.99
    empty = simpleicp_amd.orient_normals(torch.zeros((0, 3), device="cuda:0"), return_info=True)
    assert empty[0].shape == (0, 3) and empty[0].dtype == torch.float32 and empty[1] == dict.fromkeys(orient_ref.KEYS, 0)


def test_the_same_bytes_again_and_behind_other_calls(ctx, two_thousand):
    from simpleicp_amd import _lib
    X, N, ref = two_thousand
    kw = dict(away_from=(0.0, 0.0, 0.0))
    first = check(ctx, X, N, 12, ref, **kw)
    again = call(ctx, X, N, 12, upload=False, **kw)
    labels, core, cst = ctx.cluster(_lib.FIX, 0.5, 4)
    third = call(ctx, X, N, 12, upload=False, **kw)
    ctx.upload(_lib.MOV, X + np.array([0.01, -0.02, 0.015]))
    Q = np.arange(0, 2000, 2, dtype=np.int64)
    nv, pl = ctx.estimate_normals(_lib.FIX, Q, 10)
    ctx.icp_setup(Q, nv, pl)
    ctx.icp_run(np.zeros(6), np.zeros(6), np.zeros(6), 0.0, None, 5, 0.0, 0)
    fourth = call(ctx, X, N, 12, upload=False, **kw)
    for x in (again, third, fourth):
        assert x[0].tobytes() == first[0].tobytes() and x[1].tobytes() == first[1].tobytes() and x[2] == first[2]
    l2, c2, cst2 = ctx.cluster(_lib.FIX, 0.5, 4)                               # ... and the clusters are what they were
    assert np.array_equal(l2, labels) and cst2.as_dict() == cst.as_dict()


def test_pointcloud_orient_normals(two_thousand):
    from simpleicp_amd import PointCloud
    from simpleicp_amd.pointcloud import PointCloudException
    X, N, _ = two_thousand
    pc = PointCloud(X, columns=["x", "y", "z"])
    with pytest.raises(PointCloudException, match="normals"):
        pc.orient_normals()
    for j, col in enumerate(("nx", "ny", "nz")):
        pc[col] = N[:, j].astype(np.float64)
    ref = orient_ref.orient(X, N, 12, viewpoint=(0.0, 0.0, 9.0))
    pc.orient_normals(neighbors=12, viewpoint=(0.0, 0.0, 9.0))
    got = np.stack([pc[c].to_numpy() for c in ("nx", "ny", "nz")], axis=1).astype(np.float32)
    assert got.tobytes() == ref["normals"].tobytes() and pc.last_orient_stats == orient_ref.record(ref)


@pytest.fixture(scope="module")
def bunny_pair():
    d = os.path.join(os.path.dirname(__file__), "golden", "data")
    fix = np.load(os.path.join(d, "bunny_part1.npz"))["q"].astype(np.float64)
    mov = np.load(os.path.join(d, "bunny_part2.npz"))["q"].astype(np.float64)
    return np.ascontiguousarray(fix[::4]), np.ascontiguousarray(mov[::4])


def _same(a, b):
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[key], b[key]) for key in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if hasattr(a, "__dict__") and not callable(a):
        return type(a) is type(b) and _same(vars(a), vars(b))
    return (a != a and b != b) or a == b


def test_register_global_without_orient_is_what_it_was_and_with_it_reports_components(bunny_pair):
    import simpleicp_amd
    fix, mov = bunny_pair
    voxel = float(np.ptp(fix, axis=0).max()) / 25.0
    base = simpleicp_amd.register_global(fix, mov, max_distance=voxel, seed=3)
    none = simpleicp_amd.register_global(fix, mov, max_distance=voxel, seed=3, orient=None)
    assert _same(vars(base), vars(none)) and none.n_components is None
    for orient in (16, dict(neighbors=12)):
        res = simpleicp_amd.register_global(fix, mov, max_distance=voxel, seed=3, orient=orient)
        assert len(res.n_components) == 2 and all(isinstance(v, int) and v >= 1 for v in res.n_components)
        assert res.H.shape == (4, 4) and np.isfinite(res.H).all()
    again = simpleicp_amd.register_global(fix, mov, max_distance=voxel, seed=3, orient=16)
    assert _same(vars(again), vars(simpleicp_amd.register_global(fix, mov, max_distance=voxel, seed=3, orient=16)))


# ---- refusals ----
def test_refusals_name_the_argument_and_leave_the_outputs(ctx, two_thousand):
    from simpleicp_amd import _lib
    X, N, ref = two_thousand
    ctx.upload(_lib.FIX, X)
    L, F = ctx._L, _lib.FIX
    out, flipped, st = np.full((2000, 3), 7.5, np.float32), np.full(2000, FLIP_FILL, np.uint8), _lib.OrientStats()
    good = np.zeros(3)

    def refused(c, slot, nrm, k, r, o, sp, word):
        assert L.sicp_orient(c._h, slot, nrm, k, _lib._ptr(r), 0, o, _lib._ptr(flipped), sp) == _lib.ERR_INVALID
        assert word.encode() in L.sicp_last_error(), L.sicp_last_error()
        assert np.all(out == 7.5) and np.all(flipped == FLIP_FILL)

    npx, op, sp = _lib._ptr(N), _lib._ptr(out), C_.byref(st)
    refused(ctx, F, None, 12, good, op, sp, "normals is null")
    refused(ctx, F, npx, 12, good, None, sp, "normals_out")
    refused(ctx, F, npx, 12, good, op, None, "out is null")
    for bad in (1, 0, -3):
        refused(ctx, F, npx, bad, good, op, sp, "k must be >= 2")
    refused(ctx, F, npx, _lib.FPFH_MAX_K + 1, good, op, sp, "k must be <=")
    for bad in ((np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf)):
        refused(ctx, F, npx, 12, np.array(bad, dtype=np.float64), op, sp, "reference")
    refused(ctx, 2, npx, 12, good, op, sp, "slot")
    with _lib.Context(0) as other:
        refused(other, _lib.MOV, npx, 12, good, op, sp, "empty")
        other.upload(_lib.MOV, X[:10])
        refused(other, _lib.MOV, npx, 11, good, op, sp, "exceeds the number of points")
        other.upload(_lib.MOV, X, index_base=7)
        refused(other, _lib.MOV, npx, 12, good, op, sp, "shard")
    ctx.set_exchange(lambda *a: 0, 0, 1)
    try:
        refused(ctx, F, npx, 12, good, op, sp, "not supported with an exchange")
    finally:
        ctx.set_exchange(None, 0, 1)
    assert L.sicp_orient(None, F, npx, 12, None, 0, op, None, sp) == _lib.ERR_INVALID and b"null ctx" in L.sicp_last_error()
    with pytest.raises(_lib.BackendError, match="k must be"):
        ctx.orient(F, N, 1)
    check(ctx, X, N, 12, ref, away_from=(0.0, 0.0, 0.0))                      # and the context still works
