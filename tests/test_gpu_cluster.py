"""DBSCAN labels on the GPU (contract (U)) against tests/cluster_ref.py: labels, core bytes and every field
of the record for equality.  Every call goes to the C entry with outputs prefilled with a pattern, and the cloud is compared with
its bytes from before."""
import ctypes as C_
import os
from contextlib import contextmanager
from functools import lru_cache

import numpy as np
import pytest

import cluster_ref
import outlier_ref

pytestmark = pytest.mark.gpu

LABEL_FILL, CORE_FILL = -77, 0xAB


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


def call(ctx, X, r, mp, want_core=True, upload=True):
    """sicp_cluster on X in the fixed slot: (labels, core or None, record as a dict)"""
    from simpleicp_amd import _lib
    before = X.tobytes()
    if upload:
        ctx.upload(_lib.FIX, X)
    n = len(X)
    labels = np.full(n, LABEL_FILL, np.int32)
    core = np.full(n, CORE_FILL, np.uint8) if want_core else None
    st = _lib.ClusterStats()
    ctx._chk(ctx._L.sicp_cluster(ctx._h, _lib.FIX, float(r), int(mp), _lib._ptr(labels), _lib._ptr(core), C_.byref(st)))
    assert X.tobytes() == before
    assert labels.min() >= -1 and (core is None or set(np.unique(core)) <= {0, 1})
    return labels, (None if core is None else core.view(np.bool_)), st.as_dict()


def check(ctx, X, r, mp, ref):
    labels, core, st = call(ctx, X, r, mp)
    assert np.array_equal(core, ref["core"])
    assert np.array_equal(labels, ref["labels"])
    assert st == cluster_ref.record(ref)
    return labels, core, st


# ---- hand cases ----
def test_hand_cases(ctx):
    one = np.zeros((1, 3))
    l, c, st = check(ctx, one, 1.0, 1, cluster_ref.cluster(one, 1.0, 1))
    assert l.tolist() == [0] and st["n_clusters"] == 1
    l, c, st = check(ctx, one, 1.0, 2, cluster_ref.cluster(one, 1.0, 2))
    assert l.tolist() == [-1] and st["n_noise"] == 1 and st["largest_label"] == -1 and st["largest_size"] == 0
    two = np.array([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0]])
    assert call(ctx, two, 5.0, 2)[0].tolist() == [-1, -1]                     # d2 == r * r: strict
    assert call(ctx, two, np.nextafter(5.0, 6.0), 2)[0].tolist() == [0, 0]
    for r in (5.0, np.nextafter(5.0, 6.0)):
        check(ctx, two, r, 2, cluster_ref.cluster(two, r, 2))
    B = cluster_ref.bridge()
    l, c, st = check(ctx, B, 2.1, 5, cluster_ref.cluster(B, 2.1, 5))
    assert l.tolist() == [0] * 5 + [0] + [1] * 5 and not c[5] and st["n_border"] == 1 and st["n_clusters"] == 2
    Br = np.ascontiguousarray(B[::-1])
    l, c, st = check(ctx, Br, 2.1, 5, cluster_ref.cluster(Br, 2.1, 5))
    assert l.tolist() == [0] * 5 + [0] + [1] * 5 and not c[5]                 # the point at 4 still takes 0: the clusters swapped
    same = np.full((64, 3), 2.5)
    l, c, st = check(ctx, same, 1e-3, 64, cluster_ref.cluster(same, 1e-3, 64))
    assert np.all(l == 0) and c.all() and st["largest_size"] == 64
    check(ctx, same, 1e-3, 65, cluster_ref.cluster(same, 1e-3, 65))
    X = np.array([[0.0, 0, 0], [10.0, 0, 0], [0.5, 0, 0], [20.0, 0, 0], [10.4, 0, 0]])
    l, c, st = check(ctx, X, 1.0, 1, cluster_ref.cluster(X, 1.0, 1))
    assert l.tolist() == [0, 1, 0, 2, 1] and c.all()                          # min_points = 1: an isolated point is a cluster
    l, c, st = check(ctx, X, 100.0, 6, cluster_ref.cluster(X, 100.0, 6))
    assert np.all(l == -1) and st["n_clusters"] == 0                          # min_points > n
    X = np.array([[0.0, 0, 0], [0.1, 0, 0], [0.2, 0, 0], [5.0, 0, 0], [5.1, 0, 0], [5.2, 0, 0], [5.9, 0, 0]])
    l, c, st = check(ctx, X, 0.75, 3, cluster_ref.cluster(X, 0.75, 3))
    assert l.tolist() == [0, 0, 0, 1, 1, 1, 1] and not c[6]                   # a border that sees only the higher label


# ---- group, block and chunk seams ----
def lattice_blobs(seed, n):
    """cluster_ref.blobs on an integer lattice (eight steps per unit): the k-d tree road's distances are exact there"""
    return np.ascontiguousarray(np.round(cluster_ref.blobs(seed, n, n_blobs=1 if n < 100 else 4, noise=0.3) * 8.0))


@pytest.mark.parametrize("n", [15, 16, 17, 63, 64, 65, 255, 257, 4097])
def test_group_and_block_seams(ctx, n):
    X = lattice_blobs(100 + n, n)
    r, mp = 3.3, 4                                                            # r * r = 10.89: no pair of lattice points lies at r
    ref = cluster_ref.cluster_pairs(X, r, mp)
    assert ref["n_core"] > 0 and ref["n_noise"] > 0
    if n <= 2000:
        dense = cluster_ref.cluster(X, r, mp)
        assert np.array_equal(dense["labels"], ref["labels"]) and cluster_ref.record(dense) == cluster_ref.record(ref)
    check(ctx, X, r, mp, ref)


@pytest.fixture(scope="module")
def two_thousand():
    X = cluster_ref.blobs(77, 2000)
    ref = cluster_ref.cluster(X, 0.3, 8)
    assert ref["n_clusters"] >= 2 and ref["n_border"] > 0 and ref["n_noise"] > 0
    return X, ref


@pytest.mark.parametrize("chunk", [None, 64, 1000])
def test_unions_cross_chunk_boundaries(two_thousand, chunk):
    X, ref = two_thousand
    with context_with(**({} if chunk is None else {"SICP_CLUSTER_CHUNK": chunk})) as c:
        check(c, X, 0.3, 8, ref)


def test_cell_order_changes_no_byte(two_thousand):
    X, ref = two_thousand
    got = []
    for q in (1, 0):
        with context_with(SICP_ORDER_MIN_Q=q, SICP_CLUSTER_CHUNK=700) as c:
            got.append(check(c, X, 0.3, 8, ref))
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1].tobytes() == got[1][1].tobytes() and got[0][2] == got[1][2]


# ---- cell seams ----
def test_clusters_across_cell_faces_edges_and_corners(ctx):
    """1 500 cubes of 2 x 2 x 2 lattice points dropped at random lattice positions of a 150-wide box (cubes that touch merge) and
    500 single points: the grid's cells are cubes of a side the library chooses, laid from the cloud's corner; whatever the side,
    cubes at uniformly random offsets lie across its faces, edges and corners by the hundred."""
    rng = np.random.default_rng(23)
    corner = rng.integers(0, 150, (1500, 3)).astype(np.float64)
    cube = np.stack(np.meshgrid([0.0, 1.0], [0.0, 1.0], [0.0, 1.0], indexing="ij"), -1).reshape(-1, 3)
    X = np.vstack([(corner[:, None, :] + cube[None, :, :]).reshape(-1, 3), rng.integers(0, 151, (500, 3)).astype(np.float64)])
    X = np.ascontiguousarray(np.unique(X, axis=0)[rng.permutation(len(np.unique(X, axis=0)))])
    ref = cluster_ref.cluster_pairs(X, 1.25, 4)
    assert ref["n_clusters"] > 1000 and ref["n_noise"] > 100
    check(ctx, X, 1.25, 4, ref)


def test_the_box_limit_is_the_radius_filters(ctx):
    from simpleicp_amd import _lib
    rng = np.random.default_rng(29)
    t = np.sort(rng.uniform(0.0, 100.0, 2000))
    X = np.ascontiguousarray(np.column_stack([t, t, t]) + rng.uniform(-0.2, 0.2, (2000, 3)))      # a jittered space diagonal
    ctx.upload(_lib.FIX, X)
    cells = lambda r: ctx.outlier_radius_cells(_lib.FIX, r)[3]                # noqa: E731
    lo, hi = 1e-3, 400.0
    assert cells(lo) <= _lib.OUTLIER_MAX_BOX_CELLS < cells(hi)
    while np.nextafter(lo, hi) < hi:                                          # the largest radius that is accepted, its neighbour
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if cells(mid) <= _lib.OUTLIER_MAX_BOX_CELLS else (lo, mid)
    assert cells(lo) == _lib.OUTLIER_MAX_BOX_CELLS and cells(hi) > _lib.OUTLIER_MAX_BOX_CELLS
    A = cluster_ref.relation(X, lo)
    mp = int(np.median(A.sum(axis=1)))
    ref = cluster_ref.cluster(X, lo, mp, A)
    assert 0 < ref["n_core"] < 2000
    check(ctx, X, lo, mp, ref)
    labels = np.full(2000, LABEL_FILL, np.int32)
    st = _lib.ClusterStats()
    assert ctx._L.sicp_cluster(ctx._h, _lib.FIX, float(hi), mp, _lib._ptr(labels), None, C_.byref(st)) == _lib.ERR_INVALID
    mine = ctx._L.sicp_last_error()
    assert b"grid cells" in mine and b"at most 4096" in mine and np.all(labels == LABEL_FILL)
    with pytest.raises(_lib.BackendError) as e:
        ctx.outlier_radius(_lib.FIX, float(hi), 3)
    assert str(e.value).encode() == mine                                      # the radius filter's message, word for word
    check(ctx, X, lo, mp, ref)


# ---- union stress ----
@pytest.fixture(scope="module")
def snake():
    return cluster_ref.serpentine()


@pytest.mark.parametrize("order", ["shuffled", "ascending", "descending"])
def test_one_long_chain_hooked_from_everywhere(ctx, snake, order):
    X = snake
    if order == "shuffled":
        X = np.ascontiguousarray(X[np.random.default_rng(31).permutation(len(X))])
    elif order == "descending":
        X = np.ascontiguousarray(X[::-1])
    ref = cluster_ref.cluster_pairs(X, 1.25, 3)
    assert cluster_ref.record(ref) == dict(n_points=100_200, n_core=100_198, n_border=2, n_noise=0, n_clusters=1, largest_label=0,
                                           largest_size=100_200)
    check(ctx, X, 1.25, 3, ref)


def test_a_thousand_patches_rank_over_more_than_one_block(ctx):
    X = cluster_ref.patches()
    ref = cluster_ref.cluster_pairs(X, 1.25, 3)
    assert ref["n_clusters"] == 1000 and ref["n_noise"] > 100
    check(ctx, X, 1.25, 3, ref)


# ---- seeded random ----
# 30 seeds for which the reference alone (checked without a GPU) has at most 3 degenerate cases: 300, 312 and 318 are all noise;
# 309, which has one cluster, gave way to 330
RANDOM_SEEDS = [s for s in range(300, 331) if s != 309]


@lru_cache(maxsize=None)
def random_case(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(150, 2001))
    X = cluster_ref.blobs(seed, n, n_blobs=int(rng.integers(2, 7)), noise=float(rng.uniform(0.1, 0.4)), spread=float(rng.uniform(0.2, 0.5)))
    r, mp = float(rng.uniform(0.15, 0.6)), int(rng.integers(2, 16))
    return X, r, mp, cluster_ref.cluster(X, r, mp)


def degenerate(ref):
    """all noise or one cluster"""
    return ref["n_clusters"] <= 1


@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_seeded_random_clouds(ctx, seed):
    X, r, mp, ref = random_case(seed)
    check(ctx, X, r, mp, ref)


def test_few_of_the_random_clouds_are_degenerate():
    assert len(RANDOM_SEEDS) == 30 and sum(degenerate(random_case(seed)[3]) for seed in RANDOM_SEEDS) <= 3


# ---- roads ----
def test_device_outputs_and_a_null_core(ctx, two_thousand):
    import torch
    from simpleicp_amd import _lib
    X, ref = two_thousand
    ctx.upload(_lib.FIX, X)
    dev = torch.device("cuda", 0)
    labels = torch.full((2000,), LABEL_FILL, dtype=torch.int32, device=dev)
    core = torch.full((2000,), CORE_FILL, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    st = ctx.cluster(_lib.FIX, 0.3, 8, labels_ptr=labels.data_ptr(), core_ptr=core.data_ptr())
    assert np.array_equal(labels.cpu().numpy(), ref["labels"]) and np.array_equal(core.cpu().numpy().astype(bool), ref["core"])
    assert st.as_dict() == cluster_ref.record(ref)
    # a device labels_out with a host core_out, and the other way round
    host_core = np.full(2000, CORE_FILL, np.uint8)
    labels.fill_(LABEL_FILL)
    torch.cuda.synchronize()
    st2 = _lib.ClusterStats()
    ctx._chk(ctx._L.sicp_cluster(ctx._h, _lib.FIX, 0.3, 8, C_.c_void_p(labels.data_ptr()), _lib._ptr(host_core), C_.byref(st2)))
    assert np.array_equal(labels.cpu().numpy(), ref["labels"]) and np.array_equal(host_core.astype(bool), ref["core"])
    host_labels = np.full(2000, LABEL_FILL, np.int32)
    core.fill_(CORE_FILL)
    torch.cuda.synchronize()
    ctx._chk(ctx._L.sicp_cluster(ctx._h, _lib.FIX, 0.3, 8, _lib._ptr(host_labels), C_.c_void_p(core.data_ptr()), C_.byref(st2)))
    assert np.array_equal(host_labels, ref["labels"]) and np.array_equal(core.cpu().numpy().astype(bool), ref["core"])
    assert st2.as_dict() == cluster_ref.record(ref)
    # core_out NULL
    l, c, st3 = call(ctx, X, 0.3, 8, want_core=False, upload=False)
    assert c is None and np.array_equal(l, ref["labels"]) and st3 == cluster_ref.record(ref)
    l, c, st3 = ctx.cluster(_lib.FIX, 0.3, 8)                                 # the binding's host form
    assert np.array_equal(l, ref["labels"]) and np.array_equal(c, ref["core"]) and st3.as_dict() == cluster_ref.record(ref)


def test_a_strided_float32_tensor_through_cluster_labels(two_thousand):
    import torch
    import simpleicp_amd
    X, _ = two_thousand
    X32 = X.astype(np.float32)
    ref = cluster_ref.cluster(X32.astype(np.float64), 0.3, 8)
    wide = torch.zeros((2000, 7), dtype=torch.float32, device="cuda:0")
    wide[:, 1:6:2] = torch.from_numpy(X32).to("cuda:0")
    view = wide[:, 1:6:2]
    assert not view.is_contiguous()
    labels, core, info = simpleicp_amd.cluster_labels(view, 0.3, 8, return_core=True, return_info=True)
    assert labels.is_cuda and labels.dtype == torch.int32 and core.dtype == torch.bool and core.is_cuda
    assert np.array_equal(labels.cpu().numpy(), ref["labels"]) and np.array_equal(core.cpu().numpy(), ref["core"])
    assert info == cluster_ref.record(ref)
    host = simpleicp_amd.cluster_labels(X32, 0.3, 8)                          # the host road's labels
    assert isinstance(host, np.ndarray) and np.array_equal(host, labels.cpu().numpy())
    only = simpleicp_amd.cluster_labels(view, 0.3, 8)
    assert torch.equal(only, labels)
    empty = simpleicp_amd.cluster_labels(torch.zeros((0, 3), device="cuda:0"), 0.3, 8, return_info=True)
    assert empty[0].shape == (0,) and empty[0].dtype == torch.int32 and empty[1] == dict.fromkeys(cluster_ref.KEYS, 0)


def test_the_same_bytes_again_and_behind_other_calls(ctx, two_thousand):
    from simpleicp_amd import _lib
    X, ref = two_thousand
    D2 = outlier_ref.all_d2(X)
    first = check(ctx, X, 0.3, 8, ref)
    again = call(ctx, X, 0.3, 8, upload=False)
    keep, cnt, kept = ctx.outlier_radius(_lib.FIX, 0.3, 6)
    want = outlier_ref.radius(X, 0.3, 6, D2=D2)
    assert np.array_equal(keep, want["keep"]) and np.array_equal(cnt, want["count"]) and kept == want["n_kept"]
    third = call(ctx, X, 0.3, 8, upload=False)
    ctx.upload(_lib.MOV, X + np.array([0.01, -0.02, 0.015]))
    Q = np.arange(0, 2000, 2, dtype=np.int64)
    nv, pl = ctx.estimate_normals(_lib.FIX, Q, 10)
    ctx.icp_setup(Q, nv, pl)
    ctx.icp_run(np.zeros(6), np.zeros(6), np.zeros(6), 0.0, None, 5, 0.0, 0)
    fourth = call(ctx, X, 0.3, 8, upload=False)
    for x in (again, third, fourth):
        assert x[0].tobytes() == first[0].tobytes() and x[1].tobytes() == first[1].tobytes() and x[2] == first[2]
    # ... and the radius filter still gives its reference behind the cluster calls
    keep, cnt, kept = ctx.outlier_radius(_lib.FIX, 0.3, 6)
    assert np.array_equal(keep, want["keep"]) and np.array_equal(cnt, want["count"]) and kept == want["n_kept"]
    rows = np.arange(5, 1500, 7, dtype=np.int64)
    keep, cnt, kept = ctx.outlier_radius(_lib.FIX, 0.25, 3, rows=rows)
    want = outlier_ref.radius(X, 0.25, 3, rows=rows, D2=D2)
    assert np.array_equal(keep, want["keep"]) and np.array_equal(cnt, want["count"]) and kept == want["n_kept"]


def test_pointcloud_selectors_on_the_bunny_with_two_islands():
    from simpleicp_amd import PointCloud
    q = np.load(os.path.join(os.path.dirname(__file__), "golden", "data", "bunny_part1.npz"))["q"].astype(np.float64)
    rng = np.random.default_rng(37)
    body = q[rng.permutation(len(q))[:2400]]
    far = body.max(axis=0) + 0.5 * (body.max(axis=0) - body.min(axis=0))
    step = float(np.median(np.sqrt(outlier_ref.neighbour_d2(body[:1500], 6)[:, 5])))
    islands = [far + rng.uniform(0, 3 * step, (60, 3)), far * np.array([1.0, -1.0, 1.0]) + rng.uniform(0, 2 * step, (30, 3))]
    X = np.ascontiguousarray(np.vstack([body, islands[0], islands[1]]))
    pc = PointCloud(X, columns=["x", "y", "z"])
    pc.select_n_points(1800)                                                  # the selection is a cloud of its own: 1 800 of 2 490 rows
    sel = pc.idx_selected
    r, mp = 2.0 * step, 5
    ref = cluster_ref.cluster(X[sel], r, mp)
    assert ref["n_clusters"] >= 3 and ref["largest_size"] > 1000
    pc.select_largest_cluster(r, mp)
    assert np.array_equal(pc.idx_selected, sel[ref["labels"] == ref["largest_label"]]) and pc.last_cluster_stats == cluster_ref.record(ref)
    assert pc.idx_selected.max() < 2400                                       # the islands are gone
    pc.select_all_points()
    pc.select_n_points(1800)
    sizes = np.bincount(ref["labels"][ref["labels"] >= 0])
    small = int(np.sort(sizes)[-2])                                           # the second largest cluster stays, smaller ones go
    pc.select_clusters(r, mp, min_size=small)
    want = sel[(ref["labels"] >= 0) & (sizes[np.maximum(ref["labels"], 0)] >= small)]
    assert np.array_equal(pc.idx_selected, want) and pc.last_cluster_stats == cluster_ref.record(ref)
    assert len(want) > ref["largest_size"]


# ---- refusals ----
def test_refusals_name_the_argument_and_leave_the_outputs(ctx, two_thousand):
    from simpleicp_amd import _lib
    X, ref = two_thousand
    ctx.upload(_lib.FIX, X)
    L, F = ctx._L, _lib.FIX
    labels, core, st = np.full(2000, LABEL_FILL, np.int32), np.full(2000, CORE_FILL, np.uint8), _lib.ClusterStats()

    def refused(c, slot, r, mp, lp, op, word):
        assert L.sicp_cluster(c._h, slot, r, mp, lp, _lib._ptr(core), op) == _lib.ERR_INVALID
        assert word.encode() in L.sicp_last_error(), L.sicp_last_error()
        assert np.all(labels == LABEL_FILL) and np.all(core == CORE_FILL)

    lp, op = _lib._ptr(labels), C_.byref(st)
    refused(ctx, F, 0.3, 8, None, op, "labels_out")
    refused(ctx, F, 0.3, 8, lp, None, "out is null")
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        refused(ctx, F, bad, 8, lp, op, "radius")
    for bad in (0, -1, -2**40):
        refused(ctx, F, 0.3, bad, lp, op, "min_points")
    refused(ctx, 2, 0.3, 8, lp, op, "slot")
    with _lib.Context(0) as other:
        refused(other, _lib.MOV, 0.3, 8, lp, op, "empty")
        other.upload(_lib.MOV, X, index_base=7)
        refused(other, _lib.MOV, 0.3, 8, lp, op, "shard")
    ctx.set_exchange(lambda *a: 0, 0, 1)
    try:
        refused(ctx, F, 0.3, 8, lp, op, "not supported with an exchange")
    finally:
        ctx.set_exchange(None, 0, 1)
    with pytest.raises(_lib.BackendError, match="radius"):
        ctx.cluster(F, -1.0, 8)
    check(ctx, X, 0.3, 8, ref)                                                # and the context still works
