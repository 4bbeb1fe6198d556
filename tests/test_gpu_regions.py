"""Smooth regions on the GPU (contract (J)) against tests/regions_ref.py: the labels and every field of the
record for equality, on every case.  Every call goes to the C entry with the labels prefilled with a pattern, and the cloud, the
normals and the seeds are compared with their bytes from before."""
import ctypes as C_
import math
import os
from contextlib import contextmanager
from functools import lru_cache

import numpy as np
import pytest

import cluster_ref
import orient_ref
import regions_ref
from oracle import orc

pytestmark = pytest.mark.gpu

FILL = 77
COS5 = math.cos(math.radians(5.0))


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


def call(ctx, X, N, k, cos_min=COS5, radius=math.inf, oriented=False, seeds=None, min_size=1, upload=True):
    """sicp_regions on X in the fixed slot: (labels, record as a dict)"""
    from simpleicp_amd import _lib
    before = X.tobytes()
    if upload:
        ctx.upload(_lib.FIX, X)
    n = len(X)
    N = np.ascontiguousarray(N, dtype=np.float32)
    sd = None if seeds is None else np.ascontiguousarray(np.asarray(seeds) != 0).view(np.uint8)
    given = N.tobytes(), None if sd is None else sd.tobytes()
    labels = np.full(n, FILL, np.int32)
    st = _lib.RegionsStats()
    ctx._chk(ctx._L.sicp_regions(ctx._h, _lib.FIX, _lib._ptr(N), int(k), float(radius), float(cos_min), 1 if oriented else 0, _lib._ptr(sd),
                                 int(min_size), _lib._ptr(labels), C_.byref(st)))
    assert X.tobytes() == before and N.tobytes() == given[0] and (sd is None or sd.tobytes() == given[1])
    return labels, st.as_dict()


def check(ctx, X, N, k, ref=None, upload=True, **kw):
    ref = regions_ref.regions(X, N, k, kw.get("cos_min", COS5), **{a: v for a, v in kw.items() if a != "cos_min"}) if ref is None else ref
    labels, st = call(ctx, X, N, k, upload=upload, **kw)
    assert np.array_equal(labels, ref["labels"])
    assert st == regions_ref.record(ref)
    assert st["n_labelled"] == int((labels >= 0).sum()) and st["n_regions"] == (int(labels.max()) + 1 if st["n_labelled"] else 0)
    return labels, st


UP = np.array([0.0, 0.0, 1.0])


# ---- hand cases ----
def test_two_points(ctx):
    X = np.array([[0.0, 0, 0], [1.0, 0, 0]])
    labels, st = check(ctx, X, [UP, -UP], 2)
    assert labels.tolist() == [0, 0] and st["largest_size"] == 2
    labels, st = check(ctx, X, [UP, -UP], 2, oriented=True)
    assert labels.tolist() == [0, 1] and (st["largest_label"], st["largest_size"]) == (0, 1)
    labels, st = check(ctx, X, [UP, [1.0, 0, 0]], 2)
    assert labels.tolist() == [0, 1]


def test_identical_normals_are_one_region_per_component_of_the_graph(ctx):
    X, _ = orient_ref.sphere(3, 300)
    N = np.tile(np.array([0.6, 0.0, 0.8], np.float32), (300, 1))
    labels, st = check(ctx, X, N, 6)
    check(ctx, X, N, 6, cos_min=1.0, upload=False)                            # s is below 1 by rounding, or is it: the reference says
    N[::3] *= -1
    check(ctx, X, N, 6, upload=False)
    check(ctx, X, N, 6, oriented=True, upload=False)


def test_agreement_of_exactly_cos_min_links_and_the_next_double_does_not(ctx):
    X = np.array([[0.0, 0, 0], [1.0, 0, 0]])
    N = np.array([[1.0, 0, 0], [0.5, 0.8660254, 0]], np.float32)
    for oriented in (False, True):
        labels, st = check(ctx, X, N, 2, cos_min=0.5, oriented=oriented)
        assert labels.tolist() == [0, 0]
        labels, st = check(ctx, X, N, 2, cos_min=np.nextafter(0.5, 1.0), oriented=oriented)
        assert labels.tolist() == [0, 1]


def test_a_negative_zero_agreement_links_at_cos_min_zero(ctx):
    X = np.array([[0.0, 0, 0], [1.0, 0, 0]])
    N = np.array([[-1.0, -1.0, 0.0], [0.0, 0.0, -1.0]], np.float32)                  # every product is -0.0, and so is their sum
    s = regions_ref.agreement(N.astype(np.float64), np.array([0]), np.array([1]), True)
    assert s[0] == 0.0 and np.signbit(s[0])
    for oriented in (False, True):
        assert check(ctx, X, N, 2, cos_min=0.0, oriented=oriented)[0].tolist() == [0, 0]
    assert check(ctx, X, N, 2, cos_min=5e-324)[0].tolist() == [0, 1]


def test_void_normals(ctx):
    X, N, _ = regions_ref.hinge(7, 0.0, m=12)
    N = N.astype(np.float32)
    N[0] = (np.nan, 0, 1)
    N[5] = (0, 0, 0)
    N[9] = (np.inf, 0, 1)
    N[11] = (-0.0, 0.0, -0.0)
    N[40] = (0, -np.inf, 0)
    labels, st = check(ctx, X, N, 6)
    assert st["n_void"] == 5 and (labels[[0, 5, 9, 11, 40]] == -1).all()
    seeds = np.arange(len(X)) % 4 != 1
    check(ctx, X, N, 6, seeds=seeds, upload=False)
    labels, st = check(ctx, X, np.full((len(X), 3), np.nan), 6, upload=False)
    assert st["n_void"] == len(X) and st["n_regions_all"] == 0 and (labels == -1).all()


def test_sixty_four_identical_points(ctx):
    X = np.full((64, 3), 2.5)
    N = np.tile(UP, (64, 1)).astype(np.float32)
    N[1::2] = (1.0, 0, 0)
    for k in (2, 16, 64):
        check(ctx, X, N, k)
        check(ctx, X, N, k, radius=1.0, seeds=np.arange(64) % 3 != 0, upload=False)


def test_k_two_and_k_n(ctx):
    X, T = orient_ref.torus(8, 90)
    check(ctx, X, T, 2, cos_min=0.9)
    check(ctx, X, T, 90, cos_min=0.9, upload=False)
    check(ctx, X, T, 90, cos_min=0.9, radius=0.8, seeds=np.arange(90) % 5 != 0, upload=False)


def test_a_distance_of_exactly_the_radius_is_no_edge(ctx):
    X = np.array([[0.0, 0, 0], [3.0, 4.0, 0]])                                 # d2 = 25 exactly
    N = np.tile(UP, (2, 1))
    assert check(ctx, X, N, 2, radius=5.0)[0].tolist() == [0, 1]
    assert check(ctx, X, N, 2, radius=np.nextafter(5.0, 6.0))[0].tolist() == [0, 0]
    assert check(ctx, X, N, 2)[0].tolist() == [0, 0]


def test_min_size_one_and_beyond_n_and_no_seed_at_all(ctx):
    X, N, _ = regions_ref.hinge(9, 10.0, m=10)
    labels, st = check(ctx, X, N, 8, min_size=1)
    assert st["n_regions"] == 2
    labels, st = check(ctx, X, N, 8, min_size=len(X) + 1, upload=False)
    assert (labels == -1).all() and st["n_regions_all"] == 2 and st["n_regions"] == 0 and (st["largest_label"], st["largest_size"]) == (-1, 0)
    labels, st = check(ctx, X, N, 8, min_size=2**62, upload=False)
    assert (labels == -1).all()
    labels, st = check(ctx, X, N, 8, seeds=np.zeros(len(X), bool), upload=False)
    assert (labels == -1).all() and st["n_regions_all"] == 0 and st["n_smooth"] == 0 and st["n_border"] == 0


def test_a_border_that_sees_the_lower_root_only_through_the_other_ends_list(ctx):
    """Point 1 lists point 2 alone, point 0 lists point 1: the normals of 0 and 2 are 8 degrees apart, that of 1 lies between."""
    X = np.array([[0.0, 0, 0], [1.0, 0, 0], [1.4, 0, 0]])
    assert regions_ref.lists(X, 2)[0].tolist() == [[0, 1], [1, 2], [2, 1]]
    tilt = lambda d: [math.sin(math.radians(d)), 0.0, math.cos(math.radians(d))]   # noqa: E731
    N = np.array([tilt(0), tilt(4), tilt(8)])
    labels, st = check(ctx, X, N, 2, seeds=[1, 0, 1])
    assert labels.tolist() == [0, 0, 1] and st["n_border"] == 1 and (st["largest_label"], st["largest_size"]) == (0, 2)
    labels, st = check(ctx, X[::-1].copy(), N[::-1].copy(), 2, seeds=[1, 0, 1])          # the lower root in its own list now
    assert labels.tolist() == [0, 0, 1]
    labels, st = check(ctx, X, N, 2, seeds=[1, 0, 1], min_size=2)                        # the border point's second choice is not taken
    assert labels.tolist() == [0, 0, -1] and st["n_regions"] == 1
    X2 = np.array([[0.0, 0, 0], [1.0, 0, 0], [1.4, 0, 0], [1.44, 0, 0], [1.49, 0, 0]])   # {2, 3, 4} survives, {0} + its border does not
    labels, st = check(ctx, X2, np.vstack([N, N[2:], N[2:]]), 2, seeds=[1, 0, 1, 1, 1], min_size=3)
    assert labels.tolist() == [-1, -1, 0, 0, 0] and st["n_border"] == 1 and st["n_regions_all"] == 2


# ---- group, wave and block seams ----
def surface_case(seed, n, k):
    X, T = orient_ref.surface(seed, n, noise=0.002)
    N = T.astype(np.float32)
    seeds = np.random.default_rng(seed + 1).uniform(0, 1, n) < 0.8
    return X, N, seeds


@pytest.mark.parametrize("n", [15, 16, 17, 63, 64, 65, 255, 257, 4097])
def test_wave_and_block_seams(ctx, n):
    X, N, seeds = surface_case(100 + n, n, 8)
    r = float(np.sqrt(np.median(regions_ref.lists(X, 8)[1][:, -1])))
    check(ctx, X, N, 8, cos_min=math.cos(math.radians(12.0)), seeds=seeds, radius=r, min_size=3)


@pytest.mark.parametrize("k", [2, 3, 16, 17, 33])
def test_list_lengths(ctx, k):
    X, N, seeds = surface_case(300 + k, 700, k)
    knn = regions_ref.lists(X, k)
    for kw in (dict(), dict(seeds=seeds, min_size=4), dict(oriented=True, seeds=seeds, radius=float(np.sqrt(np.median(knn[1][:, -1]))))):
        check(ctx, X, N, k, regions_ref.regions(X, N, k, 0.98, knn=knn, **kw), cos_min=0.98, **kw)


# ---- one long path ----
@pytest.mark.parametrize("order", ["shuffled", "ascending", "descending"])
def test_one_long_path(ctx, order):
    """100 200 lattice points on a line at k = 3 with equal normals: every point links with its two neighbours, so whatever the
    order of the indices there is one region, rooted at index 0, of all points -- given ascending, every union hooks the
    successor under the predecessor and the chain of parents is as long as the cloud."""
    n = 100_200
    pos = np.arange(n, dtype=np.float64)
    if order == "shuffled":
        pos = pos[np.random.default_rng(31).permutation(n)]
    elif order == "descending":
        pos = pos[::-1]
    X = np.ascontiguousarray(np.column_stack([pos, np.zeros(n), np.zeros(n)]))
    N = np.tile(UP.astype(np.float32), (n, 1))
    labels, st = call(ctx, X, N, 3)
    assert (labels == 0).all()
    assert st == dict(n_points=n, n_void=0, n_smooth=n, n_border=0, n_regions_all=1, n_regions=1, n_labelled=n, largest_label=0, largest_size=n)
    # a plain point every 1 000 positions: 101 segments, and every plain point a border of the neighbouring segment with the
    # lower root.  The closed form, from the positions alone:
    seeds = pos % 1000 != 500
    at = np.empty(n, np.int64)
    at[pos.astype(np.int64)] = np.arange(n)                                    # the index of the point at every position
    seg = np.cumsum(~seeds[at])                                                # the segment of every position (plain: the one to its right)
    root = np.full(102, n, np.int64)
    np.minimum.at(root, seg[seeds[at]], at[seeds[at]])
    plain = np.flatnonzero(~seeds[at])
    home = np.where(root[seg[plain] - 1] < root[seg[plain]], seg[plain] - 1, seg[plain])
    size = np.bincount(seg[seeds[at]], minlength=102) + np.bincount(home, minlength=102)
    alive = size >= 1000
    order = np.argsort(root[:101])
    label_of = np.full(102, -1, np.int64)
    label_of[order[alive[order]]] = np.arange(int(alive[:101].sum()))
    want = np.empty(n, np.int32)
    want[at] = label_of[seg]
    want[at[plain]] = label_of[home]
    labels, st = call(ctx, X, N, 3, seeds=seeds, min_size=1000, upload=False)
    assert np.array_equal(labels, want)
    sizes = size[order[alive[order]]]
    assert st == dict(n_points=n, n_void=0, n_smooth=n - 100, n_border=100, n_regions_all=101, n_regions=len(sizes),
                      n_labelled=int(sizes.sum()), largest_label=int(np.argmax(sizes)), largest_size=int(sizes.max()))
    assert 40 <= st["n_regions"] <= 99 and st["largest_size"] in (1000, 1001)


# ---- a thousand patches ----
def test_a_thousand_patches_rank_and_survive_over_more_than_one_block(ctx):
    X, N, per = regions_ref.patches()
    assert len(X) > 4 * 1024
    knn = regions_ref.lists(X, 9)
    ref = regions_ref.regions(X, N, 9, COS5, radius=5.0, knn=knn)
    assert ref["n_regions"] == 1000 and ref["largest_size"] == 9
    check(ctx, X, N, 9, ref, radius=5.0)
    ref = regions_ref.regions(X, N, 9, COS5, radius=5.0, min_size=6, knn=knn)
    assert ref["n_regions_all"] == 1000 and ref["n_regions"] == int((per >= 6).sum()) and 400 < ref["n_regions"] < 600
    check(ctx, X, N, 9, ref, radius=5.0, min_size=6, upload=False)


# ---- lists and unions across chunks, cell order ----
@pytest.fixture(scope="module")
def two_thousand():
    X = regions_ref.noisy_box(77, 2000)
    knn = regions_ref.lists(X, 12)
    N, pl = orc.normals(X, regions_ref.lists(X, 10)[0])
    kw = dict(cos_min=math.cos(math.radians(10.0)), seeds=pl >= 0.6, min_size=20, radius=0.2)
    return X, N, kw, regions_ref.regions(X, N, 12, knn=knn, **kw)


def test_the_two_thousand_are_a_real_case(two_thousand):
    ref = two_thousand[3]
    assert ref["n_regions"] >= 3 and ref["n_regions_all"] > ref["n_regions"] and ref["n_border"] > 0 and 0 < ref["n_labelled"] < 2000


@pytest.mark.parametrize("chunk", [None, 64, 1000])
def test_unions_cross_chunk_boundaries(two_thousand, chunk):
    X, N, kw, ref = two_thousand
    with context_with(**({} if chunk is None else {"SICP_REGIONS_CHUNK": chunk})) as c:
        check(c, X, N, 12, ref, **kw)


def test_cell_order_changes_no_byte(two_thousand):
    X, N, kw, ref = two_thousand
    got = []
    for q in (1, 0):
        with context_with(SICP_ORDER_MIN_Q=q, SICP_REGIONS_CHUNK=700) as c:
            got.append(check(c, X, N, 12, ref, **kw))
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1] == got[1][1]


# ---- seeded clouds with estimated normals ----
RANDOM_SEEDS = list(range(700, 730))


@lru_cache(maxsize=None)
def random_case(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1200, 2601))
    X = (regions_ref.noisy_box, regions_ref.noisy_can)[seed % 2](seed, n)
    k = int(rng.integers(8, 17))
    knn = regions_ref.lists(X, k)
    N, pl = orc.normals(X, regions_ref.lists(X, 10)[0])
    kw = dict(cos_min=math.cos(math.radians(float(rng.uniform(6.0, 12.0)))), min_size=int(rng.integers(10, 40)))
    if seed % 2 == 0:
        kw["oriented"] = False
    else:                                          # estimated normals carry no orientation: every second case compares them as they are
        kw["oriented"] = True
    if (seed // 2) % 2 == 0:
        kw["radius"] = float(np.sqrt(np.quantile(knn[1][:, -1], 0.7)))
    if (seed // 4) % 2 == 0:
        with np.errstate(invalid="ignore"):
            kw["seeds"] = pl.astype(np.float64) >= 0.5
    else:
        kw["seeds"] = rng.uniform(0, 1, n) < 0.9
    return X, N, k, kw, regions_ref.regions(X, N, k, knn=knn, **kw)


def degenerate(ref):
    return ref["n_regions"] < 2 or ref["n_border"] == 0 or ref["n_labelled"] == ref["n_points"]


def test_at_most_three_of_the_seeded_cases_are_degenerate():
    assert sum(degenerate(random_case(seed)[4]) for seed in RANDOM_SEEDS) <= 3


@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_seeded_clouds_with_estimated_normals(ctx, seed):
    X, N, k, kw, ref = random_case(seed)
    check(ctx, X, N, k, ref, **kw)


# ---- roads ----
def test_host_and_device_outputs_device_normals_and_seeds(ctx, two_thousand):
    import torch
    from simpleicp_amd import _lib
    X, N, kw, ref = two_thousand
    ctx.upload(_lib.FIX, X)
    dev = torch.device("cuda", 0)
    labels = torch.full((2000,), FILL, dtype=torch.int32, device=dev)
    nd, sd = torch.from_numpy(N).to(dev), torch.from_numpy(kw["seeds"].view(np.uint8)).to(dev)
    torch.cuda.synchronize()
    a = (kw["cos_min"], kw["radius"], False)
    st = ctx.regions(_lib.FIX, nd, 12, *a, sd, kw["min_size"], labels_ptr=labels.data_ptr())
    assert np.array_equal(labels.cpu().numpy(), ref["labels"]) and st.as_dict() == regions_ref.record(ref)
    assert nd.cpu().numpy().tobytes() == N.tobytes() and sd.cpu().numpy().tobytes() == kw["seeds"].tobytes()
    # host normals with device seeds and a host output, device normals with host seeds, the binding's host form
    host = np.full(2000, FILL, np.int32)
    st = ctx.regions(_lib.FIX, N, 12, *a, sd, kw["min_size"], labels_ptr=host.ctypes.data)
    assert np.array_equal(host, ref["labels"]) and st.as_dict() == regions_ref.record(ref)
    labels.fill_(FILL)
    torch.cuda.synchronize()
    st = ctx.regions(_lib.FIX, nd, 12, *a, kw["seeds"], kw["min_size"], labels_ptr=labels.data_ptr())
    assert np.array_equal(labels.cpu().numpy(), ref["labels"]) and st.as_dict() == regions_ref.record(ref)
    got, st = ctx.regions(_lib.FIX, N, 12, *a, kw["seeds"], kw["min_size"])
    assert got.dtype == np.int32 and np.array_equal(got, ref["labels"]) and st.as_dict() == regions_ref.record(ref)


def test_a_strided_float32_tensor_through_smooth_regions(two_thousand):
    import torch
    import simpleicp_amd
    X, N, kw, _ = two_thousand
    X32 = X.astype(np.float32)
    X64 = X32.astype(np.float64)
    want = dict(neighbors=12, cos_min=kw["cos_min"], max_angle=None, radius=kw["radius"], min_size=kw["min_size"])
    ref = regions_ref.regions(X64, N, 12, **kw)
    wide = torch.zeros((2000, 7), dtype=torch.float32, device="cuda:0")
    wide[:, 1:6:2] = torch.from_numpy(X32).to("cuda:0")
    view = wide[:, 1:6:2]
    nwide = torch.zeros((2000, 5), dtype=torch.float32, device="cuda:0")
    nwide[:, 1:4] = torch.from_numpy(N).to("cuda:0")
    swide = torch.zeros((2000, 2), dtype=torch.bool, device="cuda:0")
    swide[:, 1] = torch.from_numpy(kw["seeds"]).to("cuda:0")
    assert not view.is_contiguous() and not nwide[:, 1:4].is_contiguous() and not swide[:, 1].is_contiguous()
    labels, info = simpleicp_amd.smooth_regions(view, nwide[:, 1:4], seeds=swide[:, 1], return_info=True, **want)
    assert labels.is_cuda and labels.dtype == torch.int32 and np.array_equal(labels.cpu().numpy(), ref["labels"])
    assert info == dict(regions_ref.record(ref), cos_min=kw["cos_min"]) and nwide[:, 1:4].cpu().numpy().tobytes() == N.tobytes()
    host = simpleicp_amd.smooth_regions(X32, N, seeds=kw["seeds"], **want)
    assert isinstance(host, np.ndarray) and host.dtype == np.int32 and np.array_equal(host, ref["labels"])
    # max_angle in degrees is its cosine formed on the host
    by_angle, info = simpleicp_amd.smooth_regions(X32, N, seeds=kw["seeds"], neighbors=12, max_angle=10.0, radius=kw["radius"],
                                                  min_size=kw["min_size"], return_info=True)
    assert info["cos_min"] == kw["cos_min"] == math.cos(math.radians(10.0)) and np.array_equal(by_angle, ref["labels"])
    # the library's own normals and min_planarity, on both roads: the same bytes, and what the reference makes of those normals
    own = dict(neighbors=12, max_angle=10.0, min_planarity=0.6, min_size=20, return_info=True)
    dev_labels, dev_info = simpleicp_amd.smooth_regions(view, **own)
    host_labels, host_info = simpleicp_amd.smooth_regions(X32, **own)
    assert np.array_equal(dev_labels.cpu().numpy(), host_labels) and dev_info == host_info and host_info["n_regions"] >= 3
    from simpleicp_amd import _lib, backend
    nv, pl = backend.get_context().estimate_normals(_lib.FIX, np.arange(2000, dtype=np.int64), 10)
    with np.errstate(invalid="ignore"):
        ref = regions_ref.regions(X64, nv, 12, math.cos(math.radians(10.0)), seeds=pl.astype(np.float64) >= 0.6, min_size=20)
    assert np.array_equal(host_labels, ref["labels"]) and host_info == dict(regions_ref.record(ref), cos_min=math.cos(math.radians(10.0)))
    empty = simpleicp_amd.smooth_regions(torch.zeros((0, 3), device="cuda:0"), return_info=True)
    assert empty[0].shape == (0,) and empty[0].dtype == torch.int32 and empty[0].is_cuda
    assert empty[1] == dict(dict.fromkeys(regions_ref.KEYS, 0), cos_min=COS5)


def test_the_same_bytes_again_and_behind_other_calls(ctx, two_thousand):
    from simpleicp_amd import _lib
    X, N, kw, ref = two_thousand
    first = check(ctx, X, N, 12, ref, **kw)
    again = call(ctx, X, N, 12, upload=False, **kw)
    ctx.cluster(_lib.FIX, 0.05, 4)
    third = call(ctx, X, N, 12, upload=False, **kw)
    ctx.orient(_lib.FIX, N, 12, reference=(0.5, 0.35, 0.25), away=True)
    fourth = call(ctx, X, N, 12, upload=False, **kw)
    ctx.upload(_lib.MOV, X + np.array([0.01, -0.02, 0.015]))
    Q = np.arange(0, 2000, 2, dtype=np.int64)
    nv, pl = ctx.estimate_normals(_lib.FIX, Q, 10)
    ctx.icp_setup(Q, nv, pl)
    ctx.icp_run(np.zeros(6), np.zeros(6), np.zeros(6), 0.0, None, 5, 0.0, 0)
    fifth = call(ctx, X, N, 12, upload=False, **kw)
    for x in (again, third, fourth, fifth):
        assert x[0].tobytes() == first[0].tobytes() and x[1] == first[1]


def test_cluster_and_orient_are_what_their_references_say_after_the_header_move(ctx):
    """sicp_cluster.hip takes its union-find and its scan from the header it now shares with sicp_regions.hip: the results are
    held to tests/cluster_ref.py and tests/orient_ref.py, behind a regions call that used the same buffers."""
    from simpleicp_amd import _lib
    X = cluster_ref.blobs(41, 1500)
    ctx.upload(_lib.FIX, X)
    call(ctx, X, np.tile(UP, (1500, 1)), 8, upload=False)
    ref = cluster_ref.cluster(X, 0.3, 5)
    labels, core, st = ctx.cluster(_lib.FIX, 0.3, 5)
    assert labels.tobytes() == ref["labels"].astype(np.int32).tobytes() and np.array_equal(core, ref["core"])
    assert st.as_dict() == cluster_ref.record(ref)
    Xs, T = orient_ref.torus(42, 1500)
    Ns, _ = orient_ref.coin(43, T)
    ctx.upload(_lib.FIX, Xs)
    call(ctx, Xs, Ns, 8, upload=False)
    oref = orient_ref.orient(Xs, Ns, 10, away_from=(0.0, 0.0, 0.0))
    out, flipped, st = ctx.orient(_lib.FIX, Ns, 10, reference=(0.0, 0.0, 0.0), away=True)
    assert out.tobytes() == oref["normals"].tobytes() and np.array_equal(flipped, oref["flipped"]) and st.as_dict() == orient_ref.record(oref)


def test_pointcloud_selectors_on_the_bunny():
    from simpleicp_amd import PointCloud
    from simpleicp_amd.pointcloud import PointCloudException
    d = os.path.join(os.path.dirname(__file__), "golden", "data")
    B = np.ascontiguousarray(np.load(os.path.join(d, "bunny_part1.npz"))["q"].astype(np.float64)[::4])
    pc = PointCloud(B, columns=["x", "y", "z"])
    pc.select_in_range(B[len(B) // 2][None, :], float(np.ptp(B, axis=0).max()) / 3.0)
    cur = pc.idx_selected
    assert 100 < len(cur) < len(B)
    X = np.ascontiguousarray(B[cur])
    # no normal columns: the library estimates them on the selected rows taken as a cloud of their own
    pc.select_regions(max_angle=15.0, neighbors=12, min_size=10)
    info = pc.last_region_stats
    from simpleicp_amd import _lib, backend
    nv, _ = backend.get_context().estimate_normals(_lib.FIX, np.arange(len(X), dtype=np.int64), 10)
    ref = regions_ref.regions(X, nv, 12, math.cos(math.radians(15.0)), min_size=10)
    assert info == dict(regions_ref.record(ref), cos_min=math.cos(math.radians(15.0))) and 0 < info["n_labelled"] < len(X)
    assert np.array_equal(pc.idx_selected, cur[ref["labels"] >= 0])
    # with normal columns: they are the normals; the largest region alone stays
    pc2 = PointCloud(X, columns=["x", "y", "z"])
    for j, col in enumerate(("nx", "ny", "nz")):
        pc2[col] = nv[:, j].astype(np.float64)
    pc2.select_largest_region(max_angle=15.0, neighbors=12, min_size=10)
    assert pc2.last_region_stats == info and np.array_equal(pc2.idx_selected, np.flatnonzero(ref["labels"] == ref["largest_label"]))
    assert pc2.num_selected_points == ref["largest_size"]
    pc2.select_largest_region(max_angle=15.0, neighbors=12, min_size=10**6)
    assert pc2.num_selected_points == 0 and pc2.last_region_stats["n_regions"] == 0
    with pytest.raises(PointCloudException, match="max_angle"):
        pc.select_regions(max_angle=0.0)
    with pytest.raises(PointCloudException, match="no keyword"):
        pc.select_regions(min_points=3)


# ---- refusals ----
def test_refusals_name_the_argument_and_leave_the_outputs(ctx, two_thousand):
    from simpleicp_amd import _lib
    X, N, kw, ref = two_thousand
    ctx.upload(_lib.FIX, X)
    L, F = ctx._L, _lib.FIX
    labels, st = np.full(2000, FILL, np.int32), _lib.RegionsStats()
    sd = kw["seeds"].view(np.uint8)

    def refused(c, slot, nrm, k, radius, cos_min, oriented, min_size, lp, sp, word):
        assert L.sicp_regions(c._h, slot, nrm, k, radius, cos_min, oriented, _lib._ptr(sd), min_size, lp, sp) == _lib.ERR_INVALID
        assert word.encode() in L.sicp_last_error(), L.sicp_last_error()
        assert np.all(labels == FILL)

    npx, lp, sp = _lib._ptr(N), _lib._ptr(labels), C_.byref(st)
    inf = math.inf
    refused(ctx, F, None, 12, inf, 0.9, 0, 1, lp, sp, "normals is null")
    refused(ctx, F, npx, 12, inf, 0.9, 0, 1, None, sp, "labels_out is null")
    refused(ctx, F, npx, 12, inf, 0.9, 0, 1, lp, None, "out is null")
    for bad in (1, 0, -3):
        refused(ctx, F, npx, bad, inf, 0.9, 0, 1, lp, sp, "k must be >= 2")
    refused(ctx, F, npx, _lib.FPFH_MAX_K + 1, inf, 0.9, 0, 1, lp, sp, "k must be <=")
    for bad in (math.nan, 1.0000001, -1e-9, -inf, inf):
        refused(ctx, F, npx, 12, inf, bad, 0, 1, lp, sp, "cos_min must be >= 0")
    for bad in (math.nan, 1.0000001, -1.0000001):
        refused(ctx, F, npx, 12, inf, bad, 1, 1, lp, sp, "cos_min must be >= -1")
    for bad in (0.0, -1.0, math.nan, -inf):
        refused(ctx, F, npx, 12, bad, 0.9, 0, 1, lp, sp, "radius must be > 0")
    for bad in (0, -5):
        refused(ctx, F, npx, 12, inf, 0.9, 0, bad, lp, sp, "min_size must be >= 1")
    refused(ctx, 2, npx, 12, inf, 0.9, 0, 1, lp, sp, "slot")
    with _lib.Context(0) as other:
        refused(other, _lib.MOV, npx, 12, inf, 0.9, 0, 1, lp, sp, "empty")
        other.upload(_lib.MOV, X[:10])
        refused(other, _lib.MOV, npx, 11, inf, 0.9, 0, 1, lp, sp, "exceeds the number of points")
        other.upload(_lib.MOV, X, index_base=7)
        refused(other, _lib.MOV, npx, 12, inf, 0.9, 0, 1, lp, sp, "shard")
    ctx.set_exchange(lambda *a: 0, 0, 1)
    try:
        refused(ctx, F, npx, 12, inf, 0.9, 0, 1, lp, sp, "not supported with an exchange")
    finally:
        ctx.set_exchange(None, 0, 1)
    assert L.sicp_regions(None, F, npx, 12, inf, 0.9, 0, None, 1, lp, sp) == _lib.ERR_INVALID and b"null ctx" in L.sicp_last_error()
    with pytest.raises(_lib.BackendError, match="k must be"):
        ctx.regions(F, N, 1, 0.9)
    check(ctx, X, N, 12, ref, **kw)                                            # and the context still works
