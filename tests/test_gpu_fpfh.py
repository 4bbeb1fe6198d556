"""FPFH descriptors on the GPU (contract (F)): the (n, 34) counts, the (n, 33) floats and the record equal the
numpy reference of tests/fpfh_ref.py bit for bit -- seeded clouds on both search paths, the extremes of k, several chunks, exact
ties, duplicates, void pairs, non-finite normals, the radius, the viewpoint, host and device memory --, the refusals, and
fpfh_features on tensors and on the bundled bunny.  (The refusal of 2^31 points is check_whole_cloud's, shared with the outlier
filters; a cloud of that size is no few-seconds test.)"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import fpfh_ref
from oracle import orc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEYS = ("n_points", "n_pairs", "n_void_pairs", "n_empty")


@pytest.fixture(scope="module")
def ctx():
    from simpleicp_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check(ctx, X, N, k, radius=np.inf, viewpoint=None, rows=None, device=False, upload=True):
    """One call against the reference: outputs in host memory; device=True: also normals and outputs in device memory.
    rows: the reference is formed for these points only.  Returns (reference, descriptors, counts)."""
    from simpleicp_amd import _lib
    X = np.ascontiguousarray(X, dtype=np.float64)
    N = np.ascontiguousarray(N, dtype=np.float32)
    if upload:
        ctx.upload(_lib.FIX, X)
    ref = fpfh_ref.fpfh(X, N, k, radius, viewpoint, rows=rows)
    F, cnt, st = ctx.fpfh(_lib.FIX, N, k, radius, viewpoint, want_counts=True)
    at = slice(None) if rows is None else np.asarray(rows)
    print(f"n={len(X)} k={k} radius={radius} viewpoint={viewpoint}: {st.as_dict()}")
    assert F.shape == (len(X), 33) and cnt.shape == (len(X), 34) and cnt.dtype == np.uint16
    assert np.array_equal(cnt[at], ref["counts"])
    assert np.array_equal(u32(F[at]), u32(ref["fpfh"]))
    if rows is None:
        assert st.as_dict() == {key: ref[key] for key in KEYS}
    else:
        assert st.n_points == len(X) and st.n_pairs == int(cnt[:, 33].astype(np.int64).sum()) and st.n_empty == int((cnt[:, 33] == 0).sum())
    if device:
        Nd = torch.tensor(N, device=DEV)
        Fd = torch.full((len(X), 33), -1.0, dtype=torch.float32, device=DEV)
        cd = torch.full((len(X), 34), -1, dtype=torch.int16, device=DEV)
        st2 = ctx.fpfh(_lib.FIX, Nd, k, radius, viewpoint, fpfh_ptr=Fd.data_ptr(), counts_ptr=cd.data_ptr())
        assert st2.as_dict() == st.as_dict()
        assert np.array_equal(u32(Fd.cpu().numpy()), u32(F)) and np.array_equal(cd.cpu().numpy().view(np.uint16), cnt)
        assert np.array_equal(Nd.cpu().numpy().view(np.uint32), N.view(np.uint32))               # the caller's normals are left alone
        # descriptors to the device, no counts asked for
        Fd.fill_(-1.0)
        ctx.fpfh(_lib.FIX, N, k, radius, viewpoint, fpfh_ptr=Fd.data_ptr())
        assert np.array_equal(u32(Fd.cpu().numpy()), u32(F))
    return ref, F, cnt


def estimated(ctx, X, k=10):
    from simpleicp_amd import _lib
    ctx.upload(_lib.FIX, np.ascontiguousarray(X, dtype=np.float64))
    return ctx.estimate_normals(_lib.FIX, np.arange(len(X), dtype=np.int64), k)[0]


def lattice(n):
    g = np.arange(n, dtype=np.float64)
    return np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))


def unit(rng, n):
    v = rng.standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


# ---- seeded clouds, both search paths ----
def test_seeded_cloud_with_estimated_normals(ctx):
    X = np.random.default_rng(2000).uniform(-1, 1, (2000, 3))
    N = estimated(ctx, X)
    ref, F, cnt = check(ctx, X, N, 16, device=True)
    assert ref["n_empty"] == 0 and ref["n_pairs"] == 2000 * 15 - ref["n_void_pairs"]
    sums = F.astype(np.float64).reshape(-1, 3, 11).sum(axis=2)
    assert np.allclose(sums, 200.0, atol=1e-3)
    assert len(np.unique(np.argmax(F[:, :11], axis=1))) > 3            # (not one bin for everybody)


def test_seeded_cloud_past_65536_points_on_the_grid(ctx):
    X = np.random.default_rng(70).uniform(-5, 5, (70_000, 3))
    N = estimated(ctx, X)
    rows = np.random.default_rng(71).choice(70_000, 300, replace=False)
    rows[:4] = (0, 69_999, 65_535, 65_536)
    check(ctx, X, N, 16, rows=rows, upload=False)


# ---- the extremes of k ----
def test_everyone_neighbours_everyone(ctx):
    rng = np.random.default_rng(40)
    ref, _, _ = check(ctx, rng.uniform(0, 1, (40, 3)), unit(rng, 40), 40, device=True)
    assert ref["n_pairs"] == 40 * 39


def test_k_2(ctx):
    rng = np.random.default_rng(2)
    ref, F, cnt = check(ctx, rng.uniform(0, 1, (500, 3)), unit(rng, 500), 2)
    assert np.all(cnt[:, 33] == 1) and np.all((cnt[:, :33] == 1).sum(axis=1) == 3)         # one pair: three bins


def test_k_128_with_300_points(ctx):
    rng = np.random.default_rng(128)
    ref, _, cnt = check(ctx, rng.uniform(0, 1, (300, 3)), unit(rng, 300), 128)
    assert np.all(cnt[:, 33] == 127)
    check(ctx, rng.uniform(0, 1, (300, 3)), unit(rng, 300), 65)                              # (one lane into the second round of 64)


# ---- several chunks ----
def test_four_chunks_give_the_bytes_of_one(ctx):
    from simpleicp_amd import _lib
    rng = np.random.default_rng(200)
    X, N = rng.uniform(0, 1, (200, 3)), unit(rng, 200)
    _, F, cnt = check(ctx, X, N, 12, radius=0.35, viewpoint=(0.5, 0.5, 4.0))
    old = os.environ.get("SICP_FPFH_CHUNK")
    os.environ["SICP_FPFH_CHUNK"] = "64"                               # (read at sicp_ctx_create)
    try:
        with _lib.Context(0) as other:
            _, F4, cnt4 = check(other, X, N, 12, radius=0.35, viewpoint=(0.5, 0.5, 4.0), device=True)
    finally:
        if old is None:
            del os.environ["SICP_FPFH_CHUNK"]
        else:
            os.environ["SICP_FPFH_CHUNK"] = old
    assert np.array_equal(u32(F4), u32(F)) and np.array_equal(cnt4, cnt)


# ---- exact ties, duplicates, void pairs, non-finite normals ----
def test_lattice_with_ties_at_the_last_rank(ctx):
    X = lattice(6)
    N = unit(np.random.default_rng(6), len(X))
    idx, d2 = orc.knn(X, X, k=9)
    assert (d2[:, 8] == d2[:, 7]).mean() > 0.5 and np.all(d2[:, 0] == 0)         # the k-th rank is one of several equidistant points
    check(ctx, X, N, 9)
    check(ctx, X, N, 8, upload=False)


def test_exact_duplicates(ctx):
    rng = np.random.default_rng(9)
    X, N = rng.uniform(0, 1, (400, 3)), unit(rng, 400)
    X[10:15] = X[3]                                                    # point 3 has five exact duplicates, each with a normal of its own
    X[399] = X[398]
    idx, d2 = orc.knn(X, X, k=8)
    assert idx[12, 0] == 3 and 12 in idx[12, 1:6] and np.all(d2[12, :6] == 0)      # rank 0 is NOT the point itself
    ref, F, cnt = check(ctx, X, N, 8)
    assert ref["n_void_pairs"] == 6 * 5 + 2 and np.all(cnt[10:15, 33] == 2) and cnt[3, 33] == 2
    ref, _, cnt = check(ctx, X, N, 6, upload=False)                    # the duplicates fill the whole list: no pair, an empty point
    assert np.all(cnt[[3, 10, 11, 12, 13, 14], 33] == 0) and ref["n_empty"] == 6


def test_a_normal_along_the_connecting_line_is_void(ctx):
    X = lattice(5)
    N = np.tile(np.float32([1, 0, 0]), (len(X), 1))
    ref, _, cnt = check(ctx, X, N, 7)
    assert ref["n_void_pairs"] > 0 and cnt[62, 33] == 4                # the centre: six neighbours, the two along x are void
    N2 = unit(np.random.default_rng(1), len(X))
    N2[62] = (0, 0, 1)                                                 # one point's normal along some of its own pairs only
    check(ctx, X, N2, 7, upload=False)


def test_nan_and_inf_normals(ctx):
    rng = np.random.default_rng(13)
    X, N = rng.uniform(0, 1, (600, 3)), unit(rng, 600)
    N[5] = np.nan
    N[77, 1] = np.inf
    N[200, 2] = -np.inf
    N[201, 0] = np.nan
    ref, F, cnt = check(ctx, X, N, 10, device=True)
    assert np.all(cnt[[5, 77, 200, 201]] == 0) and ref["n_empty"] == 4 and ref["n_void_pairs"] > 4 * 9
    assert np.isfinite(F).all() and F[5].any()                         # its neighbours' share is still there
    check(ctx, X, N, 10, viewpoint=(3.0, 0.0, 0.0), upload=False)      # NaN stays as it is under the orientation


# ---- the radius ----
def test_radius_leaves_an_isolated_point_empty(ctx):
    rng = np.random.default_rng(17)
    X, N = rng.uniform(0, 1, (500, 3)), unit(rng, 501)
    X = np.vstack([X, [[50.0, 50.0, 50.0]]])
    ref, F, cnt = check(ctx, X, N, 12, radius=0.3, device=True)
    assert ref["n_empty"] >= 1 and not cnt[500].any() and not F[500].any()
    assert cnt[:, 33].max() == 11 and cnt[:, 33].min() < 11           # the radius cuts some lists short


def test_radius_equal_to_a_neighbour_distance_is_strict(ctx):
    X = lattice(5)
    N = unit(np.random.default_rng(3), len(X))
    ref, _, cnt = check(ctx, X, N, 40, radius=2.0)
    # the centre's 39 nearest: 6 at d2 = 1, 12 at 2, 8 at 3, 6 at 4, 7 of the 24 at 5 -- within 2.0, strictly: the first 26
    assert cnt[62, 33] == 26
    ref, _, cnt = check(ctx, X, N, 40, radius=1.0, upload=False)       # d2 = 1 < 1 * 1 fails: nobody has a pair
    assert ref["n_empty"] == len(X) and ref["n_pairs"] == 0 and not cnt.any()
    check(ctx, X, N, 40, radius=np.nextafter(2.0, 3.0), upload=False)


# ---- the viewpoint ----
def test_viewpoint_on_and_off(ctx):
    rng = np.random.default_rng(23)
    X, N = rng.uniform(-1, 1, (800, 3)), unit(rng, 800)
    _, off, _ = check(ctx, X, N, 14)
    _, on, _ = check(ctx, X, N, 14, viewpoint=(0.1, -0.2, 3.0), upload=False, device=True)
    flipped = fpfh_ref.oriented(X, N, (0.1, -0.2, 3.0))[:, 0] != N[:, 0].astype(np.float64)
    assert 0.3 < flipped.mean() < 0.7 and not np.array_equal(on, off)
    # normals that already look at the viewpoint: the orientation changes nothing
    Nv = fpfh_ref.oriented(X, N, (0.1, -0.2, 3.0)).astype(np.float32)
    _, same, _ = check(ctx, X, Nv, 14, upload=False)
    assert np.array_equal(u32(same), u32(on))


def test_flat_patch(ctx):
    g = np.arange(8, dtype=np.float64)
    P = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    X = np.column_stack([P, np.zeros(64)])
    N = np.tile(np.float32([0, 0, 1]), (64, 1))
    _, F, cnt = check(ctx, X, N, 9, device=True)
    want = np.zeros(33, np.float32)
    want[[5, 16, 27]] = 200.0
    assert np.array_equal(F, np.tile(want, (64, 1)))


# ---- refusals ----
def test_refusals_leave_the_context_usable(ctx):
    from simpleicp_amd import _lib
    rng = np.random.default_rng(31)
    X, N = rng.uniform(0, 1, (100, 3)), unit(rng, 100)
    ctx.upload(_lib.FIX, X)
    L = _lib.load()
    out, st = np.zeros((100, 33), np.float32), _lib.FpfhStats()
    P = _lib._ptr

    def raw(normals=N, k=8, radius=1.0, vp=None, fpfh=out, stats=st, c=ctx, slot=_lib.FIX):
        return L.sicp_fpfh(c._h, slot, P(normals), k, radius, P(vp), P(fpfh), None, None if stats is None else C.byref(stats))

    def refused(rc, word):
        assert rc == _lib.ERR_INVALID and word in L.sicp_last_error().decode(), (rc, L.sicp_last_error())
        assert not out.any()
        assert raw() == _lib.OK and out.any()                          # the next valid call works
        out[:] = 0

    refused(raw(normals=None), "normals")
    refused(raw(fpfh=None), "fpfh_out")
    refused(raw(stats=None), "out is null")
    for k in (1, 0, -4, 129, 101):
        refused(raw(k=k), "k ")
    for r in (float("nan"), 0.0, -1.0, -float("inf")):
        refused(raw(radius=r), "radius")
    for v in ((0.0, float("nan"), 0.0), (float("inf"), 0.0, 0.0)):
        refused(raw(vp=np.array(v)), "viewpoint")
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
    assert raw(radius=float("inf")) == _lib.OK                         # +inf: no radius
    check(ctx, X, N, 8, radius=1.0, upload=False)


# ---- through Python ----
def test_fpfh_features_on_a_strided_float32_view(ctx):
    import simpleicp_amd
    rng = np.random.default_rng(41)
    T = torch.tensor(rng.uniform(-1, 1, (3000, 6)), dtype=torch.float32, device=DEV)
    V = T[:, 1:6:2]                                                    # columns 1, 3, 5: row stride 6, column stride 2
    assert not V.is_contiguous()
    Fd, cd = simpleicp_amd.fpfh_features(V, neighbors=16, radius=0.4, viewpoint=(0, 0, 5), return_counts=True)
    assert isinstance(Fd, torch.Tensor) and Fd.device == T.device and Fd.dtype == torch.float32 and tuple(Fd.shape) == (3000, 33)
    Xh = V.cpu().numpy().astype(np.float64)
    Fh, ch = simpleicp_amd.fpfh_features(Xh, neighbors=16, radius=0.4, viewpoint=(0, 0, 5), return_counts=True)
    assert isinstance(Fh, np.ndarray) and np.array_equal(u32(Fd.cpu().numpy()), u32(Fh))
    assert np.array_equal(cd.cpu().numpy().view(np.uint16), ch)
    e = simpleicp_amd.fpfh_features(V[:0])
    assert isinstance(e, torch.Tensor) and tuple(e.shape) == (0, 33) and e.device == T.device


def test_normals_none_is_the_librarys_own_normals():
    import simpleicp_amd
    from simpleicp_amd import PointCloud, _lib, backend
    rng = np.random.default_rng(43)
    X = rng.uniform(-1, 1, (2500, 3))
    F = simpleicp_amd.fpfh_features(X, neighbors=12, normal_neighbors=9)
    c = backend.get_context()
    nv = c.estimate_normals(_lib.FIX, np.arange(2500, dtype=np.int64), 9)[0]
    assert np.array_equal(u32(simpleicp_amd.fpfh_features(X, nv, neighbors=12)), u32(F))
    Xd = torch.tensor(X, device=DEV)
    assert np.array_equal(u32(simpleicp_amd.fpfh_features(Xd, neighbors=12, normal_neighbors=9).cpu().numpy()), u32(F))
    assert np.array_equal(u32(simpleicp_amd.fpfh_features(Xd, torch.tensor(nv, device=DEV), neighbors=12).cpu().numpy()), u32(F))
    assert np.array_equal(u32(simpleicp_amd.fpfh_features(Xd, nv, neighbors=12).cpu().numpy()), u32(F))
    pc = PointCloud(X, columns=["x", "y", "z"])
    assert np.array_equal(u32(pc.fpfh(12)), u32(simpleicp_amd.fpfh_features(X, neighbors=12)))
    ref = fpfh_ref.fpfh(X, nv, 12)
    assert np.array_equal(u32(F), u32(ref["fpfh"]))


def test_bundled_bunny_against_the_reference():
    import simpleicp_amd
    from simpleicp_amd import _lib, backend
    X = np.ascontiguousarray(orc.load_cloud("bunny_part1")[:5000])
    F, cnt = simpleicp_amd.fpfh_features(X, neighbors=32, normal_neighbors=10, viewpoint=(0.0, 0.0, 10.0), return_counts=True)
    nv = backend.get_context().estimate_normals(_lib.FIX, np.arange(5000, dtype=np.int64), 10)[0]
    ref = fpfh_ref.fpfh(X, nv, 32, viewpoint=(0.0, 0.0, 10.0))
    assert np.array_equal(cnt, ref["counts"]) and np.array_equal(u32(F), u32(ref["fpfh"]))
