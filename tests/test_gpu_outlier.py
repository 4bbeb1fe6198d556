"""Outlier removal on the GPU (contract (O)): every verdict byte, n_kept, mean, std, threshold, the d_i vector
and the capped counts equal the numpy reference of tests/outlier_ref.py bit for bit -- seeded clouds, tiny clouds, degenerate data,
every candidate form --, the refusals, outlier_keep on tensors, PointCloud's two selections, and the end-to-end identities of run(),
run_tensors and run_batch."""
import ctypes as C_
import os

import numpy as np
import pytest
import torch

import outlier_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEYS = ("n_candidates", "n_kept", "mean", "std", "threshold")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def ctx():
    from simpleicp_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def same_stats(st, ref):
    got = st.as_dict()
    assert (got["n_candidates"], got["n_kept"]) == (ref["n_candidates"], ref["n_kept"]), (got, {k: ref[k] for k in KEYS})
    for key in ("mean", "std", "threshold"):
        assert bits([got[key]])[0] == bits([ref[key]])[0], (key, got[key], ref[key])


def check_stat(ctx, X, k, ratio, rows=None, mask=None, d2=None, upload=True):
    """One statistical call against the reference, through host outputs and through device outputs.  Returns the reference."""
    from simpleicp_amd import _lib
    X = np.ascontiguousarray(X, dtype=np.float64)
    if upload:
        ctx.upload(_lib.FIX, X)
    ref = outlier_ref.statistical(X, k, ratio, rows=rows, mask=mask, d2=d2)
    N = len(ref["keep"])
    m = None if mask is None else torch.tensor(np.asarray(mask, dtype=np.uint8), device=DEV)
    mp = None if m is None else m.data_ptr()
    keep, d, st = ctx.outlier_statistical(_lib.FIX, k, ratio, rows=rows, mask_ptr=mp)
    print(f"k={k} ratio={ratio} N={N}: {st.as_dict()}")
    assert keep.dtype == np.bool_ and len(keep) == N and set(np.unique(keep.view(np.uint8))) <= {0, 1}
    assert np.array_equal(bits(d), bits(ref["d"]))
    same_stats(st, ref)
    assert np.array_equal(keep, ref["keep"])
    # the same call into device memory: the same bytes
    kd = torch.full((N,), 7, dtype=torch.uint8, device=DEV)
    dd = torch.full((N,), -1.0, dtype=torch.float64, device=DEV)
    st2 = ctx.outlier_statistical(_lib.FIX, k, ratio, rows=rows, mask_ptr=mp, keep_ptr=kd.data_ptr(), mean_ptr=dd.data_ptr())
    same_stats(st2, ref)
    assert np.array_equal(kd.cpu().numpy(), keep.view(np.uint8)) and np.array_equal(bits(dd.cpu().numpy()), bits(d))
    if m is not None:
        assert np.array_equal(m.cpu().numpy(), np.asarray(mask, dtype=np.uint8))             # the mask itself is left alone ...
        st3 = ctx.outlier_statistical(_lib.FIX, k, ratio, mask_ptr=mp, keep_ptr=mp)          # ... unless the verdicts go over it
        same_stats(st3, ref)
        assert np.array_equal(m.cpu().numpy(), keep.view(np.uint8))
    return ref


def check_radius(ctx, X, r, min_points, rows=None, mask=None, D2=None, upload=True):
    from simpleicp_amd import _lib
    X = np.ascontiguousarray(X, dtype=np.float64)
    if upload:
        ctx.upload(_lib.FIX, X)
    ref = outlier_ref.radius(X, r, min_points, rows=rows, mask=mask, D2=D2)
    N = len(ref["keep"])
    m = None if mask is None else torch.tensor(np.asarray(mask, dtype=np.uint8), device=DEV)
    mp = None if m is None else m.data_ptr()
    keep, cnt, kept = ctx.outlier_radius(_lib.FIX, r, min_points, rows=rows, mask_ptr=mp)
    print(f"r={r} min_points={min_points} N={N}: kept {kept} (reference {ref['n_kept']})")
    assert cnt.dtype == np.uint32 and np.array_equal(cnt, ref["count"])
    assert np.array_equal(keep, ref["keep"]) and kept == ref["n_kept"]
    kd = torch.full((N,), 7, dtype=torch.uint8, device=DEV)
    cd = torch.full((N,), 77, dtype=torch.int32, device=DEV)
    assert ctx.outlier_radius(_lib.FIX, r, min_points, rows=rows, mask_ptr=mp, keep_ptr=kd.data_ptr(), count_ptr=cd.data_ptr()) == kept
    assert np.array_equal(kd.cpu().numpy(), keep.view(np.uint8)) and np.array_equal(cd.cpu().numpy().view(np.uint32), cnt)
    if m is not None:
        assert ctx.outlier_radius(_lib.FIX, r, min_points, mask_ptr=mp, keep_ptr=mp) == kept
        assert np.array_equal(m.cpu().numpy(), keep.view(np.uint8))
    return ref


# ---- statistical filter: the seeded cloud ----
@pytest.fixture(scope="module")
def seeded():
    """20 000 uniform points and 200 planted far ones; every point's 128 ranked squared distances from the oracle, once"""
    rng = np.random.default_rng(41)
    X = np.vstack([rng.uniform(0.0, 10.0, (20_000, 3)), rng.uniform(0.0, 10.0, (200, 3)) + 14.0])
    X = np.ascontiguousarray(X)
    return X, outlier_ref.neighbour_d2(X, 128)


@pytest.mark.parametrize("k", [2, 8, 20, 33, 128])
def test_seeded_cloud(ctx, seeded, k):
    X, d2 = seeded
    for i, ratio in enumerate((2.0, 0.0, -0.5)):
        ref = check_stat(ctx, X, k, ratio, d2=d2, upload=i == 0)
        if ratio == 2.0 and k >= 8:
            assert not ref["keep"][20_000:].any() and ref["keep"][:20_000].mean() > 0.9


def test_tiny_clouds(ctx):
    rng = np.random.default_rng(42)
    check_stat(ctx, rng.normal(0, 1, (5, 3)), 5, 1.0)                # n == k
    X = rng.normal(0, 1, (70, 3))                                    # just over one wave
    for k in (2, 7, 70):
        check_stat(ctx, X, k, 0.5)


@pytest.mark.parametrize("m", [1, 2, 1024, 1025])
def test_candidate_counts_of_the_tree(ctx, seeded, m):
    X, d2 = seeded
    rows = np.random.default_rng(m).choice(len(X), m, replace=False)
    ref = check_stat(ctx, X, 8, 1.0, rows=rows, d2=d2)
    if m == 1:
        assert ref["std"] == 0.0 and ref["keep"].all()


def test_more_partials_than_one_step_of_the_second_stage(ctx, seeded):
    """1024 positions a partial, 1024 partials a step of the one-workgroup second stage: from 2^20 positions on the one-term tree
    runs two levels, as the ten-term one of test_gpu_eval.py does"""
    X, d2 = seeded
    m = 1024 * 1024 + 2049                                            # 1027 partials: an odd count, a last step of three
    rows = np.random.default_rng(46).integers(0, len(X), m)
    ref = check_stat(ctx, X, 8, 1.0, rows=rows, d2=d2)
    assert ref["n_candidates"] == m and 0.5 * m < ref["n_kept"] < m


def test_rows_in_random_order_with_repeats(ctx, seeded):
    X, d2 = seeded
    rows = np.random.default_rng(43).integers(0, len(X), 3001)
    rows[100:110] = rows[5]
    assert len(np.unique(rows)) < len(rows)
    ref = check_stat(ctx, X, 20, 1.0, rows=rows, d2=d2)
    assert len(set(ref["keep"][100:110]) | {ref["keep"][5]}) == 1      # a repeated row: an entry of its own, the same verdict


def test_masks(ctx, seeded):
    X, d2 = seeded
    mask = np.zeros(len(X), np.uint8)
    mask[np.random.default_rng(44).choice(len(X), 37, replace=False)] = 3           # any non-zero byte marks a candidate
    assert check_stat(ctx, X, 20, 1.0, mask=mask, d2=d2)["n_candidates"] == 37
    half = (np.arange(len(X)) % 2).astype(np.uint8)
    check_stat(ctx, X, 8, 2.0, mask=half, d2=d2, upload=False)
    z = check_stat(ctx, X, 20, 2.0, mask=np.zeros(len(X), np.uint8), d2=d2, upload=False)
    assert (z["n_kept"], z["mean"], z["std"], z["threshold"]) == (0, 0.0, 0.0, 0.0)


# ---- degenerate data ----
def test_coincident_points(ctx):
    rng = np.random.default_rng(45)
    X = rng.uniform(0, 5, (12_000, 3))
    X[3000:7000] = X[17]                                             # 4 000 coincident points: far more than any k
    ref = check_stat(ctx, X, 20, 2.0)
    assert np.all(ref["d"][3000:7000] == 0.0) and ref["keep"][3000:7000].all() and ref["keep"][17]
    check_stat(ctx, X, 128, 0.0, upload=False)


def test_lattice_where_every_distance_ties(ctx):
    g = np.arange(17, dtype=np.float64) * 0.25
    X = np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))
    d2 = outlier_ref.neighbour_d2(X, 27)
    for k, ratio in ((7, 0.0), (5, 1.0), (27, -0.5)):
        check_stat(ctx, X, k, ratio, d2=d2, upload=k == 7)


def test_terrestrial_stand_in(ctx):
    """bench.terrestrial_pair -- the generator test_gpu_terrestrial.py runs on, imported, not copied --, a 60 000-point scan thinned
    to every fourth point: the density falls like 1 / r^2, so the slot's grid is the one binned for a dense core.  Both filters
    walk that grid alone (the radius filter never the coarse twin).  The radius filter runs at the largest radius the cell-box
    limit admits there -- wide balls in the core, left early -- and is refused one ulp above it."""
    import bench
    from simpleicp_amd import _lib
    X = np.ascontiguousarray(bench.terrestrial_pair(60_000)[0][::4])
    assert len(X) == 15_000
    d2 = outlier_ref.neighbour_d2(X, 64)
    nn = np.sqrt(d2[:, 1])
    assert np.percentile(nn, 95) > 30 * np.percentile(nn, 5)          # the stand-in is what it claims: spacings over orders of magnitude
    check_stat(ctx, X, 20, 2.0, d2=d2)
    check_stat(ctx, X, 8, 0.0, d2=d2, upload=False)
    rows = np.random.default_rng(46).integers(0, len(X), 2000)
    check_stat(ctx, X, 20, 1.0, rows=rows, d2=d2, upload=False)
    lo, hi = 1e-4, 500.0
    assert ctx.outlier_radius_cells(_lib.FIX, lo)[3] <= _lib.OUTLIER_MAX_BOX_CELLS < ctx.outlier_radius_cells(_lib.FIX, hi)[3]
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if ctx.outlier_radius_cells(_lib.FIX, mid)[3] <= _lib.OUTLIER_MAX_BOX_CELLS:
            lo = mid
        else:
            hi = mid
    refused(lambda: ctx.outlier_radius(_lib.FIX, hi, 9), f"radius {hi:g}", "grid cells")
    full = np.count_nonzero(d2 < lo * lo, axis=1)                    # (all 64 within the ball: the true count is >= 64 > the cap)
    print(f"terrestrial: largest admitted radius {lo:g}, box {ctx.outlier_radius_cells(_lib.FIX, lo)}, "
          f"points within it: median {np.median(full)}, max {full.max()} (of the 64 ranked)")
    assert full.max() >= 10 and full.min() < 10                      # dense core and sparse rim both present at this radius
    keep, cnt, kept = ctx.outlier_radius(_lib.FIX, lo, 9)
    assert np.array_equal(cnt, np.minimum(full, 10).astype(np.uint32)) and np.array_equal(keep, full > 9) and kept == int((full > 9).sum())
    keep_r, cnt_r, kept_r = ctx.outlier_radius(_lib.FIX, lo, 9, rows=rows)
    assert np.array_equal(cnt_r, cnt[rows]) and np.array_equal(keep_r, keep[rows]) and kept_r == int(keep[rows].sum())


def test_chunks_give_the_default_chunk_s_bytes(ctx):
    from simpleicp_amd import _lib
    X = np.ascontiguousarray(np.random.default_rng(47).uniform(0, 6, (5003, 3)))
    ctx.upload(_lib.FIX, X)
    keep, d, st = ctx.outlier_statistical(_lib.FIX, 20, 1.0)
    mask = (np.arange(len(X)) % 3 != 0).astype(np.uint8)
    m = torch.tensor(mask, device=DEV)
    keep_m, d_m, st_m = ctx.outlier_statistical(_lib.FIX, 20, 1.0, mask_ptr=m.data_ptr())
    keep_r, cnt_r, kept_r = ctx.outlier_radius(_lib.FIX, 0.4, 5)
    os.environ["SICP_OUTLIER_CHUNK"] = "1000"
    try:
        small = _lib.Context(0)
    finally:
        del os.environ["SICP_OUTLIER_CHUNK"]
    with small:
        small.upload(_lib.FIX, X)
        keep2, d2_, st2 = small.outlier_statistical(_lib.FIX, 20, 1.0)                   # six chunks, the last one of 3 candidates
        assert np.array_equal(keep2, keep) and np.array_equal(bits(d2_), bits(d)) and st2.as_dict() == st.as_dict()
        keep3, d3, st3 = small.outlier_statistical(_lib.FIX, 20, 1.0, mask_ptr=m.data_ptr())
        assert np.array_equal(keep3, keep_m) and np.array_equal(bits(d3), bits(d_m)) and st3.as_dict() == st_m.as_dict()
        keep4, cnt4, kept4 = small.outlier_radius(_lib.FIX, 0.4, 5)
        assert np.array_equal(keep4, keep_r) and np.array_equal(cnt4, cnt_r) and kept4 == kept_r
    same_stats(st, outlier_ref.statistical(X, 20, 1.0))


# ---- radius filter ----
@pytest.fixture(scope="module")
def small():
    X = np.ascontiguousarray(np.random.default_rng(48).uniform(0, 1, (2000, 3)))
    return X, outlier_ref.all_d2(X)


@pytest.mark.parametrize("r", [1e-7, 0.08, 3.0])
def test_radius_seeded_cloud(ctx, small, r):
    X, D2 = small
    n = len(X)
    for i, mp in enumerate((0, 1, 7, n - 1, n)):
        ref = check_radius(ctx, X, r, mp, D2=D2, upload=i == 0)
        if r == 1e-7:
            assert ref["n_kept"] == (n if mp == 0 else 0)
        if r == 3.0:
            assert ref["n_kept"] == (0 if mp == n else n)


def test_radius_equal_to_the_lattice_spacing_is_strict(ctx):
    g = np.arange(9, dtype=np.float64) * 0.5
    X = np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))
    D2 = outlier_ref.all_d2(X)
    ref = check_radius(ctx, X, 0.5, 0, D2=D2)
    assert np.all(ref["count"] == 1)                                 # d2 == r * r exactly: the six face neighbours stay outside
    ref = check_radius(ctx, X, np.nextafter(0.5, 1.0), 6, D2=D2, upload=False)
    assert ref["count"].max() == 7 and ref["n_kept"] == 7 ** 3       # one ulp more: the interior points reach all six


def test_radius_candidates_and_outputs(ctx, small):
    X, D2 = small
    rows = np.random.default_rng(49).integers(0, len(X), 700)
    rows[10:20] = rows[3]
    ref = check_radius(ctx, X, 0.1, 5, rows=rows, D2=D2)
    assert ref["count"].max() == 6 and 0 < ref["n_kept"] < 700
    mask = np.zeros(len(X), np.uint8)
    mask[::3] = 1
    check_radius(ctx, X, 0.1, 5, mask=mask, D2=D2, upload=False)
    check_radius(ctx, X, 0.1, 5, mask=np.zeros(len(X), np.uint8), D2=D2, upload=False)


def test_radius_on_a_gridded_cloud_in_cell_order(ctx):
    """enough candidates for the cell-ordered launch (one share per XCD), checked against the oracle on a sample of rows"""
    from simpleicp_amd import _lib
    X = np.ascontiguousarray(np.random.default_rng(50).uniform(0, 30, (60_000, 3)))
    ctx.upload(_lib.FIX, X)
    keep, cnt, kept = ctx.outlier_radius(_lib.FIX, 1.0, 9)
    assert kept == int(keep.sum())
    rows = np.random.default_rng(51).choice(len(X), 1500, replace=False)
    d2 = outlier_ref.neighbour_d2(X, 64, rows)
    full = np.count_nonzero(d2 < 1.0, axis=1)
    assert full.max() < 64
    assert np.array_equal(cnt[rows], np.minimum(full, 10).astype(np.uint32)) and np.array_equal(keep[rows], full > 9)


def test_radius_cell_box_limit(ctx):
    from simpleicp_amd import _lib
    X = np.ascontiguousarray(np.random.default_rng(52).uniform(0, 100, (200_000, 3)))        # a grid of more cells than the limit
    ctx.upload(_lib.FIX, X)
    lo, hi = 1e-3, 200.0
    assert ctx.outlier_radius_cells(_lib.FIX, lo)[3] <= _lib.OUTLIER_MAX_BOX_CELLS < ctx.outlier_radius_cells(_lib.FIX, hi)[3]
    for _ in range(200):                                             # the largest accepted radius, to the ulp
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if ctx.outlier_radius_cells(_lib.FIX, mid)[3] <= _lib.OUTLIER_MAX_BOX_CELLS:
            lo = mid
        else:
            hi = mid
    assert hi == np.nextafter(lo, np.inf)
    ex = ctx.outlier_radius_cells(_lib.FIX, hi)
    assert ex[0] * ex[1] * ex[2] == ex[3] > _lib.OUTLIER_MAX_BOX_CELLS
    with pytest.raises(_lib.BackendError) as e:
        ctx.outlier_radius(_lib.FIX, hi, 3)
    msg = str(e.value)
    assert e.value.code == _lib.ERR_INVALID and f"radius {hi:g}" in msg and f"{ex[0]} x {ex[1]} x {ex[2]} = {ex[3]} grid cells" in msg
    assert f"at most {_lib.OUTLIER_MAX_BOX_CELLS}" in msg
    rows = np.arange(0, len(X), 2000)                                 # just inside: accepted, and right
    keep, cnt, kept = ctx.outlier_radius(_lib.FIX, lo, 3, rows=rows)
    d2 = outlier_ref.neighbour_d2(X, 4, rows)
    assert np.array_equal(cnt, np.minimum(np.count_nonzero(d2 < lo * lo, axis=1), 4).astype(np.uint32))


# ---- refusals ----
def refused(fn, *fragments):
    from simpleicp_amd import _lib
    with pytest.raises(_lib.BackendError) as e:
        fn()
    assert e.value.code == _lib.ERR_INVALID, str(e.value)
    for f in fragments:
        assert f in str(e.value), str(e.value)


def test_refusals(ctx):
    from simpleicp_amd import _lib
    X = np.ascontiguousarray(np.random.default_rng(53).normal(0, 1, (100, 3)))
    ctx.upload(_lib.FIX, X)
    S, R, F = ctx.outlier_statistical, ctx.outlier_radius, _lib.FIX
    t = torch.ones(100, dtype=torch.uint8, device=DEV)
    L, kept, st, buf = ctx._L, C_.c_int64(), _lib.OutlierStats(), np.zeros(100, np.uint8)
    # null outputs
    assert L.sicp_outlier_statistical(ctx._h, F, None, 0, None, 5, 2.0, None, None, C_.byref(st)) == _lib.ERR_INVALID
    assert b"keep_out" in L.sicp_last_error()
    assert L.sicp_outlier_statistical(ctx._h, F, None, 0, None, 5, 2.0, _lib._ptr(buf), None, None) == _lib.ERR_INVALID
    assert b"out is null" in L.sicp_last_error()
    assert L.sicp_outlier_radius(ctx._h, F, None, 0, None, 1.0, 1, None, None, C_.byref(kept)) == _lib.ERR_INVALID
    assert b"keep_out" in L.sicp_last_error()
    assert L.sicp_outlier_radius(ctx._h, F, None, 0, None, 1.0, 1, _lib._ptr(buf), None, None) == _lib.ERR_INVALID
    assert b"kept_out" in L.sicp_last_error()
    # rows together with a mask
    r5 = np.arange(5, dtype=np.int64)
    assert L.sicp_outlier_statistical(ctx._h, F, _lib._ptr(r5), 5, C_.c_void_p(t.data_ptr()), 5, 2.0, _lib._ptr(buf), None,
                                      C_.byref(st)) == _lib.ERR_INVALID
    assert b"rows and mask" in L.sicp_last_error()
    assert L.sicp_outlier_radius(ctx._h, F, _lib._ptr(r5), 5, C_.c_void_p(t.data_ptr()), 1.0, 1, _lib._ptr(buf), None,
                                 C_.byref(kept)) == _lib.ERR_INVALID
    assert b"rows and mask" in L.sicp_last_error()
    # rows out of range
    refused(lambda: S(F, 5, 2.0, rows=[0, 100]), "rows[1] = 100")
    refused(lambda: R(F, 1.0, 1, rows=[-1]), "rows[0] = -1")
    # k, std_ratio
    refused(lambda: S(F, 1, 2.0), "k must be >= 2")
    refused(lambda: S(F, 101, 2.0), "k (101) exceeds the number of points (100)")
    refused(lambda: S(F, 129, 2.0), "k must be <= 128")
    for bad in (float("nan"), float("inf"), -float("inf")):
        refused(lambda: S(F, 5, bad), "std_ratio")
    assert S(F, 5, -3.0)[2].n_kept >= 0                              # a negative ratio is allowed
    # radius, min_points
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused(lambda: R(F, bad, 1), "radius")
        refused(lambda: ctx.outlier_radius_cells(F, bad), "radius")
    refused(lambda: R(F, 1.0, -1), "min_points")
    # a mask in host memory
    assert L.sicp_outlier_statistical(ctx._h, F, None, 0, _lib._ptr(buf), 5, 2.0, _lib._ptr(buf), None, C_.byref(st)) == _lib.ERR_INVALID
    assert b"mask is not device memory" in L.sicp_last_error()
    # an empty slot, a shard
    with _lib.Context(0) as other:
        refused(lambda: other.outlier_statistical(_lib.MOV, 5, 2.0), "empty")
        refused(lambda: other.outlier_radius(_lib.MOV, 1.0, 1), "empty")
        other.upload(_lib.MOV, X, index_base=7)
        refused(lambda: other.outlier_statistical(_lib.MOV, 5, 2.0), "shard")
        refused(lambda: other.outlier_radius(_lib.MOV, 1.0, 1), "shard")
    # an exchange
    ctx.set_exchange(lambda *a: 0, 0, 1)
    try:
        refused(lambda: S(F, 5, 2.0), "not supported with an exchange")
        refused(lambda: R(F, 1.0, 1), "not supported with an exchange")
    finally:
        ctx.set_exchange(None, 0, 1)
    check_stat(ctx, X, 5, 2.0)                                       # and the context still works


def test_two_calls_and_two_contexts_give_the_same_bytes(ctx, seeded):
    from simpleicp_amd import _lib
    X, _ = seeded
    ctx.upload(_lib.FIX, X)
    a = ctx.outlier_statistical(_lib.FIX, 20, 1.0)
    b = ctx.outlier_statistical(_lib.FIX, 20, 1.0)
    ra, rb = ctx.outlier_radius(_lib.FIX, 0.5, 6), ctx.outlier_radius(_lib.FIX, 0.5, 6)
    with _lib.Context(0) as other:
        other.upload(_lib.FIX, X)
        c = other.outlier_statistical(_lib.FIX, 20, 1.0)
        rc = other.outlier_radius(_lib.FIX, 0.5, 6)
    for x in (b, c):
        assert np.array_equal(x[0], a[0]) and np.array_equal(bits(x[1]), bits(a[1])) and x[2].as_dict() == a[2].as_dict()
    for x in (rb, rc):
        assert np.array_equal(x[0], ra[0]) and np.array_equal(x[1], ra[1]) and x[2] == ra[2]


def test_voxel_selection_and_the_filters_share_their_candidate_buffers(seeded):
    """a voxel selection by rows and a radius filter by mask take their candidates through the same buffers of the context: after
    one another, in either order, each gives what it gives on a fresh context"""
    from simpleicp_amd import _lib
    X = seeded[0][:5000]
    rng = np.random.default_rng(47)
    rows = rng.integers(0, len(X), 3001)
    mask = torch.tensor((rng.random(len(X)) < 0.4).astype(np.uint8), device=DEV)

    def voxel(c):
        return c.voxel_select(_lib.FIX, 0.7, rows=rows)

    def radius(c):
        keep = torch.full((len(X),), 7, dtype=torch.uint8, device=DEV)
        cnt = torch.full((len(X),), 77, dtype=torch.int32, device=DEV)
        kept = c.outlier_radius(_lib.FIX, 0.5, 6, mask_ptr=mask.data_ptr(), keep_ptr=keep.data_ptr(), count_ptr=cnt.data_ptr())
        return keep.cpu().numpy(), cnt.cpu().numpy(), kept

    want = {}
    for name, op in (("voxel", voxel), ("radius", radius)):
        with _lib.Context(0) as fresh:
            fresh.upload(_lib.FIX, X)
            want[name] = op(fresh)
    assert 0 < want["voxel"].sum() < len(rows) and 0 < want["radius"][2] < int(mask.sum())
    for order in ((voxel, radius), (radius, voxel)):
        with _lib.Context(0) as c:
            c.upload(_lib.FIX, X)
            for op in order + order:                                   # ... and once more, behind the other one
                got, ref = op(c), want["voxel" if op is voxel else "radius"]
                if op is voxel:
                    assert np.array_equal(got, ref)
                else:
                    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and got[2] == ref[2]


# ---- Python ----
def dev(X, dtype=torch.float64):
    return torch.tensor(np.asarray(X), dtype=dtype, device=DEV)


def test_outlier_keep_on_tensors(seeded):
    from simpleicp_amd import outlier_keep
    X = seeded[0][:6000].copy()
    X[-50:] += 20.0
    got = outlier_keep(dev(X), neighbors=12, std_ratio=1.5)
    assert got.dtype == torch.bool and got.device.type == "cuda"
    assert np.array_equal(got.cpu().numpy(), outlier_ref.statistical(X, 12, 1.5)["keep"])
    X32 = X.astype(np.float32)
    wide = X32.astype(np.float64)                                    # float32 is widened exactly before anything is computed
    assert np.array_equal(outlier_keep(dev(X32, torch.float32), neighbors=12, std_ratio=1.5).cpu().numpy(),
                          outlier_ref.statistical(wide, 12, 1.5)["keep"])
    big = torch.zeros((len(X), 7), dtype=torch.float64, device=DEV)
    big[:, 1::2] = dev(X)
    strided = big[:, 1::2]
    assert not strided.is_contiguous()
    mask = torch.tensor(np.arange(len(X)) % 2 == 0, device=DEV)
    assert np.array_equal(outlier_keep(strided, neighbors=12, std_ratio=1.5, mask=mask).cpu().numpy(),
                          outlier_ref.statistical(X, 12, 1.5, mask=mask.cpu().numpy())["keep"])
    Xs = X[:2000]
    D2 = outlier_ref.all_d2(Xs)
    assert np.array_equal(outlier_keep(dev(Xs), radius=0.6, min_points=4).cpu().numpy(), outlier_ref.radius(Xs, 0.6, 4, D2=D2)["keep"])
    m2 = torch.tensor((np.arange(2000) % 3 == 0).astype(np.uint8), device=DEV)
    assert np.array_equal(outlier_keep(dev(Xs), radius=0.6, min_points=4, mask=m2).cpu().numpy(),
                          outlier_ref.radius(Xs, 0.6, 4, mask=m2.cpu().numpy(), D2=D2)["keep"])
    assert outlier_keep(torch.zeros((0, 3), dtype=torch.float64, device=DEV), neighbors=5).shape == (0,)


def test_point_cloud_selections(seeded):
    from simpleicp_amd import PointCloud
    X = seeded[0][:5000].copy()
    X[-40:] += 20.0
    pc = PointCloud(X, columns=["x", "y", "z"])
    pc.select_by_indices(np.arange(300, 5000))
    pc.select_statistical_inliers(16, 1.0)
    ref = outlier_ref.statistical(X, 16, 1.0, rows=np.arange(300, 5000))
    assert np.array_equal(pc.idx_selected, np.arange(300, 5000)[ref["keep"]])
    assert pc.last_outlier_stats == {key: ref[key] for key in KEYS}
    first = pc.idx_selected
    Xs = X[:2000]
    ps = PointCloud(Xs, columns=["x", "y", "z"])
    ps.select_by_indices(np.arange(100, 1900))
    ps.select_radius_inliers(0.6, 4)
    assert np.array_equal(ps.idx_selected, np.arange(100, 1900)[outlier_ref.radius(Xs, 0.6, 4, rows=np.arange(100, 1900))["keep"]])
    pc.select_n_points(20)
    assert pc.num_selected_points == 20 and np.isin(pc.idx_selected, first).all()


# ---- end to end ----
KW = dict(correspondences=600, max_iterations=30)


@pytest.fixture(scope="module")
def pair():
    from test_gpu_voxel import surface_pair
    Xf, Xm = surface_pair(20_000, 31)
    rng = np.random.default_rng(32)
    at = rng.choice(len(Xf), 150, replace=False)
    Xf = Xf.copy()
    Xf[at, 2] += rng.uniform(1.0, 3.0, 150)                          # strays above the surface
    return Xf, Xm


def lone(Xf, Xm, prefilter=None, outlier=None, **kw):
    from simpleicp_amd import PointCloud, SimpleICP
    icp = SimpleICP(verbose=False)
    pc1 = PointCloud(np.array(Xf, dtype=np.float64), columns=["x", "y", "z"])
    if prefilter is not None:
        pc1.select_statistical_inliers(*prefilter)
    icp.add_point_clouds(pc1, PointCloud(np.array(Xm, dtype=np.float64), columns=["x", "y", "z"]))
    if outlier is not None:
        icp.outlier_neighbors, icp.outlier_std_ratio = outlier
    return icp.run(**kw), icp.last_run_info, pc1.idx_selected


@pytest.fixture(scope="module")
def ref_run(pair):
    """a run() without the option whose fixed cloud went through select_statistical_inliers(20, 2.0) first"""
    Xf, Xm = pair
    return lone(Xf, Xm, prefilter=(20, 2.0), **KW)


def test_run_equals_run_on_the_prefiltered_cloud(pair, ref_run):
    from test_gpu_voxel import same
    Xf, Xm = pair
    out, info, sel = lone(Xf, Xm, outlier=(20, 2.0), **KW)
    same(out, ref_run[0], ref_run[1])
    assert info["iterations"] == ref_run[1]["iterations"] and np.array_equal(info["stats"], ref_run[1]["stats"])
    assert np.array_equal(sel, ref_run[2])
    ref = outlier_ref.statistical(Xf, 20, 2.0)
    assert info["outlier"] == {key: ref[key] for key in KEYS} and 0 < ref["n_kept"] < len(Xf)
    assert np.isin(sel, np.flatnonzero(ref["keep"])).all()
    plain, pinfo, _ = lone(Xf, Xm, **KW)                              # off: another selection, no statistics
    assert "outlier" not in pinfo and not np.array_equal(plain[0], out[0])


def test_run_tensors_and_run_batch_equal_that_run(pair, ref_run):
    from simpleicp_amd import backend, run_batch, run_tensors
    from test_gpu_voxel import same, surface_pair
    Xf, Xm = pair
    res = run_tensors(dev(Xf), dev(Xm), outlier_neighbors=20, **KW)
    assert res.path == "device" and res.error is None
    same(res, ref_run[0], ref_run[1], X_dev=True)
    ref = outlier_ref.statistical(Xf, 20, 2.0)
    assert res.outlier == {key: ref[key] for key in KEYS}
    Xf2, Xm2 = surface_pair(15_000, 33)
    today2 = lone(Xf2, Xm2, **KW)
    try:
        alone = run_batch([(Xf, Xm)], outlier_neighbors=20, **KW)
        assert alone[0].path == "batched" and alone[0].error is None
        same(alone[0], ref_run[0], ref_run[1])
        out = run_batch([(Xf, Xm), (Xf2, Xm2), (dev(Xf), dev(Xm))],
                        per_pair=[{"outlier_neighbors": 20}, None, {"outlier_neighbors": 20, "outlier_std_ratio": 2.0}], **KW)
        assert [r.path for r in out] == ["batched"] * 3 and all(r.error is None for r in out)
        same(out[0], ref_run[0], ref_run[1])
        same(out[1], today2[0], today2[1])                            # the pair without the option: today's result
        same(out[2], ref_run[0], ref_run[1], X_dev=True)
        assert out[0].outlier == out[2].outlier == res.outlier and out[1].outlier is None
    finally:
        backend.reset_batch_contexts()


def test_with_the_overlap_pass_the_selection_is_the_masked_reference(pair):
    from simpleicp_amd import _lib, run_tensors
    Xf, Xm = pair
    with _lib.Context(0) as side:
        side.upload(_lib.FIX, Xf)
        side.upload(_lib.MOV, Xm)
        near = side.select_in_range(_lib.FIX, _lib.MOV, None, np.eye(4), 0.25)
    assert 0.2 < near.mean() < 0.95
    ref = outlier_ref.statistical(Xf, 20, 2.0, mask=near)
    inl = np.flatnonzero(ref["keep"])
    out, info, sel = lone(Xf, Xm, outlier=(20, 2.0), max_overlap_distance=0.25, **KW)
    assert np.array_equal(sel, np.unique(inl[np.round(np.linspace(0, len(inl) - 1, 600)).astype(int)]))
    # run() hands the in-range rows over as a list (the trees run over its entries), the device road hands the mask over (over all
    # points): the statistics are each form's own, the verdicts the same
    by_rows = outlier_ref.statistical(Xf, 20, 2.0, rows=np.flatnonzero(near))
    assert info["outlier"] == {key: by_rows[key] for key in KEYS} and np.array_equal(by_rows["keep"], ref["keep"][near])
    res = run_tensors(dev(Xf), dev(Xm), outlier_neighbors=20, max_overlap_distance=0.25, **KW)
    assert np.array_equal(res[0], out[0]) and np.array_equal(res[3], out[3])
    assert res.outlier == {key: ref[key] for key in KEYS}
