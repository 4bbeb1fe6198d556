"""Voxel selection on the GPU (contract (V)): every verdict byte, count and kept row equals the numpy
reference of tests/voxel_ref.py bit for bit -- adversarial inputs, seeded random clouds, the bundled scans, the full-size clouds --,
voxel_keep on tensors, and the end-to-end identities of run(), run_tensors and run_batch."""
import numpy as np
import pytest
import torch

import voxel_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ctx():
    from simpleicp_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def check(ctx, X, c, o=None, rows=None, mask=None):
    """One call against the reference: verdict bytes, count, kept rows.  Returns the number kept."""
    from simpleicp_amd import _lib
    X = np.ascontiguousarray(X, dtype=np.float64)
    ctx.upload(_lib.FIX, X)
    oo = (0.0, 0.0, 0.0) if o is None else o
    want = voxel_ref.keep(X, c, oo, rows=rows, mask=mask)
    if mask is not None:
        m = torch.tensor(np.asarray(mask, dtype=np.uint8), device=DEV)
        out = torch.full((len(X),), 7, dtype=torch.uint8, device=DEV)
        kept = ctx.voxel_select_masked(_lib.FIX, m.data_ptr(), len(X), c, o, keep_ptr=out.data_ptr())
        got = out.cpu().numpy()
        assert np.array_equal(m.cpu().numpy(), np.asarray(mask, dtype=np.uint8))            # the mask itself is left alone ...
        kept2 = ctx.voxel_select_masked(_lib.FIX, m.data_ptr(), len(X), c, o)               # ... unless the verdicts go over it
        assert kept2 == kept and np.array_equal(m.cpu().numpy(), got)
    else:
        got = ctx.voxel_select(_lib.FIX, c, o, rows).view(np.uint8)
        kept = int(got.sum())
        # the same verdicts into device memory, and the count the call reports
        out = torch.full((len(got),), 7, dtype=torch.uint8, device=DEV)
        assert ctx.voxel_select(_lib.FIX, c, o, rows, keep_ptr=out.data_ptr()) == kept
        assert np.array_equal(out.cpu().numpy(), got)
    assert got.dtype == np.uint8 and set(np.unique(got)) <= {0, 1}
    assert np.array_equal(got, want.view(np.uint8))
    assert kept == int(want.sum())
    r = np.arange(len(X)) if rows is None else np.asarray(rows)
    assert np.array_equal(np.sort(r[got.astype(bool)]), voxel_ref.kept_rows(X, c, oo, rows=rows, mask=mask))
    return kept


# ---- adversarial inputs ----
def test_points_on_lattice_planes_negative_coordinates_and_negative_zero(ctx):
    c = 0.25
    g = np.arange(-12, 13) * c                                       # every coordinate exactly on a plane
    X = np.array(np.meshgrid(g, g, g[:5], indexing="ij")).reshape(3, -1).T.copy()
    X = np.concatenate([X, -X, X * 1.0000000000000002, X - 2.0 ** -52])
    X[::7] *= -1.0
    X[3] = [-0.0, 0.0, -0.0]
    X[4] = [0.0, -0.0, 0.0]
    X[5] = [-1e-300, 1e-300, -0.0]
    assert np.signbit(X[3, 0]) and (X == 0).any()
    check(ctx, X, c)
    check(ctx, X, 0.1)                                               # a cell that is no binary fraction: the division rounds
    check(ctx, X, 0.3, (0.1, -0.7, 0.05))


def test_duplicates_one_voxel_and_own_voxels(ctx):
    rng = np.random.default_rng(11)
    X = rng.uniform(-5, 5, (20_000, 3))
    X[5000:9000] = X[rng.integers(0, 5000, 4000)]                    # exact duplicates
    assert check(ctx, X, 0.5) < 16_000
    assert check(ctx, X, 1e-5) == 16_000                             # every distinct point its own voxel: 10^6 cells per axis


def test_extent_is_refused_with_the_axis_and_nothing_is_truncated(ctx):
    from simpleicp_amd import _lib
    rng = np.random.default_rng(12)
    X = rng.uniform(0, 1, (1000, 3))
    X[:, 1] *= 3.0                                                   # y is the widest axis
    ctx.upload(_lib.FIX, X)
    span = X[:, 1].max() - X[:, 1].min()
    with pytest.raises(_lib.BackendError) as e:
        ctx.voxel_select(_lib.FIX, span / 2.0 ** 21 * 0.999)         # just outside 2^21 cells along y
    assert e.value.code == _lib.ERR_INVALID
    assert "along y" in str(e.value) and "2^21" in str(e.value) and re_extent(str(e.value)) > 2 ** 21
    assert check(ctx, X, span / 2.0 ** 21 * 1.01) == 1000            # just inside: every point its own voxel
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.BackendError, match="cell"):
            ctx.voxel_select(_lib.FIX, bad)
    with pytest.raises(_lib.BackendError, match="origin"):
        ctx.voxel_select(_lib.FIX, 0.1, (0.0, float("nan"), 0.0))
    with pytest.raises(_lib.BackendError, match="rows"):
        ctx.voxel_select(_lib.FIX, 0.1, None, np.array([0, 1000]))
    t = torch.zeros(999, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.BackendError, match="slot's size"):
        ctx.voxel_select_masked(_lib.FIX, t.data_ptr(), 999, 0.1)
    with pytest.raises(_lib.BackendError, match="device memory"):
        ctx.voxel_select_masked(_lib.FIX, np.zeros(1000, np.uint8).ctypes.data, 1000, 0.1)


def re_extent(msg):
    import re
    return float(re.search(r"spans (\d+) cells", msg).group(1))


def test_all_in_one_voxel_own_voxels_and_a_cell_larger_than_the_cloud(ctx):
    rng = np.random.default_rng(13)
    X = rng.uniform(0.01, 0.99, (30_000, 3))
    assert check(ctx, X, 1.0) == 1                                   # all points in one voxel
    assert check(ctx, X, 1e6, (-5e5, -5e5, -5e5)) == 1               # a cell larger than the cloud, the cloud at its centre
    assert check(ctx, X, 1e-6) >= 29_990                             # (nearly) every point in its own voxel, 10^6 cells per axis
    X[:, 2] = np.arange(len(X)) * 0.5
    assert check(ctx, X, 0.5) == len(X)                              # exactly every point in its own voxel


def test_origin_rows_and_masks(ctx):
    rng = np.random.default_rng(14)
    X = rng.normal(0, 2, (50_000, 3))
    a = check(ctx, X, 0.4)
    b = check(ctx, X, 0.4, (0.13, -0.21, 1e-3))
    assert a != b
    # rows: a subset whose order has nothing to do with the voxels' occupancy, then with repeated entries
    rows = rng.permutation(len(X))[:20_000]
    check(ctx, X, 0.4, rows=rows)
    check(ctx, X, 0.4, (0.13, -0.21, 1e-3), rows=np.sort(rows)[::-1].copy())
    dup = np.concatenate([rows[:500], rows[:500], rows[100:200]])
    check(ctx, X, 0.4, rows=dup)
    check(ctx, X, 0.4, rows=np.array([17]))
    # masks: no byte, one byte, all bytes, any non-zero value counts
    none = np.zeros(len(X), np.uint8)
    assert check(ctx, X, 0.4, mask=none) == 0
    one = none.copy()
    one[31_337] = 1
    assert check(ctx, X, 0.4, mask=one) == 1
    assert check(ctx, X, 0.4, mask=np.ones(len(X), np.uint8)) == a
    some = (rng.random(len(X)) < 0.3).astype(np.uint8) * rng.integers(1, 256, len(X)).astype(np.uint8)
    check(ctx, X, 0.4, mask=some)


@pytest.mark.parametrize("factor", [1.0, 2.0, 1.0 / 3.0])
def test_regular_point_lattice_the_hash_s_worst_case(ctx, factor):
    c = 0.125
    s = c * factor
    g = np.arange(64) * s
    X = np.array(np.meshgrid(g, g, g, indexing="ij")).reshape(3, -1).T.copy()       # 262 144 points
    kept = check(ctx, X, c)
    if factor >= 1.0:
        assert kept == len(X)
    check(ctx, X[np.random.default_rng(15).permutation(len(X))], c, (c / 2, c / 2, c / 2))


def test_coordinates_around_a_million(ctx):
    rng = np.random.default_rng(16)
    X = 1e6 + rng.uniform(-40_000, 40_000, (200_000, 3))             # 1.6e6 cells of 0.05 per axis: inside 2^21
    X[:, 2] = 1e6 + rng.uniform(-30, 30, len(X))
    X[1000:2000] = X[:1000] + 1e-3
    check(ctx, X, 0.05)
    check(ctx, -X, 0.05, (17.0, -3.0, 0.025))


# ---- random clouds and the bundled scans ----
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 1000, 4097, 100_000, 1_000_003])
def test_seeded_random_clouds(ctx, n):
    rng = np.random.default_rng(n)
    X = rng.normal(0, 3, (n, 3)) * rng.uniform(0.2, 3, 3)
    for c in (0.05, 0.5, 4.0):
        check(ctx, X, c, tuple(rng.uniform(-1, 1, 3)))
    if n > 100:
        check(ctx, X, 0.5, rows=rng.permutation(n)[: n // 3])
        check(ctx, X, 0.5, mask=(rng.random(n) < 0.5).astype(np.uint8))


@pytest.mark.parametrize("stem", ["dragon1", "bunny_part1"])
def test_bundled_scans(ctx, clouds, stem):
    X = clouds(stem)
    span = (X.max(axis=0) - X.min(axis=0)).max()
    counts = [check(ctx, X, span / d) for d in (8, 64, 512)]
    assert counts[0] < counts[1] < counts[2] <= len(X)


def test_repeatability(ctx):
    from simpleicp_amd import _lib
    rng = np.random.default_rng(17)
    X = rng.normal(0, 2, (300_000, 3))
    ctx.upload(_lib.FIX, X)
    a = ctx.voxel_select(_lib.FIX, 0.2).copy()
    ctx.voxel_select(_lib.FIX, 3.0, None, rng.permutation(len(X))[:1000])       # another call in between: the table is reused
    b = ctx.voxel_select(_lib.FIX, 0.2)
    assert a.tobytes() == b.tobytes()
    with _lib.Context(0) as other:                                    # another context, a table of its own
        other.upload(_lib.MOV, X)
        assert other.voxel_select(_lib.MOV, 0.2).tobytes() == a.tobytes()


# ---- full size ----
def test_full_size_uniform_cloud(ctx):
    X = voxel_ref.uniform_surface(10_000_000)
    kept = check(ctx, X, 0.5)
    assert 1_000_000 < kept < len(X)


def test_full_size_terrestrial_stand_in(ctx):
    X = voxel_ref.terrestrial_scan(1_250_000)
    kept = check(ctx, X, 0.1)
    assert kept < len(X) // 2                                        # the dense core collapses, the far walls do not
    check(ctx, X, 1.0, mask=(np.linalg.norm(X, axis=1) > 10.0).astype(np.uint8))
    sparse = np.zeros(len(X), np.uint8)                              # few candidates in a large cloud: the table follows the mask
    sparse[np.random.default_rng(23).permutation(len(X))[:700]] = 1
    check(ctx, X, 0.5, mask=sparse)


# ---- voxel_keep ----
def dev(X, dtype=torch.float64):
    return torch.tensor(np.asarray(X), dtype=dtype, device=DEV)


def test_voxel_keep_on_tensors():
    from simpleicp_amd import voxel_keep
    rng = np.random.default_rng(18)
    X = rng.normal(0, 2, (120_000, 3))
    c, o = 0.3, (0.05, 0.0, -0.1)
    for dtype in (torch.float64, torch.float32):
        t = dev(X, dtype)
        wide = t.double().cpu().numpy()                               # float32 is widened exactly before the formula
        k = voxel_keep(t, c, o)
        assert k.dtype == torch.bool and k.shape == (len(X),) and k.is_cuda
        assert np.array_equal(k.cpu().numpy(), voxel_ref.keep(wide, c, o))
        assert np.array_equal(voxel_keep(t, c).cpu().numpy(), voxel_ref.keep(wide, c))
        # a strided (n, 6) view
        six = torch.zeros((len(X), 6), dtype=dtype, device=DEV)
        six[:, 3:] = t
        view = six[:, 3:]
        assert not view.is_contiguous()
        assert torch.equal(voxel_keep(view, c, o), k)
        # mask=, bool and uint8
        m = rng.random(len(X)) < 0.4
        want = voxel_ref.keep(wide, c, o, mask=m)
        assert np.array_equal(voxel_keep(t, c, o, mask=torch.tensor(m, device=DEV)).cpu().numpy(), want)
        assert np.array_equal(voxel_keep(t, c, o, mask=torch.tensor(m.astype(np.uint8) * 9, device=DEV)).cpu().numpy(), want)
        # a strided mask (a column of a label tensor): its contiguous copy is made by torch, before the library may read it
        labels = torch.zeros((len(X), 4), dtype=torch.uint8, device=DEV)
        labels[:, 2] = torch.tensor(m.astype(np.uint8) * 3, device=DEV)
        col = labels[:, 2]
        assert not col.is_contiguous()
        for _ in range(3):
            assert np.array_equal(voxel_keep(t, c, o, mask=col).cpu().numpy(), want)
        flags = torch.tensor(np.column_stack((~m, m)), device=DEV)[:, 1]            # a strided bool column
        assert not flags.is_contiguous() and np.array_equal(voxel_keep(t, c, o, mask=flags).cpu().numpy(), want)
        assert torch.equal(t, dev(X, dtype))                          # the input is untouched
        thin = t[k]
        assert thin.shape == (int(k.sum()), 3)
    assert voxel_keep(torch.zeros((0, 3), dtype=torch.float64, device=DEV), 1.0).shape == (0,)
    with pytest.raises(TypeError, match="mask"):
        voxel_keep(dev(X), c, mask=torch.zeros(5, dtype=torch.bool, device=DEV))


# ---- end to end ----
def surface_pair(n, seed, shift=(0.3, -0.2, 0.1), yaw=0.02):
    rng = np.random.default_rng(seed)
    half = np.sqrt(n / 10.0) / 2
    xy = rng.uniform(-half, half, (n, 2))
    z = 2 * np.sin(xy[:, 0] / 4) * np.cos(xy[:, 1] / 6) + rng.normal(0, 0.005, n)
    Xf = np.column_stack((xy, z))
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    Xm = (Xf + rng.normal(0, 0.005, Xf.shape)) @ R.T + np.array(shift)
    return Xf, Xm


def lone(Xf, Xm, selected=None, voxel=None, **kw):
    """SimpleICP.run on copies of two arrays (the fixed cloud's `selected` mask preset, or voxel = (size, origin)): its return,
    its last_run_info, the fixed cloud's selection afterwards."""
    from simpleicp_amd import PointCloud, SimpleICP
    icp = SimpleICP(verbose=False)
    pc1 = PointCloud(np.array(Xf, dtype=np.float64), columns=["x", "y", "z"])
    if selected is not None:
        pc1["selected"] = np.asarray(selected, dtype=bool)
    icp.add_point_clouds(pc1, PointCloud(np.array(Xm, dtype=np.float64), columns=["x", "y", "z"]))
    if voxel is not None:
        icp.voxel_size, icp.voxel_origin = voxel
    return icp.run(**kw), icp.last_run_info, pc1.idx_selected


def same(res, ref, info, X_dev=False):
    H, X, rbp, resid = ref
    assert np.array_equal(res[0], H)
    Xr = res[1].cpu().numpy() if X_dev else res[1]
    assert np.array_equal(Xr, X)
    assert np.array_equal(res[3], resid)
    for name in ("alpha1", "alpha2", "alpha3", "tx", "ty", "tz"):
        a, b = getattr(res[2], name), getattr(rbp, name)
        assert a.estimated_value == b.estimated_value and a.initial_value == b.initial_value
        assert np.array_equal(a.estimated_uncertainty, b.estimated_uncertainty, equal_nan=True)
    if hasattr(res, "iterations"):
        assert res.iterations == info["iterations"]


C, O = 0.9, (0.2, -0.1, 0.05)
KW = dict(correspondences=600, max_iterations=30)


@pytest.fixture(scope="module")
def pair():
    return surface_pair(60_000, 21)


@pytest.fixture(scope="module")
def refs(pair):
    """today's run() on the fixed cloud thinned on the host, without and with the overlap pre-pass's verdicts"""
    from simpleicp_amd import _lib
    Xf, Xm = pair
    full = lone(Xf, Xm, selected=voxel_ref.keep(Xf, C, O), **KW)
    with _lib.Context(0) as side:
        side.upload(_lib.FIX, Xf)
        side.upload(_lib.MOV, Xm)
        near = side.select_in_range(_lib.FIX, _lib.MOV, None, np.eye(4), 0.25)
    assert 0.2 < near.mean() < 0.95
    part = lone(Xf, Xm, selected=near & voxel_ref.keep(Xf, C, O, mask=near), **KW)
    assert len(full[2]) == 600 and len(part[2]) == 600               # select_n_points had something to thin in both
    assert not np.array_equal(full[0][0], part[0][0])
    return full, part


def test_run_equals_run_on_the_host_thinned_selection(pair, refs):
    Xf, Xm = pair
    for ref, d in zip(refs, (np.inf, 0.25)):
        out, info, sel = lone(Xf, Xm, voxel=(C, O), max_overlap_distance=d, **KW)
        same(out, ref[0], ref[1])
        assert info["iterations"] == ref[1]["iterations"] and np.array_equal(info["stats"], ref[1]["stats"])
        assert np.array_equal(sel, ref[2])
    # and without the attribute the selection is index-even, as before
    out, info, sel = lone(Xf, Xm, **KW)
    assert np.array_equal(sel, np.unique(np.round(np.linspace(0, len(Xf) - 1, 600)).astype(np.int64)))


def test_run_tensors_equals_the_same_runs(pair, refs):
    from simpleicp_amd import run_tensors
    Xf, Xm = pair
    for ref, d in zip(refs, (np.inf, 0.25)):
        res = run_tensors(dev(Xf), dev(Xm), voxel_size=C, voxel_origin=O, max_overlap_distance=d, **KW)
        assert res.path == "device" and res.error is None
        same(res, ref[0], ref[1], X_dev=True)


def test_run_batch_keeps_voxel_pairs_batched(pair, refs):
    from simpleicp_amd import backend, run_batch
    Xf, Xm = pair
    Xf2, Xm2 = surface_pair(30_000, 22)
    today2 = lone(Xf2, Xm2, **KW)
    try:
        out = run_batch([(Xf, Xm), (Xf2, Xm2), (dev(Xf), dev(Xm)), (Xf, Xm)],
                        per_pair=[{"voxel_size": C, "voxel_origin": O}, None,
                                  {"voxel_size": C, "voxel_origin": O, "max_overlap_distance": 0.25},
                                  {"voxel_size": C, "voxel_origin": O, "max_overlap_distance": 0.25}], **KW)
        assert [r.path for r in out] == ["batched"] * 4 and all(r.error is None for r in out)
        same(out[0], refs[0][0], refs[0][1])
        same(out[1], today2[0], today2[1])                            # the pair without a voxel size: today's result
        same(out[2], refs[1][0], refs[1][1], X_dev=True)
        same(out[3], refs[1][0], refs[1][1])
        # pooled contexts: the one that just ran a voxel pair gives a following pair without one its unchanged result
        again = run_batch([(Xf2, Xm2), (Xf, Xm)], **KW)
        today1 = lone(Xf, Xm, **KW)
        same(again[0], today2[0], today2[1])
        same(again[1], today1[0], today1[1])
        assert [r.path for r in again] == ["batched"] * 2
        # call-wide keywords reach every pair
        both = run_batch([(Xf, Xm), (Xf, Xm)], voxel_size=C, voxel_origin=O, per_pair=[None, {"max_overlap_distance": 0.25}], **KW)
        same(both[0], refs[0][0], refs[0][1])
        same(both[1], refs[1][0], refs[1][1])
    finally:
        backend.reset_batch_contexts()


def test_select_voxels_on_the_gpu(clouds):
    from simpleicp_amd import PointCloud
    X = clouds("dragon1")
    span = (X.max(axis=0) - X.min(axis=0)).max()
    pc = PointCloud(X, columns=["x", "y", "z"])
    pc.select_voxels(span / 100)
    assert np.array_equal(pc.idx_selected, voxel_ref.kept_rows(X, span / 100))
    first = pc.idx_selected
    pc.select_voxels(span / 10, origin=(span / 30, 0.0, 0.0))         # among the selected points only
    assert np.array_equal(pc.idx_selected, voxel_ref.kept_rows(X, span / 10, (span / 30, 0.0, 0.0), rows=first))
    pc.select_n_points(20)
    assert pc.num_selected_points == 20


def test_empty_selection_raises_like_an_empty_overlap(pair):
    from simpleicp_amd import SimpleICPException
    Xf, Xm = pair
    with pytest.raises(SimpleICPException, match="do not overlap"):
        lone(Xf, Xm + 1000.0, voxel=(C, O), max_overlap_distance=0.25, **KW)


# ---- refusals ----
def test_refused_with_an_exchange(ctx):
    from simpleicp_amd import _lib
    X = np.random.default_rng(19).normal(0, 1, (5000, 3))
    ctx.upload(_lib.FIX, X)
    ctx.set_exchange(lambda *a: 0, 0, 1)
    try:
        t = torch.ones(len(X), dtype=torch.uint8, device=DEV)
        with pytest.raises(_lib.BackendError) as e:
            ctx.voxel_select(_lib.FIX, 0.5)
        assert e.value.code == _lib.ERR_INVALID and "not supported with an exchange" in str(e.value)
        with pytest.raises(_lib.BackendError) as e:
            ctx.voxel_select_masked(_lib.FIX, t.data_ptr(), len(X), 0.5)
        assert e.value.code == _lib.ERR_INVALID and "not supported with an exchange" in str(e.value)
    finally:
        ctx.set_exchange(None, 0, 1)
    assert check(ctx, X, 0.5) > 0


def test_null_arguments_with_a_live_context(ctx):
    import ctypes as C_
    from simpleicp_amd import _lib
    ctx.upload(_lib.FIX, np.random.default_rng(20).normal(0, 1, (100, 3)))
    L, kept, buf = ctx._L, C_.c_int64(), np.zeros(100, np.uint8)
    assert L.sicp_voxel_select(ctx._h, _lib.FIX, None, 0, 0.5, None, None, C_.byref(kept)) == _lib.ERR_INVALID
    assert L.sicp_voxel_select(ctx._h, _lib.FIX, None, 0, 0.5, None, _lib._ptr(buf), None) == _lib.ERR_INVALID
    assert L.sicp_voxel_select(ctx._h, 5, None, 0, 0.5, None, _lib._ptr(buf), C_.byref(kept)) == _lib.ERR_INVALID
    assert L.sicp_voxel_select_masked(ctx._h, _lib.FIX, None, 100, 0.5, None, None, C_.byref(kept)) == _lib.ERR_INVALID
    assert L.sicp_voxel_select(ctx._h, _lib.MOV, None, 0, 0.5, None, _lib._ptr(buf), C_.byref(kept)) == _lib.ERR_INVALID   # an empty slot
    assert L.sicp_voxel_select(ctx._h, _lib.FIX, None, 0, 0.5, None, _lib._ptr(buf), C_.byref(kept)) == _lib.OK and kept.value > 0
