"""Planes of a cloud on the GPU (contracts (P) and (Q)) against tests/plane_ref.py: the planes' bytes, the
counts, keep_out and every field of both records for equality.  Every call goes to the C entry with outputs prefilled with a
pattern, and the inputs are compared with their bytes from before."""
import ctypes as C_
import os
from contextlib import contextmanager

import numpy as np
import pytest

import plane_ref

pytestmark = pytest.mark.gpu

PLANE_FILL, INL_FILL, KEEP_FILL = -123.25, -77, 0xAB
MD = 0.05


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


@pytest.fixture(scope="module")
def ctx():
    with context_with() as c:
        yield c


@pytest.fixture(scope="module")
def spans():
    """contexts whose scoring workgroups take 128 and 1 024 rows: many spans at small n"""
    with context_with(SICP_PLANE_SPAN=128) as a, context_with(SICP_PLANE_SPAN=1024) as b:
        yield {128: a, 1024: b}


def _u8(mask):
    return None if mask is None else np.ascontiguousarray(mask).astype(np.uint8)


def tri_call(ctx, X, mask, tri, md, want_planes=True):
    """sicp_plane_triplets: (planes or None, inliers, record as a dict)"""
    from simpleicp_amd import _lib
    X, tri, m = np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(tri, dtype=np.int32), _u8(mask)
    before = (X.tobytes(), tri.tobytes(), None if m is None else m.tobytes())
    h = len(tri)
    planes = np.full((h, 4), PLANE_FILL) if want_planes else None
    inl = np.full(h, INL_FILL, np.int32)
    st = _lib.PlaneStats()
    ctx._chk(ctx._L.sicp_plane_triplets(ctx._h, _lib._ptr(X), len(X), _lib._ptr(m), _lib._ptr(tri), h, float(md), _lib._ptr(planes),
                                        _lib._ptr(inl), C_.byref(st)))
    assert (X.tobytes(), tri.tobytes(), None if m is None else m.tobytes()) == before
    return planes, inl, st.as_dict()


def refit_call(ctx, X, mask, P, md, rounds, want_keep=False):
    """sicp_plane_refit: (planes, inliers, keep or None, record as a dict)"""
    from simpleicp_amd import _lib
    X, P, m = np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 4), _u8(mask)
    before = (X.tobytes(), P.tobytes(), None if m is None else m.tobytes())
    b = len(P)
    out, inl = np.full((b, 4), PLANE_FILL), np.full(b, INL_FILL, np.int32)
    keep = np.full(len(X), KEEP_FILL, np.uint8) if want_keep else None
    st = _lib.PlaneRefitStats()
    ctx._chk(ctx._L.sicp_plane_refit(ctx._h, _lib._ptr(X), len(X), _lib._ptr(m), _lib._ptr(P), b, float(md), int(rounds), _lib._ptr(out),
                                     _lib._ptr(inl), _lib._ptr(keep), C_.byref(st)))
    assert (X.tobytes(), P.tobytes(), None if m is None else m.tobytes()) == before
    assert keep is None or set(np.unique(keep)) <= {0, 1}
    return out, inl, (None if keep is None else keep.view(np.bool_)), st.as_dict()


def check_tri(ctx, X, mask, tri, md):
    want = plane_ref.triplets(X, mask, tri, md)
    got = tri_call(ctx, X, mask, tri, md)
    assert got[0].tobytes() == want[0].tobytes()
    assert np.array_equal(got[1], want[1]) and got[1].dtype == want[1].dtype
    assert got[2] == want[2] and tuple(got[2]) == plane_ref.KEYS
    return got


def check_refit(ctx, X, mask, P, md, rounds, want_keep=False):
    want = plane_ref.refit(X, mask, P, md, rounds, want_keep=want_keep)
    got = refit_call(ctx, X, mask, P, md, rounds, want_keep=want_keep)
    assert got[0].tobytes() == want[0].tobytes()
    assert np.array_equal(got[1], want[1])
    if want_keep:
        assert np.array_equal(got[2], want[2]) and int(got[2].sum()) == max(int(got[1][0]), 0)
    assert got[3] == want[3] and tuple(got[3]) == plane_ref.REFIT_KEYS
    return got


def seeded(seed, n, h, masked):
    """a plane with noise in clutter, h triples (three of them bad), a mask that drops a fifth of the rows (bytes 0 / 1 / 7) or None"""
    rng = np.random.default_rng(seed)
    X = plane_ref.plane_scene(seed, (3 * n) // 5, n - (3 * n) // 5)[0]
    tri = rng.integers(0, n, (h, 3), dtype=np.int32)
    if h >= 4:
        tri[1], tri[2], tri[3] = (0, n, 1), (2, 2, 1), (-1, 0, 1)
    mask = None
    if masked:
        mask = np.where(rng.random(n) < 0.2, 0, rng.choice([1, 7], n)).astype(np.uint8)
    return X, mask, tri


# ---- hand cases ----
TRIANGLE = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.3, 0.3, 0.5], [0.3, 0.3, -0.5], [2.0, 2.0, 0.25]])


def test_the_bound_is_strict(ctx):
    tri = np.array([[0, 1, 2], [0, 2, 1]], np.int32)
    P, inl, st = check_tri(ctx, TRIANGLE, None, tri, 0.5)
    assert np.array_equal(P[:, :3], [[0.0, 0.0, 1.0], [0.0, 0.0, -1.0]])       # the normal's orientation is the triple's
    assert inl.tolist() == [4, 4] and st["best"] == 0 and st["best_inliers"] == 4           # the rows at exactly 0.5 are out
    P, inl, st = check_tri(ctx, TRIANGLE, None, tri, np.nextafter(0.5, 1.0))
    assert inl.tolist() == [6, 6]
    out, cnt, keep, st = check_refit(ctx, TRIANGLE, None, P[:1], 0.5, 1, want_keep=True)
    assert cnt[0] >= 4 and keep[:3].all()


def test_void_hypotheses(ctx):
    X = np.array([[0.0, 0, 0], [1.0, 1, 1], [2.0, 2, 2], [0.0, 1, 0], [0.0, 0, 0], [1.0, 0, 0], [3.0, 1, 0.5]])
    n = len(X)
    tri = np.array([[0, 1, 2],                 # collinear
                    [0, 4, 3],                 # coincident points under different indices
                    [0, n, 1], [0, 1, -1], [2**31 - 1, 0, 1], [-2**31, 0, 1],      # out of range
                    [3, 3, 5], [3, 5, 3], [5, 3, 3],                                # repeated
                    [0, 5, 3]], np.int32)      # the one valid triangle
    P, inl, st = check_tri(ctx, X, None, tri, 0.1)
    assert inl[:9].tolist() == [-1] * 9 and inl[9] >= 3 and st["n_void"] == 9 and st["best"] == 9
    assert P[:9].tobytes() == np.zeros((9, 4)).tobytes()
    # a masked-out vertex: the valid triangle is void now, and so is every other
    mask = np.ones(n, np.uint8)
    mask[5] = 0
    P, inl, st = check_tri(ctx, X, mask, tri, 0.1)
    assert st == dict(n_points=n, n_candidates=n - 1, n_hypotheses=10, n_void=10, best=-1, best_inliers=-1)
    # a masked-out row does not count
    mask = np.ones(n, np.uint8)
    mask[4] = 0
    assert check_tri(ctx, X, mask, tri, 0.1)[1][9] == check_tri(ctx, X, None, tri, 0.1)[1][9] - 1


def test_non_finite_coordinates(ctx):
    X = plane_ref.plane_scene(3, 40, 20)[0]
    X[7] = [np.nan, 0.0, 0.0]
    X[8] = [0.0, np.inf, 0.0]
    X[9, 2] = -np.inf
    tri = np.array([[7, 1, 2], [1, 8, 2], [1, 2, 9], [1, 2, 3], [10, 11, 12]], np.int32)
    P, inl, st = check_tri(ctx, X, None, tri, MD)
    assert inl[:3].tolist() == [-1, -1, -1] and (inl[3:] >= 3).all()            # in a vertex: void; in a scored row: it fails the test
    ok = np.isfinite(X).all(axis=1)
    assert np.array_equal(check_tri(ctx, X, ok, tri, MD)[1][3:], inl[3:])
    check_refit(ctx, X, None, np.vstack([P[3:], [[0, 0, np.nan, 1.0]], [[np.inf, 0, 0, 1.0]]]), MD, 3)


def test_all_masked_out(ctx):
    X, _, tri = seeded(4, 200, 64, False)
    none = np.zeros(200, np.uint8)
    P, inl, st = check_tri(ctx, X, none, tri, MD)
    assert st == dict(n_points=200, n_candidates=0, n_hypotheses=64, n_void=64, best=-1, best_inliers=-1)
    assert (inl == -1).all() and P.tobytes() == np.zeros((64, 4)).tobytes()
    out, cnt, keep, st = check_refit(ctx, X, none, [[0.0, 0.0, 1.0, 0.0]], MD, 3, want_keep=True)
    assert cnt.tolist() == [0] and not keep.any() and st["n_improved"] == 0
    out, cnt, keep, st = check_refit(ctx, X, None, [[0.0, np.nan, 1.0, 0.0]], MD, 3, want_keep=True)       # a void plane: keep is all 0
    assert cnt.tolist() == [-1] and not keep.any() and st["n_void"] == 1 and st["best"] == -1 and out.tobytes() == np.zeros(4).tobytes()


def test_three_points_and_a_far_origin(ctx):
    X = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0]])
    P, inl, st = check_tri(ctx, X, None, [[0, 1, 2]], 1e-9)
    assert inl.tolist() == [3]
    check_refit(ctx, X, None, P, 1e-9, 2, want_keep=True)
    Y, mask, tri = seeded(5, 500, 64, True)
    Y = Y + 1e6
    check_tri(ctx, Y, mask, tri, MD)
    valid, P = plane_ref.planes(Y, mask, tri)
    check_refit(ctx, Y, mask, P[valid][:3], MD, 4)


# ---- seams ----
@pytest.mark.parametrize("span", [128, 1024])
@pytest.mark.parametrize("n", [63, 64, 65, 1023, 1024, 1025, "2s-1", "2s+1"])
def test_row_seams(spans, span, n):
    n = {"2s-1": 2 * span - 1, "2s+1": 2 * span + 1}.get(n, n)
    X, mask, tri = seeded(1000 + n, n, 70, n % 2 == 1)
    P, inl, st = check_tri(spans[span], X, mask, tri, MD)
    assert st["n_void"] >= 3 and st["best_inliers"] > n // 4
    check_refit(spans[span], X, mask, P[[st["best"], 0]], MD, 3)
    check_refit(spans[span], X, mask, P[st["best"]], MD, 3, want_keep=True)


@pytest.mark.parametrize("h", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_hypothesis_seams(ctx, spans, h):
    X, mask, tri = seeded(2000 + h, 300, h, h % 2 == 0)
    a = check_tri(ctx, X, mask, tri, MD)
    b = check_tri(spans[128], X, mask, tri, MD)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]      # another grid, the same bytes


@pytest.fixture(scope="module")
def fifteen_hundred():
    X, mask, tri = seeded(77, 1500, 80, True)
    valid, P = plane_ref.planes(X, mask, tri)
    P = P[valid]
    P = np.vstack([P[:62], [[np.nan, 0, 0, 0]], P[62:64], [[0.0, 0.0, 1.0, 500.0]]])     # 63 planes, a void one, two more, a far one: 67
    return X, mask, np.ascontiguousarray(P)


@pytest.mark.parametrize("rounds", [1, plane_ref.MAX_ROUNDS])
@pytest.mark.parametrize("b", [1, 2, 65])
def test_refit_seams(ctx, fifteen_hundred, b, rounds):
    X, mask, P = fifteen_hundred
    out, cnt, keep, st = check_refit(ctx, X, mask, P[:b] if b < 65 else P[2:67], MD, rounds, want_keep=b == 1)
    if b == 65:
        assert st["n_void"] == 1 and st["n_improved"] > 0 and cnt[-1] == 0        # the far plane has no inlier: it stays as it is


def test_a_worse_first_round_leaves_the_input(ctx):
    X, P = plane_ref.tilting_scene()
    want = plane_ref.refit(X, None, P, 0.1, 5)
    first = plane_ref.fit_masked(X, plane_ref.inlier_mask(P[0], X, np.ones(len(X), bool), 0.1), P[0])
    assert int(plane_ref.inlier_mask(first, X, np.ones(len(X), bool), 0.1).sum()) < want[1][0] == 420 and want[3]["n_improved"] == 0
    out, cnt, keep, st = check_refit(ctx, X, None, P, 0.1, 5, want_keep=True)
    assert out.tobytes() == P.tobytes() and cnt.tolist() == [420]


def test_a_refit_that_repeats_itself_ends(ctx):
    g = np.arange(12.0)
    X = np.array([[x, y, 2.0] for x in g for y in g] + [[3.0, 4.0, 7.0], [5.0, 1.0, -6.0]])
    P = np.array([[0.0, 0.0, 1.0, -2.25]])
    runs = []
    want = plane_ref.refit(X, None, P, 0.5, plane_ref.MAX_ROUNDS, rounds_run=runs)
    assert runs == [2] and want[1].tolist() == [144]                            # round 1 moves the plane onto the lattice, round 2 repeats it bit for bit
    for rounds in (1, 2, plane_ref.MAX_ROUNDS):
        check_refit(ctx, X, None, P, 0.5, rounds, want_keep=True)


def test_fewer_than_three_inliers(ctx):
    X = plane_ref.plane_scene(9, 300, 200)[0]
    far = np.array([[0.0, 0.0, 1.0, 1e3]])
    assert check_refit(ctx, X, None, far, MD, 3, want_keep=True)[1].tolist() == [0]
    two = np.zeros(len(X), bool)
    two[[5, 17]] = True
    valid, P = plane_ref.planes(X, None, [[5, 17, 30]])
    out, cnt, keep, st = check_refit(ctx, X, two, P, MD, 3, want_keep=True)
    assert cnt.tolist() == [2] and out.tobytes() == P.tobytes() and np.flatnonzero(keep).tolist() == [5, 17]


# ---- roads ----
def test_host_device_and_mixed_pointers(ctx, fifteen_hundred):
    import torch
    from simpleicp_amd import _lib
    X, mask, P = fifteen_hundred
    tri = seeded(77, 1500, 80, True)[2]
    m8 = _u8(mask)
    dev = torch.device("cuda", 0)
    want_t, want_r = tri_call(ctx, X, mask, tri, MD), refit_call(ctx, X, mask, P[:1], MD, 3, want_keep=True)
    dX, dm, dtri, dP = (torch.from_numpy(a).to(dev) for a in (X, m8, tri, np.ascontiguousarray(P[:1])))
    h = len(tri)
    for on in ((True, True, True, True), (True, False, False, True), (False, True, True, False)):      # X+mask, triples / planes_in, outputs...
        planes = torch.full((h, 4), PLANE_FILL, dtype=torch.float64, device=dev) if on[2] else np.full((h, 4), PLANE_FILL)
        inl = torch.full((h,), INL_FILL, dtype=torch.int32, device=dev) if on[3] else np.full(h, INL_FILL, np.int32)
        torch.cuda.synchronize()
        st = _lib.PlaneStats()
        ctx._chk(ctx._L.sicp_plane_triplets(ctx._h, _lib._ptr(dX if on[0] else X), 1500, _lib._ptr(dm if on[0] else m8),
                                            _lib._ptr(dtri if on[1] else tri), h, MD, _lib._ptr(planes), _lib._ptr(inl), C_.byref(st)))
        got = [a.cpu().numpy() if isinstance(a, torch.Tensor) else a for a in (planes, inl)]
        assert got[0].tobytes() == want_t[0].tobytes() and got[1].tobytes() == want_t[1].tobytes() and st.as_dict() == want_t[2]
        out = torch.full((1, 4), PLANE_FILL, dtype=torch.float64, device=dev) if on[2] else np.full((1, 4), PLANE_FILL)
        cnt = torch.full((1,), INL_FILL, dtype=torch.int32, device=dev) if on[3] else np.full(1, INL_FILL, np.int32)
        keep = torch.full((1500,), KEEP_FILL, dtype=torch.uint8, device=dev) if on[0] else np.full(1500, KEEP_FILL, np.uint8)
        torch.cuda.synchronize()
        st = _lib.PlaneRefitStats()
        ctx._chk(ctx._L.sicp_plane_refit(ctx._h, _lib._ptr(dX if on[0] else X), 1500, _lib._ptr(dm if on[0] else m8),
                                         _lib._ptr(dP if on[1] else P[:1]), 1, MD, 3, _lib._ptr(out), _lib._ptr(cnt), _lib._ptr(keep),
                                         C_.byref(st)))
        got = [a.cpu().numpy() if isinstance(a, torch.Tensor) else a for a in (out, cnt, keep)]
        assert got[0].tobytes() == want_r[0].tobytes() and got[1].tobytes() == want_r[1].tobytes()
        assert np.array_equal(got[2].astype(bool), want_r[2]) and st.as_dict() == want_r[3]
    # planes_out NULL and keep_out NULL; the binding's host forms
    none = tri_call(ctx, X, mask, tri, MD, want_planes=False)
    assert none[0] is None and none[1].tobytes() == want_t[1].tobytes() and none[2] == want_t[2]
    bare = refit_call(ctx, X, mask, P[:1], MD, 3)
    assert bare[2] is None and bare[0].tobytes() == want_r[0].tobytes() and bare[3] == want_r[3]
    planes, inl, st = ctx.plane_triplets(X, tri, MD, mask=mask)
    assert planes.tobytes() == want_t[0].tobytes() and inl.tobytes() == want_t[1].tobytes() and st.as_dict() == want_t[2]
    out, cnt, keep, st = ctx.plane_refit(X, P[:1], MD, 3, mask=mask, want_keep=True)
    assert out.tobytes() == want_r[0].tobytes() and np.array_equal(keep, want_r[2]) and st.as_dict() == want_r[3]
    check_tri(ctx, X, mask, tri, MD)                                          # ... and all of that is the reference


def test_refusals_name_the_argument_and_leave_the_outputs(ctx):
    from simpleicp_amd import _lib
    X, mask, tri = seeded(11, 100, 8, True)
    L = ctx._L
    planes, inl, keep = np.full((8, 4), PLANE_FILL), np.full(8, INL_FILL, np.int32), np.full(100, KEEP_FILL, np.uint8)
    st, st2 = _lib.PlaneStats(), _lib.PlaneRefitStats()
    xp, mp, tp, pp, ip, kp = (_lib._ptr(a) for a in (X, mask, tri, planes, inl, keep))
    P = np.array([[0.0, 0.0, 1.0, 0.0]] * 8)
    qp = _lib._ptr(P)

    def untouched():
        assert np.all(planes == PLANE_FILL) and np.all(inl == INL_FILL) and np.all(keep == KEEP_FILL)

    def tri_refused(word, c=ctx, x=xp, n=100, t=tp, h=8, md=MD, i=ip, o=C_.byref(st)):
        assert L.sicp_plane_triplets(c and c._h, x, n, mp, t, h, md, pp, i, o) == _lib.ERR_INVALID
        assert word.encode() in L.sicp_last_error(), L.sicp_last_error()
        untouched()

    def refit_refused(word, c=ctx, x=xp, n=100, q=qp, b=8, md=MD, rounds=3, p=pp, i=ip, k=None, o=C_.byref(st2)):
        assert L.sicp_plane_refit(c and c._h, x, n, mp, q, b, md, rounds, p, i, k, o) == _lib.ERR_INVALID
        assert word.encode() in L.sicp_last_error(), L.sicp_last_error()
        untouched()

    for refused in (tri_refused, refit_refused):
        refused("null ctx", c=None)
        refused("X is null", x=None)
        refused("inliers_out is null", i=None)
        refused("out is null", o=None)
        for bad in (2, 0, -5, 2**31):
            refused("n must be", n=bad)
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            refused("max_distance", md=bad)
    tri_refused("triples is null", t=None)
    for bad in (0, -3, 2**31):
        tri_refused("h must be", h=bad)
        refit_refused("b must be", b=bad)
    refit_refused("planes_in is null", q=None)
    refit_refused("planes_out is null", p=None)
    for bad in (0, -1, plane_ref.MAX_ROUNDS + 1):
        refit_refused("rounds", rounds=bad)
    refit_refused("keep_out", k=kp)                                           # b == 8
    ctx.set_exchange(lambda *a: 0, 0, 1)
    try:
        tri_refused("not supported with an exchange")
        refit_refused("not supported with an exchange")
    finally:
        ctx.set_exchange(None, 0, 1)
    with pytest.raises(_lib.BackendError, match="max_distance"):
        ctx.plane_triplets(X, tri, -1.0)
    check_tri(ctx, X, mask, tri, MD)                                          # and the context still works


# ---- the Python calls ----
@pytest.fixture(scope="module")
def two_planes():
    return plane_ref.two_plane_scene()


def same(res, want):
    plane, keep, count = want
    got = res.inliers.cpu().numpy() if hasattr(res.inliers, "cpu") else res.inliers
    assert res.plane.tobytes() == plane.tobytes() and np.array_equal(got, keep) and res.n_inliers == count == int(keep.sum())


def test_segment_plane_on_tensors_and_arrays(two_planes):
    import torch
    import simpleicp_amd
    X32 = two_planes.astype(np.float32)
    wide = X32.astype(np.float64)
    want = plane_ref.segment_plane(wide, MD, hypotheses=256, seed=3)
    assert want[2] > 600
    host = simpleicp_amd.segment_plane(X32, MD, hypotheses=256, seed=3, return_info=True)
    same(host, want)
    assert isinstance(host.inliers, np.ndarray) and host.info["hypotheses"]["n_hypotheses"] == 256 and host.info["refit"]["n_planes"] == 1
    t32 = torch.from_numpy(X32).to("cuda:0")
    dev = simpleicp_amd.segment_plane(t32, MD, hypotheses=256, seed=3)
    assert dev.inliers.is_cuda and dev.inliers.dtype == torch.bool and dev.info is None
    same(dev, want)
    strided = torch.zeros((len(X32), 7), dtype=torch.float32, device="cuda:0")
    strided[:, 1:6:2] = t32
    view = strided[:, 1:6:2]
    assert not view.is_contiguous()
    same(simpleicp_amd.segment_plane(view, MD, hypotheses=256, seed=3), want)
    mask = np.random.default_rng(5).random(len(X32)) < 0.7
    want = plane_ref.segment_plane(wide, MD, hypotheses=256, seed=[3, 1], mask=mask)
    same(simpleicp_amd.segment_plane(wide, MD, hypotheses=256, seed=[3, 1], mask=mask), want)
    got = simpleicp_amd.segment_plane(t32, MD, hypotheses=256, seed=[3, 1], mask=torch.from_numpy(mask).to("cuda:0"))
    same(got, want)
    assert not (got.inliers.cpu().numpy() & ~mask).any()


def test_segment_planes_peels_the_two_planes(two_planes):
    import torch
    import simpleicp_amd
    labels, planes = plane_ref.segment_planes(two_planes, MD, 4, 150, hypotheses=256, seed=9)
    assert len(planes) == 2 and set(np.unique(labels)) == {-1, 0, 1} and (labels == 0).sum() > (labels == 1).sum() >= 150
    got = simpleicp_amd.segment_planes(two_planes, MD, min_inliers=150, hypotheses=256, seed=9)
    assert got[0].dtype == np.int32 and np.array_equal(got[0], labels) and got[1].tobytes() == planes.tobytes()
    dev = simpleicp_amd.segment_planes(torch.from_numpy(two_planes).to("cuda:0"), MD, min_inliers=150, hypotheses=256, seed=9)
    assert dev[0].is_cuda and dev[0].dtype == torch.int32 and np.array_equal(dev[0].cpu().numpy(), labels)
    assert dev[1].tobytes() == planes.tobytes()
