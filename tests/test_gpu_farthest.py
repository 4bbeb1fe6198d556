"""Farthest point sampling on the GPU (contract (S)) against tests/farthest_ref.py: idx_out, d2_out and every
field of the record for equality, on both paths -- the single workgroup (SICP_FARTHEST_ONE_MAX at its default) and the stepped
one (0) -- wherever n allows.  Every call goes to the C entry with outputs prefilled with a pattern, and the inputs are compared
with their bytes from before."""
import ctypes as C_
import os
from contextlib import contextmanager

import numpy as np
import pytest

import farthest_ref

pytestmark = pytest.mark.gpu

IDX_FILL, D2_FILL = -777, -123.25
LIMIT = 12288                                                                 # SICP_FARTHEST_ONE_LIMIT
PATHS = ("one", "stepped")


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
def paths():
    """the two paths: a default context (n <= 12 288 in one workgroup) and one that always steps"""
    with context_with() as a, context_with(SICP_FARTHEST_ONE_MAX=0) as b:
        yield {"one": a, "stepped": b}


@pytest.fixture(scope="module")
def spans():
    """stepping contexts whose workgroups take 128 and 1 024 rows: many workgroups at small n"""
    with context_with(SICP_FARTHEST_ONE_MAX=0, SICP_FARTHEST_SPAN=128) as a, context_with(SICP_FARTHEST_ONE_MAX=0, SICP_FARTHEST_SPAN=1024) as b:
        yield {128: a, 1024: b}


def _u8(mask):
    return None if mask is None else np.ascontiguousarray(mask).astype(np.uint8)


def call(ctx, X, mask, m, start=-1, want_d2=True):
    """sicp_farthest: (idx, d2 or None, record as a dict)"""
    from simpleicp_amd import _lib
    X, m8 = np.ascontiguousarray(X, dtype=np.float64), _u8(mask)
    before = (X.tobytes(), None if m8 is None else m8.tobytes())
    idx = np.full(m, IDX_FILL, np.int64)
    d2 = np.full(m, D2_FILL) if want_d2 else None
    st = _lib.FarthestStats()
    ctx._chk(ctx._L.sicp_farthest(ctx._h, _lib._ptr(X), _lib._ptr(m8), len(X), int(m), int(start), _lib._ptr(idx), _lib._ptr(d2), C_.byref(st)))
    assert (X.tobytes(), None if m8 is None else m8.tobytes()) == before
    return idx, d2, st.as_dict()


_WANT = {}


def reference(X, mask, m, start=-1):
    """tests/farthest_ref.py, computed once per input and shared by the paths"""
    X, m8 = np.ascontiguousarray(X, dtype=np.float64), _u8(mask)
    key = (X.tobytes(), None if m8 is None else m8.tobytes(), int(m), int(start))
    if key not in _WANT:
        _WANT[key] = farthest_ref.farthest(X, m8, m, start)
    return _WANT[key]


def check(ctx, X, mask, m, start=-1):
    want = reference(X, mask, m, start)
    got = call(ctx, X, mask, m, start)
    assert np.array_equal(got[0], want[0]) and got[0].dtype == want[0].dtype
    assert got[1].tobytes() == want[1].tobytes()                              # (bytes: +0.0 is not -0.0, +inf is itself)
    assert tuple(got[2]) == farthest_ref.KEYS and got[2] == want[2]
    assert np.float64(got[2]["cover_d2"]).tobytes() == np.float64(want[2]["cover_d2"]).tobytes()
    return got


def counts(n):
    return sorted({m for m in (1, 2, 3, 64, 65, n) if m <= n})


# ---- sizes and counts ----
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1023, 1024, 1025])
def test_sizes_and_counts(paths, path, n):
    X = farthest_ref.cloud(n, n)
    for m in counts(n):                                                       # odd and even: the partials alternate between two buffers
        idx, d2, rec = check(paths[path], X, None, m)
        assert rec["n_selected"] == m and idx[0] == 0 and d2[0] == np.inf


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("n", [LIMIT - 1, LIMIT, LIMIT + 1])
def test_at_the_single_workgroup_limit(paths, path, n):
    """n = 12 289 steps on both contexts: the default context takes the single workgroup up to 12 288 rows and not one beyond"""
    X = farthest_ref.cloud(n, n)
    mask = np.random.default_rng(n).random(n) < 0.9
    mask[-3:] = True
    for m, start in ((64, -1), (65, n - 1)):
        idx, d2, rec = check(paths[path], X, mask, m, start)
        assert rec["n_selected"] == m and idx.max() < n


@pytest.mark.parametrize("n", [2047, 2048, 2049, 4095, 4097, 8191, 8192, 8193])
def test_every_row_count_of_a_lane(paths, n):
    """the single workgroup's kernels of 2, 4, 8 and 12 rows a lane at their seams (1 row: test_sizes_and_counts; the last
    rows of 12: test_at_the_single_workgroup_limit)"""
    X = farthest_ref.cloud(n, n)
    check(paths["one"], X, None, 65, n - 1)


@pytest.mark.parametrize("span,n", [(128, 255), (128, 256), (128, 257), (1024, 2047), (1024, 2048), (1024, 2049)])
def test_two_spans_give_or_take_a_row(spans, span, n):
    X = farthest_ref.cloud(span + n, n)
    mask = np.random.default_rng(n).random(n) < 0.8
    mask[[0, span - 1, span, n - 1]] = True
    for m in (64, 65):
        check(spans[span], X, None, m, n - 1)
        check(spans[span], X, mask, m)


def test_more_spans_than_workgroups(spans, paths):
    """1 027 spans of 128 rows on 1 024 workgroups: the first three workgroups take a second span, the last of them a short one"""
    n = 128 * 1026 + 5
    X = farthest_ref.cloud(7, n)
    X[n - 2] = [40.0, 40.0, 40.0]                                             # the farthest row lies in the strided, short span
    idx, d2, rec = check(spans[128], X, None, 4)
    assert n - 2 in idx[:2]
    assert call(paths["stepped"], X, None, 4)[0].tolist() == idx.tolist()    # ... and on the grid the call chooses itself


def test_the_span_the_call_chooses_beyond_its_least(paths):
    """300 001 rows: the call's own rule gives spans of 320 rows (above its least of 256) on 938 workgroups, the last one short"""
    n = 300001
    X = farthest_ref.cloud(8, n)
    X[n - 1] = [-40.0, 40.0, -40.0]
    idx, d2, rec = check(paths["stepped"], X, None, 4)
    assert idx[1] == n - 1


# ---- values ----
@pytest.mark.parametrize("path", PATHS)
def test_lattice_ties(paths, path):
    X = farthest_ref.lattice(5)                                               # 125 rows: ties at almost every pick
    idx, d2, rec = check(paths[path], X, None, 125)
    assert idx[:2].tolist() == [0, 124] and sorted(idx) == list(range(125)) and rec["cover_d2"] == 0.0
    check(paths[path], farthest_ref.lattice(11), None, 64, 665)              # 1 331 rows, from the centre: 6-, 8- and 12-fold ties


@pytest.mark.parametrize("path", PATHS)
def test_duplicates_end_the_selection(paths, path):
    X = farthest_ref.repeated(7, 5)
    idx, d2, rec = check(paths[path], X, None, 35)
    assert rec["n_selected"] == 7 and rec["cover_d2"] == 0.0 and (idx[7:] == -1).all() and d2[7:].tobytes() == np.zeros(28).tobytes()
    check(paths[path], X, None, 7)
    check(paths[path], X, None, 8)
    check(paths[path], farthest_ref.repeated(300, 4), None, 1200)            # ends at 300 of 1 200 picks: 900 launches find it ended
    same = np.tile([[1.5, -2.0, 3.0]], (100, 1))                              # all rows equal: one pick
    idx, d2, rec = check(paths[path], same, None, 10, 37)
    assert rec["n_selected"] == 1 and idx[0] == 37 and (idx[1:] == -1).all()


@pytest.mark.parametrize("path", PATHS)
def test_offset_and_overflowing_coordinates(paths, path):
    X = farthest_ref.cloud(3, 1500) + 1e6                                      # differences of large numbers: the fused form shows
    check(paths[path], X, None, 64)
    far = np.array([[0.0, 0, 0], [1e200, 0, 0], [0, 1e200, 0], [1.0, 0, 0], [0, 0, -1e200], [1e200, 0, 0]])
    idx, d2, rec = check(paths[path], far, None, 3)                           # d2 = +inf ties: the lowest row
    assert idx.tolist() == [0, 1, 2] and rec["cover_d2"] == np.inf
    idx, d2, rec = check(paths[path], far, None, 6)
    assert rec["n_selected"] == 5 and idx[5] == -1                            # row 5 repeats row 1


@pytest.mark.parametrize("path", PATHS)
def test_rows_that_are_no_candidates(paths, path):
    n = 700
    X = farthest_ref.cloud(9, n)
    X[[0, 5, 64, 699]] = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan]]
    mask = np.where(np.random.default_rng(9).random(n) < 0.3, 0, np.random.default_rng(10).choice([1, 7, 255], n)).astype(np.uint8)
    mask[[0, 5, 1, 698]] = [1, 1, 0, 1]
    idx, d2, rec = check(paths[path], X, None, n)                             # NaN and inf rows, no mask
    assert rec["n_candidates"] == rec["n_selected"] == n - 4 and idx[0] == 1
    idx, d2, rec = check(paths[path], X, mask, n)                             # ... and a mask
    assert rec["n_selected"] == rec["n_candidates"] < n - 4 and (mask[idx[:rec["n_selected"]]] != 0).all()
    check(paths[path], X, mask, 65, 698)                                      # start = the last candidate
    good = farthest_ref.cloud(11, n)
    check(paths[path], good, None, 64, n - 1)                                 # start = n - 1
    for start in (1, 0, 699):                                                 # start masked out, start a NaN row (twice)
        idx, d2, rec = check(paths[path], X, mask, 9, start)
        assert rec["n_selected"] == 0 and (idx == -1).all() and d2.tobytes() == np.zeros(9).tobytes() and rec["cover_d2"] == 0.0
    idx, d2, rec = check(paths[path], X, np.zeros(n, np.uint8), 9)            # an all-masked cloud
    assert rec == dict(n_points=n, n_candidates=0, n_selected=0, cover_d2=0.0)
    idx, d2, rec = check(paths[path], np.full((70, 3), np.nan), None, 3)      # ... and one without a finite row
    assert rec["n_candidates"] == 0 and (idx == -1).all()


# ---- both paths, the prefix ----
def test_paths_agree_and_a_prefix_is_the_run(paths, spans):
    X = farthest_ref.cloud(12, 3000)
    mask = np.random.default_rng(12).random(3000) < 0.6
    runs = [call(c, X, mask, 256, 2999 if mask[2999] else -1) for c in (paths["one"], paths["stepped"], spans[128], spans[1024])]
    for r in runs[1:]:
        assert r[0].tobytes() == runs[0][0].tobytes() and r[1].tobytes() == runs[0][1].tobytes() and r[2] == runs[0][2]
    idx, d2, rec = runs[0]
    assert (d2[2:] <= d2[1:-1]).all() and rec["n_selected"] == 256            # D_t never increases, exactly
    for c in (paths["one"], paths["stepped"]):
        for k in (1, 2, 65, 255):
            a, b, r = call(c, X, mask, k, int(idx[0]))
            assert a.tobytes() == idx[:k].tobytes() and b.tobytes() == d2[:k].tobytes() and r["cover_d2"] == d2[k]
    assert np.array_equal(idx, reference(X, mask, 256, int(idx[0]))[0])


# ---- pointers ----
@pytest.mark.parametrize("path", PATHS)
def test_host_device_and_mixed_pointers(paths, path):
    import torch
    from simpleicp_amd import _lib
    ctx = paths[path]
    n, m = 1500, 65
    X = farthest_ref.cloud(13, n)
    mask = (np.random.default_rng(13).random(n) < 0.7).astype(np.uint8)
    want = reference(X, mask, m)
    dev = torch.device("cuda", 0)
    dX, dm = torch.from_numpy(X).to(dev), torch.from_numpy(mask).to(dev)
    # (X, mask, idx_out, d2_out) on the device?  d2_out None: NULL
    for on in ((1, 1, 1, 1), (1, 0, 0, 1), (0, 1, 1, 0), (1, 0, 1, None), (0, 0, 0, None), (1, None, 1, 1)):
        idx = torch.full((m,), IDX_FILL, dtype=torch.int64, device=dev) if on[2] else np.full(m, IDX_FILL, np.int64)
        d2 = None if on[3] is None else torch.full((m,), D2_FILL, dtype=torch.float64, device=dev) if on[3] else np.full(m, D2_FILL)
        mk = None if on[1] is None else dm if on[1] else mask
        torch.cuda.synchronize()
        st = _lib.FarthestStats()
        ctx._chk(ctx._L.sicp_farthest(ctx._h, _lib._ptr(dX if on[0] else X), _lib._ptr(mk), n, m, -1, _lib._ptr(idx), _lib._ptr(d2), C_.byref(st)))
        w = want if mk is not None else reference(X, None, m)
        got = [a.cpu().numpy() if isinstance(a, torch.Tensor) else a for a in (idx, d2)]
        assert np.array_equal(got[0], w[0]) and st.as_dict() == w[2]
        assert got[1] is None or got[1].tobytes() == w[1].tobytes()
    assert dX.cpu().numpy().tobytes() == X.tobytes() and dm.cpu().numpy().tobytes() == mask.tobytes()
    idx, d2, st = ctx.farthest(X, m, mask=mask)                               # the binding's host form
    assert np.array_equal(idx, want[0]) and d2.tobytes() == want[1].tobytes() and st.as_dict() == want[2]
    assert ctx.farthest(X, m, mask=mask, want_d2=False)[1] is None


# ---- refusals ----
@pytest.mark.parametrize("path", PATHS)
def test_refusals_name_the_argument_and_leave_the_outputs(paths, path):
    from simpleicp_amd import _lib
    ctx = paths[path]
    L = ctx._L
    X = farthest_ref.cloud(14, 100)
    mask = np.ones(100, np.uint8)
    idx, d2 = np.full(8, IDX_FILL, np.int64), np.full(8, D2_FILL)
    st = _lib.FarthestStats()
    xp, mp, ip, dp = (_lib._ptr(a) for a in (X, mask, idx, d2))

    def refused(word, c=ctx, x=xp, n=100, m=8, start=-1, i=ip, o=C_.byref(st)):
        assert L.sicp_farthest(c and c._h, x, mp, n, m, start, i, dp, o) == _lib.ERR_INVALID
        assert word.encode() in L.sicp_last_error(), L.sicp_last_error()
        assert np.all(idx == IDX_FILL) and np.all(d2 == D2_FILL)

    refused("null ctx", c=None)
    refused("X is null", x=None)
    refused("idx_out is null", i=None)
    refused("out is null", o=None)
    for bad in (0, -5):
        refused("n must be >= 1", n=bad)
    refused("n must be < 2^31", n=2**31, x=C_.c_void_p(8))                    # (a pointer that is never read)
    refused("n must be < 2^31", n=2**40, x=C_.c_void_p(8))
    for bad in (0, -1, 101, 2**31):
        refused("m must be", m=bad)
    for bad in (-2, 100, 2**31, -2**40):
        refused("start must be", start=bad)
    ctx.set_exchange(lambda *a: 0, 0, 1)
    try:
        refused("not supported with an exchange")
    finally:
        ctx.set_exchange(None, 0, 1)
    with pytest.raises(_lib.BackendError, match="m must be"):
        ctx.farthest(X, 101)
    check(ctx, X, mask, 8)                                                    # and the context still works


# ---- the Python calls ----
def test_farthest_points_on_tensors_and_arrays():
    import torch
    import simpleicp_amd
    X32 = farthest_ref.cloud(15, 3000).astype(np.float32)
    wide = X32.astype(np.float64)
    want = reference(wide, None, 100)
    host = simpleicp_amd.farthest_points(X32, 100, return_distances=True, return_info=True)
    assert isinstance(host[0], np.ndarray) and np.array_equal(host[0], want[0]) and host[1].tobytes() == want[1].tobytes() and host[2] == want[2]
    t32 = torch.from_numpy(X32).to("cuda:0")
    dev = simpleicp_amd.farthest_points(t32, 100, return_distances=True)
    assert dev[0].is_cuda and dev[0].dtype == torch.int64 and dev[1].dtype == torch.float64
    assert np.array_equal(dev[0].cpu().numpy(), want[0]) and dev[1].cpu().numpy().tobytes() == want[1].tobytes()
    assert torch.equal(t32[dev[0]], t32[torch.from_numpy(want[0]).to("cuda:0")])                 # X[farthest_points(X, k)] reads as it should
    strided = torch.zeros((len(X32), 7), dtype=torch.float32, device="cuda:0")
    strided[:, 1:6:2] = t32
    view = strided[:, 1:6:2]
    assert not view.is_contiguous()
    assert np.array_equal(simpleicp_amd.farthest_points(view, 100).cpu().numpy(), want[0])
    mask = np.random.default_rng(5).random(len(X32)) < 0.7
    want = reference(wide, mask, 64, 2)
    for mk in (torch.from_numpy(mask).to("cuda:0"), torch.from_numpy(mask.astype(np.uint8) * 9).to("cuda:0")):
        got, info = simpleicp_amd.farthest_points(t32, 64, start=2 if mask[2] else None, mask=mk, return_info=True)
        w = want if mask[2] else reference(wide, mask, 64)
        assert np.array_equal(got.cpu().numpy(), w[0]) and info == w[2]
    # not padded: duplicates on the device; more than 12 288 rows step
    R = torch.from_numpy(farthest_ref.repeated(7, 5)).to("cuda:0")
    assert len(simpleicp_amd.farthest_points(R, 35)) == 7
    big = farthest_ref.cloud(16, 13000).astype(np.float32)
    assert np.array_equal(simpleicp_amd.farthest_points(torch.from_numpy(big).to("cuda:0"), 16).cpu().numpy(),
                          reference(big.astype(np.float64), None, 16)[0])


def test_select_farthest_on_the_library():
    from simpleicp_amd import PointCloud
    X = farthest_ref.cloud(17, 2000)
    pc = PointCloud(X, columns=["x", "y", "z"])
    pc.select_by_indices(np.flatnonzero(np.random.default_rng(17).random(2000) < 0.5))
    sel = pc.idx_selected
    mask = np.zeros(2000, bool)
    mask[sel] = True
    want = reference(X, mask, 50, int(sel[3]))
    pc.select_farthest(50, start=int(sel[3]))
    assert np.array_equal(pc.idx_selected, np.sort(want[0])) and np.array_equal(pc.last_farthest[0], want[0])
    assert pc.last_farthest[1].tobytes() == want[1].tobytes() and pc.last_farthest[2] == want[2]
