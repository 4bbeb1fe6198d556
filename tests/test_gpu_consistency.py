"""Match consistency on the GPU (contract (C)): the degrees, the core numbers and the record equal the numpy
reference of tests/consistency_ref.py exactly -- at the word, row-block, column-chunk and one-launch seams, on both paths of the
peeling (SICP_CONSISTENCY, read at sicp_ctx_create), from host and from device memory --, thresholds met exactly, rows that are
not finite, duplicates, closed forms at the cap, a peel longer than one host batch, scratch that grows, the refusals, and the chain
register_global(prune=...) on two disjoint samples of the bundled bunny."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import consistency_ref
import global_ref
import robust_ref
from test_gpu_robust import EXTENT, bunny_pair, bunny_reference, pose_error, u64   # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CAP = 32768
ONE_MAX = 4096                                                        # the one-launch path's bound; also a column chunk of the build
BATCH = 16                                                            # sub-rounds the sweeps path enqueues between two looks


def forced(path):
    """A context of its own whose peeling takes `path` wherever it applies (SICP_CONSISTENCY is read at sicp_ctx_create)."""
    from simpleicp_amd import _lib
    old = os.environ.get("SICP_CONSISTENCY")
    os.environ["SICP_CONSISTENCY"] = path
    try:
        return _lib.Context(0)
    finally:
        if old is None:
            del os.environ["SICP_CONSISTENCY"]
        else:
            os.environ["SICP_CONSISTENCY"] = old


@pytest.fixture(scope="module")
def paths():
    """The context as users get it, and one per forced path."""
    from simpleicp_amd import _lib
    ctxs = {"default": _lib.Context(0), "sweeps": forced("sweeps"), "one": forced("one")}
    yield ctxs
    for c in ctxs.values():
        c.close()


def rotation(axis, angle):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


R_TRUE, T_TRUE = rotation([1.0, 2.0, 3.0], 0.7), np.array([0.3, -0.2, 0.1])


def noisy_copy(rng, m, wrong=0.8, noise=0.002):
    src = rng.uniform(-1, 1, (m, 3))
    dst = src @ R_TRUE.T + T_TRUE + rng.normal(0, noise, (m, 3))
    bad = rng.choice(m, int(wrong * m), replace=False)
    dst[bad] = rng.uniform(-1, 1, (len(bad), 3))
    return src, dst


def on_host(ctx, src, dst, tol, ml):
    degree, core, st = ctx.match_consistency(src, dst, tol, ml)
    return degree, core, st.as_dict()


def on_device(ctx, src, dst, tol, ml):
    m = len(src)
    S, D = torch.tensor(src, device=DEV), torch.tensor(dst, device=DEV)
    degree = torch.full((m,), -7, dtype=torch.int32, device=DEV)
    core = torch.full((m,), -7, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    st = ctx.match_consistency(S.data_ptr(), D.data_ptr(), tol, ml, m=m, degree_ptr=degree.data_ptr(), core_ptr=core.data_ptr())
    assert np.array_equal(u64(S.cpu().numpy()), u64(src)) and np.array_equal(u64(D.cpu().numpy()), u64(dst))
    return degree.cpu().numpy(), core.cpu().numpy(), st.as_dict()


def same(got, want, what=""):
    degree, core, stats = got
    rdegree, rcore, rec = want
    assert degree.dtype == core.dtype == np.int32, what
    assert np.array_equal(degree, rdegree), what
    assert np.array_equal(core, rcore), what
    assert stats.pop("n_subrounds") >= 1, what                        # (informative: the one field that may differ between the paths)
    assert stats == rec, what


def check(paths, src, dst, tol, ml, want=None):
    """Every context -- the default and both forced paths -- on both roads against the reference (computed once)."""
    if want is None:
        want = consistency_ref.consistency(src, dst, tol, ml)
    for name, c in paths.items():
        for road in (on_host, on_device):
            same(road(c, src, dst, tol, ml), want, f"path {name}, {road.__name__}, m={len(src)}")
    return want


# ---- equality with the reference at the seams, on both paths and both roads ----
# a word (64), a row block of the build (32), the build's column chunk and the one-launch path's bound (both 4 096)
@pytest.mark.parametrize("m", [3, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, ONE_MAX - 1, ONE_MAX, ONE_MAX + 1])
def test_consistency_equals_the_reference(paths, m):
    rng = np.random.default_rng(1000 + m)
    src, dst = noisy_copy(rng, m, wrong=0.8 if m > 33 else 0.3)
    degree, core, rec = check(paths, src, dst, 0.01, 0.1)
    print(f"m {m}: {rec}")
    assert rec["n_valid"] == m and rec["max_core"] >= 1
    if m == 1025:
        # the Python road: arrays and CUDA tensors, float32 widened exactly; the outputs stay where the inputs are
        import simpleicp_amd
        s32 = src.astype(np.float32)
        want = consistency_ref.consistency(s32.astype(np.float64), dst, 0.01, 0.1)
        res_a = simpleicp_amd.consistent_matches(s32, dst, tolerance=0.01, min_length=0.1)
        res_t = simpleicp_amd.consistent_matches(torch.tensor(s32, device=DEV), torch.tensor(dst, device=DEV), tolerance=0.01, min_length=0.1)
        assert isinstance(res_a.keep, np.ndarray) and res_a.keep.dtype == bool
        for t in (res_t.keep, res_t.core, res_t.degree):
            assert isinstance(t, torch.Tensor) and t.device.type == "cuda"
        assert res_t.keep.dtype == torch.bool and res_t.core.dtype == res_t.degree.dtype == torch.int32
        same((res_a.degree, res_a.core, dict(res_a.stats)), want, "arrays")
        same((res_t.degree.cpu().numpy(), res_t.core.cpu().numpy(), dict(res_t.stats)), want, "tensors")
        keep = consistency_ref.keep_mask(want[1], want[2])
        assert np.array_equal(res_a.keep, keep) and np.array_equal(res_t.keep.cpu().numpy(), keep) and keep.sum() == want[2]["n_max_core"]


def test_thresholds_exactly_met(paths):
    """Integer coordinates whose lengths are exact: rows 0 and 1 are 5 apart in src (3-4-5) and 13 apart in dst (5-12-13), so
    |a - b| is exactly 8; row 2 is far from both."""
    src = np.array([[0.0, 0, 0], [3, 4, 0], [1000, 0, 0]])
    dst = np.array([[0.0, 0, 0], [5, 12, 0], [0, 0, 1]])
    for tol, ml, edge in ((8.0, 0.0, True), (np.nextafter(8.0, 0.0), 0.0, False), (8.0, 5.0, True), (8.0, np.nextafter(5.0, 6.0), False),
                          (np.nextafter(8.0, 9.0), np.nextafter(5.0, 0.0), True)):
        degree, core, rec = check(paths, src, dst, tol, ml)
        assert degree.tolist() == ([1, 1, 0] if edge else [0, 0, 0]) and core.tolist() == degree.tolist(), (tol, ml)
        assert rec["n_edges"] == int(edge) and rec["n_max_core"] == (2 if edge else 0)
    # ... and with the roles of the clouds swapped: min_length holds for both lengths
    degree, _, _ = check(paths, dst, src, 8.0, np.nextafter(5.0, 6.0))
    assert not degree.any()


def test_rows_that_are_not_finite(paths):
    m = 130
    rng = np.random.default_rng(130)
    src, dst = noisy_copy(rng, m, wrong=0.5)
    bad_s, bad_d = src.copy(), dst.copy()
    bad_s[[0, 64], [0, 2]] = [np.nan, -np.inf]
    bad_d[[63, 129], [1, 0]] = [np.inf, np.nan]
    bad = [0, 63, 64, 129]                                            # the first row, a word seam, the last row; either cloud
    degree, core, rec = check(paths, bad_s, bad_d, 0.05, 0.1)
    assert not degree[bad].any() and not core[bad].any() and rec["n_valid"] == m - 4 and rec["max_core"] >= 1
    # their neighbours' counts exclude them: the other rows are those of the clouds without the four
    rest = np.setdiff1d(np.arange(m), bad)
    d2, c2, _ = consistency_ref.consistency(src[rest], dst[rest], 0.05, 0.1)
    assert np.array_equal(degree[rest], d2) and np.array_equal(core[rest], c2)
    # every row invalid
    degree, core, rec = check(paths, np.full((70, 3), np.nan), dst[:70], 0.05, 0.0)
    assert rec == dict(n_rows=70, n_valid=0, n_edges=0, max_degree=0, max_core=0, n_max_core=0)
    # lengths whose squares overflow are not finite: no edge, though the rows are valid
    huge = np.array([[1e200, 0, 0], [-1e200, 0, 0], [0, 1e200, 0], [0.0, 0, 0]])
    degree, _, rec = check(paths, huge, huge, 1.0, 0.0)
    assert rec["n_valid"] == 4 and not degree.any()


def test_duplicates(paths):
    rng = np.random.default_rng(9)
    src = rng.integers(-50, 50, (70, 3)).astype(np.float64)
    src[10] = src[3]
    src[69] = src[64]
    dst = src + np.array([7.0, -2.0, 5.0])                            # exact: every pair of lengths is equal
    degree, core, rec = check(paths, src, dst, 1e-9, 0.0)             # min_length = 0: exact duplicates are compatible
    assert np.all(degree == 69) and np.all(core == 69) and rec["n_edges"] == 70 * 69 // 2
    degree, core, rec = check(paths, src, dst, 1e-9, 0.5)             # any min_length > 0 keeps them apart
    dup = [3, 10, 64, 69]
    assert np.all(degree[dup] == 68) and np.all(np.delete(degree, dup) == 69) and rec["n_edges"] == 70 * 69 // 2 - 2
    assert np.all(core == 68)                                         # (the two missing edges: everybody still has 68 partners inside)


def test_closed_forms_at_the_cap(paths):
    rng = np.random.default_rng(5)
    src = rng.uniform(-1, 1, (CAP, 3))
    for name in ("default", "one"):                                   # (beyond its bound a forced one-launch path is the sweeps path)
        degree, core, st = on_device(paths[name], src, src, 1e-9, 0.0)
        assert np.all(degree == CAP - 1) and np.all(core == CAP - 1)
        assert st == dict(n_rows=CAP, n_valid=CAP, n_edges=CAP * (CAP - 1) // 2, max_degree=CAP - 1, max_core=CAP - 1, n_max_core=CAP,
                          n_subrounds=1)
    # every dst length is twice the src length: off by the length itself, far more than the tolerance
    degree, core, st = on_device(paths["default"], src, 2.0 * src, 1e-9, 0.0)
    assert not degree.any() and not core.any()
    assert st == dict(n_rows=CAP, n_valid=CAP, n_edges=0, max_degree=0, max_core=0, n_max_core=0, n_subrounds=1)


def test_a_peel_longer_than_one_host_batch(paths):
    """A collinear cloud with uneven spacing (multiples of 1/8), stretched by 1 + 1/64 (exact): rows are compatible iff they are
    at most 64 apart, a band whose width in rows grows along the line as the spacing shrinks."""
    m = 300
    gaps = 1.0 + 7.0 * (np.arange(m) % 17) / 17.0 + 30.0 / (1 + np.arange(m) // 20)
    x = np.cumsum(np.round(gaps * 8) / 8)
    src = np.column_stack([x, np.zeros(m), np.zeros(m)])
    dst = src * (1.0 + 1.0 / 64.0)
    A = consistency_ref.adjacency(src, dst, 1.0, 0.0)
    passes = consistency_ref.subrounds(A)
    assert passes > 4 * BATCH
    want = consistency_ref.consistency(src, dst, 1.0, 0.0, A=A)
    assert len(set(want[1].tolist())) >= 8                            # many levels
    check(paths, src, dst, 1.0, 0.0, want)
    assert on_host(paths["sweeps"], src, dst, 1.0, 0.0)[2]["n_subrounds"] > BATCH


def test_scratch_grows_with_the_calls():
    rng = np.random.default_rng(77)
    small, large = noisy_copy(rng, 70), noisy_copy(rng, 1100)
    for path in ("sweeps", "one"):
        fresh, used = forced(path), forced(path)
        try:
            want_large, want_small = on_host(fresh, *large, 0.01, 0.1), on_device(fresh, *small, 0.01, 0.1)
            for rows, want in ((small, want_small), (large, want_large), (small, want_small), (large, want_large)):
                for road in (on_host, on_device):
                    got = road(used, *rows, 0.01, 0.1)
                    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], path
        finally:
            fresh.close()
            used.close()
    same(want_large, consistency_ref.consistency(*large, 0.01, 0.1))


def test_refusals_leave_the_context_usable(paths):
    from simpleicp_amd import _lib
    ctx = paths["default"]
    L, P = _lib.load(), _lib._ptr
    src, dst = noisy_copy(np.random.default_rng(2), 20, wrong=0.0)
    degree, core, st = np.full(20, -7, np.int32), np.full(20, -7, np.int32), _lib.ConsistencyStats()

    def raw(s=src, d=dst, m=20, tol=0.05, ml=0.0, do=degree, co=core, stats=st):
        return L.sicp_match_consistency(ctx._h, P(s), P(d), m, tol, ml, P(do), P(co), None if stats is None else C.byref(stats))

    def refused(rc, word):
        assert rc == _lib.ERR_INVALID and word in L.sicp_last_error().decode(), (rc, L.sicp_last_error())
        assert np.all(degree == -7) and np.all(core == -7)

    refused(raw(s=None), "src")
    refused(raw(d=None), "dst")
    refused(raw(do=None), "degree_out")
    refused(raw(co=None), "core_out")
    refused(raw(stats=None), "out is null")
    refused(raw(m=2), "m ")
    refused(raw(m=CAP + 1), "m ")                                     # (refused before a byte of the arrays is read)
    refused(raw(m=-1), "m ")
    for tol in (0.0, -1.0, float("nan"), float("inf")):
        refused(raw(tol=tol), "tolerance")
    for ml in (-1e-300, float("nan"), float("inf")):
        refused(raw(ml=ml), "min_length")
    ctx.set_exchange(lambda *a: 0, 0, 1)
    try:
        refused(raw(), "not supported with an exchange")
    finally:
        ctx.set_exchange(None, 0, 1)
    assert raw() == _lib.OK
    same((degree, core, st.as_dict()), consistency_ref.consistency(src, dst, 0.05, 0.0))


# ---- the chain on the bundled bunny (the fixtures of test_gpu_robust.py) ----
PRUNE = dict(prune=10_000.0, prune_min_length=20_000.0)


def test_pruned_chain_on_the_bunny(bunny_pair, bunny_reference):
    """Asserted: under both methods the chain is the reference chain's bit for bit -- the reference's pruning, then the existing
    references --, twice, on both roads, and n_consistent is what the reference says.  No ranking against the unpruned chain is
    asserted; the counts and the errors against the truth are printed (DESIGN.md section 21 records them)."""
    import simpleicp_amd
    A, B, vA, vB, R, t = bunny_pair
    src, dst, n_matches = bunny_reference
    degree, core, rec = consistency_ref.consistency(src, dst, PRUNE["prune"], PRUNE["prune_min_length"])
    keep = consistency_ref.keep_mask(core, rec)
    ks, kd = np.ascontiguousarray(src[keep]), np.ascontiguousarray(dst[keep])
    print(f"{n_matches} matches, {int(keep.sum())} in the maximal core ({rec})")
    assert keep.sum() >= 3
    kw = dict(max_distance=10_000.0, viewpoint_fixed=tuple(vA), viewpoint_movable=tuple(vB))
    At, Bt = torch.tensor(A, device=DEV), torch.tensor(B, device=DEV)
    # the robust method
    P, inl, _, rrec = robust_ref.robust(ks, kd, None, 10_000.0, 64, 1.4, 0.0)
    res = simpleicp_amd.register_global(At, Bt, method="robust", **PRUNE, **kw)
    again = simpleicp_amd.register_global(At, Bt, method="robust", **PRUNE, **kw)
    host = simpleicp_amd.register_global(A, B, method="robust", **PRUNE, **kw)
    assert res.n_matches == n_matches and res.n_consistent == int(keep.sum()) and res.stats == rrec and res.inliers == inl[0]
    assert np.array_equal(u64(res.H[:3, :3].ravel()), u64(P[0, :9])) and np.array_equal(u64(res.H[:3, 3]), u64(P[0, 9:]))
    for other in (again, host):
        assert np.array_equal(u64(other.H), u64(res.H)) and (other.inliers, other.n_consistent, other.stats) == (res.inliers, res.n_consistent, res.stats)
    angle, shift = pose_error(res.H, R, t)
    print(f"pruned, robust: {res.inliers} inliers of {res.n_consistent}, rotation error {angle:.2f} deg, translation error "
          f"{shift / EXTENT:.4f} of the extent")
    plain = simpleicp_amd.register_global(A, B, method="robust", **kw)
    assert plain.n_consistent is None and plain.n_matches == n_matches
    angle, shift = pose_error(plain.H, R, t)
    print(f"unpruned, robust: {plain.inliers} inliers of {n_matches}, rotation error {angle:.2f} deg, translation error "
          f"{shift / EXTENT:.4f} of the extent")
    # the random triples: rows of the pruned set
    for seed in (0, 1, 2):
        tri = np.random.default_rng(seed).integers(0, len(ks), (1000, 3), dtype=np.int32)
        poses, rinl, rst = global_ref.ransac(ks, kd, tri, 10_000.0, 0.9)
        rst = rst.as_dict() if hasattr(rst, "as_dict") else dict(rst)
        ran = simpleicp_amd.register_global(At, Bt, hypotheses=1000, seed=seed, **PRUNE, **kw)
        ran2 = simpleicp_amd.register_global(A, B, hypotheses=1000, seed=seed, **PRUNE, **kw)
        best = rst["best"]
        assert ran.stats == rst and ran.n_consistent == int(keep.sum()) and ran.n_matches == n_matches
        assert ran.index == best and ran.inliers == rinl[best]
        assert np.array_equal(u64(ran.H[:3, :3].ravel()), u64(poses[best, :9])) and np.array_equal(u64(ran.H[:3, 3]), u64(poses[best, 9:]))
        assert np.array_equal(u64(ran2.H), u64(ran.H)) and (ran2.index, ran2.inliers, ran2.stats) == (ran.index, ran.inliers, ran.stats)
        angle, shift = pose_error(ran.H, R, t)
        print(f"pruned, triples seed {seed}: {ran.inliers} inliers of {ran.n_consistent}, rotation error {angle:.2f} deg, translation "
              f"error {shift / EXTENT:.4f} of the extent")
