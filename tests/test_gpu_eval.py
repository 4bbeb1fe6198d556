"""Evaluation on the GPU (contract (E)): every field of the record equals the numpy reference of
tests/eval_ref.py bit for bit -- the query counts at which the reduction changes shape, a searched cloud for the brute-force scan
and one for the grid, adversarial inputs --, repeatability and side effects, known answers, the refusals, and the end-to-end
identities of run(), run_tensors, run_batch and evaluate_registration."""
import ctypes as C

import numpy as np
import pytest
import torch

import eval_ref
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
QS = [1, 2, 63, 64, 65, 1023, 1024, 1025, 4097, 70_001]


@pytest.fixture(scope="module")
def ctx():
    from simpleicp_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def sums_of(rec):
    return np.array([rec.sum_d2, *rec.sum_p, *rec.sum_pp], dtype=np.float64)


def same_bits(rec, want):
    assert rec.n_queries == want["n_queries"]
    assert rec.n_inliers == want["n_inliers"]
    got = sums_of(rec)
    assert np.array_equal(got.view(np.uint64), want["sums"].view(np.uint64)), (got, want["sums"])


def check(ctx, Xq, Xs, H=None, d=np.inf, rows=None, nn=None):
    """One call against the reference, the clouds uploaded first.  Returns the reference's record."""
    from simpleicp_amd import _lib
    ctx.upload(_lib.FIX, np.ascontiguousarray(Xq, dtype=np.float64))
    ctx.upload(_lib.MOV, np.ascontiguousarray(Xs, dtype=np.float64))
    want = eval_ref.evaluate(Xq, Xs, H, d, rows=rows, nn=nn)
    same_bits(ctx.evaluate(_lib.FIX, _lib.MOV, H, d, rows), want)
    return want


def rigid(a, b, t):
    ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(b), np.sin(b)
    H = np.eye(4)
    H[:3, :3] = np.array([[ca, -sa, 0], [sa, ca, 0], [0, 0, 1.0]]) @ np.array([[cb, 0, sb], [0, 1.0, 0], [-sb, 0, cb]])
    H[:3, 3] = t
    return H


# ---- the query counts, on both search paths ----
@pytest.fixture(scope="module")
def queries():
    return np.random.default_rng(31).uniform(-5, 5, (QS[-1], 3))


# (5 000 points: the brute-force scan; 70 000 -- more than 65 536 -- the grid)
@pytest.mark.parametrize("n,d,kernel", [(5000, 0.3, "k_knn1_scan"), (70_000, 0.12, "k_grid")])
def test_every_query_count_on_both_search_paths(ctx, queries, n, d, kernel):
    from simpleicp_amd import _lib
    Xs = np.random.default_rng(n).uniform(-5.2, 5.2, (n, 3))
    H = rigid(0.02, -0.03, [0.05, -0.02, 0.01])
    nn = eval_ref.neighbours(queries, Xs, H, d)                      # once, shared by every count
    assert 0.2 < (nn[0] >= 0).mean() < 0.8
    ctx.upload(_lib.MOV, Xs)
    for Q in QS:
        want = eval_ref.evaluate(queries, Xs, H, d, rows=np.arange(Q), nn=nn)
        ctx.upload(_lib.FIX, queries[:Q])                            # sel_idx NULL: the slot's points in their order
        same_bits(ctx.evaluate(_lib.FIX, _lib.MOV, H, d), want)
        assert ctx.last_match_kernel().startswith(kernel)
    # the same prefixes as rows of the whole cloud
    ctx.upload(_lib.FIX, queries)
    for Q in QS:
        same_bits(ctx.evaluate(_lib.FIX, _lib.MOV, H, d, np.arange(Q)), eval_ref.evaluate(queries, Xs, H, d, rows=np.arange(Q), nn=nn))


def test_more_partials_than_one_step_of_the_second_stage(ctx):
    """1024 queries a partial, 1024 partials a step of the one-workgroup second stage: from 2^20 queries on it runs two levels"""
    rng = np.random.default_rng(40)
    Q = 1024 * 1024 + 2049                                            # 1027 partials: an odd count, a last step of three
    Xq = rng.uniform(-4, 4, (Q, 3)) + [100.0, 0.0, -30.0]
    Xs = rng.uniform(-4, 4, (48, 3)) + [100.0, 0.0, -30.0]
    want = check(ctx, Xq, Xs, rigid(0.001, 0.002, [0.01, 0.0, 0.0]), 1.5)
    assert 0.1 * Q < want["n_inliers"] < 0.9 * Q


# ---- adversarial inputs ----
def test_nothing_and_everything_in_range(ctx):
    rng = np.random.default_rng(32)
    Xq, Xs = rng.uniform(-1, 1, (3000, 3)), rng.uniform(-1, 1, (2500, 3))
    far = check(ctx, Xq, Xs + 100.0, d=5.0)
    assert far["n_inliers"] == 0 and not far["sums"].view(np.uint64).any()          # every sum is +0.0
    allin = check(ctx, Xq, Xs, d=np.inf)                              # max_distance = inf
    assert allin["n_inliers"] == 3000
    assert check(ctx, Xq, Xs + 100.0, d=np.inf)["n_inliers"] == 3000
    assert check(ctx, Xq, Xs, d=0.0)["n_inliers"] == 0                # d2 < 0 never holds


def test_the_bound_is_strict(ctx):
    Xs = np.array([[3.0, 4.0, 0.0], [50.0, 50.0, 50.0], [-7.0, 0.0, 0.0]])
    Xq = np.array([[0.0, 0.0, 0.0], [50.0, 50.0, 45.0], [-7.0, 0.0, 0.0], [1.0, 1.0, 1.0]])   # d2 = 25, 25, 0, 14
    out = check(ctx, Xq, Xs, d=5.0)
    assert out["n_inliers"] == 2 and out["sums"][0] == 14.0           # a neighbour exactly at the distance is out
    assert check(ctx, Xq, Xs, d=np.nextafter(5.0, 6.0))["n_inliers"] == 4
    assert check(ctx, Xq, Xs, d=np.nextafter(5.0, 0.0))["n_inliers"] == 2


def test_duplicates_negative_zero_and_single_queries(ctx):
    rng = np.random.default_rng(33)
    Xs = rng.uniform(-2, 2, (4000, 3))
    Xs[1000:1500] = Xs[rng.integers(0, 1000, 500)]
    Xq = rng.uniform(-2, 2, (2600, 3))
    Xq[700:900] = Xq[5]
    Xq[900:1100] = Xs[rng.integers(0, 4000, 200)]                    # queries that ARE cloud points: d2 = 0
    assert check(ctx, Xq, Xs, d=0.2)["n_inliers"] > 200
    # a sum of negative zeros is -0.0 where the contract adds no padding (Q a power of two), +0.0 where it does
    Z = np.array([[-0.0, -0.0, 1.0]])
    for reps in (1, 2, 3, 64, 65, 1024):
        want = check(ctx, np.repeat(Z, reps, axis=0), Xs, d=np.inf)
        assert np.signbit(want["sums"][1]) == (reps in (1, 2, 64, 1024)) and want["sums"][1] == 0.0


def test_offset_coordinates_round_at_every_level(ctx):
    rng = np.random.default_rng(34)
    Xs = rng.uniform(-3, 3, (6000, 3)) + 1e6
    Xq = rng.uniform(-3, 3, (9001, 3)) + 1e6
    want = check(ctx, Xq, Xs, d=0.25)
    assert 0 < want["n_inliers"] < 9001
    # (a data condition: here the plain left-to-right sum differs from the tree, so the order is really tested)
    t = eval_ref.terms(Xq, *eval_ref.neighbours(Xq, Xs, None, 0.25))
    assert np.cumsum(t[:, 4])[-1] != want["sums"][4]


def test_symmetric_cloud_cancels(ctx):
    rng = np.random.default_rng(35)
    half = rng.uniform(-4, 4, (2500, 3))
    Xq = np.empty((5000, 3))
    Xq[0::2], Xq[1::2] = half, -half
    want = check(ctx, Xq, np.concatenate([half[::2], -half[::2]]) * 1.001, d=np.inf)
    assert (want["sums"][1:4] == 0.0).all()                           # adjacent pairs cancel exactly
    perm = rng.permutation(5000)
    check(ctx, Xq[perm], np.concatenate([half[::2], -half[::2]]) * 1.001, d=0.05)


def test_rows_in_any_order_and_in_device_memory(ctx):
    from simpleicp_amd import _lib
    rng = np.random.default_rng(36)
    Xq, Xs = rng.uniform(-3, 3, (20_000, 3)) * [1.0, 30.0, 0.01], rng.uniform(-3, 3, (8000, 3)) * [1.0, 30.0, 0.01]
    H, d = rigid(-0.01, 0.02, [0.0, 0.3, 0.0]), 0.4
    nn = eval_ref.neighbours(Xq, Xs, H, d)
    rows = rng.permutation(20_000)[:7777]
    a = check(ctx, Xq, Xs, H, d, rows=rows, nn=nn)
    b = check(ctx, Xq, Xs, H, d, rows=np.sort(rows), nn=nn)
    assert a["n_inliers"] == b["n_inliers"] and not np.array_equal(a["sums"].view(np.uint64), b["sums"].view(np.uint64))
    check(ctx, Xq, Xs, H, d, rows=np.concatenate([rows[:100], rows[:100]]), nn=nn)        # a row may come twice
    t = torch.tensor(rows, device=DEV)
    same_bits(ctx.evaluate(_lib.FIX, _lib.MOV, H, d, t), a)


# ---- repeatability and side effects ----
def test_repeatable_and_without_side_effects(ctx):
    from simpleicp_amd import _lib
    rng = np.random.default_rng(37)
    Xq, Xs = rng.uniform(-3, 3, (30_000, 3)), rng.uniform(-3, 3, (70_000, 3))
    ctx.upload(_lib.FIX, Xq)
    ctx.upload(_lib.MOV, Xs)
    H = rigid(0.01, 0.01, [0.01, 0.0, 0.0])
    before = ctx.select_in_range(_lib.FIX, _lib.MOV, None, H, 0.08)
    r1 = ctx.evaluate(_lib.FIX, _lib.MOV, H, 0.08)
    r2 = ctx.evaluate(_lib.FIX, _lib.MOV, H, 0.08)
    assert bytes(r1) == bytes(r2) and len(bytes(r1)) == 96
    assert r1.n_inliers == int(before.sum()) and 0 < r1.n_inliers < 30_000
    assert np.array_equal(ctx.select_in_range(_lib.FIX, _lib.MOV, None, H, 0.08), before)
    assert np.array_equal(ctx.download(_lib.FIX), Xq) and np.array_equal(ctx.download(_lib.MOV), Xs)
    # a smaller call after a larger one reuses the scratch
    same_bits(ctx.evaluate(_lib.FIX, _lib.MOV, H, 0.08, np.arange(100)), eval_ref.evaluate(Xq[:100], Xs, H, 0.08))
    assert bytes(ctx.evaluate(_lib.FIX, _lib.MOV, H, 0.08)) == bytes(r1)


# ---- known answers ----
def test_known_answers(ctx):
    from simpleicp_amd import Evaluation, _lib
    X = np.random.default_rng(38).uniform(-1, 1, (12_345, 3))
    ctx.upload(_lib.FIX, X)
    ctx.upload(_lib.MOV, X)
    ev = Evaluation.from_record(ctx.evaluate(_lib.FIX, _lib.MOV, None, 0.5))
    assert ev.fitness == 1.0 and ev.sum_d2 == 0.0 and ev.inlier_rmse == 0.0 and ev.n_queries == 12_345
    assert np.allclose(ev.centroid, X.mean(axis=0), rtol=0, atol=1e-12)
    assert np.allclose(ev.information, eval_ref.information_rows(X), rtol=1e-12, atol=1e-9)
    shift = np.eye(4)
    shift[0, 3] = 10 * (X[:, 0].max() - X[:, 0].min())
    ev = Evaluation.from_record(ctx.evaluate(_lib.FIX, _lib.MOV, shift, 0.5))
    assert ev.fitness == 0.0 and ev.n_inliers == 0 and ev.inlier_rmse == 0.0 and not ev.information.any()


# ---- refusals ----
def test_refusals_name_the_argument(ctx):
    from simpleicp_amd import _lib
    X = np.random.default_rng(39).normal(0, 1, (500, 3))
    ctx.upload(_lib.FIX, X)
    ctx.upload(_lib.MOV, X)
    for bad, word in ((dict(max_distance=float("nan")), "max_distance"), (dict(max_distance=-1.0), "max_distance"),
                      (dict(rows=np.array([0, 500])), r"sel_idx\[1\]"), (dict(rows=np.array([-1])), r"sel_idx\[0\]")):
        with pytest.raises(_lib.BackendError, match=word) as e:
            ctx.evaluate(_lib.FIX, _lib.MOV, **bad)
        assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(ValueError, match="rows"):
        ctx.evaluate(_lib.FIX, _lib.MOV, rows=np.empty(0, np.int64))
    with pytest.raises(_lib.BackendError, match="query_slot and search_slot"):
        ctx.evaluate(_lib.FIX, _lib.FIX)
    rec = _lib.EvalRecord()
    L = ctx._L
    assert L.sicp_evaluate(ctx._h, _lib.FIX, _lib.MOV, None, 0, None, 1.0, None) == _lib.ERR_INVALID
    assert b"out" in L.sicp_last_error()
    assert L.sicp_evaluate(ctx._h, 5, _lib.MOV, None, 0, None, 1.0, C.byref(rec)) == _lib.ERR_INVALID
    with _lib.Context(0) as empty:
        empty.upload(_lib.FIX, X)
        with pytest.raises(_lib.BackendError, match="empty"):
            empty.evaluate(_lib.FIX, _lib.MOV)
        empty.upload(_lib.MOV, X)
        empty.upload(_lib.FIX, X, index_base=1000)                    # a shard
        with pytest.raises(_lib.BackendError, match="shard"):
            empty.evaluate(_lib.FIX, _lib.MOV)
    ctx.set_exchange(lambda *a: 0, 0, 1)
    try:
        with pytest.raises(_lib.BackendError, match="not supported with an exchange") as e:
            ctx.evaluate(_lib.FIX, _lib.MOV)
        assert e.value.code == _lib.ERR_INVALID
    finally:
        ctx.set_exchange(None, 0, 1)
    assert ctx.evaluate(_lib.FIX, _lib.MOV, None, np.inf).n_inliers == 500         # +inf is allowed


# ---- end to end ----
def dev(X):
    return torch.tensor(np.ascontiguousarray(X), dtype=torch.float64, device=DEV)


def fields(ev):
    return (ev.n_queries, ev.n_inliers, np.array([ev.sum_d2, *ev.sum_p, *ev.sum_pp]).tobytes())


@pytest.fixture(scope="module")
def dragon(clouds):
    """the bundled pair, its run() without the evaluation, and the distance.  The movable cloud is the fixed one moved rigidly, both
    stored on a lattice of 1e-4: after the run the nearest neighbours lie a lattice step apart or less, and half a step splits
    the fixed points into inliers and outliers"""
    from simpleicp_amd import PointCloud, SimpleICP
    g, files, kw = load_golden("dragon")
    Xf, Xm = clouds(files[0]), clouds(files[1])
    d = 0.5e-4
    icp = SimpleICP(verbose=False)
    icp.add_point_clouds(PointCloud(Xf, columns=["x", "y", "z"]), PointCloud(Xm.copy(), columns=["x", "y", "z"]))
    plain = icp.run(**kw)
    assert icp.evaluation is None and "evaluation" not in icp.last_run_info
    return Xf, Xm, kw, d, plain


def test_run_reports_what_evaluate_registration_reports(dragon):
    from simpleicp_amd import PointCloud, SimpleICP, evaluate_registration
    Xf, Xm, kw, d, plain = dragon
    icp = SimpleICP(verbose=False)
    icp.add_point_clouds(PointCloud(Xf, columns=["x", "y", "z"]), PointCloud(Xm.copy(), columns=["x", "y", "z"]))
    icp.evaluate_distance = d
    H, X, rbp, res = icp.run(**kw)
    # the run itself is the run without it, bit for bit
    assert H.tobytes() == plain[0].tobytes() and res.tobytes() == plain[3].tobytes() and X.tobytes() == plain[1].tobytes()
    ev = icp.evaluation
    assert ev is icp.last_run_info["evaluation"]
    assert ev.n_queries == len(Xf) and 0 < ev.n_inliers < len(Xf) and 0 < ev.inlier_rmse < d
    alone = evaluate_registration(PointCloud(Xf, columns=["x", "y", "z"]), PointCloud(Xm.copy(), columns=["x", "y", "z"]), H, d)
    assert fields(alone) == fields(ev)
    assert fields(evaluate_registration(Xf, Xm, H, d)) == fields(ev)
    assert fields(evaluate_registration(dev(Xf), dev(Xm), H, d)) == fields(ev)


def test_run_tensors_reports_the_same_record(dragon):
    from simpleicp_amd import evaluate_registration, run_tensors
    Xf, Xm, kw, d, plain = dragon
    tf, tm = dev(Xf), dev(Xm)
    res = run_tensors(tf, tm, evaluate_distance=d, **kw)
    assert res.path == "device" and res.H.tobytes() == plain[0].tobytes() and res.residuals.tobytes() == plain[3].tobytes()
    assert fields(res.evaluation) == fields(evaluate_registration(Xf, Xm, plain[0], d))
    off = run_tensors(tf, tm, **kw)
    assert off.evaluation is None and off.H.tobytes() == res.H.tobytes()
    assert torch.equal(off.X_mov_transformed, res.X_mov_transformed)
    assert np.array_equal(tf.cpu().numpy(), Xf) and np.array_equal(tm.cpu().numpy(), Xm)      # the inputs are not modified


def test_run_batch_keeps_the_pairs_batched(dragon):
    from simpleicp_amd import backend, evaluate_registration, run_batch
    Xf, Xm, kw, d, plain = dragon
    want = fields(evaluate_registration(Xf, Xm, plain[0], d))
    try:
        out = run_batch([(Xf, Xm), (dev(Xf), dev(Xm)), (Xf, Xm)], evaluate_distance=d,
                        per_pair=[None, None, {"evaluate_distance": None}], **kw)
        assert [r.path for r in out] == ["batched"] * 3 and all(r.error is None for r in out)
        for r in out:
            assert r.H.tobytes() == plain[0].tobytes() and r.residuals.tobytes() == plain[3].tobytes()
        assert fields(out[0].evaluation) == want and fields(out[1].evaluation) == want
        assert out[2].evaluation is None
        assert np.array_equal(out[0].X_mov_transformed, plain[1]) and np.array_equal(out[2].X_mov_transformed, plain[1])
        bad = run_batch([(Xf, Xm + 1e4)], evaluate_distance=d, max_overlap_distance=d, **{k: v for k, v in kw.items()
                                                                                       if k != "max_overlap_distance"})
        assert bad[0].error is not None and bad[0].evaluation is None
    finally:
        backend.reset_batch_contexts()


def test_of_movable_is_the_inverse_direction(dragon):
    from simpleicp_amd import evaluate_registration
    Xf, Xm, kw, d, plain = dragon
    Xf, Xm, H = Xf[::4], Xm[::4], plain[0]
    Hi = np.eye(4)
    Hi[:3, :3] = H[:3, :3].T
    Hi[:3, 3] = -(H[:3, :3].T @ H[:3, 3])
    ev = evaluate_registration(Xf, Xm, H, d, of="movable")
    want = eval_ref.evaluate(Xm, Xf, Hi, d)
    assert (ev.n_queries, ev.n_inliers) == (len(Xm), want["n_inliers"]) and 0 < ev.n_inliers < len(Xm)
    assert np.array([ev.sum_d2, *ev.sum_p, *ev.sum_pp]).tobytes() == want["sums"].tobytes()
    fwd = evaluate_registration(Xf, Xm, H, d)
    same_bits_ev(fwd, eval_ref.evaluate(Xf, Xm, H, d))


def same_bits_ev(ev, want):
    assert (ev.n_queries, ev.n_inliers) == (want["n_queries"], want["n_inliers"])
    assert np.array([ev.sum_d2, *ev.sum_p, *ev.sum_pp]).tobytes() == want["sums"].tobytes()
