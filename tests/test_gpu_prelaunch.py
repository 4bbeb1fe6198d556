"""The tail -> match hand-over of a small-Q chain ("The tail -> match hand-over"): the next match is launched early on the
context's second stream and waits for the tail's ticket.  Every case runs with the hand-over and again with SICP_CHAIN_PRELAUNCH=0
(the single-stream chain) in a fresh context and requires every IterResult of every iteration and icp_state() to agree bit for bit."""
import functools
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 20_000
KW = dict(x=np.zeros(6), obs=np.zeros(6), obs_weight=np.zeros(6), min_planarity=0.3, distance_weight=1.0, max_iterations=9,
          min_change=0.0)


@functools.lru_cache(maxsize=None)
def surface_pair(n=N, seed=7):
    rng = np.random.default_rng(seed)
    half = np.sqrt(n / 10.0) / 2
    xy = rng.uniform(-half, half, (n, 2))
    z = 2 * np.sin(xy[:, 0] / 4) * np.cos(xy[:, 1] / 6) + rng.normal(0, 0.005, n)
    Xf = np.column_stack((xy, z))
    c, s = np.cos(0.02), np.sin(0.02)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    Xm = (Xf + rng.normal(0, 0.005, Xf.shape)) @ R.T + np.array((0.3, -0.2, 0.1))
    Xf.setflags(write=False); Xm.setflags(write=False)
    return Xf, Xm


def setup(ctx, Q, planarity=None):
    from simpleicp_amd import _lib
    Xf, _ = surface_pair()
    sel = np.unique(np.round(np.linspace(0, len(Xf) - 1, Q)).astype(np.int64))
    assert len(sel) == Q
    nv, pl = ctx.estimate_normals(_lib.FIX, sel, 8)
    ctx.icp_setup(sel, nv, pl if planarity is None else planarity(pl))


def context(monkeypatch, on):
    from simpleicp_amd import _lib
    if on:
        monkeypatch.delenv("SICP_CHAIN_PRELAUNCH", raising=False)
    else:
        monkeypatch.setenv("SICP_CHAIN_PRELAUNCH", "0")
    ctx = _lib.Context(0)                    # (the switch is read here)
    Xf, Xm = surface_pair()
    ctx.upload(_lib.FIX, Xf)
    ctx.upload(_lib.MOV, Xm)
    return ctx


def run(ctx, **kw):
    """(error code or None, the iterations' records as bytes, icp_state(), matches launched early, seconds)"""
    from simpleicp_amd import _lib
    t0 = time.perf_counter()
    try:
        res, code = ctx.icp_run(**dict(KW, **kw)), None
    except _lib.BackendError as e:
        res, code = e.results, e.code
    dt = time.perf_counter() - t0
    return code, [bytes(r) for r in res], ctx.icp_state(), ctx.chain_info()["last_run"], dt


def same(a, b):
    assert a[0] == b[0]
    assert len(a[1]) == len(b[1]) and all(r == s for r, s in zip(a[1], b[1]))
    for u, v in zip(a[2], b[2]):
        assert np.array_equal(u, v, equal_nan=True)


def both(monkeypatch, script):
    """script(ctx) -> list of run() results, once per switch position"""
    out = []
    for on in (True, False):
        ctx = context(monkeypatch, on)
        try:
            out.append(script(ctx))
        finally:
            ctx.close()
    for a, b in zip(*out):
        same(a, b)
    assert all(r[3] == 0 for r in out[1])               # SICP_CHAIN_PRELAUNCH=0: never
    return out[0]


@pytest.mark.parametrize("Q", [40, 1000, 1024, 1025, 2048, 2049])
def test_query_counts(monkeypatch, Q):
    """The road is taken up to 1024 correspondences (one match workgroup per CU at most, four correspondences per tail lane: the
    tail fits next to a waiting match wave); above, and at 2049 where the tail is another chain altogether, it is not.  1024 is
    the tightest case the road takes (256 match workgroups: one per CU of the device), 1025 the first it leaves."""
    def script(ctx):
        setup(ctx, Q)
        return [run(ctx)]
    (r,) = both(monkeypatch, script)
    assert r[0] is None and len(r[1]) == 9
    assert r[3] == (8 if Q <= 1024 else 0)


@pytest.mark.parametrize("iters", [1, 2, 3, 9])
def test_iteration_counts(monkeypatch, iters):
    """A lone match, one launch per stream, odd and even tails."""
    def script(ctx):
        setup(ctx, 1000)
        return [run(ctx, max_iterations=iters)]
    (r,) = both(monkeypatch, script)
    assert len(r[1]) == iters and r[3] == (iters - 1 if iters > 1 else 0)


def test_convergence_leaves_queued_launches(monkeypatch):
    """The launches queued behind the converged iteration leave through the stop path, ticket included."""
    def script(ctx):
        setup(ctx, 1000)
        return [run(ctx, max_iterations=30, min_change=1.0)]
    (r,) = both(monkeypatch, script)
    assert r[0] is None and 2 <= len(r[1]) < 30 and r[3] > 0 and r[4] < 1.0


def test_runs_back_to_back_with_a_new_setup(monkeypatch):
    """Sequence numbers carry on over runs and setups: a ticket of an earlier run never releases a later wait."""
    def script(ctx):
        out = []
        setup(ctx, 1000)
        out.append(run(ctx))
        setup(ctx, 333)
        out.append(run(ctx, max_iterations=5))
        out.append(run(ctx, x=np.array([0.001, 0.0, -0.001, 0.01, 0.0, 0.02]), max_iterations=4))
        return out
    rs = both(monkeypatch, script)
    assert [r[3] for r in rs] == [8, 4, 3]


@pytest.mark.parametrize("planar", [0, 4])
def test_early_exits_publish_the_ticket(monkeypatch, planar):
    """No correspondence passes the planarity test (m == 0) / fewer than six are kept: the tail's early exits publish the ticket,
    the matches queued behind them are released at once and the call returns its status long before a wait could expire."""
    from simpleicp_amd import _lib

    def planarity(pl):
        out = np.zeros_like(pl)
        out[:planar] = 1.0
        return out

    def script(ctx):
        setup(ctx, 1000, planarity)
        return [run(ctx)]
    (r,) = both(monkeypatch, script)
    assert r[0] == _lib.ERR_TOO_FEW and len(r[1]) == 1
    assert r[4] < 1.0


def test_timing_events_fall_back_to_one_stream(monkeypatch):
    def script(ctx):
        setup(ctx, 1000)
        ctx.timing_enable(True)
        a = run(ctx)
        ctx.timing_enable(False)
        return [a, run(ctx, max_iterations=4)]
    a, b = both(monkeypatch, script)
    assert a[3] == 0 and b[3] == 3


def test_other_roads_after_a_prelaunched_run(monkeypatch):
    """A batch of two and a device-tensor run in a process that has handed over early: they agree with their own lone runs."""
    import torch
    from simpleicp_amd import PointCloud, SimpleICP, run_batch, run_tensors
    monkeypatch.delenv("SICP_CHAIN_PRELAUNCH", raising=False)
    ctx = context(monkeypatch, True)
    try:
        setup(ctx, 1000)
        assert run(ctx)[3] == 8
    finally:
        ctx.close()
    Xf, Xm = surface_pair()
    kw = dict(correspondences=600, max_iterations=6, neighbors=8)

    def cloud(X):
        return PointCloud(np.array(X, copy=True), columns=["x", "y", "z"])

    def lone(A, B):
        icp = SimpleICP(verbose=False)
        icp.add_point_clouds(cloud(A), cloud(B))
        return icp.run(**kw)

    pairs = [(Xf, Xm), (Xf[:8000], Xm[:8000])]
    refs = [lone(A, B) for A, B in pairs]
    for res, ref in zip(run_batch([(cloud(A), cloud(B)) for A, B in pairs], **kw), refs):
        assert res.error is None and np.array_equal(res.H, ref[0]) and np.array_equal(res.residuals, ref[3])
    dev = torch.device("cuda:0")
    res = run_tensors(torch.as_tensor(np.array(Xf), device=dev), torch.as_tensor(np.array(Xm), device=dev), **kw)
    assert np.array_equal(res.H, refs[0][0]) and np.array_equal(res.residuals, refs[0][3])
