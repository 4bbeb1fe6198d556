"""Rejection by the angle between normals on the device (include/simpleicp_hip_normals.h) against tests/normal_angle_ref.py --
the oracle's k-NN, normals and rejection plus contract (N) restated in numpy float64."""
import math

import numpy as np
import pytest

import normal_angle_ref as ref
from oracle import orc

pytestmark = pytest.mark.gpu

Z6 = np.zeros(6)


@pytest.fixture()
def ctx():
    with _lib_context() as c:
        yield c


def _lib_context():
    from simpleicp_amd import _lib
    return _lib.Context()


def _lib_H(x):
    from simpleicp_amd import _lib
    return _lib.params_to_H(x)


def _fixed_side(Xf, Q, k=10):
    sel = orc.select_n_points(len(Xf), Q)
    sel = np.arange(len(Xf)) if sel is None else np.unique(sel)
    nn, _ = orc.knn(Xf, Xf[sel], k=k)
    n1, pl = orc.normals(Xf, nn)
    return sel, n1, pl


# (fixed, movable, correspondences, movable points kept (None = all), max angle in degrees, initial rotation about z in degrees)
CASES = {
    "dragon_q1000": ("dragon1", "dragon2", 1000, None, 30.0, 0.0),          # single-workgroup tail
    "bunny_q10000": ("bunny_part1", "bunny_part2", 10000, None, 25.0, 10.0),   # k_reject_reg
    "dragon_q70000": ("dragon1", "dragon2", 70000, 10000, 30.0, 0.0),       # many-queries search + k_hsel_all; reduced movable cloud
}
_case_cache = {}


def _case(name):
    """The clouds, the fixed side and the reference run of a case; the data condition is asserted here: the reference's verdict
    drops between 2 % and 60 % of the planarity-surviving correspondences in iteration 0, and its run ends with >= 6
    correspondences before max_iterations -- a later change of data cannot hollow the tests out."""
    if name not in _case_cache:
        fix, mov, Q, nmov, angle, rot = CASES[name]
        Xf, Xm = orc.load_cloud(fix), orc.load_cloud(mov)
        if nmov is not None:
            Xm = np.ascontiguousarray(Xm[orc.select_n_points(len(Xm), nmov)])
        sel, n1, pl = _fixed_side(Xf, Q)
        obs = np.array([0.0, 0.0, math.radians(rot), 0.0, 0.0, 0.0])
        cos_max = math.cos(math.radians(angle))
        r = ref.run(Xm, Xf[sel], n1, pl, obs, Z6, 0.3, cos_max, 10)
        share = ref.dropped_share(r["first"])
        print(f"{name}: reference drops {share:.3f} of the planar correspondences in iteration 0, {r['iterations']} iterations, "
              f"{r['last']['n']} kept")
        assert 0.02 <= share <= 0.60
        assert r["last"]["n"] >= 6 and r["iterations"] < 100
        _case_cache[name] = dict(Xf=Xf, Xm=Xm, sel=sel, n1=n1, pl=pl, obs=obs, cos_max=cos_max, angle=angle, rot=rot, ref=r, Q=Q)
    return _case_cache[name]


def _setup(ctx, c):
    from simpleicp_amd import _lib
    ctx.upload(_lib.FIX, c["Xf"])
    ctx.upload(_lib.MOV, c["Xm"])
    ctx.icp_setup(c["sel"], c["n1"], c["pl"])


# ---- the verdict kernel through the operator ----------------------------------------------------------------------------------

def _surface(rng, n, offset=(0.0, 0.0, 0.0), lattice=False, coincident=False):
    if lattice:                                     # integer lattice on two planes: exact distance ties everywhere
        m = int(math.isqrt(n // 2))
        gx, gy = np.meshgrid(np.arange(m, dtype=float), np.arange(m, dtype=float))
        a = np.column_stack([gx.ravel(), gy.ravel(), np.zeros(m * m)])
        b = np.column_stack([gx.ravel(), np.zeros(m * m), gy.ravel() + 1.0])
        X = np.vstack([a, b])
    else:
        xy = rng.uniform(-5, 5, (n, 2))
        z = 0.4 * np.sin(xy[:, 0]) + 0.3 * np.cos(1.3 * xy[:, 1]) + 0.01 * rng.standard_normal(n)
        X = np.column_stack([xy, z])
        half = n // 2
        X[half:] = np.column_stack([X[half:, 0], 0.5 * X[half:, 2] + 5.0, X[half:, 1]])      # a second, upright sheet: a corner scene
    if coincident:                                  # blocks of 12 identical points: degenerate neighbourhoods
        X = np.repeat(X[: len(X) // 12], 12, axis=0)
    return np.ascontiguousarray(X + np.asarray(offset))


KINDS = ["random", "ties", "coincident", "utm", "far_origin"]


def _verdict_case(kind):
    """Clouds, fixed side and H of a verdict test (host only)."""
    rng = np.random.default_rng(7)
    offset = {"utm": (5.0e5, 5.4e6, 300.0), "far_origin": (1.0e7, -1.0e7, 1.0e7)}.get(kind, (0.0, 0.0, 0.0))
    Xm = _surface(rng, 6000, offset, lattice=kind == "ties", coincident=kind == "coincident")
    x = np.array([0.02, -0.015, 0.03, 0.0, 0.0, 0.0])
    H = orc.params_to_H(x)
    Xf = orc.transform(H, Xm[rng.permutation(len(Xm))[:3000]] + 0.02 * rng.standard_normal((3000, 3)))
    sel, n1, pl = _fixed_side(Xf, 1500)
    return Xf, Xm, sel, n1, pl, H


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("source", ["cache", "columns", "per_correspondence"])
def test_verdict_masks_bit_equal(ctx, kind, source):
    from simpleicp_amd import _lib
    Xf, Xm, sel, n1, pl, H = _verdict_case(kind)
    k = 10
    cos_max = math.cos(math.radians(5.0 if kind == "ties" else 35.0))      # (on the lattice only the corner's pairs tilt: a tight angle drops some)
    ctx.upload(_lib.FIX, Xf)
    ctx.upload(_lib.MOV, Xm)
    ctx.icp_setup(sel, n1, pl)
    idx, _ = ctx.corr_match(H)
    nn, _ = orc.knn(Xm, Xf[sel], k=1, H=H)
    assert np.array_equal(idx, nn[:, 0])
    n2 = ref.movable_normals(Xm, idx, k)
    if source != "cache":                           # the caller's own normals, some of them NaN: those must fail
        n2 = n2.copy()
        n2[idx % 17 == 0] = np.nan
    c = ref.cos_of(n1, n2, H)
    assert not np.any(np.abs(np.abs(c[np.isfinite(c)]) - cos_max) < 1e-12)        # (no verdict hangs on the last bit of the test's own data)
    want = ref.verdict(n1, n2, H, cos_max)
    if source == "columns":
        col = np.full((len(Xm), 3), np.nan, np.float32)
        col[idx] = n2
        ctx.set_normals(_lib.MOV, col)
        n_alive = ctx.corr_reject_normal_angle(cos_max, k, H)
    elif source == "per_correspondence":
        n_alive = ctx.corr_reject_normal_angle(cos_max, k, H, n2)
    else:
        n_alive = ctx.corr_reject_normal_angle(cos_max, k, H)
    _, _, alive, _ = ctx.icp_state(pc2_idx=False, dist=False, residual=False)
    assert want.any() and not want.all()
    assert np.array_equal(alive, want) and n_alive == int(want.sum())
    info = ctx.normal_angle_info()
    assert info["normal_angle_dropped"] == int((~want).sum())
    if source == "cache":
        assert info["normals_estimated"] == len(np.unique(idx))
        nv, have = ctx.normal_cache()
        assert np.array_equal(np.flatnonzero(have), np.unique(idx))
        assert np.array_equal(nv[idx].view(np.uint32), n2.view(np.uint32))


# ---- the cache ----------------------------------------------------------------------------------------------------------------

def test_cache_contents_and_lifetime(ctx):
    from simpleicp_amd import _lib
    c = _case("dragon_q1000")
    _setup(ctx, c)
    ctx.normal_angle_set(c["cos_max"], 10)
    assert ctx.normal_angle_info()["normal_cache_bytes"] == 0          # allocated by the first run that needs it
    x, seen = c["obs"].copy(), set()
    for _ in range(4):
        R = ctx.icp_iterate(x, c["obs"], Z6, 0.3, 1.0)
        idx, _, _, _ = ctx.icp_state(dist=False, keep=False, residual=False)
        seen.update(int(m) for m in idx[c["pl"] >= np.float32(0.3)])
        x = np.array(R.x[:])
    rows = np.array(sorted(seen), dtype=np.int64)
    info = ctx.normal_angle_info()
    assert info["normals_estimated"] == len(rows)                      # one estimate per distinct matched point, none twice
    assert info["normal_cache_bytes"] >= 12 * len(c["Xm"])
    nv, have = ctx.normal_cache()
    assert np.array_equal(np.flatnonzero(have), rows)                  # never matched = still "not computed"
    want, _ = ctx.estimate_normals(_lib.MOV, rows, 10)
    assert np.array_equal(nv[rows].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(want.view(np.uint32), ref.movable_normals(c["Xm"], rows, 10).view(np.uint32))
    # a second run on the same uploaded cloud: nothing is estimated again
    ctx.icp_setup(c["sel"], c["n1"], c["pl"])
    x = c["obs"].copy()
    for _ in range(4):
        x = np.array(ctx.icp_iterate(x, c["obs"], Z6, 0.3, 1.0).x[:])
    info = ctx.normal_angle_info()
    assert info["normals_estimated"] == 0 and info["normal_miss_free_iterations"] == 4
    # a transform or an upload of the slot empties it
    ctx.transform(_lib.MOV, np.eye(4))
    assert not ctx.normal_cache()[1].any() and ctx.normal_angle_info()["normal_cache_bytes"] == 0
    ctx.icp_iterate(c["obs"], c["obs"], Z6, 0.3, 1.0)
    assert ctx.normal_cache()[1].any()
    ctx.upload(_lib.MOV, c["Xm"])
    assert not ctx.normal_cache()[1].any()


def test_one_context_across_correspondence_counts(ctx):
    """A context is reused from run to run (the pool behind run()): 70 000 correspondences (the four-per-wave sweep, whose spill list
    shares a buffer with the one-per-wave sweep's slot list), then 1000, then 5000 (more slots than the run before it walked), each
    from an empty cache -- so that every planar correspondence misses -- against the reference's first iteration."""
    from simpleicp_amd import _lib
    c = _case("dragon_q70000")
    Xf, Xm = c["Xf"], c["Xm"]
    ctx.upload(_lib.FIX, Xf)
    ctx.normal_angle_set(c["cos_max"], 10)
    for Q in (70000, 1000, 5000, 70000, 5000):
        sel, n1, pl = (c["sel"], c["n1"], c["pl"]) if Q == 70000 else _fixed_side(Xf, Q)
        o = c["ref"]["its"][0] if Q == 70000 else ref.iteration(Xm, Xf[sel], n1, pl, c["obs"], 1.0, c["obs"], Z6, 0.3, c["cos_max"], 10)
        ctx.upload(_lib.MOV, Xm)                     # (empties the cache; the context and its buffers stay)
        ctx.icp_setup(sel, n1, pl)
        R = ctx.icp_iterate(c["obs"], c["obs"], Z6, 0.3, 1.0)
        idx, dist, keep, _ = ctx.icp_state(residual=False)
        assert np.array_equal(idx, o["nn"]) and np.array_equal(dist, o["dist"])
        assert np.array_equal(keep, o["keep"])
        assert R.n_planar == int((o["planar_ok"] & o["angle_ok"]).sum()) and (R.median, R.mad) == (o["median"], o["mad"])
        rows = np.unique(idx[o["planar_ok"]])
        nv, have = ctx.normal_cache()
        assert np.array_equal(np.flatnonzero(have), rows) and ctx.normal_angle_info()["normals_estimated"] == len(rows)
        assert np.array_equal(nv[rows].view(np.uint32), ref.movable_normals(Xm, rows, 10).view(np.uint32))


# ---- whole iterations and runs ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_iterations_against_reference(ctx, name):
    """Every iteration of the reference run, the device started from the reference's estimate: indices, distances, keep masks,
    median / MAD bit for bit, the estimate to 1e-9."""
    c = _case(name)
    _setup(ctx, c)
    ctx.normal_angle_set(c["cos_max"], 10)
    p1 = c["Xf"][c["sel"]]
    its = c["ref"]["its"]
    for o in its[: 4 if c["Q"] > 20000 else 8]:
        R = ctx.icp_iterate(o["x_prev"], c["obs"], Z6, 0.3, 1.0)
        idx, dist, keep, resid = ctx.icp_state()
        assert np.array_equal(idx, o["nn"])
        assert np.array_equal(dist, o["dist"])
        assert np.array_equal(keep, o["keep"])
        assert R.n_planar == int((o["planar_ok"] & o["angle_ok"]).sum())
        assert R.n_kept == o["n"] and R.median == o["median"] and R.mad == o["mad"]
        xg = np.array(R.x[:])
        assert np.abs(xg - o["x"]).max() < 1e-9
        assert np.allclose(resid[keep], orc.residuals(xg, p1, c["n1"], c["Xm"][idx], keep), rtol=0, atol=1e-13)
        assert ctx.normal_angle_info()["normal_angle_dropped"] == int((o["planar_ok"] & ~o["angle_ok"]).sum())


def _operator_iteration(ctx, c, x, H):
    """match -> reject_wrt_planarity -> reject_wrt_normal_angle -> reject distances -> estimate, through the operator ABI"""
    ctx.corr_match(H)
    ctx.corr_reject_planarity(0.3, c["pl"], None)
    ctx.corr_reject_normal_angle(c["cos_max"], 10, H)
    med, mad, n = ctx.corr_reject_distances()
    R = ctx.estimate_parameters(x, c["obs"], Z6, 1.0)
    return R, med, mad, n


@pytest.mark.parametrize("name", list(CASES))
def test_chained_run_equals_iterate_loop_equals_operators(ctx, name):
    c = _case(name)
    r = c["ref"]
    _setup(ctx, c)
    ctx.normal_angle_set(c["cos_max"], 10)
    x, loop = c["obs"].copy(), []
    for it in range(100):
        R = ctx.icp_iterate(x, c["obs"], Z6, 0.3, 1.0)
        loop.append(R)
        x = np.array(R.x[:])
        ch = lambda a, b: abs((a - b) / b * 100)      # noqa: E731
        if it > 0 and ch(R.res_mean, loop[-2].res_mean) < 1 and ch(R.res_std, loop[-2].res_std) < 1:
            break
    _, _, keep_loop, _ = ctx.icp_state(pc2_idx=False, dist=False, residual=False)
    ctx.icp_setup(c["sel"], c["n1"], c["pl"])
    whole = ctx.icp_run(c["obs"], c["obs"], Z6, 0.3, 1.0, max_iterations=100, min_change=1.0)
    _, _, keep_whole, _ = ctx.icp_state(pc2_idx=False, dist=False, residual=False)
    assert len(whole) == len(loop) == r["iterations"]
    for a, b, o in zip(whole, loop, r["its"]):
        assert np.abs(np.array(a.x[:]) - np.array(b.x[:])).max() < 1e-13
        assert a.n_kept == b.n_kept == o["n"] and a.n_planar == b.n_planar
        assert np.abs(np.array(a.x[:]) - o["x"]).max() < 1e-9
    assert np.array_equal(keep_whole, keep_loop) and np.array_equal(keep_whole, r["last"]["keep"])
    # the operator road, iteration by iteration, each from the estimate AND the H the chained run recorded for the iteration before
    # (sicp_icp_iterate forms that same H from the estimate it is handed, so matches, distances and verdicts are comparable bit for
    # bit); against a host-driven iteration from the same estimate on a second context
    ctx.normal_angle_set(None)
    ctx.icp_setup(c["sel"], c["n1"], c["pl"])
    with _lib_context() as ref_ctx:
        _setup(ref_ctx, c)
        ref_ctx.normal_angle_set(c["cos_max"], 10)
        x, H = c["obs"].copy(), _lib_H(c["obs"])
        for a in whole:
            assert np.array_equal(H, _lib_H(x))
            R, med, mad, n = _operator_iteration(ctx, c, x, H)
            idx_o, dist_o, alive_o, _ = ctx.icp_state(residual=False)
            b = ref_ctx.icp_iterate(x, c["obs"], Z6, 0.3, 1.0)
            idx_i, dist_i, keep_i, _ = ref_ctx.icp_state(residual=False)
            assert np.array_equal(idx_o, idx_i) and np.array_equal(dist_o, dist_i)
            assert np.array_equal(alive_o, keep_i)
            assert (med, mad, n) == (b.median, b.mad, b.n_kept)
            assert int(alive_o.sum()) == n == a.n_kept
            assert np.abs(np.array(R.x[:]) - np.array(a.x[:])).max() < 1e-9
            x, H = np.array(a.x[:]), np.array(a.H[:]).reshape(4, 4)


# ---- through the front doors --------------------------------------------------------------------------------------------------

def _front_case():
    c = _case("dragon_q1000")
    return c, c["Xf"], c["Xm"]


def test_front_doors_agree():
    import torch
    import simpleicp_amd
    from simpleicp_amd import PointCloud, SimpleICP, batch
    c, Xf, Xm = _front_case()
    icp = SimpleICP(verbose=False)
    icp.add_point_clouds(PointCloud(Xf, columns=["x", "y", "z"]), PointCloud(Xm, columns=["x", "y", "z"]))
    icp.max_normal_angle = c["angle"]
    H, X_new, rbp, res = icp.run()
    info = icp.last_run_info
    assert info["normals_estimated"] > 0 and info["normal_cache_bytes"] > 0
    r = c["ref"]
    assert info["iterations"] == r["iterations"]
    assert np.abs(H - r["H"]).max() < 1e-9 and len(res) == r["last"]["n"]
    est = lambda p: np.array([getattr(p, n).estimated_value for n in ("alpha1", "alpha2", "alpha3", "tx", "ty", "tz")])   # noqa: E731
    for dtype in (torch.float64, torch.float32):
        tf = torch.as_tensor(Xf, dtype=dtype, device="cuda")
        tm = torch.as_tensor(Xm, dtype=dtype, device="cuda")
        out = simpleicp_amd.run_tensors(tf, tm, max_normal_angle=c["angle"])
        if dtype == torch.float64:
            assert np.array_equal(out.H, H) and np.array_equal(out.residuals, res) and np.array_equal(est(out.rbp), est(rbp))
        else:
            # float32 inputs are the float32-rounded clouds widened exactly: the same doors and the reference on THOSE clouds
            Xf32, Xm32 = Xf.astype(np.float32).astype(np.float64), Xm.astype(np.float32).astype(np.float64)
            sel32, n32, pl32 = _fixed_side(Xf32, 1000)
            r32 = ref.run(Xm32, Xf32[sel32], n32, pl32, Z6, Z6, 0.3, c["cos_max"], 10)
            assert 0.02 <= ref.dropped_share(r32["first"]) <= 0.60 and r32["last"]["n"] >= 6 and r32["iterations"] < 100
            icp32 = SimpleICP(verbose=False)
            icp32.add_point_clouds(PointCloud(Xf32, columns=["x", "y", "z"]), PointCloud(Xm32, columns=["x", "y", "z"]))
            icp32.max_normal_angle = c["angle"]
            H32, _, rbp32, res32 = icp32.run()
            assert np.array_equal(out.H, H32) and np.array_equal(out.residuals, res32) and np.array_equal(est(out.rbp), est(rbp32))
            assert out.iterations == r32["iterations"] and len(res32) == r32["last"]["n"]
            assert np.abs(H32 - r32["H"]).max() < 1e-9
            b32 = simpleicp_amd.run_batch([(Xf32, Xm32), (tf, tm)], max_normal_angle=c["angle"])
            for o in b32:
                assert o.error is None and o.path == "fallback"
                assert np.array_equal(o.H, H32) and np.array_equal(o.residuals, res32) and np.array_equal(est(o.rbp), est(rbp32))
    # run_batch: host and device pairs, one member with and one without the angle
    tf = torch.as_tensor(Xf, dtype=torch.float64, device="cuda")
    tm = torch.as_tensor(Xm, dtype=torch.float64, device="cuda")
    outs = simpleicp_amd.run_batch([(Xf, Xm), (Xf, Xm), (tf, tm), (tf, tm)],
                                   per_pair=[{"max_normal_angle": c["angle"]}, None, {"max_normal_angle": c["angle"]}, None])
    assert batch.last_run_info["fallback"] == 2
    assert [o.path for o in outs] == ["fallback", "batched", "fallback", "batched"]
    for o in (outs[0], outs[2]):
        assert o.error is None and np.array_equal(o.H, H) and np.array_equal(o.residuals, res) and np.array_equal(est(o.rbp), est(rbp))
    plain = SimpleICP(verbose=False)
    plain.add_point_clouds(PointCloud(Xf, columns=["x", "y", "z"]), PointCloud(Xm, columns=["x", "y", "z"]))
    H0, _, _, res0 = plain.run()
    for o in (outs[1], outs[3]):
        assert np.array_equal(o.H, H0) and np.array_equal(o.residuals, res0)
    assert not np.array_equal(H0, H)


def test_run_uses_the_movable_clouds_own_normals():
    """pc2 carries nx, ny, nz: they are used as they are (here: deliberately not the estimated ones)."""
    from simpleicp_amd import PointCloud, SimpleICP
    c, Xf, Xm = _front_case()
    nv = ref.movable_normals(Xm, np.arange(len(Xm)), 6)                 # another neighbourhood than run()'s
    pc2 = PointCloud(Xm, columns=["x", "y", "z"])
    pc2["nx"], pc2["ny"], pc2["nz"] = nv[:, 0], nv[:, 1], nv[:, 2]
    icp = SimpleICP(verbose=False)
    icp.add_point_clouds(PointCloud(Xf, columns=["x", "y", "z"]), pc2)
    icp.max_normal_angle = c["angle"]
    H, _, _, res = icp.run()
    assert icp.last_run_info["normals_estimated"] == 0
    sel, n1, pl = c["sel"], c["n1"], c["pl"]
    r = ref.run(Xm, Xf[sel], n1, pl, Z6, Z6, 0.3, c["cos_max"], 10, mov_normals=nv)
    assert np.abs(H - r["H"]).max() < 1e-9 and len(res) == r["last"]["n"]


def test_corrpts_operator():
    from simpleicp_amd import PointCloud
    from simpleicp_amd.corrpts import CorrPts
    c, Xf, Xm = _front_case()
    pc1, pc2 = PointCloud(Xf, columns=["x", "y", "z"]), PointCloud(Xm, columns=["x", "y", "z"])
    pc1.select_n_points(1000)
    pc1.estimate_normals(10)
    cp = CorrPts(pc1, pc2)
    cp.match()
    with pytest.raises(NotImplementedError):
        cp.reject_wrt_to_angle_between_normals()
    before = cp.num_corr_pts
    n1 = np.column_stack([cp.pc1_nx, cp.pc1_ny, cp.pc1_nz]).astype(np.float32)
    idx = cp._df["pc2_idx"].to_numpy()
    want = ref.verdict(n1, ref.movable_normals(Xm, idx, 10), np.eye(4), c["cos_max"])
    cp.reject_wrt_normal_angle(c["angle"])
    assert before == len(want) and cp.num_corr_pts == int(want.sum())
    assert np.array_equal(cp._df["pc2_idx"].to_numpy(), idx[want])


# ---- off means off, and the refusal -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", [("dragon1", "dragon2"), ("bunny_part1", "bunny_part2")])
def test_off_means_off(pair):
    from simpleicp_amd import PointCloud, SimpleICP

    def run(touch):
        icp = SimpleICP(verbose=False)
        icp.add_point_clouds(PointCloud(orc.load_cloud(pair[0]), columns=["x", "y", "z"]),
                             PointCloud(orc.load_cloud(pair[1]), columns=["x", "y", "z"]))
        if touch:
            icp.max_normal_angle = None
        H, X, rbp, res = icp.run()
        return H, X, res, icp.last_run_info

    H, X, res, info = run(True)
    assert info["normal_cache_bytes"] == 0 and info["normals_estimated"] == 0
    # a context on which the setting was never touched: the C ABI driven directly
    from simpleicp_amd import _lib
    Xf, Xm = orc.load_cloud(pair[0]), orc.load_cloud(pair[1])
    with _lib.Context() as c:
        c.upload(_lib.FIX, Xf)
        c.upload(_lib.MOV, Xm)
        pc1 = PointCloud(Xf, columns=["x", "y", "z"])
        pc1.select_n_points(1000)
        sel = pc1.idx_selected
        nv, pl = c.estimate_normals(_lib.FIX, sel, 10)
        c.icp_setup(sel, nv, pl)
        whole = c.icp_run(Z6, Z6, Z6, 0.3, 1.0, 100, 1.0)
        assert c.normal_angle_info() == {"normals_estimated": 0, "normal_angle_dropped": 0, "normal_cache_bytes": 0,
                                         "normal_miss_free_iterations": 0}
        assert np.array_equal(np.array(whole[-1].H[:]).reshape(4, 4), H)
        _, _, keep, r = c.icp_state(pc2_idx=False, dist=False)
        assert np.array_equal(r[keep], res)


def test_refused_with_an_exchange(ctx):
    from simpleicp_amd import _lib
    c = _case("dragon_q1000")
    _setup(ctx, c)
    ctx.set_exchange(lambda *a: 0, 0, 1)
    with pytest.raises(_lib.BackendError) as e:
        ctx.normal_angle_set(c["cos_max"], 10)
    assert e.value.code == _lib.ERR_INVALID and "not supported with an exchange" in str(e.value)
    ctx.normal_angle_set(None)                       # off is never refused
    ctx.set_exchange(None, 0, 1)
    ctx.normal_angle_set(c["cos_max"], 10)
