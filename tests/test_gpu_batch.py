"""run_batch / sicp_icp_run_batch on the GPU: every member bit-identical to its lone run (SimpleICP.run, sicp_icp_run), the
fallback, failures mid-batch, the member contexts' state afterwards, batch sizes, batch-wide refusals, and the upload_start fix."""
import numpy as np
import pandas as pd
import pytest

from conftest import GOLDEN_CASES, GOLDEN_CHAIN, load_golden

pytestmark = pytest.mark.gpu


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


def cloud(X):
    from simpleicp_amd import PointCloud
    return PointCloud(np.array(X, copy=True), columns=["x", "y", "z"])


def lone(pc1, pc2, **kw):
    from simpleicp_amd import PointCloud, SimpleICP
    icp = SimpleICP(verbose=False)
    icp.add_point_clouds(PointCloud(pc1.copy(deep=True)), PointCloud(pc2.copy(deep=True)))
    return icp.run(**kw), icp.last_run_info


def assert_same(res, ref, info):
    H, X, rbp, resid = ref
    assert res.error is None
    assert np.array_equal(res.H, H)
    assert np.array_equal(res.X_mov_transformed, X)
    assert np.array_equal(res.residuals, resid)
    assert res.iterations == info["iterations"]
    for name in ("alpha1", "alpha2", "alpha3", "tx", "ty", "tz"):
        a, b = getattr(res.rbp, name), getattr(rbp, name)
        assert a.estimated_value == b.estimated_value and a.initial_value == b.initial_value
        assert np.array_equal(a.estimated_uncertainty, b.estimated_uncertainty, equal_nan=True)


def golden_pair(name, clouds):
    g, files, kw = load_golden(name)
    pc_fix, pc_mov = cloud(clouds(files[0])), cloud(clouds(files[1]))
    if "mov_sel_idx" in g.files:
        pc_mov.idx_selected = g["mov_sel_idx"]
        v = np.full(len(pc_mov), np.nan, np.float32)
        v[g["mov_planarity_rows"]] = g["mov_planarity_vals"]
        pc_mov["planarity"] = pd.arrays.SparseArray(v)
    return pc_fix, pc_mov, kw


def test_golden_cases_in_one_batch(clouds):
    from simpleicp_amd import run_batch
    names = GOLDEN_CASES + GOLDEN_CHAIN
    pairs, per = [], []
    for name in names:
        pc_fix, pc_mov, kw = golden_pair(name, clouds)
        pairs.append((pc_fix, pc_mov))
        per.append(kw)
    out = run_batch(pairs, per_pair=per)
    for name, (pc_fix, pc_mov), kw, res in zip(names, pairs, per, out):
        ref, info = lone(pc_fix, pc_mov, **kw)
        assert_same(res, ref, info)
        assert res.path == ("fallback" if name == "dragon_q5000" else "batched"), name


def test_synthetic_batch_mixed_sizes():
    from simpleicp_amd import SimpleICPException, run_batch
    rng = np.random.default_rng(42)
    sizes = [1000, 3000, 10_000, 30_000] * 16
    sizes[::16] = [200_000] * 4
    qs = [6, 40, 200, 256, 257, 512, 513, 1024, 1025, 1500, 2048, 100, 700, 1800, 64, 300] * 4
    pairs, per = [], []
    for i, (n, q) in enumerate(zip(sizes, qs)):
        Xf, Xm = surface_pair(n, 100 + i, shift=(rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), 0.05), yaw=rng.uniform(-0.05, 0.05))
        pairs.append((cloud(Xf), cloud(Xm)))
        per.append({"correspondences": q, "max_iterations": int(rng.integers(1, 30)), "min_change": float(rng.choice([0.0, 0.1, 1.0]))})
    out = run_batch(pairs, per_pair=per, neighbors=8)
    assert len(out) == 64
    n_failed = 0
    for (pc_fix, pc_mov), kw, res in zip(pairs, per, out):
        assert res.path == "batched"
        try:
            ref, info = lone(pc_fix, pc_mov, neighbors=8, **kw)
        except SimpleICPException as e:                        # (a handful of correspondences may not leave 6)
            assert isinstance(res.error, SimpleICPException) and str(res.error) == str(e)
            n_failed += 1
            continue
        assert_same(res, ref, info)
    assert n_failed <= 4


def test_failures_mid_batch():
    from simpleicp_amd import SimpleICPException, run_batch
    good = [surface_pair(5000, s) for s in range(4)]
    Xf, Xm = surface_pair(5000, 9)
    pairs = [(cloud(a), cloud(b)) for a, b in good[:2]] + [(cloud(Xf), cloud(Xm + np.array([500.0, 0, 0]))), (cloud(Xf), cloud(Xm))] \
        + [(cloud(a), cloud(b)) for a, b in good[2:]]
    per = [None, None, {"max_overlap_distance": 1.0}, {"min_planarity": 1.0}, None, None]
    out = run_batch(pairs, per_pair=per, correspondences=500)
    for i in (2, 3):
        with pytest.raises(SimpleICPException) as ei:
            lone(*pairs[i], correspondences=500, **per[i])
        assert isinstance(out[i].error, SimpleICPException) and str(out[i].error) == str(ei.value)
    for i in (0, 1, 4, 5):
        ref, info = lone(*pairs[i], correspondences=500)
        assert_same(out[i], ref, info)


def prepared(Xf, Xm, Q, seed=0):
    from simpleicp_amd import _lib
    ctx = _lib.Context(0)
    ctx.upload(_lib.FIX, Xf)
    ctx.upload(_lib.MOV, Xm)
    sel = np.unique(np.round(np.linspace(0, len(Xf) - 1, Q)).astype(np.int64))
    nv, pl = ctx.estimate_normals(_lib.FIX, sel, 8)
    ctx.icp_setup(sel, nv, pl)
    return ctx


KW = dict(x=np.zeros(6), obs=np.zeros(6), obs_weight=np.zeros(6), min_planarity=0.3, distance_weight=1.0, max_iterations=20,
          min_change=0.5)


def same_results(a, b):
    assert len(a) == len(b)
    for r, s in zip(a, b):
        assert bytes(r) == bytes(s)


def test_c_level_state_and_continuation():
    from simpleicp_amd import _lib
    data = [surface_pair(n, 50 + i) for i, n in enumerate((2000, 8000, 20_000))]
    Qs = (100, 600, 1900)
    alone = [prepared(Xf, Xm, q) for (Xf, Xm), q in zip(data, Qs)]
    batch = [prepared(Xf, Xm, q) for (Xf, Xm), q in zip(data, Qs)]
    ref = [c.icp_run(**KW) for c in alone]
    runs, fb = batch[0].icp_run_batch([(c, KW) for c in batch])
    assert fb == 0
    for r, c, a, lone_res in zip(runs, batch, alone, ref):
        assert r.status == _lib.OK and r.path == _lib.BATCH_PATH_BATCHED
        same_results(r.results, lone_res)
        for u, v in zip(c.icp_state(), a.icp_state()):
            assert np.array_equal(u, v)
        assert np.array_equal(c.icp_uncertainties(), a.icp_uncertainties(), equal_nan=True)
        x = np.array(lone_res[-1].x[:])
        assert np.array_equal(c.icp_normal_equations(x), a.icp_normal_equations(x))
        kw2 = dict(KW, x=x + 0.001, max_iterations=3)
        same_results(c.icp_run(**kw2), a.icp_run(**kw2))
    for c in alone + batch:
        c.close()


def test_batch_of_one_and_of_300():
    from simpleicp_amd import _lib
    Xf, Xm = surface_pair(3000, 7)
    a, b = prepared(Xf, Xm, 300), prepared(Xf, Xm, 300)
    runs, _ = b.icp_run_batch([(b, KW)])
    same_results(runs[0].results, a.icp_run(**KW))
    a.close(); b.close()
    data = [surface_pair(1000, 200 + i % 5) for i in range(300)]
    ctxs = [prepared(Xf, Xm, 40 + (i % 7) * 30) for i, (Xf, Xm) in enumerate(data)]
    kws = [dict(KW, max_iterations=5 + i % 11) for i in range(300)]
    runs, fb = ctxs[0].icp_run_batch(list(zip(ctxs, kws)))
    assert fb == 0 and len(runs) == 300
    refs = {}
    for i, r in enumerate(runs):
        key = (i % 5, i % 7, i % 11)
        if key not in refs and len(refs) < 40:
            c = prepared(*data[i], 40 + (i % 7) * 30)
            refs[key] = c.icp_run(**kws[i])
            c.close()
        if key in refs:
            assert r.status == _lib.OK
            same_results(r.results, refs[key])
    for c in ctxs:
        c.close()


def test_batch_wide_refusals_launch_nothing():
    from simpleicp_amd import _lib
    Xf, Xm = surface_pair(2000, 3)
    a, b = prepared(Xf, Xm, 200), prepared(Xf, Xm, 200)
    a.icp_run(**KW)
    before = a.icp_state()
    with pytest.raises(_lib.BackendError, match="already in the batch") as ei:
        a.icp_run_batch([(a, KW), (b, KW), (a, KW)])
    assert ei.value.code == _lib.ERR_INVALID
    bare = _lib.Context(0)
    bare.upload(_lib.FIX, Xf)
    bare.upload(_lib.MOV, Xm)
    with pytest.raises(_lib.BackendError, match="sicp_icp_setup") as ei:
        a.icp_run_batch([(a, KW), (bare, KW)])
    assert ei.value.code == _lib.ERR_INVALID
    for u, v in zip(a.icp_state(), before):
        assert np.array_equal(u, v)
    with pytest.raises(_lib.BackendError):
        b.icp_state()                                            # b never ran: nothing was launched for it
    for c in (a, b, bare):
        c.close()


def test_back_to_back_same_slot_uploads_from_float32():
    from simpleicp_amd import _lib
    rng = np.random.default_rng(1)
    first = rng.normal(size=(300_000, 3)).astype(np.float32)
    second = rng.normal(size=(200_000, 3)).astype(np.float32)
    with _lib.Context(0) as ctx:
        ctx.upload_start(_lib.MOV, xyz=first)
        ctx.upload_start(_lib.MOV, xyz=second)
        ctx.upload_wait(_lib.MOV)
        assert ctx.size(_lib.MOV) == len(second)
        assert np.array_equal(ctx.download(_lib.MOV), second.astype(np.float64))


def test_synthetic_sample_against_oracle():
    """An independent reference for the batched loop: the CPU oracle's sicp_icp_run (tests/oracle_backend.py) on the same clouds,
    selection and normals, one member per EPT bucket; estimates to 1e-9, the same number of iterations."""
    from tests.oracle_backend import OracleContext
    from simpleicp_amd import _lib
    data = [surface_pair(n, 300 + i) for i, n in enumerate((3000, 6000, 12_000, 20_000))]
    Qs = (200, 450, 900, 2000)
    ctxs, orcs = [], []
    for (Xf, Xm), q in zip(data, Qs):
        c = prepared(Xf, Xm, q)
        sel = np.unique(np.round(np.linspace(0, len(Xf) - 1, q)).astype(np.int64))
        nv, pl = c.estimate_normals(_lib.FIX, sel, 8)
        o = OracleContext()
        o.upload(_lib.FIX, Xf)
        o.upload(_lib.MOV, Xm)
        o.icp_setup(sel, nv, pl)
        ctxs.append(c)
        orcs.append(o)
    runs, fb = ctxs[0].icp_run_batch([(c, KW) for c in ctxs])
    assert fb == 0
    for r, o in zip(runs, orcs):
        assert r.status == _lib.OK
        ref = o.icp_run(**KW)
        assert len(r.results) == len(ref)
        assert np.abs(np.array(r.results[-1].x[:]) - np.array(ref[-1].x[:])).max() < 1e-9
    for c in ctxs:
        c.close()


def test_member_with_exchange_is_refused():
    from simpleicp_amd import _lib
    Xf, Xm = surface_pair(2000, 4)
    a, b = prepared(Xf, Xm, 200), prepared(Xf, Xm, 200)
    b.set_exchange(lambda what, x, y, z, count: 1, 0, 2)          # (never called: nothing is launched)
    with pytest.raises(_lib.BackendError, match="exchange or communicator") as ei:
        a.icp_run_batch([(a, KW), (b, KW)])
    assert ei.value.code == _lib.ERR_INVALID
    with pytest.raises(_lib.BackendError):
        a.icp_state()                                           # a never ran either
    for c in (a, b):
        c.close()
