"""run_tensors and the device-cloud ABI on the GPU: every fixture equals run() bit for bit from float64 tensors, float32 inputs equal
run() on the widened data, strided views equal their contiguous copies, the C entries one by one (ingest, egress, device selection),
run()'s exceptions, untouched inputs, the stream rule, and device pairs inside run_batch."""
import numpy as np
import pytest
import torch

from conftest import GOLDEN_CASES, load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


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


def lone(Xf, Xm, **kw):
    """SimpleICP.run on copies of two (n, 3) float64 arrays: its return and its last_run_info."""
    from simpleicp_amd import PointCloud, SimpleICP
    icp = SimpleICP(verbose=False)
    icp.add_point_clouds(PointCloud(np.array(Xf, dtype=np.float64), columns=["x", "y", "z"]),
                         PointCloud(np.array(Xm, dtype=np.float64), columns=["x", "y", "z"]))
    return icp.run(**kw), icp.last_run_info


def assert_same(res, ref, info, dtype=torch.float64):
    """test_gpu_batch.assert_same on a result whose transformed cloud is a device tensor (compared after .cpu().numpy())."""
    H, X, rbp, resid = ref
    assert res.error is None
    assert np.array_equal(res.H, H)
    Xt = res.X_mov_transformed
    assert isinstance(Xt, torch.Tensor) and Xt.is_cuda and Xt.dtype == dtype and Xt.is_contiguous() and Xt.shape == X.shape
    assert np.array_equal(Xt.cpu().numpy(), X if dtype == torch.float64 else X.astype(np.float32))
    assert np.array_equal(res.residuals, resid)
    assert res.iterations == info["iterations"]
    for name in ("alpha1", "alpha2", "alpha3", "tx", "ty", "tz"):
        a, b = getattr(res.rbp, name), getattr(rbp, name)
        assert a.estimated_value == b.estimated_value and a.initial_value == b.initial_value
        assert np.array_equal(a.estimated_uncertainty, b.estimated_uncertainty, equal_nan=True)


def dev(X, dtype=torch.float64):
    return torch.tensor(np.asarray(X), dtype=dtype, device=DEV)


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_golden_f64_equals_run(name, clouds):
    from simpleicp_amd import run_tensors
    _, files, kw = load_golden(name)
    Xf, Xm = clouds(files[0]), clouds(files[1])
    ref, info = lone(Xf, Xm, **kw)
    res = run_tensors(dev(Xf), dev(Xm), **kw)
    assert res.path == "device"
    assert_same(res, ref, info)
    H, X_new, rbp, resid = res                               # unpacks like run()'s tuple
    assert H is res.H and X_new is res.X_mov_transformed and rbp is res.rbp and resid is res.residuals
    assert res.n_kept == len(resid) and np.isfinite(res.res_mean)


@pytest.mark.parametrize("name", ["dragon", "bunny", "webots"])
def test_float32_inputs_equal_run_on_widened_data(name, clouds):
    from simpleicp_amd import run_tensors
    _, files, kw = load_golden(name)
    Xf32, Xm32 = (dev(clouds(f), torch.float32) for f in files[:2])
    ref, info = lone(Xf32.double().cpu().numpy(), Xm32.double().cpu().numpy(), **kw)
    res = run_tensors(Xf32, Xm32, **kw)
    assert_same(res, ref, info, dtype=torch.float32)         # (f32 output = run()'s f64 output rounded to nearest)


def test_strided_views_equal_contiguous_copies():
    from simpleicp_amd import run_tensors
    Xf, Xm = surface_pair(40_000, 5)
    kw = dict(correspondences=700, max_overlap_distance=1.0)
    base = run_tensors(dev(Xf), dev(Xm), **kw)
    wide = torch.zeros((len(Xm), 6), dtype=torch.float64, device=DEV)
    wide[:, :3] = dev(Xm)
    cols = dev(Xm.T.copy())                                  # (3, n): .T is (n, 3) with strides (1, n)
    for view in (wide[:, :3], cols.T):
        assert not view.is_contiguous()
        r = run_tensors(dev(Xf), view, **kw)
        assert np.array_equal(r.H, base.H) and torch.equal(r.X_mov_transformed, base.X_mov_transformed)
        assert np.array_equal(r.residuals, base.residuals) and r.iterations == base.iterations
    every2 = dev(Xf)[::2]
    r = run_tensors(every2, dev(Xm), **kw)
    c = run_tensors(every2.contiguous(), dev(Xm), **kw)
    assert np.array_equal(r.H, c.H) and torch.equal(r.X_mov_transformed, c.X_mov_transformed)
    assert np.array_equal(r.residuals, c.residuals)
    f32 = dev(Xf, torch.float32)
    r = run_tensors(torch.cat([f32, f32], 1)[:, 3:], dev(Xm), **kw)           # a float32 feats[:, 3:6]-style view
    c = run_tensors(f32, dev(Xm), **kw)
    assert np.array_equal(r.H, c.H) and torch.equal(r.X_mov_transformed, c.X_mov_transformed)


def test_upload_strided_then_download_equals_input_widened():
    from simpleicp_amd import _lib
    rng = np.random.default_rng(1)
    with _lib.Context(0) as ctx:
        for n in (1, 7, 1000, 1025, 300_001):
            X = rng.normal(0, 50, (n, 3))
            for dtype, code in ((torch.float64, _lib.DT_F64), (torch.float32, _lib.DT_F32)):
                t = dev(X, dtype)
                wide = torch.zeros((n, 5), dtype=dtype, device=DEV)
                wide[:, 1:4] = t
                tr = dev(X.T.copy(), dtype).T
                for v in (t, wide[:, 1:4], tr):
                    ctx.upload_strided(_lib.FIX, v.data_ptr(), code, n, v.stride(0), v.stride(1))
                    assert np.array_equal(ctx.download(_lib.FIX), t.double().cpu().numpy()), (n, dtype, v.stride())
            # the slot's statistics are the plain upload's: both searches see the same cloud
            ctx.upload_strided(_lib.MOV, dev(X).data_ptr(), _lib.DT_F64, n, 3, 1)
            ctx.upload(_lib.FIX, X)
            q = rng.normal(0, 50, (64, 3))
            assert np.array_equal(ctx.knn(_lib.MOV, q)[0], ctx.knn(_lib.FIX, q)[0])


def test_upload_strided_refuses_host_memory_and_non_finite():
    from simpleicp_amd import _lib
    X = np.random.default_rng(2).normal(0, 1, (100, 3))
    with _lib.Context(0) as ctx:
        with pytest.raises(_lib.BackendError, match="not device memory"):
            ctx.upload_strided(_lib.FIX, X.ctypes.data, _lib.DT_F64, 100, 3, 1)
        X[17, 1] = np.nan
        with pytest.raises(_lib.BackendError) as host:
            ctx.upload(_lib.FIX, X)
        with pytest.raises(_lib.BackendError) as devr:
            ctx.upload_strided(_lib.FIX, dev(X).data_ptr(), _lib.DT_F64, 100, 3, 1)
        assert str(devr.value) == str(host.value) and devr.value.code == host.value.code
        assert ctx.size(_lib.FIX) == 0


def test_write_strided_f64_equals_transform_and_download():
    from simpleicp_amd import _lib
    rng = np.random.default_rng(4)
    H = _lib.params_to_H(np.array([0.01, -0.02, 0.3, 1.5, -2.0, 0.25]))
    with _lib.Context(0) as ctx:
        for n in (1, 255, 257, 100_003):
            X = rng.normal(0, 30, (n, 3))
            ctx.upload(_lib.MOV, X)
            out = torch.empty((n, 3), dtype=torch.float64, device=DEV)
            ctx.write_strided(_lib.MOV, H, out.data_ptr(), _lib.DT_F64, 3, 1)
            out32 = torch.empty((n, 3), dtype=torch.float32, device=DEV)
            ctx.write_strided(_lib.MOV, H, out32.data_ptr(), _lib.DT_F32, 3, 1)
            wide = torch.zeros((n, 7), dtype=torch.float64, device=DEV)
            ctx.write_strided(_lib.MOV, H, wide[:, 2:5].data_ptr(), _lib.DT_F64, 7, 1)
            assert np.array_equal(ctx.download(_lib.MOV), X)                 # the slot itself is not transformed
            ctx.transform(_lib.MOV, H)
            ref = ctx.download(_lib.MOV)
            assert np.array_equal(out.cpu().numpy(), ref)
            assert np.array_equal(out32.cpu().numpy(), ref.astype(np.float32))
            w = wide.cpu().numpy()
            assert np.array_equal(w[:, 2:5], ref) and not w[:, :2].any() and not w[:, 5:].any()


def test_select_n_device_picks_select_n_points_rows():
    from simpleicp_amd import PointCloud, _lib
    from simpleicp_amd.pointcloud import _ALL
    rng = np.random.default_rng(9)
    cases = [(1, 1, 1.0), (5, 10, 0.5), (1000, 10, 0.5), (4096, 4096, 0.3), (100_000, 1000, 0.01), (100_000, 1000, 0.999),
             (1_000_003, 10_000, 0.2), (2_000_000, 1000, None), (777, 50, 0.0)]
    cases += [(int(n), int(q), float(p)) for n, q, p in zip(rng.integers(1, 300_000, 25), rng.integers(1, 5000, 25), rng.random(25))]
    with _lib.Context(0) as ctx:
        for n, Q, p in cases:
            pc = PointCloud(np.zeros((n, 3)), columns=["x", "y", "z"])
            sel = torch.full((Q,), -7, dtype=torch.int64, device=DEV)
            if p is None:
                ref = pc.select_n_points(Q, _cur=_ALL)
                q = ctx.select_n_device(None, n, Q, sel.data_ptr())
            else:
                mask = rng.random(n) < p
                ref = pc.select_n_points(Q, _cur=np.flatnonzero(mask))
                q = ctx.select_n_device(dev(mask, torch.uint8).data_ptr(), n, Q, sel.data_ptr())
            got = sel.cpu().numpy()
            assert q == len(ref) and np.array_equal(got[:q], ref), (n, Q, p)
            assert (got[q:] == -7).all()


def test_run_exceptions_same_type_and_message():
    from simpleicp_amd import run_tensors
    Xf, Xm = surface_pair(20_000, 11)
    far = Xm + np.array([500.0, 0, 0])
    bad = Xf.copy()
    bad[123, 2] = np.nan
    for A, B, kw in ((Xf, far, {"max_overlap_distance": 1.0}), (Xf, Xm, {"min_planarity": 1.0}), (bad, Xm, {}), (Xf, bad, {})):
        with pytest.raises(Exception) as host:
            lone(A, B, correspondences=500, **kw)
        with pytest.raises(Exception) as devr:
            run_tensors(dev(A), dev(B), correspondences=500, **kw)
        assert type(devr.value) is type(host.value) and str(devr.value) == str(host.value), kw


def test_inputs_unchanged():
    from simpleicp_amd import run_tensors
    Xf, Xm = surface_pair(30_000, 12)
    A, B = dev(Xf), dev(Xm, torch.float32)
    a0, b0 = A.clone(), B.clone()
    run_tensors(A, B, correspondences=800, max_overlap_distance=2.0)
    assert torch.equal(A, a0) and torch.equal(B, b0)


def test_input_written_on_current_stream_just_before_the_call():
    """The stream rule: the library's stream waits for torch's current stream -- no synchronise in between."""
    from simpleicp_amd import run_tensors
    Xf, Xm = surface_pair(200_000, 13)
    ref, info = lone(Xf, Xm, correspondences=1000)
    src = dev(Xm)
    X = torch.full_like(src, 7.0)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(50_000_000)                    # (keeps the write below late)
        for _ in range(20):
            X.copy_(src * 2.0)
            X.mul_(0.5)
        res = run_tensors(dev(Xf), X, correspondences=1000)
    assert_same(res, ref, info)


def test_run_batch_mixes_device_and_host_pairs():
    from simpleicp_amd import run_batch, run_tensors
    pairs, kinds = [], []
    for i in range(6):
        Xf, Xm = surface_pair(20_000 + 3000 * i, 30 + i)
        if i % 3 == 0:
            pairs.append((dev(Xf), dev(Xm))); kinds.append("f64")
        elif i % 3 == 1:
            pairs.append((Xf, Xm)); kinds.append("host")
        else:
            pairs.append((dev(Xf, torch.float32), dev(Xm, torch.float32))); kinds.append("f32")
    per = [None, {"max_overlap_distance": 1.0}, {"correspondences": 300}, {"max_iterations": 5}, None, {"min_change": 0.1}]
    out = run_batch(pairs, per_pair=per, correspondences=600)
    for (A, B), kind, kw, res in zip(pairs, kinds, per, out):
        kw = {"correspondences": 600, **(kw or {})}
        assert res.error is None and res.path == "batched"
        if kind == "host":
            ref, info = lone(A, B, **kw)
            from test_gpu_batch import assert_same as host_same
            host_same(res, ref, info)
            assert isinstance(res.X_mov_transformed, np.ndarray)
        else:
            lone_dev = run_tensors(A, B, **kw)
            assert np.array_equal(res.H, lone_dev.H) and torch.equal(res.X_mov_transformed, lone_dev.X_mov_transformed)
            assert np.array_equal(res.residuals, lone_dev.residuals) and res.iterations == lone_dev.iterations
            if kind == "f64":
                ref, info = lone(A.cpu().numpy(), B.cpu().numpy(), **kw)
                assert_same(res, ref, info)
    again = run_batch(pairs, per_pair=per, correspondences=600, return_transformed=False)
    for res, first in zip(again, out):
        assert res.X_mov_transformed is None and np.array_equal(res.H, first.H)
    bad = run_batch([(dev(Xf), dev(Xm + np.array([500.0, 0, 0])))], max_overlap_distance=1.0)
    assert bad[0].error is not None and "do not overlap" in str(bad[0].error)


def test_one_million_points_q10000_equals_run():
    from simpleicp_amd import run_tensors
    Xf, Xm = surface_pair(1_300_000, 21)
    ref, info = lone(Xf, Xm, correspondences=10_000, max_overlap_distance=1.0)
    res = run_tensors(dev(Xf), dev(Xm), correspondences=10_000, max_overlap_distance=1.0)
    assert_same(res, ref, info)
