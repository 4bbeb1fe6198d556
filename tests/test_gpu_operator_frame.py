"""The frame the stand-alone operators share ("An operator call's frame"): the counter words and the staging buffers of
one context serve call after call, and a selection of rows gives the same answer from host and from device memory.  What the
operators compute is checked against the references in their own files; here every comparison is call against call, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def test_five_operators_after_one_another_equal_fresh_contexts():
    """sicp_fpfh, sicp_feature_match, sicp_outlier_radius, sicp_voxel_select, sicp_ransac_triplets on one context, every array in
    host memory (so every output is staged), then the same calls in reverse order: each gives the bytes it gives on a context
    that has done nothing else."""
    from simpleicp_amd import _lib
    rng = np.random.default_rng(300)
    X = rng.uniform(0, 1, (300, 3))
    N = rng.standard_normal((300, 3))
    N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(np.float32)
    q = rng.uniform(0, 100, (70, 33)).astype(np.float32)
    t = rng.uniform(0, 100, (130, 33)).astype(np.float32)
    src = rng.uniform(-1, 1, (9, 3))
    dst = src[:, [1, 2, 0]] + [0.5, -0.25, 2.0] + rng.normal(0, 1e-3, (9, 3))       # a rotation, a shift and some noise
    dst[7] += 0.4                                                                  # ... and one wrong match
    tri = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8], [2, 2, 5], [8, 0, 4]], dtype=np.int32)   # (the fourth is void)

    def fpfh(c):
        F, cnt, st = c.fpfh(_lib.FIX, N, 8, 0.4, (0.5, 0.5, 3.0), want_counts=True)
        return F.tobytes(), cnt.tobytes(), st.as_dict()

    def match(c):
        idx, d2, st = c.feature_match(q, t)
        return idx.tobytes(), d2.tobytes(), st.as_dict()

    def radius(c):
        keep, cnt, kept = c.outlier_radius(_lib.FIX, 0.15, 4)
        return keep.tobytes(), cnt.tobytes(), kept

    def voxel(c):
        return c.voxel_select(_lib.FIX, 0.2).tobytes()

    def ransac(c):
        poses, inl, st = c.ransac_triplets(src, dst, tri, 0.05, 0.5)
        return poses.tobytes(), inl.tobytes(), st.as_dict()

    ops = (fpfh, match, radius, voxel, ransac)
    want = {}
    for op in ops:
        with _lib.Context(0) as fresh:
            fresh.upload(_lib.FIX, X)
            want[op] = op(fresh)
    # (the data makes every counter word matter: pairs counted, points kept and dropped, a best hypothesis, a void one)
    assert want[fpfh][2]["n_pairs"] > 0 and 0 < want[radius][2] < 300 and 0 < np.frombuffer(want[voxel], np.uint8).sum() < 300
    assert want[ransac][2]["n_void"] == 1 and want[ransac][2]["best_inliers"] >= 3
    with _lib.Context(0) as c:
        c.upload(_lib.FIX, X)
        for op in ops + ops[::-1]:
            assert op(c) == want[op], op.__name__


def test_selected_rows_from_host_and_from_device_memory():
    """sicp_evaluate, sicp_select_in_range and sicp_estimate_normals take sel_idx from host and from device memory: 65 rows (a wave
    and one: the padded tail of the query columns is in use) of a 500-point cloud, the same answer both ways."""
    from simpleicp_amd import _lib
    rng = np.random.default_rng(500)
    Xq, Xs = rng.uniform(-1, 1, (500, 3)), rng.uniform(-1, 1, (400, 3))
    rows = rng.permutation(500)[:65].astype(np.int64)
    rows_d = torch.tensor(rows, device=DEV)
    L = _lib.load()
    with _lib.Context(0) as c:
        c.upload(_lib.FIX, Xq)
        c.upload(_lib.MOV, Xs)
        a, b = c.evaluate(_lib.FIX, _lib.MOV, None, 0.2, rows), c.evaluate(_lib.FIX, _lib.MOV, None, 0.2, rows_d)
        assert bytes(a) == bytes(b) and a.n_queries == 65 and 0 < a.n_inliers < 65

        in_range = c.select_in_range(_lib.FIX, _lib.MOV, rows, None, 0.2)
        out = np.full(65, 7, np.uint8)
        rc = L.sicp_select_in_range(c._h, _lib.FIX, _lib.MOV, C.c_void_p(rows_d.data_ptr()), 65, None, 0.2, _lib._ptr(out))
        assert rc == _lib.OK, L.sicp_last_error()
        assert np.array_equal(out, in_range.view(np.uint8)) and int(out.sum()) == a.n_inliers

        nv, pl, nn = c.estimate_normals(_lib.FIX, rows, 8, want_nn=True)
        nv_d, pl_d, nn_d = np.full((65, 3), 7, np.float32), np.full(65, 7, np.float32), np.full((65, 8), -7, np.int64)
        rc = L.sicp_estimate_normals(c._h, _lib.FIX, C.c_void_p(rows_d.data_ptr()), 65, 8, _lib._ptr(nv_d), _lib._ptr(pl_d),
                                     _lib._ptr(nn_d))
        assert rc == _lib.OK, L.sicp_last_error()
        assert nv_d.tobytes() == nv.tobytes() and pl_d.tobytes() == pl.tobytes() and np.array_equal(nn_d, nn)
        assert np.array_equal(nn[:, 0], rows)                         # (every selected point is its own nearest neighbour)
    assert np.array_equal(rows_d.cpu().numpy(), rows)                 # the selection itself is left alone
