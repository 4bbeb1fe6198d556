"""Every option at once on every road: SimpleICP.run, run_tensors, run_batch with a host pair and run_batch with a device pair
give the same bits when the overlap pre-pass, the outlier removal, the voxel step, the rejection by the angle between normals and
the evaluation are all switched on together.  The tests of each feature switch on one option; this one is about how they combine."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KW = dict(correspondences=200, neighbors=10, max_iterations=30, max_overlap_distance=0.5)
OPTIONS = dict(outlier_neighbors=8, outlier_std_ratio=2.0, voxel_size=0.4, voxel_origin=(0.05, -0.1, 0.02), max_normal_angle=45.0,
               evaluate_distance=0.3)
STAT_KEYS = ("n_candidates", "n_kept", "mean", "std", "threshold")


def dev(X):
    return torch.tensor(np.asarray(X), dtype=torch.float64, device=DEV)


@pytest.fixture(scope="module")
def pair():
    """3000 points on a gently curved surface plus 30 far-off points; the movable cloud is the surface under a small rigid motion
    with the strip x > 4 cut off."""
    rng = np.random.default_rng(41)
    half = 8.5
    xy = rng.uniform(-half, half, (3000, 2))
    S = np.column_stack((xy, 2 * np.sin(xy[:, 0] / 4) * np.cos(xy[:, 1] / 6) + rng.normal(0, 0.005, 3000)))
    far = np.column_stack((rng.uniform(-half, 4.0, (30, 2)), rng.uniform(3.5, 6.0, 30)))
    Xf = np.vstack((S, far))[rng.permutation(3030)]
    c, s = np.cos(0.01), np.sin(0.01)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    Xm = (S[S[:, 0] <= 4.0] + rng.normal(0, 0.005, (int((S[:, 0] <= 4.0).sum()), 3))) @ R.T + np.array([0.06, -0.04, 0.03])
    return np.ascontiguousarray(Xf), np.ascontiguousarray(Xm)


def lone(Xf, Xm, options, **kw):
    """SimpleICP.run on copies of the two arrays with the options as attributes, as a record like a BatchResult's."""
    from simpleicp_amd import PointCloud, SimpleICP
    icp = SimpleICP(verbose=False)
    icp.add_point_clouds(PointCloud(np.array(Xf), columns=["x", "y", "z"]), PointCloud(np.array(Xm), columns=["x", "y", "z"]))
    for name, value in options.items():
        setattr(icp, name, value)
    H, X, rbp, residuals = icp.run(**kw)
    info = icp.last_run_info
    return dict(H=H, X=X, rbp=rbp, residuals=residuals, iterations=info["iterations"], outlier=info.get("outlier"),
                evaluation=info.get("evaluation"))


def of_result(r):
    assert r.error is None
    X = r.X_mov_transformed
    return dict(H=r.H, X=X.cpu().numpy() if isinstance(X, torch.Tensor) else X, rbp=r.rbp, residuals=r.residuals,
                iterations=r.iterations, outlier=r.outlier, evaluation=r.evaluation)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_statistics(a, b, what, bitwise=True):
    """The outlier statistics a and b (None: the step was off).  bitwise False: between a host pair and a device pair behind a finite
    overlap bound.  There the host road hands the candidates to the step as a list of rows and the device road as a mask over all
    points, so the pairwise trees behind mean and std add the same <= 3030 terms in another order (tests/test_gpu_outlier.py,
    test_with_the_overlap_pass_the_selection_is_the_masked_reference): the counts are equal, the three sums agree to
    3030 * 2^-53 < 1e-12 relative."""
    print(what, "outlier statistics", a, b)
    if a is None or b is None:
        assert a is None and b is None, what
        return
    assert [a[k] for k in STAT_KEYS[:2]] == [b[k] for k in STAT_KEYS[:2]], what
    fa, fb = np.array([a[k] for k in STAT_KEYS[2:]]), np.array([b[k] for k in STAT_KEYS[2:]])
    assert np.array_equal(bits(fa), bits(fb)) if bitwise else np.all(np.abs(fa - fb) <= 1e-12 * np.abs(fb)), what


def same(got, ref, what, statistics_bitwise=True):
    print(what, "iterations", got["iterations"], ref["iterations"], "evaluation", got["evaluation"], ref["evaluation"])
    assert np.array_equal(bits(got["H"]), bits(ref["H"])), what
    assert np.array_equal(bits(got["residuals"]), bits(ref["residuals"])), what
    assert np.array_equal(bits(got["X"]), bits(ref["X"])), what
    for name in ("alpha1", "alpha2", "alpha3", "tx", "ty", "tz"):
        a, b = getattr(got["rbp"], name), getattr(ref["rbp"], name)
        assert np.array_equal(bits([a.estimated_value, a.initial_value]), bits([b.estimated_value, b.initial_value])), (what, name)
        assert np.array_equal(bits([a.estimated_uncertainty]), bits([b.estimated_uncertainty])), (what, name)
    assert got["iterations"] == ref["iterations"], what
    same_statistics(got["outlier"], ref["outlier"], what, statistics_bitwise)
    a, b = got["evaluation"], ref["evaluation"]
    assert (a.n_queries, a.n_inliers) == (b.n_queries, b.n_inliers), what
    assert np.array_equal(bits((a.sum_d2,) + a.sum_p + a.sum_pp), bits((b.sum_d2,) + b.sum_p + b.sum_pp)), what


def test_every_option_at_once_on_every_road(pair):
    from simpleicp_amd import backend, run_batch, run_tensors
    Xf, Xm = pair
    ref = lone(Xf, Xm, OPTIONS, **KW)
    # every step took something away, and enough is left for the correspondences
    st, ev = ref["outlier"], ref["evaluation"]
    assert 0 < st["n_kept"] < st["n_candidates"] < len(Xf) and ref["iterations"] >= 2
    assert 0 < ev.n_inliers < ev.n_queries == len(Xf)
    alone = of_result(run_tensors(dev(Xf), dev(Xm), **OPTIONS, **KW))
    same(alone, ref, "run_tensors", statistics_bitwise=False)
    try:
        out = run_batch([(Xf, Xm), (dev(Xf), dev(Xm))], **OPTIONS, **KW)
        assert [r.path for r in out] == ["fallback", "fallback"]          # (the normal-angle option takes a member out of the batched loop)
        same(of_result(out[0]), ref, "run_batch host pair")
        same(of_result(out[1]), ref, "run_batch device pair", statistics_bitwise=False)
        same_statistics(out[1].outlier, alone["outlier"], "the two device roads")
    finally:
        backend.reset_batch_contexts()


def test_four_members_with_options_of_their_own_equal_their_lone_runs(pair):
    from simpleicp_amd import backend, run_batch
    Xf, Xm = pair
    options = {k: v for k, v in OPTIONS.items() if k != "max_normal_angle"}
    per_pair = [None, {"voxel_size": 0.6}, {"outlier_neighbors": 16}, {"voxel_size": 0.3, "outlier_neighbors": 5}]
    refs = [lone(Xf, Xm, dict(options, **(p or {})), **KW) for p in per_pair]
    assert len({r["H"].tobytes() for r in refs}) == 4                      # (the members' options matter)
    try:
        out = run_batch([(Xf, Xm), (Xf, Xm), (dev(Xf), dev(Xm)), (Xf, Xm)], per_pair=per_pair, **options, **KW)
        assert [r.path for r in out] == ["batched"] * 4
        for i, (r, ref) in enumerate(zip(out, refs)):
            same(of_result(r), ref, f"member {i}", statistics_bitwise=i != 2)              # (member 2 is the device pair)
    finally:
        backend.reset_batch_contexts()
