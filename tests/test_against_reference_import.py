"""The host-side mirror against the UNMODIFIED reference package: everything the mirror does WITHOUT the device -- the math
helpers, the PointCloud selection bookkeeping, the RigidBodyParameters schema, the argument checks and their messages, the
public surface of the operator classes -- is compared call by call on seeded inputs.  The reference's answers to exactly these
calls are stored under tests/golden/reference_calls.{npz,json} (oracle/record_reference.py, run where the reference is, with
`lmfit` replaced by the 40-line stand-in of oracle/shim that make_golden.py uses too); the calls are replayed here on the
mirror.  CPU only."""
import dataclasses
import inspect
import json

import numpy as np
import pytest

from conftest import GOLDEN

ARG_CHECKS = [
    {"distance_weights": 0}, {"distance_weights": -1.5}, {"rbp_observed_values": (0, 0, 0)},
    {"rbp_observation_weights": (0,) * 5}, {"rbp_observation_weights": (0, 0, -1, 0, 0, 0)},
    {"rbp_observation_weights": (np.inf,) * 6},
]


@pytest.fixture(scope="module")
def ref():
    """What the reference answered (arrays, and the strings / names / signatures)."""
    arr = np.load(GOLDEN / "reference_calls.npz", allow_pickle=False)
    js = json.loads((GOLDEN / "reference_calls.json").read_text())
    return dict(arr={k: arr[k] for k in arr.files}, **js)


def _decode_default(d):
    """oracle/record_reference.py::encode_default, inverted."""
    if isinstance(d, dict):
        if "empty" in d:
            return inspect.Parameter.empty
        if "inf" in d:
            return float("inf") * d["inf"]
        return tuple(_decode_default(x) for x in d["tuple"])
    return d


def test_mathutils_call_by_call(ref):
    from simpleicp_amd import mathutils as mine
    a_ = ref["arr"]
    rng = np.random.default_rng(0)
    for i in range(200):
        a = rng.uniform(-1.5, 1.5, 3)
        R0, R1 = a_["math_R"][i], mine.euler_angles_to_rotation_matrix(*a)
        assert np.abs(R0 - R1).max() <= 2.3e-16                             # np.cos on a scalar vs libm: an ulp at most
        assert np.allclose(mine.rotation_matrix_to_euler_angles(R1), a, atol=1e-14)
        assert np.allclose(a_["math_eul"][i], mine.rotation_matrix_to_euler_angles(R0), atol=1e-15)
        assert np.array_equal(a_["math_lin"][i], mine.euler_angles_to_linearized_rotation_matrix(*a))
        t = rng.normal(size=3)
        assert np.array_equal(a_["math_hom"][i], mine.create_homogeneous_transformation_matrix(R0, t))
    X = rng.normal(size=(50, 3))
    Xh0, Xh1 = a_["math_Xh"].copy(), mine.euler_coord_to_homogeneous_coord(X)
    assert np.array_equal(Xh0, Xh1)
    Xh0[:, 3] = rng.uniform(0.5, 2.0, 50)
    assert np.array_equal(a_["math_Xe"], mine.homogeneous_coord_to_euler_coord(Xh0))


def test_pointcloud_selection_bookkeeping_call_by_call(ref):
    """pointcloud.py:51-147: the same sequence of host-side calls leaves the reference's state (its selection after every call)."""
    from simpleicp_amd import PointCloud as Mine
    rng = np.random.default_rng(1)
    for n in (1, 7, 1000, 20_011):
        X = rng.normal(size=(n, 3))
        b = Mine(X, columns=["x", "y", "z"])
        masks, counts = ref["arr"][f"pc_masks_{n}"], ref["arr"][f"pc_counts_{n}"]
        state = iter(range(len(counts)))

        def same():
            i = next(state)
            idx = np.flatnonzero(np.unpackbits(masks[i], count=n))
            assert b.num_points == n and b.num_selected_points == counts[i]
            assert np.array_equal(b.idx_selected, idx)
            assert np.array_equal(b.X, X) and np.array_equal(b.X_selected, X[idx])
            for j, c in enumerate("xyz"):
                assert np.array_equal(getattr(b, c), X[:, j])
                assert np.array_equal(getattr(b, c + "_selected"), X[idx, j])
            assert b["selected"].dtype == bool
        same()
        for m in (n + 5, max(1, n // 2), max(1, n // 3), 5, 1):           # select_n_points narrows the CURRENT selection
            b.select_n_points(m)
            same()
        b.select_all_points()
        pick = rng.choice(n, max(1, n // 4), replace=False)
        b.select_by_indices(pick)
        same()
        b.select_by_indices(pick[: len(pick) // 2])
        same()
        b.idx_selected = np.sort(pick)
        same()
        b.unselect_all_points()
        same()
        b.select_n_points(3)                                               # nothing selected: nothing to narrow
        same()
        assert next(state, None) is None
    from simpleicp_amd import PointCloudException
    with pytest.raises(PointCloudException) as e1:
        Mine(np.zeros((3, 2)), columns=["x", "y"])
    assert str(e1.value) == ref["pointcloud_exceptions"][0]
    with pytest.raises(PointCloudException) as e1:                         # pointcloud.py:158-159, before any search
        Mine(np.zeros((3, 3)), columns=["x", "y", "z"]).select_in_range(np.zeros((4, 2)), 1.0)
    assert str(e1.value) == ref["pointcloud_exceptions"][1]


def test_rigid_body_parameters_schema_and_H(ref):
    from simpleicp_amd import Parameter as MyP, RigidBodyParameters as MyR
    assert ref["rbp_fields"] == [f.name for f in dataclasses.fields(MyR)]
    assert ref["parameter_fields"] == [f.name for f in dataclasses.fields(MyP)]
    rng = np.random.default_rng(2)
    b = MyR()
    for i, attr in enumerate(("initial_value", "observed_value", "observation_weight", "estimated_value", "estimated_uncertainty")):
        v = list(rng.uniform(-0.3, 0.3, 6))
        b.set_parameter_attributes_from_list(attr, v)
        assert list(ref["arr"]["rbp_lists"][i]) == b.get_parameter_attributes_as_list(attr)
    assert np.abs(ref["arr"]["rbp_H"] - b.H).max() <= 2.3e-16
    for i, name in enumerate(("alpha1", "alpha2", "alpha3", "tx", "ty", "tz")):
        q = getattr(b, name)
        for j, prop in enumerate(("initial_value_scaled", "observed_value_scaled", "estimated_value_scaled", "estimated_uncertainty_scaled")):
            assert ref["arr"]["rbp_scaled"][i, j] == getattr(q, prop)
        assert ref["arr"]["rbp_scale_for_logging"][i] == q.scale_for_logging


@pytest.mark.parametrize("kwargs", ARG_CHECKS)
def test_argument_checks_raise_the_reference_s_messages(ref, kwargs):
    """simpleicp.py:327-353: raises before any work is done (here: before a device is asked for), with the reference's text."""
    from simpleicp_amd import PointCloud as MineP, SimpleICP as Mine, SimpleICPException
    X = np.random.default_rng(3).normal(size=(50, 3))
    b = Mine(verbose=False)
    b.add_point_clouds(MineP(X, columns=["x", "y", "z"]), MineP(X + 0.01, columns=["x", "y", "z"]))
    with pytest.raises(SimpleICPException) as e1:
        b.run(**kwargs)
    assert str(e1.value) == ref["argument_check_messages"][ARG_CHECKS.index(kwargs)]


def test_public_surface_of_every_mirrored_class(ref):
    """Same public methods / properties, same parameter names and defaults."""
    from simpleicp_amd import PointCloud, SimpleICP
    from simpleicp_amd.corrpts import CorrPts
    from simpleicp_amd.optimization import SimpleICPOptimization
    mine_by_name = {"PointCloud": PointCloud, "SimpleICP": SimpleICP, "CorrPts": CorrPts, "SimpleICPOptimization": SimpleICPOptimization}
    assert sorted(ref["public_surface"]) == sorted(mine_by_name)
    for cname, theirs in ref["public_surface"].items():
        mine = mine_by_name[cname]
        for n, t in theirs["members"].items():
            assert hasattr(mine, n), (cname, n)
            m = inspect.getattr_static(mine, n)
            if t["kind"] == "property":
                assert isinstance(m, property), (cname, n)
            elif t["kind"] == "callable":
                sm = inspect.signature(getattr(mine, n))
                tp = [(pn, _decode_default(d)) for pn, d in t["params"]]
                mp = [(p.name, p.default) for p in sm.parameters.values() if not p.name.startswith("_")]
                assert [x[0] for x in tp] == [x[0] for x in mp], (cname, n, tp, mp)
                for (pn, d0), (_, d1) in zip(tp, mp):
                    same = (d0 is d1) or (d0 == d1) or (isinstance(d0, float) and isinstance(d1, float) and np.isinf(d0) and np.isinf(d1))
                    assert same, (cname, n, pn, d0, d1)
        if theirs["init"] is not None:
            assert theirs["init"] == list(inspect.signature(mine.__init__).parameters), cname
    assert set(ref["package_names"]) >= {"SimpleICP", "PointCloud", "RigidBodyParameters"}
    import simpleicp_amd
    for n in ("SimpleICP", "PointCloud", "RigidBodyParameters"):
        assert hasattr(simpleicp_amd, n)
