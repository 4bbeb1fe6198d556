"""Record what the UNMODIFIED reference answers on the seeded inputs of the CPU tests that compare against it, so that those
tests run without the reference:

    python oracle/record_reference.py [--out DIR]      (default: tests/golden; needs the reference, like make_golden.py)

  reference_calls.npz / .json   tests/test_against_reference_import.py: math helpers, PointCloud selection bookkeeping,
                                RigidBodyParameters, the argument checks' messages, the public surface of the mirrored classes
  live/loop_<seed>.npz          tests/test_live_operator_loop.py: make_golden.run_case on live_data.cloud_pair(seed)
  live/runs.npz                 tests/test_live_reference_runs.py: SimpleICP.run on live_data.cloud_pair(seed)

The call sequences and seeds below are the tests' own; the tests replay them on this package and compare.
"""
import argparse
import dataclasses
import inspect
import json
import logging
import re
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import make_golden as mg  # noqa: E402  (puts the reference and the lmfit stand-in on sys.path)
import simpleicp as ref  # noqa: E402
from simpleicp import mathutils, optimization, pointcloud, simpleicp as driver  # noqa: E402
from simpleicp.corrpts import CorrPts  # noqa: E402
from simpleicp.optimization import SimpleICPOptimization  # noqa: E402
from live_data import cloud_pair  # noqa: E402

# tests/test_live_operator_loop.py and tests/test_live_reference_runs.py parametrise over these (seed, kwargs)
LOOP_CASES = [
    (0, {}),
    (1, {"max_overlap_distance": 0.6, "correspondences": 400}),
    (3, {"rbp_observed_values": (0.0, 0.0, 1.0, 0.05, 0.0, 0.0), "rbp_observation_weights": (np.inf, 0.0, 20.0, 100.0, 0.0, 0.0)}),
    (5, {"correspondences": 2500, "neighbors": 8, "distance_weights": None, "max_iterations": 4}),
]
RUN_CASES = [
    (0, {}),
    (1, {"max_overlap_distance": 0.6, "correspondences": 400}),
    (2, {"correspondences": 300, "neighbors": 6, "min_planarity": 0.45, "distance_weights": None, "max_iterations": 5}),
    (3, {"rbp_observed_values": (0.0, 0.0, 1.0, 0.05, 0.0, 0.0), "rbp_observation_weights": (np.inf, 0.0, 20.0, 100.0, 0.0, 0.0)}),
    (4, {"min_change": 0.01, "max_iterations": 9, "correspondences": 700}),
]
ARG_CHECKS = [
    {"distance_weights": 0}, {"distance_weights": -1.5}, {"rbp_observed_values": (0, 0, 0)},
    {"rbp_observation_weights": (0,) * 5}, {"rbp_observation_weights": (0, 0, -1, 0, 0, 0)},
    {"rbp_observation_weights": (np.inf,) * 6},
]
PC_SIZES = (1, 7, 1000, 20_011)


def encode_default(d):
    """A signature default as JSON (tests/test_against_reference_import.py decodes it)."""
    if d is inspect.Parameter.empty:
        return {"empty": True}
    if isinstance(d, float) and np.isinf(d):
        return {"inf": 1 if d > 0 else -1}
    if isinstance(d, tuple):
        return {"tuple": [encode_default(x) for x in d]}
    if d is None or isinstance(d, (bool, int, float, str)):
        return d
    raise TypeError(f"no JSON form for the default {d!r}")


def mathutils_calls(arr):
    rng = np.random.default_rng(0)
    R, eul, lin, hom = [], [], [], []
    for _ in range(200):
        a = rng.uniform(-1.5, 1.5, 3)
        R0 = mathutils.euler_angles_to_rotation_matrix(*a)
        R.append(R0)
        eul.append(mathutils.rotation_matrix_to_euler_angles(R0))
        lin.append(mathutils.euler_angles_to_linearized_rotation_matrix(*a))
        t = rng.normal(size=3)
        hom.append(mathutils.create_homogeneous_transformation_matrix(R0, t))
    X = rng.normal(size=(50, 3))
    Xh = mathutils.euler_coord_to_homogeneous_coord(X)
    arr["math_Xh"] = Xh.copy()
    Xh[:, 3] = rng.uniform(0.5, 2.0, 50)
    arr["math_Xe"] = mathutils.homogeneous_coord_to_euler_coord(Xh)
    arr["math_R"], arr["math_eul"], arr["math_lin"], arr["math_hom"] = map(np.array, (R, eul, lin, hom))


def pointcloud_calls(arr, js):
    """One row per state the test compares: the selection mask (packed) and num_selected_points."""
    rng = np.random.default_rng(1)
    for n in PC_SIZES:
        X = rng.normal(size=(n, 3))
        a = ref.PointCloud(X, columns=["x", "y", "z"])
        masks, counts = [], []

        def state():
            idx = np.asarray(a.idx_selected)
            mask = np.zeros(n, bool)
            mask[idx] = True
            assert np.array_equal(np.flatnonzero(mask), idx) and a.num_points == n
            assert np.array_equal(a.X, X) and np.array_equal(a.X_selected, X[idx]) and a["selected"].dtype == bool
            for i, c in enumerate("xyz"):
                assert np.array_equal(getattr(a, c), X[:, i]) and np.array_equal(getattr(a, c + "_selected"), X[idx, i])
            masks.append(np.packbits(mask))
            counts.append(a.num_selected_points)
        state()
        for m in (n + 5, max(1, n // 2), max(1, n // 3), 5, 1):
            a.select_n_points(m)
            state()
        a.select_all_points()
        pick = rng.choice(n, max(1, n // 4), replace=False)
        a.select_by_indices(pick)
        state()
        a.select_by_indices(pick[: len(pick) // 2])
        state()
        a.idx_selected = np.sort(pick)
        state()
        a.unselect_all_points()
        state()
        a.select_n_points(3)
        state()
        arr[f"pc_masks_{n}"], arr[f"pc_counts_{n}"] = np.array(masks), np.array(counts, np.int64)
    msgs = []
    try:
        ref.PointCloud(np.zeros((3, 2)), columns=["x", "y"])
    except pointcloud.PointCloudException as e:
        msgs.append(str(e))
    try:
        ref.PointCloud(np.zeros((3, 3)), columns=["x", "y", "z"]).select_in_range(np.zeros((4, 2)), 1.0)
    except pointcloud.PointCloudException as e:
        msgs.append(str(e))
    assert len(msgs) == 2
    js["pointcloud_exceptions"] = msgs


def rbp_calls(arr, js):
    js["rbp_fields"] = [f.name for f in dataclasses.fields(optimization.RigidBodyParameters)]
    js["parameter_fields"] = [f.name for f in dataclasses.fields(optimization.Parameter)]
    rng = np.random.default_rng(2)
    a = optimization.RigidBodyParameters()
    lists = []
    for attr in ("initial_value", "observed_value", "observation_weight", "estimated_value", "estimated_uncertainty"):
        a.set_parameter_attributes_from_list(attr, list(rng.uniform(-0.3, 0.3, 6)))
        lists.append(a.get_parameter_attributes_as_list(attr))
    arr["rbp_lists"], arr["rbp_H"] = np.array(lists), np.array(a.H)
    props = ("initial_value_scaled", "observed_value_scaled", "estimated_value_scaled", "estimated_uncertainty_scaled")
    arr["rbp_scaled"] = np.array([[getattr(getattr(a, p), q) for q in props] for p in ("alpha1", "alpha2", "alpha3", "tx", "ty", "tz")])
    arr["rbp_scale_for_logging"] = np.array([getattr(a, p).scale_for_logging for p in ("alpha1", "alpha2", "alpha3", "tx", "ty", "tz")])


def argument_check_messages(js):
    X = np.random.default_rng(3).normal(size=(50, 3))
    msgs = []
    for kwargs in ARG_CHECKS:
        a = ref.SimpleICP(verbose=False)
        a.add_point_clouds(ref.PointCloud(X, columns=["x", "y", "z"]), ref.PointCloud(X + 0.01, columns=["x", "y", "z"]))
        try:
            a.run(**kwargs)
        except driver.SimpleICPException as e:
            msgs.append(str(e))
        else:
            raise AssertionError(f"no exception for {kwargs}")
    js["argument_check_messages"] = msgs


def public_surface(js):
    import pandas as pd
    out = {}
    for cls in (ref.PointCloud, ref.SimpleICP, CorrPts, SimpleICPOptimization):
        base = set(dir(pd.DataFrame)) if issubclass(cls, pd.DataFrame) else set()
        members = {}
        for n in vars(cls):
            if n.startswith("_") or n in base:
                continue
            t = inspect.getattr_static(cls, n)
            if isinstance(t, property):
                members[n] = {"kind": "property"}
            elif callable(t) or isinstance(t, staticmethod):
                sig = inspect.signature(getattr(cls, n))
                members[n] = {"kind": "callable", "params": [[p.name, encode_default(p.default)] for p in sig.parameters.values()
                                                             if not p.name.startswith("_")]}
            else:
                members[n] = {"kind": "other"}
        init = None if issubclass(cls, pd.DataFrame) else list(inspect.signature(cls.__init__).parameters)
        out[cls.__name__] = {"members": members, "init": init}
    js["public_surface"] = out
    js["package_names"] = sorted(n for n in ref.__dict__ if not n.startswith("_"))


def live_loops(out):
    """make_golden.run_case on the live pairs: the per-stage dumps tests/operator_flow.py::reference_loop replays."""
    (out / "live").mkdir(parents=True, exist_ok=True)
    for seed, kwargs in LOOP_CASES:
        P, M = cloud_pair(seed)
        data = {"fix.xyz": P, "mov.xyz": M}
        mg.GOLD, mg.store_cloud = out / "live", (lambda name: data[name])
        mg.run_case(f"loop_{seed}", "fix.xyz", "mov.xyz", kwargs)


class _Capture:
    def __init__(self, name):
        self.log, self.records = logging.getLogger(name), []
        self.handler = logging.Handler()
        self.handler.emit = lambda r: self.records.append(r.getMessage())

    def __enter__(self):
        self.old = self.log.level
        self.log.setLevel(logging.INFO)
        self.log.addHandler(self.handler)
        return self.records

    def __exit__(self, *exc):
        self.log.removeHandler(self.handler)
        self.log.setLevel(self.old)


def live_runs(out):
    """SimpleICP.run on the live pairs: the rows it selected and its normals there (handed to the mirror), and what it returned."""
    arr = {}
    for seed, kwargs in RUN_CASES:
        P, M = cloud_pair(seed)
        a_fix, a_mov = ref.PointCloud(P, columns=["x", "y", "z"]), ref.PointCloud(M.copy(), columns=["x", "y", "z"])
        a = ref.SimpleICP(verbose=False)
        a.add_point_clouds(a_fix, a_mov)
        with _Capture("simpleicp") as log:
            H, X, rbp, res = a.run(**kwargs)
        sel = np.asarray(a_fix.idx_selected)
        arr[f"s{seed}_sel"] = sel
        arr[f"s{seed}_normals"] = np.stack([a_fix[c].to_numpy()[sel].astype(np.float32) for c in ("nx", "ny", "nz", "planarity")])
        arr[f"s{seed}_H"] = H
        arr[f"s{seed}_X"] = X.astype(np.float32)                    # compared to 1e-4: float32 keeps 1e-6 at these magnitudes
        arr[f"s{seed}_res"] = np.array([len(res), np.std(res)])
        arr[f"s{seed}_x"] = np.array(rbp.get_parameter_attributes_as_list("estimated_value"))
        arr[f"s{seed}_s"] = np.array(rbp.get_parameter_attributes_as_list("estimated_uncertainty"))
        rows = sum(1 for m in log if re.match(r"^\s*\d+ \|", m))
        stopped = any(m.startswith("Convergence criteria fulfilled") for m in log)
        arr[f"s{seed}_rows_stopped"] = np.array([rows, int(stopped)])
    np.savez_compressed(out / "live" / "runs.npz", **arr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=ROOT / "tests" / "golden")
    out = ap.parse_args().out
    out.mkdir(parents=True, exist_ok=True)
    arr, js = {}, {}
    mathutils_calls(arr)
    pointcloud_calls(arr, js)
    rbp_calls(arr, js)
    argument_check_messages(js)
    public_surface(js)
    np.savez_compressed(out / "reference_calls.npz", **arr)
    (out / "reference_calls.json").write_text(json.dumps(js, indent=1, sort_keys=True) + "\n")
    live_loops(out)
    live_runs(out)
    print(f"wrote {out / 'reference_calls.npz'}, {out / 'reference_calls.json'}, {out / 'live'}")


if __name__ == "__main__":
    main()
