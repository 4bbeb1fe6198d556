"""tests/operator_flow.py::reference_loop on other data than the nine fixtures: the committed fixture generator
(oracle/make_golden.py: the unmodified reference with recording wrappers around its CorrPts / SimpleICPOptimization methods),
pointed at seeded random cloud pairs, recorded tests/golden/live/loop_<seed>.npz (oracle/record_reference.py), and the
reference's loop is replayed with the mirror classes (on the oracle-backed stand-in context) against those per-stage dumps --
picks, bit-equal distances, rows after each rejection, estimate -- exactly as the GPU tests do against the committed fixtures.
CPU only."""
from pathlib import Path

import numpy as np
import pytest

import operator_flow as flow
import oracle_backend
from conftest import GOLDEN
from live_data import cloud_pair as _pair


@pytest.mark.parametrize("seed,kwargs", [
    (0, {}),
    (1, {"max_overlap_distance": 0.6, "correspondences": 400}),
    (3, {"rbp_observed_values": (0.0, 0.0, 1.0, 0.05, 0.0, 0.0), "rbp_observation_weights": (np.inf, 0.0, 20.0, 100.0, 0.0, 0.0)}),
    (5, {"correspondences": 2500, "neighbors": 8, "distance_weights": None, "max_iterations": 4}),
])
def test_reference_loop_replayed_on_fresh_data(seed, kwargs, monkeypatch):
    P, M = _pair(seed)
    data = {"fix.xyz": P, "mov.xyz": M}
    g = np.load(GOLDEN / "live" / f"loop_{seed}.npz", allow_pickle=False)
    assert str(g["kwargs"]) == repr(kwargs)                  # the recording is this case's
    assert int(g["iterations"]) >= 2
    monkeypatch.setattr(flow, "load_golden", lambda name: (g, ["fix.xyz", "mov.xyz"], dict(kwargs)))
    oracle_backend.install(monkeypatch)
    flow.reference_loop("live", lambda f: data[Path(f).name])
