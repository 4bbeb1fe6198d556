"""Other data than the nine committed fixtures: the UNMODIFIED reference and this package's SimpleICP.run (its host logic on
the oracle-backed stand-in context, tests/oracle_backend.py) register the same seeded random cloud pairs with the same keyword
arguments -- partial overlap, fixed and observed parameters, an automatic weight, few iterations.  The reference's own normals
are handed over (its LAPACK signs are arbitrary and its result depends on them), as the fixtures do.  Then:
the same iteration count, the same correspondence counts up to a cKDTree tie pick, H to the reference's solver tolerance.
The reference's runs are stored in tests/golden/live/runs.npz (oracle/record_reference.py, which runs these CASES).  CPU only."""
import numpy as np
import pandas as pd
import pytest

import oracle_backend
from conftest import GOLDEN
from live_data import cloud_pair as _pair

CASES = [
    (0, {}),
    (1, {"max_overlap_distance": 0.6, "correspondences": 400}),
    (2, {"correspondences": 300, "neighbors": 6, "min_planarity": 0.45, "distance_weights": None, "max_iterations": 5}),
    (3, {"rbp_observed_values": (0.0, 0.0, 1.0, 0.05, 0.0, 0.0), "rbp_observation_weights": (np.inf, 0.0, 20.0, 100.0, 0.0, 0.0)}),
    (4, {"min_change": 0.01, "max_iterations": 9, "correspondences": 700}),
]


@pytest.mark.parametrize("seed,kwargs", CASES)
def test_reference_and_mirror_agree_on_fresh_data(seed, kwargs, monkeypatch):
    from simpleicp_amd import PointCloud, SimpleICP
    P, M = _pair(seed)
    g = np.load(GOLDEN / "live" / "runs.npz", allow_pickle=False)
    H0, X0 = g[f"s{seed}_H"], g[f"s{seed}_X"].astype(np.float64)   # (X stored in float32: 1e-6 here, compared to 1e-4)
    n_res0, std_res0 = g[f"s{seed}_res"]
    rows_a, stopped_a = (int(v) for v in g[f"s{seed}_rows_stopped"])

    oracle_backend.install(monkeypatch)
    b_fix, b_mov = PointCloud(P, columns=["x", "y", "z"]), PointCloud(M.copy(), columns=["x", "y", "z"])
    sel = g[f"s{seed}_sel"]                                    # the rows the reference estimated normals for
    for c, col in zip(("nx", "ny", "nz", "planarity"), g[f"s{seed}_normals"]):
        v = np.full(len(P), np.nan, np.float32)
        v[sel] = col
        b_fix[c] = pd.arrays.SparseArray(v)
    b = SimpleICP(verbose=False)
    b.add_point_clouds(b_fix, b_mov)
    with _Capture("simpleicp_amd") as log_b:
        H1, X1, rbp1, res1 = b.run(**kwargs)

    assert np.array_equal(b_fix.idx_selected, sel)             # overlap pre-pass + sub-sampling: the same rows
    assert np.abs(H1 - H0).max() < 2e-6, np.abs(H1 - H0).max()
    assert abs(len(res1) - n_res0) <= 2 and abs(res1.std() - std_res0) < 1e-5
    assert np.abs(X1 - X0).max() < 1e-4 and np.array_equal(X1, b_mov.X)
    x0 = g[f"s{seed}_x"]
    x1 = np.array(rbp1.get_parameter_attributes_as_list("estimated_value"))
    ow = np.array(kwargs.get("rbp_observation_weights", (0.,) * 6), float)
    assert np.abs(x1 - x0).max() < 2e-6 and np.array_equal(x1[~np.isfinite(ow)], x0[~np.isfinite(ow)])
    s0 = g[f"s{seed}_s"]
    s1 = np.array(rbp1.get_parameter_attributes_as_list("estimated_uncertainty"))
    free = np.isfinite(ow)
    assert np.allclose(s1[free], s0[free], rtol=5e-3) and np.all(np.isnan(s1[~free])) and np.all(np.isnan(s0[~free]))
    # iteration count: one table row per iteration (simpleicp.py:275-280), except the converging one (it breaks before its row)
    stopped_b = any(m.startswith("Convergence criteria fulfilled") for m in log_b)
    assert rows_a == _rows(log_b) > 0 and bool(stopped_a) == stopped_b
    assert b.last_run_info["iterations"] == _rows(log_b) + int(stopped_b)


def _rows(records):
    import re
    return sum(1 for m in records if re.match(r"^\s*\d+ \|", m))


class _Capture:
    """Collects the INFO messages of one package's loggers for the duration of a run."""

    def __init__(self, name):
        import logging
        self.log, self.records = logging.getLogger(name), []
        self.handler = logging.Handler()
        self.handler.emit = lambda r: self.records.append(r.getMessage())

    def __enter__(self):
        import logging
        self.old = self.log.level
        self.log.setLevel(logging.INFO)
        self.log.addHandler(self.handler)
        return self.records

    def __exit__(self, *exc):
        self.log.removeHandler(self.handler)
        self.log.setLevel(self.old)
