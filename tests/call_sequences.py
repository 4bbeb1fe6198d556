"""What SimpleICP.run and run_batch (one host pair) ASK of the backend, LOG and RETURN OR RAISE, case by case, on the stand-in
backends of the host tests.  TEST INFRASTRUCTURE ONLY.

oracle/record_call_sequences.py wrote tests/golden/call_sequences.json with ``record_all()`` on the commit before the options and
the preparation of run / run_batch / run_tensors were unified; tests/test_call_sequences.py replays every case and compares with
``==``.  A record holds names, strings and numbers only.  Floating-point results are rounded to 10 significant digits: a change in
what is called, in which order and with which arguments moves them grossly or not at all, and a record must not depend on the last
bits of another machine's LAPACK."""
import ctypes as C
import itertools
import logging
import re

import numpy as np

import eval_ref
import outlier_ref
import voxel_ref
from simpleicp_amd import _lib
from tests.helpers.batch_oracle import BatchOracleContext
from tests.oracle_backend import OracleContext

OPTION_NAMES = ("max_normal_angle", "voxel_size", "voxel_origin", "evaluate_distance", "outlier_neighbors", "outlier_std_ratio")
STAT_KEYS = ("n_candidates", "n_kept", "mean", "std", "threshold")


class _Answers:
    """The entry points of the voxel step, the outlier removal and the evaluation, answered by the numpy references."""

    def voxel_select(self, slot, voxel_size, origin=None, rows=None, keep_ptr=None):
        assert keep_ptr is None
        return voxel_ref.keep(self.cloud[slot][0], voxel_size, (0.0, 0.0, 0.0) if origin is None else tuple(origin), rows=rows)

    def outlier_statistical(self, slot, k, std_ratio, rows=None, mask_ptr=None, keep_ptr=None, mean_ptr=None):
        assert mask_ptr is None and keep_ptr is None and mean_ptr is None
        r = outlier_ref.statistical(self.cloud[slot][0], k, std_ratio, rows=rows)
        return r["keep"], r["d"], {key: r[key] for key in STAT_KEYS}

    def evaluate(self, query_slot, search_slot, H=None, max_distance=np.inf, rows=None):
        r = eval_ref.evaluate(self.cloud[query_slot][0], self.cloud[search_slot][0], H, max_distance, rows)
        return _lib.EvalRecord(r["n_queries"], r["n_inliers"], r["sums"][0], (C.c_double * 3)(*r["sums"][1:4]),
                               (C.c_double * 6)(*r["sums"][4:10]))


def _brief(v):
    """An argument as a name, a string or a number."""
    if v is None or isinstance(v, (bool, int, str)):
        return v
    if isinstance(v, float):
        return _num(v)
    if isinstance(v, np.ndarray):
        return f"array{v.shape}"
    if isinstance(v, (tuple, list)) and len(v) <= 6:
        return [_brief(e) for e in v]
    return type(v).__name__


def _traced(cls):
    """cls with every public method writing its name and its arguments into ``self.trace`` -- when the caller is the package,
    not the stand-in itself."""
    def wrap(name, f):
        def traced(self, *a, **k):
            depth = self.__dict__.get("_depth", 0)
            if depth == 0:
                self.__dict__.setdefault("trace", []).append([name, [_brief(v) for v in a], {key: _brief(v) for key, v in sorted(k.items())}])
            self.__dict__["_depth"] = depth + 1
            try:
                return f(self, *a, **k)
            finally:
                self.__dict__["_depth"] = depth
        return traced
    body = {}
    for name in dir(cls):
        f = getattr(cls, name)
        if not name.startswith("_") and callable(f):
            body[name] = wrap(name, f)
    return type("Traced" + cls.__name__, (cls,), body)


class _Full(_Answers, OracleContext):
    pass


class _FullBatch(_Answers, BatchOracleContext):
    pass


CONTEXTS = {"full": (_traced(_Full), _traced(_FullBatch)),
            "plain": (_traced(OracleContext), _traced(BatchOracleContext))}     # (no voxel step, no outlier removal, no evaluation)


def _num(v):
    v = float(v)
    return float(f"{v:.10g}") if np.isfinite(v) else str(v)          # ("nan" / "inf": strings compare equal, NaN does not)


def _nums(a):
    return [_num(v) for v in np.asarray(a, dtype=float).ravel()]


def clouds():
    """A fixed cloud of 400 points on a gently curved surface with 10 far-off points among its rows, and the movable cloud: the
    fixed one under a small rigid motion with the strip x > 7.5 cut off."""
    rng = np.random.default_rng(20)
    xy = rng.uniform(0.0, 10.0, (400, 2))
    X = np.column_stack((xy, 0.3 * np.sin(0.5 * xy[:, 0]) + 0.02 * xy[:, 1] ** 2))
    X[rng.choice(400, 10, replace=False), 2] += rng.uniform(4.0, 6.0, 10)
    a = 0.01
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    M = X[X[:, 0] <= 7.5] @ R.T + np.array([0.03, -0.02, 0.01])
    return np.ascontiguousarray(X), np.ascontiguousarray(M)


RUN = dict(correspondences=50, neighbors=10, max_iterations=4)
ON = dict(max_overlap_distance=0.5, outlier_neighbors=8, voxel_size=0.8, evaluate_distance=0.3)


def cases():
    """name -> dict(run=run()'s keywords, options=the six options, fix / mov = rows to select beforehand or None, backend)."""
    out = {}
    for bits in itertools.product((0, 1), repeat=4):
        on = {k: v for (k, v), b in zip(ON.items(), bits) if b}
        run = dict(RUN)
        if "max_overlap_distance" in on:
            run["max_overlap_distance"] = on.pop("max_overlap_distance")
        out["combo_" + "".join(map(str, bits))] = dict(run=run, options=on)
    everything = {k: v for k, v in ON.items() if k != "max_overlap_distance"}
    near = dict(RUN, max_overlap_distance=0.5)
    out["fixed_partial"] = dict(run=near, options=everything, fix=list(range(40, 330)))
    out["fixed_partial_plain"] = dict(run=dict(RUN), options={}, fix=list(range(40, 330)))
    out["movable_partial"] = dict(run=near, options=everything, mov=list(range(0, 300, 2)))
    out["movable_partial_plain"] = dict(run=dict(RUN), options={}, mov=list(range(0, 300, 2)))
    out["empty_overlap"] = dict(run=dict(RUN, max_overlap_distance=1e-9), options={})
    out["empty_overlap_everything"] = dict(run=dict(RUN, max_overlap_distance=1e-9), options=everything)
    out["empty_movable_selection"] = dict(run=near, options=everything, mov=[])
    out["empty_fixed_selection_overlap"] = dict(run=near, options={}, fix=[])
    out["empty_fixed_selection_outlier"] = dict(run=dict(RUN), options=dict(outlier_neighbors=8, voxel_size=0.8), fix=[])
    out["empty_fixed_selection_voxel"] = dict(run=dict(RUN), options=dict(voxel_size=0.8), fix=[])
    out["empty_fixed_selection_voxel_overlap"] = dict(run=near, options=dict(voxel_size=0.8), fix=[])
    out["too_many_outlier_neighbors"] = dict(run=dict(RUN), options=dict(outlier_neighbors=120), fix_rows=100)
    out["too_many_outlier_neighbors_bad_weights"] = dict(run=dict(RUN, distance_weights=-1.0), options=dict(outlier_neighbors=120),
                                                         fix_rows=100)
    out["bad_all_four"] = dict(run=dict(RUN), options=dict(max_normal_angle=120.0, voxel_size=-1.0, evaluate_distance=-1.0,
                                                           outlier_neighbors=1))
    out["bad_voxel_evaluate_outlier"] = dict(run=dict(RUN), options=dict(voxel_size=-1.0, evaluate_distance=-1.0, outlier_neighbors=1))
    out["bad_origin_outlier_ratio"] = dict(run=dict(RUN), options=dict(voxel_size=1.0, voxel_origin=(0.0, 0.0), outlier_neighbors=8,
                                                                       outlier_std_ratio=float("nan")))
    out["bad_evaluate_outlier"] = dict(run=dict(RUN), options=dict(evaluate_distance=-1.0, outlier_neighbors=1))
    out["bad_weights_bad_voxel"] = dict(run=dict(RUN, distance_weights=-1.0), options=dict(voxel_size=-1.0))
    out["bad_weights_count_bad_outlier"] = dict(run=dict(RUN, rbp_observation_weights=(0.0,) * 5), options=dict(outlier_neighbors=1))
    out["debug_dirpath_bad_voxel"] = dict(run=dict(RUN, debug_dirpath="DEBUG_DIR"), options=dict(voxel_size=-1.0), batch_only=True)
    out["unknown_keyword"] = dict(run=dict(RUN, correspondances=50), options=dict(voxel_size=-1.0), batch_only=True)
    out["unknown_keyword_in_pair"] = dict(run=dict(RUN), options={}, per_pair={"voxel_sise": 1.0, "outlier_neighbors": 1}, batch_only=True)
    out["options_in_pair"] = dict(run=near, options=dict(voxel_size=5.0, outlier_neighbors=8, outlier_std_ratio=3.0),
                                  per_pair=dict(voxel_size=0.8, outlier_std_ratio=1.0, evaluate_distance=0.3, correspondences=40),
                                  batch_only=True)
    out["normal_angle_without_backend"] = dict(run=near, options=dict(everything, max_normal_angle=45.0))
    out["plain_backend_voxel_evaluate"] = dict(run=dict(RUN), options=dict(voxel_size=0.8, evaluate_distance=0.3), backend="plain")
    out["plain_backend_outlier_evaluate"] = dict(run=dict(RUN), options=dict(outlier_neighbors=8, evaluate_distance=0.3), backend="plain")
    out["plain_backend_nothing"] = dict(run=near, options={}, backend="plain")
    return out


def _pair(case):
    from simpleicp_amd import PointCloud
    X, M = clouds()
    if "fix_rows" in case:
        X = X[:case["fix_rows"]]
    pc1, pc2 = PointCloud(X, columns=["x", "y", "z"]), PointCloud(M, columns=["x", "y", "z"])
    for pc, rows in ((pc1, case.get("fix")), (pc2, case.get("mov"))):
        if rows is not None:
            pc.select_by_indices(rows)
    return pc1, pc2


def _logged(fn):
    """(what fn returns or None, (type name, message) of what it raises or None, the package's log lines, run times masked)."""
    lines = []
    handler = logging.Handler()
    handler.emit = lambda r: lines.append(re.sub(r"\d+\.\d{3} seconds", "T seconds", r.getMessage()))
    log = logging.getLogger("simpleicp_amd")
    old = log.level
    log.addHandler(handler)
    log.setLevel(logging.INFO)
    out = raised = None
    try:
        out = fn()
    except Exception as e:                                   # noqa: BLE001 (the record is which exception, with which words)
        raised = [type(e).__name__, str(e)]
    finally:
        log.removeHandler(handler)
        log.setLevel(old)
    return out, raised, lines


def _evaluation(ev):
    return None if ev is None else dict(n_queries=int(ev.n_queries), n_inliers=int(ev.n_inliers), fitness=_num(ev.fitness),
                                        inlier_rmse=_num(ev.inlier_rmse), information=_nums(ev.information))


def _outlier(st):
    return None if st is None else {key: _num(st[key]) for key in STAT_KEYS}


def _rbp(rbp):
    return [[_num(getattr(rbp, n).estimated_value), _num(getattr(rbp, n).estimated_uncertainty), _num(getattr(rbp, n).initial_value)]
            for n in ("alpha1", "alpha2", "alpha3", "tx", "ty", "tz")]


def record_run(case, monkeypatch):
    """One case through SimpleICP.run."""
    from simpleicp_amd import SimpleICP, backend
    ctx = CONTEXTS[case.get("backend", "full")][0]()
    monkeypatch.setattr(backend, "get_context", lambda: ctx)
    pc1, pc2 = _pair(case)
    icp = SimpleICP(verbose=False)
    icp.add_point_clouds(pc1, pc2)
    for name, value in case["options"].items():
        assert name in OPTION_NAMES
        setattr(icp, name, value)
    out, raised, lines = _logged(lambda: icp.run(**case["run"]))
    rec = dict(raised=raised, log=lines, calls=ctx.__dict__.get("trace", []), fixed_selected=[int(i) for i in pc1.idx_selected],
               movable_selected=int(pc2.num_selected_points))
    if out is not None:
        H, X_new, rbp, residuals = out
        info = icp.last_run_info
        rec["result"] = dict(H=_nums(H), X_new=[len(X_new), _num(np.sum(X_new))], rbp=_rbp(rbp), residuals=_nums(residuals),
                             iterations=info["iterations"], stats=[[int(n), _num(m), _num(s)] for n, m, s in info["stats"]],
                             info_keys=sorted(k for k in info if k != "seconds"), outlier=_outlier(info.get("outlier")),
                             evaluation=_evaluation(info.get("evaluation")), evaluation_attribute=_evaluation(icp.evaluation))
    return rec


def record_batch(case, monkeypatch):
    """One case as the only pair of a run_batch call: options call-wide, case['per_pair'] as the pair's own dict."""
    import simpleicp_amd
    from simpleicp_amd import backend
    made = []

    def factory(device):
        made.append(CONTEXTS[case.get("backend", "full")][1]())
        return made[-1]
    backend.reset_batch_contexts()
    monkeypatch.setattr(backend, "batch_context_factory", factory)
    try:
        pc1, pc2 = _pair(case)
        per_pair = None if "per_pair" not in case else [case["per_pair"]]
        out, raised, lines = _logged(lambda: simpleicp_amd.run_batch([(pc1, pc2)], per_pair=per_pair, **case["options"], **case["run"]))
        rec = dict(raised=raised, log=lines, calls=[c.__dict__.get("trace", []) for c in made],
                   inputs_untouched=bool(pc1.num_selected_points == (len(case["fix"]) if case.get("fix") is not None else pc1.num_points)))
        if out is not None:
            r, = out
            rec["result"] = dict(error=None if r.error is None else [type(r.error).__name__, str(r.error)], path=r.path,
                                 iterations=r.iterations, n_kept=int(r.n_kept), res_mean=_num(r.res_mean), res_std=_num(r.res_std),
                                 outlier=_outlier(r.outlier), evaluation=_evaluation(r.evaluation))
            if r.error is None:
                rec["result"].update(H=_nums(r.H), X_new=[len(r.X_mov_transformed), _num(np.sum(r.X_mov_transformed))], rbp=_rbp(r.rbp),
                                     residuals=_nums(r.residuals))
        return rec
    finally:
        backend.reset_batch_contexts()


SHARDED_CASES = ("combo_0000", "combo_1000", "combo_0100", "combo_0010", "combo_0001", "combo_0111", "fixed_partial_plain",
                 "movable_partial_plain", "empty_overlap", "empty_movable_selection", "bad_all_four", "too_many_outlier_neighbors")


def record_sharded_run(case, monkeypatch):
    """One case through SimpleICP.run as rank 1 of a torch.distributed job of two: run()'s own sharded branch (the refusals, the
    movable cloud's shard, what it attaches and detaches), with the job itself -- simpleicp_amd.dist's group and exchange -- replaced
    by its answers."""
    from simpleicp_amd import dist
    events = []
    monkeypatch.setattr(dist, "is_distributed", lambda: True)
    monkeypatch.setattr(dist, "rank_world", lambda: (1, 2))
    monkeypatch.setattr(dist, "agree", lambda flag, group=None: bool(flag))
    monkeypatch.setattr(dist, "attach", lambda ctx, **k: events.append(["attach", {key: _brief(v) for key, v in sorted(k.items())}]) or "callback")
    monkeypatch.setattr(dist, "detach", lambda ctx: events.append(["detach"]))
    monkeypatch.setattr(dist, "forget", lambda ctx: events.append(["forget"]))
    for cls in CONTEXTS[case.get("backend", "full")]:
        monkeypatch.setattr(cls, "exchange_info", lambda self: {"form": "records_allgather", "count": 4}, raising=False)
    rec = record_run(case, monkeypatch)
    rec["job"] = events
    return rec


def record_all_sharded(monkeypatch_factory):
    """monkeypatch_factory(): a context manager that yields a fresh monkeypatch and undoes it."""
    out = {}
    for name in SHARDED_CASES:
        with monkeypatch_factory() as monkeypatch:
            out[name] = record_sharded_run(cases()[name], monkeypatch)
    return out


def record_all(monkeypatch):
    out = {}
    for name, case in cases().items():
        out[name] = {"run_batch": record_batch(case, monkeypatch)}
        if not case.get("batch_only"):
            out[name]["run"] = record_run(case, monkeypatch)
    return out
