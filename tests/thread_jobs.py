"""Jobs, a schedule and the overlap bookkeeping of the threaded tests (tests/test_gpu_threads.py, tests/test_threads_host.py,
tests/helpers/threads_first_use.py).  TEST INFRASTRUCTURE ONLY.

A JOB is a function of a `Runner` and a seed that returns a dict of numpy arrays.  It makes every library call through
``run.call(tag, fn, *args)``: the runner looks at the stop event first (after the first failure anywhere nothing more is started on
the GPU), then notes ``perf_counter()`` at entry and at exit.  ``run.meet()`` is where the threads of a round wait for each other
once their preparation is done, so that the calls a round is about start side by side; alone (the serial leg) it does nothing.
A job creates its contexts itself, never looks at ``os.environ`` and hands every array over as host memory.

What a job should return comes from ``expected(job, seed)``: the CPU oracle (oracle/orc.py) and the numpy references of the
operators' own test files, computed before any thread starts.  Every key of it has a KIND: "bits" (indices, masks, counts,
descriptors, eigenvalues, distances, messages: the bytes must be equal) or an absolute bound (estimates: 1e-9; normals and
planarity: the float32 bounds of tests/test_gpu_kernels.py).  A key the expectation does not name is compared between the serial
and the threaded leg only -- bit for bit, like every other key."""
import hashlib
import re
import threading
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent

N_RUN = 20_000                 # points of either cloud of an icp_run job
N_NORMALS = 30_000
RING_SMALL, RING_TWO_CHUNKS = 5_000, (1 << 19) + 1        # DL_CH = 1 << 19 (sicp_clouds.cpp): one point into the second chunk
# iterations per sicp_icp_run and calls per job: Q = 1 000 is the single-workgroup tail with the next match launched early
# (iterations - 1 tickets), 2 049 the three-launch path, 16 385 the one-launch forms that meet at grid barriers
RUNS = {1000: dict(iterations=9, reps=24), 2049: dict(iterations=6, reps=4), 16385: dict(iterations=6, reps=2)}
PRELAUNCHED = {1000: RUNS[1000]["iterations"] - 1, 2049: 0, 16385: 0}      # (tests/test_gpu_prelaunch.py::test_query_counts)
CHURN_REPS = 12
REFUSAL_REPS = 200


class Stopped(Exception):
    """Another thread failed: this one starts nothing more."""


# ---- the runner, the schedule, the overlaps --------------------------------------------------------------------------------------------
class Runner:
    """What a job calls the library through.  records: [(thread, job, tag, entry, exit)]."""

    def __init__(self, thread=0, job="", stop=None, records=None, meet=None):
        self.thread, self.job, self.stop, self._meet = thread, job, stop, meet
        self.records = [] if records is None else records

    def call(self, tag, fn, *args, **kwargs):
        if self.stop is not None and self.stop.is_set():
            raise Stopped(tag)
        t0 = time.perf_counter()
        try:
            return fn(*args, **kwargs)
        finally:
            self.records.append((self.thread, self.job, tag, t0, time.perf_counter()))

    def meet(self):
        if self._meet is not None:
            self._meet()


def overlapping(records, first, second):
    """The pairs of records (a, b) of different threads, first(a) and second(b) true, whose intervals share wall time."""
    A, B = [r for r in records if first(r)], [r for r in records if second(r)]
    return [(a, b) for a in A for b in B if a[0] != b[0] and max(a[3], b[3]) < min(a[4], b[4])]


def tagged(*tags):
    return lambda r: r[2] in tags


def run_schedule(schedule, jobs, watchdog_s, rounds_meet=True):
    """schedule[t][r] = (job name, seed) of thread t in round r; jobs[name](runner, seed) -> result.  Every thread is a daemon;
    all start on one barrier and meet again at every round's beginning and (through Runner.meet) once inside every round.  The
    first exception sets the stop event, breaks the barriers and is raised here; so is a thread still alive after watchdog_s.
    Returns (results[t][r], records)."""
    T, R = len(schedule), len(schedule[0])
    assert all(len(row) == R for row in schedule)
    stop, errors, records = threading.Event(), [], []
    start = threading.Barrier(T)
    inner = [threading.Barrier(T) for _ in range(R)]
    outer = [threading.Barrier(T) for _ in range(R)]
    results = [[None] * R for _ in range(T)]
    deadline = time.monotonic() + watchdog_s

    def wait(barrier):
        try:
            barrier.wait(timeout=max(0.0, deadline - time.monotonic()))
        except threading.BrokenBarrierError:
            if not stop.is_set():                            # (nobody gave up: the wait itself ran out of time)
                errors.append((-1, TimeoutError(f"a thread did not reach a meeting point within {watchdog_s:.0f} s")))
                give_up()
            raise Stopped("a barrier was broken") from None

    def give_up():
        stop.set()
        for b in [start] + inner + outer:
            b.abort()

    def worker(t):
        try:
            wait(start)
            for r, (name, seed) in enumerate(schedule[t]):
                wait(outer[r])
                met = []

                def meet(r=r, met=met):
                    if not met:                              # (once per round, whatever the job does)
                        met.append(1)
                        wait(inner[r])
                run = Runner(t, name, stop, records, meet if rounds_meet else None)
                results[t][r] = jobs[name](run, seed)
                run.meet()                                   # (a job without a meeting point of its own)
        except Stopped:
            pass
        except BaseException as e:                           # noqa: BLE001 (collected, raised by the main thread)
            errors.append((t, e))
            give_up()

    threads = [threading.Thread(target=worker, args=(t,), daemon=True, name=f"sicp-job-{t}") for t in range(T)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(max(0.0, deadline - time.monotonic()))
    hung = [th.name for th in threads if th.is_alive()]
    if hung:
        give_up()
        raise TimeoutError(f"{hung} still running after {watchdog_s:.0f} s: nothing more is started")
    if errors:
        t, e = errors[0]
        if isinstance(e, TimeoutError):
            raise e
        err = RuntimeError(f"thread {t}: {type(e).__name__}: {e}")
        last = max((r for r in records if r[0] == t), key=lambda r: r[4], default=None)
        # (the call that failed, and the other threads' calls that shared wall time with it)
        err.beside = [] if last is None else [last] + [r for r in records if r[0] != t and max(r[3], last[3]) < min(r[4], last[4])]
        raise err from e
    return results, records


# ---- how long a threaded run may take ---------------------------------------------------------------------------------------------------
def barrier_spin_bound():
    """The polls after which a waiting block of a grid barrier gives up (sicp_lanes.h, grid_barrier)."""
    text = (ROOT / "simpleicp_amd" / "csrc" / "sicp_lanes.h").read_text()
    (shift,) = re.findall(r"\+\+spins > \(1L << (\d+)\)", text)
    return 1 << int(shift)


def barrier_launches(schedule):
    """Launches that meet at a grid barrier: k_hsel_all and k_lm_all<true> per iteration of a Q = 16 385 run, and the lone first
    iteration the job runs before."""
    per_job = 2 * (1 + RUNS[16385]["iterations"] * RUNS[16385]["reps"])
    return per_job * sum(name == "run16385" for row in schedule for name, _ in row)


def ticket_waiting_runs(schedule):
    """Runs whose matches are launched early and poll the tail's ticket (k_grid_nn_wait): the repeated runs of a Q = 1 000 job."""
    return RUNS[1000]["reps"] * sum(name == "run1000" for row in schedule for name, _ in row)


# A poll is s_sleep 4 (256 clocks) and one agent-scope load: sicp_lanes.h puts the whole bound at "about two seconds", a microsecond
# a poll; twice that is allowed here.  A launch whose barrier cannot meet waits the bound out ONCE (GridBar::error ends its other
# phases within 1 024 polls) and the call returns SICP_ERR_HIP -- the worst case is every barrier launch of the schedule doing so
# one after the other.  The early matches' ticket wait has the same bound (sicp_grid_nn_one.inc: `++spins > (1L << 21)`, the one
# that did expire before the runs took turns): the first one to give up sets the run's stop flag and the error word, every launch
# queued behind it leaves at once, so a RUN waits the bound out once at the most -- the runs are counted, not their launches.
# The allowance is for everything else: 12 contexts' worth of uploads, a few hundred short kernels and two 12 MiB clouds over the
# link per ring job, which a loaded machine does in seconds.
POLL_SECONDS = 2e-6
ALLOWANCE_SECONDS = 60.0


def watchdog_seconds(schedule):
    return barrier_spin_bound() * POLL_SECONDS * (barrier_launches(schedule) + ticket_waiting_runs(schedule)) + ALLOWANCE_SECONDS


# ---- data -------------------------------------------------------------------------------------------------------------------------------
def surface_pair(n, seed):
    """A fixed cloud on a wavy surface and the movable one: noisy, 20 mrad and a few decimetres off (tests/test_gpu_prelaunch.py)."""
    rng = np.random.default_rng(1000 + seed)
    half = np.sqrt(n / 10.0) / 2
    xy = rng.uniform(-half, half, (n, 2))
    z = 2 * np.sin(xy[:, 0] / 4) * np.cos(xy[:, 1] / 6) + rng.normal(0, 0.005, n)
    Xf = np.column_stack((xy, z))
    c, s = np.cos(0.02), np.sin(0.02)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    Xm = (Xf + rng.normal(0, 0.005, Xf.shape)) @ R.T + np.array((0.3, -0.2, 0.1))
    return np.ascontiguousarray(Xf), np.ascontiguousarray(Xm)


def ring_cloud(n, seed):
    """n points whose every coordinate says which seed and which row it belongs to."""
    i = np.arange(n, dtype=np.float64)
    return np.ascontiguousarray(np.column_stack((i + 0.25 * seed, -i - 1000.0 * (seed + 1), (seed + 1) * 1e6 + np.sqrt(i))))


_cache, _cache_lock = {}, threading.Lock()


def cached(key, make):
    with _cache_lock:
        if key not in _cache:
            _cache[key] = make()
        return _cache[key]


def run_inputs(Q, seed):
    """Clouds, the selected rows and THE ORACLE'S normals of them (an input of the job: what follows is bit-comparable)."""
    def make():
        from oracle import orc
        Xf, Xm = surface_pair(N_RUN, seed)
        sel = np.unique(np.round(np.linspace(0, N_RUN - 1, Q)).astype(np.int64))
        assert len(sel) == Q
        nn, _ = orc.knn(Xf, Xf[sel], k=8)
        nv, pl = orc.normals(Xf, nn)
        return Xf, Xm, sel, np.ascontiguousarray(nv, dtype=np.float32), np.ascontiguousarray(pl, dtype=np.float32)
    return cached(("run", Q, seed), make)


def operator_inputs(seed):
    def make():
        import fuzz_operators as fo
        from fuzz_sequence import _small_H, _surface
        rng = np.random.default_rng(5000 + seed)
        F = _surface(rng, 777)
        M = np.ascontiguousarray((F[rng.permutation(777)[:600]] + rng.normal(0, 0.01, (600, 3))))
        N = rng.standard_normal((600, 3))
        N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(np.float32)
        N[17] = np.nan
        src, dst = fo.matched_rows(rng, 300)
        big_src, big_dst = fo.matched_rows(rng, 1025)
        q, t = rng.uniform(0, 100, (300, 33)).astype(np.float32), rng.uniform(0, 100, (257, 33)).astype(np.float32)
        q[5] = np.nan
        return dict(F=np.ascontiguousarray(F), M=M, N=N, H=_small_H(rng), src=src, dst=dst, big_src=big_src, big_dst=big_dst, q=q, t=t,
                    tri=rng.integers(0, 300, (256, 3), dtype=np.int32), start=fo.start_poses(rng, 5))
    return cached(("operators", seed), make)


# ---- jobs -------------------------------------------------------------------------------------------------------------------------------
def _context(run, lean=False):
    from simpleicp_amd import _lib
    ctx = run.call("ctx_create", _lib.Context, 0)
    if lean:
        run.call("ctx_lean", ctx.make_lean)
    return ctx


def _records(res):
    return np.frombuffer(b"".join(bytes(r) for r in res), dtype=np.uint8).copy()


def _xs(res):
    return np.array([list(r.x) for r in res], dtype=np.float64).reshape(len(res), 6)


def job_run(Q):
    it, reps = RUNS[Q]["iterations"], RUNS[Q]["reps"]

    def job(run, seed):
        from simpleicp_amd import _lib
        Xf, Xm, sel, nv, pl = run_inputs(Q, seed)
        z = np.zeros(6)
        ctx = _context(run)
        try:
            run.call("upload", ctx.upload, _lib.FIX, Xf)
            run.call("upload", ctx.upload, _lib.MOV, Xm)
            # one iteration alone: its correspondences, distances and verdicts are the oracle's to the bit
            run.call("icp_setup", ctx.icp_setup, sel, nv, pl)
            first = run.call(f"icp_run_first:{Q}", ctx.icp_run, z, z, z, 0.3, 1.0, 1, 0.0)
            idx, dist, keep, _ = run.call("icp_state", ctx.icp_state)
            out = dict(first_idx=idx, first_dist=dist, first_keep=keep.view(np.uint8),
                       first_counts=np.array([first[0].n_planar, first[0].n_kept], np.int64),
                       first_median_mad=np.array([first[0].median, first[0].mad]))
            run.meet()
            runs = []
            for _ in range(reps):
                run.call("icp_setup", ctx.icp_setup, sel, nv, pl)
                res = run.call(f"icp_run:{Q}", ctx.icp_run, z, z, z, 0.3, 1.0, it, 0.0)
                runs.append((_records(res), run.call("chain_info", ctx.chain_info)["last_run"]))
            same = all(np.array_equal(r[0], runs[0][0]) and r[1] == runs[0][1] for r in runs)
            idx, dist, keep, resid = run.call("icp_state", ctx.icp_state)
            out.update(x=_xs(res), records=runs[0][0], repeats_agree=np.array([same]), prelaunched=np.array([runs[0][1]], np.int64),
                       last_idx=idx, last_dist=dist, last_keep=keep.view(np.uint8), last_resid=resid)
            return out
        finally:
            ctx.close()
    return job


def expected_run(Q, seed):
    from oracle import orc
    Xf, Xm, sel, nv, pl = run_inputs(Q, seed)
    z, x, xs = np.zeros(6), np.zeros(6), []
    for i in range(RUNS[Q]["iterations"]):
        o = orc.icp_iteration(Xm, Xf[sel], nv, pl, x, x, 1.0, z, z, 0.3)
        if i == 0:
            first = o
        x = o["x"]
        xs.append(x)
    return {"first_idx": ("bits", np.asarray(first["nn"], np.int64)), "first_dist": ("bits", np.asarray(first["dist"], np.float64)),
            "first_keep": ("bits", np.asarray(first["keep"]).astype(np.uint8)),
            "first_counts": ("bits", np.array([np.count_nonzero(pl >= np.float32(0.3)), first["n"]], np.int64)),
            "first_median_mad": ("bits", np.array([first["median"], first["mad"]])),
            "x": (1e-9, np.array(xs)), "repeats_agree": ("bits", np.array([True])),
            "prelaunched": ("bits", np.array([PRELAUNCHED[Q]], np.int64))}


def job_normals(run, seed):
    from simpleicp_amd import _lib
    P = surface_pair(N_NORMALS, 40 + seed)[0]
    ctx = _context(run)
    try:
        run.call("upload", ctx.upload, _lib.FIX, P)
        run.meet()
        nv, pl, nn = run.call("estimate_normals", ctx.estimate_normals, _lib.FIX, np.arange(N_NORMALS), 10, True)
        return dict(nn=nn, normals=nv, planarity=pl)
    finally:
        ctx.close()


def expected_normals(seed):
    from oracle import orc
    P = surface_pair(N_NORMALS, 40 + seed)[0]
    nn, _ = orc.knn(P, P, k=10)
    nv, pl = orc.normals(P, nn)
    # (one float32 ulp for the float64 sqrt and division: tests/test_gpu_kernels.py, __graft_entry__.smoke)
    return {"nn": ("bits", np.asarray(nn, np.int64)), "normals": (2e-7, nv), "planarity": (2e-6, pl)}


def _stats(st):
    return np.array(list(st.as_dict().values()), dtype=np.float64)


def job_operators(run, seed):
    """The stand-alone operators one after the other on one context, at the sizes of tests/fuzz_operators.py, every array host
    memory: voxel, both outlier filters, FPFH, ISS keypoints, evaluation, descriptor match, RANSAC, refit, robust, consistency."""
    from simpleicp_amd import _lib
    d = operator_inputs(seed)
    ctx = _context(run)
    try:
        run.call("upload", ctx.upload, _lib.FIX, d["F"])
        run.call("upload", ctx.upload, _lib.MOV, d["M"])
        run.meet()
        out = {}
        out["voxel_keep"] = run.call("voxel_select", ctx.voxel_select, _lib.FIX, 0.3, (0.1, -0.2, 0.05)).view(np.uint8)
        keep, dist, st = run.call("outlier_statistical", ctx.outlier_statistical, _lib.MOV, 8, 1.0)
        out.update(stat_keep=keep.view(np.uint8), stat_d=dist, stat_record=_stats(st))
        keep, cnt, kept = run.call("outlier_radius", ctx.outlier_radius, _lib.FIX, 0.3, 4)
        out.update(radius_keep=keep.view(np.uint8), radius_count=cnt, radius_kept=np.array([kept], np.int64))
        F, cnt, st = run.call("fpfh", ctx.fpfh, _lib.MOV, d["N"], 12, 0.8, (0.0, 0.0, 10.0), want_counts=True)
        out.update(fpfh=F, fpfh_counts=cnt, fpfh_record=_stats(st))
        keep, sal, eig, st = run.call("keypoints", ctx.keypoints, _lib.FIX, 12, np.inf, 6, np.inf, 0.975, 0.975, 5, want_saliency=True)
        out.update(iss_keep=keep.view(np.uint8), iss_saliency=sal, iss_eig=eig, iss_record=_stats(st))
        rec = run.call("evaluate", ctx.evaluate, _lib.FIX, _lib.MOV, d["H"], 0.3)
        out["eval_counts"] = np.array([rec.n_queries, rec.n_inliers], np.int64)
        out["eval_sums"] = np.array([rec.sum_d2, *rec.sum_p, *rec.sum_pp], dtype=np.float64)
        idx, d2, st = run.call("feature_match", ctx.feature_match, d["q"], d["t"])
        out.update(match_idx=idx, match_d2=d2, match_record=_stats(st))
        poses, inl, st = run.call("ransac_triplets", ctx.ransac_triplets, d["src"], d["dst"], d["tri"], 0.02, 0.9)
        out.update(ransac_poses=poses, ransac_inliers=inl, ransac_record=_stats(st))
        poses, inl, st = run.call("pose_refit", ctx.pose_refit, d["src"], d["dst"], d["start"], 0.05, 2)
        out.update(refit_poses=poses, refit_inliers=inl, refit_record=_stats(st))
        poses, inl, scales, st = run.call("pose_robust", ctx.pose_robust, d["src"], d["dst"], d["start"], 0.01, 2, 1.4, 0.0)
        out.update(robust_poses=poses, robust_inliers=inl, robust_scales=scales, robust_record=_stats(st))
        degree, core, st = run.call("match_consistency", ctx.match_consistency, d["big_src"], d["big_dst"], 0.01, 0.1)
        rec = st.as_dict()
        rec.pop("n_subrounds")                                # (how the peel was scheduled, not what it found)
        out.update(cons_degree=degree, cons_core=core, cons_record=np.array(list(rec.values()), np.float64))
        return out
    finally:
        ctx.close()


def expected_operators(seed):
    import consistency_ref
    import eval_ref
    import fpfh_ref
    import global_ref
    import iss_ref
    import outlier_ref
    import posefit_ref
    import robust_ref
    import voxel_ref
    from simpleicp_amd import _lib
    d = operator_inputs(seed)
    F, M = d["F"], d["M"]

    def rec(cls, values):
        return np.array([values[name] for name, _ in cls._fields_], dtype=np.float64)
    e = {}
    e["voxel_keep"] = voxel_ref.keep(F, 0.3, (0.1, -0.2, 0.05)).view(np.uint8)
    r = outlier_ref.statistical(M, 8, 1.0)
    e.update(stat_keep=r["keep"].view(np.uint8), stat_d=r["d"], stat_record=rec(_lib.OutlierStats, r))
    r = outlier_ref.radius(F, 0.3, 4)
    e.update(radius_keep=r["keep"].view(np.uint8), radius_count=np.asarray(r["count"], np.uint32), radius_kept=np.array([r["n_kept"]], np.int64))
    r = fpfh_ref.fpfh(M, d["N"], 12, 0.8, (0.0, 0.0, 10.0))
    e.update(fpfh=np.asarray(r["fpfh"], np.float32), fpfh_counts=np.asarray(r["counts"], np.uint16), fpfh_record=rec(_lib.FpfhStats, r))
    r = iss_ref.keypoints(F, 12, np.inf, 6, np.inf, 0.975, 0.975, 5)
    e.update(iss_keep=r["keep"].view(np.uint8), iss_saliency=r["saliency"], iss_eig=r["eig"], iss_record=rec(_lib.KeypointStats, r))
    r = eval_ref.evaluate(F, M, d["H"], 0.3, None)
    e.update(eval_counts=np.array([r["n_queries"], r["n_inliers"]], np.int64), eval_sums=np.asarray(r["sums"], np.float64))
    idx, d2, st = global_ref.match(d["q"], d["t"])
    e.update(match_idx=np.asarray(idx, np.int32), match_d2=np.asarray(d2, np.float32), match_record=rec(_lib.MatchStats, st))
    poses, inl, st = global_ref.ransac(d["src"], d["dst"], d["tri"], 0.02, 0.9)
    e.update(ransac_poses=poses, ransac_inliers=np.asarray(inl, np.int32), ransac_record=rec(_lib.RansacStats, st))
    poses, inl, st = posefit_ref.refit(d["src"], d["dst"], d["start"], 0.05, 2)
    e.update(refit_poses=poses, refit_inliers=np.asarray(inl, np.int32), refit_record=rec(_lib.PosefitStats, st))
    poses, inl, scales, st = robust_ref.robust(d["src"], d["dst"], d["start"], 0.01, 2, 1.4, 0.0)
    e.update(robust_poses=poses, robust_inliers=np.asarray(inl, np.int32), robust_scales=scales, robust_record=rec(_lib.RobustStats, st))
    degree, core, st = consistency_ref.consistency(d["big_src"], d["big_dst"], 0.01, 0.1)
    names = [n for n, _ in _lib.ConsistencyStats._fields_ if n != "n_subrounds"]
    e.update(cons_degree=np.asarray(degree, np.int32), cons_core=np.asarray(core, np.int32),
             cons_record=np.array([st[n] for n in names], np.float64))
    return {k: ("bits", np.asarray(v)) for k, v in e.items()}


REFUSALS = ("null ctx", "slot must be SICP_FIX or SICP_MOV", "k must be <= 128 ({k} given)")


def job_refusals(run, seed):
    """Three calls refused before any device work, each message read back at once, then a valid call -- over and over.  The bad k
    is the thread's own (200 + seed), so a message that crossed threads would show."""
    import ctypes as C
    from simpleicp_amd import _lib
    L = _lib.load()
    P = surface_pair(2000, 70 + seed)[0]
    q = np.ascontiguousarray(P[::7] + 0.01)
    k = 200 + seed
    n = C.c_int64()
    nrm = np.zeros((len(P), 3), np.float32)
    ctx = _context(run)
    try:
        run.call("upload", ctx.upload, _lib.FIX, P)
        run.meet()
        said, wrong = None, 0
        for _ in range(REFUSAL_REPS):
            got = []
            for fn in (lambda: L.sicp_cloud_size(None, 0, C.byref(n)), lambda: L.sicp_cloud_size(ctx._h, 5, C.byref(n))):
                rc = run.call("refusal", fn)
                got.append((rc, L.sicp_last_error()))
            try:
                run.call("refusal", ctx.fpfh, _lib.FIX, nrm, k)
                got.append((0, b""))
            except _lib.BackendError as e:
                got.append((e.code, str(e).encode()))
            idx, d2 = run.call("knn", ctx.knn, _lib.FIX, q, 1)
            this = (tuple(got), idx.tobytes(), d2.tobytes())
            said = this if said is None else said
            wrong += this != said
        codes = np.array([rc for rc, _ in said[0]], np.int64)
        return dict(messages=np.frombuffer(b"\n".join(m for _, m in said[0]), np.uint8).copy(), codes=codes,
                    changed=np.array([wrong], np.int64), idx=idx, d2=d2)
    finally:
        ctx.close()


def expected_refusals(seed):
    from oracle import orc
    from simpleicp_amd import _lib
    P = surface_pair(2000, 70 + seed)[0]
    idx, d2 = orc.knn(P, np.ascontiguousarray(P[::7] + 0.01), k=1)
    text = "\n".join(REFUSALS).format(k=200 + seed).encode()
    return {"messages": ("bits", np.frombuffer(text, np.uint8)), "codes": ("bits", np.full(3, _lib.ERR_INVALID, np.int64)),
            "changed": ("bits", np.zeros(1, np.int64)), "idx": ("bits", np.asarray(idx, np.int64)), "d2": ("bits", np.asarray(d2, np.float64))}


def job_ring(run, seed):
    """A lean context (its staged uploads and download_both go through the ONE pinned ring of the process's lean contexts): a small
    cloud up the staged road and back, then one of two download chunks."""
    from simpleicp_amd import _lib
    small, large = ring_cloud(RING_SMALL, seed), ring_cloud(RING_TWO_CHUNKS, seed)
    ctx = _context(run, lean=True)
    try:
        run.meet()
        out = {}
        for name, X in (("small", small), ("large", large)):
            run.call("ring:upload", ctx.upload, _lib.MOV, X)
            rows, cols = run.call("ring:download_both", ctx.download_both, _lib.MOV)
            out[name + "_rows"], out[name + "_columns"] = rows, np.ascontiguousarray(np.stack(cols))
        return out
    finally:
        ctx.close()


def expected_ring(seed):
    out = {}
    for name, n in (("small", RING_SMALL), ("large", RING_TWO_CHUNKS)):
        X = ring_cloud(n, seed)
        out[name + "_rows"], out[name + "_columns"] = ("bits", X), ("bits", np.ascontiguousarray(X.T))
    return out


def job_churn(run, seed):
    """Create a context, upload, download, close -- in a loop: allocation and free synchronise the device under the others."""
    from simpleicp_amd import _lib
    X = ring_cloud(RING_SMALL, 100 + seed)
    run.meet()
    wrong = 0
    for _ in range(CHURN_REPS):
        ctx = run.call("churn:ctx_create", _lib.Context, 0)
        try:
            run.call("churn:upload", ctx.upload, _lib.FIX, X)
            back = run.call("churn:download", ctx.download, _lib.FIX)
        finally:
            run.call("churn:close", ctx.close)
        wrong += not np.array_equal(back, X)
    return dict(back=back, wrong=np.array([wrong], np.int64))


def expected_churn(seed):
    return {"back": ("bits", ring_cloud(RING_SMALL, 100 + seed)), "wrong": ("bits", np.zeros(1, np.int64))}


JOBS = {"run1000": job_run(1000), "run2049": job_run(2049), "run16385": job_run(16385), "normals": job_normals,
        "operators": job_operators, "refusals": job_refusals, "ring": job_ring, "churn": job_churn}
EXPECTED = {"run1000": lambda s: expected_run(1000, s), "run2049": lambda s: expected_run(2049, s),
            "run16385": lambda s: expected_run(16385, s), "normals": expected_normals, "operators": expected_operators,
            "refusals": expected_refusals, "ring": expected_ring, "churn": expected_churn}

# Four threads, three rounds, nothing drawn at run time.
# Round 0: two one-launch runs (a) and the prelaunched chain (b) while the fourth thread creates and closes contexts beside all
#          three (e).  The runs of (a) and (b) take turns per device (device_wait_turn, sicp_icp.cpp): their CALLS overlap -- one
#          inside the library, the others waiting for the turn -- their kernels do not.  What these pairings show is that the turn
#          is contended and that the results behind it are the runs' own.  The contexts that come and go take no turn: their
#          allocations, frees and stream destructions do run beside the waiting kernels.
# Round 1: three lean contexts on the shared ring (c), the stand-alone operators beside them.
# Round 2: the prelaunched chain again, now beside work that takes no turn and does run at the same time -- the three-launch path
#          and the normals' sweep (f) -- and refusals beside all three (d).
SCHEDULE = [
    [("run16385", 0), ("ring", 0), ("run2049", 0)],
    [("run16385", 1), ("ring", 1), ("normals", 1)],
    [("run1000", 2), ("ring", 2), ("run1000", 5)],
    [("churn", 3), ("operators", 2), ("refusals", 3)],
]
# the process whose first library calls are four threads' (tests/helpers/threads_first_use.py)
FIRST_USE_SCHEDULE = [[("run16385", t % 2), ("ring", t)] for t in range(4)]
COMPUTE = ("icp_run:1000", "icp_run:2049", "icp_run:16385", "estimate_normals", "voxel_select", "outlier_statistical", "outlier_radius",
           "fpfh", "keypoints", "evaluate", "feature_match", "ransac_triplets", "pose_refit", "pose_robust", "match_consistency")
CHURN = ("churn:ctx_create", "churn:upload", "churn:download", "churn:close")
RING = ("ring:upload", "ring:download_both")
PAIRINGS = {
    "a: one-launch run beside one-launch run (calls; the kernels take turns)": (tagged("icp_run:16385"), tagged("icp_run:16385")),
    "b: prelaunched run beside one-launch run (calls; the kernels take turns)": (tagged("icp_run:1000"), tagged("icp_run:16385")),
    "d: refusals beside everything else": (tagged("refusal"), lambda r: r[2] != "refusal" and r[1] != "refusals"),
    "e: contexts created and closed beside compute": (tagged(*CHURN), tagged(*COMPUTE)),
    "e: contexts closed beside the prelaunched run": (tagged("churn:close"), tagged("icp_run:1000")),
    "e: contexts created beside the one-launch runs": (tagged("churn:ctx_create"), tagged("icp_run:16385")),
    "f: prelaunched run beside the three-launch run and the normals": (tagged("icp_run:1000"), tagged("icp_run:2049", "estimate_normals")),
}


def ring_threads_overlap(records):
    """(c): every two of the three lean contexts had ring calls in flight at the same time.  -> the thread pairs that did not"""
    threads = sorted({r[0] for r in records if r[2] in RING})
    return [(s, t) for i, s in enumerate(threads) for t in threads[i + 1:]
            if not overlapping(records, lambda r, s=s: r[0] == s and r[2] in RING, lambda r, t=t: r[0] == t and r[2] in RING)]


# ---- comparing --------------------------------------------------------------------------------------------------------------------------
def against_expected(got, want, who):
    """Problems of a job's result against its expectation, each key at its own kind."""
    bad = []
    for key, (kind, value) in want.items():
        if key not in got:
            bad.append(f"{who}: no {key}")
            continue
        g, v = np.asarray(got[key]), np.asarray(value)
        if g.shape != v.shape:
            bad.append(f"{who}: {key} has shape {g.shape}, the reference {v.shape}")
        elif kind == "bits":
            if g.dtype != v.dtype or g.tobytes() != v.tobytes():
                n = int(np.count_nonzero(~((g == v) | ((g != g) & (v != v))))) if g.dtype == v.dtype else -1
                bad.append(f"{who}: {key} ({g.dtype}) differs from the reference ({v.dtype}) in {n} entries of {v.size}")
        else:
            ok = np.isfinite(v)
            err = float(np.abs(g[ok].astype(np.float64) - v[ok]).max()) if ok.any() else 0.0
            if not err <= kind or not np.array_equal(np.isfinite(g), ok):
                bad.append(f"{who}: {key} is off the reference by {err:.3e} (allowed {kind:.0e})")
    return bad


def against_serial(got, serial, who):
    """Problems of a threaded result against the same job run alone: every key, every byte."""
    bad = [f"{who}: keys {sorted(got)} against {sorted(serial)} alone"] if sorted(got) != sorted(serial) else []
    for key in sorted(set(got) & set(serial)):
        g, s = np.asarray(got[key]), np.asarray(serial[key])
        if g.dtype != s.dtype or g.shape != s.shape or g.tobytes() != s.tobytes():
            n = int(np.count_nonzero(g != s)) if g.shape == s.shape else -1
            bad.append(f"{who}: {key} differs from the run alone in {n} entries of {s.size}")
    return bad


def digest(result, keys=None):
    """sha256 over the named keys (all: sorted) of a result: names, dtypes, shapes, bytes."""
    h = hashlib.sha256()
    for key in sorted(result if keys is None else keys):
        a = np.ascontiguousarray(result[key])
        h.update(f"{key}|{a.dtype}|{a.shape}|".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def key_digests(result):
    return {key: digest(result, [key]) for key in sorted(result)}
