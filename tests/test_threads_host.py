"""The threaded tests' own machinery (tests/thread_jobs.py) on stub jobs, and the library's last-error text under eight threads --
refusals that come before any device work, so the real library answers them on a machine without a GPU.  No device needed.
(A slot that is none and a k out of range are refused only once a context is there: tests/test_gpu_threads.py asks for those.)"""
import ctypes as C
import threading

import numpy as np
import pytest

import thread_jobs as tj


# ---- the real library: eight threads, one refusal each ---------------------------------------------------------------------------------
def _refusals(L, thread):
    """name -> (the call, its message): what thread `thread` may ask for."""
    n, cnt, pos, ctx = C.c_int64(), C.c_int64(), (C.c_int64 * 4)(), C.c_void_p()
    buf = (C.c_double * 16)()
    path = f"/nonexistent/sicp-thread-{thread}.xyz".encode()
    return [
        (lambda: L.sicp_cloud_size(None, 0, C.byref(n)), b"null ctx"),
        (lambda: L.sicp_device_count(None), b"count_out is null"),
        (lambda: L.sicp_ctx_create(0, None), b"ctx_out is null"),
        (lambda: L.sicp_cloud_upload(None, 0, None, 1, 0), b"xyz is null"),
        (lambda: L.sicp_cloud_upload_columns(None, 0, buf, None, buf, 1, 0), b"x / y / z is null"),
        (lambda: L.sicp_select_positions(-1 - thread, 0, pos, C.byref(cnt)), b"m must be >= 0 and Q > 0"),
        (lambda: L.sicp_xyz_count(path, C.byref(n)), b"cannot open " + path),
        (lambda: L.sicp_ctx_device_name(ctx, C.create_string_buffer(8), 8), b"bad arguments"),
    ]


def test_every_thread_reads_its_own_last_error():
    """Each of eight threads asks for ONE refusal, 500 times, with a call that succeeds in between: the text is always its own
    (sicp_api.cpp: g_err is thread_local), whatever the other seven were just told."""
    from simpleicp_amd import _lib
    L = _lib.load()
    _lib.device_version()

    def job(run, thread):
        ask, want = _refusals(L, thread)[thread]
        pos, cnt = (C.c_int64 * 4)(), C.c_int64()
        run.meet()
        wrong = []
        for i in range(500):
            rc = run.call("refusal", ask)
            said = L.sicp_last_error()
            if rc != _lib.ERR_INVALID or said != want:
                wrong.append((i, rc, said))
            assert run.call("fine", L.sicp_select_positions, 3, 4, pos, C.byref(cnt)) == _lib.OK and cnt.value == 3
            if L.sicp_last_error() != want:                    # (a call that succeeds leaves the text alone)
                wrong.append((i, "after a success", L.sicp_last_error()))
        return wrong[:5]
    results, records = tj.run_schedule([[("refuse", t)] for t in range(8)], {"refuse": job}, tj.ALLOWANCE_SECONDS)
    assert [row[0] for row in results] == [[]] * 8
    assert len({_refusals(L, t)[t][1] for t in range(8)}) == 8
    assert sum(r[2] == "refusal" for r in records) == 8 * 500


def test_the_binding_releases_the_interpreter_lock():
    """ctypes.CDLL drops the GIL around every call, PyDLL keeps it: with PyDLL no two calls could ever overlap."""
    from simpleicp_amd import _lib
    L = _lib.load()
    assert type(L) is C.CDLL and not isinstance(L, C.PyDLL)


# ---- the schedule, the overlaps, the stop event: stub jobs ------------------------------------------------------------------------------
def test_overlapping_wants_other_threads_and_shared_time():
    rec = [(0, "j", "a", 0.0, 2.0), (0, "j", "b", 1.0, 3.0), (1, "j", "b", 1.5, 1.6), (2, "j", "b", 2.0, 4.0), (3, "j", "a", 5.0, 6.0)]
    got = tj.overlapping(rec, tj.tagged("a"), tj.tagged("b"))
    assert got == [(rec[0], rec[2])]                         # (the same thread does not count, nor an interval that only touches)
    assert tj.overlapping(rec, tj.tagged("a"), tj.tagged("a")) == []
    assert tj.ring_threads_overlap([(0, "ring", "ring:upload", 0.0, 1.0), (1, "ring", "ring:upload", 0.5, 1.5),
                                    (2, "ring", "ring:download_both", 1.2, 2.0)]) == [(0, 2)]


def test_schedule_runs_every_job_and_the_meeting_point_makes_calls_overlap():
    """Three rounds on four threads; in every round the calls tagged "hot" wait for each other INSIDE the call (a barrier of the four),
    so they overlap by construction -- and the bookkeeping must say so for every pair of threads."""
    inside = threading.Barrier(4)

    def job(run, seed):
        a = run.call("prepare", lambda: seed * 2)
        run.meet()
        run.call("hot", inside.wait, 30)
        return a + 1
    schedule = [[("stub", 10 * t + r) for r in range(3)] for t in range(4)]
    results, records = tj.run_schedule(schedule, {"stub": job}, 60.0)
    assert results == [[2 * (10 * t + r) + 1 for r in range(3)] for t in range(4)]
    assert len(records) == 24 and {r[0] for r in records} == {0, 1, 2, 3} and all(r[4] >= r[3] for r in records)
    # (4 threads x 3 rounds: every hot call overlaps the three others of its round, and none of another round)
    assert len(tj.overlapping(records, tj.tagged("hot"), tj.tagged("hot"))) == 3 * 4 * 3
    assert tj.overlapping(records, tj.tagged("prepare"), tj.tagged("hot")) == []       # (the meeting point lies between them)


def test_first_failure_stops_every_thread_before_its_next_call():
    """Thread 2 fails in round 0.  The others are past their first call and waiting at the meeting point: they leave it, start no
    further call, and the failure is what the main thread raises."""
    started = threading.Barrier(4)

    def job(run, seed):
        run.call("first", started.wait, 30)                  # (all four are in their jobs before anything fails)
        if seed == 2:
            raise ValueError("planted")
        run.meet()
        run.call("after", lambda: None)
        return seed
    records = []
    real = tj.Runner.call

    def noting(self, tag, fn, *a, **k):
        records.append(tag)
        return real(self, tag, fn, *a, **k)
    tj.Runner.call = noting
    try:
        with pytest.raises(RuntimeError, match="thread 2: ValueError: planted"):
            tj.run_schedule([[("stub", t), ("stub", t + 10)] for t in range(4)], {"stub": job}, 60.0)
    finally:
        tj.Runner.call = real
    assert sorted(records) == ["first"] * 4


def test_runner_refuses_to_start_a_call_once_stopped():
    stop, made = threading.Event(), []
    run = tj.Runner(stop=stop)
    run.call("one", made.append, 1)
    stop.set()
    with pytest.raises(tj.Stopped):
        run.call("two", made.append, 2)
    assert made == [1] and [r[2] for r in run.records] == ["one"]


def test_watchdog_raises_instead_of_waiting():
    """A deadline that has already passed: the threads cannot all be at the start in no time, the run ends in TimeoutError at once
    (nothing here waits for a limit to run out) and no job is started."""
    made = []
    with pytest.raises(TimeoutError):
        tj.run_schedule([[("stub", t)] for t in range(4)], {"stub": lambda run, seed: made.append(seed)}, -1.0)
    assert made == []


def test_watchdog_is_sized_from_the_barrier_bound():
    assert tj.barrier_spin_bound() == 1 << 21                # sicp_lanes.h: `if (++spins > (1L << 21))`
    text = (tj.ROOT / "simpleicp_amd" / "csrc" / "sicp_grid_nn_one.inc").read_text()
    assert "if (++spins > (1L << 21))" in text               # (the early match's ticket wait: the same bound)
    launches = tj.barrier_launches(tj.SCHEDULE)
    assert launches == 2 * 2 * (1 + tj.RUNS[16385]["iterations"] * tj.RUNS[16385]["reps"])
    runs = tj.ticket_waiting_runs(tj.SCHEDULE)
    assert runs == 2 * tj.RUNS[1000]["reps"]
    assert tj.watchdog_seconds(tj.SCHEDULE) == (1 << 21) * tj.POLL_SECONDS * (launches + runs) + tj.ALLOWANCE_SECONDS
    assert tj.ticket_waiting_runs(tj.FIRST_USE_SCHEDULE) == 0 and tj.barrier_launches(tj.FIRST_USE_SCHEDULE) == 2 * launches


def test_schedule_holds_what_it_is_meant_to_overlap():
    """Four threads, three rounds, every job with a reference; the pairings' jobs share a round."""
    S = tj.SCHEDULE
    assert len(S) == 4 and all(len(row) == 3 for row in S)
    assert all(name in tj.JOBS and name in tj.EXPECTED for row in S + tj.FIRST_USE_SCHEDULE for name, _ in row)
    rounds = [[row[r][0] for row in S] for r in range(3)]
    assert sorted(rounds[0]) == ["churn", "run1000", "run16385", "run16385"]
    assert sorted(rounds[1]) == ["operators", "ring", "ring", "ring"]
    assert sorted(rounds[2]) == ["normals", "refusals", "run1000", "run2049"]
    assert all(len({seed for name, seed in [row[r] for row in S] if name == job}) == rounds[r].count(job)
               for r in range(3) for job in set(rounds[r]))            # (no two threads of a round work on the same data)
    assert len(tj.FIRST_USE_SCHEDULE) == 4 and all([name for name, _ in row] == ["run16385", "ring"] for row in tj.FIRST_USE_SCHEDULE)


def test_comparisons_tell_bits_from_bounds():
    want = {"idx": ("bits", np.array([1, 2, 3], np.int64)), "x": (1e-9, np.array([1.0, 2.0]))}
    good = {"idx": np.array([1, 2, 3], np.int64), "x": np.array([1.0 + 5e-10, 2.0]), "extra": np.zeros(2)}
    assert tj.against_expected(good, want, "w") == []
    assert len(tj.against_expected(dict(good, idx=np.array([1, 2, 4], np.int64)), want, "w")) == 1
    assert len(tj.against_expected(dict(good, idx=np.array([1, 2, 3], np.int32)), want, "w")) == 1
    assert len(tj.against_expected(dict(good, x=np.array([1.0 + 2e-9, 2.0])), want, "w")) == 1
    assert len(tj.against_expected(dict(good, x=np.array([np.nan, 2.0])), want, "w")) == 1
    assert tj.against_serial(good, {k: v.copy() for k, v in good.items()}, "w") == []
    assert len(tj.against_serial(dict(good, x=np.array([1.0 + 6e-10, 2.0])), good, "w")) == 1     # (alone against threaded: every bit)
    assert tj.key_digests(good) == tj.key_digests({k: v.copy() for k, v in good.items()})
    assert tj.digest(good, ["idx"]) != tj.digest(dict(good, idx=good["idx"].astype(np.int32)), ["idx"])
