"""Contexts used from several host threads at once, one context per thread ("Ownership/threading"), held to the
bits of the same work done alone.  The jobs, the schedule and the bookkeeping are tests/thread_jobs.py; every expectation is the
CPU oracle's or a numpy reference's, computed before a thread starts.  Each job first runs alone against its expectation (a plain
defect shows here), then the schedule runs on four threads and every result is held against the same expectation AND, byte for
byte, against the run alone (a difference here is a leak between contexts).  The library is deterministic to the bit, so nothing
is allowed to differ.  GPU only."""
import ctypes as C
import json
import subprocess
import sys
import time

import numpy as np
import pytest

import thread_jobs as tj
from conftest import ROOT

pytestmark = pytest.mark.gpu

KEYS = sorted({entry for row in tj.SCHEDULE for entry in row})
_expected, _alone = {}, {}


def expected(key):
    if key not in _expected:
        _expected[key] = tj.EXPECTED[key[0]](key[1])
    return _expected[key]


def _stop_the_session(what, e):
    """An error of the library itself or a hang, not a mismatch: nothing more is started on a device that may have faulted
    (tests/test_gpu_operator_sequences.py does the same)."""
    import traceback
    traceback.print_exception(type(e), e, e.__traceback__)
    pytest.exit(f"{what}: {type(e).__name__}: {e}", returncode=3)


def alone(key):
    """The job on the calling thread, nothing else on the device: (result, seconds)."""
    if key not in _alone:
        expected(key)                                        # (the reference first: nothing of it is computed beside GPU work)
        t0 = time.perf_counter()
        try:
            res = tj.JOBS[key[0]](tj.Runner(job=key[0]), key[1])
        except Exception as e:  # noqa: BLE001
            _stop_the_session(f"{key} alone", e)
        _alone[key] = (res, time.perf_counter() - t0)
    return _alone[key]


@pytest.mark.parametrize("key", KEYS, ids=[f"{name}-{seed}" for name, seed in KEYS])
def test_job_alone_agrees_with_its_reference(key):
    res, seconds = alone(key)
    print(f"{key}: {seconds * 1e3:.1f} ms alone")
    assert tj.against_expected(res, expected(key), f"{key} alone") == []


@pytest.fixture(scope="module")
def threaded():
    """The schedule on four threads: (results[t][r], records, seconds)."""
    for key in KEYS:
        alone(key)                                           # (references and serial legs are done before a thread starts)
    watchdog = tj.watchdog_seconds(tj.SCHEDULE)
    t0 = time.perf_counter()
    try:
        results, records = tj.run_schedule(tj.SCHEDULE, tj.JOBS, watchdog)
    except TimeoutError as e:
        _stop_the_session("the threaded schedule", e)
    except RuntimeError as e:
        # an error RETURN of the library (a bounded wait that expired is one: tests/test_gpu_kernels.py,
        # test_grid_barrier_timeout_is_an_error_not_a_hang), not a hang: the schedule has stopped, the session goes on
        beside = "\n".join(f"  thread {r[0]} {r[1]} {r[2]}: {(r[4] - r[3]) * 1e3:.2f} ms" for r in getattr(e, "beside", []))
        pytest.fail(f"{e}\nthe call that failed, and the calls beside it:\n{beside}")
    return results, records, time.perf_counter() - t0


def test_threads_agree_with_the_references_and_with_the_runs_alone(threaded):
    results, records, seconds = threaded
    print(f"{len(records)} calls on {len(tj.SCHEDULE)} threads in {seconds * 1e3:.1f} ms")
    bad = []
    for t, row in enumerate(tj.SCHEDULE):
        for r, key in enumerate(row):
            who = f"thread {t} round {r} {key}"
            bad += tj.against_expected(results[t][r], expected(key), who)
            bad += tj.against_serial(results[t][r], alone(key)[0], who)
    assert bad == []


@pytest.mark.parametrize("pairing", sorted(tj.PAIRINGS))
def test_the_pairing_did_overlap(threaded, pairing):
    """Not vacuous: calls of the two kinds, from different threads, were in flight at the same wall time.  For (a) and (b) that
    is one call inside the library and the other waiting for its device's turn (thread_jobs.SCHEDULE says what runs side by side)."""
    first, second = tj.PAIRINGS[pairing]
    pairs = tj.overlapping(threaded[1], first, second)
    print(f"{pairing}: {len(pairs)} overlapping pairs of calls")
    assert pairs, pairing


def test_the_three_ring_jobs_did_overlap(threaded):
    """(c): every two of the three lean contexts were inside a staged upload or a download_both at the same time -- the shared
    ring's lock was contended."""
    assert sorted({r[0] for r in threaded[1] if r[2] in tj.RING}) == [0, 1, 2]
    assert tj.ring_threads_overlap(threaded[1]) == []


def test_refusals_keep_to_their_thread():
    """Eight threads, each with a context of its own and ONE refusal to ask for -- a null context, a slot that is none, a k of its
    own that is too large -- 200 times: the text read back is always that thread's."""
    from simpleicp_amd import _lib
    L = _lib.load()
    n = C.c_int64()
    nrm, out, st = np.zeros((500, 3), np.float32), np.empty((500, 33), np.float32), _lib.FpfhStats()
    P = tj.surface_pair(500, 9)[0]
    _lib.fpfh_version()

    def job(run, seed):
        ctx = run.call("ctx_create", _lib.Context, 0)
        try:
            run.call("upload", ctx.upload, _lib.FIX, P)
            k = 130 + seed
            ask = [lambda: L.sicp_cloud_size(None, 0, C.byref(n)), lambda: L.sicp_cloud_size(ctx._h, 2 + seed, C.byref(n)),
                   lambda: L.sicp_fpfh(ctx._h, _lib.FIX, _lib._ptr(nrm), k, np.inf, None, _lib._ptr(out), None, C.byref(st))][seed % 3]
            want = tj.REFUSALS[seed % 3].format(k=k).encode()
            run.meet()
            wrong = 0
            for _ in range(200):
                rc = run.call("refusal", ask)
                wrong += rc != _lib.ERR_INVALID or L.sicp_last_error() != want
            return wrong
        finally:
            ctx.close()
    schedule = [[("refuse", t)] for t in range(8)]
    try:
        results, records = tj.run_schedule(schedule, {"refuse": job}, tj.ALLOWANCE_SECONDS)
    except TimeoutError as e:
        _stop_the_session("eight threads of refusals", e)
    assert [row[0] for row in results] == [0] * 8
    assert tj.overlapping(records, tj.tagged("refusal"), tj.tagged("refusal"))


def test_first_use_raced_in_a_fresh_process():
    """tests/helpers/threads_first_use.py: the first calls of a process are four threads'.  Its digests against the references
    (every bit-comparable key), its estimates to 1e-9, and every key against this process's runs alone."""
    helper = ROOT / "tests" / "helpers" / "threads_first_use.py"
    schedule = tj.FIRST_USE_SCHEDULE
    for key in sorted({entry for row in schedule for entry in row}):
        alone(key)
    limit = int(tj.watchdog_seconds(schedule)) + 60                     # (+ the interpreter, numpy and the library coming up)
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, str(helper)], capture_output=True, text=True)
    if r.returncode in (124, 137, 134, 139, -6, -9, -11):
        # a hang, an abort or a segmentation fault of the child: nothing more is started on the device
        _stop_the_session("the first-use child", RuntimeError(f"exit {r.returncode}\n{r.stdout[-1000:]}\n{r.stderr[-3000:]}"))
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    lines = [json.loads(s) for s in r.stdout.splitlines() if s.startswith("{")]
    # the race did happen: every two of the four threads were inside their first sicp_ctx_create at the same time
    assert lines[-1] == {"first_creates_overlapping": [[s, t] for s in range(4) for t in range(s + 1, 4)]}, lines[-1]
    assert len(lines) == 1 + sum(len(row) for row in schedule)
    bad = []
    for line in lines[:-1]:
        key, who = (line["job"], line["seed"]), f"child thread {line['thread']} {line['job']}"
        want, serial = expected(key), alone(key)[0]
        for name, (kind, value) in want.items():
            if kind == "bits" and line["digests"].get(name) != tj.digest({name: value}, [name]):
                bad.append(f"{who}: {name} differs from the reference")
        if "x" in want:
            x = np.array([[float.fromhex(v) for v in it] for it in line["x"]])
            if not np.abs(x - want["x"][1]).max() <= want["x"][0]:
                bad.append(f"{who}: x is off the reference by {np.abs(x - want['x'][1]).max():.3e}")
        if line["digests"] != tj.key_digests(serial):
            bad.append(f"{who}: {sorted(k for k, v in tj.key_digests(serial).items() if line['digests'].get(k) != v)} differ from the run alone")
    assert bad == []
