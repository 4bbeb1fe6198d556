"""A process whose very FIRST calls into libsimpleicp_hip.so come from four threads at once: each creates a context and runs the
one-launch Q = 16 385 job, then a ring job on a lean context (tests/thread_jobs.py: FIRST_USE_SCHEDULE).  What a warm process has
long initialised -- the runtime, the code objects, resident_blocks' cache, the lean contexts' shared ring -- is raced here.  Every
input is made BEFORE the threads start, so that the first thing a thread does behind the start barrier is sicp_ctx_create.  Run as
a child process by tests/test_gpu_threads.py; prints one JSON line per thread and job (a sha256 per key of the result, the
estimates as hex) and one for the race: the pairs of threads whose first sicp_ctx_create calls shared wall time."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import thread_jobs as tj  # noqa: E402


def main():
    schedule = tj.FIRST_USE_SCHEDULE
    for row in schedule:
        for job, seed in row:
            if job == "run16385":
                tj.run_inputs(16385, seed)                   # (the oracle's normals: CPU work, nothing of the library)
    results, records = tj.run_schedule(schedule, tj.JOBS, tj.watchdog_seconds(schedule))
    first = {}
    for r in sorted(records, key=lambda r: r[3]):
        if r[2] == "ctx_create":
            first.setdefault(r[0], r)
    ids = {id(r) for r in first.values()}
    pairs = tj.overlapping(records, lambda r: id(r) in ids, lambda r: id(r) in ids)
    for t, row in enumerate(results):
        for (job, seed), res in zip(schedule[t], row):
            line = dict(thread=t, job=job, seed=seed, digests=tj.key_digests(res))
            if "x" in res:
                line["x"] = [[float(v).hex() for v in it] for it in res["x"]]
            print(json.dumps(line), flush=True)
    print(json.dumps(dict(first_creates_overlapping=sorted({tuple(sorted((a[0], b[0]))) for a, b in pairs}))), flush=True)


if __name__ == "__main__":
    main()
