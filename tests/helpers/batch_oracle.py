"""A stand-in batch member for the CPU tests of run_batch: tests/oracle_backend.OracleContext plus ``icp_run_batch`` as a loop
over each member's own ``icp_run`` (what sicp_icp_run_batch promises to equal), and ``make_lean``.  TEST INFRASTRUCTURE ONLY."""
from simpleicp_amd import _lib
from tests.oracle_backend import OracleContext


class BatchOracleContext(OracleContext):
    def make_lean(self):
        pass

    def icp_run_batch(self, members):
        assert members and members[0][0] is self
        out = []
        for ctx, kw in members:
            try:
                res = ctx.icp_run(**kw)
                out.append(_lib.BatchRun(res, _lib.OK, "", _lib.BATCH_PATH_BATCHED))
            except _lib.BackendError as e:
                out.append(_lib.BatchRun(getattr(e, "results", []), e.code, str(e), _lib.BATCH_PATH_BATCHED))
        return out, 0


def install(monkeypatch):
    """Route the member pool of ``backend`` (run_batch) AND ``backend.get_context()`` (SimpleICP.run) to stand-ins.  The caller
    empties the pool afterwards (``backend.reset_batch_contexts()``: tests/test_batch_host.py's ``stand_in`` fixture), so that no
    stand-in outlives its test in the process-wide pool."""
    from simpleicp_amd import backend
    backend.reset_batch_contexts()
    monkeypatch.setattr(backend, "batch_context_factory", lambda device: BatchOracleContext())
    ctx = BatchOracleContext()
    monkeypatch.setattr(backend, "get_context", lambda: ctx)
    return ctx
