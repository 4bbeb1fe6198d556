"""Process-wide default GPU context used by PointCloud / SimpleICP, and the pool of member contexts run_batch uses.

One process drives one GPU (``LOCAL_RANK`` picks it under torch.distributed.run); the context is
created lazily on first use and raises ``BackendError`` when no MI355X is visible -- there is no
host fallback.
"""
from __future__ import annotations

import os

from . import _lib

_ctx = None


def default_device() -> int:
    return int(os.environ.get("SIMPLEICP_DEVICE", os.environ.get("LOCAL_RANK", "0")))


def get_context() -> "_lib.Context":
    global _ctx
    if _ctx is None:
        _ctx = _lib.Context(default_device())
    return _ctx


def reset_context():
    global _ctx
    if _ctx is not None:
        _ctx.close()
    _ctx = None


# ---- member contexts of run_batch (simpleicp_amd/batch.py): created on demand, reused from call to call, lean ----
_batch_ctxs = []


def _new_batch_context(device):
    ctx = _lib.Context(device)
    ctx.make_lean()
    return ctx


batch_context_factory = _new_batch_context      # (tests replace it, the way tests/oracle_backend.install replaces get_context)


def get_batch_contexts(n) -> list:
    """n member contexts of the pool (on the default device), the first n it holds; more are created when it holds fewer."""
    while len(_batch_ctxs) < n:
        _batch_ctxs.append(batch_context_factory(default_device()))
    return _batch_ctxs[:n]


def reset_batch_contexts():
    """Closes every member context of the pool (their device and pinned memory goes with them)."""
    while _batch_ctxs:
        ctx = _batch_ctxs.pop()
        if hasattr(ctx, "close"):
            ctx.close()
