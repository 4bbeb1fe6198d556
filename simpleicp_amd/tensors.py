"""run_tensors -- ICP on point clouds that are already torch tensors on the GPU: no coordinate-sized array crosses the host link.

The road (include/simpleicp_hip_device.h): both clouds are read where they lie (k_ingest: any strides, float32 widened exactly to
float64), the overlap pre-pass leaves its verdicts in device memory, the selection is compacted and picked on the device
(sicp_select_n_device), the normals and sicp_icp_setup take device buffers, ONE sicp_icp_run runs the loop, and the transformed
movable cloud is written into a new tensor (k_egress).  What comes back is what ``SimpleICP.run`` returns for the same clouds
(widened to float64), bit for bit; ``X_mov_transformed`` is a new contiguous device tensor in ``X_mov``'s dtype (float32: the
float64 result rounded to nearest).  The inputs are never modified.

Stream rule: the library works on its context's own stream.  Before it reads the inputs, that stream waits for torch's CURRENT
stream on the inputs' device, so whatever torch queued there that writes them comes first (no synchronise needed).  Every library
call returns complete: when run_tensors returns, the output tensor is finished and any stream may read it.  Work on OTHER torch
streams that writes an input must be ordered before the call by the caller, as for any torch op on the current stream.

torch is imported here only, on the first call: ``import simpleicp_amd`` stays free of it (a plain run() must not pay for the import;
dist.py says why).
"""
from __future__ import annotations

import logging
import time

import numpy as np

from . import _lib, backend, dist
from . import evaluation
from .icp import SimpleICP, SimpleICPException, _DeviceSelection, _iterate, _outlier_of, _prepare, _rbp_and_residuals, _start_pose, _voxel_of

_log = logging.getLogger(__name__)

_KINDS = {"u8": "uint8", "i64": "int64", "f32": "float32"}


def _is_device_tensor(c) -> bool:
    """A CUDA torch tensor (told without importing torch: a process that never imported it holds none)."""
    return type(c).__module__.startswith("torch") and bool(getattr(c, "is_cuda", False))


def _check_cloud(name, t, device):
    """An (n, 3) float32 / float64 torch tensor on cuda:<device>; anything else is refused before any device work."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, not {type(t).__name__} (host arrays go through SimpleICP.run() or run_batch)")
    if t.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{name} must be float32 or float64, not {t.dtype}")
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name} must have shape (n, 3), not {tuple(t.shape)}")
    if t.device.type != "cuda":
        raise ValueError(f"{name} is on {t.device}: run_tensors takes clouds on the GPU; clouds in host memory go through "
                         "SimpleICP.run() or run_batch")
    if t.device.index != device:
        raise ValueError(f"{name} is on {t.device}, the library's context on cuda:{device}")


def _wait_for_torch(ctx, dev):
    """The stream rule: the library's stream waits for torch's current stream before it reads anything."""
    import torch
    torch.cuda.ExternalStream(ctx.stream_ptr(), device=dev).wait_stream(torch.cuda.current_stream(dev))


def _upload(ctx, slot, t):
    dt = _lib.DT_F64 if t.element_size() == 8 else _lib.DT_F32
    ctx.upload_strided(slot, t.data_ptr(), dt, t.shape[0], t.stride(0), t.stride(1))


def prepare(ctx, X_fix, X_mov, kw, extras, info):
    """What a run (kw: its RunKeywords, extras: its RunExtras) does up to its first iteration, for a device pair on ctx: the stream
    wait, both uploads, _prepare on a _DeviceSelection.  Returns ((obs, ow, H), the statistics of the outlier removal or None,
    scratch) -- scratch: device buffers that must live until the run is over."""
    import torch
    pose = _start_pose(kw)
    dev = X_fix.device
    _wait_for_torch(ctx, dev)

    def alloc(shape, kind):
        b = torch.empty(shape, dtype=getattr(torch, _KINDS[kind]), device=dev)
        return b, b.data_ptr()

    _upload(ctx, _lib.FIX, X_fix)
    _upload(ctx, _lib.MOV, X_mov)
    selection = _DeviceSelection(ctx, X_fix.shape[0], alloc)
    stats = _prepare(selection, kw, extras, pose[2], info)
    return pose, stats, selection.scratch


def transformed(ctx, X_mov, H):
    """A new contiguous (n, 3) tensor in X_mov's dtype holding the movable cloud under H (k_egress; the slot stays as it is)."""
    import torch
    out = torch.empty((X_mov.shape[0], 3), dtype=X_mov.dtype, device=X_mov.device)
    ctx.write_strided(_lib.MOV, H, out.data_ptr(), _lib.DT_F64 if out.element_size() == 8 else _lib.DT_F32, 3, 1)
    return out


def run_tensors(X_fix, X_mov, max_normal_angle=None, voxel_size=None, voxel_origin=None, evaluate_distance=None,
                outlier_neighbors=None, outlier_std_ratio=2.0, **run_kwargs):
    """Registers X_mov to X_fix -- (n, 3) float32 / float64 torch tensors on the GPU of the library's context, any strides -- with
    ``run()``'s keyword arguments.  Returns a BatchResult (path "device") that unpacks as ``(H, X_mov_transformed, rbp,
    residuals)``: H, rbp and residuals are run()'s host values, X_mov_transformed a new device tensor; it also carries
    ``iterations``, ``n_kept``, ``res_mean`` and ``res_std``.  Raises what run() raises, with the same messages.
    ``max_normal_angle`` (degrees, None = off): SimpleICP's attribute of that name; the movable normals are estimated on the device.
    ``voxel_size`` / ``voxel_origin`` (None = off / zeros): SimpleICP's attributes of those names, applied to the fixed cloud on the
    device; the movable cloud is thinned by the caller (``X_mov[voxel_keep(X_mov, c)]``).
    ``evaluate_distance`` (None = off): SimpleICP's attribute of that name -- every fixed point is scored under the final H on the
    device, the Evaluation is the result's ``evaluation``.
    ``outlier_neighbors`` / ``outlier_std_ratio`` (None = off / 2.0): SimpleICP's attributes of those names, applied to the fixed
    cloud on the device (contract (O)); the statistics are the result's ``outlier``.  The movable cloud is thinned by the caller
    (``X_mov[outlier_keep(X_mov, neighbors=20)]``)."""
    from .batch import BatchResult, merged_keywords
    t_start = time.time()
    options = dict(max_normal_angle=max_normal_angle, voxel_size=voxel_size, voxel_origin=voxel_origin,
                   evaluate_distance=evaluate_distance, outlier_neighbors=outlier_neighbors, outlier_std_ratio=outlier_std_ratio)
    kw, extras = merged_keywords("run_tensors", options, run_kwargs)
    if dist.is_distributed():
        raise SimpleICPException("run_tensors does not run in a torch.distributed job: call SimpleICP.run on each rank instead")
    device = backend.default_device()
    _check_cloud("X_fix", X_fix, device)
    _check_cloud("X_mov", X_mov, device)
    extras.check_fixed_size(X_fix.shape[0])
    ctx = backend.get_context()
    ctx._corr_owner = None            # (an operator-level CorrPts object loses the device state to this run)
    dist.detach(ctx)
    # (the evaluation's entry point is asked for before anything is uploaded, the other options' by _prepare)
    if extras.evaluate is not None:
        evaluation.need_backend(ctx)
    (obs, ow, H), outlier_stats, scratch = prepare(ctx, X_fix, X_mov, kw, extras, _log.info)
    R, x_start, x, H, stats, it = _iterate(ctx, obs, ow, H, kw)
    rbp, residuals = _rbp_and_residuals(ctx, R, obs, ow, x_start, x)
    SimpleICP._log_result(H, rbp)
    ev = evaluation.after_run(ctx, H, extras.evaluate, _log.info) if extras.evaluate is not None else None
    X_new = transformed(ctx, X_mov, H)
    del scratch
    _log.info(f"Finished in {time.time() - t_start:.3f} seconds!")
    return BatchResult.of_run((H, X_new, rbp, residuals), R, it + 1, "device", ev, outlier_stats)


def _keep_opening(who, X, mask, needs=None):
    """The common opening of voxel_keep and outlier_keep: X and mask checked, X in the library's fixed slot.  Returns (ctx, n, m8,
    keep) -- the context, the number of points, the mask as contiguous uint8 (None: no mask) and the uint8 tensor (n,) the verdicts
    go to; ctx None for an empty X, keep is the (empty) result then.  needs: (entry point, what it is in words) the context must
    have."""
    import torch
    if dist.is_distributed():
        raise SimpleICPException(f"{who} does not run in a torch.distributed job: thin the clouds with one process first")
    device = backend.default_device()
    _check_cloud("X", X, device)
    n = X.shape[0]
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8) or tuple(mask.shape) != (n,):
            raise TypeError("mask must be a bool or uint8 torch.Tensor of shape (n,)")
        if mask.device != X.device:
            raise ValueError(f"mask is on {mask.device}, X on {X.device}")
    if n == 0:
        return None, 0, None, torch.zeros(0, dtype=torch.bool, device=X.device)
    ctx = backend.get_context()
    ctx._corr_owner = None
    dist.detach(ctx)
    if needs is not None and not hasattr(ctx, needs[0]):
        raise _lib.BackendError(f"this backend has no {needs[1]}")
    # everything torch has to do for this call -- the contiguous copy of a strided mask -- is queued on its current stream BEFORE
    # the library's stream is made to wait for that stream: the library never reads a buffer torch is still writing
    m8 = None if mask is None else mask.contiguous().view(torch.uint8)
    keep = torch.empty(n, dtype=torch.uint8, device=X.device)
    _wait_for_torch(ctx, X.device)
    _upload(ctx, _lib.FIX, X)
    return ctx, n, m8, keep


def voxel_keep(X, voxel_size, origin=None, mask=None):
    """The keep verdicts of contract (V) for X -- an (n, 3) float32 / float64 torch tensor on the GPU of the
    library's context, any strides; float32 is widened exactly before the formula -- as a torch.bool tensor (n,): True for the
    lowest-index point of every voxel of the lattice (cell ``voxel_size``, ``origin`` None = zeros).  ``mask`` (a bool / uint8 (n,)
    tensor on the same device): only the points it marks are candidates, every other point is False.  Ingest and stream rule are
    run_tensors'.  ``X[voxel_keep(X, c)]`` is the thinned cloud; the library's fixed slot holds X afterwards."""
    import torch
    voxel = _voxel_of(voxel_size, origin)
    ctx, n, m8, keep = _keep_opening("voxel_keep", X, mask)
    if ctx is None:
        return keep
    if m8 is None:
        ctx.voxel_select(_lib.FIX, voxel[0], voxel[1], keep_ptr=keep.data_ptr())
    else:
        ctx.voxel_select_masked(_lib.FIX, m8.data_ptr(), n, voxel[0], voxel[1], keep_ptr=keep.data_ptr())
    del m8                                               # (the call returned complete: nothing reads it any more)
    return keep.view(torch.bool)


def outlier_keep(X, *, neighbors=None, std_ratio=2.0, radius=None, min_points=None, mask=None):
    """The keep verdicts of contract (O) for X -- an (n, 3) float32 / float64 torch tensor on the GPU of the
    library's context, any strides; float32 is widened exactly first -- as a torch.bool tensor (n,).  Exactly one filter is named:
    ``neighbors`` (with ``std_ratio``): the statistical one -- True where the mean distance to the ``neighbors`` nearest points of X
    (the point itself included) is at most mean + std_ratio * std over the candidates; ``radius`` (with ``min_points``): True where
    more than ``min_points`` points of X, the point itself included, lie strictly within ``radius``.  ``mask`` (a bool / uint8 (n,)
    tensor on the same device): only the points it marks are candidates -- every other point is False --, while neighbours are
    searched among all of X.  Ingest and stream rule are run_tensors'.  ``X[outlier_keep(X, neighbors=20)]`` is the cleaned cloud;
    the library's fixed slot holds X afterwards."""
    import torch
    if (neighbors is None) == (radius is None):
        raise ValueError("outlier_keep takes exactly one of neighbors= (statistical filter) and radius= (radius filter)")
    if neighbors is not None:
        if min_points is not None:
            raise ValueError("min_points belongs to the radius filter (radius=)")
        try:
            outlier = _outlier_of(neighbors, std_ratio)
        except SimpleICPException as e:
            raise ValueError(str(e).replace("outlier_neighbors", "neighbors").replace("outlier_std_ratio", "std_ratio")) from None
    else:
        try:
            r = float(radius)
            ok = not isinstance(radius, (bool, str, bytes)) and np.isfinite(r) and r > 0.0
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError("radius must be a finite number > 0.")
        if min_points is None or isinstance(min_points, (bool, float, str, bytes)) or int(min_points) != min_points or min_points < 0:
            raise ValueError("min_points must be an integer >= 0.")
    ctx, n, m8, keep = _keep_opening("outlier_keep", X, mask, needs=("outlier_statistical", "outlier removal"))
    if ctx is None:
        return keep
    mp = None if m8 is None else m8.data_ptr()
    if neighbors is not None:
        ctx.outlier_statistical(_lib.FIX, outlier[0], outlier[1], mask_ptr=mp, keep_ptr=keep.data_ptr())
    else:
        ctx.outlier_radius(_lib.FIX, r, int(min_points), mask_ptr=mp, keep_ptr=keep.data_ptr())
    del m8
    return keep.view(torch.bool)
