"""run_batch -- many (fixed, movable) pairs registered in one call, their iterations batched on the GPU.

Each pair gets exactly the preparation ``SimpleICP.run`` gives it (uploads, overlap pre-pass, ``select_n_points``, normals,
selection masks, the movable cloud's planarity column), on a context of the pool in ``backend`` (one per pair, reused from call
to call); then ONE ``sicp_icp_run_batch`` call runs every pair's loop (include/simpleicp_hip_batch.h): per iteration one match
launch and one tail launch per k_icp_tail instantiation for all pairs.  Every pair's result is what ``run()`` returns for it, bit
for bit; the batch never picks a "best" pair -- several initial guesses of one pair are several members, each reported.

Unlike ``run()`` the inputs are not modified: the pairs' clouds are copied before their preparation.  A pair of CUDA torch tensors
takes the device road of ``run_tensors`` (simpleicp_amd/tensors.py) on its pool context: nothing coordinate-sized crosses the host
link, its iterations go through the same batched call, and its X_mov_transformed is a device tensor.
"""
from __future__ import annotations

import inspect
import logging
import time
from collections import namedtuple
from typing import Optional, Sequence

import numpy as np

from . import _lib, backend, dist, evaluation
from .icp import (EXTRA_DEFAULTS as _EXTRA_DEFAULTS, RunExtras, RunKeywords, SimpleICP, SimpleICPException, _HostSelection,
                  _movable_rows, _prepare, _rbp_and_residuals, _start_pose)
from .pointcloud import PointCloud, PointCloudException
from .rbp import H_from_params

_log = logging.getLogger(__name__)

# where the last run_batch call spent its time (seconds): the pairs' preparation on the host, the batched loops, the results
last_run_info: dict = {}

# run()'s keyword arguments and their defaults, read off its signature (a default changed there is the batch's as well)
_RUN_DEFAULTS = {name: prm.default for name, prm in inspect.signature(SimpleICP.run).parameters.items() if name != "self"}
# (_EXTRA_DEFAULTS, icp.EXTRA_DEFAULTS: the keywords of run_batch / run_tensors / the per_pair dicts that are not run()'s)


def merged_keywords(who, extras, run_kwargs, pair=None, check_arguments=True):
    """What one pair of ``who`` (run_batch / run_tensors) runs with: run()'s defaults and the call's options ``extras`` (the names
    of _EXTRA_DEFAULTS), overridden by the call's keywords, overridden by the pair's own (a dict or None) -- as (RunKeywords,
    RunExtras), refused as run() refuses them.  check_arguments False: RunKeywords.check() is left to the caller (run_batch
    reports a bad argument of run() as the pair's error, not as its own)."""
    kw = dict(_RUN_DEFAULTS, **extras)
    for src in (run_kwargs, pair or {}):
        unknown = set(src) - set(kw)
        if unknown:
            raise TypeError(f"{who} got unexpected keyword argument(s) {sorted(unknown)}")
        kw.update(src)
    if kw["debug_dirpath"]:
        raise SimpleICPException(f"{who} writes no debug files (debug_dirpath): run that pair with SimpleICP.run")
    run_kw = RunKeywords(**{name: kw[name] for name in _RUN_DEFAULTS})
    if check_arguments:
        run_kw.check()
    return run_kw, RunExtras.checked(**{name: kw[name] for name in _EXTRA_DEFAULTS})


class BatchResult(tuple):
    """One pair's outcome: unpacks like ``run()``'s ``(H, X_mov_transformed, rbp, residuals)``; besides ``iterations``,
    ``n_kept`` / ``res_mean`` / ``res_std`` of the last iteration, and ``error`` (None, or the exception ``run()`` would
    have raised for this pair -- then the four values are None), and ``evaluation`` (the Evaluation of the pair under its final H
    when evaluate_distance was set for it; None when it was not, and for a pair with ``error``), and ``outlier`` (the statistics
    of the pair's outlier removal -- n_candidates, n_kept, mean, std, threshold -- when outlier_neighbors was set for it, else None)."""

    def __new__(cls, H=None, X_mov_transformed=None, rbp=None, residuals=None, iterations=0, n_kept=0, res_mean=np.nan,
                res_std=np.nan, error=None, path=None, evaluation=None, outlier=None):
        self = super().__new__(cls, (H, X_mov_transformed, rbp, residuals))
        self.iterations, self.n_kept, self.res_mean, self.res_std = iterations, n_kept, res_mean, res_std
        self.error = error
        self.evaluation = evaluation
        self.outlier = outlier
        self.path = path          # "batched" / "fallback" (the pair ran through sicp_icp_run: Q > 2048 and the like) / "device" (run_tensors)
        return self

    @classmethod
    def of_run(cls, values, R, iterations, path, evaluation=None, outlier=None):
        """From what run() returns (``values``), the last iteration's record R (None: no iteration ran) and their number."""
        return cls(*values, iterations=iterations, n_kept=int(R.n_kept) if R is not None else 0,
                   res_mean=R.res_mean if R is not None else np.nan, res_std=R.res_std if R is not None else np.nan,
                   path=path, evaluation=evaluation, outlier=outlier)

    H = property(lambda self: self[0])
    X_mov_transformed = property(lambda self: self[1])
    rbp = property(lambda self: self[2])
    residuals = property(lambda self: self[3])


def _cloud(c) -> PointCloud:
    """A copy of a PointCloud, or a new one from an (n, 3) array."""
    if isinstance(c, PointCloud):
        return PointCloud(c.copy(deep=True))
    X = np.asarray(c, dtype=float)
    if X.ndim != 2 or X.shape[1] != 3:
        raise ValueError("a cloud must be a PointCloud or an (n, 3) array")
    return PointCloud(X, columns=["x", "y", "z"])


def _quiet(*_args, **_kw):
    pass


def run_batch(pairs: Sequence, *, per_pair: Optional[Sequence[Optional[dict]]] = None, return_transformed: bool = True,
              max_normal_angle: Optional[float] = None, voxel_size: Optional[float] = None, voxel_origin=None,
              evaluate_distance: Optional[float] = None, outlier_neighbors: Optional[int] = None, outlier_std_ratio: float = 2.0,
              **run_kwargs) -> list:
    """Registers every ``(fixed, movable)`` pair of ``pairs`` (PointClouds or (n, 3) arrays, or two CUDA torch tensors as for
    ``run_tensors``) with ``run()``'s keyword arguments ``run_kwargs``, overridden per pair by ``per_pair[i]`` (a dict or None).
    Returns one BatchResult per pair, in order.  ``return_transformed=False``: no X_mov_transformed (None), no download of the
    movable clouds (no egress of a device pair's).  ``max_normal_angle`` (degrees; also a key of the per_pair dicts): SimpleICP's
    attribute of that name -- a pair that has it runs its loop on its own (``path`` "fallback"), the others stay batched.
    ``voxel_size`` / ``voxel_origin`` (keys of the per_pair dicts too): SimpleICP's attributes of those names; only the pair's
    preparation changes, its loop stays batched.  ``evaluate_distance`` (a key of the per_pair dicts too; None = off): SimpleICP's
    attribute of that name -- the pair stays batched, after the batched loop it is scored under its final H on its pool context
    (``BatchResult.evaluation``).  ``outlier_neighbors`` / ``outlier_std_ratio`` (keys of the per_pair dicts too; None = off):
    SimpleICP's attributes of those names; only the pair's preparation changes, its loop stays batched
    (``BatchResult.outlier``)."""
    t0 = time.time()
    pairs = list(pairs)
    if per_pair is not None and len(per_pair) != len(pairs):
        raise ValueError(f"per_pair has {len(per_pair)} entries for {len(pairs)} pairs")
    if dist.is_distributed():
        raise SimpleICPException("run_batch does not run in a torch.distributed job: call SimpleICP.run on each rank instead")
    options = dict(max_normal_angle=max_normal_angle, voxel_size=voxel_size, voxel_origin=voxel_origin,
                   evaluate_distance=evaluate_distance, outlier_neighbors=outlier_neighbors, outlier_std_ratio=outlier_std_ratio)
    checked = [merged_keywords("run_batch", options, run_kwargs, per_pair[i] if per_pair is not None else None, check_arguments=False)
               for i in range(len(pairs))]
    if not pairs:
        return []
    on_device = [_device_pair(fix, mov) for fix, mov in pairs]
    if any(on_device):
        from . import tensors
        for (fix, mov), d in zip(pairs, on_device):
            if d:                          # (refused before any device work, like run_tensors' arguments)
                tensors._check_cloud("a fixed cloud", fix, backend.default_device())
                tensors._check_cloud("a movable cloud", mov, backend.default_device())

    ctxs = backend.get_batch_contexts(len(pairs))
    out = [None] * len(pairs)
    prepared = []
    members = []
    for i, ((fix, mov), (kw, extras)) in enumerate(zip(pairs, checked)):
        ctx = ctxs[i]
        ctx._corr_owner = None
        try:
            # (the evaluation's entry point is asked for before the pair's clouds are looked at, the other options' by _prepare)
            if extras.evaluate is not None:
                evaluation.need_backend(ctx)
            if on_device[i]:
                kw.check()
                extras.check_fixed_size(fix.shape[0])
                pose, stats, scratch = tensors.prepare(ctx, fix, mov, kw, extras, _quiet)
                pc2, msel, dev = None, None, (mov, scratch)
            else:
                pc1, pc2 = _cloud(fix), _cloud(mov)
                extras.check_fixed_size(pc1.num_points)
                kw.check()
                pose = _start_pose(kw)
                # SimpleICP.run's uploads on one GPU (the fixed cloud behind the caller, the movable one behind it)
                pc1._upload(ctx, _lib.FIX, background=True)
                selection = _HostSelection(ctx, pc1, pc2, *_movable_rows(pc2))
                pc2._upload(ctx, _lib.MOV, background=True)
                ctx.upload_wait(_lib.FIX)
                stats = _prepare(selection, kw, extras, pose[2], _quiet)
                msel, dev = selection.msel, None
        except (SimpleICPException, PointCloudException, _lib.BackendError) as e:
            # what run() would raise for this pair (no overlap, a non-finite coordinate, ...): the pair's error, the others go on
            out[i] = BatchResult(error=e)
            continue
        obs, ow, _ = pose
        members.append((ctx, dict(x=obs.copy(), obs=obs, obs_weight=ow, min_planarity=kw.min_planarity, distance_weight=kw.distance_weights,
                                  max_iterations=kw.max_iterations, min_change=kw.min_change)))
        prepared.append(_Prepared(i, ctx, pc2, msel, obs, ow, dev, extras.evaluate, stats))

    t1 = time.time()
    runs, fallback = members[0][0].icp_run_batch(members) if members else ([], 0)
    t2 = time.time()
    for p, r in zip(prepared, runs):
        out[p.i] = _result(p, r, return_transformed)
    last_run_info.clear()
    last_run_info.update(pairs=len(pairs), fallback=fallback, prepare_s=t1 - t0, batch_s=t2 - t1, results_s=time.time() - t2)
    n_err = sum(1 for o in out if o.error is not None)
    _log.info(f"run_batch: {len(pairs)} pairs ({len(members) - fallback} batched, {fallback} fallback, {n_err} failed) "
              f"in {time.time() - t0:.3f} seconds")
    return out


# a pair whose preparation went through, as its epilogue needs it -- i: its index; pc2, msel: its movable PointCloud and the rows of
# it that were searched (None: all); dev: (X_mov, scratch) of a device pair, else None; evaluate: its evaluate_distance or None;
# outlier: the statistics of its outlier removal or None
_Prepared = namedtuple("_Prepared", "i ctx pc2 msel obs ow dev evaluate outlier")


def _device_pair(fix, mov) -> bool:
    from .tensors import _is_device_tensor
    d = (_is_device_tensor(fix), _is_device_tensor(mov))
    if d[0] != d[1]:
        raise ValueError("a pair holds one CUDA tensor and one host cloud: both members go on the GPU (run_tensors) or both on the host")
    return d[0]


def _result(p, r, return_transformed) -> BatchResult:
    """SimpleICP.run's epilogue for the prepared member p and its BatchRun r: what run() returns, or the exception it raises (for a
    device pair run_tensors' epilogue: the transformed cloud is a new device tensor)."""
    ctx, obs = p.ctx, p.obs
    path = "fallback" if r.path == _lib.BATCH_PATH_FALLBACK else "batched"
    whole = r.results
    if r.status != _lib.OK:
        if r.status == _lib.ERR_TOO_FEW:
            err = SimpleICPException(str(_lib.BackendError(r.error, r.status)))
        else:
            err = _lib.BackendError(r.error, r.status)
            err.results = whole
        last = whole[-1] if whole else None
        return BatchResult(iterations=len(whole), n_kept=int(last.n_kept) if last else 0, error=err, path=path, outlier=p.outlier)
    R = whole[-1] if whole else None
    H, x_start, x = H_from_params(obs), None, None
    if R is not None:
        x_start = np.array(whole[-2].x[:]) if len(whole) > 1 else obs.copy()
        x = np.array(R.x[:])
        H = np.array(R.H[:]).reshape(4, 4)
    rbp, residuals = _rbp_and_residuals(ctx, R, obs, p.ow, x_start, x)
    # (before the movable slot is uploaded again / transformed below: both clouds are as the loop left them)
    ev = evaluation.after_run(ctx, H, p.evaluate) if p.evaluate is not None else None
    X_new = None
    if return_transformed and p.dev is not None:
        from . import tensors
        X_new = tensors.transformed(ctx, p.dev[0], H)
    elif return_transformed:
        if p.msel is not None:
            p.pc2._upload(ctx, _lib.MOV)
        ctx.transform(_lib.MOV, H)
        X_new, _ = ctx.download_both(_lib.MOV)     # (through the lean contexts' shared pinned ring, like run()'s download)
    return BatchResult.of_run((H, X_new, rbp, residuals), R, len(whole), path, ev, p.outlier)
