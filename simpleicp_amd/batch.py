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
from typing import Optional, Sequence

import numpy as np

from . import _lib, backend, dist, evaluation
from .icp import (SimpleICP, SimpleICPException, _cos_of_max_angle, _evaluate_distance_of, _rbp_and_residuals, _select_and_setup,
                  _check_outlier_size, _outlier_of, _voxel_of)
from .pointcloud import PointCloud, PointCloudException
from .rbp import H_from_params

_log = logging.getLogger(__name__)

# where the last run_batch call spent its time (seconds): the pairs' preparation on the host, the batched loops, the results
last_run_info: dict = {}

# run()'s keyword arguments and their defaults, read off its signature (a default changed there is the batch's as well)
_RUN_DEFAULTS = {name: prm.default for name, prm in inspect.signature(SimpleICP.run).parameters.items() if name != "self"}
# keywords of run_batch / run_tensors / the per_pair dicts that are not run()'s (SimpleICP carries them as attributes)
_EXTRA_DEFAULTS = {"max_normal_angle": None, "voxel_size": None, "voxel_origin": None, "evaluate_distance": None,
                   "outlier_neighbors": None, "outlier_std_ratio": 2.0}


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
    kws = []
    for i in range(len(pairs)):
        kw = dict(_RUN_DEFAULTS, max_normal_angle=max_normal_angle, voxel_size=voxel_size, voxel_origin=voxel_origin,
                  evaluate_distance=evaluate_distance, outlier_neighbors=outlier_neighbors, outlier_std_ratio=outlier_std_ratio)
        for src in (run_kwargs, (per_pair[i] or {}) if per_pair is not None else {}):
            unknown = set(src) - set(_RUN_DEFAULTS) - set(_EXTRA_DEFAULTS)
            if unknown:
                raise TypeError(f"run_batch got unexpected keyword argument(s) {sorted(unknown)}")
            kw.update(src)
        if kw["debug_dirpath"]:
            raise SimpleICPException("run_batch writes no debug files (debug_dirpath): run that pair with SimpleICP.run")
        _cos_of_max_angle(kw["max_normal_angle"])
        kw["voxel"] = _voxel_of(kw["voxel_size"], kw["voxel_origin"])
        kw["evaluate"] = _evaluate_distance_of(kw["evaluate_distance"])
        kw["outlier"] = _outlier_of(kw["outlier_neighbors"], kw["outlier_std_ratio"])
        kw["outlier_stats"] = {}
        kws.append(kw)
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
    prepared = []          # (pair index, ctx, pc2, msel, obs, ow, device pair: (X_mov, its scratch) or None, evaluate_distance or None, outlier statistics or None)
    members = []
    for i, ((fix, mov), kw) in enumerate(zip(pairs, kws)):
        ctx = ctxs[i]
        ctx._corr_owner = None
        try:
            if kw["evaluate"] is not None:
                evaluation.need_backend(ctx)
            if on_device[i]:
                SimpleICP._check_arguments(kw["distance_weights"], kw["rbp_observed_values"], kw["rbp_observation_weights"])
                _check_outlier_size(kw["outlier"], fix.shape[0])
                obs, ow, _, scratch = tensors.prepare(ctx, fix, mov, kw, _quiet)
                members.append((ctx, _member_kwargs(obs, ow, kw)))
                prepared.append((i, ctx, None, None, obs, ow, (mov, scratch), kw["evaluate"],
                                 kw["outlier_stats"] if kw["outlier"] is not None else None))
                continue
            pc1, pc2 = _cloud(fix), _cloud(mov)
            _check_outlier_size(kw["outlier"], pc1.num_points)
            SimpleICP._check_arguments(kw["distance_weights"], kw["rbp_observed_values"], kw["rbp_observation_weights"])
            obs = np.array(kw["rbp_observed_values"], dtype=float)
            obs[:3] = obs[:3] * np.pi / 180
            ow = np.array(kw["rbp_observation_weights"], dtype=float)
            H = H_from_params(obs)
            # SimpleICP.run's uploads on one GPU (the fixed cloud behind the caller, the movable one behind it)
            pc1._upload(ctx, _lib.FIX, background=True)
            partial = not bool(pc2["selected"].to_numpy().all())
            msel = pc2.idx_selected if partial else None
            if partial and not len(msel):
                raise SimpleICPException("The movable point cloud has no selected points.")
            n_search = len(msel) if partial else pc2.num_points

            def upload_movable(rows=None, pc2=pc2, ctx=ctx):
                n = pc2.num_points if rows is None else len(rows)
                pc2._upload(ctx, _lib.MOV, 0, n, index_base=0, rows=rows)

            sel0 = pc1._selection()
            pc2._upload(ctx, _lib.MOV, background=True)
            ctx.upload_wait(_lib.FIX)
            _select_and_setup(ctx, pc1, pc2, msel, n_search, upload_movable, sel0, H, kw["correspondences"], kw["neighbors"],
                              kw["max_overlap_distance"], info=_quiet, max_normal_angle=kw["max_normal_angle"], voxel=kw["voxel"],
                              outlier=kw["outlier"], outlier_stats=kw["outlier_stats"])
        except (SimpleICPException, PointCloudException, _lib.BackendError) as e:
            # what run() would raise for this pair (no overlap, a non-finite coordinate, ...): the pair's error, the others go on
            out[i] = BatchResult(error=e)
            continue
        members.append((ctx, _member_kwargs(obs, ow, kw)))
        prepared.append((i, ctx, pc2, msel, obs, ow, None, kw["evaluate"], kw["outlier_stats"] if kw["outlier"] is not None else None))

    t1 = time.time()
    runs, fallback = members[0][0].icp_run_batch(members) if members else ([], 0)
    t2 = time.time()
    for (i, ctx, pc2, msel, obs, ow, dev, eval_d, ostats), r in zip(prepared, runs):
        out[i] = _result(ctx, pc2, msel, obs, ow, r, return_transformed, dev, eval_d)
        out[i].outlier = ostats
    last_run_info.clear()
    last_run_info.update(pairs=len(pairs), fallback=fallback, prepare_s=t1 - t0, batch_s=t2 - t1, results_s=time.time() - t2)
    n_err = sum(1 for o in out if o.error is not None)
    _log.info(f"run_batch: {len(pairs)} pairs ({len(members) - fallback} batched, {fallback} fallback, {n_err} failed) "
              f"in {time.time() - t0:.3f} seconds")
    return out


def _device_pair(fix, mov) -> bool:
    from .tensors import _is_device_tensor
    d = (_is_device_tensor(fix), _is_device_tensor(mov))
    if d[0] != d[1]:
        raise ValueError("a pair holds one CUDA tensor and one host cloud: both members go on the GPU (run_tensors) or both on the host")
    return d[0]


def _member_kwargs(obs, ow, kw) -> dict:
    return dict(x=obs.copy(), obs=obs, obs_weight=ow, min_planarity=kw["min_planarity"], distance_weight=kw["distance_weights"],
                max_iterations=kw["max_iterations"], min_change=kw["min_change"])


def _result(ctx, pc2, msel, obs, ow, r, return_transformed, dev=None, eval_d=None) -> BatchResult:
    """SimpleICP.run's epilogue for one member: what it returns, or the exception it raises.  dev: (X_mov, scratch) of a device pair
    (run_tensors' epilogue: the transformed cloud is a new device tensor).  eval_d: the pair's evaluate_distance (None: off)."""
    path = "fallback" if r.path == _lib.BATCH_PATH_FALLBACK else "batched"
    whole = r.results
    if r.status != _lib.OK:
        if r.status == _lib.ERR_TOO_FEW:
            err = SimpleICPException(str(_lib.BackendError(r.error, r.status)))
        else:
            err = _lib.BackendError(r.error, r.status)
            err.results = whole
        last = whole[-1] if whole else None
        return BatchResult(iterations=len(whole), n_kept=int(last.n_kept) if last else 0, error=err, path=path)
    R = whole[-1] if whole else None
    H, x_start, x = H_from_params(obs), None, None
    if R is not None:
        x_start = np.array(whole[-2].x[:]) if len(whole) > 1 else obs.copy()
        x = np.array(R.x[:])
        H = np.array(R.H[:]).reshape(4, 4)
    rbp, residuals = _rbp_and_residuals(ctx, R, obs, ow, x_start, x)
    # (before the movable slot is uploaded again / transformed below: both clouds are as the loop left them)
    ev = evaluation.after_run(ctx, H, eval_d) if eval_d is not None else None
    X_new = None
    if return_transformed and dev is not None:
        from . import tensors
        X_new = tensors.transformed(ctx, dev[0], H)
    elif return_transformed:
        if msel is not None:
            pc2._upload(ctx, _lib.MOV)
        ctx.transform(_lib.MOV, H)
        X_new, _ = ctx.download_both(_lib.MOV)     # (through the lean contexts' shared pinned ring, like run()'s download)
    return BatchResult(H, X_new, rbp, residuals, iterations=len(whole), n_kept=int(R.n_kept) if R else 0,
                       res_mean=R.res_mean if R else np.nan, res_std=R.res_std if R else np.nan, path=path, evaluation=ev)
