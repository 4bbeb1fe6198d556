"""SimpleICP -- call-compatible with /root/reference/python/simpleicp/simpleicp.py:41-379.

Same constructor, ``add_point_clouds``, ``run(**kwargs)`` signature, return tuple, exceptions,
side effects on the two PointCloud objects and log lines as the reference; the per-iteration
work (match, point-to-plane distances, planarity + MAD rejection, least-squares estimate) is
ONE C-ABI call into the HIP library with both clouds resident in HBM for the whole run.

Differences by design (documented in DESIGN.md):
  * the movable cloud is never transformed back and forth on the host (simpleicp.py:188,202):
    the transform is fused into the GPU scan, so the reference's ulp-level coordinate drift
    does not occur;
  * the NLLS problem of optimization.py:93-101 is minimised by Levenberg-Marquardt on fused
    6x6 normal-equation reductions instead of lmfit/scipy TRF with a finite-difference
    Jacobian -- same objective, same minimiser (tests pin H against the reference);
  * under torch.distributed (world_size > 1) the movable cloud is sharded across the GPUs.
"""
from __future__ import annotations

import inspect
import logging
import math
import os
import time
from collections import namedtuple
from dataclasses import dataclass, fields
from pathlib import Path
from typing import Optional, Tuple

import numpy as np

from . import _lib, backend, dist, evaluation
from .pointcloud import _ALL, PointCloud, voxel_arguments
from .rbp import H_from_params, RigidBodyParameters

_log = logging.getLogger(__name__)
_PKG_LOG = logging.getLogger(__package__)
_ATTRS = ("nx", "ny", "nz", "planarity")

# the options that are not run()'s arguments (its signature is the reference's): SimpleICP's attributes of these names, keywords of
# run_batch / run_tensors and keys of the per_pair dicts, with the values those keywords default to
EXTRA_DEFAULTS = {"max_normal_angle": None, "voxel_size": None, "voxel_origin": None, "evaluate_distance": None,
                  "outlier_neighbors": None, "outlier_std_ratio": 2.0}


class SimpleICPException(Exception):
    """Raised when the SimpleICP class is misused (simpleicp.py:382)."""


def _enable_verbose_logging() -> None:
    """INFO to stdout, once (simpleicp.py:25-38)."""
    _PKG_LOG.setLevel(logging.INFO)
    for h in _PKG_LOG.handlers:
        if getattr(h, "_simpleicp_verbose", False):
            return
    h = logging.StreamHandler()
    h.setFormatter(logging.Formatter("%(message)s"))
    h._simpleicp_verbose = True
    _PKG_LOG.addHandler(h)


def _percent_change(new: float, old: float) -> float:
    if old == 0:
        return 0.0 if new == 0 else np.inf
    return abs((new - old) / old * 100)


def _no_overlap(max_overlap_distance) -> SimpleICPException:
    return SimpleICPException(
        "Point clouds do not overlap within max_overlap_distance = "
        f"{max_overlap_distance:.5f}! Consider increasing the value of "
        "max_overlap_distance."
    )


def _cos_of_max_angle(max_normal_angle):
    """max_normal_angle (degrees, None = no such rejection) -> the cos_max of contract (N), computed once; 0 < angle <= 90."""
    if max_normal_angle is None:
        return None
    try:
        ok = 0.0 < float(max_normal_angle) <= 90.0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise SimpleICPException("max_normal_angle must be an angle in degrees, > 0 and <= 90.")
    return math.cos(math.radians(float(max_normal_angle)))


def _voxel_of(voxel_size, voxel_origin=None):
    """voxel_size (None = no voxel selection) and voxel_origin -> (cell, origin) of contract (V), checked once."""
    if voxel_size is None:
        return None
    return voxel_arguments(voxel_size, voxel_origin, SimpleICPException)


def _evaluate_distance_of(evaluate_distance):
    """evaluate_distance (None = no evaluation) -> the search bound of contract (E), checked once."""
    if evaluate_distance is None:
        return None
    return evaluation._distance_of(evaluate_distance, SimpleICPException, "evaluate_distance")


def _outlier_of(outlier_neighbors, outlier_std_ratio=2.0):
    """outlier_neighbors (None = no outlier removal) and outlier_std_ratio -> (k, std_ratio) of contract (O), checked once."""
    if outlier_neighbors is None:
        return None
    k, ok = 0, not isinstance(outlier_neighbors, (bool, str, bytes, float))
    if ok:
        try:
            k = int(outlier_neighbors)
            ok = k == outlier_neighbors and 2 <= k <= _lib.OUTLIER_MAX_K
        except (TypeError, ValueError):
            ok = False
    if not ok:
        raise SimpleICPException(f"outlier_neighbors must be an integer >= 2 and <= {_lib.OUTLIER_MAX_K}.")
    try:
        ratio = float(outlier_std_ratio)
        ok = not isinstance(outlier_std_ratio, (bool, str, bytes)) and math.isfinite(ratio)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise SimpleICPException("outlier_std_ratio must be a finite number.")
    return k, ratio


def _check_outlier_size(outlier, n_fix):
    """The neighbour count against the fixed cloud's size: refused like the option's other argument errors, before any upload."""
    if outlier is not None and outlier[0] > n_fix:
        raise SimpleICPException(f"outlier_neighbors ({outlier[0]}) exceeds the number of points of the fixed point cloud ({n_fix}).")


@dataclass(frozen=True)
class RunExtras:
    """The checked values of the options of EXTRA_DEFAULTS: what a run gets besides run()'s arguments, on every road."""
    max_normal_angle: Optional[float] = None
    cos_max: Optional[float] = None           # of max_normal_angle, contract (N); None = no such rejection
    voxel: Optional[tuple] = None             # (cell, origin) of contract (V); None = no voxel selection
    evaluate: Optional[float] = None          # the search bound of contract (E); None = no evaluation
    outlier: Optional[tuple] = None           # (k, std_ratio) of contract (O); None = no outlier removal

    @classmethod
    def checked(cls, max_normal_angle=None, voxel_size=None, voxel_origin=None, evaluate_distance=None, outlier_neighbors=None,
                outlier_std_ratio=2.0):
        """From the raw values (the names of EXTRA_DEFAULTS).  Of several bad ones the first in this order is reported: the angle,
        the voxels, the evaluation, the outliers."""
        return cls(max_normal_angle, _cos_of_max_angle(max_normal_angle), _voxel_of(voxel_size, voxel_origin),
                   _evaluate_distance_of(evaluate_distance), _outlier_of(outlier_neighbors, outlier_std_ratio))

    def check_fixed_size(self, n_fix):
        _check_outlier_size(self.outlier, n_fix)

    def refuse_sharded(self):
        """In a torch.distributed job none of the three runs."""
        for on, name, instead in ((self.voxel, "voxel_size", "thin the clouds with one process first"),
                                  (self.outlier, "outlier_neighbors", "thin the clouds with one process first"),
                                  (self.evaluate, "evaluate_distance", "score the result with one process")):
            if on is not None:
                raise SimpleICPException(f"{name} does not run in a torch.distributed job: {instead}")

    def need_backend(self, ctx):
        """A backend (a stand-in) without the entry point of an option that is on is an error, never a run without the option.
        (The rejection by the angle between normals is refused where it is set: _set_normal_angle.)"""
        for on, entry, what in ((self.voxel, "voxel_select", "voxel selection"), (self.outlier, "outlier_statistical", "outlier removal")):
            if on is not None and not hasattr(ctx, entry):
                raise _lib.BackendError(f"this backend has no {what}")
        if self.evaluate is not None:
            evaluation.need_backend(ctx)


def _start_pose(kw):
    """(obs, ow, H): the observed parameter values in radians, their weights, and the pose the run starts from."""
    obs = np.array(kw.rbp_observed_values, dtype=float)
    obs[:3] = obs[:3] * np.pi / 180                       # degree -> rad (simpleicp.py:146-148)
    ow = np.array(kw.rbp_observation_weights, dtype=float)
    return obs, ow, H_from_params(obs)


def _movable_rows(pc2):
    """(msel, n_search): the rows of the movable cloud that are searched (None: all of them) and their number.  CorrPts.match
    searches pc2.X_selected only and maps the hits through pc2.idx_selected (corrpts.py:131-135); a movable cloud with a partial
    `selected` mask (e.g. the fixed cloud of an earlier run) is uploaded as that subset, after the overlap pre-pass, which looks at
    ALL its points (simpleicp.py:157: pc2.X)."""
    partial = not bool(pc2["selected"].to_numpy().all())
    msel = pc2.idx_selected if partial else None
    if partial and not len(msel):
        raise SimpleICPException("The movable point cloud has no selected points.")
    return msel, (len(msel) if partial else pc2.num_points)


def _set_normal_angle(ctx, cos_max, neighbors, pc2=None, msel=None, n_search=0):
    """The context's normal-angle setting for the run about to start -- set on every run, off (cos_max None) included, so that a
    pooled context never inherits it --, with pc2's own nx, ny, nz columns when it has them (of the selected subset when pc2 is
    partially selected; without them the normals are estimated on the device among the points of the movable slot, i.e. of that
    subset)."""
    if not hasattr(ctx, "normal_angle_set"):
        # (a stand-in backend that predates the setting has nothing to switch off; asked to switch it on, it cannot)
        if cos_max is not None:
            raise _lib.BackendError("this backend has no rejection by the angle between normals")
        return
    if cos_max is not None and pc2 is not None and {"nx", "ny", "nz"}.issubset(pc2.columns):
        nv = np.column_stack([np.asarray(pc2[c].to_numpy(), dtype=np.float32) for c in ("nx", "ny", "nz")])
        ctx.set_normals(_lib.MOV, nv if msel is None else nv[msel], n_global=n_search)
    ctx.normal_angle_set(cos_max, neighbors)


class _HostSelection:
    """The fixed cloud's selection of a pair of PointClouds, for _prepare: pc1's `selected` column, carried along as ``sel``
    (_ALL or an index array: every pass over the mask is a pass over N_f).  msel, n_search: _movable_rows(pc2).
    upload_movable(rows): how a sharded run uploads the movable cloud's subset (None: one GPU, the whole subset)."""

    def __init__(self, ctx, pc1, pc2, msel, n_search, upload_movable=None):
        self.ctx, self.pc1, self.pc2, self.msel, self.n_search = ctx, pc1, pc2, msel, n_search
        self.upload_movable = upload_movable or (lambda rows: pc2._upload(ctx, _lib.MOV, rows=rows))
        self.sel = pc1._selection()

    def _rows(self):
        return None if self.sel is _ALL else self.sel

    def is_empty(self):
        return not (self.sel is _ALL or len(self.sel) > 0)

    def overlap(self, H, d):
        if not self.is_empty():
            # both clouds are resident already: only the verdicts cross the host link
            self.sel = self.pc1._keep_selected(self.sel, self.ctx.select_in_range(_lib.FIX, _lib.MOV, self._rows(), H, d))

    def outliers(self, k, std_ratio):
        keep, _, st = self.ctx.outlier_statistical(_lib.FIX, k, std_ratio, rows=self._rows())
        self.sel = self.pc1._keep_selected(self.sel, keep)
        return st

    def voxels(self, cell, origin):
        if not self.is_empty():
            self.sel = self.pc1._keep_selected(self.sel, self.ctx.voxel_select(_lib.FIX, cell, origin, self._rows()))

    def pick_and_setup(self, kw, extras, info):
        ctx, pc1, pc2, msel = self.ctx, self.pc1, self.pc2, self.msel
        info("Select points for correspondences in fixed point cloud ...")
        sel = self.sel = pc1.select_n_points(kw.correspondences, _cur=self.sel)
        # (simpleicp.py:174,254 save and restore pc1's selection around every iteration because the
        # reference's rejections edit it; here the masks live on the device and pc1 is never touched)
        if not set(_ATTRS).issubset(pc1.columns):
            info("Estimate normals of selected points ...")
            pc1.estimate_normals(kw.neighbors, _ctx=ctx, _uploaded=True, _sel=sel)
        normals, planarity = pc1._attributes_of(sel)
        ctx.upload_wait(_lib.MOV)                # (the movable cloud's verdict -- a non-finite coordinate -- is raised here)
        if msel is not None:
            self.upload_movable(msel)            # from here on the searched cloud is pc2's selected subset
        if "planarity" in pc2.columns:
            # reject_wrt_planarity tests pc2's column as well when it exists (corrpts.py:158-163; NaN fails)
            rows, vals = pc2._planarity_pairs(msel)
            ctx.set_planarity(_lib.MOV, vals, rows=rows, n_global=self.n_search)
        _set_normal_angle(ctx, extras.cos_max, kw.neighbors, pc2, msel, self.n_search)
        ctx.icp_setup(sel, normals, planarity)


class _DeviceSelection:
    """The fixed cloud's selection of a pair uploaded from device memory (run_tensors, run_batch's device pairs; every point
    selected to start with, no normals or planarity columns), for _prepare: a u8 mask in device memory (none: every point), so
    that every array the steps hand on stays there -- the overlap verdicts, the kept rows and the picks of select_n_points
    (sicp_select_n_device), the normals.  alloc(shape, kind) returns a device buffer (kind "u8" / "i64" / "f32") and its address;
    the buffers of the pick are kept in ``scratch``, which must outlive the run's sicp_icp_setup."""

    def __init__(self, ctx, n_fix, alloc):
        self.ctx, self.n_fix, self.alloc = ctx, n_fix, alloc
        self.mask = self.mask_p = self.scratch = None

    def _new_mask(self):
        self.mask, self.mask_p = self.alloc((self.n_fix,), "u8")
        return self.mask_p

    def is_empty(self):
        return False                  # (not known on the host before the pick: pick_and_setup tells)

    def overlap(self, H, d):
        self.ctx.select_in_range_into(_lib.FIX, _lib.MOV, H, d, self._new_mask())

    def outliers(self, k, std_ratio):
        if self.mask is None:
            return self.ctx.outlier_statistical(_lib.FIX, k, std_ratio, keep_ptr=self._new_mask())
        return self.ctx.outlier_statistical(_lib.FIX, k, std_ratio, mask_ptr=self.mask_p, keep_ptr=self.mask_p)   # (the verdicts replace the mask)

    def voxels(self, cell, origin):
        if self.mask is None:
            self.ctx.voxel_select(_lib.FIX, cell, origin, keep_ptr=self._new_mask())
        else:
            self.ctx.voxel_select_masked(_lib.FIX, self.mask_p, self.n_fix, cell, origin)      # (the verdicts replace the mask)

    def pick_and_setup(self, kw, extras, info):
        ctx, alloc = self.ctx, self.alloc
        sel, sel_p = alloc((max(int(kw.correspondences), 1),), "i64")
        Q = ctx.select_n_device(self.mask_p, self.n_fix, int(kw.correspondences), sel_p)
        if self.mask is not None and Q == 0:
            raise _no_overlap(kw.max_overlap_distance)
        info("Select points for correspondences in fixed point cloud ...")
        info("Estimate normals of selected points ...")
        nv, nv_p = alloc((Q, 3), "f32")
        pl, pl_p = alloc((Q,), "f32")
        ctx.estimate_normals_into(_lib.FIX, sel_p, Q, int(kw.neighbors), nv_p, pl_p)
        _set_normal_angle(ctx, extras.cos_max, kw.neighbors)
        ctx.icp_setup_device(sel_p, Q, nv_p, pl_p)
        self.mask = self.mask_p = None            # (every call returned complete: nothing reads the mask any more)
        self.scratch = (sel, nv, pl)


def _prepare(selection, kw, extras, H, info=None):
    """What a run does between the uploads and its first iteration, on every road (SimpleICP.run, run_batch, run_tensors), in this
    order: overlap pre-pass under the initial H, statistical outlier removal, one point per voxel, select_n_points, normals,
    the normal-angle setting, sicp_icp_setup -- the last four behind selection.pick_and_setup.  selection: a _HostSelection or a
    _DeviceSelection; info: where the progress lines go (the log).  Returns the statistics of the outlier removal (None: off)."""
    info = info or _log.info
    extras.need_backend(selection.ctx)
    bounded = np.isfinite(kw.max_overlap_distance)
    if bounded:
        info("Consider partial overlap of point clouds ...")
        selection.overlap(H, float(kw.max_overlap_distance))
        if selection.is_empty():
            raise _no_overlap(kw.max_overlap_distance)
    stats = None
    if extras.outlier is not None:
        # after the overlap pre-pass (only points that can take part are judged), before the voxel step (a voxel's representative
        # is then always an inlier); the neighbours are searched among ALL points of the fixed cloud
        if selection.is_empty():
            raise SimpleICPException("The fixed point cloud has no selected points left for the outlier removal.")
        stats = _lib._stats_dict(selection.outliers(*extras.outlier))
        info(f"Remove statistical outliers ... kept {stats['n_kept']} of {stats['n_candidates']} points "
             f"(mean {stats['mean']:.5f}, std {stats['std']:.5f}, threshold {stats['threshold']:.5f})")
    if extras.voxel is not None:
        # after the overlap pre-pass, so that a voxel's representative always lies inside the overlap
        info("Keep one point per voxel ...")
        selection.voxels(*extras.voxel)
        if selection.is_empty():
            # (reachable only with no selected point to start from; the exception an empty overlap raises, with words of its own)
            if bounded:
                raise _no_overlap(kw.max_overlap_distance)
            raise SimpleICPException("The fixed point cloud has no selected points left for the voxel selection.")
    # The two roads differ from here on, and each keeps its ways.  The host road knows above whether anything is left (with words
    # of its own where no overlap bound is to blame) and logs "Select points ..." before it picks.  The device road learns the
    # count only from its pick: whatever emptied the mask, it raises _no_overlap then, and logs "Select points ..." after it.
    selection.pick_and_setup(kw, extras, info)
    return stats


def _iterate(ctx, obs, ow, H, kw, hooks=None):
    """The iterations of a run (kw: its RunKeywords) after sicp_icp_setup, with run()'s log lines.  hooks None: ONE sicp_icp_run (same convergence test)
    whose records are replayed; (before(it, H), after(it, H)): a debug run, one ABI call per iteration with the hooks around it.
    Returns (R, x_start, x, H, stats, it) of the last iteration (R None when none ran)."""
    x = obs.copy()
    min_planarity, max_iterations, min_change = kw.min_planarity, kw.max_iterations, kw.min_change
    w = kw.distance_weights
    stats = []            # (n, mean, std) of the residuals per iteration
    R = None
    x_start = None
    it = -1
    _log.info("Start iterations ...")

    def too_few(e):
        if e.code == _lib.ERR_TOO_FEW:
            raise SimpleICPException(str(e)) from None
        raise e

    # without debug dumps nothing on the host needs the intermediate states: the whole loop runs behind
    # ONE ABI call (sicp_icp_run, same convergence test) and the per-iteration log is replayed below
    whole, failed = None, None
    if hooks is None:
        try:
            whole = ctx.icp_run(x, obs, ow, min_planarity, w, max_iterations, min_change)
        except _lib.BackendError as e:
            if e.code != _lib.ERR_TOO_FEW:
                raise
            whole, failed = e.results[:-1], e          # log the iterations before the failing one first
    for it in range(0, max_iterations if whole is None else len(whole)):
        if hooks is not None:
            hooks[0](it, H)
        x_start = x.copy()
        if whole is not None:
            R = whole[it]
        else:
            try:
                R = ctx.icp_iterate(x, obs, ow, min_planarity, w)
            except _lib.BackendError as e:
                too_few(e)
        if hooks is not None:
            hooks[1](it, H)
        if w is None:
            w = R.weight_used                            # frozen after iteration 0 (simpleicp.py:229-234)
        x = np.array(R.x[:])
        H = np.array(R.H[:]).reshape(4, 4)
        stats.append((int(R.n_kept), R.res_mean, R.res_std))

        if it > 0 and SimpleICP._converged(stats[it], stats[it - 1], min_change):
            _log.info("Convergence criteria fulfilled -> stop iteration!")
            break

        if it == 0:
            _log.info(f"{'Iteration':>9s} | {'correspondences':>15s} | {'mean(residuals)':>15s} | "
                      f"{'std(residuals)':>15s}")
            _log.info(f"{'orig:0':>9s} | {int(R.n_kept):15d} | {R.dist_mean:15.4f} | {R.dist_std:15.4f}")
        _log.info(f"{it + 1:9d} | {stats[it][0]:15d} | {stats[it][1]:15.4f} | {stats[it][2]:15.4f}")

    if failed is not None:
        too_few(failed)
    return R, x_start, x, H, stats, it


def _rbp_and_residuals(ctx, R, obs, ow, x_start, x):
    """The RigidBodyParameters and the residuals run() returns after its last iteration R (None: no iteration ran)."""
    rbp = RigidBodyParameters()
    rbp.set_parameter_attributes_from_list("observed_value", list(obs))
    rbp.set_parameter_attributes_from_list("observation_weight", list(ow))
    residuals = np.empty(0)
    if R is not None:
        rbp.set_parameter_attributes_from_list("initial_value", list(x_start))
        rbp.set_parameter_attributes_from_list("estimated_value", list(x))
        sigma = ctx.icp_uncertainties()
        for name, s, free in zip(("alpha1", "alpha2", "alpha3", "tx", "ty", "tz"), sigma, np.isfinite(ow)):
            if free:
                getattr(rbp, name).estimated_uncertainty = float(s)
        _, _, keep, res = ctx.icp_state(pc2_idx=False, dist=False)
        residuals = res[keep]
    return rbp, residuals


class SimpleICP:
    # Rejection by the angle between normals: degrees, 0 < angle <= 90; None = off.  An attribute, set after
    # construction (``icp.max_normal_angle = 30.0``), because run()'s signature is the reference's.  A correspondence whose fixed and
    # matched movable normals (unoriented) enclose a larger angle is dropped together with the planarity test.  The movable normals
    # are pc2's nx / ny / nz columns when it has them, else they are estimated on the device with run()'s ``neighbors`` among the
    # points of the movable cloud that take part in the search (its selected subset when it is partially selected).
    max_normal_angle: Optional[float] = None
    # Voxel selection: a cell size, None = off.  After the overlap pre-pass and before select_n_points the
    # fixed cloud's selection is thinned to the lowest-index point of every voxel of the lattice (cell voxel_size, origin
    # voxel_origin), so the correspondences are even in space, not in index.  Attributes for the same reason as max_normal_angle.
    voxel_size: Optional[float] = None
    voxel_origin: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    # Evaluation: a distance, None = off.  After the last iteration, while both clouds are still resident,
    # EVERY point of the fixed cloud (selected or not) searches its nearest neighbour among the movable cloud under the final H,
    # strictly within this distance; the Evaluation (fitness, inlier RMSE, information matrix) goes to ``self.evaluation`` and
    # ``last_run_info["evaluation"]``.  A movable cloud that was uploaded as its selected subset (a partial `selected` mask) is
    # searched as that subset.  H, rbp, the residuals and the transformed cloud are the same bits either way.  An attribute for
    # the same reason as max_normal_angle.
    evaluate_distance: Optional[float] = None
    # Statistical outlier removal: a neighbour count, None = off.  After the overlap pre-pass and before the
    # voxel step the fixed cloud's selection loses every point whose mean distance to its outlier_neighbors nearest points of the
    # fixed cloud (itself included) exceeds mean + outlier_std_ratio * std over the selection -- contract (O).  The statistics go to
    # ``last_run_info["outlier"]``.  The movable cloud is thinned by the caller.  Attributes for the same reason as max_normal_angle.
    outlier_neighbors: Optional[int] = None
    outlier_std_ratio: float = 2.0

    def __init__(self, verbose: bool = True) -> None:
        self.pc1: Optional[PointCloud] = None
        self.pc2: Optional[PointCloud] = None
        self.last_run_info: dict = {}
        self.evaluation: Optional[evaluation.Evaluation] = None      # of the last run that had evaluate_distance set
        if verbose:
            _enable_verbose_logging()

    def add_point_clouds(self, pc_fix: PointCloud, pc_mov: PointCloud) -> None:
        self.pc1 = pc_fix      # fixed
        self.pc2 = pc_mov      # movable: gets transformed

    # --------------------------------------------------------------------------------------
    def run(
        self,
        correspondences: int = 1000,
        neighbors: int = 10,
        min_planarity: float = 0.3,
        max_overlap_distance: float = np.inf,
        min_change: float = 1.0,
        max_iterations: int = 100,
        distance_weights: Optional[float] = 1,
        rbp_observed_values: Tuple[float] = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
        rbp_observation_weights: Tuple[float] = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
        debug_dirpath: str = "",
    ) -> Tuple[np.ndarray, np.ndarray, RigidBodyParameters, np.ndarray]:
        """See the reference docstring (simpleicp.py:88-133): identical arguments/returns.
        Returns (H, X_mov_transformed, rbp, distance_residuals)."""
        kw = RunKeywords(correspondences, neighbors, min_planarity, max_overlap_distance, min_change, max_iterations,
                         distance_weights, rbp_observed_values, rbp_observation_weights, debug_dirpath)
        kw.check()
        extras = RunExtras.checked(**{name: getattr(self, name) for name in EXTRA_DEFAULTS})
        t_start = time.time()
        pc1, pc2 = self.pc1, self.pc2
        extras.check_fixed_size(pc1.num_points)
        ctx = backend.get_context()
        ctx._corr_owner = None            # (an operator-level CorrPts object loses the device state to this run)
        sharded = dist.is_distributed() or (os.environ.get("SICP_FORCE_EXCHANGE") == "1" and dist.is_initialized())
        if sharded:
            extras.refuse_sharded()
        extras.need_backend(ctx)
        self.evaluation = None

        if debug_dirpath:
            _log.info(f'Write debug files to directory "{debug_dirpath}"')
            Path(debug_dirpath).mkdir(parents=True, exist_ok=True)

        pose = _start_pose(kw)

        # both clouds go to HBM once and stay there (straight from the frames' storage: no host gather).  One process: each travels
        # on the library's helper thread (a stream of its own) while this thread does what needs no device -- the masks -- and, behind
        # the movable cloud's upload, the fixed cloud's grid and normals; the first call that names a slot waits for its upload
        pc1._upload(ctx, _lib.FIX, background=not sharded)
        msel, n_search = _movable_rows(pc2)
        rank, world = dist.rank_world() if sharded else (0, 1)

        # what the ranks shard: index ranges of the movable cloud by default; the QUERIES (cloud
        # replicated on every rank) when the match dominates, i.e. for large correspondence counts
        # ... and only when a whole copy of the cloud (+ its grid) fits comfortably in every rank's free memory; a cloud that
        # only fits in shards stays sharded whatever the correspondence count (the verdict is the same on every rank of a
        # homogeneous node; SICP_PARTITION pins it explicitly)
        # ... and always when the searched cloud has fewer rows than there are ranks: some index shard would be empty, which an
        # upload refuses -- on those ranks alone, while the others went on into the run's collectives.  Every rank knows both
        # numbers, so all of them take the replicated cloud together (n_search <= pc2.num_points covers the first upload too)
        qshard = sharded and (n_search < world or os.environ.get("SICP_PARTITION", "") == "queries"
                              or (os.environ.get("SICP_PARTITION", "") != "cloud" and correspondences >= 100_000
                                  and dist.agree(dist.queries_partition_fits(ctx, n_search))))

        def upload_movable(rows=None):
            n = pc2.num_points if rows is None else len(rows)
            lo, hi = (0, n) if qshard else dist.shard_bounds(n, rank, world)
            pc2._upload(ctx, _lib.MOV, lo, hi, index_base=lo, rows=rows)

        selection = _HostSelection(ctx, pc1, pc2, msel, n_search, upload_movable)
        if sharded:
            upload_movable()
        else:
            pc2._upload(ctx, _lib.MOV, background=True)       # (waits for the fixed cloud's: one helper at a time)
            ctx.upload_wait(_lib.FIX)                         # ... whose verdict (a non-finite coordinate) is raised here
        self._job = {"ranks": world, "partition": None, "exchange": None}
        if sharded:
            how = dist.attach(ctx, gn_shard=(not qshard) and os.environ.get("SICP_GN_SHARD", "") != "0"
                              and (correspondences >= 262144 or os.environ.get("SICP_GN_SHARD") == "1"),
                              partition=_lib.PART_QUERIES if qshard else _lib.PART_CLOUD)
            self._job.update(partition="queries" if qshard else "cloud", exchange=how)
        else:
            dist.detach(ctx)
        try:
            return self._run_uploaded(selection, kw, extras, pose, sharded, t_start)
        except BaseException:
            # ANY way out of a sharded run that is not its normal end (a backend error, a host-side exception between two
            # collectives, KeyboardInterrupt, MemoryError) may leave this rank out of step with its peers: never revive the
            # communicator such a run used
            if sharded:
                dist.forget(ctx)
            raise
        finally:
            # the exchange lives on the process-wide context: a later standalone PointCloud operator must not issue a
            # collective the other ranks never join
            dist.detach(ctx)

    def _run_uploaded(self, selection, kw, extras, pose, sharded, t_start):
        ctx, pc1, pc2, msel = selection.ctx, self.pc1, self.pc2, selection.msel
        obs, ow, H = pose
        debug_dirpath = kw.debug_dirpath
        if debug_dirpath:
            X_fix, X_mov = pc1.X, pc2.X

        outlier_stats = _prepare(selection, kw, extras, H)

        hooks = None
        if debug_dirpath:
            def before(it, H):
                if it == 0:
                    pc1.write_xyz(Path(debug_dirpath).joinpath(f"iteration{it:03d}_preoptim_pcfix.xyz"))
                self._write_cloud(Path(debug_dirpath).joinpath(f"iteration{it:03d}_preoptim_pcmov.xyz"), X_mov, H)

            def after(it, H):
                self._write_correspondences(ctx, Path(debug_dirpath).joinpath(
                    f"iteration{it:03d}_preoptim_correspondences.xyz"), X_fix, X_mov if msel is None else X_mov[msel], selection.sel, H)
            hooks = (before, after)
        R, x_start, x, H, stats, it = _iterate(ctx, obs, ow, H, kw, hooks)
        rbp, residuals = _rbp_and_residuals(ctx, R, obs, ow, x_start, x)
        # (read before the final transform of the movable slot, which empties the cache of estimated normals)
        angle_info = ctx.normal_angle_info() if hasattr(ctx, "normal_angle_info") else {}

        self._log_result(H, rbp)
        if extras.evaluate is not None:
            # (before the movable slot is uploaded again / transformed below: both clouds are as the loop left them)
            self.evaluation = evaluation.after_run(ctx, H, extras.evaluate, _log.info)

        # final transformation of the caller's movable cloud (simpleicp.py:316): all of its points
        if sharded or msel is not None:
            pc2._upload(ctx, _lib.MOV)
        X_new = pc2._transform(H, ctx, _lib.MOV)
        if debug_dirpath:
            pc2.write_xyz(Path(debug_dirpath).joinpath(f"iteration{it:03d}_postoptim_pcmov.xyz"))

        self.last_run_info = {"iterations": it + 1, "stats": stats, "seconds": time.time() - t_start, **getattr(self, "_job", {})}
        self.last_run_info.update(angle_info)
        if extras.evaluate is not None:
            self.last_run_info["evaluation"] = self.evaluation
        if outlier_stats is not None:
            self.last_run_info["outlier"] = outlier_stats
        if sharded:
            # how the shards' winners met: "records_allgather" / "key_allreduces" (cloud shards) / "query_slices", and how often
            xi = ctx.exchange_info()
            self.last_run_info.update(winner_exchange=xi["form"], exchanges=xi["count"])
        _log.info(f"Finished in {time.time() - t_start:.3f} seconds!")
        return H, X_new, rbp, residuals

    # --------------------------------------------------------------------------------------
    @staticmethod
    def _converged(new, old, min_change) -> bool:
        """simpleicp.py:356-379 on (n, mean, std) triples."""
        return (_percent_change(new[1], old[1]) < min_change) and (_percent_change(new[2], old[2]) < min_change)

    @staticmethod
    def _write_cloud(file, X, H):
        Xh = np.column_stack((X, np.ones(len(X))))
        Xt = (H @ Xh.T).T[:, :3]
        from . import io
        io.write_xyz(file, Xt, decimals=3, header="//X Y Z")

    @staticmethod
    def _write_correspondences(ctx, file, X_fix, X_mov, sel, H):
        """corrpts.py:213-237: kept correspondences, movable points in the pre-optimisation pose."""
        idx, d, keep, _ = ctx.icp_state(residual=False)
        p2 = X_mov[idx[keep]]
        p2 = (H @ np.column_stack((p2, np.ones(len(p2)))).T).T[:, :3]
        from . import io
        io.write_xyz(file, np.column_stack((X_fix[sel[keep]], p2, d[keep])), decimals=-1,
                     header="//X1 Y1 Z1 X2 Y2 Z2 point_to_plane_distance")

    @staticmethod
    def _log_result(H, rbp):
        _log.info("Estimated transformation matrix H:")
        for r in range(4):
            _log.info(f"[{H[r, 0]:12.6f} {H[r, 1]:12.6f} {H[r, 2]:12.6f} {H[r, 3]:12.6f}]")
        _log.info("... which corresponds to the following rigid-body transformation parameters:")
        _log.info(f"{'parameter':>9s} | {'est.value':>15s} | {'est.uncertainty':>15s} | {'obs.value':>15s} | "
                  f"{'obs.weight':>15s}")
        for f in fields(rbp):
            p = getattr(rbp, f.name)
            _log.info(f"{f.name:>9s} | {p.estimated_value_scaled:15.6f} | {p.estimated_uncertainty_scaled:15.6f} | "
                      f"{p.observed_value_scaled:15.6f} | {p.observation_weight:15.3e}")
        _log.info("(Unit of est.value, est.uncertainty, and obs.value for alpha1/2/3 is degree)")

    @staticmethod
    def _check_arguments(distance_weights, rbp_observed_values, rbp_observation_weights):
        """simpleicp.py:327-353 -- same checks, same messages."""
        if distance_weights is not None and distance_weights <= 0:
            raise SimpleICPException("distance_weights must be > 0.")
        if len(rbp_observed_values) != 6:
            raise SimpleICPException("rbp_observed_values must have exactly 6 elements.")
        if len(rbp_observation_weights) != 6:
            raise SimpleICPException("rbp_observation_weights must have exactly 6 elements.")
        if not all(w >= 0 for w in rbp_observation_weights):
            raise SimpleICPException("All elements of rbp_observation_weights must be >= 0.")
        if not any(np.isfinite(rbp_observation_weights)):
            raise SimpleICPException("At least one element in rbp_observation_weights must be finite.")


class RunKeywords(namedtuple("RunKeywords", [name for name in inspect.signature(SimpleICP.run).parameters if name != "self"])):
    """run()'s arguments as one record: run() fills it from its parameters, run_batch and run_tensors from their keywords."""

    def check(self):
        SimpleICP._check_arguments(self.distance_weights, self.rbp_observed_values, self.rbp_observation_weights)
