"""How good a registration is: fitness, inlier RMSE and the information matrix of one cloud against the other under H.

Contract (E), DESIGN.md section 14 (include/simpleicp_hip_eval.h): an exact radius-bounded 1-NN of every query point among the
searched cloud under H, and the reduction of its results, on the GPU; 96 bytes come back.  ``evaluate_registration`` is the
stand-alone call; ``SimpleICP.evaluate_distance`` and the ``evaluate_distance=`` keyword of ``run_tensors`` / ``run_batch`` score
a run under its final H while both clouds are still resident.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Tuple

import numpy as np

from . import _lib, backend, dist


@dataclass(frozen=True)
class Evaluation:
    """The record of one evaluation.  ``sum_d2`` is the sum of the inliers' squared distances to their nearest neighbour,
    ``sum_p`` of their coordinates (x, y, z) and ``sum_pp`` of their products (xx, yy, zz, xy, xz, yz): the tree sums of contract
    (E), in the query cloud's own frame.  Everything else is formed from them on the host."""
    n_queries: int
    n_inliers: int
    sum_d2: float
    sum_p: Tuple[float, float, float]
    sum_pp: Tuple[float, float, float, float, float, float]

    @classmethod
    def from_record(cls, rec) -> "Evaluation":
        return cls(int(rec.n_queries), int(rec.n_inliers), float(rec.sum_d2), tuple(float(v) for v in rec.sum_p),
                   tuple(float(v) for v in rec.sum_pp))

    @property
    def fitness(self) -> float:
        """Share of the queries that have a neighbour within the distance."""
        return self.n_inliers / self.n_queries

    @property
    def inlier_rmse(self) -> float:
        """Root mean square of the inliers' distances; 0.0 when there is no inlier (as Open3D reports it)."""
        return math.sqrt(self.sum_d2 / self.n_inliers) if self.n_inliers else 0.0

    @property
    def centroid(self) -> np.ndarray:
        """Mean of the inliers (NaN when there is none)."""
        return np.array(self.sum_p) / self.n_inliers if self.n_inliers else np.full(3, np.nan)

    @property
    def information(self) -> np.ndarray:
        """The 6 x 6 information matrix sum(G^T G), G = [ -[p]x | I ], over the inliers p, in the parameter order of ``rbp``
        (three rotations, then the translation): the pose-graph edge weight of Open3D's convention
        (get_information_matrix_from_point_clouds), in the query cloud's frame.  It is NOT a covariance of ``rbp`` -- the
        estimated uncertainties of a run remain that."""
        sx, sy, sz = self.sum_p
        xx, yy, zz, xy, xz, yz = self.sum_pp
        L = np.zeros((6, 6))
        L[0, 0], L[1, 1], L[2, 2] = yy + zz, xx + zz, xx + yy
        L[0, 1] = L[1, 0] = -xy
        L[0, 2] = L[2, 0] = -xz
        L[1, 2] = L[2, 1] = -yz
        B = np.array([[0.0, -sz, sy], [sz, 0.0, -sx], [-sy, sx, 0.0]])
        L[0:3, 3:6] = B
        L[3:6, 0:3] = B.T
        L[3:6, 3:6] = float(self.n_inliers) * np.eye(3)
        return L


def _distance_of(max_distance, exc=ValueError, name="max_distance"):
    """The search bound as a float: >= 0, +inf allowed, NaN refused."""
    try:
        d = float(max_distance)
    except (TypeError, ValueError):
        raise exc(f"{name} must be a number >= 0, not {max_distance!r}") from None
    if math.isnan(d) or d < 0:
        raise exc(f"{name} must be >= 0, not {max_distance!r}")
    return d


def need_backend(ctx):
    if not hasattr(ctx, "evaluate"):
        raise _lib.BackendError("this backend has no evaluation")


def rigid_inverse(H) -> np.ndarray:
    """[[R^T, -R^T t], [0, 1]] of a 4 x 4 rigid H, in float64 numpy."""
    H = np.asarray(H, dtype=np.float64).reshape(4, 4)
    Hi = np.eye(4)
    Hi[:3, :3] = H[:3, :3].T
    Hi[:3, 3] = -(H[:3, :3].T @ H[:3, 3])
    return Hi


def evaluate_registration(fix, mov, H, max_distance, of="fixed") -> Evaluation:
    """Scores the transform H (4 x 4, movable -> fixed) of the pair: both clouds are (n, 3) arrays, PointClouds (all their points,
    whatever is selected), or CUDA torch tensors -- tensors take run_tensors' device road: nothing coordinate-sized crosses the host
    link.  ``of="fixed"``: every fixed point searches its nearest neighbour among H * movable, strictly within ``max_distance``;
    ``of="movable"``: every movable point searches among the fixed cloud under the rigid inverse of H (Open3D's
    evaluate_registration(source=movable, target=fixed): fitness relative to the source, sums in the movable cloud's frame).
    The inputs are not modified."""
    from .pointcloud import PointCloud
    from .tensors import _check_cloud, _is_device_tensor, _upload
    if of not in ("fixed", "movable"):
        raise ValueError(f'of must be "fixed" or "movable", not {of!r}')
    d = _distance_of(max_distance)
    H = np.asarray(H, dtype=np.float64)
    if H.shape != (4, 4) or not np.isfinite(H).all():
        raise ValueError("H must be a finite 4 x 4 matrix")
    on_device = (_is_device_tensor(fix), _is_device_tensor(mov))
    if on_device[0] != on_device[1]:
        raise ValueError("one cloud is a CUDA tensor and the other is not: both go on the GPU or both on the host")
    if dist.is_distributed():
        raise RuntimeError("evaluate_registration does not run in a torch.distributed job")
    if on_device[0]:
        import torch
        device = backend.default_device()
        _check_cloud("fix", fix, device)
        _check_cloud("mov", mov, device)
    else:
        host = []
        for c in (fix, mov):
            if not isinstance(c, PointCloud):
                c = np.ascontiguousarray(c, dtype=np.float64)
                if c.ndim != 2 or c.shape[1] != 3:
                    raise ValueError("a cloud must be a PointCloud, an (n, 3) array or a CUDA tensor")
            host.append(c)
    ctx = backend.get_context()
    need_backend(ctx)
    ctx._corr_owner = None            # (an operator-level CorrPts object loses the device state to this call)
    dist.detach(ctx)
    if on_device[0]:
        # run_tensors' stream rule: the library's stream waits for torch's current stream before it reads the inputs
        torch.cuda.ExternalStream(ctx.stream_ptr(), device=fix.device).wait_stream(torch.cuda.current_stream(fix.device))
        _upload(ctx, _lib.FIX, fix)
        _upload(ctx, _lib.MOV, mov)
    else:
        for slot, c in zip((_lib.FIX, _lib.MOV), host):
            if isinstance(c, PointCloud):
                c._upload(ctx, slot)
            else:
                ctx.upload(slot, c)
    if of == "fixed":
        rec = ctx.evaluate(_lib.FIX, _lib.MOV, H, d)
    else:
        rec = ctx.evaluate(_lib.MOV, _lib.FIX, rigid_inverse(H), d)
    return Evaluation.from_record(rec)


def after_run(ctx, H, distance, info=None) -> Evaluation:
    """What a run does when evaluate_distance is set, after its last iteration and before its movable slot is touched again: every
    point of the resident fixed cloud against the resident movable cloud under the final H."""
    ev = Evaluation.from_record(ctx.evaluate(_lib.FIX, _lib.MOV, H, distance))
    if info is not None:
        info(f"Evaluation within {distance:g}: fitness {ev.fitness:.6f} ({ev.n_inliers} of {ev.n_queries} fixed points), "
             f"inlier RMSE {ev.inlier_rmse:.6f}")
    return ev
