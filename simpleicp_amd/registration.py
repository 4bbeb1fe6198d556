"""Global registration: descriptors matched across two clouds, poses from triples of matches scored by their inliers.

Contracts (M) and (R), DESIGN.md section 18 (include/simpleicp_hip_global.h).  ``fpfh_features`` describes the clouds,
``match_features`` finds every row's nearest descriptor, ``ransac_pose`` turns triples of matches into poses and counts their
inliers -- all on the GPU, reproducible bit for bit; the random triples are drawn on the host from a seed.  ``register_global`` is
the three in a row.  What comes back is a coarse pose and its runners-up: ``run_batch`` over ``candidates`` with
``evaluate_distance=`` refines and ranks them.

Contract (L), DESIGN.md section 19 (include/simpleicp_hip_posefit.h): ``fit_pose`` is the least-squares rigid fit of matched
rows, ``refine_pose`` refits poses on their own inliers, and ``register_global(..., refine=r)`` sends its ``top`` candidates
through that refit before it ranks them.

Contract (G), DESIGN.md section 20 (include/simpleicp_hip_robust.h): ``robust_pose`` fits a pose to all matches at once under
Geman-McClure weights whose scale is tightened round by round, and ``register_global(..., method="robust")`` ends the chain with
it instead of the random triples.

Contract (C), DESIGN.md section 21 (include/simpleicp_hip_consistency.h): ``consistent_matches`` tests every pair of matches for
equal lengths in both clouds and keeps the maximal core of that graph, and ``register_global(..., prune=tolerance)`` sends the
matches through it before either estimator sees them.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

from . import _lib, backend, dist
from ._lib import _stats_dict
from .features import _int_in, fpfh_features, keypoint_arguments, keypoint_keep, orient_arguments, orient_normals
from .tensors import _is_device_tensor, _wait_for_torch


class GlobalResult:
    """What ``ransac_pose`` and ``register_global`` return.  ``H``: the best pose as a 4x4 float64 array (None: no hypothesis was
    valid); ``inliers`` and ``index``: its inlier count and the row of its triple (-1: none); ``stats``: the call's record
    (n_hypotheses, n_void, n_pruned, best, best_inliers); ``candidates``: the ``top`` best as ``(H, inliers, index)``, ordered by
    ``(-inliers, index)``; ``n_matches``: the matches the poses were drawn from (``register_global`` only); ``refined``: the
    record of the refit the candidates went through (n_poses, n_void, n_improved, best, best_inliers -- ``best`` a position among
    the unrefined candidates), None without one; ``n_consistent``: the matches the pruning left for the estimator
    (``register_global(..., prune=...)`` only, None without it; ``n_matches`` stays the count before it); ``n_keypoints``: the
    ``(fixed, movable)`` numbers of keypoints the chain ran on (``register_global(..., keypoints=...)`` only, None without it);
    ``n_components``: the ``(fixed, movable)`` numbers of components the normals were oriented in
    (``register_global(..., orient=...)`` only, None without it)."""

    def __init__(self, candidates, stats, n_matches=None, refined=None, n_consistent=None, n_keypoints=None, n_components=None):
        self.candidates = list(candidates)
        self.stats = dict(stats)
        self.n_matches = n_matches
        self.n_consistent = n_consistent
        self.n_keypoints = n_keypoints
        self.n_components = n_components
        self.refined = None if refined is None else dict(refined)
        self.H, self.inliers, self.index = self.candidates[0] if self.candidates else (None, -1, -1)

    def __repr__(self):
        return f"GlobalResult(inliers={self.inliers}, index={self.index}, n_matches={self.n_matches}, stats={self.stats})"


def _refuse_distributed(who):
    if dist.is_distributed():
        from .icp import SimpleICPException
        raise SimpleICPException(f"{who} does not run in a torch.distributed job: register the clouds with one process first")


def _context(entry, what="global registration"):
    """The library's context, detached from any job, for a call of its `entry`: what the entry is in words, for a backend without."""
    ctx = backend.get_context()
    if not hasattr(ctx, entry):
        raise _lib.BackendError(f"this backend has no {what}")
    dist.detach(ctx)
    return ctx


def _is_torch(a):
    return _is_device_tensor(a) or type(a).__module__.startswith("torch")


def _check_tensor(name, t, width):
    import torch
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a CUDA torch.Tensor like its partner, not {type(t).__name__}")
    if t.device.type != "cuda":
        raise ValueError(f"{name} is on {t.device}: tensors must be on the GPU; rows in host memory go in as numpy arrays")
    device = backend.default_device()
    if t.device.index != device:
        raise ValueError(f"{name} is on {t.device}, the library's context on cuda:{device}")
    if t.dim() != 2 or (width is not None and t.shape[1] != width):
        raise ValueError(f"{name} must have shape (n, {'dim' if width is None else width}), not {tuple(t.shape)}")


# ---- matching ----
def _match_shapes(nq, nt, wq, wt):
    if wq != wt:
        raise ValueError(f"query and target must have the same width, not {wq} and {wt}")
    if not 1 <= wq <= _lib.MATCH_MAX_DIM:
        raise ValueError(f"the descriptors' width must be >= 1 and <= {_lib.MATCH_MAX_DIM}, not {wq}")
    if nt >= 2**31:
        raise ValueError("target must have fewer than 2^31 rows")


def _match_host(ctx, q, t):
    """(idx int64, d2 float32) of one call; an empty side needs no backend: nobody is matched."""
    if q.shape[0] == 0 or t.shape[0] == 0:
        return np.full(q.shape[0], -1, np.int64), np.full(q.shape[0], np.inf, np.float32)
    idx, d2, _ = ctx().feature_match(q, t)
    return idx.astype(np.int64), d2


def _match_device(ctx, q, t):
    import torch
    nq, nt = q.shape[0], t.shape[0]
    if nq == 0 or nt == 0:
        return (torch.full((nq,), -1, dtype=torch.int64, device=q.device),
                torch.full((nq,), math.inf, dtype=torch.float32, device=q.device))
    c = ctx()
    idx = torch.empty(nq, dtype=torch.int32, device=q.device)
    d2 = torch.empty(nq, dtype=torch.float32, device=q.device)
    _wait_for_torch(c, q.device)
    c.feature_match(q.data_ptr(), t.data_ptr(), nq, nt, q.shape[1], idx_ptr=idx.data_ptr(), d2_ptr=d2.data_ptr())
    return idx.to(torch.int64), d2


def match_features(query, target, *, mutual=False, return_distance=False):
    """For every row of ``query`` the row of ``target`` with the nearest descriptor (contract (M)): float32
    squared differences summed in column order, ties to the lowest row, a row at a NaN or infinite distance never chosen.

    ``query`` (nq, dim), ``target`` (nt, dim): float32, both numpy arrays or both CUDA torch tensors (the stream rule is
    run_tensors'), dim at most 64.  Returns ``idx``: (nq,) int64 -- a tensor for tensors, an array for arrays --, -1 for a row
    without a match.  ``mutual=True``: a second call with the roles swapped, and ``idx[i] = -1`` unless ``back[idx[i]] == i``.
    ``return_distance=True``: also the (nq,) float32 squared distance to the nearest row (+inf where there is none), whatever the
    mutual test says."""
    on_device = _is_torch(query) or _is_torch(target)
    if on_device:
        import torch
        _check_tensor("query", query, None)
        _check_tensor("target", target, None)
        for name, a in (("query", query), ("target", target)):
            if a.dtype != torch.float32:
                raise TypeError(f"{name} must be float32, not {a.dtype}")
    else:
        for name, a in (("query", query), ("target", target)):
            if not isinstance(a, np.ndarray):
                raise TypeError(f"{name} must be a numpy array or a CUDA torch.Tensor, not {type(a).__name__}")
            if a.dtype != np.float32:
                raise TypeError(f"{name} must be float32, not {a.dtype}")
            if a.ndim != 2:
                raise ValueError(f"{name} must have shape (n, dim), not {a.shape}")
    _match_shapes(query.shape[0], target.shape[0], query.shape[1], target.shape[1])
    _refuse_distributed("match_features")
    held = []

    def ctx():
        if not held:
            held.append(_context("feature_match"))
        return held[0]

    if on_device:
        q, t = query.contiguous(), target.contiguous()
        one = _match_device
    else:
        q, t = np.ascontiguousarray(query), np.ascontiguousarray(target)
        one = _match_host
    idx, d2 = one(ctx, q, t)
    if mutual and q.shape[0] and t.shape[0]:                          # (an empty side matches nobody: nothing to confirm)
        back, _ = one(ctx, t, q)
        found = idx >= 0
        safe = idx.clamp(min=0) if on_device else np.maximum(idx, 0)
        agree = found & (back[safe] == (torch.arange(len(idx), device=idx.device) if on_device else np.arange(len(idx))))
        idx = torch.where(agree, idx, torch.full_like(idx, -1)) if on_device else np.where(agree, idx, -1)
    return (idx, d2) if return_distance else idx


# ---- poses ----
def _number(name, v):
    if isinstance(v, (bool, str, bytes)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise TypeError(f"{name} must be a number, not {v!r}")
    return float(v)


def _positive(name, v):
    d = _number(name, v)
    if not math.isfinite(d) or not d > 0.0:
        raise ValueError(f"{name} must be finite and > 0, not {v!r}")
    return d


def ransac_arguments(max_distance, hypotheses=4096, edge_ratio=0.9, seed=0, triples=None, top=1):
    """(max_distance, hypotheses, edge_ratio, seed, triples as (h, 3) int32 or None, top), checked: TypeError / ValueError."""
    d = _positive("max_distance", max_distance)
    h = _int_in("hypotheses", hypotheses, 1, 2**31 - 1)
    r = _number("edge_ratio", edge_ratio)
    if not 0.0 <= r <= 1.0:
        raise ValueError(f"edge_ratio must be >= 0 and <= 1, not {edge_ratio!r}")
    s = _int_in("seed", seed, 0, 2**63 - 1)
    k = _int_in("top", top, 1, 2**31 - 1)
    tri = None
    if triples is not None:
        tri = np.asarray(triples)
        if tri.dtype.kind not in "iu":
            raise TypeError(f"triples must be integers, not {tri.dtype}")
        if tri.ndim != 2 or tri.shape[1] != 3 or tri.shape[0] < 1:
            raise ValueError(f"triples must have shape (h, 3), h >= 1, not {tri.shape}")
        if tri.size and (tri.min() < -2**31 or tri.max() > 2**31 - 1):
            raise ValueError("triples must fit 32-bit integers")
        tri = np.ascontiguousarray(tri, dtype=np.int32)
    return d, h, r, s, tri, k


def _as_H(pose):
    H = np.eye(4)
    H[:3, :3] = np.asarray(pose[:9], dtype=np.float64).reshape(3, 3)
    H[:3, 3] = pose[9:12]
    return H


def _packed_poses(H):
    """H -- one 4x4 pose or a stack (b, 4, 4), an array or a tensor -- as the (b, 12) float64 rows the entry points take (R
    row-major, then t), and whether it was one pose."""
    if _is_torch(H):
        H = H.detach().cpu().numpy()
    H = np.asarray(H, dtype=np.float64)
    if H.shape[-2:] != (4, 4) or H.ndim not in (2, 3) or H.shape[0] < 1:
        raise ValueError(f"H must have shape (4, 4) or (b, 4, 4), b >= 1, not {H.shape}")
    stack = H.reshape(-1, 4, 4)
    return np.ascontiguousarray(np.concatenate([stack[:, :3, :3].reshape(-1, 9), stack[:, :3, 3]], axis=1)), H.ndim == 2


def _best(inliers, top):
    """The rows of the `top` best hypotheses, ordered by (-inliers, index); void and pruned ones never."""
    valid = np.flatnonzero(inliers >= 0)
    order = valid[np.lexsort((valid, -inliers[valid].astype(np.int64)))]
    return order[:top]


def _matched_rows(src, dst):
    """(on_device, src, dst, m) of two sets of matched rows, checked: both numpy (made float64) or both CUDA tensors."""
    on_device = _is_torch(src) or _is_torch(dst)
    if on_device:
        import torch
        _check_tensor("src", src, 3)
        _check_tensor("dst", dst, 3)
        for name, a in (("src", src), ("dst", dst)):
            if a.dtype not in (torch.float32, torch.float64):
                raise TypeError(f"{name} must be float32 or float64, not {a.dtype}")
    else:
        src, dst = np.ascontiguousarray(src, dtype=np.float64), np.ascontiguousarray(dst, dtype=np.float64)
        for name, a in (("src", src), ("dst", dst)):
            if a.ndim != 2 or a.shape[1] != 3:
                raise ValueError(f"{name} must have shape (m, 3), not {a.shape}")
    m = src.shape[0]
    if dst.shape[0] != m:
        raise ValueError(f"src and dst must have the same number of rows, not {m} and {dst.shape[0]}")
    if m < 3:
        raise ValueError(f"a pose needs at least 3 matches, not {m}")
    if m >= 2**31:
        raise ValueError("src must have fewer than 2^31 rows")
    return on_device, src, dst, m


def _on_device_f64(ctx, src, dst):
    """The tensors as the kernels read them (float32 widened exactly), the library's stream behind torch's."""
    import torch
    S, D = src.to(torch.float64).contiguous(), dst.to(torch.float64).contiguous()
    _wait_for_torch(ctx, S.device)
    return S, D


# matched rows where an operator reads them: the context, whether they are device tensors, both sets as float64, their number
_Rows = namedtuple("_Rows", "ctx on_device S D m")


def _open_rows(who, src, dst, entry, what, checked=_matched_rows):
    """The opening of an operator over matched rows: the rows checked, the job refused, the context that has `entry` (`what`: the
    entry in words), and on the tensor road the float64 tensors with the library's stream behind torch's."""
    on_device, src, dst, m = checked(src, dst)
    _refuse_distributed(who)
    ctx = _context(entry, what)
    S, D = _on_device_f64(ctx, src, dst) if on_device else (src, dst)
    return _Rows(ctx, on_device, S, D, m)


def _refit(rows, poses, max_distance, rounds):
    """sicp_pose_refit on rows that are where they are: (poses (b, 12), inliers (b,) int32, the record as a dict).  The poses
    (None: the plain fit) and the results are a few hundred bytes of host memory on either road."""
    ctx, on_device, S, D, m = rows
    if not on_device:
        out, inl, st = ctx.pose_refit(S, D, poses, max_distance, rounds)
    else:
        b = 1 if poses is None else len(poses)
        out, inl = np.empty((b, 12), np.float64), np.empty(b, np.int32)
        st = ctx.pose_refit(S.data_ptr(), D.data_ptr(), None if poses is None else poses.ctypes.data, max_distance, rounds, m=m, b=b,
                            poses_ptr=out.ctypes.data, inliers_ptr=inl.ctypes.data)
    return out, inl, _stats_dict(st)


def _ransac_pose(src, dst, max_distance, hypotheses=4096, edge_ratio=0.9, seed=0, triples=None, top=1, refine=0):
    """ransac_pose, and with refine >= 1 the refit of its candidates."""
    d, h, r, s, tri, top = ransac_arguments(max_distance, hypotheses, edge_ratio, seed, triples, top)
    refine = _int_in("refine", refine, 0, _lib.POSEFIT_MAX_ROUNDS)
    on_device, src, dst, m = _matched_rows(src, dst)
    _refuse_distributed("ransac_pose")
    if tri is None:
        tri = np.random.default_rng(s).integers(0, m, (h, 3), dtype=np.int32)
    ctx = _context("ransac_triplets")
    if refine and not hasattr(ctx, "pose_refit"):
        raise _lib.BackendError("this backend has no pose refit")
    if on_device:
        import torch
        S, D = _on_device_f64(ctx, src, dst)
        poses_d = torch.empty((len(tri), 12), dtype=torch.float64, device=S.device)
        inl_d = torch.empty(len(tri), dtype=torch.int32, device=S.device)
        st = ctx.ransac_triplets(S.data_ptr(), D.data_ptr(), tri.ctypes.data, d, r, m=m, h=len(tri), poses_ptr=poses_d.data_ptr(),
                                 inliers_ptr=inl_d.data_ptr())
        inl = inl_d.cpu().numpy()
        rows = _best(inl, top)
        poses = poses_d[torch.as_tensor(rows, device=S.device)].cpu().numpy() if len(rows) else np.empty((0, 12))
    else:
        S, D = src, dst
        allp, inl, st = ctx.ransac_triplets(src, dst, tri, d, r)
        rows = _best(inl, top)
        poses = allp[rows]
    stats = _stats_dict(st)
    counts, refined = inl[rows], None
    if refine and len(rows):
        # the `top` candidates refitted on their own inliers (contract (L)) while the rows are where they are, then ranked again
        poses, counts, refined = _refit(_Rows(ctx, on_device, S, D, m), np.ascontiguousarray(poses, dtype=np.float64), d, refine)
        again = np.lexsort((rows, -counts.astype(np.int64)))
        poses, counts, rows = poses[again], counts[again], rows[again]
    return GlobalResult([(_as_H(p), int(n), int(k)) for p, n, k in zip(poses, counts, rows)], stats, refined=refined)


def ransac_pose(src, dst, *, max_distance, hypotheses=4096, edge_ratio=0.9, seed=0, triples=None, top=1):
    """The pose R, t that brings ``src[c]`` onto ``dst[c]`` for the most rows c (contract (R)): every triple
    of matches gives one pose -- the minimal solver, exact for congruent triangles; triples whose edge lengths differ by more
    than ``edge_ratio`` are pruned first (Open3D's edge-length checker) -- and a pose's score is the number of rows within
    ``max_distance`` (strict).  A coarse pose: ``refine_pose`` refits it on its inliers, ICP refines it.

    ``src``, ``dst``: (m, 3) matched points, both numpy arrays or both CUDA torch tensors; float32 is widened exactly.
    ``triples``: (h, 3) integers; None: ``np.random.default_rng(seed).integers(0, m, (hypotheses, 3), dtype=np.int32)``, drawn on
    the host (a repeated index is simply a void hypothesis).  Returns a ``GlobalResult``; its ``candidates`` are the ``top`` best."""
    return _ransac_pose(src, dst, max_distance, hypotheses, edge_ratio, seed, triples, top)


# ---- least-squares poses (contract (L)) ----
def _refit_distance(max_distance):
    d = _number("max_distance", max_distance)
    if math.isnan(d) or not d > 0.0:
        raise ValueError(f"max_distance must be > 0 (math.inf: every row counts), not {max_distance!r}")
    return d


def fit_pose(src, dst):
    """The rigid pose that brings ``src[c]`` closest to ``dst[c]`` in the least-squares sense over all rows whose six coordinates
    are finite (Kabsch / Horn; contract (L)): centroids and centred cross sums by the fixed pair tree, the
    rotation from the top eigenvector of Horn's 4x4 matrix by a fixed number of Jacobi sweeps -- the same bits on every run.

    ``src``, ``dst``: (m, 3) matched points, m >= 3, both numpy arrays or both CUDA torch tensors; float32 is widened exactly.
    Returns the 4x4 float64 ``H``; None when fewer than three rows are finite or the fit is not."""
    poses, inl, _ = _refit(_open_rows("fit_pose", src, dst, "pose_refit", "pose refit"), None, math.inf, 1)
    return _as_H(poses[0]) if inl[0] >= 0 else None


def refine_pose(src, dst, H, *, max_distance, rounds=3):
    """Poses refitted on their own inliers (contract (L)): per round the least-squares fit (``fit_pose``'s)
    of the rows within ``max_distance`` (strict; ``math.inf``: every row at a finite distance) of their partner under the
    current pose; the next round starts from that fit.  What comes back is the pose with the most inliers among the one given
    and every round's -- the earliest on a tie, so never a pose with fewer inliers than the one that went in.

    ``src``, ``dst`` as for ``fit_pose``; ``H``: one 4x4 pose or a stack (b, 4, 4).  Returns ``(H, inliers)`` in the same shape:
    float64 poses and their inlier counts (an int, or a (b,) int64 array); a pose with a non-finite entry comes back as zeros
    with -1."""
    d = _refit_distance(max_distance)
    r = _int_in("rounds", rounds, 1, _lib.POSEFIT_MAX_ROUNDS)
    poses, single = _packed_poses(H)
    out, inl, _ = _refit(_open_rows("refine_pose", src, dst, "pose_refit", "pose refit"), poses, d, r)
    Hs = np.stack([_as_H(p) if n >= 0 else np.zeros((4, 4)) for p, n in zip(out, inl)])
    return (Hs[0], int(inl[0])) if single else (Hs, inl.astype(np.int64))


# ---- robust poses (contract (G)) ----
def robust_arguments(max_distance, rounds=64, divisor=1.4, start_scale=None):
    """(max_distance, rounds, divisor, start_scale: 0.0 for None), checked: TypeError / ValueError."""
    d = _positive("max_distance", max_distance)
    r = _int_in("rounds", rounds, 1, _lib.ROBUST_MAX_ROUNDS)
    q = _number("divisor", divisor)
    if not math.isfinite(q) or not q > 1.0:
        raise ValueError(f"divisor must be finite and > 1, not {divisor!r}")
    s = 0.0
    if start_scale is not None:
        s = _number("start_scale", start_scale)
        if not math.isfinite(s) or not s > 0.0:
            raise ValueError(f"start_scale must be finite and > 0 (None: chosen from the residuals), not {start_scale!r}")
    return d, r, q, s


def _robust(rows, poses, d, r, q, s):
    """sicp_pose_robust on rows that are where they are: (poses (b, 12), inliers (b,) int32, scales (b,), the record as a dict)."""
    ctx, on_device, S, D, m = rows
    if not on_device:
        out, inl, scales, st = ctx.pose_robust(S, D, poses, d, r, q, s)
    else:
        b = 1 if poses is None else len(poses)
        out, inl, scales = np.empty((b, 12), np.float64), np.empty(b, np.int32), np.empty(b, np.float64)
        st = ctx.pose_robust(S.data_ptr(), D.data_ptr(), None if poses is None else poses.ctypes.data, d, r, q, s, m=m, b=b,
                             poses_ptr=out.ctypes.data, inliers_ptr=inl.ctypes.data, scales_ptr=scales.ctypes.data)
    return out, inl, scales, _stats_dict(st)


def robust_pose(src, dst, *, max_distance, H=None, rounds=64, divisor=1.4, start_scale=None):
    """The rigid pose that brings ``src[c]`` onto ``dst[c]`` for the matches that agree with each other, wrong matches among them
    (contract (G)): every round weights every row by the Geman-McClure weight ``(s / (s + d2))**2`` of its
    squared residual under the current pose and refits the weighted least-squares pose (Horn, ``fit_pose``'s arithmetic); ``s``
    starts at ``start_scale`` (None: twice the largest squared residual under the start) and is divided by ``divisor`` after
    every round, never below ``max_distance**2`` -- graduated non-convexity, as Fast Global Registration runs it.  No seed, no
    hypotheses: the same bits on every run.  The answer is the pose of the last round.

    ``src``, ``dst`` as for ``fit_pose``; ``H``: the start -- None (the identity), one 4x4 pose or a stack (b, 4, 4).  Returns
    ``(H, inliers)``: float64 poses in H's shape ((4, 4) for None) and the rows within ``max_distance`` (strict) of their partner
    under them (an int, or a (b,) int64 array); a start with a non-finite entry, or without a single row at a finite distance,
    comes back as zeros with -1."""
    d, r, q, s = robust_arguments(max_distance, rounds, divisor, start_scale)
    poses, single = None, True
    if H is not None:
        poses, single = _packed_poses(H)
    out, inl, _, _ = _robust(_open_rows("robust_pose", src, dst, "pose_robust", "robust pose fit"), poses, d, r, q, s)
    Hs = np.stack([_as_H(p) if n >= 0 else np.zeros((4, 4)) for p, n in zip(out, inl)])
    return (Hs[0], int(inl[0])) if single else (Hs, inl.astype(np.int64))


# ---- matches pruned by pairwise length consistency (contract (C)) ----
class ConsistencyResult:
    """What ``consistent_matches`` returns.  ``keep``: (m,) bool, the rows of the maximal core -- ``core == max_core`` where
    ``max_core >= 1``, else all False; ``core``, ``degree``: (m,) int32, every row's core number and its number of compatible
    rows; ``stats``: the call's record (n_rows, n_valid, n_edges, max_degree, max_core, n_max_core, n_subrounds).  Tensors for
    tensors, arrays for arrays."""

    def __init__(self, keep, core, degree, stats):
        self.keep, self.core, self.degree, self.stats = keep, core, degree, dict(stats)

    def __repr__(self):
        return f"ConsistencyResult(kept={int(self.keep.sum())}, stats={self.stats})"


def consistency_arguments(tolerance, min_length=0.0):
    """(tolerance, min_length), checked: TypeError / ValueError."""
    t = _positive("tolerance", tolerance)
    l = _number("min_length", min_length)
    if not math.isfinite(l) or l < 0.0:
        raise ValueError(f"min_length must be finite and >= 0, not {min_length!r}")
    return t, l


def _consistency_rows(src, dst):
    """_matched_rows, and the operator's cap."""
    on_device, src, dst, m = _matched_rows(src, dst)
    if m > _lib.CONSISTENCY_MAX_ROWS:
        raise ValueError(f"consistent_matches takes at most {_lib.CONSISTENCY_MAX_ROWS} matches, not {m}: thin the matches first "
                         "(nothing is subsampled silently)")
    return on_device, src, dst, m


def _consistency(rows, t, l):
    """sicp_match_consistency on rows that are where they are: the ConsistencyResult (tensors on the tensor road)."""
    ctx, on_device, S, D, m = rows
    if not on_device:
        degree, core, st = ctx.match_consistency(S, D, t, l)
    else:
        import torch
        degree = torch.empty(m, dtype=torch.int32, device=S.device)
        core = torch.empty(m, dtype=torch.int32, device=S.device)
        st = ctx.match_consistency(S.data_ptr(), D.data_ptr(), t, l, m=m, degree_ptr=degree.data_ptr(), core_ptr=core.data_ptr())
    stats = _stats_dict(st)
    keep = core == stats["max_core"] if stats["max_core"] >= 1 else core < 0       # (no core number is negative: all False)
    return ConsistencyResult(keep, core, degree, stats)


def consistent_matches(src, dst, *, tolerance, min_length=0.0):
    """The matches that agree with each other in length (contract (C)): a rigid motion keeps lengths, so rows
    i and j can both be right only if ``|src[i] - src[j]|`` and ``|dst[i] - dst[j]|`` differ by at most ``tolerance``; pairs closer
    than ``min_length`` in either cloud say little and are not compatible.  These tests form a graph on the matches -- the right
    ones a clique in it --, and what is kept is its maximal core: the rows of the largest core number (TEASER++'s k-core
    heuristic).  All integers, no seed: the same result on every run.

    ``src``, ``dst``: (m, 3) matched points, 3 <= m <= 32 768 (thin the matches first if there are more), both numpy arrays or both
    CUDA torch tensors; float32 is widened exactly.  Returns a ``ConsistencyResult``; a pose estimator then takes
    ``src[res.keep]``, ``dst[res.keep]``."""
    t, l = consistency_arguments(tolerance, min_length)
    return _consistency(_open_rows("consistent_matches", src, dst, "match_consistency", "match consistency", _consistency_rows), t, l)


def _oriented_fpfh(X, neighbors, normal_neighbors, viewpoint, orient):
    """(the descriptors of X over its estimated normals sent through orient_normals, the number of components): the vote goes
    towards the viewpoint, or away from the centre of the bounding box."""
    if viewpoint is not None:
        vote = dict(viewpoint=viewpoint)
    elif _is_torch(X):
        vote = dict(away_from=((X.min(dim=0).values.double() + X.max(dim=0).values.double()) * 0.5).cpu().numpy())
    else:
        P = np.asarray(X, dtype=np.float64)
        vote = dict(away_from=(P.min(axis=0) + P.max(axis=0)) * 0.5)
    normals, info = orient_normals(X, normal_neighbors=normal_neighbors, return_info=True, **orient, **vote)
    return fpfh_features(X, normals, neighbors=neighbors), info["n_components"]


def register_global(fixed, movable, *, max_distance, neighbors=32, normal_neighbors=10, viewpoint_fixed=None, viewpoint_movable=None,
                    mutual=True, **ransac_kwargs):
    """A coarse pose of ``movable`` onto ``fixed`` without an initial guess -- in the direction of ``run()``'s H --: the FPFH
    descriptors of both clouds (``fpfh_features``: ``neighbors``, ``normal_neighbors``, a viewpoint per cloud), every movable
    point's nearest fixed descriptor (``match_features``, ``mutual``), poses from triples of those matches (``ransac_pose``:
    ``max_distance`` and its other keywords).  Both clouds (n, 3) numpy arrays or both CUDA torch tensors.

    ``refine=r`` (0 .. 64, default 0: nothing) refits the ``top`` candidates on their own inliers in r rounds (``refine_pose``
    with the same ``max_distance``) and ranks them again by ``(-inliers, index)``; ``index`` stays the row of the triple, ``stats``
    the record of the hypotheses, ``refined`` the refit's.

    ``method="robust"`` (default ``"ransac"``) ends the chain with ``robust_pose`` from the identity over all matches instead of
    the triples; its keywords are then ``rounds``, ``divisor`` and ``start_scale``, and ``ransac_pose``'s are refused.  The
    result has one candidate ``(H, inliers, -1)`` -- none when the fit is void -- and the robust fit's record (n_poses, n_void,
    best, best_inliers) as ``stats``.

    ``prune=tolerance`` (default None: nothing), under either method, sends the matched rows through ``consistent_matches``
    (``min_length=prune_min_length``, default 0.0) before the estimator, which then sees only the rows of the maximal core:
    ``n_consistent`` is their number, ``n_matches`` stays the count before the pruning, fewer than three rows left give the result
    without a pose, and ``index`` (and ``triples``) are rows of the pruned set.  More than 32 768 matches raise ``ValueError``.

    ``keypoints=`` (default None: nothing changes, bit for bit), under either method: True, or a dict of ``keypoint_keep``'s
    keywords.  Both clouds are described over all their points as before; then descriptors and coordinates are gathered at each
    cloud's ISS keypoints and the rest of the chain -- matching, pruning, the estimator -- runs on those rows alone.
    ``n_keypoints = (fixed, movable)`` is their number, fewer than three on a side give the result without a pose, and ``index``
    (and ``triples``) are rows of the keypoint sets (of their matched, of their pruned rows), not of the clouds.

    ``orient=`` (default None: nothing changes, bit for bit), under either method: an int k, or a dict of ``orient_normals``'
    keywords (``neighbors``).  Each cloud's estimated normals go through ``orient_normals`` before the descriptors.  With
    ``viewpoint_fixed`` / ``viewpoint_movable`` the viewpoint becomes the VOTE's reference -- every component is turned towards it
    as a whole -- and ``fpfh_features`` gets no viewpoint; without one the vote is away from the centre of the cloud's bounding
    box, ``(min + max) * 0.5``: exact and independent of the order of the points, so the chain stays reproducible bit for bit.
    That centre is a convention, not physics: it is right for a closed surface seen from outside and only consistent elsewhere.
    ``n_components = (fixed, movable)`` reports the components; more than one means signs that no neighbourhood relates.

    Returns ``ransac_pose``'s GlobalResult with ``n_matches`` set; fewer than three matches give a result without a pose.
    ICP stays the caller's: ``run_batch`` over ``candidates`` with ``evaluate_distance=``."""
    orient = ransac_kwargs.pop("orient", None)
    if orient is not None:
        if isinstance(orient, dict):
            if set(orient) - {"neighbors"}:
                raise TypeError(f"orient= takes orient_normals' keyword neighbors, not {sorted(set(orient) - {'neighbors'})[0]!r}")
        elif isinstance(orient, (bool, float, str, bytes)) or not isinstance(orient, (int, np.integer)):
            raise TypeError(f"orient must be None, an int or a dict of orient_normals' keywords, not {orient!r}")
        else:
            orient = dict(neighbors=int(orient))
        orient_arguments(normal_neighbors=normal_neighbors, **orient)
    keypoints = ransac_kwargs.pop("keypoints", None)
    if keypoints is not None:
        if keypoints is True:
            keypoints = {}
        elif not isinstance(keypoints, dict):
            raise TypeError(f"keypoints must be None, True or a dict of keypoint_keep's keywords, not {keypoints!r}")
        if "return_saliency" in keypoints:
            raise TypeError("keypoints= takes keypoint_keep's keywords without return_saliency")
        keypoint_arguments(**keypoints)
    prune = ransac_kwargs.pop("prune", None)
    if prune is None:
        if "prune_min_length" in ransac_kwargs:
            raise TypeError("register_global() got prune_min_length without prune")
    else:
        prune = consistency_arguments(prune, ransac_kwargs.pop("prune_min_length", 0.0))
    method = ransac_kwargs.pop("method", "ransac")
    if not isinstance(method, str):
        raise TypeError(f"method must be 'ransac' or 'robust', not {method!r}")
    if method not in ("ransac", "robust"):
        raise ValueError(f"method must be 'ransac' or 'robust', not {method!r}")
    robust = method == "robust"
    unknown = set(ransac_kwargs) - ({"rounds", "divisor", "start_scale"} if robust else
                                    {"hypotheses", "edge_ratio", "seed", "triples", "top", "refine"})
    if unknown:
        raise TypeError(f"register_global() got an unexpected keyword argument {sorted(unknown)[0]!r}" +
                        (" (method='robust')" if robust else ""))
    if robust:
        fit = robust_arguments(max_distance, **ransac_kwargs)
    else:
        refine = _int_in("refine", ransac_kwargs.pop("refine", 0), 0, _lib.POSEFIT_MAX_ROUNDS)
        ransac_arguments(max_distance, **ransac_kwargs)
    if not isinstance(mutual, (bool, np.bool_)):
        raise TypeError(f"mutual must be True or False, not {mutual!r}")
    if _is_torch(fixed) != _is_torch(movable):
        raise TypeError("fixed and movable must both be numpy arrays or both be CUDA torch tensors")
    _refuse_distributed("register_global")
    n_components = None
    if orient is None:
        f_fix = fpfh_features(fixed, neighbors=neighbors, normal_neighbors=normal_neighbors, viewpoint=viewpoint_fixed)
        f_mov = fpfh_features(movable, neighbors=neighbors, normal_neighbors=normal_neighbors, viewpoint=viewpoint_movable)
    else:
        f_fix, c_fix = _oriented_fpfh(fixed, neighbors, normal_neighbors, viewpoint_fixed, orient)
        f_mov, c_mov = _oriented_fpfh(movable, neighbors, normal_neighbors, viewpoint_movable, orient)
        n_components = (c_fix, c_mov)
    none = dict(n_poses=0, n_void=0, best=-1, best_inliers=-1) if robust else \
        dict(n_hypotheses=0, n_void=0, n_pruned=0, best=-1, best_inliers=-1)
    n_keypoints = None
    if keypoints is not None:
        # descriptors and coordinates gathered at each cloud's keypoints, where they are: the chain goes on with those rows
        if not _is_torch(movable):
            fixed, movable = np.asarray(fixed, dtype=np.float64), np.asarray(movable, dtype=np.float64)
        k_fix, k_mov = keypoint_keep(fixed, **keypoints), keypoint_keep(movable, **keypoints)
        n_keypoints = (int(k_fix.sum()), int(k_mov.sum()))
        if min(n_keypoints) < 3:
            return GlobalResult([], none, 0, n_keypoints=n_keypoints, n_components=n_components)
        fixed, movable, f_fix, f_mov = fixed[k_fix], movable[k_mov], f_fix[k_fix], f_mov[k_mov]
    idx = match_features(f_mov, f_fix, mutual=bool(mutual))
    keep = idx >= 0
    n_matches = int(keep.sum())
    if n_matches < 3:
        return GlobalResult([], none, n_matches, n_keypoints=n_keypoints, n_components=n_components)
    if not _is_torch(movable):
        fixed, movable = np.asarray(fixed, dtype=np.float64), np.asarray(movable, dtype=np.float64)
    src, dst, n_consistent = movable[keep], fixed[idx[keep]], None
    if prune is not None:
        # the matched rows through sicp_match_consistency while they are where they are: the estimator sees the maximal core
        rows = _open_rows("register_global", src, dst, "match_consistency", "match consistency", _consistency_rows)
        kept = _consistency(rows, *prune).keep
        src, dst, n_consistent = rows.S[kept], rows.D[kept], int(kept.sum())
        if n_consistent < 3:
            return GlobalResult([], none, n_matches, n_consistent=n_consistent, n_keypoints=n_keypoints, n_components=n_components)
    if robust:
        # the matched rows through sicp_pose_robust from the identity while they are where they are
        rows = _open_rows("register_global", src, dst, "pose_robust", "robust pose fit")
        poses, inl, _, stats = _robust(rows, None, *fit)
        return GlobalResult([(_as_H(poses[0]), int(inl[0]), -1)] if inl[0] >= 0 else [], stats, n_matches, n_consistent=n_consistent,
                            n_keypoints=n_keypoints, n_components=n_components)
    res = _ransac_pose(src, dst, max_distance, refine=refine, **ransac_kwargs)
    res.n_matches, res.n_consistent, res.n_keypoints, res.n_components = n_matches, n_consistent, n_keypoints, n_components
    return res
