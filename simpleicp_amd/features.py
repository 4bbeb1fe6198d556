"""FPFH descriptors: 33 floats per point, the local shape descriptor a global registration matches clouds by -- and ISS keypoints,
the points worth describing (``keypoint_keep``; contract (I), DESIGN.md section 22, include/simpleicp_hip_keypoints.h) -- and DBSCAN
labels, the points that belong together (``cluster_labels``; contract (U), DESIGN.md section 23, include/simpleicp_hip_cluster.h)
-- and the dominant plane, what goes before the clusters on a scene with a ground (``segment_plane``, ``segment_planes``; contracts
(P) and (Q), DESIGN.md section 24, include/simpleicp_hip_plane.h) -- and farthest point sampling, exactly k points evenly spread
in space (``farthest_points``; contract (S), DESIGN.md section 25, include/simpleicp_hip_farthest.h) -- and normals oriented
consistently, what the descriptor's signs stand on (``orient_normals``; contract (H), DESIGN.md section 26,
include/simpleicp_hip_orient.h) -- and the smooth regions, every patch whose neighbouring normals agree (``smooth_regions``;
contract (J), DESIGN.md section 27, include/simpleicp_hip_regions.h) -- and moving-least-squares smoothing, the coordinates
themselves improved before any of these reads them (``denoise_points``; contract (W), DESIGN.md section 28,
include/simpleicp_hip_denoise.h).

Contract (F), DESIGN.md section 17 (include/simpleicp_hip_fpfh.h): every point's k nearest points from the library's own search,
a normal per point, two passes over those lists -- all on the GPU, reproducible bit for bit.  What follows the descriptor is
``simpleicp_amd/registration.py``: ``match_features`` for the matches, ``ransac_pose`` for poses from triples of them,
``run_batch`` over the poses with ``evaluate_distance=`` to rank them.
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib, backend, dist


def _int_in(name, v, lo, hi):
    if isinstance(v, (bool, float, str, bytes)) or not isinstance(v, (int, np.integer)):
        raise TypeError(f"{name} must be an integer, not {v!r}")
    if not lo <= int(v) <= hi:
        raise ValueError(f"{name} must be >= {lo} and <= {hi}, not {v!r}")
    return int(v)


def fpfh_arguments(neighbors, radius, normal_neighbors, viewpoint):
    """(k, radius as a float -- inf: none --, normal_neighbors, viewpoint as three floats or None), checked: TypeError / ValueError."""
    k = _int_in("neighbors", neighbors, 2, _lib.FPFH_MAX_K)
    kn = _int_in("normal_neighbors", normal_neighbors, 2, 2**31 - 1)
    r = _radius_of("radius", radius)
    vp = None
    if viewpoint is not None:
        try:
            vp = np.asarray(viewpoint, dtype=np.float64)
        except (TypeError, ValueError):
            raise TypeError(f"viewpoint must be three numbers, not {viewpoint!r}") from None
        if vp.shape != (3,) or not np.isfinite(vp).all():
            raise ValueError(f"viewpoint must be three finite numbers, not {viewpoint!r}")
    return k, r, kn, vp


def _check_counts(n, k, kn, estimating):
    if k > n:
        raise ValueError(f"neighbors ({k}) exceeds the number of points ({n})")
    if estimating and kn > n:
        raise ValueError(f"normal_neighbors ({kn}) exceeds the number of points ({n})")


def _host_points(X):
    """X of a host call as it is uploaded -- a PointCloud as it is, anything else as an (n, 3) float64 array -- and its number of
    points."""
    from .pointcloud import PointCloud
    if isinstance(X, PointCloud):
        return X, len(X)
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[1] != 3:
        raise ValueError("X must be a PointCloud, an (n, 3) array or a CUDA tensor")
    return X, X.shape[0]


def _host_opening(who, instead, X, needs):
    """The common opening of fpfh_features and keypoint_keep on the host road, after their own checks (the tensor road's is
    tensors._keep_opening): the context, with X in the library's fixed slot.  needs: (entry point, what it is in words) the context
    must have."""
    if dist.is_distributed():
        from .icp import SimpleICPException
        raise SimpleICPException(f"{who} does not run in a torch.distributed job: {instead} with one process first")
    ctx = backend.get_context()
    if not hasattr(ctx, needs[0]):
        raise _lib.BackendError(f"this backend has no {needs[1]}")
    ctx._corr_owner = None            # (an operator-level CorrPts object loses the device state to this call)
    dist.detach(ctx)
    if isinstance(X, np.ndarray):
        ctx.upload(_lib.FIX, X)
    else:
        X._upload(ctx, _lib.FIX)
    return ctx


def fpfh_features(X, normals=None, *, neighbors=32, radius=None, normal_neighbors=10, viewpoint=None, return_counts=False):
    """The FPFH descriptors of X as an (n, 33) float32 array: bins 0..10 the angle of the Darboux frame's third feature, 11..21
    and 22..32 the two cosines, each group summing to 200 (contract (F)).

    X: an (n, 3) array, a PointCloud (all its points, whatever is selected) or a CUDA torch tensor (float32 / float64, any
    strides; ingest and stream rule are run_tensors').  A tensor gives a torch tensor on its device, anything else numpy.
    ``neighbors``: k of the k-NN list of every point, the point itself included (2 .. 128); ``radius``: only neighbours strictly
    closer count (None: all k - 1) -- Open3D's hybrid search (radius, max_nn).
    ``normals``: (n, 3), one per point; None: a PointCloud's own nx / ny / nz columns if it has them, else the library's normals
    from ``normal_neighbors`` points.  ``viewpoint``: three numbers; every normal is turned towards it first -- the library's own
    normals carry no physical orientation, and the descriptor depends on the signs.
    ``return_counts``: also the (n, 34) SPFH counts of pass 1 (33 bins and the number of pairs; uint16 in numpy, int16 in torch).
    The library's fixed slot holds X afterwards."""
    from .pointcloud import PointCloud
    from .tensors import _is_device_tensor
    k, r, kn, vp = fpfh_arguments(neighbors, radius, normal_neighbors, viewpoint)
    if _is_device_tensor(X) or type(X).__module__.startswith("torch"):
        return _on_device(X, normals, k, r, kn, vp, bool(return_counts))
    X, n = _host_points(X)
    own = None
    if isinstance(X, PointCloud) and normals is None and all(c in X for c in ("nx", "ny", "nz")):
        own = np.stack([np.asarray(X[c].to_numpy(), dtype=np.float32) for c in ("nx", "ny", "nz")], axis=1)
    if normals is not None:
        own = np.ascontiguousarray(normals, dtype=np.float32)
        if own.shape != (n, 3):
            raise ValueError(f"normals must have shape ({n}, 3), not {own.shape}")
    if n == 0:
        out = np.empty((0, _lib.FPFH_BINS), np.float32)
        return (out, np.empty((0, _lib.FPFH_BINS + 1), np.uint16)) if return_counts else out
    _check_counts(n, k, kn, own is None)
    ctx = _host_opening("fpfh_features", "describe the clouds", X, ("fpfh", "FPFH descriptors"))
    if own is None:                   # (host callers hold no device allocator: the normals make the round trip, 12 bytes per point)
        own = ctx.estimate_normals(_lib.FIX, np.arange(n, dtype=np.int64), kn)[0]
    out, cnt, _ = ctx.fpfh(_lib.FIX, own, k, r, vp, want_counts=bool(return_counts))
    return (out, cnt) if return_counts else out


def _on_device(X, normals, k, r, kn, vp, return_counts):
    import torch
    from .tensors import _keep_opening, _wait_for_torch
    if normals is not None and not isinstance(normals, (torch.Tensor, np.ndarray)):
        raise TypeError("normals must be a torch.Tensor or a numpy array of shape (n, 3)")
    if isinstance(X, torch.Tensor) and X.dim() == 2:
        if normals is not None and tuple(normals.shape) != (X.shape[0], 3):
            raise ValueError(f"normals must have shape ({X.shape[0]}, 3), not {tuple(normals.shape)}")
        if X.shape[0] > 0:
            _check_counts(X.shape[0], k, kn, normals is None)
    ctx, n, _, _ = _keep_opening("fpfh_features", X, None, needs=("fpfh", "FPFH descriptors"))
    dev = X.device
    out = torch.empty((n, _lib.FPFH_BINS), dtype=torch.float32, device=dev)
    cnt = torch.empty((n, _lib.FPFH_BINS + 1), dtype=torch.int16, device=dev) if return_counts else None
    if ctx is None:
        return (out, cnt) if return_counts else out
    if normals is None:               # the library's normals of all points, left in device memory
        sel = torch.arange(n, dtype=torch.int64, device=dev)
        nv = torch.empty((n, 3), dtype=torch.float32, device=dev)
        pl = torch.empty(n, dtype=torch.float32, device=dev)
    elif isinstance(normals, torch.Tensor):
        if normals.device != dev:
            raise ValueError(f"normals is on {normals.device}, X on {dev}")
        nv = normals.to(torch.float32).contiguous()
    else:
        nv = torch.from_numpy(np.ascontiguousarray(normals, dtype=np.float32)).to(dev)
    # what torch queued for this call on its current stream (the index vector, the normals' copy) comes before the library reads it
    _wait_for_torch(ctx, dev)
    if normals is None:
        ctx.estimate_normals_into(_lib.FIX, sel.data_ptr(), n, kn, nv.data_ptr(), pl.data_ptr())
    ctx.fpfh(_lib.FIX, nv, k, r, vp, fpfh_ptr=out.data_ptr(), counts_ptr=None if cnt is None else cnt.data_ptr())
    return (out, cnt) if return_counts else out


# ---- ISS keypoints (contract (I)) ----


def _radius_of(name, radius):
    if radius is None:
        return math.inf
    if isinstance(radius, (bool, str, bytes)) or not isinstance(radius, (int, float, np.integer, np.floating)):
        raise TypeError(f"{name} must be a number > 0 or None, not {radius!r}")
    r = float(radius)
    if math.isnan(r) or not r > 0.0:
        raise ValueError(f"{name} must be > 0 (None: no radius), not {radius!r}")
    return r


def _gamma_of(name, gamma):
    if isinstance(gamma, (bool, str, bytes)) or not isinstance(gamma, (int, float, np.integer, np.floating)):
        raise TypeError(f"{name} must be a number > 0, not {gamma!r}")
    g = float(gamma)
    if not math.isfinite(g) or not g > 0.0:
        raise ValueError(f"{name} must be finite and > 0, not {gamma!r}")
    return g


def keypoint_arguments(neighbors=32, salient_radius=None, nms_neighbors=None, nms_radius=None, gamma21=0.975, gamma32=0.975,
                       min_neighbors=5):
    """(k_s, salient radius -- inf: none --, k_n, nms radius, gamma21, gamma32, min_neighbors), checked: TypeError / ValueError."""
    k_s = _int_in("neighbors", neighbors, 2, _lib.KEYPOINTS_MAX_K)
    k_n = k_s if nms_neighbors is None else _int_in("nms_neighbors", nms_neighbors, 2, _lib.KEYPOINTS_MAX_K)
    return (k_s, _radius_of("salient_radius", salient_radius), k_n, _radius_of("nms_radius", nms_radius), _gamma_of("gamma21", gamma21),
            _gamma_of("gamma32", gamma32), _int_in("min_neighbors", min_neighbors, 1, 2**62))


def _check_keypoint_counts(n, a):
    if a[0] > n:
        raise ValueError(f"neighbors ({a[0]}) exceeds the number of points ({n})")
    if a[2] > n:
        raise ValueError(f"nms_neighbors ({a[2]}) exceeds the number of points ({n})")


_NO_KEYPOINTS = dict(n_points=0, n_salient=0, n_keypoints=0, n_small=0, n_clipped_salient=0, n_clipped_nms=0)


def keypoint_keep(X, *, neighbors=32, salient_radius=None, nms_neighbors=None, nms_radius=None, gamma21=0.975, gamma32=0.975,
                  min_neighbors=5, return_saliency=False):
    """The ISS keypoints of X (Intrinsic Shape Signatures; contract (I)) as a bool mask (n,): True where
    the point's neighbourhood is not flat, not a line and not a ball, and where it is the most salient point around.
    ``X[keypoint_keep(X)]`` are the keypoints, as ``X[voxel_keep(X, c)]`` is the thinned cloud.

    X: an (n, 3) array, a PointCloud (all its points, whatever is selected) or a CUDA torch tensor (float32 / float64, any
    strides; ingest and stream rule are run_tensors').  A tensor gives a torch.bool tensor on its device, anything else numpy.
    ``neighbors``: k of the support, the point itself included (2 .. 128); ``salient_radius``: only neighbours strictly closer
    count (None: all k).  The eigenvalues e1 >= e2 >= e3 of the support's covariance make the point salient iff
    e2 < ``gamma21`` * e1, e3 < ``gamma32`` * e2 and e3 > 0, with at least ``min_neighbors`` points counted; its saliency is e3.
    ``nms_neighbors`` (None: ``neighbors``) and ``nms_radius`` (None: none): a salient point is a keypoint iff none of these
    neighbours has a larger saliency -- of equals the lowest index stays -- and at least ``min_neighbors`` of them are counted.
    ``return_saliency``: also the (n,) float64 saliency (0 where not salient), the (n, 3) float64 eigenvalues and the call's
    record as a dict (n_points, n_salient, n_keypoints, n_small, n_clipped_salient, n_clipped_nms -- the clipped counts say how
    many balls held more points than k).  The library's fixed slot holds X afterwards."""
    from .tensors import _is_device_tensor
    a = keypoint_arguments(neighbors, salient_radius, nms_neighbors, nms_radius, gamma21, gamma32, min_neighbors)
    if not isinstance(return_saliency, (bool, np.bool_)):
        raise TypeError(f"return_saliency must be True or False, not {return_saliency!r}")
    if _is_device_tensor(X) or type(X).__module__.startswith("torch"):
        return _keypoints_on_device(X, a, bool(return_saliency))
    X, n = _host_points(X)
    if n == 0:
        keep = np.zeros(0, bool)
        return (keep, np.empty(0), np.empty((0, 3)), dict(_NO_KEYPOINTS)) if return_saliency else keep
    _check_keypoint_counts(n, a)
    ctx = _host_opening("keypoint_keep", "choose the keypoints", X, ("keypoints", "ISS keypoints"))
    keep, sal, eig, st = ctx.keypoints(_lib.FIX, *a, want_saliency=bool(return_saliency))
    return (keep, sal, eig, _lib._stats_dict(st)) if return_saliency else keep


def _keypoints_on_device(X, a, return_saliency):
    import torch
    from .tensors import _keep_opening
    if isinstance(X, torch.Tensor) and X.dim() == 2 and X.shape[0] > 0:
        _check_keypoint_counts(X.shape[0], a)
    ctx, n, _, keep = _keep_opening("keypoint_keep", X, None, needs=("keypoints", "ISS keypoints"))
    sal = torch.empty(n, dtype=torch.float64, device=X.device) if return_saliency else None
    eig = torch.empty((n, 3), dtype=torch.float64, device=X.device) if return_saliency else None
    if ctx is None:
        return (keep, sal, eig, dict(_NO_KEYPOINTS)) if return_saliency else keep
    st = ctx.keypoints(_lib.FIX, *a, keep_ptr=keep.data_ptr(), saliency_ptr=None if sal is None else sal.data_ptr(),
                       eig_ptr=None if eig is None else eig.data_ptr())
    keep = keep.view(torch.bool)
    return (keep, sal, eig, _lib._stats_dict(st)) if return_saliency else keep


# ---- DBSCAN labels (contract (U)) ----

_NO_CLUSTERS = dict(n_points=0, n_core=0, n_border=0, n_noise=0, n_clusters=0, largest_label=0, largest_size=0)


def cluster_arguments(radius, min_points=10):
    """(radius as a float, min_points as an int), checked: ValueError naming the keyword."""
    try:
        r = float(radius)
        ok = not isinstance(radius, (bool, str, bytes)) and math.isfinite(r) and r > 0.0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"radius must be a finite number > 0, not {radius!r}")
    if isinstance(min_points, (bool, float, str, bytes)) or not isinstance(min_points, (int, np.integer)) or not 1 <= int(min_points) < 2**63:
        raise ValueError(f"min_points must be an integer >= 1, not {min_points!r}")
    return r, int(min_points)


def cluster_labels(X, radius, min_points=10, return_core=False, return_info=False):
    """The DBSCAN labels of X as an int32 vector (n,) (contract (U)): a point with at least ``min_points``
    points of X, itself included, strictly closer than ``radius`` is a core point; the clusters are the connected components of the
    core points, labelled 0, 1, 2, ... in the order of their first core point; a point that is not core takes the smallest label
    among its core neighbours' clusters; every other point is noise, -1.  Where no pair of points lies at exactly ``radius`` these
    are ``sklearn.cluster.DBSCAN(eps=radius, min_samples=min_points).fit(X).labels_``.

    X: an (n, 3) array, a PointCloud (all its points, whatever is selected) or a CUDA torch tensor (float32 / float64, any
    strides; ingest and stream rule are run_tensors').  A tensor gives a torch.int32 tensor on its device, anything else numpy.
    ``return_core``: also the (n,) bool core flags; ``return_info``: also the call's record as a dict (n_points, n_core, n_border,
    n_noise, n_clusters, largest_label, largest_size -- of equal sizes the lowest label; no cluster: -1 and 0).  The results come
    as (labels[, core][, info]).  The library's fixed slot holds X afterwards."""
    from .tensors import _is_device_tensor
    r, mp = cluster_arguments(radius, min_points)
    for name, v in (("return_core", return_core), ("return_info", return_info)):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f"{name} must be True or False, not {v!r}")

    def answer(labels, core, info):
        out = (labels,) + ((core,) if return_core else ()) + ((info,) if return_info else ())
        return out if len(out) > 1 else labels
    if _is_device_tensor(X) or type(X).__module__.startswith("torch"):
        return answer(*_cluster_on_device(X, r, mp, bool(return_core)))
    X, n = _host_points(X)
    if n == 0:
        return answer(np.zeros(0, np.int32), np.zeros(0, bool), dict(_NO_CLUSTERS))
    ctx = _host_opening("cluster_labels", "cluster the clouds", X, ("cluster", "clustering"))
    labels, core, st = ctx.cluster(_lib.FIX, r, mp)
    return answer(labels, core, _lib._stats_dict(st))


def _cluster_on_device(X, r, mp, return_core):
    import torch
    from .tensors import _keep_opening
    ctx, n, _, core = _keep_opening("cluster_labels", X, None, needs=("cluster", "clustering"))
    labels = torch.empty(n, dtype=torch.int32, device=X.device)
    if ctx is None:
        return labels, core, dict(_NO_CLUSTERS)
    st = ctx.cluster(_lib.FIX, r, mp, labels_ptr=labels.data_ptr(), core_ptr=core.data_ptr() if return_core else None)
    return labels, core.view(torch.bool), _lib._stats_dict(st)


# ---- planes of a cloud (contracts (P) and (Q)) ----


class PlaneResult:
    """What ``segment_plane`` returns.  ``plane``: (4,) float64, the unit normal and d -- a point x lies on it where
    ``normal . x + d == 0``; ``inliers``: the (n,) bool mask of the candidate rows strictly within ``max_distance`` of it (numpy,
    or a tensor on the input's device); ``n_inliers``: their number; ``info`` (``return_info=True``; else None): the two calls'
    records as dicts, ``{"hypotheses": {n_points, n_candidates, n_hypotheses, n_void, best, best_inliers}, "refit": {n_planes,
    n_void, n_improved, best, best_inliers}}``."""

    def __init__(self, plane, inliers, n_inliers, info=None):
        self.plane, self.inliers, self.n_inliers, self.info = plane, inliers, int(n_inliers), info

    def __repr__(self):
        return f"PlaneResult(plane={self.plane!r}, n_inliers={self.n_inliers})"


def _seed_of(seed):
    """A seed of np.random.default_rng: an integer >= 0, or a sequence of them (segment_planes' [seed, j])."""
    if isinstance(seed, (list, tuple)):
        if not seed:
            raise ValueError("seed must not be empty")
        return [_int_in("seed", s, 0, 2**63 - 1) for s in seed]
    return _int_in("seed", seed, 0, 2**63 - 1)


def plane_arguments(max_distance, hypotheses=1024, seed=0, triples=None, refine=3):
    """(max_distance, hypotheses, seed, triples as (h, 3) int32 or None, refine), checked: TypeError / ValueError.  ``refine`` is
    the number of rounds of the refit, 1 .. 16: the refit is what forms the inlier mask, so there is no ``refine=0``."""
    if isinstance(max_distance, (bool, str, bytes)) or not isinstance(max_distance, (int, float, np.integer, np.floating)):
        raise TypeError(f"max_distance must be a number, not {max_distance!r}")
    d = float(max_distance)
    if not math.isfinite(d) or not d > 0.0:
        raise ValueError(f"max_distance must be finite and > 0, not {max_distance!r}")
    h = _int_in("hypotheses", hypotheses, 1, 2**31 - 1)
    s = _seed_of(seed)
    r = _int_in("refine", refine, 1, _lib.PLANE_MAX_ROUNDS)
    tri = None
    if triples is not None:
        tri = np.asarray(triples)
        if tri.dtype.kind not in "iu":
            raise TypeError(f"triples must be integers, not {tri.dtype}")
        if tri.ndim != 2 or tri.shape[1] != 3 or tri.shape[0] < 1:
            raise ValueError(f"triples must have shape (h, 3) with h >= 1, not {tri.shape}")
        if tri.size and (tri.min() < -2**31 or tri.max() >= 2**31):
            raise ValueError("triples must fit int32")
        tri = np.ascontiguousarray(tri, dtype=np.int32)
    return d, h, s, tri, r


def plane_triples(n, mask, hypotheses, seed):
    """The triples ``segment_plane`` draws, on the host: ``np.random.default_rng(seed).integers(0, n, (hypotheses, 3),
    dtype=np.int32)`` without a mask; with one ``integers(0, k, ...)`` mapped through the ascending indices of the k candidate
    rows (for a tensor mask ``torch.nonzero`` on its device: only the 3 * hypotheses indices move)."""
    rng = np.random.default_rng(seed)
    if mask is None:
        return rng.integers(0, n, (hypotheses, 3), dtype=np.int32)
    if type(mask).__module__.startswith("torch"):
        import torch
        rows = torch.nonzero(mask).squeeze(1)
        at = rng.integers(0, rows.numel(), (hypotheses, 3), dtype=np.int32)
        picked = rows[torch.as_tensor(at.ravel().astype(np.int64), device=rows.device)].cpu().numpy()
        return np.ascontiguousarray(picked.reshape(hypotheses, 3), dtype=np.int32)
    rows = np.flatnonzero(mask)
    return np.ascontiguousarray(rows[rng.integers(0, len(rows), (hypotheses, 3), dtype=np.int32)], dtype=np.int32)


def _rows_and_mask(X, mask):
    """(on_device, the rows as the entries read them -- float64, contiguous --, the mask as contiguous bool or None, n): the
    cloud and the mask of a call over a cloud's rows, checked."""
    from .pointcloud import PointCloud
    from .tensors import _check_cloud, _is_device_tensor
    if _is_device_tensor(X) or type(X).__module__.startswith("torch"):
        import torch
        _check_cloud("X", X, backend.default_device())
        n = X.shape[0]
        if mask is not None:
            if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8) or tuple(mask.shape) != (n,):
                raise TypeError("mask must be a bool or uint8 torch.Tensor of shape (n,)")
            if mask.device != X.device:
                raise ValueError(f"mask is on {mask.device}, X on {X.device}")
            mask = (mask != 0).contiguous()
        rows, on_device = X.to(torch.float64).contiguous(), True
    else:
        rows = np.ascontiguousarray(X.X if isinstance(X, PointCloud) else X, dtype=np.float64)
        if rows.ndim != 2 or rows.shape[1] != 3:
            raise ValueError("X must be a PointCloud, an (n, 3) array or a CUDA tensor")
        n, on_device = rows.shape[0], False
        if mask is not None:
            mask = np.asarray(mask)
            if mask.dtype.kind not in "bui" or mask.shape != (n,):
                raise TypeError(f"mask must be a bool or integer array of shape ({n},)")
            mask = np.ascontiguousarray(mask != 0)
    if n >= 2**31:
        raise ValueError("X must have fewer than 2^31 rows")
    return on_device, rows, mask, n


def _plane_rows(X, mask):
    """_rows_and_mask, and k, the number of candidate rows: a plane needs three."""
    on_device, rows, mask, n = _rows_and_mask(X, mask)
    k = n if mask is None else int(mask.sum())
    if k < 3:
        raise ValueError(f"a plane needs at least 3 candidate rows, not {k}")
    return on_device, rows, mask, n, k


def _plane_context(who, ctx=None):
    if dist.is_distributed():
        from .icp import SimpleICPException
        raise SimpleICPException(f"{who} does not run in a torch.distributed job: segment the clouds with one process first")
    ctx = ctx or backend.get_context()
    if not hasattr(ctx, "plane_triplets") or not hasattr(ctx, "plane_refit"):
        raise _lib.BackendError("this backend has no plane segmentation")
    dist.detach(ctx)
    return ctx


def _segment_plane(ctx, on_device, rows, mask, n, d, h, seed, tri, rounds, return_info):
    """segment_plane behind its checks; None when no hypothesis is valid."""
    if tri is None:
        tri = plane_triples(n, mask, h, seed)
    if on_device:
        import torch
        from .tensors import _wait_for_torch
        m8 = None if mask is None else mask.view(torch.uint8)
        keep = torch.empty(n, dtype=torch.uint8, device=rows.device)
        _wait_for_torch(ctx, rows.device)             # (the float64 copy, the mask's bytes and torch.nonzero come first)
        mp = None if m8 is None else m8.data_ptr()
        planes, inl = np.empty((len(tri), 4), np.float64), np.empty(len(tri), np.int32)
        st = _lib._stats_dict(ctx.plane_triplets(rows.data_ptr(), tri.ctypes.data, d, mask=mp, n=n, h=len(tri), planes_ptr=planes.ctypes.data,
                                                 inliers_ptr=inl.ctypes.data))
    else:
        planes, inl, st = ctx.plane_triplets(rows, tri, d, mask=mask)
        st = _lib._stats_dict(st)
    if st["best"] < 0:
        return None
    start = np.ascontiguousarray(planes[st["best"]:st["best"] + 1], dtype=np.float64)
    if on_device:
        out, cnt = np.empty((1, 4), np.float64), np.empty(1, np.int32)
        st2 = ctx.plane_refit(rows.data_ptr(), start.ctypes.data, d, rounds, mask=mp, n=n, b=1, planes_ptr=out.ctypes.data,
                              inliers_ptr=cnt.ctypes.data, keep_ptr=keep.data_ptr())
        keep = keep.view(torch.bool)
    else:
        out, cnt, keep, st2 = ctx.plane_refit(rows, start, d, rounds, mask=mask, want_keep=True)
    info = {"hypotheses": st, "refit": _lib._stats_dict(st2)} if return_info else None
    return PlaneResult(np.array(out[0], dtype=np.float64), keep, int(cnt[0]), info)


def segment_plane(X, max_distance, *, hypotheses=1024, seed=0, triples=None, refine=3, mask=None, return_info=False):
    """The dominant plane of X -- ground, floor, table, wall -- by RANSAC (contracts (P) and (Q)): every
    triple of points gives one plane, a plane's score is the number of candidate rows strictly within ``max_distance`` of it, and
    the best plane is refitted on its own inliers in ``refine`` rounds (the least-squares plane of the inliers; what comes back
    never has fewer inliers than the best hypothesis).  ``X[~segment_plane(X, d).inliers]`` is the cloud without it: what
    ``cluster_labels`` takes apart into objects.  Open3D's ``segment_plane``, reproducible bit for bit.

    X: an (n, 3) array, a PointCloud (all its points, whatever is selected) or a CUDA torch tensor (float32 / float64, any strides;
    float32 is widened exactly, the rows stay on the device; the stream rule is run_tensors').  ``mask`` (n,): only the rows it
    marks are candidates -- they alone count and define planes; bool / integer array, or a bool / uint8 tensor on X's device.
    ``triples``: (h, 3) integers; None: drawn on the host from ``seed`` (``plane_triples``; a repeated index is simply a void
    hypothesis).  ``refine``: rounds of the refit, 1 .. 16 -- the refit forms the inlier mask, so 0 is refused with ValueError.
    Returns a ``PlaneResult``; ValueError when no hypothesis is valid (fewer than three candidates, or all triples degenerate)."""
    d, h, s, tri, r = plane_arguments(max_distance, hypotheses, seed, triples, refine)
    if not isinstance(return_info, (bool, np.bool_)):
        raise TypeError(f"return_info must be True or False, not {return_info!r}")
    on_device, rows, mask, n, _ = _plane_rows(X, mask)
    res = _segment_plane(_plane_context("segment_plane"), on_device, rows, mask, n, d, h, s, tri, r, bool(return_info))
    if res is None:
        raise ValueError("no hypothesis is valid: every triple is degenerate, repeats a row or names a row that is no candidate")
    return res


def segment_planes(X, max_distance, *, min_inliers, max_planes=4, hypotheses=1024, seed=0, refine=3):
    """The planes of X, peeled off one after the other: round j is ``segment_plane`` on the rows no plane has taken yet
    (``mask = labels == -1``) with ``seed = [seed, j]``; it stops after ``max_planes`` planes, when a plane has fewer than
    ``min_inliers`` inliers (that plane is dropped), when fewer than three rows are left, or when no hypothesis is valid.
    ``min_inliers`` has no default: it is what tells a plane from clutter in the caller's scene.

    Returns ``(labels, planes)``: (n,) int32 -- -1, or 0, 1, ... in the order of extraction; numpy, or a tensor on X's device --
    and the (k, 4) float64 planes."""
    d, h, s, _, r = plane_arguments(max_distance, hypotheses, seed, None, refine)
    if isinstance(s, list):
        raise TypeError("seed must be one integer: round j draws from [seed, j]")
    most = _int_in("max_planes", max_planes, 1, 2**31 - 1)
    least = _int_in("min_inliers", min_inliers, 1, 2**31 - 1)
    on_device, rows, _, n, _ = _plane_rows(X, None)
    ctx = _plane_context("segment_planes")
    if on_device:
        import torch
        labels = torch.full((n,), -1, dtype=torch.int32, device=rows.device)
    else:
        labels = np.full(n, -1, np.int32)
    planes = []
    for j in range(most):
        left = labels == -1
        if int(left.sum()) < 3:
            break
        res = _segment_plane(ctx, on_device, rows, left, n, d, h, [s, j], None, r, False)
        if res is None or res.n_inliers < least:
            break
        labels[res.inliers] = j
        planes.append(res.plane)
    return labels, np.array(planes, dtype=np.float64).reshape(-1, 4)


# ---- farthest point sampling (contract (S)) ----


def farthest_arguments(count, start=None):
    """(count, start as the C entry takes it: a row, or -1 for None), checked: TypeError / ValueError."""
    c = _int_in("count", count, 1, 2**31 - 1)
    s = -1 if start is None else _int_in("start", start, 0, 2**31 - 2)
    return c, s


def _farthest_context(who, ctx=None):
    if dist.is_distributed():
        from .icp import SimpleICPException
        raise SimpleICPException(f"{who} does not run in a torch.distributed job: sample the clouds with one process first")
    ctx = ctx or backend.get_context()
    if not hasattr(ctx, "farthest"):
        raise _lib.BackendError("this backend has no farthest point sampling")
    dist.detach(ctx)
    return ctx


def _farthest(ctx, on_device, rows, mask, n, count, start, want_d2):
    """farthest_points behind its checks: (picks in pick order, their squared distances or None, the record as a dict)."""
    m = min(count, n)                               # (no more picks than rows: the result is not padded)
    if on_device:
        import torch
        from .tensors import _wait_for_torch
        idx = torch.empty(m, dtype=torch.int64, device=rows.device)
        d2 = torch.empty(m, dtype=torch.float64, device=rows.device) if want_d2 else None
        m8 = None if mask is None else mask.view(torch.uint8)
        _wait_for_torch(ctx, rows.device)             # (the float64 copy and the mask's bytes come first)
        st = ctx.farthest(rows.data_ptr(), m, start, mask=None if m8 is None else m8.data_ptr(), n=n, idx_ptr=idx.data_ptr(),
                          d2_ptr=None if d2 is None else d2.data_ptr())
    else:
        idx, d2, st = ctx.farthest(rows, m, start, mask=mask, want_d2=want_d2)
    st = _lib._stats_dict(st)
    k = st["n_selected"]
    return idx[:k], None if d2 is None else d2[:k], st


def farthest_points(X, count, *, start=None, mask=None, return_distances=False, return_info=False):
    """Farthest point sampling (contract (S)): ``count`` rows of X, evenly spread in space -- the first is
    ``start`` (None: the lowest candidate row), every further one the candidate row farthest from all rows taken so far, the
    lowest row among equally far ones.  Open3D's ``farthest_point_down_sample`` and pytorch3d's ``sample_farthest_points``,
    reproducible bit for bit; ``X[farthest_points(X, 1000)]`` is the sample.  A sequence, not a set: the first k picks are the
    picks for ``count=k``.

    X: an (n, 3) array, a PointCloud (all its points, whatever is selected) or a CUDA torch tensor (float32 / float64, any strides;
    float32 is widened exactly, the rows stay on the device; the stream rule is run_tensors').  ``mask`` (n,): only the rows it
    marks are candidates; bool / integer array, or a bool / uint8 tensor on X's device.  A row with a coordinate that is not
    finite is never a candidate.  Returns the picks in pick order, int64 -- numpy, or a tensor on X's device --, as many as were
    taken: fewer than ``count`` where the candidates hold fewer distinct points (an exact duplicate of a taken row is never
    taken) or X has fewer rows, none where ``start`` is no candidate.  ``return_distances=True``: also the (k,) float64 SQUARED
    distance of every pick to the picks before it (+inf for the first) -- they never increase, entry t is the covering radius
    of the first t picks.  ``return_info=True``: also the record, ``{n_points, n_candidates, n_selected, cover_d2}``."""
    c, s = farthest_arguments(count, start)
    for name, flag in (("return_distances", return_distances), ("return_info", return_info)):
        if not isinstance(flag, (bool, np.bool_)):
            raise TypeError(f"{name} must be True or False, not {flag!r}")
    on_device, rows, mask, n = _rows_and_mask(X, mask)
    if n == 0:
        raise ValueError("X has no rows")
    if s >= n:
        raise ValueError(f"start must be a row of X, 0 .. {n - 1}, not {start!r}")
    idx, d2, st = _farthest(_farthest_context("farthest_points"), on_device, rows, mask, n, c, s, bool(return_distances))
    out = (idx,) + ((d2,) if return_distances else ()) + ((st,) if return_info else ())
    return out[0] if len(out) == 1 else out


# ---- consistent normal orientation (contract (H)) ----

_NO_ORIENT = dict(n_points=0, n_void=0, n_components=0, n_forest_edges=0, n_flipped=0, n_components_voted=0, rounds=0)


def _count_of(name, v, lo, hi):
    if isinstance(v, (bool, float, str, bytes)) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{name} must be an integer >= {lo} and <= {hi}, not {v!r}")
    return int(v)


def _point_of(name, v):
    try:
        r = np.asarray(v, dtype=np.float64)
        ok = r.shape == (3,) and bool(np.isfinite(r).all())
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{name} must be three finite numbers, not {v!r}")
    return r


def orient_arguments(neighbors=16, normal_neighbors=10, viewpoint=None, away_from=None):
    """(k, normal_neighbors, the vote's reference as three floats or None, away), checked: ValueError naming the keyword."""
    k = _count_of("neighbors", neighbors, 2, _lib.FPFH_MAX_K)
    kn = _count_of("normal_neighbors", normal_neighbors, 2, 2**31 - 1)
    if viewpoint is not None and away_from is not None:
        raise ValueError("viewpoint and away_from exclude each other: a component is turned towards the one or away from the other")
    if viewpoint is not None:
        return k, kn, _point_of("viewpoint", viewpoint), False
    if away_from is not None:
        return k, kn, _point_of("away_from", away_from), True
    return k, kn, None, False


def orient_normals(X, normals=None, *, neighbors=16, normal_neighbors=10, viewpoint=None, away_from=None, return_flipped=False,
                   return_info=False):
    """The normals of X with consistent signs, (n, 3) float32 (contract (H)): neighbouring normals are made
    to agree along the minimum spanning forest of the k-NN graph (``neighbors`` = k, the point itself included, 2 .. 128), the
    edges ordered by how parallel their normals are -- Hoppe's propagation, Open3D's ``orient_normals_consistent_tangent_plane``,
    reproducible bit for bit.  A normal is only ever negated, never changed.  In every connected component of the graph the
    lowest-index point keeps its sign; with ``viewpoint`` (three numbers) a component is then turned as a whole so that most of
    its normals look towards it, with ``away_from`` so that most look away from it (one vote per component, not per point: a
    grazing angle is one vote among many); a tie leaves it.  The two exclude each other.

    X: an (n, 3) array, a PointCloud (all its points, whatever is selected) or a CUDA torch tensor (float32 / float64, any
    strides; ingest and stream rule are run_tensors').  A tensor gives a torch tensor on its device, anything else numpy.
    ``normals``: (n, 3), one per point; None: a PointCloud's own nx / ny / nz columns if it has them, else the library's normals
    from ``normal_neighbors`` points -- as ``fpfh_features`` chooses them.  A normal with a component that is not finite, or all
    zero, stands alone and stays.  ``return_flipped``: also the (n,) bool mask of the negated normals; ``return_info``: also the
    call's record as a dict (n_points, n_void, n_components -- void points included --, n_forest_edges, n_flipped,
    n_components_voted -- the components the vote turned --, rounds).  The results come as (normals[, flipped][, info]).  The
    library's fixed slot holds X afterwards."""
    from .pointcloud import PointCloud
    from .tensors import _is_device_tensor
    k, kn, ref, away = orient_arguments(neighbors, normal_neighbors, viewpoint, away_from)
    for name, v in (("return_flipped", return_flipped), ("return_info", return_info)):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f"{name} must be True or False, not {v!r}")

    def answer(out, flipped, info):
        res = (out,) + ((flipped,) if return_flipped else ()) + ((info,) if return_info else ())
        return res if len(res) > 1 else out
    if _is_device_tensor(X) or type(X).__module__.startswith("torch"):
        return answer(*_orient_on_device(X, normals, k, kn, ref, away))
    X, n = _host_points(X)
    own = None
    if isinstance(X, PointCloud) and normals is None and all(c in X for c in ("nx", "ny", "nz")):
        own = np.stack([np.asarray(X[c].to_numpy(), dtype=np.float32) for c in ("nx", "ny", "nz")], axis=1)
    if normals is not None:
        own = np.ascontiguousarray(normals, dtype=np.float32)
        if own.shape != (n, 3):
            raise ValueError(f"normals must have shape ({n}, 3), not {own.shape}")
    if n == 0:
        return answer(np.empty((0, 3), np.float32), np.zeros(0, bool), dict(_NO_ORIENT))
    _check_counts(n, k, kn, own is None)
    ctx = _host_opening("orient_normals", "orient the normals", X, ("orient", "normal orientation"))
    if own is None:
        own = ctx.estimate_normals(_lib.FIX, np.arange(n, dtype=np.int64), kn)[0]
    out, flipped, st = ctx.orient(_lib.FIX, own, k, ref, away)
    return answer(out, flipped, _lib._stats_dict(st))


def _orient_on_device(X, normals, k, kn, ref, away):
    import torch
    from .tensors import _keep_opening, _wait_for_torch
    if normals is not None and not isinstance(normals, (torch.Tensor, np.ndarray)):
        raise ValueError("normals must be a torch.Tensor or a numpy array of shape (n, 3)")
    if isinstance(X, torch.Tensor) and X.dim() == 2:
        if normals is not None and tuple(normals.shape) != (X.shape[0], 3):
            raise ValueError(f"normals must have shape ({X.shape[0]}, 3), not {tuple(normals.shape)}")
        if X.shape[0] > 0:
            _check_counts(X.shape[0], k, kn, normals is None)
    ctx, n, _, flipped = _keep_opening("orient_normals", X, None, needs=("orient", "normal orientation"))
    dev = X.device
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    if ctx is None:
        return out, flipped, dict(_NO_ORIENT)
    if normals is None:               # the library's normals of all points, left in device memory: they are oriented in place
        sel = torch.arange(n, dtype=torch.int64, device=dev)
        pl = torch.empty(n, dtype=torch.float32, device=dev)
        nv = out
    elif isinstance(normals, torch.Tensor):
        if normals.device != dev:
            raise ValueError(f"normals is on {normals.device}, X on {dev}")
        nv = normals.to(torch.float32).contiguous()
    else:
        nv = torch.from_numpy(np.ascontiguousarray(normals, dtype=np.float32)).to(dev)
    # what torch queued for this call on its current stream (the index vector, the normals' copy) comes before the library reads it
    _wait_for_torch(ctx, dev)
    if normals is None:
        ctx.estimate_normals_into(_lib.FIX, sel.data_ptr(), n, kn, nv.data_ptr(), pl.data_ptr())
    st = ctx.orient(_lib.FIX, nv, k, ref, away, normals_ptr=out.data_ptr(), flipped_ptr=flipped.data_ptr())
    return out, flipped.view(torch.bool), _lib._stats_dict(st)


# ---- smooth regions (contract (J)) ----

_NO_REGIONS = dict(n_points=0, n_void=0, n_smooth=0, n_border=0, n_regions_all=0, n_regions=0, n_labelled=0, largest_label=0,
                   largest_size=0)


def _number_of(name, v):
    if isinstance(v, (bool, str, bytes)) or not isinstance(v, (int, float, np.integer, np.floating)) or math.isnan(float(v)):
        raise ValueError(f"{name} must be a number, not {v!r}")
    return float(v)


def regions_arguments(neighbors=16, max_angle=5.0, cos_min=None, radius=None, min_planarity=None, min_size=1, oriented=False,
                      normal_neighbors=10):
    """(k, cos_min, radius as a float -- inf: none --, min_planarity or None, min_size, oriented, normal_neighbors), checked:
    ValueError naming the keyword.  cos_min = math.cos(math.radians(max_angle)) unless it is given itself."""
    if not isinstance(oriented, (bool, np.bool_)):
        raise ValueError(f"oriented must be True or False, not {oriented!r}")
    k = _count_of("neighbors", neighbors, 2, _lib.FPFH_MAX_K)
    kn = _count_of("normal_neighbors", normal_neighbors, 2, 2**31 - 1)
    if cos_min is not None:
        if max_angle is not None and max_angle != 5.0:
            raise ValueError("cos_min and max_angle exclude each other: the one is the cosine of the other")
        cm, lo = _number_of("cos_min", cos_min), -1.0 if oriented else 0.0
        if not lo <= cm <= 1.0:
            raise ValueError(f"cos_min must be >= {lo:g} and <= 1, not {cos_min!r}")
    else:
        a, hi = _number_of("max_angle", max_angle), 180.0 if oriented else 90.0
        if not 0.0 < a <= hi:
            raise ValueError(f"max_angle must be > 0 and <= {hi:g} degrees, not {max_angle!r}")
        cm = math.cos(math.radians(a))
    try:
        r = _radius_of("radius", radius)
    except TypeError as e:
        raise ValueError(str(e)) from None
    mp = None
    if min_planarity is not None:
        mp = _number_of("min_planarity", min_planarity)
    ms = _count_of("min_size", min_size, 1, 2**63 - 1)
    return k, cm, r, mp, ms, bool(oriented), kn


def smooth_regions(X, normals=None, *, neighbors=16, max_angle=5.0, cos_min=None, radius=None, seeds=None, min_planarity=None,
                   min_size=1, oriented=False, normal_neighbors=10, return_info=False):
    """The smooth regions of X as an int32 vector (n,) (contract (J)): region growing over the normals,
    PCL's ``RegionGrowing``.  Two points are joined where one is among the other's ``neighbors`` nearest points (the point itself
    included, 2 .. 128; with ``radius`` only those strictly closer) and their normals differ by at most ``max_angle`` degrees --
    unoriented, |dot| >= cos(max_angle), unless ``oriented`` (then ``max_angle`` may go up to 180).  ``cos_min`` gives the cosine
    itself instead of ``max_angle``.  Every patch of the surface, flat or curved, becomes one region and patches end where the
    surface creases; regions are numbered 0, 1, 2, ... in the order of their lowest index, -1 is no region.  The result depends
    on the inputs alone -- no queue order as in PCL.

    ``seeds`` ((n,) bool): only these points pass a label on; a point that is no seed joins the region with the lowest root among
    the seeds it agrees with and never connects two regions.  ``min_planarity=p`` with the library's own normals
    (``normals=None``) makes ``seeds = planarity >= p`` (NaN: no seed): PCL's curvature threshold.  Regions of fewer than
    ``min_size`` members get -1, the others are renumbered.

    X: an (n, 3) array, a PointCloud (all its points, whatever is selected) or a CUDA torch tensor (float32 / float64, any
    strides; ingest and stream rule are run_tensors').  A tensor gives a torch.int32 tensor on its device, anything else numpy;
    a tensor's rows, normals and seeds never leave the device.  ``normals``: (n, 3), one per point; None: a PointCloud's own
    nx / ny / nz columns if it has them, else the library's normals from ``normal_neighbors`` points.  A normal with a component
    that is not finite, or all zero, belongs to no region.  ``return_info``: also the call's record as a dict (n_points, n_void,
    n_smooth, n_border, n_regions_all, n_regions, n_labelled, largest_label, largest_size -- no region: -1 and 0 -- and cos_min).
    The library's fixed slot holds X afterwards."""
    from .pointcloud import PointCloud
    from .tensors import _is_device_tensor
    k, cm, r, mp, ms, oriented, kn = regions_arguments(neighbors, max_angle, cos_min, radius, min_planarity, min_size, oriented,
                                                       normal_neighbors)
    if not isinstance(return_info, (bool, np.bool_)):
        raise ValueError(f"return_info must be True or False, not {return_info!r}")
    if mp is not None and seeds is not None:
        raise ValueError("min_planarity and seeds exclude each other: min_planarity makes the seeds")
    if mp is not None and normals is not None:
        raise ValueError("min_planarity needs the library's own normals (normals=None): given normals come without a planarity")

    def answer(labels, info):
        return (labels, dict(info, cos_min=cm)) if return_info else labels
    if _is_device_tensor(X) or type(X).__module__.startswith("torch"):
        return answer(*_regions_on_device(X, normals, seeds, k, cm, r, mp, ms, oriented, kn))
    X, n = _host_points(X)
    own = None
    if isinstance(X, PointCloud) and normals is None and mp is None and all(c in X for c in ("nx", "ny", "nz")):
        own = np.stack([np.asarray(X[c].to_numpy(), dtype=np.float32) for c in ("nx", "ny", "nz")], axis=1)
    if normals is not None:
        own = np.ascontiguousarray(normals, dtype=np.float32)
        if own.shape != (n, 3):
            raise ValueError(f"normals must have shape ({n}, 3), not {own.shape}")
    if seeds is not None:
        seeds = np.ascontiguousarray(np.asarray(seeds) != 0)
        if seeds.shape != (n,):
            raise ValueError(f"seeds must have shape ({n},), not {seeds.shape}")
    if n == 0:
        return answer(np.zeros(0, np.int32), dict(_NO_REGIONS))
    _check_counts(n, k, kn, own is None)
    ctx = _host_opening("smooth_regions", "label the clouds", X, ("regions", "smooth regions"))
    if own is None:
        own, pl = ctx.estimate_normals(_lib.FIX, np.arange(n, dtype=np.int64), kn)
        if mp is not None:
            with np.errstate(invalid="ignore"):
                seeds = pl.astype(np.float64) >= mp
    labels, st = ctx.regions(_lib.FIX, own, k, cm, r, oriented, seeds, ms)
    return answer(labels, _lib._stats_dict(st))


def _regions_on_device(X, normals, seeds, k, cm, r, mp, ms, oriented, kn):
    import torch
    from .tensors import _keep_opening, _wait_for_torch
    if normals is not None and not isinstance(normals, (torch.Tensor, np.ndarray)):
        raise ValueError("normals must be a torch.Tensor or a numpy array of shape (n, 3)")
    if seeds is not None and not isinstance(seeds, (torch.Tensor, np.ndarray)):
        raise ValueError("seeds must be a torch.Tensor or a numpy array of shape (n,)")
    if isinstance(X, torch.Tensor) and X.dim() == 2:
        if normals is not None and tuple(normals.shape) != (X.shape[0], 3):
            raise ValueError(f"normals must have shape ({X.shape[0]}, 3), not {tuple(normals.shape)}")
        if seeds is not None and tuple(seeds.shape) != (X.shape[0],):
            raise ValueError(f"seeds must have shape ({X.shape[0]},), not {tuple(seeds.shape)}")
        if X.shape[0] > 0:
            _check_counts(X.shape[0], k, kn, normals is None)
    ctx, n, _, _ = _keep_opening("smooth_regions", X, None, needs=("regions", "smooth regions"))
    dev = X.device
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    if ctx is None:
        return labels, dict(_NO_REGIONS)
    pl = None
    if normals is None:               # the library's normals of all points, left in device memory
        sel = torch.arange(n, dtype=torch.int64, device=dev)
        nv = torch.empty((n, 3), dtype=torch.float32, device=dev)
        pl = torch.empty(n, dtype=torch.float32, device=dev)
    elif isinstance(normals, torch.Tensor):
        if normals.device != dev:
            raise ValueError(f"normals is on {normals.device}, X on {dev}")
        nv = normals.to(torch.float32).contiguous()
    else:
        nv = torch.from_numpy(np.ascontiguousarray(normals, dtype=np.float32)).to(dev)
    sd = None
    if isinstance(seeds, torch.Tensor):
        if seeds.device != dev:
            raise ValueError(f"seeds is on {seeds.device}, X on {dev}")
        sd = (seeds != 0).contiguous().view(torch.uint8)
    elif seeds is not None:
        sd = torch.from_numpy(np.ascontiguousarray(np.asarray(seeds) != 0).view(np.uint8)).to(dev)
    # what torch queued for this call on its current stream (the index vector, the copies) comes before the library reads it
    _wait_for_torch(ctx, dev)
    if normals is None:
        ctx.estimate_normals_into(_lib.FIX, sel.data_ptr(), n, kn, nv.data_ptr(), pl.data_ptr())
        if mp is not None:
            # the planarity was written on the library's stream: torch's waits for it, and the library's for the comparison
            ext = torch.cuda.ExternalStream(ctx.stream_ptr(), device=dev)
            torch.cuda.current_stream(dev).wait_stream(ext)
            sd = (pl.to(torch.float64) >= mp).view(torch.uint8)
            _wait_for_torch(ctx, dev)
    st = ctx.regions(_lib.FIX, nv, k, cm, r, oriented, sd, ms, labels_ptr=labels.data_ptr())
    return labels, _lib._stats_dict(st)


# ---- moving-least-squares smoothing (contract (W)) ----

_NO_DENOISE = dict(n_points=0, n_small=0, n_moved=0, n_clipped=0, max_displacement=0.0)


def denoise_arguments(neighbors=16, radius=None, bandwidth=None, strength=1.0, min_neighbors=3, rounds=1):
    """(k, radius as a float -- inf: none --, bandwidth likewise, strength, min_neighbors, rounds), checked: ValueError naming the
    keyword."""
    k = _count_of("neighbors", neighbors, 2, _lib.KEYPOINTS_MAX_K)
    try:
        r, b = _radius_of("radius", radius), _radius_of("bandwidth", bandwidth)
    except TypeError as e:
        raise ValueError(str(e)) from None
    s = _number_of("strength", strength)
    if not 0.0 <= s <= 1.0:
        raise ValueError(f"strength must be >= 0 and <= 1, not {strength!r}")
    return k, r, b, s, _count_of("min_neighbors", min_neighbors, 1, 2**62), _count_of("rounds", rounds, 1, 2**31 - 1)


def denoise_points(X, *, neighbors=16, radius=None, bandwidth=None, strength=1.0, min_neighbors=3, rounds=1, return_normals=False,
                   return_displacement=False, return_info=False):
    """X smoothed by moving least squares at order 0/1 as an (n, 3) float64 array (contract (W)): every point
    is projected onto the plane fitted to its ``neighbors`` nearest points (the point itself included, 2 .. 128; with ``radius``
    only those strictly closer) -- PCL's ``MovingLeastSquares`` without a polynomial, CloudCompare's "MLS smooth".  The plane goes
    through the weighted mean of the support, its normal is the eigenvector of the smallest eigenvalue of the weighted covariance;
    ``bandwidth=b`` weighs a neighbour at squared distance d2 by (1 - d2 / b^2)^2 where that is positive, else 0 (None: all 1).
    The point moves by ``strength`` (0 .. 1) times its signed distance along the normal; one with fewer than ``min_neighbors``
    counted neighbours stays where it is.  All points are projected from the input positions, none sees another's output: the
    result depends on the inputs alone, bit for bit.  ``rounds`` > 1 feeds each round's output to the next as a cloud of its own.

    X: an (n, 3) array, a PointCloud (all its points, whatever is selected) or a CUDA torch tensor (float32 / float64, any
    strides; ingest and stream rule are run_tensors').  A tensor gives a torch tensor on its device, anything else numpy; a
    tensor's rows never leave the device.  The result is always float64: on a georeferenced cloud a float32 store would swallow
    the displacement.  ``return_normals``: also the planes' (n, 3) float32 normals (largest component positive; zeros where the
    point stayed for want of neighbours); ``return_displacement``: also the (n,) float64 signed displacements, out = x - g *
    normal; ``return_info``: also the call's record as a dict (n_points, n_small, n_moved, n_clipped -- the balls that held more
    points than ``neighbors`` --, max_displacement, and rounds) -- all three those of the last round.  The results come as
    (points[, normals][, displacement][, info]).  The library's fixed slot holds the last round's input afterwards."""
    from .tensors import _is_device_tensor
    a = denoise_arguments(neighbors, radius, bandwidth, strength, min_neighbors, rounds)
    for name, v in (("return_normals", return_normals), ("return_displacement", return_displacement), ("return_info", return_info)):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f"{name} must be True or False, not {v!r}")

    def answer(points, normals, displacement, info):
        out = ((points,) + ((normals,) if return_normals else ()) + ((displacement,) if return_displacement else ())
               + ((dict(info, rounds=a[5]),) if return_info else ()))
        return out if len(out) > 1 else points
    if _is_device_tensor(X) or type(X).__module__.startswith("torch"):
        return answer(*_denoise_on_device(X, a, bool(return_normals), bool(return_displacement)))
    X, n = _host_points(X)
    if n == 0:
        return answer(np.empty((0, 3), np.float64), np.empty((0, 3), np.float32), np.empty(0, np.float64), dict(_NO_DENOISE))
    if a[0] > n:
        raise ValueError(f"neighbors ({a[0]}) exceeds the number of points ({n})")
    for r in range(a[5]):
        last = r == a[5] - 1
        ctx = _host_opening("denoise_points", "smooth the clouds", X, ("denoise", "denoising"))
        X, nrm, disp, st = ctx.denoise(_lib.FIX, *a[:5], want_normals=last and bool(return_normals),
                                       want_displacement=last and bool(return_displacement))
    return answer(X, nrm, disp, _lib._stats_dict(st))


def _denoise_on_device(X, a, return_normals, return_displacement):
    import torch
    from .tensors import _keep_opening
    if isinstance(X, torch.Tensor) and X.dim() == 2 and 0 < X.shape[0] < a[0]:
        raise ValueError(f"neighbors ({a[0]}) exceeds the number of points ({X.shape[0]})")
    for r in range(a[5]):
        last = r == a[5] - 1
        ctx, n, _, _ = _keep_opening("denoise_points", X, None, needs=("denoise", "denoising"))
        dev = X.device
        out = torch.empty((n, 3), dtype=torch.float64, device=dev)
        nrm = torch.empty((n, 3), dtype=torch.float32, device=dev) if last and return_normals else None
        disp = torch.empty(n, dtype=torch.float64, device=dev) if last and return_displacement else None
        if ctx is None:
            return out, nrm, disp, dict(_NO_DENOISE)
        st = ctx.denoise(_lib.FIX, *a[:5], points_ptr=out.data_ptr(), normals_ptr=None if nrm is None else nrm.data_ptr(),
                         displacement_ptr=None if disp is None else disp.data_ptr())
        X = out                       # (the call returned complete: the next round reads what this one wrote)
    return out, nrm, disp, _lib._stats_dict(st)
