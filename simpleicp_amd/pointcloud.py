"""PointCloud -- API mirror of /root/reference/python/simpleicp/pointcloud.py:15-226.

A ``pandas.DataFrame`` with columns ``x, y, z`` (float64), a boolean ``selected`` column and,
after ``estimate_normals``, float32 sparse columns ``nx, ny, nz, planarity`` (NaN where not
estimated) -- exactly the layout the reference's callers see.  The three operators that are
on the ICP hot path run on the GPU through the C ABI (no host fallback):

  select_in_range   -> exact 1-NN with a strict upper bound (pruned grid search; brute force on small clouds)  (pointcloud.py:149-171)
  estimate_normals  -> exact k-NN + covariance + 3x3 eigen (one sweep per query on the grid)              (pointcloud.py:173-203)
  transform_by_H    -> in-place rigid transform, contract (T)       (pointcloud.py:205-217)
"""
from __future__ import annotations

from pathlib import Path
from typing import List

import numpy as np
import pandas as pd

from . import _lib, backend

_PANDAS_MAJOR = int(pd.__version__.split(".")[0])
_XYZ = ["x", "y", "z"]
_ALL = object()          # selection sentinel: "every point" (no index vector materialised)
_ATTRS = ("nx", "ny", "nz", "planarity")

try:                                       # O(selected) construction of the sparse attribute columns
    from pandas._libs.sparse import IntIndex as _IntIndex
except ImportError:                        # pragma: no cover - falls back to the dense constructor
    _IntIndex = None


class PointCloudException(Exception):
    """Raised when the PointCloud class is misused (pointcloud.py:229)."""


def voxel_arguments(voxel_size, origin=None, exc=ValueError):
    """(cell size as a float, origin as three floats) of contract (V), DESIGN.md section 13: the cell finite and > 0, the origin
    (None = zeros) three finite numbers; anything else raises ``exc`` before any device work."""
    try:
        c = float(voxel_size)
        ok = not isinstance(voxel_size, (bool, str, bytes)) and np.isfinite(c) and c > 0.0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise exc("voxel_size must be a finite number > 0.")
    try:
        o = tuple(float(v) for v in ((0.0, 0.0, 0.0) if origin is None else origin))
        ok = len(o) == 3 and all(np.isfinite(v) for v in o)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise exc("voxel_origin must be three finite numbers.")
    return c, o


class PointCloud(pd.DataFrame):
    last_outlier_stats = None             # select_statistical_inliers leaves its statistics here (a dict)
    last_keypoint_stats = None            # select_keypoints leaves its record here (a dict)
    last_plane = None                     # select_plane leaves its PlaneResult here (inliers over the whole cloud)
    last_orient_stats = None              # orient_normals leaves its record here (a dict)
    last_farthest = None                  # select_farthest leaves (picks in pick order, squared distances, record) here
    last_cluster_stats = None             # select_largest_cluster / select_clusters leave their record here (a dict)
    last_region_stats = None              # select_regions / select_largest_region leave their record here (a dict)
    last_denoise_stats = None             # denoise leaves its record here (a dict)

    def __init__(self, *args, **kwargs) -> None:
        kwargs.pop("remapping", None)     # accepted and ignored, like the reference (pointcloud.py:25)
        super().__init__(*args, **kwargs)
        for c in _XYZ:
            if c not in self:
                raise PointCloudException(f'Column "{c}" is missing in DataFrame.')
        self._num_points = len(self)
        if "selected" not in self:
            self["selected"] = np.ones(self._num_points, dtype=bool)

    # ---- views (pointcloud.py:51-110) ---------------------------------------------------
    def _col(self, name, only_selected=False):
        v = self[name].to_numpy()
        return v[self["selected"].to_numpy()] if only_selected else v

    @property
    def x(self) -> np.ndarray:
        return self._col("x")

    @property
    def y(self) -> np.ndarray:
        return self._col("y")

    @property
    def z(self) -> np.ndarray:
        return self._col("z")

    @property
    def x_selected(self) -> np.ndarray:
        return self._col("x", True)

    @property
    def y_selected(self) -> np.ndarray:
        return self._col("y", True)

    @property
    def z_selected(self) -> np.ndarray:
        return self._col("z", True)

    @property
    def X(self) -> np.ndarray:
        """(n,3) float64 copy of the coordinates."""
        return self[_XYZ].to_numpy()

    def _xyz_buffers(self):
        """The coordinates WITHOUT a host copy where the frame's storage allows it (10 M points = 240 MB):
        ("aos", (n,3) C-contiguous read-only view) for a frame still backed by the caller's (n,3) array,
        ("soa", (x, y, z) contiguous vectors) once columns have been assigned; else a gathered copy."""
        cols = [self[c].to_numpy() for c in _XYZ]
        n = len(cols[0])
        if n == 0 or any(c.dtype != np.float64 or c.ndim != 1 for c in cols):
            return "aos", self.X
        ptr = [c.__array_interface__["data"][0] for c in cols]
        if all(c.strides == (24,) for c in cols) and ptr[1] == ptr[0] + 8 and ptr[2] == ptr[0] + 16:
            return "aos", np.lib.stride_tricks.as_strided(cols[0], (n, 3), (24, 8), writeable=False)
        if all(c.strides == (8,) for c in cols):
            return "soa", cols
        return "aos", self.X

    def _upload(self, ctx, slot, lo=0, hi=None, index_base=0, rows=None, background=False):
        """Rows [lo, hi) (of the subset ``rows`` when given) into the library's slot; returns a row getter
        ``rows(idx) -> (len(idx),3)``.  ``background``: the whole cloud on the library's helper thread (`Context.upload_start`); the
        next call that names the slot waits for it."""
        kind, buf = self._xyz_buffers()
        if background and rows is None and lo == 0 and hi is None:
            if kind == "aos":
                ctx.upload_start(slot, xyz=buf, index_base=index_base)
                return lambda idx: buf[idx]
            ctx.upload_start(slot, columns=buf, index_base=index_base)
            return lambda idx: np.column_stack([b[idx] for b in buf])
        if rows is not None:
            part = rows[lo:hi]
            sub = buf[part] if kind == "aos" else np.column_stack([b[part] for b in buf])
            ctx.upload(slot, sub, index_base=index_base)
            return lambda idx: sub[idx]
        hi = self._num_points if hi is None else hi
        if kind == "aos":
            ctx.upload(slot, buf[lo:hi], index_base=index_base)
            return lambda idx: buf[idx]
        ctx.upload_columns(slot, buf[0][lo:hi], buf[1][lo:hi], buf[2][lo:hi], index_base=index_base)
        return lambda idx: np.column_stack([b[idx] for b in buf])

    def _attributes_of(self, idx):
        """(normals (len(idx),3) f32, planarity f32) of the rows ``idx`` (sorted) -- O(len(idx)) on the
        sparse columns estimate_normals creates, dense fallback for columns a caller assigned."""
        out = []
        for c in _ATTRS:
            arr = self[c].array
            if isinstance(arr, pd.arrays.SparseArray) and np.isnan(arr.fill_value) and hasattr(arr.sp_index, "indices"):
                pos_all = arr.sp_index.indices
                v = np.full(len(idx), np.nan, dtype=np.float32)
                if len(pos_all):
                    pos = np.minimum(np.searchsorted(pos_all, idx), len(pos_all) - 1)
                    hit = pos_all[pos] == idx
                    v[hit] = np.asarray(arr.sp_values, dtype=np.float32)[pos[hit]]
                out.append(v)
            else:
                out.append(np.asarray(self[c].to_numpy(), dtype=np.float32)[idx])
        return np.column_stack(out[:3]), out[3]

    def _planarity_pairs(self, rows=None):
        """(positions int64, values float32) of the non-NaN entries of the `planarity` column; positions count
        within ``rows`` (sorted row subset) when given.  O(stored values) on the sparse column estimate_normals
        creates."""
        arr = self["planarity"].array
        if isinstance(arr, pd.arrays.SparseArray) and np.isnan(arr.fill_value) and hasattr(arr.sp_index, "indices"):
            at = np.asarray(arr.sp_index.indices, dtype=np.int64)
            vals = np.asarray(arr.sp_values, dtype=np.float32)
        else:
            dense = np.asarray(self["planarity"].to_numpy(), dtype=np.float32)
            at = np.flatnonzero(~np.isnan(dense))
            vals = dense[at]
        ok = ~np.isnan(vals)
        at, vals = at[ok], vals[ok]
        if rows is None:
            return at, vals
        pos = np.searchsorted(rows, at)
        hit = (pos < len(rows)) & (rows[np.minimum(pos, len(rows) - 1)] == at)
        return pos[hit].astype(np.int64), vals[hit]

    @property
    def X_selected(self) -> np.ndarray:
        return self.loc[self["selected"], _XYZ].to_numpy()

    @property
    def idx_selected(self) -> np.ndarray:
        return np.flatnonzero(self["selected"].to_numpy())

    @idx_selected.setter
    def idx_selected(self, idx_selected: List[int]) -> None:
        self._set_idx_selected(idx_selected)

    def _set_idx_selected(self, idx_selected) -> None:
        """(Internal callers use this instead of ``self.idx_selected = ...``: pandas' __setattr__ evaluates the property's
        GETTER first -- a flatnonzero over all N points -- before it reaches the setter.)"""
        mask = np.zeros(self._num_points, dtype=bool)
        mask[np.asarray(idx_selected, dtype=np.int64)] = True
        self["selected"] = mask

    @property
    def num_points(self) -> int:
        return self._num_points

    @property
    def num_selected_points(self) -> int:
        return int(np.count_nonzero(self["selected"].to_numpy()))

    # ---- selection (pointcloud.py:112-171) ----------------------------------------------
    def select_all_points(self) -> None:
        self["selected"] = np.ones(self._num_points, dtype=bool)

    def unselect_all_points(self) -> None:
        self["selected"] = np.zeros(self._num_points, dtype=bool)

    def select_by_indices(self, indices: List[int]) -> None:
        """Keeps the currently selected points whose index is in ``indices``."""
        self._set_idx_selected(np.intersect1d(self.idx_selected, indices))

    def select_n_points(self, n: int, _cur=None):
        """Equidistant sub-sampling of the current selection (np.round = half-to-even;
        duplicates collapse, so fewer than n points may remain) -- pointcloud.py:132-147.
        (Internal callers pass the selection they already hold -- ``_ALL`` for "every point", which spares a pass over
        the mask and an index vector of N entries -- and get the new one back.)"""
        if _cur is _ALL:
            if self._num_points > n:
                cur = np.unique(np.round(np.linspace(0, self._num_points - 1, n)).astype(np.int64))
                self._set_idx_selected(cur)
                return cur
            return np.arange(self._num_points, dtype=np.int64)
        cur = self.idx_selected if _cur is None else _cur
        if len(cur) > n:
            pos = np.round(np.linspace(0, len(cur) - 1, n)).astype(int)
            cur = np.unique(cur[pos])
            self._set_idx_selected(cur)
        return cur if _cur is not None else None

    def _selection(self):
        """``_ALL`` when every point is selected (one vectorised count over the mask), else the selected indices."""
        mask = self["selected"].to_numpy()
        if int(np.count_nonzero(mask)) == self._num_points:
            return _ALL
        return np.flatnonzero(mask)

    def _keep_selected(self, cur, near):
        """Narrows the selection ``cur`` (``_ALL`` or sorted indices) to the entries flagged in ``near`` (one 0/1 byte
        per entry of ``cur``); writes the `selected` column and returns the new index vector."""
        near = np.asarray(near).view(bool) if np.asarray(near).dtype.itemsize == 1 else np.asarray(near, dtype=bool)
        if cur is _ALL:
            idx = np.flatnonzero(near)
            self["selected"] = near                      # the verdicts ARE the new mask
            return idx
        idx = cur[near]
        self._set_idx_selected(idx)
        return idx

    def select_in_range(self, X: np.ndarray, max_range: float, _ctx=None, _slot=None) -> None:
        """Keeps selected points whose nearest neighbour in X is closer than max_range
        (strict, like cKDTree's distance_upper_bound)."""
        if np.shape(X)[1] != 3:
            raise PointCloudException("X must have 3 columns!")
        ctx = _ctx or backend.get_context()
        if _slot is None:
            ctx.upload(_lib.MOV, np.asarray(X, dtype=np.float64))
        cur = self.idx_selected
        if len(cur) == 0:
            return
        self._upload(ctx, _lib.FIX)
        near = ctx.select_in_range(_lib.FIX, _lib.MOV, None if len(cur) == self._num_points else cur,
                                   max_range=float(max_range))
        self._set_idx_selected(cur[near])

    def select_voxels(self, voxel_size: float, origin=(0.0, 0.0, 0.0), _ctx=None) -> None:
        """Keeps, among the selected points, the lowest-index point of every voxel of the lattice with cell ``voxel_size`` and
        ``origin`` (voxel of a point: ``np.floor((X - origin) / voxel_size)``; contract (V)) and deselects the
        rest.  Not in the reference; composes with select_in_range and select_n_points the way those compose with each other."""
        c, o = voxel_arguments(voxel_size, origin, PointCloudException)
        ctx = _ctx or backend.get_context()
        cur = self.idx_selected
        if len(cur) == 0:
            return
        self._upload(ctx, _lib.FIX)
        keep = ctx.voxel_select(_lib.FIX, c, o, None if len(cur) == self._num_points else cur)
        self._set_idx_selected(cur[keep])

    def select_statistical_inliers(self, neighbors: int = 20, std_ratio: float = 2.0, _ctx=None) -> None:
        """Keeps, among the selected points, those whose mean distance to their ``neighbors`` nearest points of the cloud (ALL its
        points, the point itself included) is at most mean + ``std_ratio`` * std over the selected points, and deselects the rest
        (contract (O)).  The statistics of the call (n_candidates, n_kept, mean, std, threshold) are left in
        ``last_outlier_stats``.  Not in the reference; composes with select_in_range, select_voxels and select_n_points."""
        if isinstance(neighbors, (bool, float, str, bytes)) or int(neighbors) != neighbors or not 2 <= neighbors <= _lib.OUTLIER_MAX_K:
            raise PointCloudException(f"neighbors must be an integer >= 2 and <= {_lib.OUTLIER_MAX_K}.")
        try:
            ratio = float(std_ratio)
            ok = not isinstance(std_ratio, (bool, str, bytes)) and np.isfinite(ratio)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise PointCloudException("std_ratio must be a finite number.")
        ctx = _ctx or backend.get_context()
        cur = self.idx_selected
        if len(cur) == 0:
            return
        self._upload(ctx, _lib.FIX)
        keep, _, st = ctx.outlier_statistical(_lib.FIX, int(neighbors), ratio, rows=None if len(cur) == self._num_points else cur)
        self.last_outlier_stats = _lib._stats_dict(st)
        self._set_idx_selected(cur[keep])

    def select_keypoints(self, neighbors: int = 32, salient_radius=None, nms_neighbors=None, nms_radius=None, gamma21: float = 0.975,
                         gamma32: float = 0.975, min_neighbors: int = 5, _ctx=None) -> None:
        """Keeps, among the selected points, the ISS keypoints of the WHOLE cloud and deselects the rest (contract (I), DESIGN.md
        section 22; the keywords are ``keypoint_keep``'s): support and suppression are always among ALL points of the cloud, so a
        selected point may lose to one that is not selected.  The record of the call is left in ``last_keypoint_stats``.  Not in
        the reference; composes with select_in_range, select_voxels and select_n_points."""
        from .features import _check_keypoint_counts, keypoint_arguments
        try:
            a = keypoint_arguments(neighbors, salient_radius, nms_neighbors, nms_radius, gamma21, gamma32, min_neighbors)
        except (TypeError, ValueError) as e:
            raise PointCloudException(str(e)) from None
        cur = self.idx_selected
        if len(cur) == 0:
            return
        try:
            _check_keypoint_counts(self._num_points, a)
        except ValueError as e:
            raise PointCloudException(str(e)) from None
        ctx = _ctx or backend.get_context()
        self._upload(ctx, _lib.FIX)
        keep, _, _, st = ctx.keypoints(_lib.FIX, *a)
        self.last_keypoint_stats = _lib._stats_dict(st)
        self._set_idx_selected(cur[np.asarray(keep)[cur]])

    def select_radius_inliers(self, radius: float, min_points: int, _ctx=None) -> None:
        """Keeps, among the selected points, those with more than ``min_points`` points of the cloud (ALL its points, the point
        itself included) strictly closer than ``radius``, and deselects the rest (contract (O))."""
        try:
            r = float(radius)
            ok = not isinstance(radius, (bool, str, bytes)) and np.isfinite(r) and r > 0.0
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise PointCloudException("radius must be a finite number > 0.")
        if isinstance(min_points, (bool, float, str, bytes)) or int(min_points) != min_points or min_points < 0:
            raise PointCloudException("min_points must be an integer >= 0.")
        ctx = _ctx or backend.get_context()
        cur = self.idx_selected
        if len(cur) == 0:
            return
        self._upload(ctx, _lib.FIX)
        keep, _, _ = ctx.outlier_radius(_lib.FIX, r, int(min_points), rows=None if len(cur) == self._num_points else cur)
        self._set_idx_selected(cur[keep])

    def _cluster_selected(self, radius, min_points, ctx):
        """(selected indices, their DBSCAN labels as a cloud of their own) -- (indices, None) when nothing is selected; the record
        is left in ``last_cluster_stats``."""
        from .features import cluster_arguments
        try:
            r, mp = cluster_arguments(radius, min_points)
        except ValueError as e:
            raise PointCloudException(str(e)) from None
        cur = self.idx_selected
        if len(cur) == 0:
            return cur, None
        ctx = ctx or backend.get_context()
        self._upload(ctx, _lib.FIX, rows=None if len(cur) == self._num_points else cur)
        labels, _, st = ctx.cluster(_lib.FIX, r, mp)
        self.last_cluster_stats = _lib._stats_dict(st)
        return cur, np.asarray(labels)

    def select_largest_cluster(self, radius: float, min_points: int = 10, _ctx=None) -> None:
        """Keeps, among the selected points, the largest DBSCAN cluster of the SELECTED points taken as a cloud of their own --
        the selected rows are uploaded, the points that are not selected play no part -- and deselects the rest (contract (U),
        DESIGN.md section 23; ``radius`` and ``min_points`` are ``cluster_labels``'s).  Of equally large clusters the one with the
        lowest label stays; without any cluster nothing stays selected.  The record of the call is left in ``last_cluster_stats``.
        Not in the reference; composes with select_in_range, select_voxels and select_n_points."""
        cur, labels = self._cluster_selected(radius, min_points, _ctx)
        if labels is None:
            return
        self._set_idx_selected(cur[labels == self.last_cluster_stats["largest_label"]] if self.last_cluster_stats["n_clusters"] else cur[:0])

    def select_clusters(self, radius: float, min_points: int = 10, min_size: int = 1, _ctx=None) -> None:
        """Keeps, among the selected points, those in a DBSCAN cluster (of the SELECTED points taken as a cloud of their own) with
        at least ``min_size`` members, core and border, and deselects the rest -- noise always goes (contract (U), DESIGN.md section
        23).  The record of the call is left in ``last_cluster_stats``.  Not in the reference; composes with select_in_range,
        select_voxels and select_n_points."""
        if isinstance(min_size, (bool, float, str, bytes)) or not isinstance(min_size, (int, np.integer)) or min_size < 1:
            raise PointCloudException("min_size must be an integer >= 1.")
        cur, labels = self._cluster_selected(radius, min_points, _ctx)
        if labels is None:
            return
        sizes = np.bincount(labels[labels >= 0], minlength=1)
        self._set_idx_selected(cur[(labels >= 0) & (sizes[np.maximum(labels, 0)] >= int(min_size))])

    def _regions_selected(self, kw):
        """(selected indices, their smooth-region labels as a cloud of their own) -- (indices, None) when nothing is selected;
        the record is left in ``last_region_stats``."""
        from . import features
        unknown = set(kw) - {"max_angle", "neighbors", "min_size", "cos_min", "radius", "min_planarity", "oriented", "normal_neighbors"}
        if unknown:
            raise PointCloudException(f"select_regions takes no keyword {sorted(unknown)[0]!r}")
        cur = self.idx_selected
        own = all(c in self for c in ("nx", "ny", "nz"))
        try:
            features.regions_arguments(**kw)
            if len(cur) == 0:
                return cur, None
            X = np.ascontiguousarray(np.stack([self[c].to_numpy()[cur] for c in ("x", "y", "z")], axis=1), dtype=np.float64)
            N = None
            if own and kw.get("min_planarity") is None:
                N = np.stack([np.asarray(self[c].to_numpy()[cur], dtype=np.float32) for c in ("nx", "ny", "nz")], axis=1)
            labels, info = features.smooth_regions(X, N, return_info=True, **kw)
        except ValueError as e:
            raise PointCloudException(str(e)) from None
        self.last_region_stats = info
        return cur, np.asarray(labels)

    def select_regions(self, max_angle: float = 5.0, neighbors: int = 16, min_size: int = 1, **kw) -> None:
        """Keeps, among the selected points, those in a smooth region (of the SELECTED points taken as a cloud of their own) with
        at least ``min_size`` members, and deselects the rest -- what no region takes always goes (contract (J), DESIGN.md section
        27; the arguments and the keywords ``cos_min``, ``radius``, ``min_planarity``, ``oriented``, ``normal_neighbors`` are
        ``smooth_regions``'s).  The cloud's nx / ny / nz columns are the normals where it has them, else the library estimates them.
        The record of the call is left in ``last_region_stats``.  Not in the reference; composes with select_in_range,
        select_voxels and select_n_points."""
        cur, labels = self._regions_selected(dict(kw, max_angle=max_angle, neighbors=neighbors, min_size=min_size))
        if labels is not None:
            self._set_idx_selected(cur[labels >= 0])

    def select_largest_region(self, max_angle: float = 5.0, neighbors: int = 16, min_size: int = 1, **kw) -> None:
        """Keeps, among the selected points, the largest smooth region of the SELECTED points taken as a cloud of their own and
        deselects the rest (``select_regions``'s arguments).  Of equally large regions the one with the lowest label stays;
        without any region nothing stays selected.  The record of the call is left in ``last_region_stats``."""
        cur, labels = self._regions_selected(dict(kw, max_angle=max_angle, neighbors=neighbors, min_size=min_size))
        if labels is not None:
            self._set_idx_selected(cur[labels == self.last_region_stats["largest_label"]] if self.last_region_stats["n_regions"] else cur[:0])

    def denoise(self, neighbors: int = 16, **kw) -> None:
        """Rewrites the x / y / z of the selected points, smoothed by moving least squares as a cloud of their own -- each
        projected onto the plane fitted to its ``neighbors`` nearest selected points; the points that are not selected play no
        part and stay as they are (contract (W); the keywords ``radius``, ``bandwidth``, ``strength``,
        ``min_neighbors``, ``rounds`` are ``denoise_points``'s).  The nx / ny / nz / planarity columns, if present, are left
        alone: they describe the coordinates as they were, estimate them again where they matter.  The record of the call is
        left in ``last_denoise_stats``.  Not in the reference; composes with select_in_range, select_voxels and
        select_n_points."""
        from . import features
        unknown = set(kw) - {"radius", "bandwidth", "strength", "min_neighbors", "rounds"}
        if unknown:
            raise PointCloudException(f"denoise takes no keyword {sorted(unknown)[0]!r}")
        cur = self.idx_selected
        try:
            a = features.denoise_arguments(neighbors=neighbors, **kw)
            if len(cur) == 0:
                self.last_denoise_stats = dict(features._NO_DENOISE, rounds=a[5])
                return
            X = np.ascontiguousarray(np.stack([self[c].to_numpy()[cur] for c in _XYZ], axis=1), dtype=np.float64)
            P, info = features.denoise_points(X, neighbors=neighbors, return_info=True, **kw)
        except ValueError as e:
            raise PointCloudException(str(e)) from None
        self.last_denoise_stats = info
        for axis, name in enumerate(_XYZ):
            col = np.array(self[name].to_numpy(), dtype=np.float64)   # (a copy: the frame's own column is not written in place)
            col[cur] = P[:, axis]
            self._adopt_column(name, col)

    def select_plane(self, max_distance: float, invert: bool = False, _ctx=None, **kw) -> None:
        """Keeps, among the selected points, the inliers of the dominant plane of the SELECTED points -- the selection goes in as
        ``segment_plane``'s mask over the whole cloud, so the points that are not selected neither count nor define a plane --
        and deselects the rest (contracts (P) and (Q); ``max_distance`` and the keywords ``hypotheses``,
        ``seed``, ``triples``, ``refine`` are ``segment_plane``'s).  ``invert=True``: keeps the complement instead, the selected
        points off the plane -- the call before ``select_largest_cluster`` on a scene with a ground.  The ``PlaneResult`` of the
        call is left in ``last_plane``.  Not in the reference; composes with select_in_range, select_voxels and select_n_points."""
        from . import features
        if not isinstance(invert, (bool, np.bool_)):
            raise PointCloudException(f"invert must be True or False, not {invert!r}")
        unknown = set(kw) - {"hypotheses", "seed", "triples", "refine"}
        if unknown:
            raise PointCloudException(f"select_plane takes no keyword {sorted(unknown)[0]!r}")
        try:
            d, h, s, tri, r = features.plane_arguments(max_distance, **kw)
        except (TypeError, ValueError) as e:
            raise PointCloudException(str(e)) from None
        selected = np.ascontiguousarray(self["selected"].to_numpy(), dtype=bool)
        if not selected.any():
            return
        try:
            on_device, rows, mask, n, _ = features._plane_rows(self, selected)
            res = features._segment_plane(features._plane_context("select_plane", _ctx), on_device, rows, mask, n, d, h, s, tri, r, True)
        except ValueError as e:
            raise PointCloudException(str(e)) from None
        if res is None:
            raise PointCloudException("no hypothesis is valid: the selected points give no plane")
        self.last_plane = res
        self._set_idx_selected(np.flatnonzero(selected & ~res.inliers if invert else res.inliers))

    def select_farthest(self, count: int, start=None, _ctx=None) -> None:
        """Keeps ``count`` of the selected points, evenly spread in space, and deselects the rest: farthest point sampling
        (contract (S)) with the selection as ``farthest_points``' mask over the whole cloud.  ``start`` is a
        row of the cloud, the first pick (None: the lowest selected row); a start that is not selected is refused.  Fewer than
        ``count`` stay where the selected points hold fewer distinct positions.  The picks in pick order, their squared distances
        and the record of the call are left in ``last_farthest``.  Not in the reference; what ``select_n_points`` is in the order
        of the file, this is in space; composes with select_in_range, select_voxels and select_plane."""
        from . import features
        try:
            c, s = features.farthest_arguments(count, start)
        except (TypeError, ValueError) as e:
            raise PointCloudException(str(e)) from None
        selected = np.ascontiguousarray(self["selected"].to_numpy(), dtype=bool)
        if s >= self._num_points or (s >= 0 and not selected[s]):
            raise PointCloudException(f"start must be a selected point of the cloud, not {start!r}")
        if not selected.any():
            return
        on_device, rows, mask, n = features._rows_and_mask(self, selected)
        idx, d2, st = features._farthest(features._farthest_context("select_farthest", _ctx), on_device, rows, mask, n, c, s, True)
        self.last_farthest = (idx, d2, st)
        self._set_idx_selected(idx)

    def fpfh(self, neighbors: int = 32, radius=None) -> np.ndarray:
        """The (n, 33) float32 FPFH descriptors of ALL points (contract (F)): ``fpfh_features(self,
        neighbors=neighbors, radius=radius)`` -- the cloud's own nx / ny / nz columns where it has them (a point without a normal
        has no pairs of its own: its row holds its neighbours' share alone), the library's normals otherwise.  Not in the reference."""
        from .features import fpfh_features
        return fpfh_features(self, neighbors=neighbors, radius=radius)

    def orient_normals(self, neighbors: int = 16, viewpoint=None, away_from=None) -> None:
        """Rewrites the nx / ny / nz columns with consistent signs (contract (H)): ``orient_normals(self,
        neighbors=..., viewpoint=..., away_from=...)`` over ALL points with the cloud's own normals -- a point without one stands
        alone and stays as it is.  Raises where the cloud has no normals.  The record of the call is left in
        ``last_orient_stats``.  Not in the reference."""
        from . import features
        if not all(c in self for c in ("nx", "ny", "nz")):
            raise PointCloudException("orient_normals needs the normals of the cloud: call estimate_normals first")
        try:
            out, info = features.orient_normals(self, neighbors=neighbors, viewpoint=viewpoint, away_from=away_from, return_info=True)
        except ValueError as e:
            raise PointCloudException(str(e)) from None
        for j, c in enumerate(("nx", "ny", "nz")):
            self[c] = out[:, j].astype(self[c].to_numpy().dtype, copy=False)
        self.last_orient_stats = info

    # ---- attributes (pointcloud.py:173-203) ---------------------------------------------
    def estimate_normals(self, neighbors: int, _ctx=None, _uploaded=False, _sel=None) -> None:
        """Normal vector + planarity of every SELECTED point from its `neighbors` nearest
        points among ALL points (itself included)."""
        ctx = _ctx or backend.get_context()
        if not _uploaded:
            self._upload(ctx, _lib.FIX)
        sel = self.idx_selected if _sel is None else _sel
        vals = {c: np.empty(0, dtype=np.float32) for c in _ATTRS}
        if len(sel):
            nv, pl = ctx.estimate_normals(_lib.FIX, sel, int(neighbors))
            vals = {"nx": nv[:, 0], "ny": nv[:, 1], "nz": nv[:, 2], "planarity": pl}
        for c, v in vals.items():
            self[c] = self._sparse_column(sel, v)

    def _sparse_column(self, idx, values):
        """float32 sparse column, NaN everywhere but ``values`` at the (sorted) rows ``idx`` -- what
        ``SparseArray(dense)`` gives (NaN results are not stored either), without touching n elements."""
        values = np.ascontiguousarray(values, dtype=np.float32)
        if _IntIndex is not None and self._num_points < 2**31:
            ok = ~np.isnan(values)
            return pd.arrays.SparseArray(values[ok], sparse_index=_IntIndex(self._num_points, idx[ok].astype(np.int32)),
                                         fill_value=np.nan, dtype=pd.SparseDtype(np.float32, np.nan))
        dense = np.full(self._num_points, np.nan, dtype=np.float32)
        dense[idx] = values
        return pd.arrays.SparseArray(dense)

    # ---- geometry (pointcloud.py:205-217) -----------------------------------------------
    def transform_by_H(self, H: np.ndarray, _ctx=None, _slot=None) -> None:
        """x,y,z <- (H @ [x y z 1]^T)[:3]  in place."""
        self._transform(H, _ctx, _slot)

    def _transform(self, H, ctx=None, slot=None) -> np.ndarray:
        """transform_by_H; hands back the (n,3) array of new coordinates it downloaded (= self.X)."""
        ctx = ctx or backend.get_context()
        if slot is None:
            slot = _lib.MOV
            self._upload(ctx, slot)
        ctx.transform(slot, np.asarray(H, dtype=np.float64))
        # run() returns the (n, 3) rows, the frame wants three contiguous columns: both come out of ONE pass over the link
        # (sicp_cloud_download_both: the device's columns through a pinned double buffer, fanned out -- and transposed -- by
        # host threads) and the columns are handed to the frame WITHOUT pandas' defensive copy of freshly made arrays
        # nobody else holds
        Xt, cols = ctx.download_both(slot)
        for name, col in zip(_XYZ, cols):
            self._adopt_column(name, col)
        return Xt

    def _adopt_column(self, name, values):
        """``self[name] = values`` for an array this object just created: same result, no copy.
        The copy-free road is pandas-internal (`DataFrame._set_item_mgr`, what `__setitem__` calls after sanitising) and
        is taken only on the pandas line it was written and tested against (2.x: 2.0 ... 2.3, tests/test_host_mirror.py);
        every other pandas -- and every column that is not a plain float64 vector of the frame's length -- goes through
        the public `__setitem__` and pays the copy."""
        fast = (_PANDAS_MAJOR == 2 and hasattr(self, "_set_item_mgr") and name in self.columns
                and isinstance(values, np.ndarray) and values.dtype == np.float64 and values.ndim == 1
                and len(values) == len(self.index))
        if fast:
            try:
                self._set_item_mgr(name, values)
                return
            except (TypeError, AttributeError):           # another signature after all: the public road
                pass
        self[name] = values

    # ---- I/O (pointcloud.py:219-226) ------------------------------------------------------
    def write_xyz(self, file: Path):
        """CloudCompare-style text file: header `//X Y Z`, 3 decimals."""
        from . import io
        io.write_xyz(file, self.X, decimals=3, header="//X Y Z")     # same bytes as pandas' to_csv(float_format="%.3f")
