"""simpleicp_amd -- MI355X-native (gfx950) ICP inner loop behind simpleICP's Python API.

Drop-in for ``from simpleicp import SimpleICP, PointCloud, RigidBodyParameters``
(/root/reference/python/simpleicp/__init__.py:12-14); the hot path runs in hand-written HIP
kernels (simpleicp_amd/csrc) loaded through a C ABI (include/simpleicp_hip.h).

The reference's other modules keep their names for callers that drive the loop themselves:
``simpleicp_amd.corrpts.CorrPts``, ``simpleicp_amd.optimization.SimpleICPOptimization``,
``simpleicp_amd.mathutils``, ``simpleicp_amd.simpleicp`` (operator by operator on the same kernels).
"""
import logging as _logging

__version__ = "0.1.0"

_logging.getLogger(__name__).addHandler(_logging.NullHandler())

from .pointcloud import PointCloud, PointCloudException          # noqa: E402
from .rbp import Parameter, RigidBodyParameters                  # noqa: E402
from .icp import SimpleICP, SimpleICPException                   # noqa: E402
from .batch import BatchResult, run_batch                        # noqa: E402
from .tensors import outlier_keep, run_tensors, voxel_keep                     # noqa: E402  (imports torch on its first call only)

from .evaluation import Evaluation, evaluate_registration        # noqa: E402
from .features import (cluster_labels, denoise_points, farthest_points, fpfh_features, keypoint_keep, orient_normals, segment_plane,   # noqa: E402
                       segment_planes, smooth_regions, PlaneResult)
from .registration import (consistent_matches, fit_pose, match_features, ransac_pose, refine_pose, register_global,   # noqa: E402
                           robust_pose, ConsistencyResult, GlobalResult)
from . import io                                                 # noqa: E402,F401

__all__ = ["SimpleICP", "SimpleICPException", "PointCloud", "PointCloudException",
           "RigidBodyParameters", "Parameter", "run_batch", "BatchResult", "run_tensors", "voxel_keep", "outlier_keep", "Evaluation",
           "evaluate_registration", "fpfh_features", "keypoint_keep", "match_features", "ransac_pose", "register_global", "GlobalResult", "fit_pose",
           "refine_pose", "robust_pose", "consistent_matches", "ConsistencyResult", "cluster_labels", "segment_plane",
           "segment_planes", "PlaneResult", "farthest_points", "orient_normals", "smooth_regions", "denoise_points"]
