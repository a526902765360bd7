"""Alias package: `import stillleben as sl` resolves to the MI355X-native implementation
(stillleben_amd), so that scripts written against the reference (e.g. its examples/ycb.py)
run unchanged.  The package is assembled the way the reference's python/stillleben/__init__.py:6-13 assembles it: the
sub-modules, then everything the main extension module `stillleben.lib.libstillleben_python` exports."""
import sys as _sys

import stillleben_amd as _impl
from stillleben_amd import camera_model, diff, extension, losses, profiling  # noqa: F401
from .lib.libstillleben_python import *  # noqa: F401,F403
from .lib.libstillleben_python import _set_install_prefix  # noqa: F401
from stillleben_amd import AssetTable, SceneBatch  # noqa: F401  (additive: the batch dimension of the GPU path)
from stillleben_amd import EnvironmentBank  # noqa: F401  (additive: the environment bank of a SceneBatch)
from stillleben_amd import ObjectStats  # noqa: F401  (additive: per-object visibility statistics)
from stillleben_amd import ObjectMasks  # noqa: F401  (additive: per-object masks as bit tiles and COCO run lengths)
from stillleben_amd import bop  # noqa: F401  (additive: BOP entries of a SceneBatch's views)
from stillleben_amd import pose_pnp, PosePnP  # noqa: F401  (additive: the pose of every set of 2D-3D correspondences)
from stillleben_amd import keypoint_vote, KeypointVotes  # noqa: F401  (additive: predicted vector fields to 2D keypoints)
from stillleben_amd import keypoint_vote3d, KeypointVotes3D  # noqa: F401  (additive: predicted 3D offsets to camera-frame keypoints)
from stillleben_amd import pose_fit, PoseFit  # noqa: F401  (additive: the pose of every set of 3D-3D correspondences)
from stillleben_amd import pose_align, PoseAlign  # noqa: F401  (additive: the robust pose of every set of 3D-3D correspondences)
from stillleben_amd import pose_icp, PoseICP  # noqa: F401  (additive: ICP refinement of a pose against the depth's camera points)
from stillleben_amd import render_flow, RenderFlow  # noqa: F401  (additive: optical flow, scene flow and occlusion between two renders)
from stillleben_amd import point_knn, PointNeighbours, PointPyramid  # noqa: F401  (additive: k nearest neighbours between point sets)

__all__ = _impl.__all__
for _name in ("camera_model", "diff", "extension", "losses", "profiling"):
    _sys.modules[__name__ + "." + _name] = getattr(_impl, _name)
