"""stillleben_amd -- MI355X-native (gfx950, HIP) implementation of stillleben's hot path:
tabletop settling (replaces PhysX) + G-buffer rendering (replaces Magnum/OpenGL) + sl.diff,
behind the reference's Python surface (python/stillleben/__init__.py:15-42).

    import stillleben_amd as sl        # or `import stillleben as sl` via the alias package
"""
import os
import warnings

import torch  # noqa: F401  (device memory + streams)

from ._context import init, init_cuda, _set_install_prefix  # noqa: F401
from ._math import quat_to_matrix as _q2m, matrix_to_quat as _m2q
from .mesh import Mesh, Range3D  # noqa: F401
from .object import Object  # noqa: F401
from .scene import Scene  # noqa: F401
from .render_pass import RenderPass, RenderPassResult  # noqa: F401
from .extras import (Animator, ImageLoader, ImageSaver, LightMap, MeshCache, Texture, Texture2D,  # noqa: F401
                     Viewer, view, render_debug_image)
from .manipulation_sim import ManipulationSim  # noqa: F401
from .job_queue import JobQueue  # noqa: F401
from .scene_batch import AssetTable, SceneBatch  # noqa: F401  (additive: the batch dimension of the GPU path)
from .environment import EnvironmentBank  # noqa: F401  (additive: light maps / backgrounds / plane textures of a SceneBatch)
from .object_stats import ObjectStats  # noqa: F401  (additive: per-object visibility statistics, BOP's scene_gt_info)
from .object_masks import ObjectMasks  # noqa: F401  (additive: per-object masks, BOP's mask/, mask_visib/ and scene_gt_coco)
from . import camera_model, diff, losses, extension, profiling  # noqa: F401
from . import bop  # noqa: F401  (additive: BOP scene_camera / scene_gt entries from a SceneBatch's records)
from . import depth_sensor  # noqa: F401  (additive: the depth channel's sensor model, the sibling of camera_model)
from . import object_crops  # noqa: F401  (additive: per-object windows of a render for object-centric networks)
from .object_crops import ObjectCrops  # noqa: F401
from . import object_points  # noqa: F401  (additive: K pixels per visible object and the render's targets gathered there)
from .object_points import ObjectPoints  # noqa: F401
from . import object_keypoints  # noqa: F401  (additive: FPS keypoint banks, their projections and the per-pixel vector field)
from .object_keypoints import KeypointBank, ObjectKeypoints  # noqa: F401
from . import object_regions  # noqa: F401  (additive: surface-region banks, per-vertex and per-pixel region labels)
from .object_regions import RegionBank, ObjectRegions  # noqa: F401
from . import pose_error  # noqa: F401  (additive: ADD, ADD-S, MSSD, MSPD against a batch's ground truth, with class symmetries)
from .pose_error import ModelBank, PoseErrors  # noqa: F401
from . import pose_vsd  # noqa: F401  (additive: BOP's VSD against a batch's ground truth, by a depth raster in LDS)
from .pose_vsd import PoseVSD, SurfaceBank  # noqa: F401
from . import pose_pnp  # noqa: F401  (additive: the pose of every set of 2D-3D correspondences by P3P RANSAC and refinement)
from .pose_pnp import PosePnP  # noqa: F401
from . import keypoint_vote  # noqa: F401  (additive: predicted vector fields to 2D keypoints by RANSAC voting, PVNet's layer)
from .keypoint_vote import KeypointVotes  # noqa: F401
from . import keypoint_vote3d  # noqa: F401  (additive: predicted 3D offsets to camera-frame keypoints by mean shift, PVN3D's decoder)
from .keypoint_vote3d import KeypointVotes3D  # noqa: F401
from . import pose_fit  # noqa: F401  (additive: the pose of every set of 3D-3D correspondences, Horn's closed form)
from .pose_fit import PoseFit  # noqa: F401
from . import pose_align  # noqa: F401  (additive: the pose of every set of 3D-3D correspondences with the most inliers, RANSAC round Horn's fit)
from .pose_align import PoseAlign  # noqa: F401
from . import pose_icp  # noqa: F401  (additive: ICP refinement of a pose against the depth's camera points, on a model bank)
from .pose_icp import PoseICP  # noqa: F401
from . import render_flow  # noqa: F401  (additive: optical flow, scene flow and occlusion between two renders of a scene)
from .render_flow import RenderFlow  # noqa: F401
from . import point_knn  # noqa: F401  (additive: the k nearest neighbours between point sets and the RandLA pyramid)
from .point_knn import PointNeighbours, PointPyramid  # noqa: F401

__all__ = [
    'init', 'init_cuda', 'render_debug_image', 'Animator', 'ImageLoader', 'ImageSaver', 'LightMap',
    'Mesh', 'MeshCache', 'Object', 'Range3D', 'RenderPass', 'RenderPassResult', 'Scene', 'Texture',
    'Texture2D', 'Viewer', 'view', 'ManipulationSim', 'JobQueue', 'AssetTable', 'SceneBatch',
    'camera_model', 'diff', 'extension', 'losses', 'quat_to_matrix', 'matrix_to_quat', 'ObjectStats', 'ObjectMasks', 'EnvironmentBank',
    'bop', 'depth_sensor', 'object_crops', 'ObjectCrops', 'object_points', 'ObjectPoints',
    'object_keypoints', 'KeypointBank', 'ObjectKeypoints', 'object_regions', 'RegionBank', 'ObjectRegions',
    'pose_error', 'ModelBank', 'PoseErrors',
    'pose_vsd', 'SurfaceBank', 'PoseVSD',
    'pose_pnp', 'PosePnP',
    'keypoint_vote', 'KeypointVotes',
    'keypoint_vote3d', 'KeypointVotes3D',
    'pose_fit', 'PoseFit',
    'pose_align', 'PoseAlign',
    'pose_icp', 'PoseICP',
    'render_flow', 'RenderFlow',
    'point_knn', 'PointNeighbours', 'PointPyramid',
]


def quat_to_matrix(q):
    """[x y z w] -> 3x3 rotation (reference python/src/py_magnum.cpp:83-97)."""
    if hasattr(q, "detach"):
        q = q.detach().cpu().numpy()
    return torch.from_numpy(_q2m(q))


def matrix_to_quat(m):
    if hasattr(m, "detach"):
        m = m.detach().cpu().numpy()
    return torch.from_numpy(_m2q(m))


STILLLEBEN_PATH = os.path.dirname(os.path.abspath(__file__))
