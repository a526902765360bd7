"""ctypes mirror of include/slhip.h and loader of the C-ABI library ``lib/libslhip.so``.

The product path has NO fallback: if the library is missing or no gfx950 device is present the
calls raise (see :func:`lib`).  The struct definitions are also used by the tests to drive the
CPU oracle (``oracle/libslref.so``) with the very same binary scene description.
"""
import ctypes as C
import os

import numpy as np

NUM_LIGHTS = 3
CHUNK_TRIS = 256

DRAW_HAS_BASE_TEX = 1
DRAW_VERTEX_COLORS = 2
DRAW_CASTS_SHADOW = 4
DRAW_ALPHA_TEST = 8
DRAW_NO_VERTEX_ID = 16
DRAW_HAS_NORMAL_TEX = 32
DRAW_HAS_MR_TEX = 64
DRAW_HAS_OCCLUSION_TEX = 128
DRAW_HAS_EMISSIVE_TEX = 256
DRAW_HAS_STICKER = 512
# SLHIP_SAMPLER_*: wrap S | wrap T << 2 (0 repeat, 1 clamp, 2 mirror) | mag linear 0x10 | min linear 0x20 | mip mode << 6
SAMPLER_DEFAULT = 0x10 | 0x20 | (2 << 6)

OUT_RGB = 0x01
OUT_COORD = 0x02
OUT_CLASS = 0x04
OUT_INSTANCE = 0x08
OUT_NORMALS = 0x10
OUT_VERTEX_IDX = 0x20
OUT_BARY = 0x40
OUT_CAM_COORD = 0x80
OUT_ALL = 0xFF
OUT_GT6 = 0x1F
RENDER_SSAO = 0x100
RENDER_SHADOWS = 0x200
RENDER_SHADOW_RESET = 0x400
RENDER_KEEP_HDR = 0x800
OBJECT_STATS_CAPACITY = 1     # SLHIP_OBJECT_STATS_CAPACITY: status of slhip_render_object_stats when the word pool is too small
OBJECT_MASKS_CAPACITY = 2     # SLHIP_OBJECT_MASKS_CAPACITY: status of slhip_render_object_masks when the word or the run pool is too small
OBJECT_CROPS_CAPACITY = 3     # SLHIP_OBJECT_CROPS_CAPACITY: status of slhip_object_crops_select when d_crops is too small
CROP_RGB, CROP_COORD, CROP_NORMALS, CROP_INSTANCE, CROP_MASK = 1, 2, 4, 8, 16      # SLHIP_CROP_*
OBJECT_CROPS_MAX_SIZE = 1024
OBJECT_POINTS_CAPACITY = 4    # SLHIP_OBJECT_POINTS_CAPACITY: status of slhip_object_points_select when d_sets is too small
POINTS_PIXEL, POINTS_CAMERA, POINTS_COORD, POINTS_NORMALS, POINTS_RGB = 1, 2, 4, 8, 16      # SLHIP_POINTS_*
OBJECT_POINTS_MAX = 16384
KEYPOINTS_MAX = 32            # SLHIP_KEYPOINTS_MAX
KEYPOINT_IN_FRONT, KEYPOINT_INSIDE, KEYPOINT_UNOCCLUDED = 1, 2, 4      # SLHIP_KEYPOINT_*: the flag bits of a projected keypoint
KEYPOINT_FIELD_OFFSET, KEYPOINT_FIELD_UNIT = 0, 1                      # SLHIP_KEYPOINT_FIELD_*
POSE_POINTS_MAX, POSE_SYMMETRIES_MAX = 4096, 1024                      # SLHIP_POSE_POINTS_MAX, SLHIP_POSE_SYMMETRIES_MAX
POSE_OUT_ADD, POSE_OUT_ADDS, POSE_OUT_MSSD, POSE_OUT_MSPD = 1, 2, 4, 8      # SLHIP_POSE_OUT_*
VSD_TAUS_MAX, VSD_WIDTH_MAX = 16, 4096                                    # SLHIP_VSD_TAUS_MAX, SLHIP_VSD_WIDTH_MAX
VSD_NORMALIZED, VSD_CLIPPED = 1, 1                                        # SLHIP_VSD_NORMALIZED (params.flags), SLHIP_VSD_CLIPPED (output flags)
VSD_OUT_VSD, VSD_OUT_COUNTS, VSD_OUT_COST, VSD_OUT_FLAGS = 1, 2, 4, 8     # SLHIP_VSD_OUT_*
PNP_POINTS_MAX, PNP_HYPOTHESES_MAX, PNP_REFINE_MAX = 4096, 4096, 16          # SLHIP_PNP_*_MAX
PNP_OUT_POSE, PNP_OUT_N_INLIERS, PNP_OUT_RMS, PNP_OUT_INLIERS, PNP_OUT_BEST, PNP_OUT_FLAGS = 1, 2, 4, 8, 16, 32      # SLHIP_PNP_OUT_*
PNP_INSUFFICIENT, PNP_NO_MODEL, PNP_REFINE_STOPPED, PNP_REFINE_REJECTED = 1, 2, 4, 8      # SLHIP_PNP_*: the flag bits of a set
VOTE_POINTS_MAX, VOTE_HYPOTHESES_MAX = 4096, 1024                            # SLHIP_VOTE_*_MAX
VOTE_OUT_UV, VOTE_OUT_N_INLIERS, VOTE_OUT_BEST, VOTE_OUT_FLAGS, VOTE_OUT_MEAN, VOTE_OUT_COV, VOTE_OUT_INLIERS = 1, 2, 4, 8, 16, 32, 64      # SLHIP_VOTE_OUT_*
VOTE_INSUFFICIENT, VOTE_NO_MODEL, VOTE_REFINE_STOPPED, VOTE_REFINE_REJECTED = 1, 2, 4, 8      # SLHIP_VOTE_*: the flag bits of a (set, keypoint)
VOTE3D_POINTS_MAX, VOTE3D_SEEDS_MAX, VOTE3D_ITERS_MAX = 4096, 1024, 64           # SLHIP_VOTE3D_*_MAX
(VOTE3D_OUT_XYZ, VOTE3D_OUT_N_SUPPORT, VOTE3D_OUT_BEST, VOTE3D_OUT_ITERS, VOTE3D_OUT_FLAGS, VOTE3D_OUT_MEAN, VOTE3D_OUT_COV,
 VOTE3D_OUT_SUPPORT) = 1, 2, 4, 8, 16, 32, 64, 128                               # SLHIP_VOTE3D_OUT_*
VOTE3D_INSUFFICIENT, VOTE3D_NO_MODEL, VOTE3D_NOT_CONVERGED = 1, 2, 4             # SLHIP_VOTE3D_*: the flag bits of a (set, keypoint)
FIT_POINTS_MAX = 4096                                                            # SLHIP_FIT_POINTS_MAX
FIT_OUT_POSE, FIT_OUT_N_USED, FIT_OUT_RMS, FIT_OUT_FLAGS = 1, 2, 4, 8            # SLHIP_FIT_OUT_*
FIT_INSUFFICIENT, FIT_DEGENERATE = 1, 2                                          # SLHIP_FIT_*: the flag bits of a set
ALIGN_POINTS_MAX, ALIGN_HYPOTHESES_MAX, ALIGN_REFINE_MAX = 4096, 4096, 16       # SLHIP_ALIGN_*_MAX
ALIGN_OUT_POSE, ALIGN_OUT_N_INLIERS, ALIGN_OUT_RMS, ALIGN_OUT_INLIERS, ALIGN_OUT_BEST, ALIGN_OUT_FLAGS = 1, 2, 4, 8, 16, 32      # SLHIP_ALIGN_OUT_*
ALIGN_INSUFFICIENT, ALIGN_NO_MODEL, ALIGN_REFINE_STOPPED, ALIGN_REFINE_REJECTED = 1, 2, 4, 8      # SLHIP_ALIGN_*: the flag bits of a set
ICP_POINTS_MAX, ICP_ITERS_MAX = 4096, 64                                         # SLHIP_ICP_POINTS_MAX, SLHIP_ICP_ITERS_MAX
ICP_OUT_POSE, ICP_OUT_N_PAIRS, ICP_OUT_RMS, ICP_OUT_ITERS, ICP_OUT_FLAGS, ICP_OUT_NEAREST = 1, 2, 4, 8, 16, 32      # SLHIP_ICP_OUT_*
ICP_BAD_CLASS, ICP_NO_INIT, ICP_INSUFFICIENT, ICP_DEGENERATE, ICP_CONVERGED = 1, 2, 4, 8, 16      # SLHIP_ICP_*: the flag bits of a set
ICP_FAILED = 15                                                                  # SLHIP_ICP_FAILED: the failure bits
REGIONS_MAX, REGION_NONE = 255, 255                                   # SLHIP_REGIONS_MAX, SLHIP_REGION_NONE
REGIONS_OUT_LOCAL, REGIONS_OUT_HISTOGRAM = 1, 2                        # SLHIP_REGIONS_OUT_*
FLOW_SLOTS_MAX = 256                                                   # SLHIP_FLOW_SLOTS_MAX
FLOW_VALID, FLOW_INSIDE, FLOW_VISIBLE = 1, 2, 4                        # SLHIP_FLOW_*: the flag bits of a pixel of the render flow
FLOW_OUT_FLOW, FLOW_OUT_SCENE, FLOW_OUT_FLAGS, FLOW_OUT_COUNTS = 1, 2, 4, 8      # SLHIP_FLOW_OUT_*
FLOW_MATCH_INSTANCE = 1                                                # SLHIP_FLOW_MATCH_INSTANCE (params.flags)
KNN_K_MAX, KNN_BLOCK, KNN_TILE = 32, 256, 1024                         # SLHIP_KNN_K_MAX, SLHIP_KNN_BLOCK, SLHIP_KNN_TILE
KNN_OUT_IDX, KNN_OUT_DIST2, KNN_OUT_COUNT = 1, 2, 4                    # SLHIP_KNN_OUT_*
ABI_VERSION = 5
DEFAULT_HULL_PAIRS, DEFAULT_CONTACTS = 2048, 1024   # SLHIP_DEFAULT_HULL_PAIRS / SLHIP_DEFAULT_CONTACTS of include/slhip.h
COMM_ID_BYTES = 128


class MeshPool(C.Structure):
    _fields_ = [
        ("d_pos", C.c_void_p),
        ("d_nrm", C.c_void_p),
        ("d_uv", C.c_void_p),
        ("d_col", C.c_void_p),
        ("d_tan", C.c_void_p),
        ("d_idx", C.c_void_p),
        ("d_tex", C.c_void_p),
        ("n_vertices", C.c_uint64),
        ("n_indices", C.c_uint64),
        ("n_tex_bytes", C.c_uint64),
        ("d_light_maps", C.c_void_p),
        ("n_light_maps", C.c_uint64),
    ]


class LightMapRec(C.Structure):
    """slhip_light_map: device pointers + sizes of one image-based-lighting texture set."""

    _fields_ = [
        ("d_env", C.c_void_p),
        ("d_irradiance", C.c_void_p),
        ("d_prefilter", C.c_void_p),
        ("d_brdf_lut", C.c_void_p),
        ("env_size", C.c_uint32),
        ("env_levels", C.c_uint32),
        ("irr_size", C.c_uint32),
        ("pre_size", C.c_uint32),
        ("pre_levels", C.c_uint32),
        ("lut_size", C.c_uint32),
    ]


# numpy dtypes with the exact layout of slhip_draw / slhip_scene / slhip_chunk
DRAW_DTYPE = np.dtype(
    [
        ("mesh_to_object", np.float32, (16,)),
        ("object_to_world", np.float32, (16,)),
        ("normal_to_world", np.float32, (12,)),
        ("base_color", np.float32, (4,)),
        ("emissive", np.float32, (4,)),
        ("alpha_cutoff", np.float32),
        ("metallic", np.float32),
        ("roughness", np.float32),
        ("scene", np.uint32),
        ("class_index", np.uint32),
        ("instance_index", np.uint32),
        ("flags", np.uint32),
        ("n_verts", np.uint32),
        ("vtx_base", np.uint32),
        ("idx_base", np.uint32),
        ("n_tris", np.uint32),
        ("prim_base", np.uint32),
        ("tex_offset", np.uint32),
        ("tex_w", np.uint32),
        ("tex_h", np.uint32),
        ("clip_base", np.uint32),
        ("normal_tex", np.uint32, (3,)),      # offset, w, h
        ("mr_tex", np.uint32, (3,)),
        ("occlusion_tex", np.uint32, (3,)),
        ("emissive_tex", np.uint32, (3,)),
        ("sticker_tex", np.uint32, (3,)),
        ("tex_sampler", np.uint8, (8,)),     # base, normal, metallic-roughness, occlusion, emissive
        ("_pad", np.uint32, (3,)),
        ("sticker_projection", np.float32, (16,)),
        ("sticker_range", np.float32, (4,)),
    ],
    align=False,
)
assert DRAW_DTYPE.itemsize == 432, DRAW_DTYPE.itemsize

SCENE_DTYPE = np.dtype(
    [
        ("proj", np.float32, (16,)),
        ("world_to_cam", np.float32, (16,)),
        ("cam_position", np.float32, (4,)),
        ("light_dir", np.float32, (NUM_LIGHTS, 4)),
        ("light_color", np.float32, (NUM_LIGHTS, 4)),
        ("shadow_mat", np.float32, (NUM_LIGHTS, 16)),
        ("ambient", np.float32, (4,)),
        ("manual_exposure", np.float32),
        ("draw_begin", np.uint32),
        ("draw_end", np.uint32),
        ("n_prims", np.uint32),
        ("light_map", np.uint32),     # 1 + index into the pool's light maps, 0 = none
        ("bg_tex", np.uint32, (3,)),  # background image: offset, w, h (w = 0: none)
    ],
    align=False,
)
assert SCENE_DTYPE.itemsize == 480, SCENE_DTYPE.itemsize

CHUNK_DTYPE = np.dtype(
    [("scene", np.uint32), ("draw", np.uint32), ("first_tri", np.uint32), ("count", np.uint32)]
)

# slhip_object_stats (include/slhip.h): per (scene, slot) visibility statistics, 40 bytes
OBJECT_STATS_DTYPE = np.dtype([("px_visib", np.uint32), ("px_all", np.uint32), ("bbox_visib", np.int32, (4,)),
                               ("bbox_obj", np.int32, (4,))])
assert OBJECT_STATS_DTYPE.itemsize == 40, OBJECT_STATS_DTYPE.itemsize

# slhip_object_mask (include/slhip.h): per (scene, slot) layout of the bit tiles and run lengths of both mask kinds, 56 bytes
OBJECT_MASK_DTYPE = np.dtype([("tile_box", np.int32, (4,)), ("word_offset", np.uint64, (2,)), ("rle_offset", np.uint64, (2,)),
                              ("rle_count", np.uint32, (2,))])
assert OBJECT_MASK_DTYPE.itemsize == 56, OBJECT_MASK_DTYPE.itemsize

# slhip_host_object / slhip_host_scene (include/slhip.h): flat descriptors for the C++ record assembly
HOST_OBJECT_DTYPE = np.dtype([
    ("pose", np.float32, (16,)), ("bbox_center", np.float32, (4,)), ("color", np.float32, (4,)), ("force_color", np.uint32),
    ("tmpl_begin", np.uint32), ("tmpl_count", np.uint32), ("instance_index", np.uint32), ("metallic", np.float32),
    ("roughness", np.float32), ("casts_shadows", np.uint32), ("_pad", np.uint32)])
assert HOST_OBJECT_DTYPE.itemsize == 128
HOST_SCENE_DTYPE = np.dtype([
    ("proj", np.float32, (16,)), ("proj_inv", np.float32, (16,)), ("camera_pose", np.float32, (16,)),
    ("light_dir", np.float32, (NUM_LIGHTS, 4)), ("light_color", np.float32, (NUM_LIGHTS, 4)), ("ambient", np.float32, (4,)),
    ("plane_pose", np.float32, (16,)), ("plane_size", np.float32, (2,)), ("plane_template", np.int32),
    ("manual_exposure", np.float32), ("obj_begin", np.uint32), ("obj_end", np.uint32), ("light_map", np.uint32),
    ("bg_tex", np.uint32, (3,))])
assert HOST_SCENE_DTYPE.itemsize == 408


class RenderOut(C.Structure):
    _fields_ = [
        ("d_rgb", C.c_void_p),
        ("d_coord", C.c_void_p),
        ("d_class", C.c_void_p),
        ("d_instance", C.c_void_p),
        ("d_normals", C.c_void_p),
        ("d_vertex_idx", C.c_void_p),
        ("d_bary", C.c_void_p),
        ("d_cam_coord", C.c_void_p),
    ]


class RenderScratch(C.Structure):
    _fields_ = [
        ("d_vis", C.c_void_p),
        ("d_hdr", C.c_void_p),
        ("d_ao", C.c_void_p),
        ("d_shadow", C.c_void_p),
        ("d_queue", C.c_void_p),
        ("d_lum", C.c_void_p),
        ("d_clip", C.c_void_p),
        ("d_shadow_tiles", C.c_void_p),
        ("queue_capacity", C.c_uint32),
        ("shadow_res", C.c_uint32),
        ("n_clip_verts", C.c_uint32),
        ("shadow_lights", C.c_uint32),
        ("d_vattr", C.c_void_p),
    ]


_LIB = None
# slhip_camera_params (include/slhip.h), 268 bytes
CAMERA_DTYPE = np.dtype([
    ("translation", np.float32, (6,)), ("scaling", np.float32, (3,)),
    ("blur_kernel", np.float32, (25,)), ("post_kernel", np.float32, (25,)),
    ("exposure_gain", np.float32), ("noise_a", np.float32), ("noise_b", np.float32), ("hue_shift", np.float32),
    ("blur_enabled", np.uint32), ("noise_enabled", np.uint32), ("seed_lo", np.uint32), ("seed_hi", np.uint32),
])
assert CAMERA_DTYPE.itemsize == 268
# slhip_depth_sensor_params (include/slhip.h), 60 bytes
DEPTH_SENSOR_DTYPE = np.dtype([
    ("fb", np.float32), ("z_min", np.float32), ("z_max", np.float32), ("shadow_margin", np.float32), ("cos_min", np.float32),
    ("window_radius", np.uint32), ("window_tol", np.float32), ("min_support", np.uint32), ("sigma_lateral", np.float32),
    ("sigma_disparity", np.float32), ("subpixel", np.uint32), ("dropout_p", np.float32), ("depth_scale", np.float32),
    ("seed_lo", np.uint32), ("seed_hi", np.uint32),
])
assert DEPTH_SENSOR_DTYPE.itemsize == 60

# slhip_object_crop_params (include/slhip.h), 64 bytes
OBJECT_CROP_PARAMS_DTYPE = np.dtype([
    ("size", np.uint32), ("box", np.uint32), ("pad", np.float32), ("jitter_scale", np.float32), ("jitter_shift", np.float32),
    ("min_px", np.uint32), ("min_visib_fract", np.float32), ("fx", np.float32), ("fy", np.float32), ("cx", np.float32),
    ("cy", np.float32), ("seed_lo", np.uint32), ("seed_hi", np.uint32), ("scene_id_base", np.uint32), ("outputs", np.uint32),
    ("isolate", np.uint32),
])
assert OBJECT_CROP_PARAMS_DTYPE.itemsize == 64
# slhip_object_crop (include/slhip.h), 48 bytes: one window
OBJECT_CROP_DTYPE = np.dtype([("scene", np.uint32), ("slot", np.uint32), ("x0", np.float32), ("y0", np.float32),
                              ("side", np.float32), ("step", np.float32), ("K", np.float32, (4,)), ("_pad", np.uint32, (2,))])
assert OBJECT_CROP_DTYPE.itemsize == 48


class ObjectCropsOut(C.Structure):
    """slhip_object_crops_out: the output pointers of slhip_object_crops_gather."""

    _fields_ = [("d_rgb", C.c_void_p), ("d_coord", C.c_void_p), ("d_normals", C.c_void_p), ("d_instance", C.c_void_p),
                ("d_mask", C.c_void_p)]


# slhip_object_point_params (include/slhip.h), 48 bytes
OBJECT_POINT_PARAMS_DTYPE = np.dtype([
    ("n_points", np.uint32), ("min_px", np.uint32), ("min_visib_fract", np.float32), ("fx", np.float32), ("fy", np.float32),
    ("cx", np.float32), ("cy", np.float32), ("seed_lo", np.uint32), ("seed_hi", np.uint32), ("scene_id_base", np.uint32),
    ("outputs", np.uint32), ("_pad", np.uint32),
])
assert OBJECT_POINT_PARAMS_DTYPE.itemsize == 48
# slhip_object_point_set (include/slhip.h), 16 bytes: one set of points
OBJECT_POINT_SET_DTYPE = np.dtype([("scene", np.uint32), ("slot", np.uint32), ("n_visib", np.uint32), ("_pad", np.uint32)])
assert OBJECT_POINT_SET_DTYPE.itemsize == 16


class ObjectPointsOut(C.Structure):
    """slhip_object_points_out: the output pointers of slhip_object_points_gather."""

    _fields_ = [("d_pixel", C.c_void_p), ("d_camera", C.c_void_p), ("d_coord", C.c_void_p), ("d_normals", C.c_void_p),
                ("d_rgb", C.c_void_p)]


# slhip_object_keypoint_params (include/slhip.h), 48 bytes
OBJECT_KEYPOINT_PARAMS_DTYPE = np.dtype([
    ("fx", np.float32), ("fy", np.float32), ("cx", np.float32), ("cy", np.float32), ("W", np.int32), ("H", np.int32),
    ("depth_tol", np.float32), ("n_keypoints", np.uint32), ("n_objects", np.uint32), ("mode", np.uint32), ("_pad", np.uint32, (2,)),
])
assert OBJECT_KEYPOINT_PARAMS_DTYPE.itemsize == 48
# slhip_object_region_params (include/slhip.h), 32 bytes
OBJECT_REGION_PARAMS_DTYPE = np.dtype([
    ("W", np.int32), ("H", np.int32), ("n_images", np.uint32), ("n_objects", np.uint32), ("n_regions", np.uint32),
    ("n_assets", np.uint32), ("outputs", np.uint32), ("_pad", np.uint32),
])
assert OBJECT_REGION_PARAMS_DTYPE.itemsize == 32
# slhip_render_flow_params (include/slhip.h), 48 bytes
RENDER_FLOW_PARAMS_DTYPE = np.dtype([
    ("fx", np.float32), ("fy", np.float32), ("cx", np.float32), ("cy", np.float32), ("W", np.int32), ("H", np.int32),
    ("n_slots", np.uint32), ("max_depth", np.float32), ("depth_tol", np.float32), ("depth_rel", np.float32), ("outputs", np.uint32),
    ("flags", np.uint32),
])
assert RENDER_FLOW_PARAMS_DTYPE.itemsize == 48
# slhip_pose_error_params (include/slhip.h), 32 bytes
POSE_ERROR_PARAMS_DTYPE = np.dtype([
    ("fx", np.float32), ("fy", np.float32), ("cx", np.float32), ("cy", np.float32), ("n_objects", np.uint32),
    ("n_hypotheses", np.uint32), ("outputs", np.uint32), ("_pad", np.uint32),
])
assert POSE_ERROR_PARAMS_DTYPE.itemsize == 32


class PoseBank(C.Structure):
    """slhip_pose_bank: the arrays of a model bank (device pointers, or host pointers for the _host entries)."""

    _fields_ = [("points", C.c_void_p), ("count", C.c_void_p), ("symmetries", C.c_void_p), ("n_sym", C.c_void_p),
                ("n_assets", C.c_uint32), ("n_points", C.c_uint32), ("n_symmetries", C.c_uint32), ("_pad", C.c_uint32)]


assert C.sizeof(PoseBank) == 48


class PoseErrorOut(C.Structure):
    """slhip_pose_error_out: the output pointers of slhip_pose_error."""

    _fields_ = [("add", C.c_void_p), ("adds", C.c_void_p), ("mssd", C.c_void_p), ("mssd_sym", C.c_void_p), ("mspd", C.c_void_p),
                ("mspd_sym", C.c_void_p)]


# slhip_pose_vsd_params (include/slhip.h), 128 bytes
POSE_VSD_PARAMS_DTYPE = np.dtype([
    ("fx", np.float32), ("fy", np.float32), ("cx", np.float32), ("cy", np.float32), ("W", np.int32), ("H", np.int32),
    ("n_objects", np.uint32), ("n_hypotheses", np.uint32), ("n_taus", np.uint32), ("delta", np.float32), ("z_near", np.float32),
    ("flags", np.uint32), ("outputs", np.uint32), ("_pad", np.uint32, (3,)), ("taus", np.float32, (VSD_TAUS_MAX,)),
])
assert POSE_VSD_PARAMS_DTYPE.itemsize == 128


class PoseSurface(C.Structure):
    """slhip_pose_surface: the arrays of a surface bank (device pointers, or host pointers for the _host entries)."""

    _fields_ = [("vertices", C.c_void_p), ("triangles", C.c_void_p), ("tri_begin", C.c_void_p), ("tri_count", C.c_void_p),
                ("diameter", C.c_void_p), ("n_assets", C.c_uint32), ("n_vertices", C.c_uint32), ("n_triangles", C.c_uint32),
                ("_pad", C.c_uint32)]


assert C.sizeof(PoseSurface) == 56


class PoseVsdOut(C.Structure):
    """slhip_pose_vsd_out: the output pointers of slhip_pose_vsd."""

    _fields_ = [("vsd", C.c_void_p), ("counts", C.c_void_p), ("n_cost", C.c_void_p), ("flags", C.c_void_p)]


# slhip_pose_pnp_params (include/slhip.h), 64 bytes
POSE_PNP_PARAMS_DTYPE = np.dtype([
    ("fx", np.float32), ("fy", np.float32), ("cx", np.float32), ("cy", np.float32), ("n_sets", np.uint32), ("n_points", np.uint32),
    ("n_hypotheses", np.uint32), ("threshold_px", np.float32), ("refine_iters", np.uint32), ("min_inliers", np.uint32),
    ("seed_lo", np.uint32), ("seed_hi", np.uint32), ("set_id_base", np.uint32), ("outputs", np.uint32), ("_pad", np.uint32, (2,)),
])
assert POSE_PNP_PARAMS_DTYPE.itemsize == 64


class PosePnpOut(C.Structure):
    """slhip_pose_pnp_out: the output pointers of slhip_pose_pnp."""

    _fields_ = [("pose", C.c_void_p), ("n_inliers", C.c_void_p), ("rms", C.c_void_p), ("inliers", C.c_void_p), ("best", C.c_void_p),
                ("flags", C.c_void_p)]


# slhip_keypoint_vote_params (include/slhip.h), 64 bytes
KEYPOINT_VOTE_PARAMS_DTYPE = np.dtype([
    ("W", np.uint32), ("H", np.uint32), ("n_sets", np.uint32), ("n_points", np.uint32), ("n_keypoints", np.uint32),
    ("n_hypotheses", np.uint32), ("inlier_cos", np.float32), ("min_inliers", np.uint32), ("min_sin", np.float32), ("outputs", np.uint32),
    ("seed_lo", np.uint32), ("seed_hi", np.uint32), ("set_id_base", np.uint32), ("_pad", np.uint32, (3,)),
])
assert KEYPOINT_VOTE_PARAMS_DTYPE.itemsize == 64


class KeypointVoteOut(C.Structure):
    """slhip_keypoint_vote_out: the output pointers of slhip_keypoint_vote."""

    _fields_ = [("uv", C.c_void_p), ("n_inliers", C.c_void_p), ("best", C.c_void_p), ("flags", C.c_void_p), ("mean", C.c_void_p),
                ("cov", C.c_void_p), ("inliers", C.c_void_p)]


# slhip_keypoint_vote3d_params (include/slhip.h), 64 bytes
KEYPOINT_VOTE3D_PARAMS_DTYPE = np.dtype([
    ("n_sets", np.uint32), ("n_points", np.uint32), ("n_keypoints", np.uint32), ("n_seeds", np.uint32), ("bandwidth", np.float32),
    ("max_iters", np.uint32), ("tol", np.float32), ("min_support", np.uint32), ("outputs", np.uint32), ("_pad", np.uint32, (7,)),
])
assert KEYPOINT_VOTE3D_PARAMS_DTYPE.itemsize == 64


class KeypointVote3dOut(C.Structure):
    """slhip_keypoint_vote3d_out: the output pointers of slhip_keypoint_vote3d."""

    _fields_ = [("xyz", C.c_void_p), ("n_support", C.c_void_p), ("best", C.c_void_p), ("iters", C.c_void_p), ("flags", C.c_void_p),
                ("mean", C.c_void_p), ("cov", C.c_void_p), ("support", C.c_void_p)]


# slhip_pose_fit_params (include/slhip.h), 64 bytes
POSE_FIT_PARAMS_DTYPE = np.dtype([
    ("n_sets", np.uint32), ("n_points", np.uint32), ("min_gap", np.float32), ("outputs", np.uint32), ("_pad", np.uint32, (12,)),
])
assert POSE_FIT_PARAMS_DTYPE.itemsize == 64


class PoseFitOut(C.Structure):
    """slhip_pose_fit_out: the output pointers of slhip_pose_fit."""

    _fields_ = [("pose", C.c_void_p), ("n_used", C.c_void_p), ("rms", C.c_void_p), ("flags", C.c_void_p)]


# slhip_pose_align_params (include/slhip.h), 64 bytes
POSE_ALIGN_PARAMS_DTYPE = np.dtype([
    ("n_sets", np.uint32), ("n_points", np.uint32), ("n_hypotheses", np.uint32), ("threshold", np.float32), ("min_gap", np.float32),
    ("refine_iters", np.uint32), ("min_inliers", np.uint32), ("seed_lo", np.uint32), ("seed_hi", np.uint32), ("set_id_base", np.uint32),
    ("outputs", np.uint32), ("_pad", np.uint32, (5,)),
])
assert POSE_ALIGN_PARAMS_DTYPE.itemsize == 64


class PoseAlignOut(C.Structure):
    """slhip_pose_align_out: the output pointers of slhip_pose_align."""

    _fields_ = [("pose", C.c_void_p), ("n_inliers", C.c_void_p), ("rms", C.c_void_p), ("inliers", C.c_void_p), ("best", C.c_void_p),
                ("flags", C.c_void_p)]


# slhip_pose_icp_params (include/slhip.h), 64 bytes
POSE_ICP_PARAMS_DTYPE = np.dtype([
    ("n_sets", np.uint32), ("n_points", np.uint32), ("max_iters", np.uint32), ("min_pairs", np.uint32), ("max_dist", np.float32),
    ("dist_scale", np.float32), ("min_dist", np.float32), ("min_gap", np.float32), ("tol_rot", np.float32), ("tol_trans", np.float32),
    ("outputs", np.uint32), ("_pad", np.uint32, (5,)),
])
assert POSE_ICP_PARAMS_DTYPE.itemsize == 64


class PoseIcpOut(C.Structure):
    """slhip_pose_icp_out: the output pointers of slhip_pose_icp."""

    _fields_ = [("pose", C.c_void_p), ("n_pairs", C.c_void_p), ("rms", C.c_void_p), ("iters", C.c_void_p), ("flags", C.c_void_p),
                ("nearest", C.c_void_p)]


# slhip_point_knn_params (include/slhip.h), 48 bytes
POINT_KNN_PARAMS_DTYPE = np.dtype([
    ("n_sets", np.uint32), ("n_queries", np.uint32), ("n_refs", np.uint32), ("query_stride", np.uint32), ("ref_stride", np.uint32),
    ("k", np.uint32), ("max_dist", np.float32), ("skip_same", np.uint32), ("outputs", np.uint32), ("_pad", np.uint32, (3,)),
])
assert POINT_KNN_PARAMS_DTYPE.itemsize == 48


class PointKnnOut(C.Structure):
    """slhip_point_knn_out: the output pointers of slhip_point_knn."""

    _fields_ = [("idx", C.c_void_p), ("dist2", C.c_void_p), ("count", C.c_void_p)]


# slhip_asset / slhip_synth_params / slhip_synth_object / slhip_synth_scene (include/slhip.h)
ASSET_DTYPE = np.dtype([
    ("mesh_to_object", np.float32, (16,)), ("bbox_min", np.float32, (4,)), ("bbox_max", np.float32, (4,)),
    ("com", np.float32, (4,)), ("inv_inertia", np.float32, (12,)), ("mass", np.float32), ("mu_s", np.float32),
    ("mu_d", np.float32), ("restitution", np.float32), ("bsphere", np.float32, (4,)), ("hull_begin", np.uint32),
    ("hull_end", np.uint32), ("draw_begin", np.uint32), ("draw_count", np.uint32), ("n_verts", np.uint32),
    ("n_chunks", np.uint32), ("_pad", np.uint32, (2,)),
])
assert ASSET_DTYPE.itemsize == 224
SYNTH_PARAMS_DTYPE = np.dtype([
    ("n_scenes", np.uint32), ("n_objects", np.uint32), ("n_assets", np.uint32), ("flags", np.uint32),
    ("seed_lo", np.uint32), ("seed_hi", np.uint32), ("scene_id_base", np.uint32), ("render_chunk", np.uint32),
    ("max_draws_per_scene", np.uint32), ("max_chunks_per_scene", np.uint32), ("max_clip_verts_per_scene", np.uint32),
    ("plane_z", np.float32), ("proj", np.float32, (16,)), ("proj_inv", np.float32, (16,)), ("plane_size", np.float32, (2,)),
    ("manual_exposure", np.float32), ("_pad0", np.float32), ("light_color", np.float32, (4,)), ("ambient", np.float32, (4,)),
])
assert SYNTH_PARAMS_DTYPE.itemsize == 224
SYNTH_OBJECT_DTYPE = np.dtype([("asset", np.uint32), ("instance_index", np.uint32), ("metallic", np.float32),
                               ("roughness", np.float32)])
SYNTH_SCENE_DTYPE = np.dtype([("plane_pose", np.float32, (16,)), ("camera_pose", np.float32, (16,))])
# slhip_env_light_set / slhip_env_texture / slhip_synth_env (include/slhip.h): the environment bank of slhip_synth_place_env
ENV_LIGHT_SET_DTYPE = np.dtype([("light_map", np.uint32), ("n_lights", np.uint32), ("_pad", np.uint32, (2,)),
                                ("light_dir", np.float32, (NUM_LIGHTS, 4)), ("light_color", np.float32, (NUM_LIGHTS, 4))])
assert ENV_LIGHT_SET_DTYPE.itemsize == 112
ENV_TEXTURE_DTYPE = np.dtype([("offset", np.uint32), ("w", np.uint32), ("h", np.uint32), ("sampler", np.uint32)])
assert ENV_TEXTURE_DTYPE.itemsize == 16


class SynthEnv(C.Structure):
    _fields_ = [
        ("d_light_sets", C.c_void_p),
        ("d_backgrounds", C.c_void_p),
        ("d_plane_textures", C.c_void_p),
        ("d_env_ids", C.c_void_p),
        ("n_light_sets", C.c_uint32),
        ("n_backgrounds", C.c_uint32),
        ("n_plane_textures", C.c_uint32),
        ("p_light_map", C.c_float),
        ("p_background", C.c_float),
        ("p_plane_texture", C.c_float),
    ]


assert C.sizeof(SynthEnv) == 56


class SynthView(C.Structure):
    """slhip_synth_view: which camera slhip_synth_place_view gives the scenes."""

    _fields_ = [
        ("view", C.c_uint32),
        ("_pad", C.c_uint32),
        ("d_camera_poses", C.c_void_p),
        ("d_object_to_camera", C.c_void_p),
    ]


assert C.sizeof(SynthView) == 24
VIEW_KEY_STEP = (0x9E3779B9, 0xBB67AE85)      # Philox key of view v: (seed_lo + v * step[0], seed_hi + v * step[1]) mod 2^32


def view_key(seed_lo, seed_hi, view):
    """The Philox key azimuth and elevation of view `view` are drawn with (include/slhip.h, "Randomness")."""
    return ((int(seed_lo) + int(view) * VIEW_KEY_STEP[0]) & 0xFFFFFFFF, (int(seed_hi) + int(view) * VIEW_KEY_STEP[1]) & 0xFFFFFFFF)


SYNTH_STREAM_ENV = 4     # Philox stream of the environment draws (include/slhip.h, "Randomness")
SYNTH_STREAM_CROP = 5    # Philox stream of the crop jitter (slhip_object_crops_select)
SYNTH_STREAM_POINTS = 6  # Philox stream of the point ranks (slhip_object_points_gather)
SYNTH_STREAM_PNP = 7     # Philox stream of the correspondence samples (slhip_pose_pnp)
SYNTH_STREAM_VOTE = 8    # Philox stream of the voter samples (slhip_keypoint_vote)
SYNTH_STREAM_ALIGN = 9   # Philox stream of the alignment samples (slhip_pose_align)
SYNTH_SAMPLE_DISTINCT = 1
SYNTH_RANDOM_PBR = 2
SYNTH_SHADOWS = 4
SYNTH_MAX_ASSETS = 1024

# SLHIP_LIB selects another build of the same library (developer A/B runs); there is no fallback
_LIB_PATH = os.environ.get("SLHIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libslhip.so")


class SlhipError(RuntimeError):
    pass


def lib_path():
    return _LIB_PATH


def lib():
    """Loads lib/libslhip.so (built by ``__graft_entry__.build()``); raises if absent."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(_LIB_PATH):
        raise SlhipError(
            "stillleben_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (there is no CPU fallback)" % _LIB_PATH
        )
    L = C.CDLL(_LIB_PATH)
    L.slhip_abi_version.restype = C.c_int
    L.slhip_last_error.restype = C.c_char_p
    L.slhip_device_init.argtypes = [C.c_int]
    L.slhip_render.argtypes = [
        C.POINTER(MeshPool), C.c_void_p, C.c_void_p, C.c_void_p,
        C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
        C.c_void_p, C.POINTER(RenderOut), C.POINTER(RenderScratch), C.c_void_p,
    ]
    L.slhip_render_scratch_bytes.argtypes = [
        C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64 * 7)
    ]
    L.slhip_settle_solver_wave_lds.restype = C.c_int
    L.slhip_settle_solver_wave_lds.argtypes = []
    L.slhip_timing_enable.argtypes = [C.c_int]
    L.slhip_render_timings.argtypes = [C.POINTER(C.c_float * 8)]
    L.slhip_diff_sobel_valid.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.slhip_diff_dilate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.slhip_diff_image_gradients.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.slhip_diff_pose_backward.argtypes = [C.c_void_p] * 7 + [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4
    L.slhip_diff_pose_backward_batch.argtypes = [C.c_void_p] * 4 + [C.c_uint64] + [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p] * 4
    L.slhip_diff_vertex_backward.argtypes = [C.c_void_p] * 8 + [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4
    L.slhip_settle.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_uint64, C.c_void_p]
    L.slhip_settle_status.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p]
    L.slhip_host_shadow_matrices.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.slhip_host_normal_matrix.argtypes = [C.c_void_p, C.c_void_p]
    L.slhip_host_convex_hull.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.slhip_host_fill_holes.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
    L.slhip_records_count.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.slhip_records_build_render.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                             C.c_uint32, C.c_void_p, C.c_uint32]
    L.slhip_render_object_stats.argtypes = [
        C.POINTER(MeshPool), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
        C.POINTER(RenderScratch), C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p,
    ]
    L.slhip_render_object_stats_bytes.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    L.slhip_render_object_masks.argtypes = [
        C.POINTER(MeshPool), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
        C.POINTER(RenderScratch), C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64),
        C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p,
    ]
    L.slhip_render_object_masks_bytes.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64),
                                                  C.POINTER(C.c_uint64)]
    L.slhip_object_masks_expand.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                            C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    L.slhip_render_ssao_skipped.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64 * 2), C.c_void_p]
    L.slhip_render_ssao_levels.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64 * 8), C.c_void_p]
    L.slhip_render_ssao_run_slots.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64 * 4), C.c_void_p]
    L.slhip_render_ssao_level_tables.argtypes = [C.POINTER(C.c_float * 5), C.POINTER(C.c_uint32 * 6), C.POINTER(C.c_uint8 * 384)]
    L.slhip_settle_caps.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64 * 10), C.c_void_p]
    L.slhip_settle_timing_enable.argtypes = [C.c_int]
    L.slhip_settle_timings.argtypes = [C.POINTER(C.c_float * 5), C.POINTER(C.c_uint32 * 5)]
    if hasattr(L, "slhip_settle_timing_every"):      # (absent from older builds selected through SLHIP_LIB for A/B runs)
        L.slhip_settle_timing_every.argtypes = [C.c_uint32]
        L.slhip_settle_timings_by_step.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.slhip_settle_scratch_bytes.argtypes = [C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64)]
    L.slhip_overlap_any.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.slhip_light_map_floats.argtypes = [C.c_uint32] * 6 + [C.POINTER(C.c_uint64 * 4)]
    L.slhip_light_map_build.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.slhip_camera_model.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    if hasattr(L, "slhip_depth_sensor"):             # (absent from older builds selected through SLHIP_LIB for A/B runs)
        L.slhip_depth_sensor_check_params.argtypes = [C.c_void_p, C.c_uint32, C.c_int]
        L.slhip_depth_sensor_timing_enable.argtypes = [C.c_int]
        L.slhip_depth_sensor_timings.argtypes = [C.POINTER(C.c_float * 2)]
        L.slhip_depth_sensor_scratch_bytes.argtypes = [C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
        L.slhip_depth_sensor.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "slhip_object_crops_select"):      # (absent from older builds selected through SLHIP_LIB for A/B runs)
        L.slhip_object_crops_check_params.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.slhip_object_crops_scratch_bytes.argtypes = [C.c_uint32, C.POINTER(C.c_uint64)]
        L.slhip_object_crops_select.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_void_p,
                                                C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]
        L.slhip_object_crops_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(RenderOut), C.c_uint32, C.c_int,
                                                C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(ObjectCropsOut), C.c_void_p]
        L.slhip_object_crops_timing_enable.argtypes = [C.c_int]
        L.slhip_object_crops_timings.argtypes = [C.POINTER(C.c_float * 2)]
    if hasattr(L, "slhip_object_points_select"):     # (absent from older builds selected through SLHIP_LIB for A/B runs)
        L.slhip_object_points_check_params.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.slhip_object_points_scratch_bytes.argtypes = [C.c_uint32, C.POINTER(C.c_uint64)]
        L.slhip_object_points_select.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                                 C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]
        L.slhip_object_points_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(RenderOut), C.c_void_p, C.c_uint32,
                                                 C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32,
                                                 C.POINTER(ObjectPointsOut), C.c_void_p]
        L.slhip_object_points_host_pixels.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                                      C.c_void_p]
        L.slhip_object_points_timing_enable.argtypes = [C.c_int]
        L.slhip_object_points_timings.argtypes = [C.POINTER(C.c_float * 2)]
    if hasattr(L, "slhip_object_keypoints_field"):   # (absent from older builds selected through SLHIP_LIB for A/B runs)
        L.slhip_object_keypoints_check_params.argtypes = [C.c_void_p]
        L.slhip_object_keypoints_fps_bytes.argtypes = [C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)]
        L.slhip_object_keypoints_fps.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32,
                                                 C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.slhip_object_keypoints_fps_host.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                                      C.c_uint32, C.c_void_p, C.c_void_p]
        L.slhip_object_keypoints_project.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                                     C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.slhip_object_keypoints_field.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                                   C.c_uint32, C.c_void_p, C.c_void_p]
        L.slhip_object_keypoints_timing_enable.argtypes = [C.c_int]
        L.slhip_object_keypoints_timings.argtypes = [C.POINTER(C.c_float * 3)]
    if hasattr(L, "slhip_object_regions_label"):     # (absent from older builds selected through SLHIP_LIB for A/B runs)
        L.slhip_object_regions_check_params.argtypes = [C.c_void_p]
        L.slhip_object_regions_centres_bytes.argtypes = [C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)]
        L.slhip_object_regions_centres.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32,
                                                   C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.slhip_object_regions_centres_host.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                                        C.c_uint32, C.c_void_p, C.c_void_p]
        L.slhip_object_regions_vertices.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                                    C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.slhip_object_regions_vertices_host.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                                         C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.slhip_object_regions_label.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]
        L.slhip_object_regions_label_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.c_void_p]
        L.slhip_object_regions_timing_enable.argtypes = [C.c_int]
        L.slhip_object_regions_timings.argtypes = [C.POINTER(C.c_float * 3)]
    if hasattr(L, "slhip_pose_error"):               # (absent from older builds selected through SLHIP_LIB for A/B runs)
        L.slhip_pose_error_check_params.argtypes = [C.c_void_p]
        L.slhip_pose_error_diameter.argtypes = [C.POINTER(PoseBank), C.c_void_p, C.c_void_p]
        L.slhip_pose_error_diameter_host.argtypes = [C.POINTER(PoseBank), C.c_void_p]
        L.slhip_pose_error.argtypes = [C.c_void_p, C.POINTER(PoseBank), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                       C.POINTER(PoseErrorOut), C.c_void_p]
        L.slhip_pose_error_host.argtypes = [C.c_void_p, C.POINTER(PoseBank), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                            C.c_uint32, C.POINTER(PoseErrorOut)]
        L.slhip_pose_error_timing_enable.argtypes = [C.c_int]
        L.slhip_pose_error_timings.argtypes = [C.POINTER(C.c_float * 2)]
    if hasattr(L, "slhip_pose_vsd"):                 # (absent from older builds selected through SLHIP_LIB for A/B runs)
        L.slhip_pose_vsd_check_params.argtypes = [C.c_void_p]
        L.slhip_pose_vsd.argtypes = [C.c_void_p, C.POINTER(PoseSurface), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_uint32, C.c_uint32, C.POINTER(PoseVsdOut), C.c_void_p]
        L.slhip_pose_vsd_host.argtypes = [C.c_void_p, C.POINTER(PoseSurface), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(PoseVsdOut)]
        L.slhip_pose_depth.argtypes = [C.c_void_p, C.POINTER(PoseSurface), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                       C.c_void_p, C.c_void_p]
        L.slhip_pose_depth_host.argtypes = [C.c_void_p, C.POINTER(PoseSurface), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                            C.c_void_p, C.c_void_p]
        L.slhip_pose_vsd_band_pixels.argtypes = []
        L.slhip_pose_vsd_timing_enable.argtypes = [C.c_int]
        L.slhip_pose_vsd_timings.argtypes = [C.POINTER(C.c_float * 2)]
    if hasattr(L, "slhip_pose_pnp"):                 # (absent from older builds selected through SLHIP_LIB for A/B runs)
        L.slhip_pose_pnp_check_params.argtypes = [C.c_void_p]
        L.slhip_pose_pnp.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PosePnpOut), C.c_void_p]
        L.slhip_pose_pnp_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PosePnpOut)]
        L.slhip_pose_pnp_p3p_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.slhip_pose_pnp_timing_enable.argtypes = [C.c_int]
        L.slhip_pose_pnp_timings.argtypes = [C.POINTER(C.c_float * 2)]
    if hasattr(L, "slhip_keypoint_vote"):            # (absent from older builds selected through SLHIP_LIB for A/B runs)
        L.slhip_keypoint_vote_check_params.argtypes = [C.c_void_p]
        L.slhip_keypoint_vote.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(KeypointVoteOut), C.c_void_p]
        L.slhip_keypoint_vote_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(KeypointVoteOut)]
        L.slhip_keypoint_vote_timing_enable.argtypes = [C.c_int]
        L.slhip_keypoint_vote_timings.argtypes = [C.POINTER(C.c_float * 2)]
    if hasattr(L, "slhip_keypoint_vote3d"):          # (absent from older builds selected through SLHIP_LIB for A/B runs)
        L.slhip_keypoint_vote3d_check_params.argtypes = [C.c_void_p]
        L.slhip_keypoint_vote3d.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(KeypointVote3dOut), C.c_void_p]
        L.slhip_keypoint_vote3d_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(KeypointVote3dOut)]
        L.slhip_keypoint_vote3d_timing_enable.argtypes = [C.c_int]
        L.slhip_keypoint_vote3d_timings.argtypes = [C.POINTER(C.c_float * 1)]
    if hasattr(L, "slhip_pose_fit"):                 # (absent from older builds selected through SLHIP_LIB for A/B runs)
        L.slhip_pose_fit_check_params.argtypes = [C.c_void_p]
        L.slhip_pose_fit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PoseFitOut), C.c_void_p]
        L.slhip_pose_fit_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PoseFitOut)]
        L.slhip_pose_fit_timing_enable.argtypes = [C.c_int]
        L.slhip_pose_fit_timings.argtypes = [C.POINTER(C.c_float * 1)]
    if hasattr(L, "slhip_pose_align"):               # (absent from older builds selected through SLHIP_LIB for A/B runs)
        L.slhip_pose_align_check_params.argtypes = [C.c_void_p]
        L.slhip_pose_align.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PoseAlignOut), C.c_void_p]
        L.slhip_pose_align_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PoseAlignOut)]
        L.slhip_pose_align_timing_enable.argtypes = [C.c_int]
        L.slhip_pose_align_timings.argtypes = [C.POINTER(C.c_float * 1)]
    if hasattr(L, "slhip_pose_icp"):                 # (absent from older builds selected through SLHIP_LIB for A/B runs)
        L.slhip_pose_icp_check_params.argtypes = [C.c_void_p]
        L.slhip_pose_icp.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PoseBank), C.POINTER(PoseIcpOut), C.c_void_p]
        L.slhip_pose_icp_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PoseBank), C.POINTER(PoseIcpOut)]
        L.slhip_pose_icp_timing_enable.argtypes = [C.c_int]
        L.slhip_pose_icp_timings.argtypes = [C.POINTER(C.c_float * 1)]
    if hasattr(L, "slhip_render_flow"):              # (absent from older builds selected through SLHIP_LIB for A/B runs)
        L.slhip_render_flow_check_params.argtypes = [C.c_void_p]
        L.slhip_render_flow.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                        C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.slhip_render_flow_host.argtypes = L.slhip_render_flow.argtypes[:-1]
        L.slhip_render_flow_motion.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.slhip_render_flow_motion_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    if hasattr(L, "slhip_point_knn"):                # (absent from older builds selected through SLHIP_LIB for A/B runs)
        L.slhip_point_knn_check_params.argtypes = [C.c_void_p]
        L.slhip_point_knn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PointKnnOut), C.c_void_p]
        L.slhip_point_knn_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PointKnnOut)]
        L.slhip_point_knn_timing_enable.argtypes = [C.c_int]
        L.slhip_point_knn_timings.argtypes = [C.POINTER(C.c_float * 1)]
    L.slhip_stream_create_cu_range.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    L.slhip_stream_destroy.argtypes = [C.c_void_p]
    L.slhip_synth_stage.argtypes = [C.c_void_p] * 8
    L.slhip_synth_place.argtypes = [C.c_void_p] * 10
    if hasattr(L, "slhip_synth_place_env"):          # (absent from older builds selected through SLHIP_LIB for A/B runs)
        L.slhip_synth_place_env.argtypes = [C.c_void_p, C.POINTER(SynthEnv)] + [C.c_void_p] * 10
    if hasattr(L, "slhip_synth_place_view"):
        L.slhip_synth_place_view.argtypes = [C.c_void_p, C.POINTER(SynthEnv), C.POINTER(SynthView)] + [C.c_void_p] * 10
    L.slhip_comm_unique_id.argtypes = [C.c_void_p]
    L.slhip_comm_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.slhip_comm_destroy.argtypes = [C.c_void_p]
    L.slhip_comm_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.slhip_allgather.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.slhip_allgather_group.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    _LIB = L
    return L


def check(status, what):
    if status != 0:
        msg = lib().slhip_last_error()
        raise SlhipError("%s failed (%d): %s" % (what, status, msg.decode() if msg else "?"))
