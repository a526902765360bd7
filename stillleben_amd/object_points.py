"""Object points -- this project's addition (the reference has no counterpart): a fixed number of pixels per visible object of a
render, drawn inside its visible mask, and what the render shows there -- the input of networks that take K points per object
(DenseFusion, PVN3D, FFB6D, PointNet-style refiners, ICP-style losses): the "choose" indices, the camera-frame point cloud from
ideal or sensor-like depth, and per point the object coordinates (the dense correspondence target), the normal and the colour.
Everything stays on the device: `extract` runs slhip_object_points_select (statistics and mask records -> a compact list of sets
in ascending (scene, slot) order) and slhip_object_points_gather (one workgroup per set finds the pixels in the visible mask's
bit tiles and gathers there) of include/slhip.h; there is no CPU path and no dense mask.

    buffers = batch.render(0, object_masks=True)
    points = batch.points(buffers, n_points=1024)                        # or sl.object_points.extract(...)
    points.camera, points.coord, points.index, points.valid, points.scene, points.slot

The K pixels are a stratified draw over the object's visible pixels in tile order: without replacement and spread over the whole
mask when the object shows at least K pixels, the mask repeated when it shows fewer; the same seed gives the same points.
DESIGN.md "Object points" states the rules operation by operation."""
import ctypes as C

import numpy as np
import torch

from . import _abi, _device, _record_set

__all__ = ["OUTPUTS", "ObjectPoints", "make_params", "check_params", "extract"]

OUTPUTS = {"pixel": _abi.POINTS_PIXEL, "camera": _abi.POINTS_CAMERA, "coord": _abi.POINTS_COORD, "normals": _abi.POINTS_NORMALS,
           "rgb": _abi.POINTS_RGB}
_TENSORS = ("records", "pixel", "camera", "coord", "normals", "rgb", "scene_global", "object_to_camera")


def make_params(intrinsics, n_points=1024, min_px=1, min_visib_fract=0.0, outputs=("pixel", "camera", "coord"), seed=0,
                scene_id_base=0):
    """One slhip_object_point_params record (numpy).  `intrinsics`: (fx, fy, cx, cy) the picture was rendered with.  `seed`:
    an integer, or the (lo, hi) pair of a Philox key."""
    bits = _record_set.output_bits(outputs, OUTPUTS)
    p = np.zeros((), _abi.OBJECT_POINT_PARAMS_DTYPE)
    p["n_points"], p["min_px"], p["min_visib_fract"] = int(n_points), int(min_px), np.float32(min_visib_fract)
    p["fx"], p["fy"], p["cx"], p["cy"] = (np.float32(v) for v in intrinsics)
    _record_set.set_key(p, seed, scene_id_base)
    p["outputs"] = bits
    return p


def check_params(params, width, height):
    """Raises SlhipError when the record breaks a rule of slhip_object_points_check_params.  Needs no device."""
    rec = np.ascontiguousarray(np.asarray(params, dtype=_abi.OBJECT_POINT_PARAMS_DTYPE).reshape(1))
    _abi.check(_abi.lib().slhip_object_points_check_params(rec.ctypes.data, int(width), int(height)), "slhip_object_points")
    return rec


class ObjectPoints(_record_set.RecordSet):
    """n sets of K points.  Tensors (None when not asked for):
        pixel    int16 [n, K, 2] (x, y)          camera   float32 [n, K, 4] (X, Y, Z, valid), the renderer's camera frame
        coord    float32 [n, K, 4] (object xyz, camera z)                   normals  float32 [n, K, 4]
        rgb      uint8 [n, K, 4]
    and, as views of `records` (int32 [n, 4], the slhip_object_point_set array): scene, slot, n_visib  int32 [n].
        valid    bool [n, K]: the camera point has a depth (camera w != 0)
        index    int64 [n, K]: y * W + x, the "choose" of DenseFusion
    SceneBatch.points adds scene_global (int32 [n]) and, when the batch keeps it, object_to_camera (float32 [n, 3, 4])."""

    _TENSORS, _ITEM = _TENSORS, "set"

    def __init__(self, records, width, pixel=None, camera=None, coord=None, normals=None, rgb=None, scene_global=None,
                 object_to_camera=None):
        super().__init__(records, scene_global, object_to_camera)
        self.width = int(width)
        self.pixel, self.camera, self.coord, self.normals, self.rgb = pixel, camera, coord, normals, rgb

    def _like(self, records):
        return ObjectPoints(records, self.width)

    @property
    def n_visib(self):
        return self.records[..., 2]

    @property
    def valid(self):
        return None if self.camera is None else self.camera[..., 3] != 0

    @property
    def index(self):
        return None if self.pixel is None else self.pixel[..., 1].long() * self.width + self.pixel[..., 0].long()

    def __repr__(self):
        n = self.records.shape[0] if self.records.dim() == 2 else 1
        shown = [k for k in _TENSORS[1:6] if getattr(self, k) is not None]
        k = getattr(self, shown[0]).shape[-2] if shown else 0
        return "ObjectPoints(%d x %d: %s)" % (n, k, ", ".join(shown))


def extract(buffers, intrinsics, n_points=1024, min_px=1, min_visib_fract=0.0, outputs=("pixel", "camera", "coord"), depth=None,
            seed=0, scene_id_base=0, stats=None, masks=None):
    """The point sets of every eligible (scene, slot) of `buffers` (a RenderBuffers), in ascending (scene, slot) order.

    intrinsics       (fx, fy, cx, cy) the picture was rendered with
    n_points         K, 1..16384
    min_px, min_visib_fract   a slot with fewer visible pixels, or a smaller visible share of its silhouette, gets no set
    outputs          any of "pixel", "camera", "coord", "normals", "rgb"
    depth            float32 [B, H, W] the camera points take their z from (sl.depth_sensor's float output: its holes, 0, give
                     invalid points); default: the w of `coord`, the ideal depth
    seed, scene_id_base   Philox key and first scene id of the draw (stream 6 of include/slhip.h, "Randomness")
    stats, masks     default to buffers.object_stats / buffers.object_masks; the masks are required (render with
                     object_masks=True): the pixels are found in their bit tiles

    Synchronises the current stream once (the number of sets sizes the outputs)."""
    params = make_params(intrinsics, n_points, min_px, min_visib_fract, outputs, seed, scene_id_base)
    masks = getattr(buffers, "object_masks", None) if masks is None else masks
    if masks is None:
        raise RuntimeError("object_points needs the masks of the render: render with object_masks=True, or pass masks=")
    if stats is None:
        stats = getattr(buffers, "object_stats", None)
        stats = masks.stats if stats is None else stats
    if stats is None:
        raise RuntimeError("object_points needs the statistics of the render: render with object_masks=True, or pass stats=")
    bits = int(params["outputs"])
    need = [("coord", bits & _abi.POINTS_COORD or (bits & _abi.POINTS_CAMERA and depth is None)),
            ("normals", bits & _abi.POINTS_NORMALS), ("rgb", bits & _abi.POINTS_RGB)]
    used = _record_set.rendered("object_points", buffers, need)
    H, W = masks.size
    B, S = (int(v) for v in masks.records.shape[:2])
    rec = check_params(params, W, H)
    d_stats = stats.records()
    if bits & _abi.POINTS_CAMERA and depth is not None:
        if depth.dtype != torch.float32 or tuple(depth.shape) != (B, H, W) or not depth.is_contiguous():
            raise ValueError("object_points: `depth` must be a contiguous float32 [%d, %d, %d] tensor" % (B, H, W))
        used.append(depth)
    tensors = [masks.records, masks.words, d_stats] + used
    dev = _device.require_cuda("object_points", tensors, "buffers, depth, statistics and masks")
    for name, wanted in need:
        t = getattr(buffers, name)
        if wanted and (tuple(t.shape) != (B, H, W, 4) or not t.is_contiguous()):
            raise ValueError("object_points: `%s` must be a contiguous [%d, %d, %d, 4] tensor" % (name, B, H, W))
    if tuple(d_stats.shape[:2]) != (B, S) or not masks.records.is_contiguous():
        raise ValueError("object_points: statistics of %s (scenes, slots) for masks of %s" % (tuple(d_stats.shape[:2]), (B, S)))
    K = int(params["n_points"])
    records, scratch = _record_set.select("slhip_object_points_select", rec, [d_stats, masks.records], B, S, (), 4, dev)
    n = len(records)
    points = ObjectPoints(records, W, **_record_set.empty_outputs(n, bits, dev, (
        ("pixel", _abi.POINTS_PIXEL, (K, 2), torch.int16), ("camera", _abi.POINTS_CAMERA, (K, 4), torch.float32),
        ("coord", _abi.POINTS_COORD, (K, 4), torch.float32), ("normals", _abi.POINTS_NORMALS, (K, 4), torch.float32),
        ("rgb", _abi.POINTS_RGB, (K, 4), torch.uint8))))
    if n:
        ptr = _device.ptr
        src = _abi.RenderOut()
        src.d_rgb, src.d_coord, src.d_normals = (ptr(getattr(buffers, k, None)) for k in ("rgb", "coord", "normals"))
        d_depth, stride = None, 0
        if bits & _abi.POINTS_CAMERA:      # the sensor's plane, or the w of coord read in place as slhip_depth_sensor reads it
            d_depth, stride = (depth.data_ptr(), 1) if depth is not None else (buffers.coord.data_ptr() + 12, 4)
        out = _abi.ObjectPointsOut()
        out.d_pixel, out.d_camera, out.d_coord, out.d_normals, out.d_rgb = (ptr(t) for t in (points.pixel, points.camera, points.coord,
                                                                                              points.normals, points.rgb))
        with torch.cuda.device(dev):
            st = _abi.lib().slhip_object_points_gather(rec.ctypes.data, C.c_void_p(records.data_ptr()), n, C.byref(src), C.c_void_p(d_depth),
                                              stride, B, W, H, C.c_void_p(masks.records.data_ptr()),
                                              C.c_void_p(masks.words.data_ptr()), S, C.byref(out), _device.stream_ptr(dev))
        _abi.check(st, "slhip_object_points_gather")
    points._keepalive = (buffers, depth, d_stats, masks, scratch)      # the gather is asynchronous: its inputs live as long as its outputs
    return points
