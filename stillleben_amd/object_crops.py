"""Object crops -- this project's addition (the reference has no counterpart): one fixed-size square window per visible object
of a render, the input of an object-centric network in the style of CosyPose, GDR-Net or ZebraPose.  The window is cut round
the object's 2D box, enlarged by `pad`, and randomly scaled and shifted ("dynamic zoom-in"); with it come the object-coordinate
map, the visible and amodal masks and the window's intrinsics.  Everything stays on the device: `extract` runs
slhip_object_crops_select (statistics -> a compact list of windows in ascending (scene, slot) order) and
slhip_object_crops_gather (one thread per output pixel) of include/slhip.h; there is no CPU path.

    buffers = batch.render(0, object_masks=True)
    crops = batch.crops(buffers, size=128, jitter_scale=0.25, jitter_shift=0.25)       # or sl.object_crops.extract(...)
    crops.rgb, crops.coord, crops.mask_visib, crops.mask_all, crops.K3x3(), crops.scene, crops.slot

rgb is resampled bilinearly, everything else takes the nearest pixel; outside the picture every channel is 0.  There is NO
anti-aliasing filter: a window larger than `size` source pixels (step > 1) is point-sampled, not prefiltered.  DESIGN.md
"Object crops" states the rules operation by operation."""
import ctypes as C

import numpy as np
import torch

from . import _abi, _device, _record_set

__all__ = ["OUTPUTS", "BOXES", "ObjectCrops", "make_params", "check_params", "extract"]

OUTPUTS = {"rgb": _abi.CROP_RGB, "coord": _abi.CROP_COORD, "normals": _abi.CROP_NORMALS, "instance": _abi.CROP_INSTANCE,
           "mask": _abi.CROP_MASK}
BOXES = {"visib": 0, "obj": 1}
_TENSORS = ("records", "rgb", "coord", "normals", "instance", "mask", "scene_global", "object_to_camera")


def make_params(intrinsics, size=128, box="visib", pad=1.4, jitter_scale=0.0, jitter_shift=0.0, min_px=1, min_visib_fract=0.0,
                outputs=("rgb", "coord", "mask"), isolate=True, seed=0, scene_id_base=0):
    """One slhip_object_crop_params record (numpy).  `intrinsics`: (fx, fy, cx, cy) the picture was rendered with.  `seed`:
    an integer, or the (lo, hi) pair of a Philox key."""
    if box not in BOXES:
        raise ValueError("box must be 'visib' (bbox_visib) or 'obj' (bbox_obj), not %r" % (box,))
    bits = _record_set.output_bits(outputs, OUTPUTS)
    p = np.zeros((), _abi.OBJECT_CROP_PARAMS_DTYPE)
    p["size"], p["box"] = int(size), BOXES[box]
    p["pad"], p["jitter_scale"], p["jitter_shift"] = np.float32(pad), np.float32(jitter_scale), np.float32(jitter_shift)
    p["min_px"], p["min_visib_fract"] = int(min_px), np.float32(min_visib_fract)
    p["fx"], p["fy"], p["cx"], p["cy"] = (np.float32(v) for v in intrinsics)
    _record_set.set_key(p, seed, scene_id_base)
    p["outputs"], p["isolate"] = bits, 1 if isolate else 0
    return p


def check_params(params, width, height):
    """Raises SlhipError when the record breaks a rule of slhip_object_crops_check_params.  Needs no device."""
    rec = np.ascontiguousarray(np.asarray(params, dtype=_abi.OBJECT_CROP_PARAMS_DTYPE).reshape(1))
    _abi.check(_abi.lib().slhip_object_crops_check_params(rec.ctypes.data, int(width), int(height)), "slhip_object_crops")
    return rec


class ObjectCrops(_record_set.RecordSet):
    """n windows of N x N pixels.  Tensors (None when not asked for):
        rgb       uint8 [n, N, N, 4]       coord    float32 [n, N, N, 4] (object xyz, camera z)
        normals   float32 [n, N, N, 4]     instance int16 [n, N, N]
        mask      uint8 [n, N, N]: bit 0 visible, bit 1 amodal -- mask_visib / mask_all give them as bool
    and, as views of `records` (int32 [n, 12], the slhip_object_crop array):
        scene, slot  int32 [n]             box  float32 [n, 4] = x0, y0, side, step
        K            float32 [n, 4] = fx', fy', cx', cy' of the window; K3x3() the matrices
    SceneBatch.crops adds scene_global (int32 [n]) and, when the batch keeps it, object_to_camera (float32 [n, 3, 4])."""

    _TENSORS, _ITEM = _TENSORS, "crop"

    def __init__(self, records, size, rgb=None, coord=None, normals=None, instance=None, mask=None, scene_global=None,
                 object_to_camera=None):
        super().__init__(records, scene_global, object_to_camera)
        self.size = int(size)
        self.rgb, self.coord, self.normals, self.instance, self.mask = rgb, coord, normals, instance, mask

    def _like(self, records):
        return ObjectCrops(records, self.size)

    @property
    def box(self):
        return self.records[..., 2:6].view(torch.float32)

    @property
    def K(self):
        return self.records[..., 6:10].view(torch.float32)

    def K3x3(self):
        """float32 [n, 3, 3] (or [3, 3] for a single crop): [[fx', 0, cx'], [0, fy', cy'], [0, 0, 1]]."""
        k = self.K
        m = torch.zeros(tuple(k.shape[:-1]) + (3, 3), dtype=torch.float32, device=k.device)
        m[..., 0, 0], m[..., 1, 1], m[..., 0, 2], m[..., 1, 2], m[..., 2, 2] = k[..., 0], k[..., 1], k[..., 2], k[..., 3], 1.0
        return m

    @property
    def mask_visib(self):
        return None if self.mask is None else (self.mask & 1) != 0

    @property
    def mask_all(self):
        return None if self.mask is None else (self.mask & 2) != 0

    def __repr__(self):
        n = self.records.shape[0] if self.records.dim() == 2 else 1
        return "ObjectCrops(%d x %d x %d: %s)" % (n, self.size, self.size, ", ".join(
            k for k in ("rgb", "coord", "normals", "instance", "mask") if getattr(self, k) is not None))


def extract(buffers, intrinsics, size=128, box="visib", pad=1.4, jitter_scale=0.0, jitter_shift=0.0, min_px=1,
            min_visib_fract=0.0, outputs=("rgb", "coord", "mask"), isolate=True, seed=0, scene_id_base=0, stats=None, masks=None):
    """The crops of every eligible (scene, slot) of `buffers` (a RenderBuffers), in ascending (scene, slot) order.

    intrinsics       (fx, fy, cx, cy) the picture was rendered with
    size             N, 1..1024
    box              "visib" (bbox_visib) or "obj" (bbox_obj, the whole silhouette's box)
    pad              side of the window / longer side of the box
    jitter_scale     in [0, 1): the side is scaled by a uniform factor in 1 +- jitter_scale
    jitter_shift     in [0, 1]: the centre moves by a uniform +- jitter_shift of the box's width and height
    min_px, min_visib_fract   a slot with fewer visible pixels, or a smaller visible share of its silhouette, gets no crop
    outputs          any of "rgb", "coord", "normals", "instance", "mask"
    isolate          coord and normals are zero wherever the window does not show this object
    seed, scene_id_base   Philox key and first scene id of the jitter (stream 5 of include/slhip.h, "Randomness")
    stats, masks     default to buffers.object_stats / buffers.object_masks; without masks the amodal bit stays 0

    rgb is bilinear, the rest nearest; there is no anti-aliasing filter for windows larger than N source pixels.
    Synchronises the current stream once (the number of crops sizes the outputs)."""
    params = make_params(intrinsics, size, box, pad, jitter_scale, jitter_shift, min_px, min_visib_fract, outputs, isolate, seed,
                         scene_id_base)
    stats = buffers.object_stats if stats is None else stats
    masks = getattr(buffers, "object_masks", None) if masks is None else masks
    if stats is None:
        raise RuntimeError("object_crops needs the statistics of the render: render with object_stats=True or "
                           "object_masks=True, or pass stats=")
    bits = int(params["outputs"])
    need = [("rgb", bits & _abi.CROP_RGB), ("coord", bits & _abi.CROP_COORD), ("normals", bits & _abi.CROP_NORMALS),
            ("instance", bits & (_abi.CROP_INSTANCE | _abi.CROP_MASK)
             or (params["isolate"] and bits & (_abi.CROP_COORD | _abi.CROP_NORMALS)))]
    used = _record_set.rendered("object_crops", buffers, need)
    B, H, W = (int(v) for v in used[0].shape[:3])
    rec = check_params(params, W, H)
    d_stats = stats.records()
    tensors = used + [d_stats] + ([masks.records, masks.words] if masks is not None else [])
    dev = _device.require_cuda("object_crops", tensors, "buffers, statistics and masks")
    for name, wanted in need:
        t = getattr(buffers, name)
        if wanted and (tuple(t.shape[:3]) != (B, H, W) or not t.is_contiguous()):
            raise ValueError("object_crops: `%s` must be a contiguous [%d, %d, %d, C] tensor" % (name, B, H, W))
    S = int(d_stats.shape[1])
    if int(d_stats.shape[0]) != B:
        raise ValueError("object_crops: statistics of %d scenes for a picture of %d" % (int(d_stats.shape[0]), B))
    if masks is not None and (tuple(masks.records.shape[:2]) != (B, S) or tuple(masks.size) != (H, W)
                              or not masks.records.is_contiguous()):
        raise ValueError("object_crops: the masks do not belong to this picture (%s records, size %s)"
                         % (tuple(masks.records.shape), masks.size))
    N = int(params["size"])
    records, scratch = _record_set.select("slhip_object_crops_select", rec, [d_stats], B, S, (W, H), 12, dev)
    n = len(records)
    crops = ObjectCrops(records, N, **_record_set.empty_outputs(n, bits, dev, (
        ("rgb", _abi.CROP_RGB, (N, N, 4), torch.uint8), ("coord", _abi.CROP_COORD, (N, N, 4), torch.float32),
        ("normals", _abi.CROP_NORMALS, (N, N, 4), torch.float32), ("instance", _abi.CROP_INSTANCE, (N, N), torch.int16),
        ("mask", _abi.CROP_MASK, (N, N), torch.uint8))))
    if n:
        ptr = _device.ptr
        src = _abi.RenderOut()
        src.d_rgb, src.d_coord, src.d_normals, src.d_instance = (ptr(getattr(buffers, k)) for k in ("rgb", "coord", "normals", "instance"))
        out = _abi.ObjectCropsOut()
        out.d_rgb, out.d_coord, out.d_normals, out.d_instance, out.d_mask = (ptr(t) for t in (crops.rgb, crops.coord, crops.normals,
                                                                                              crops.instance, crops.mask))
        with torch.cuda.device(dev):
            st = _abi.lib().slhip_object_crops_gather(rec.ctypes.data, C.c_void_p(records.data_ptr()), n, C.byref(src), B, W, H,
                                             C.c_void_p(ptr(masks.records) if masks is not None else None),
                                             C.c_void_p(ptr(masks.words) if masks is not None else None), S,
                                             C.byref(out), _device.stream_ptr(dev))
        _abi.check(st, "slhip_object_crops_gather")
    crops._keepalive = (buffers, d_stats, masks, scratch)      # the gather is asynchronous: its inputs live as long as its outputs
    return crops
