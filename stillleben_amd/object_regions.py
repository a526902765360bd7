"""Object regions -- this project's addition (the reference has no counterpart): the targets of pose networks that classify
every pixel into a surface region of its object and regress inside it (GDR-Net's surface region attention, EPOS' surface
fragments and fragment-local coordinates, SO-Pose, the coarse levels of ZebraPose).  The `coord` target gives object-frame xyz
per pixel and `sl.object_keypoints` farthest-point centres per class; this module joins the two.  Everything stays on the
device, through three entries of include/slhip.h: slhip_object_regions_centres (farthest point sampling of up to 255 centres per
class, the keypoints' rule and kernel), slhip_object_regions_vertices (the region of every mesh vertex, per-region counts and
extents; both once per asset table) and slhip_object_regions_label (the region of every pixel, one byte each, optionally the
coordinates relative to the region's centre and a per-object histogram).  There is no CPU path.

    bank = sl.object_regions.bank(table, n_regions=64)                   # once: centres [A, 64, 4], count, extent, vertex_region
    buffers = batch.render(0)
    reg = batch.regions(buffers, bank=bank, local=True, histogram=True)  # or sl.object_regions.label(...)
    reg.region                                                           # uint8 [B, H, W], 255 where no object
    reg.local, reg.histogram, reg.visible
    sl.ObjectRegions.of_crops(crops, batch_classes, bank)                # the same on the windows of sl.object_crops
    reg.at(batch.points(buffers, n_points=1024))                         # uint8 [n, K]: the regions of the sampled pixels

DESIGN.md "Object regions" states the rules operation by operation."""
import ctypes as C

import numpy as np
import torch

from . import _abi, _device

__all__ = ["NONE", "RegionBank", "ObjectRegions", "make_params", "check_params", "centres", "vertices", "bank", "label",
           "centres_host", "vertices_host", "label_host"]

NONE = _abi.REGION_NONE


def make_params(size, n_images, n_objects, n_regions, n_assets, local=False, histogram=False):
    """One slhip_object_region_params record (numpy).  `size`: (W, H)."""
    p = np.zeros((), _abi.OBJECT_REGION_PARAMS_DTYPE)
    p["W"], p["H"] = int(size[0]), int(size[1])
    p["n_images"], p["n_objects"], p["n_regions"], p["n_assets"] = int(n_images), int(n_objects), int(n_regions), int(n_assets)
    p["outputs"] = (_abi.REGIONS_OUT_LOCAL if local else 0) | (_abi.REGIONS_OUT_HISTOGRAM if histogram else 0)
    return p


def check_params(params):
    """Raises SlhipError when the record breaks a rule of slhip_object_regions_check_params.  Needs no device."""
    rec = np.ascontiguousarray(np.asarray(params, dtype=_abi.OBJECT_REGION_PARAMS_DTYPE).reshape(1))
    _abi.check(_abi.lib().slhip_object_regions_check_params(rec.ctypes.data), "slhip_object_regions")
    return rec


# ---- host twins: the CPU tests' handles ----------------------------------------------------------------------------------------
def centres_host(positions, assets, templates, n_regions):
    """slhip_object_regions_centres_host: (centres float32 [A, R, 4], vertex int32 [A, R]) on host arrays.  Needs no device."""
    return _device.fps_host(positions, assets, templates, n_regions, "slhip_object_regions_centres_host")


def vertices_host(positions, assets, templates, centres):
    """slhip_object_regions_vertices_host: (vertex_region uint8 [V], count int32 [A, R], extent float32 [A, R, 4]) on host
    arrays.  Needs no device."""
    pos, assets, templates = _device.host_table(positions, assets, templates)
    cen = np.ascontiguousarray(centres, dtype=np.float32)
    A, R = len(assets), int(cen.shape[1])
    if cen.shape != (A, R, 4):
        raise ValueError("object_regions: centres must be [%d, R, 4]" % A)
    vr, count, extent = np.zeros(len(pos), np.uint8), np.zeros((A, R), np.int32), np.zeros((A, R, 4), np.float32)
    st = _abi.lib().slhip_object_regions_vertices_host(pos.ctypes.data if len(pos) else None, len(pos), assets.ctypes.data, A,
                                                       templates.ctypes.data if len(templates) else None, len(templates),
                                                       cen.ctypes.data, R, vr.ctypes.data if len(pos) else None, count.ctypes.data,
                                                       extent.ctypes.data)
    _abi.check(st, "slhip_object_regions_vertices_host")
    return vr, count, extent


def label_host(instance, coord, classes, centres, local=False, histogram=False, class_stride=1):
    """slhip_object_regions_label_host on host arrays: instance int16 [N, H, W], coord float32 [N, H, W, 4], classes int32 read at
    (image * O + object) * class_stride ([N, O] for stride 1, [N, O, 4] for stride 4), centres float32 [A, R, 4].  Returns
    (region uint8 [N, H, W], local float32 [N, H, W, 4] or None, histogram uint32 [N, O, R] or None).  Needs no device."""
    inst = np.ascontiguousarray(instance, dtype=np.int16)
    xyz = np.ascontiguousarray(coord, dtype=np.float32)
    cls = np.ascontiguousarray(classes, dtype=np.int32)
    cen = np.ascontiguousarray(centres, dtype=np.float32)
    N, H, W = inst.shape
    O, (A, R) = int(cls.shape[1]), cen.shape[:2]
    if xyz.shape != (N, H, W, 4) or cls.size != N * O * class_stride:
        raise ValueError("object_regions: coord must be [N, H, W, 4] and classes [N, O] (or [N, O, class_stride])")
    rec = check_params(make_params((W, H), N, O, R, A, local, histogram))
    region = np.zeros((N, H, W), np.uint8)
    loc = np.zeros((N, H, W, 4), np.float32) if local else None
    hist = np.zeros((N, O, R), np.uint32) if histogram else None
    st = _abi.lib().slhip_object_regions_label_host(rec.ctypes.data, inst.ctypes.data, xyz.ctypes.data, cls.ctypes.data, int(class_stride),
                                                    cen.ctypes.data, region.ctypes.data, None if loc is None else loc.ctypes.data,
                                                    None if hist is None else hist.ctypes.data)
    _abi.check(st, "slhip_object_regions_label_host")
    return region, loc, hist


# ---- the bank, once per asset table --------------------------------------------------------------------------------------------
def centres(table, n_regions):
    """Farthest point sampling of `n_regions` (1..255) centres of every class of an sl.AssetTable on the device, by the rule of
    sl.object_keypoints.fps: (centres float32 [A, R, 4] = (x, y, z, 1) in the object frame -- the frame of the `coord` target --,
    vertex int32 [A, R], the mesh vertex each one is).  The first 32 are the keypoint FPS, bit for bit.  Asynchronous on the
    current stream."""
    return _device.fps(table, n_regions, "slhip_object_regions_centres", "slhip_object_regions_centres_bytes")


def vertices(table, centres):
    """The region of every pool vertex under `centres` (float32 [A, R, 4] on the table's device; any bank, not only FPS):
    (vertex_region uint8 [n_vertices], 255 for a vertex of no class; count int32 [A, R]; extent float32 [A, R, 4] = the largest
    |dx|, |dy|, |dz| and d2 of the region's vertices against its centre, zeros for an empty region -- what EPOS normalises
    fragment coordinates by).  Asynchronous on the current stream."""
    eng, d_pos, d_assets, d_templates = _device.table_on_device(table)
    dev = eng.device
    A = len(table)
    if not isinstance(centres, torch.Tensor):
        raise _abi.SlhipError(_device.no_cpu("object_regions"))
    _device.require_cuda("object_regions", (centres,), "the centres and the asset table", device=dev)
    if centres.dtype != torch.float32 or centres.dim() != 3 or tuple(centres.shape[::2]) != (A, 4) or not centres.is_contiguous():
        raise ValueError("object_regions: the centres must be a contiguous float32 [%d, R, 4] tensor" % A)
    R, V = int(centres.shape[1]), int(eng.pool.n_vertices)
    vr = torch.empty((V,), dtype=torch.uint8, device=dev)
    count = torch.empty((A, R), dtype=torch.int32, device=dev)
    extent = torch.empty((A, R, 4), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        st = _abi.lib().slhip_object_regions_vertices(C.c_void_p(d_pos.data_ptr()), V, C.c_void_p(d_assets.data_ptr()), A,
                                                      C.c_void_p(d_templates.data_ptr()), len(table.templates),
                                                      C.c_void_p(centres.data_ptr()), R, C.c_void_p(vr.data_ptr()),
                                                      C.c_void_p(count.data_ptr()), C.c_void_p(extent.data_ptr()),
                                                      _device.stream_ptr(dev))
    _abi.check(st, "slhip_object_regions_vertices")
    vr._keepalive = (d_pos, d_assets, d_templates, centres)      # the launch is asynchronous
    return vr, count, extent


class RegionBank:
    """centres float32 [A, R, 4] = (x, y, z, 1) per class in the object frame; vertex int32 [A, R], the mesh vertex of every
    centre; vertex_region uint8 [n_vertices], the region of every pool vertex (255: a vertex of no class); count int32 [A, R]
    and extent float32 [A, R, 4] = (max |dx|, max |dy|, max |dz|, max d2) of every region's vertices.  All but `centres` may be
    None (a bank built from a bare tensor)."""

    def __init__(self, centres, vertex=None, vertex_region=None, count=None, extent=None):
        self.centres, self.vertex, self.vertex_region, self.count, self.extent = centres, vertex, vertex_region, count, extent
        if centres.dim() != 3 or centres.shape[2] != 4:
            raise ValueError("RegionBank: centres must be [A, R, 4]")

    def __len__(self):
        return int(self.centres.shape[1])


def bank(table, n_regions=64):
    """The RegionBank of an sl.AssetTable: `n_regions` (1..255) FPS centres per class and the regions of the table's vertices,
    on the table's device."""
    cen, vertex = centres(table, n_regions)
    vr, count, extent = vertices(table, cen)
    return RegionBank(cen, vertex, vr, count, extent)


# ---- per pixel -----------------------------------------------------------------------------------------------------------------
class ObjectRegions:
    """The regions of every pixel of N pictures.  Tensors:
        region     uint8 [N, H, W]: the nearest centre of the pixel's object coordinate among the centres of its object's class,
                   255 (sl.object_regions.NONE) for background, an instance outside [1, O], a class outside the bank and a
                   coordinate that is not finite
        local      float32 [N, H, W, 4] = (x - cx, y - cy, z - cz, d2) against the winning centre, zeros where region is NONE
                   (None unless asked for)
        histogram  int32 [N, O, R]: the pixels of object o of picture n in region r (None unless asked for; the library's
                   uint32 counters in the integer type torch computes with)
        visible    bool [N, O, R] = histogram > 0: which regions of an object can be seen
    `params`: the slhip_object_region_params record."""

    def __init__(self, region, local=None, histogram=None, params=None):
        self.region, self.local, self.histogram, self.params = region, local, histogram, params
        self._keepalive = ()

    @property
    def visible(self):
        return None if self.histogram is None else self.histogram > 0

    def at(self, points):
        """The regions of the pixels of an ObjectPoints of the same pictures: uint8 [n, K] =
        region.view(N, -1)[points.scene, points.index].  Plain torch, on whatever device the tensors live."""
        if points.pixel is None:
            raise RuntimeError("at() needs the points' pixel output")
        flat = self.region.reshape(self.region.shape[0], -1)
        return flat[points.scene.long()[..., None], points.index]

    @staticmethod
    def of_crops(crops, classes, bank, local=False, histogram=False, n_objects=None):
        """The regions of the windows of an ObjectCrops (with its `instance` and `coord` outputs): window i is picture i, with
        the classes of its scene, classes[crops.scene].  `classes`: int32 [B, O] of the pictures the crops were cut from, or
        their slhip_synth_object records as a uint8 tensor (a chunk's slice of SceneBatch.d_objects, with n_objects=O).  The
        same kernel as label()."""
        if crops.instance is None or crops.coord is None:
            raise RuntimeError("of_crops needs the crops' instance and coord outputs")
        if isinstance(classes, torch.Tensor) and classes.dtype == torch.uint8 and n_objects:
            classes = _device.class_tensor(classes, n_objects)
        if not isinstance(classes, torch.Tensor) or classes.dtype != torch.int32 or classes.dim() != 2:
            raise ValueError("object_regions: of_crops takes the classes as an int32 [B, O] tensor (or uint8 records and n_objects)")
        return label(crops.instance, crops.coord, classes[crops.scene.long()].contiguous(), bank, local=local, histogram=histogram)


def label(instance, coord, classes, bank, local=False, histogram=False, n_objects=None):
    """The region of every pixel: an ObjectRegions.

    instance   int16 [N, H, W] or [N, H, W, 1] on the device (the instance target; instance i is object i - 1)
    coord      float32 [N, H, W, 4] (the coord target: object xyz; its w is not read)
    classes    int32 [N, O]: the class of every object, or the slhip_synth_object records of the N * O objects as a uint8 tensor
               (SceneBatch.d_objects, read in place; then `n_objects` = O).  A class outside [0, A) gives NONE.
    bank       a RegionBank or a float32 [A, R, 4] device tensor, R <= 255
    local, histogram   also write those outputs (16 bytes per pixel; 4 bytes per (picture, object, region))

    Asynchronous on the current stream."""
    cen = bank.centres if isinstance(bank, RegionBank) else bank
    dev = _device.require_cuda("object_regions", (instance, coord, cen), "instance, coord and the bank",
                               "instance, coord, classes and the bank must be torch tensors")
    if instance.dtype != torch.int16 or instance.dim() not in (3, 4) or (instance.dim() == 4 and instance.shape[3] != 1) \
            or not instance.is_contiguous():
        raise ValueError("object_regions: `instance` must be a contiguous int16 [N, H, W] tensor")
    N, H, W = (int(v) for v in instance.shape[:3])
    if coord.dtype != torch.float32 or tuple(coord.shape) != (N, H, W, 4) or not coord.is_contiguous():
        raise ValueError("object_regions: `coord` must be a contiguous float32 [%d, %d, %d, 4] tensor" % (N, H, W))
    if cen.dtype != torch.float32 or cen.dim() != 3 or cen.shape[2] != 4 or not cen.is_contiguous():
        raise ValueError("object_regions: the bank must be a contiguous float32 [A, R, 4] tensor")
    A, R = int(cen.shape[0]), int(cen.shape[1])
    keep, p_classes, stride, O = _device.object_classes("object_regions", classes, N, dev, n_objects)
    rec = check_params(make_params((W, H), N, O, R, A, local, histogram))
    region = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    loc = torch.empty((N, H, W, 4), dtype=torch.float32, device=dev) if local else None
    hist = torch.empty((N, O, R), dtype=torch.int32, device=dev) if histogram else None
    if N:
        with torch.cuda.device(dev):
            st = _abi.lib().slhip_object_regions_label(rec.ctypes.data, C.c_void_p(instance.data_ptr()), C.c_void_p(coord.data_ptr()),
                                                       C.c_void_p(p_classes), stride, C.c_void_p(cen.data_ptr()),
                                                       C.c_void_p(region.data_ptr()), C.c_void_p(loc.data_ptr() if local else None),
                                                       C.c_void_p(hist.data_ptr() if histogram else None), _device.stream_ptr(dev))
        _abi.check(st, "slhip_object_regions_label")
    out = ObjectRegions(region, loc, hist, rec[0].copy())
    out._keepalive = (instance, coord, keep, cen)      # the launch is asynchronous: its inputs live as long as its outputs
    return out
