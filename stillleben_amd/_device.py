"""What the per-object outputs (object_crops, object_points, object_keypoints, object_regions) share on their way into the
library: the checks of device tensors, pointers, scratch, the asset table's device arrays, the slhip_synth_object decode and the
farthest point sampling behind the keypoint and region banks.  `name` is the calling module's name in every message."""
import ctypes as C

import numpy as np
import torch

from . import _abi


def no_cpu(name):
    return "%s runs on the HIP device: pass cuda tensors (there is no CPU path)" % name


def require_cuda(name, tensors, what, tensor_text=None, device=None):
    """Every one of `tensors`, in turn: is a torch tensor (checked when `tensor_text` gives the ValueError's wording), lives on
    the HIP device (SlhipError), and on `device` -- default: the first one's (ValueError naming `what`).  Returns the device."""
    for t in tensors:
        if tensor_text is not None and not isinstance(t, torch.Tensor):
            raise ValueError("%s: %s" % (name, tensor_text))
        if not t.is_cuda:
            raise _abi.SlhipError(no_cpu(name))
        device = t.device if device is None else device
        if t.device != device:
            raise ValueError("%s: %s are on different devices" % (name, what))
    return device


def stream_ptr(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def ptr(t):
    return t.data_ptr() if t is not None else None


def scratch(nbytes, dev):
    return torch.empty(max(16, int(nbytes)), dtype=torch.uint8, device=dev)


def scratch_for(entry, dev, *args):
    """The scratch tensor sized by the library's `entry` (a *_bytes function: args..., uint64* out)."""
    nbytes = C.c_uint64(0)
    _abi.check(getattr(_abi.lib(), entry)(*args, C.byref(nbytes)), entry)
    return scratch(nbytes.value, dev)


def table_on_device(table):
    """(engine, pool positions, slhip_asset records, slhip_draw templates) of an sl.AssetTable, the last three on the device"""
    eng = table.eng
    if eng is None:
        raise _abi.SlhipError("this AssetTable was built on host pools (test helper); build it without them to use the device")
    d_assets, d_templates = table.device()
    eng.pool_abi()
    return eng, eng._pool_dev[0], d_assets, d_templates


def host_table(positions, assets, templates):
    pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 4)
    assets = np.ascontiguousarray(assets, dtype=_abi.ASSET_DTYPE).reshape(-1)
    templates = np.ascontiguousarray(templates, dtype=_abi.DRAW_DTYPE).reshape(-1)
    return pos, assets, templates


def class_tensor(records, n_objects):
    """int32 [B, O]: the classes (.asset, the first word) of slhip_synth_object records held in a uint8 tensor"""
    O, size = int(n_objects), _abi.SYNTH_OBJECT_DTYPE.itemsize
    whole = records.numel() // (O * size) * O * size
    return records[:whole].view(torch.int32).view(-1, O, size // 4)[..., 0]


def object_classes(name, classes, N, dev, n_objects):
    """(tensor to keep, int32 pointer, stride in int32 units, O) of the classes of N x O objects: an int32 [N, O] tensor, or
    their slhip_synth_object records as a uint8 tensor, read in place (then `n_objects` = O)"""
    require_cuda(name, (classes,), "instance and classes", "`classes` must be a torch tensor", dev)
    if classes.dtype == torch.uint8:      # slhip_synth_object records: .asset is their first word
        size = _abi.SYNTH_OBJECT_DTYPE.itemsize
        if n_objects is None or int(n_objects) < 1:
            raise ValueError("%s: object records need n_objects" % name)
        O = int(n_objects)
        if classes.dim() != 1 or classes.numel() < N * O * size or not classes.is_contiguous() or classes.data_ptr() % 4:
            raise ValueError("%s: the object records must hold %d x %d slhip_synth_object" % (name, N, O))
        return classes, classes.data_ptr(), size // 4, O
    if classes.dtype != torch.int32 or classes.dim() != 2 or classes.shape[0] != N or not classes.is_contiguous():
        raise ValueError("%s: `classes` must be a contiguous int32 [%d, O] tensor (or uint8 object records)" % (name, N))
    return classes, classes.data_ptr(), 1, int(classes.shape[1])


# ---- farthest point sampling: sl.object_keypoints.fps / fps_host, sl.object_regions.centres / centres_host -----------------------
def fps_host(positions, assets, templates, n, entry):
    """`entry` (slhip_object_keypoints_fps_host, slhip_object_regions_centres_host) on host arrays: (points float32 [A, n, 4],
    vertex int32 [A, n])"""
    pos, assets, templates = host_table(positions, assets, templates)
    A = len(assets)
    points, vertex = np.zeros((A, max(int(n), 0), 4), np.float32), np.zeros((A, max(int(n), 0)), np.int32)
    st = getattr(_abi.lib(), entry)(pos.ctypes.data if len(pos) else None, len(pos), assets.ctypes.data, A,
                                    templates.ctypes.data if len(templates) else None, len(templates), int(n),
                                    points.ctypes.data, vertex.ctypes.data)
    _abi.check(st, entry)
    return points, vertex


def fps(table, n, entry, bytes_entry):
    """`entry` (slhip_object_keypoints_fps, slhip_object_regions_centres) on the device arrays of an sl.AssetTable, with the
    scratch that `bytes_entry` sizes: (points float32 [A, n, 4], vertex int32 [A, n]).  Asynchronous on the current stream."""
    eng, d_pos, d_assets, d_templates = table_on_device(table)
    A, dev = len(table), eng.device
    max_verts = int(table.records["n_verts"].max(initial=0))
    work = scratch_for(bytes_entry, dev, A, max_verts)
    points = torch.empty((A, max(int(n), 0), 4), dtype=torch.float32, device=dev)
    vertex = torch.empty((A, max(int(n), 0)), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        st = getattr(_abi.lib(), entry)(C.c_void_p(d_pos.data_ptr()), int(eng.pool.n_vertices), C.c_void_p(d_assets.data_ptr()), A,
                                        C.c_void_p(d_templates.data_ptr()), len(table.templates), int(n), max_verts,
                                        C.c_void_p(work.data_ptr()), C.c_void_p(points.data_ptr()), C.c_void_p(vertex.data_ptr()),
                                        stream_ptr(dev))
    _abi.check(st, entry)
    points._keepalive = (d_pos, d_assets, d_templates, work)      # the launch is asynchronous
    return points, vertex
