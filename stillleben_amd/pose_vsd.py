"""Pose VSD -- this project's addition (the reference has no counterpart): BOP's Visible Surface Discrepancy of pose estimates
against a batch's ground truth, the third of BOP's pose errors beside MSSD and MSPD (sl.pose_error) and the only one that looks
at the picture.  The object is drawn as depth at the ground truth and at the estimate by a rasteriser whose two depth planes
never leave LDS; both are compared where either is visible in the scene's depth image.  Two entries of include/slhip.h:
slhip_pose_vsd and slhip_pose_depth (the raster alone, as dense planes: what render-and-compare refiners look at).  There is no
CPU path.

    surf = sl.pose_vsd.surface(table)                                    # once: a SurfaceBank
    batch.place(object_to_camera=True); buffers = batch.render(0)
    v = batch.pose_vsd(estimates, surf, buffers, chunk=0)                # estimates [B, O, Hy, 3, 4] or [B, O, 3, 4]
    v.vsd, v.counts, v.n_cost, v.flags; v.recall()                       # AR_VSD over BOP19's taus and thresholds

DESIGN.md "Pose VSD" states the rules operation by operation."""
import ctypes as C

import numpy as np
import torch

from . import _abi, _device
from . import pose_error as _pe

__all__ = ["OUTPUTS", "TAUS", "THRESHOLDS", "SurfaceBank", "PoseVSD", "make_params", "check_params", "surface", "evaluate",
           "evaluate_host", "render_depth", "render_depth_host", "band_pixels"]

NAME = "pose_vsd"
OUTPUTS = {"vsd": _abi.VSD_OUT_VSD, "counts": _abi.VSD_OUT_COUNTS, "n_cost": _abi.VSD_OUT_COST, "flags": _abi.VSD_OUT_FLAGS}
TAUS = tuple(0.05 * k for k in range(1, 11))            # BOP19: 0.05, 0.10, ..., 0.50 of the diameter
THRESHOLDS = tuple(0.05 * k for k in range(1, 11))      # BOP19: a pose is correct when vsd < theta
Z_NEAR = 1e-3


def output_mask(outputs):
    if isinstance(outputs, int):
        return outputs
    mask = 0
    for name in outputs:
        if name not in OUTPUTS:
            raise ValueError("outputs: unknown %r (known: %s)" % (name, ", ".join(OUTPUTS)))
        mask |= OUTPUTS[name]
    return mask


def make_params(intrinsics, size, n_objects, n_hypotheses, taus=TAUS, delta=0.015, normalized=True, z_near=Z_NEAR,
                outputs=("vsd", "counts", "n_cost", "flags")):
    """One slhip_pose_vsd_params record (numpy).  `intrinsics`: (fx, fy, cx, cy); `size`: (W, H); `outputs`: names or the mask."""
    p = np.zeros((), _abi.POSE_VSD_PARAMS_DTYPE)
    p["fx"], p["fy"], p["cx"], p["cy"] = (np.float32(v) for v in intrinsics)
    p["W"], p["H"] = int(size[0]), int(size[1])
    taus = np.asarray(taus, np.float32).reshape(-1)
    p["n_objects"], p["n_hypotheses"], p["n_taus"] = int(n_objects), int(n_hypotheses), len(taus)
    p["taus"][:min(len(taus), _abi.VSD_TAUS_MAX)] = taus[:_abi.VSD_TAUS_MAX]
    p["delta"], p["z_near"] = np.float32(delta), np.float32(z_near)
    p["flags"], p["outputs"] = _abi.VSD_NORMALIZED if normalized else 0, output_mask(outputs)
    return p


def check_params(params):
    """Raises SlhipError when the record breaks a rule of slhip_pose_vsd_check_params.  Needs no device."""
    rec = np.ascontiguousarray(np.asarray(params, dtype=_abi.POSE_VSD_PARAMS_DTYPE).reshape(1))
    _abi.check(_abi.lib().slhip_pose_vsd_check_params(rec.ctypes.data), "slhip_pose_vsd")
    return rec


def band_pixels():
    """The pixels one LDS band of the kernel holds."""
    return int(_abi.lib().slhip_pose_vsd_band_pixels())


# ---- the surface bank ------------------------------------------------------------------------------------------------------------
class SurfaceBank:
    """The triangles of every class, all tensors on one device:
        vertices   float32 [V, 4]  (x, y, z, 1) in the object frame (the frame of the `coord` target)
        triangles  int32 [N, 3]    absolute indices into vertices (uint32 in the library)
        tri_begin  int32 [A], tri_count int32 [A]   class a owns triangles [tri_begin[a], tri_begin[a] + tri_count[a])
        diameter   float32 [A] or None (then thresholds cannot be normalised)"""

    def __init__(self, vertices, triangles, tri_begin, tri_count, diameter=None):
        self.vertices, self.triangles, self.tri_begin, self.tri_count, self.diameter = vertices, triangles, tri_begin, tri_count, diameter
        if vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 4 or not vertices.is_contiguous() or not len(vertices):
            raise ValueError("SurfaceBank: vertices must be a contiguous float32 [V, 4] tensor, V >= 1")
        if triangles.dtype != torch.int32 or triangles.dim() != 2 or triangles.shape[1] != 3 or not triangles.is_contiguous() or not len(triangles):
            raise ValueError("SurfaceBank: triangles must be a contiguous int32 [N, 3] tensor, N >= 1")
        A = int(tri_begin.shape[0]) if tri_begin.dim() == 1 else -1
        for t, what in ((tri_begin, "tri_begin"), (tri_count, "tri_count")):
            if t.dtype != torch.int32 or tuple(t.shape) != (A,) or not t.is_contiguous() or A < 1:
                raise ValueError("SurfaceBank: %s must be a contiguous int32 [A] tensor" % what)
        if diameter is not None and (diameter.dtype != torch.float32 or tuple(diameter.shape) != (A,) or not diameter.is_contiguous()):
            raise ValueError("SurfaceBank: diameter must be a contiguous float32 [A] tensor")

    def __len__(self):
        return int(self.tri_begin.shape[0])

    def tensors(self):
        return (self.vertices, self.triangles, self.tri_begin, self.tri_count) + (() if self.diameter is None else (self.diameter,))

    def record(self):
        """the slhip_pose_surface record over the tensors' memory"""
        return _abi.PoseSurface(self.vertices.data_ptr(), self.triangles.data_ptr(), self.tri_begin.data_ptr(), self.tri_count.data_ptr(),
                                _device.ptr(self.diameter), len(self), int(self.vertices.shape[0]), int(self.triangles.shape[0]), 0)


def table_surface(positions, indices, records, templates):
    """positions float32 [V, 4] and indices (the pool's, any device), records / templates: the table's slhip_asset and slhip_draw
    records (numpy).  Returns (vertices, triangles, tri_begin, tri_count, per-class (first vertex, count)) on the positions'
    device: per class its n_verts vertices under mesh_to_object, rows ((m0 x + m1 y) + m2 z) + m3, and the n_tris triangles from
    idx_base of each of its draw_count templates, offset by the class's vertex base.  A class whose vertices or indices leave
    the pool has no triangles."""
    dev = positions.device
    indices = indices.reshape(-1)
    verts, tris, begin, count, spans = [], [], [], [], []
    n_v = n_t = 0
    for a in records:
        db, dc, V = int(a["draw_begin"]), int(a["draw_count"]), int(a["n_verts"])
        begin.append(n_t)
        ok = dc > 0 and V > 0 and db + dc <= len(templates)
        base = int(templates[db]["vtx_base"]) if ok else 0
        ok = ok and base + V <= positions.shape[0]
        ok = ok and all(int(t["idx_base"]) + 3 * int(t["n_tris"]) <= indices.numel() for t in templates[db:db + dc])
        if not ok:
            count.append(0)
            spans.append((n_v, 0))
            continue
        v = positions[base:base + V]
        m = torch.from_numpy(np.ascontiguousarray(a["mesh_to_object"], dtype=np.float32).reshape(4, 4)).to(dev)
        out = torch.ones((V, 4), dtype=torch.float32, device=dev)
        x, y, z = v[:, 0], v[:, 1], v[:, 2]
        for r in range(3):
            out[:, r] = ((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3]
        verts.append(out)
        n = 0
        for t in templates[db:db + dc]:
            ib, nt = int(t["idx_base"]), int(t["n_tris"])
            tris.append(indices[ib:ib + 3 * nt].to(torch.int64).reshape(-1, 3) + n_v)      # (indices are relative to the class's base)
            n += nt
        count.append(n)
        spans.append((n_v, V))
        n_v += V
        n_t += n
    vertices = torch.cat(verts) if verts else torch.ones((1, 4), dtype=torch.float32, device=dev)
    triangles = torch.cat(tris).to(torch.int32) if n_t else torch.zeros((1, 3), dtype=torch.int32, device=dev)
    as_t = lambda l: torch.tensor(l, dtype=torch.int32, device=dev)      # noqa: E731
    return vertices.contiguous(), triangles.contiguous(), as_t(begin), as_t(count), spans


def surface(table=None, vertices=None, triangles=None, tri_begin=None, tri_count=None, diameter=None, n_points=_abi.POSE_POINTS_MAX):
    """The SurfaceBank of an sl.AssetTable on its device, or of the caller's own tensors (`vertices`, `triangles`, `tri_begin`,
    `tri_count`; `table` may then be None).  diameter: None -- with a table, sl.pose_error.diameters over a point bank of the
    same vertices (sample_indices of at most `n_points` per class), else no diameter --, or [A] values (a dataset's
    models_info diameter, in the table's unit)."""
    spans = None
    if vertices is None:
        eng, d_pos, _, _ = _device.table_on_device(table)
        vertices, triangles, tri_begin, tri_count, spans = table_surface(d_pos.view(-1, 4), eng._pool_dev[4], table.records, table.templates)
    dev = vertices.device
    to32 = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()      # noqa: E731
    bank = SurfaceBank(vertices.contiguous(), to32(triangles), to32(tri_begin), to32(tri_count))
    if diameter is not None:
        bank.diameter = torch.as_tensor(np.asarray(diameter, np.float32).reshape(len(bank))).to(dev)
    elif spans is not None:
        picks = [first + _pe.sample_indices(n, n_points) for first, n in spans]
        N = max(1, max(len(p) for p in picks))
        points = torch.zeros((len(bank), N, 4), dtype=torch.float32, device=dev)
        for c, idx in enumerate(picks):
            if len(idx):
                points[c, :len(idx)] = vertices[torch.from_numpy(idx).to(dev)]
        count = torch.tensor([len(p) for p in picks], dtype=torch.int32, device=dev)
        bank.diameter = _pe.bank(None, points=points, count=count).diameter
    return bank


# ---- the errors ------------------------------------------------------------------------------------------------------------------
class PoseVSD:
    """The VSD of every (scene, object, hypothesis): float32 vsd [B, O, Hy, T], int32 counts [B, O, Hy, 4] (visib_gt, visib_est,
    inter, union), int32 n_cost [B, O, Hy, T], int32 flags [B, O, Hy] (bit 1: a triangle was clipped at z_near); without a
    hypothesis axis in, none out; those not asked for are None.  +inf and -1: a class without a surface; NaN and -1: a pose that
    is not finite.  `classes`: int32 [B, O]."""

    def __init__(self, classes, taus, vsd=None, counts=None, n_cost=None, flags=None):
        self.classes, self.taus = classes, tuple(float(t) for t in taus)
        self.vsd, self.counts, self.n_cost, self.flags = vsd, counts, n_cost, flags
        self._keepalive = ()

    def recall(self, thresholds=THRESHOLDS):
        """AR_VSD as BOP defines it: the mean over taus and thresholds of `vsd < theta`, over the finite entries.  Plain torch."""
        if self.vsd is None:
            raise RuntimeError("pose_vsd: the `vsd` output was not asked for")
        v = self.vsd
        thr = torch.as_tensor(thresholds, dtype=torch.float32, device=v.device).reshape(-1)
        finite = torch.isfinite(v)
        hit = (v[..., None] < thr) & finite[..., None]
        return hit.sum().float() / (finite.sum() * thr.numel()).clamp(min=1).float()


def _surface_record(vertices, triangles, tri_begin, tri_count, diameter=None):
    """(record, arrays kept alive) of host arrays"""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 4)
    t = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
    b, n = np.ascontiguousarray(tri_begin, np.uint32).reshape(-1), np.ascontiguousarray(tri_count, np.uint32).reshape(-1)
    d = None if diameter is None else np.ascontiguousarray(diameter, np.float32).reshape(-1)
    rec = _abi.PoseSurface(v.ctypes.data, t.ctypes.data, b.ctypes.data, n.ctypes.data, None if d is None else d.ctypes.data, len(b), len(v),
                           len(t), 0)
    return rec, (v, t, b, n, d)


def _poses_host(a, lead):
    a = np.ascontiguousarray(a, np.float32)
    if a.shape[:len(lead)] != tuple(lead) or a.shape[-2:] != (3, 4):
        raise ValueError("pose_vsd: poses of shape %r do not match %r" % (a.shape, tuple(lead)))
    return a


def evaluate_host(object_to_camera, estimates, classes, vertices, triangles, tri_begin, tri_count, depth, intrinsics, diameter=None,
                  taus=TAUS, delta=0.015, normalized=True, z_near=Z_NEAR, outputs=("vsd", "counts", "n_cost", "flags")):
    """slhip_pose_vsd_host on host arrays: a dict of the outputs asked for.  classes int32 [B, O]; object_to_camera [B, O, 3, 4];
    estimates [B, O, Hy, 3, 4]; depth [B, H, W] or [B, H, W, 4] (read at w).  Needs no device: the CPU tests' handle."""
    est = np.ascontiguousarray(estimates, np.float32)
    B, O, Hy = est.shape[:3]
    gt = _poses_host(object_to_camera, (B, O))
    cls = np.ascontiguousarray(classes, np.int32).reshape(B, O)
    depth = np.ascontiguousarray(depth, np.float32)
    stride = 4 if depth.ndim == 4 else 1
    H, W = depth.shape[1:3]
    rec, keep = _surface_record(vertices, triangles, tri_begin, tri_count, diameter)
    p = make_params(intrinsics, (W, H), O, Hy, taus, delta, normalized, z_near, outputs).reshape(1)
    T, mask = int(p["n_taus"][0]), int(p["outputs"][0])
    outs = {"vsd": np.zeros((B, O, Hy, T), np.float32), "counts": np.zeros((B, O, Hy, 4), np.int32),
            "n_cost": np.zeros((B, O, Hy, T), np.int32), "flags": np.zeros((B, O, Hy), np.uint32)}
    o = _abi.PoseVsdOut(*(outs[k].ctypes.data for k in ("vsd", "counts", "n_cost", "flags")))
    first = depth.ctypes.data + (12 if stride == 4 else 0)
    st = _abi.lib().slhip_pose_vsd_host(p.ctypes.data, C.byref(rec), cls.ctypes.data, 1, gt.ctypes.data, est.ctypes.data, first, stride,
                                        B, C.byref(o))
    _abi.check(st, "slhip_pose_vsd_host")
    return {k: v for k, v in outs.items() if mask & OUTPUTS[k]}


def render_depth_host(poses, classes, vertices, triangles, tri_begin, tri_count, intrinsics, size, z_near=Z_NEAR):
    """slhip_pose_depth_host on host arrays: (depth float32 [B, O, Hy, H, W], flags uint32 [B, O, Hy]).  Needs no device."""
    poses = np.ascontiguousarray(poses, np.float32)
    B, O, Hy = poses.shape[:3]
    cls = np.ascontiguousarray(classes, np.int32).reshape(B, O)
    rec, keep = _surface_record(vertices, triangles, tri_begin, tri_count)
    p = make_params(intrinsics, size, O, Hy, normalized=False, z_near=z_near).reshape(1)
    depth, flags = np.zeros((B, O, Hy, int(size[1]), int(size[0])), np.float32), np.zeros((B, O, Hy), np.uint32)
    st = _abi.lib().slhip_pose_depth_host(p.ctypes.data, C.byref(rec), cls.ctypes.data, 1, poses.ctypes.data, B, depth.ctypes.data,
                                          flags.ctypes.data)
    _abi.check(st, "slhip_pose_depth_host")
    return depth, flags


def _device_args(object_to_camera, poses, objects, surf, what):
    """the checks evaluate and render_depth share: (device, B, O, poses [B, O, Hy, 3, 4], squeeze, classes to keep, pointer, stride,
    int32 classes [B, O])"""
    if not isinstance(surf, SurfaceBank):
        raise TypeError("pose_vsd: `surface` must be a SurfaceBank (sl.pose_vsd.surface(table))")
    lead = (poses,) if object_to_camera is None else (object_to_camera, poses)
    dev = _device.require_cuda(NAME, lead + surf.tensors(), "the poses and the surface", "the poses must be torch tensors")
    squeeze = poses.dim() == 4
    if squeeze:
        poses = poses[:, :, None]
    if poses.dtype != torch.float32 or poses.dim() != 5 or tuple(poses.shape[3:]) != (3, 4) or not poses.is_contiguous():
        raise ValueError("pose_vsd: %s must be a contiguous float32 [B, O, Hy, 3, 4] (or [B, O, 3, 4]) tensor" % what)
    B, O = int(poses.shape[0]), int(poses.shape[1])
    o2c = object_to_camera
    if o2c is not None and (o2c.dtype != torch.float32 or tuple(o2c.shape) != (B, O, 3, 4) or not o2c.is_contiguous()):
        raise ValueError("pose_vsd: object_to_camera must be a contiguous float32 [%d, %d, 3, 4] tensor" % (B, O))
    if isinstance(objects, torch.Tensor) and objects.dtype in (torch.int16, torch.int64):
        objects = objects.to(torch.int32).contiguous()
    keep, p_classes, stride, O_ = _device.object_classes(NAME, objects, B, dev, O)
    if O_ != O:
        raise ValueError("pose_vsd: `objects` holds %d objects per scene, the poses %d" % (O_, O))
    classes = _device.class_tensor(keep, O)[:B] if keep.dtype == torch.uint8 else keep
    return dev, B, O, poses, squeeze, keep, p_classes, stride, classes


def evaluate(object_to_camera, estimates, objects, surface, depth, intrinsics, taus=TAUS, delta=0.015, normalized=True, z_near=Z_NEAR,
             outputs=("vsd", "counts", "n_cost", "flags")):
    """The VSD of pose estimates against the ground truth: a PoseVSD.

    object_to_camera  float32 [B, O, 3, 4] on the device (SceneBatch.place(object_to_camera=True))
    estimates         float32 [B, O, Hy, 3, 4], or [B, O, 3, 4] (one hypothesis; the outputs lose that axis again)
    objects           the slhip_synth_object records of the B * O objects as a uint8 device tensor, read in place, or the class of
                      every object as an integer tensor [B, O]
    surface           a SurfaceBank (sl.pose_vsd.surface(table))
    depth             float32 [B, H, W], or [B, H, W, 4] read at w (the `coord` target of a render: camera z, 3000 on the background)
    intrinsics        (fx, fy, cx, cy)
    taus, delta       the misalignment tolerances (fractions of the class's diameter when `normalized`) and the visibility
                      tolerance, in the table's unit
    outputs           names among "vsd", "counts", "n_cost", "flags"

    Asynchronous on the current stream."""
    dev, B, O, est, squeeze, keep, p_classes, stride, classes = _device_args(object_to_camera, estimates, objects, surface, "estimates")
    _device.require_cuda(NAME, (depth,), "the poses and the depth", "`depth` must be a torch tensor", dev)
    if (depth.dtype != torch.float32 or depth.dim() not in (3, 4) or depth.shape[0] != B or (depth.dim() == 4 and depth.shape[3] != 4)
            or not depth.is_contiguous()):
        raise ValueError("pose_vsd: depth must be a contiguous float32 [%d, H, W] or [%d, H, W, 4] tensor" % (B, B))
    if normalized and surface.diameter is None:
        raise ValueError("pose_vsd: normalised thresholds need a SurfaceBank with a diameter")
    d_stride = 4 if depth.dim() == 4 else 1
    Hy, H, W = int(est.shape[2]), int(depth.shape[1]), int(depth.shape[2])
    rec = check_params(make_params(intrinsics, (W, H), O, Hy, taus, delta, normalized, z_near, outputs))
    T, mask = int(rec["n_taus"][0]), int(rec["outputs"][0])

    def new(bit, shape):
        return torch.empty(shape, dtype=torch.float32 if bit == _abi.VSD_OUT_VSD else torch.int32, device=dev) if mask & bit else None

    res = PoseVSD(classes, rec["taus"][0][:T], new(_abi.VSD_OUT_VSD, (B, O, Hy, T)), new(_abi.VSD_OUT_COUNTS, (B, O, Hy, 4)),
                  new(_abi.VSD_OUT_COST, (B, O, Hy, T)), new(_abi.VSD_OUT_FLAGS, (B, O, Hy)))
    names = ("vsd", "counts", "n_cost", "flags")
    if B:
        out = _abi.PoseVsdOut(*(_device.ptr(getattr(res, k)) for k in names))
        srec = surface.record()
        with torch.cuda.device(dev):
            st = _abi.lib().slhip_pose_vsd(rec.ctypes.data, C.byref(srec), C.c_void_p(p_classes), stride, C.c_void_p(object_to_camera.data_ptr()),
                                           C.c_void_p(est.data_ptr()), C.c_void_p(depth.data_ptr() + (12 if d_stride == 4 else 0)), d_stride,
                                           B, C.byref(out), _device.stream_ptr(dev))
        _abi.check(st, "slhip_pose_vsd")
    if squeeze:
        for k in names:
            if getattr(res, k) is not None:
                setattr(res, k, getattr(res, k)[:, :, 0])
    res._keepalive = (object_to_camera, est, keep, depth) + surface.tensors()      # the launch is asynchronous
    return res


def render_depth(poses, objects, surface, intrinsics, size, z_near=Z_NEAR):
    """The depth of every pose's raster alone: (depth float32 [B, O, Hy, H, W], 0 where nothing is covered; flags int32
    [B, O, Hy]) -- without the hypothesis axis when `poses` [B, O, 3, 4] has none.  `size`: (W, H).  Asynchronous on the current
    stream."""
    dev, B, O, poses, squeeze, keep, p_classes, stride, classes = _device_args(None, poses, objects, surface, "poses")
    Hy, W, H = int(poses.shape[2]), int(size[0]), int(size[1])
    rec = check_params(make_params(intrinsics, (W, H), O, Hy, normalized=False, z_near=z_near))
    depth = torch.empty((B, O, Hy, H, W), dtype=torch.float32, device=dev)
    flags = torch.empty((B, O, Hy), dtype=torch.int32, device=dev)
    if B:
        srec = surface.record()
        with torch.cuda.device(dev):
            st = _abi.lib().slhip_pose_depth(rec.ctypes.data, C.byref(srec), C.c_void_p(p_classes), stride, C.c_void_p(poses.data_ptr()), B,
                                             C.c_void_p(depth.data_ptr()), C.c_void_p(flags.data_ptr()), _device.stream_ptr(dev))
        _abi.check(st, "slhip_pose_depth")
    depth._keepalive = (poses, keep) + surface.tensors()
    return (depth[:, :, 0], flags[:, :, 0]) if squeeze else (depth, flags)
