"""Object keypoints -- this project's addition (the reference has no counterpart): the targets of keypoint-voting pose networks.
`sl.object_points` gives those networks their input; this module gives them what they regress: per-point offsets to a fixed set
of 3D keypoints of the object's class and to its centre (PVN3D, FFB6D) and per-pixel vectors towards the projected keypoints
(PVNet and its successors).  Everything stays on the device, through three entries of include/slhip.h:
slhip_object_keypoints_fps (farthest point sampling on the mesh pool, once per asset table), slhip_object_keypoints_project
(camera points, pixel positions and visibility flags per scene and object) and slhip_object_keypoints_field (the per-pixel
field, a pure write stream).  There is no CPU path.

    bank = sl.object_keypoints.bank(table, n_fps=8)                      # once: [A, 9, 4], the centre and 8 FPS points
    batch.place(object_to_camera=True)
    buffers = batch.render(0, object_masks=True)
    kps = batch.keypoints(buffers, bank=bank)                            # or sl.object_keypoints.project(...)
    kps.camera, kps.uv, kps.flags, kps.inside, kps.unoccluded
    field = kps.field(buffers.instance, mode="unit", scenes=(0, 8))      # [8, H, W, Kp, 2]: 19.7 MB per 640 x 480 image at Kp = 8
    offsets = kps.offsets(batch.points(buffers, n_points=1024))          # [n, K, Kp, 3]

DESIGN.md "Object keypoints" states the rules operation by operation."""
import ctypes as C

import numpy as np
import torch

from . import _abi, _device

__all__ = ["MODES", "KeypointBank", "ObjectKeypoints", "make_params", "check_params", "fps", "bank", "project"]

MODES = {"offset": _abi.KEYPOINT_FIELD_OFFSET, "unit": _abi.KEYPOINT_FIELD_UNIT}


def make_params(intrinsics, size, n_keypoints, n_objects, depth_tol=0.005, mode="unit"):
    """One slhip_object_keypoint_params record (numpy).  `intrinsics`: (fx, fy, cx, cy) the picture was rendered with; `size`:
    (W, H); `mode`: "offset", "unit" or the number."""
    if isinstance(mode, str):
        if mode not in MODES:
            raise ValueError("mode: unknown %r (known: %s)" % (mode, ", ".join(MODES)))
        mode = MODES[mode]
    p = np.zeros((), _abi.OBJECT_KEYPOINT_PARAMS_DTYPE)
    p["fx"], p["fy"], p["cx"], p["cy"] = (np.float32(v) for v in intrinsics)
    p["W"], p["H"] = int(size[0]), int(size[1])
    p["depth_tol"] = np.float32(depth_tol)
    p["n_keypoints"], p["n_objects"], p["mode"] = int(n_keypoints), int(n_objects), int(mode)
    return p


def check_params(params):
    """Raises SlhipError when the record breaks a rule of slhip_object_keypoints_check_params.  Needs no device."""
    rec = np.ascontiguousarray(np.asarray(params, dtype=_abi.OBJECT_KEYPOINT_PARAMS_DTYPE).reshape(1))
    _abi.check(_abi.lib().slhip_object_keypoints_check_params(rec.ctypes.data), "slhip_object_keypoints")
    return rec


def fps_host(positions, assets, templates, n):
    """slhip_object_keypoints_fps_host: the FPS rule on host arrays (positions float32 [V, 4], slhip_asset and slhip_draw
    records).  Returns (keypoints float32 [A, n, 4], vertex int32 [A, n]).  Needs no device: the CPU tests' handle."""
    return _device.fps_host(positions, assets, templates, n, "slhip_object_keypoints_fps_host")


def fps(table, n):
    """Farthest point sampling of every class of an sl.AssetTable on the device: (keypoints float32 [A, n, 4] = (x, y, z, 1) in
    the object frame -- the frame of the `coord` target --, vertex int32 [A, n], the mesh vertex each one is).  The first point
    is the vertex farthest from the bbox centre; ties go to the lowest vertex index.  Asynchronous on the current stream."""
    return _device.fps(table, n, "slhip_object_keypoints_fps", "slhip_object_keypoints_fps_bytes")


class KeypointBank:
    """points float32 [A, Kp, 4] = (x, y, z, 1) per class in the object frame; names: Kp strings ("center", "fps0", ...,
    "corner0", ...); vertex int32 [A, n_fps], the mesh vertices of the FPS points (None without them)."""

    def __init__(self, points, names, vertex=None):
        self.points, self.names, self.vertex = points, tuple(names), vertex
        if points.dim() != 3 or points.shape[2] != 4 or points.shape[1] != len(self.names):
            raise ValueError("KeypointBank: points must be [A, Kp, 4] with one name per keypoint")

    def __len__(self):
        return int(self.points.shape[1])

    def index(self, name):
        return self.names.index(name)


def assemble_bank(records, fps_points, center=True, corners=False, vertex=None):
    """The bank layout in torch: the optional bbox centre o, the FPS points, the optional eight bbox corners (corner c takes
    x from bbox_max when c & 1, y when c & 2, z when c & 4).  `records`: the table's slhip_asset records (numpy); `fps_points`:
    [A, n, 4] on any device, or None."""
    dev = fps_points.device if fps_points is not None else torch.device("cpu")
    lo = torch.from_numpy(np.ascontiguousarray(records["bbox_min"][:, :3], dtype=np.float32)).to(dev)
    hi = torch.from_numpy(np.ascontiguousarray(records["bbox_max"][:, :3], dtype=np.float32)).to(dev)
    one = torch.ones((len(records), 1, 1), dtype=torch.float32, device=dev)
    parts, names = [], []
    if center:
        parts.append(torch.cat([((lo + hi) * 0.5)[:, None], one], dim=2))
        names.append("center")
    if fps_points is not None and fps_points.shape[1]:
        parts.append(fps_points)
        names += ["fps%d" % i for i in range(fps_points.shape[1])]
    if corners:
        pick = torch.tensor([[(c >> a) & 1 for a in range(3)] for c in range(8)], dtype=torch.bool, device=dev)
        xyz = torch.where(pick[None], hi[:, None], lo[:, None])
        parts.append(torch.cat([xyz, one.expand(-1, 8, -1)], dim=2))
        names += ["corner%d" % c for c in range(8)]
    if not parts:
        raise ValueError("a keypoint bank needs at least one keypoint")
    points = torch.cat(parts, dim=1).contiguous()
    if points.shape[1] > _abi.KEYPOINTS_MAX:
        raise ValueError("a keypoint bank holds at most %d keypoints per class, not %d" % (_abi.KEYPOINTS_MAX, points.shape[1]))
    return KeypointBank(points, names, vertex)


def bank(table, n_fps=8, center=True, corners=False):
    """A KeypointBank of an sl.AssetTable: [centre] + n_fps FPS points + [8 bbox corners] per class, on the table's device."""
    pts, vertex = fps(table, n_fps) if n_fps else (None, None)
    if pts is None:
        pts = torch.empty((len(table), 0, 4), dtype=torch.float32, device=table.eng.device)
    return assemble_bank(table.records, pts, center, corners, vertex)


def _offsets(camera, points, scene0=0):
    """camera [B, O, Kp, 4]; the ObjectPoints' scene_global (or scene), slot, camera [n, K, 4] and valid -> [n, K, Kp, 3]"""
    if points.camera is None:
        raise RuntimeError("offsets needs the points' camera output")
    scene = points.scene_global - scene0 if points.scene_global is not None else points.scene
    kp = camera[scene.long(), (points.slot - 1).long()][..., :3]                 # [n, Kp, 3]
    out = kp[:, None] - points.camera[..., None, :3]                             # [n, K, Kp, 3]
    return torch.where(points.valid[..., None, None], out, torch.zeros((), dtype=out.dtype, device=out.device))


class ObjectKeypoints:
    """The keypoints of every (scene, object) of a picture.  Tensors:
        camera  float32 [B, O, Kp, 4] (X, Y, Z, 1) in the renderer's camera frame, zeros when not in front
        uv      float32 [B, O, Kp, 2] pixel position (pixel index x covers [x, x + 1)), zeros when not in front
        flags   uint8 [B, O, Kp]: 1 in front, 2 inside the picture, 4 unoccluded (only with a depth plane)
    and in_front, inside, unoccluded: bool views of the flags.  `params`: the slhip_object_keypoint_params record.  `scene0`: the
    batch's scene that scene 0 is (SceneBatch.keypoints of a later render chunk)."""

    def __init__(self, camera, uv, flags, params, names=None, scene0=0):
        self.camera, self.uv, self.flags, self.params, self.names, self.scene0 = camera, uv, flags, params, names, int(scene0)
        self._keepalive = ()

    @property
    def in_front(self):
        return (self.flags & _abi.KEYPOINT_IN_FRONT) != 0

    @property
    def inside(self):
        return (self.flags & _abi.KEYPOINT_INSIDE) != 0

    @property
    def unoccluded(self):
        return (self.flags & _abi.KEYPOINT_UNOCCLUDED) != 0

    def field(self, instance, mode="unit", scenes=None, out=None):
        """The per-pixel vector field float32 [count, H, W, Kp, 2] of scenes (first, count) -- default: all -- of `instance`
        (int16 [B, H, W] or [B, H, W, 1], the instance target the keypoints' picture was rendered with; instance i is object
        i - 1).  mode "offset": keypoint minus pixel centre, in pixels; "unit": that vector normalised ((0, 0) where it is
        zero).  Keypoints not in front and pixels of no object give zeros.  One 640 x 480 image at Kp = 8 is 19.7 MB: take
        slices of a render chunk.  `out`: a contiguous tensor of that shape to write into.  Asynchronous on the current stream."""
        B, O, Kp = (int(v) for v in self.flags.shape)
        W, H = int(self.params["W"]), int(self.params["H"])
        if not isinstance(instance, torch.Tensor) or instance.dtype != torch.int16:
            raise ValueError("object_keypoints: `instance` must be an int16 tensor")
        dev = _device.require_cuda("object_keypoints", (self.uv, instance), "instance and keypoints")
        if tuple(instance.shape) not in ((B, H, W), (B, H, W, 1)) or not instance.is_contiguous():
            raise ValueError("object_keypoints: `instance` must be a contiguous [%d, %d, %d] tensor" % (B, H, W))
        first, count = (0, B) if scenes is None else (int(scenes[0]), int(scenes[1]))
        if first < 0 or count < 0 or first + count > B:
            raise ValueError("object_keypoints: scenes (%d, %d) reach outside the %d scenes" % (first, count, B))
        if isinstance(mode, str):
            if mode not in MODES:
                raise ValueError("mode: unknown %r (known: %s)" % (mode, ", ".join(MODES)))
            mode = MODES[mode]
        p = np.array(self.params)
        p["mode"] = int(mode)
        rec = check_params(p)
        if out is None:
            out = torch.empty((count, H, W, Kp, 2), dtype=torch.float32, device=dev)
        elif out.dtype != torch.float32 or tuple(out.shape) != (count, H, W, Kp, 2) or not out.is_contiguous() or out.device != dev:
            raise ValueError("object_keypoints: `out` must be a contiguous float32 [%d, %d, %d, %d, 2] tensor on %s" % (count, H, W, Kp, dev))
        with torch.cuda.device(dev):
            st = _abi.lib().slhip_object_keypoints_field(rec.ctypes.data, C.c_void_p(instance.data_ptr()), C.c_void_p(self.uv.data_ptr()),
                                                         C.c_void_p(self.flags.data_ptr()), B, first, count, C.c_void_p(out.data_ptr()),
                                                         _device.stream_ptr(dev))
        _abi.check(st, "slhip_object_keypoints_field")
        out._keepalive = (instance, self.uv, self.flags)      # the launch is asynchronous: its inputs live as long as its output
        return out

    def offsets(self, points):
        """The PVN3D / FFB6D targets of an ObjectPoints of the same picture: float32 [n, K, Kp, 3] =
        camera[points.scene_global - scene0, points.slot - 1][:, None] - points.camera[..., None, :3], zeros where
        points.valid is false.  Plain torch, on whatever device the tensors live."""
        return _offsets(self.camera, points, self.scene0)


def project(object_to_camera, objects, bank, intrinsics, size, depth=None, depth_tol=0.005):
    """Projects the bank's keypoints of every object of every scene: an ObjectKeypoints.

    object_to_camera  float32 [B, O, 3, 4] on the device (SceneBatch.place(object_to_camera=True))
    objects           the slhip_synth_object records of the B * O objects as a uint8 device tensor (SceneBatch.d_objects), or
                      the class of every object as an integer tensor [B, O]; a class outside the bank gives zeros
    bank              a KeypointBank or a float32 [A, Kp, 4] device tensor (any points, not only FPS), Kp <= 32
    intrinsics, size  (fx, fy, cx, cy) and (W, H) the picture was rendered with
    depth             float32 [B, H, W] (a plane such as sl.depth_sensor's float output) or [B, H, W, 4] (the coord target:
                      its w is read in place): enables the `unoccluded` flag
    depth_tol         metres a keypoint may lie behind the plane and still count as unoccluded, finite and >= 0.  The
                      default of 0.005 is a convenience, not a measured value: choose it for the meshes and the depth at hand
                      (surface keypoints of a rendered object lie ON the plane up to float32 rounding and the pixel's slope).

    Asynchronous on the current stream."""
    names = bank.names if isinstance(bank, KeypointBank) else None
    pts = bank.points if isinstance(bank, KeypointBank) else bank
    o2c = object_to_camera
    dev = _device.require_cuda("object_keypoints", (o2c, pts, objects) + (() if depth is None else (depth,)),
                               "object_to_camera, objects, bank and depth",
                               "object_to_camera, objects, bank and depth must be torch tensors")
    if o2c.dtype != torch.float32 or o2c.dim() != 4 or tuple(o2c.shape[2:]) != (3, 4) or not o2c.is_contiguous():
        raise ValueError("object_keypoints: object_to_camera must be a contiguous float32 [B, O, 3, 4] tensor")
    B, O = int(o2c.shape[0]), int(o2c.shape[1])
    if pts.dtype != torch.float32 or pts.dim() != 3 or pts.shape[2] != 4 or not pts.is_contiguous():
        raise ValueError("object_keypoints: the bank must be a contiguous float32 [A, Kp, 4] tensor")
    A, Kp = int(pts.shape[0]), int(pts.shape[1])
    if objects.dtype == torch.uint8:
        if objects.numel() < B * O * _abi.SYNTH_OBJECT_DTYPE.itemsize or not objects.is_contiguous():
            raise ValueError("object_keypoints: the object records must hold %d x %d slhip_synth_object" % (B, O))
        d_objects = objects
    else:
        if tuple(objects.shape) != (B, O) or objects.dtype not in (torch.int16, torch.int32, torch.int64):
            raise ValueError("object_keypoints: asset ids must be an integer [%d, %d] tensor" % (B, O))
        d_objects = torch.zeros((B, O, 4), dtype=torch.int32, device=o2c.device)
        d_objects[..., 0] = objects.to(torch.int32)
    rec = check_params(make_params(intrinsics, size, Kp, O, depth_tol, "unit"))
    W, H = int(size[0]), int(size[1])
    d_depth, stride = None, 0
    if depth is not None:
        if depth.dtype != torch.float32 or tuple(depth.shape) not in ((B, H, W), (B, H, W, 4)) or not depth.is_contiguous():
            raise ValueError("object_keypoints: `depth` must be a contiguous float32 [%d, %d, %d] plane or [.., 4] coord target" % (B, H, W))
        d_depth, stride = (depth.data_ptr(), 1) if depth.dim() == 3 else (depth.data_ptr() + 12, 4)
    camera = torch.empty((B, O, Kp, 4), dtype=torch.float32, device=dev)
    uv = torch.empty((B, O, Kp, 2), dtype=torch.float32, device=dev)
    flags = torch.empty((B, O, Kp), dtype=torch.uint8, device=dev)
    if B:
        with torch.cuda.device(dev):
            st = _abi.lib().slhip_object_keypoints_project(rec.ctypes.data, C.c_void_p(pts.data_ptr()), A, C.c_void_p(d_objects.data_ptr()),
                                                           C.c_void_p(o2c.data_ptr()), B, C.c_void_p(d_depth), stride,
                                                           C.c_void_p(camera.data_ptr()), C.c_void_p(uv.data_ptr()),
                                                           C.c_void_p(flags.data_ptr()), _device.stream_ptr(dev))
        _abi.check(st, "slhip_object_keypoints_project")
    out = ObjectKeypoints(camera, uv, flags, rec[0].copy(), names)
    out._keepalive = (o2c, d_objects, pts, depth)      # the projection is asynchronous: its inputs live as long as its outputs
    return out
