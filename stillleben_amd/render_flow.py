"""Render flow -- this project's addition (the reference has no counterpart): where every pixel of one render lands in another
render of the same scene.  Optical flow, scene flow and an occlusion flag per pixel and the co-visibility per instance slot: the
targets of flow networks (RAFT and its kin) and of flow-based 6D refiners (Coupled Iterative Refinement, SCFlow, PFA, GenFlow,
DeepIM's auxiliary flow head), from exact geometry and exact motion.  Everything stays on the device, through two entries of
include/slhip.h: slhip_render_flow (one lane per pixel) and slhip_render_flow_motion (the rigid motion of a frame between two
pictures).  There is no CPU path; `compute_host` and `motion_host` run the library's host twins of the same rules.

    batch.place(view=0, object_to_camera=True)
    a, state_a = batch.render(0), batch.view_state()
    batch.place(view=1, object_to_camera=True)                           # another camera -- or settle() further, same camera
    b = batch.render(0)
    f = batch.flow(a, state_a, b, outputs=("flow", "flags", "counts"))   # a -> b; state_b=None: the view now placed
    f.flow, f.flags, f.valid, f.inside, f.visible, f.occluded, f.covisibility()

DESIGN.md "Render flow" states the rules operation by operation."""
import ctypes as C

import numpy as np
import torch

from . import _abi, _device, _record_set

__all__ = ["OUTPUTS", "RenderFlow", "ViewState", "make_params", "check_params", "motion", "motion_host", "compute", "compute_host"]

NAME = "render_flow"
OUTPUTS = {"flow": _abi.FLOW_OUT_FLOW, "scene_flow": _abi.FLOW_OUT_SCENE, "flags": _abi.FLOW_OUT_FLAGS, "counts": _abi.FLOW_OUT_COUNTS}
# convenience defaults, NOT measured values: a moved surface point lies ON picture b's surface up to float32 rounding and the
# slope of the surface across the footprint's pixels; choose both for the meshes, the depth and the baseline at hand
DEPTH_TOL, DEPTH_REL = 0.005, 0.01


def make_params(intrinsics, size, n_slots, max_depth=3000.0, depth_tol=DEPTH_TOL, depth_rel=DEPTH_REL, match_instance=True,
                outputs=("flow", "flags")):
    """One slhip_render_flow_params record (numpy).  `intrinsics`: (fx, fy, cx, cy) both pictures were rendered with; `size`:
    (W, H); `max_depth`: the renderer writes 3000 where nothing was hit, so 3000 drops the background and keeps the plane;
    `depth_tol` + `depth_rel` * Z': how far behind picture b's surface a moved point still counts as visible (the defaults are
    conveniences, not measured values); `outputs`: names or the bit mask."""
    p = np.zeros((), _abi.RENDER_FLOW_PARAMS_DTYPE)
    p["fx"], p["fy"], p["cx"], p["cy"] = (np.float32(v) for v in intrinsics)
    p["W"], p["H"], p["n_slots"] = int(size[0]), int(size[1]), int(n_slots)
    p["max_depth"], p["depth_tol"], p["depth_rel"] = np.float32(max_depth), np.float32(depth_tol), np.float32(depth_rel)
    p["outputs"] = outputs if isinstance(outputs, int) else _record_set.output_bits(outputs, OUTPUTS)
    p["flags"] = _abi.FLOW_MATCH_INSTANCE if match_instance else 0
    return p


def check_params(params):
    """Raises SlhipError when the record breaks a rule of slhip_render_flow_check_params.  Needs no device."""
    rec = np.ascontiguousarray(np.asarray(params, dtype=_abi.RENDER_FLOW_PARAMS_DTYPE).reshape(1))
    _abi.check(_abi.lib().slhip_render_flow_check_params(rec.ctypes.data), "slhip_render_flow")
    return rec


class ViewState:
    """What SceneBatch.flow needs of a view once the next one is placed (SceneBatch.view_state()): clones of
    object_to_camera float32 [n_scenes, O, 3, 4] and of rows 0-2 of every scene's world_to_cam, float32 [n_scenes, 3, 4]."""

    def __init__(self, object_to_camera, world_to_cam, view=0):
        self.object_to_camera, self.world_to_cam, self.view = object_to_camera, world_to_cam, int(view)


class RenderFlow:
    """The flow of every pixel of picture a (torch tensors on the device from `compute`, numpy arrays from `compute_host`; those
    not asked for are None):
        flow        float32 [B, H, W, 2] pixels: where the pixel's surface point lands in picture b minus the pixel's centre
        scene_flow  float32 [B, H, W, 3] the point in camera frame b minus the point in camera frame a, the unit of the depth
        flags       uint8 [B, H, W]: 1 valid, 2 inside picture b, 4 visible in picture b (only with a depth of b)
        counts      int32 [B, n_slots, 4]: per instance slot its pixels in a, of those the valid, the inside, the visible ones
    A pixel that is not valid has zeros and flags 0.  valid, inside, visible, occluded (= inside and not visible): bool views of
    the flags.  `params`: the slhip_render_flow_params record."""

    def __init__(self, flow=None, scene_flow=None, flags=None, counts=None, params=None):
        self.flow, self.scene_flow, self.flags, self.counts, self.params = flow, scene_flow, flags, counts, params
        self.scene0 = 0      # the batch's scene that scene 0 is (SceneBatch.flow of a later render chunk)
        self._keepalive = ()

    def _bit(self, bit):
        if self.flags is None:
            raise RuntimeError("render_flow: the `flags` output was not asked for")
        return (self.flags & bit) != 0

    @property
    def valid(self):
        return self._bit(_abi.FLOW_VALID)

    @property
    def inside(self):
        return self._bit(_abi.FLOW_INSIDE)

    @property
    def visible(self):
        return self._bit(_abi.FLOW_VISIBLE)

    @property
    def occluded(self):
        return self.inside & ~self.visible

    def covisibility(self):
        """visible / valid per slot, float32 [B, n_slots], NaN where a slot has no valid pixel."""
        if self.counts is None:
            raise RuntimeError("render_flow: the `counts` output was not asked for")
        c = self.counts
        if isinstance(c, np.ndarray):
            with np.errstate(invalid="ignore", divide="ignore"):
                return (c[..., 3].astype(np.float32) / c[..., 1].astype(np.float32)).astype(np.float32)
        return c[..., 3].float() / c[..., 1].float()      # 0 / 0 = NaN; visible <= valid, so never x / 0 with x > 0


def _frames(name, t):
    """rows 0-2 of [..., 3, 4] or [..., 4, 4] as a contiguous [n, 3, 4] and the leading shape"""
    if t.dtype != torch.float32 or t.dim() < 2 or tuple(t.shape[-2:]) not in ((3, 4), (4, 4)):
        raise ValueError("render_flow: `%s` must be a float32 [..., 3, 4] or [..., 4, 4] tensor" % name)
    return t[..., :3, :].reshape(-1, 3, 4).contiguous(), tuple(t.shape[:-2])


def motion(from_, to):
    """The motion of rigid frames between two pictures: to o inv_rigid(from_), float32 [..., 3, 4] on the device.  from_, to:
    float32 [..., 3, 4] or [..., 4, 4] device tensors of the same leading shape (rows 0-2 taken): a frame's pose in camera a
    and in camera b -- object_to_camera of two views for an object, world_to_cam of two views for the plane and the
    background.  Rigid inputs are assumed, not checked; a frame with a non-finite entry gives NaNs.  Asynchronous on the
    current stream."""
    dev = _device.require_cuda(NAME, (from_, to), "from_ and to", "from_ and to must be torch tensors")
    f, lead = _frames("from_", from_)
    t, lead_t = _frames("to", to)
    if lead != lead_t:
        raise ValueError("render_flow: from_ %s and to %s differ in their leading shape" % (lead, lead_t))
    out = torch.empty_like(f)
    if f.shape[0]:
        with torch.cuda.device(dev):
            st = _abi.lib().slhip_render_flow_motion(C.c_void_p(f.data_ptr()), C.c_void_p(t.data_ptr()), int(f.shape[0]),
                                                     C.c_void_p(out.data_ptr()), _device.stream_ptr(dev))
        _abi.check(st, "slhip_render_flow_motion")
    out = out.view(lead + (3, 4))
    out._keepalive = (f, t)      # the launch is asynchronous: its inputs live as long as its output
    return out


def motion_host(from_, to):
    """slhip_render_flow_motion_host on host arrays [..., 3, 4] or [..., 4, 4]: float32 [..., 3, 4].  Needs no device."""
    f = np.ascontiguousarray(np.asarray(from_, np.float32)[..., :3, :])
    t = np.ascontiguousarray(np.asarray(to, np.float32)[..., :3, :])
    if f.shape != t.shape or f.shape[-1] != 4:
        raise ValueError("render_flow: from_ and to must both be [..., 3, 4] or [..., 4, 4]")
    out = np.zeros(f.shape, np.float32)
    n = f.size // 12
    if n:
        _abi.check(_abi.lib().slhip_render_flow_motion_host(f.ctypes.data, t.ctypes.data, n, out.ctypes.data),
                   "slhip_render_flow_motion_host")
    return out


def _empty(shape_of, bits, make):
    return {name: make(*shape_of[name]) if bits & bit else None for name, bit in OUTPUTS.items()}


def _shapes(B, H, W, S):
    return {"flow": ((B, H, W, 2), "float32"), "scene_flow": ((B, H, W, 3), "float32"), "flags": ((B, H, W), "uint8"),
            "counts": ((B, S, 4), "int32")}


def compute_host(depth_a, instance_a, motion, intrinsics, depth_b=None, instance_b=None, **kw):
    """slhip_render_flow_host on host arrays: a RenderFlow of numpy arrays.  The arguments of `compute`, as numpy arrays
    (instances int16 or uint16).  Needs no device: the CPU tests' handle."""
    def plane(name, d):
        d = np.ascontiguousarray(d, np.float32)
        if d.ndim == 4 and d.shape[3] == 4:
            return d, d.ctypes.data + 12, 4
        if d.ndim != 3:
            raise ValueError("render_flow: `%s` must be a [B, H, W] plane or a [B, H, W, 4] coord target" % name)
        return d, d.ctypes.data, 1

    def inst(name, i, shape):
        i = np.ascontiguousarray(i)
        if i.dtype not in (np.int16, np.uint16) or i.shape[:3] != shape or i.size != int(np.prod(shape)):
            raise ValueError("render_flow: `%s` must be an int16 %s array" % (name, list(shape)))
        return i

    da, pa, sa = plane("depth_a", depth_a)
    B, H, W = da.shape[:3]
    ia = inst("instance_a", instance_a, (B, H, W))
    m = np.ascontiguousarray(motion, np.float32)
    if m.ndim != 4 or m.shape[0] != B or m.shape[2:] != (3, 4):
        raise ValueError("render_flow: `motion` must be [%d, n_slots, 3, 4]" % B)
    db, pb, sb = (None, None, 0) if depth_b is None else plane("depth_b", depth_b)
    if db is not None and db.shape[:3] != (B, H, W):
        raise ValueError("render_flow: depth_b must have the size of depth_a")
    ib = None if instance_b is None else inst("instance_b", instance_b, (B, H, W))
    rec = check_params(make_params(intrinsics, (W, H), m.shape[1], **kw))
    out = _empty(_shapes(B, H, W, m.shape[1]), int(rec["outputs"][0]), lambda s, t: np.zeros(s, t))
    ptr = {k: (v.ctypes.data if v is not None else None) for k, v in out.items()}
    st = _abi.lib().slhip_render_flow_host(rec.ctypes.data, pa, sa, ia.ctypes.data, m.ctypes.data, pb, sb,
                                           ib.ctypes.data if ib is not None else None, B, ptr["flow"], ptr["scene_flow"],
                                           ptr["flags"], ptr["counts"])
    _abi.check(st, "slhip_render_flow_host")
    return RenderFlow(params=rec[0].copy(), **out)


def compute(depth_a, instance_a, motion, intrinsics, depth_b=None, instance_b=None, max_depth=3000.0, depth_tol=DEPTH_TOL,
            depth_rel=DEPTH_REL, match_instance=True, outputs=("flow", "flags")):
    """The flow of every pixel of picture a into picture b: a RenderFlow.

    depth_a, depth_b      float32 [B, H, W] (a plane) or [B, H, W, 4] (the coord target: its w is read in place) on the device.
                          Without depth_b nothing is `visible` and that count is 0
    instance_a, instance_b  int16 [B, H, W] or [B, H, W, 1], as rendered; without instance_b (or with match_instance=False) a
                          footprint pixel of b passes by its depth alone
    motion                float32 [B, n_slots, 3, 4], n_slots <= 256: row i moves a point of camera frame a to camera frame b
                          for the pixels of instance i (`motion()`); slot 0 is the plane and the background
    intrinsics            (fx, fy, cx, cy) both pictures were rendered with
    max_depth             a pixel of a at or beyond it is not valid: the renderer writes 3000 where nothing was hit
    depth_tol, depth_rel  a moved point at Z' is visible where Z' <= z_b + depth_tol + depth_rel * Z' on its footprint.  The
                          defaults of 0.005 and 0.01 are conveniences, not measured values: choose them for the meshes, the
                          depth and the baseline at hand
    outputs               names of OUTPUTS, or the bit mask

    Asynchronous on the current stream."""
    tensors = (depth_a, instance_a, motion) + tuple(t for t in (depth_b, instance_b) if t is not None)
    dev = _device.require_cuda(NAME, tensors, "depths, instances and motion", "depths, instances and motion must be torch tensors")
    if depth_a.dtype != torch.float32 or depth_a.dim() not in (3, 4) or (depth_a.dim() == 4 and depth_a.shape[3] != 4) or not depth_a.is_contiguous():
        raise ValueError("render_flow: `depth_a` must be a contiguous float32 [B, H, W] plane or [B, H, W, 4] coord target")
    B, H, W = (int(v) for v in depth_a.shape[:3])

    def plane(name, d):
        if d.dtype != torch.float32 or tuple(d.shape) not in ((B, H, W), (B, H, W, 4)) or not d.is_contiguous():
            raise ValueError("render_flow: `%s` must be a contiguous float32 [%d, %d, %d] plane or [.., 4] coord target" % (name, B, H, W))
        return (d.data_ptr(), 1) if d.dim() == 3 else (d.data_ptr() + 12, 4)

    def inst(name, i):
        if i.dtype != torch.int16 or tuple(i.shape) not in ((B, H, W), (B, H, W, 1)) or not i.is_contiguous():
            raise ValueError("render_flow: `%s` must be a contiguous int16 [%d, %d, %d] tensor" % (name, B, H, W))
        return i.data_ptr()

    pa, sa = plane("depth_a", depth_a)
    ia = inst("instance_a", instance_a)
    pb, sb = (None, 0) if depth_b is None else plane("depth_b", depth_b)
    ib = None if instance_b is None else inst("instance_b", instance_b)
    if motion.dtype != torch.float32 or motion.dim() != 4 or motion.shape[0] != B or tuple(motion.shape[2:]) != (3, 4) or not motion.is_contiguous():
        raise ValueError("render_flow: `motion` must be a contiguous float32 [%d, n_slots, 3, 4] tensor" % B)
    S = int(motion.shape[1])
    rec = check_params(make_params(intrinsics, (W, H), S, max_depth, depth_tol, depth_rel, match_instance, outputs))
    out = _empty(_shapes(B, H, W, S), int(rec["outputs"][0]),
                 lambda s, t: torch.empty(s, dtype=getattr(torch, t), device=dev))
    if B:
        with torch.cuda.device(dev):
            st = _abi.lib().slhip_render_flow(rec.ctypes.data, C.c_void_p(pa), sa, C.c_void_p(ia), C.c_void_p(motion.data_ptr()),
                                              C.c_void_p(pb), sb, C.c_void_p(ib), B, *(C.c_void_p(_device.ptr(out[k])) for k in OUTPUTS),
                                              _device.stream_ptr(dev))
        _abi.check(st, "slhip_render_flow")
    res = RenderFlow(params=rec[0].copy(), **out)
    res._keepalive = (depth_a, instance_a, motion, depth_b, instance_b)      # the call is asynchronous: its inputs live as long as its outputs
    return res
