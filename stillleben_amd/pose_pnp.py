"""Pose PnP -- this project's addition (the reference has no counterpart): the pose of every set of K 2D-3D correspondences by
P3P inside RANSAC and Gauss-Newton on the inliers, the step by which correspondence-based methods (GDR-Net's PnP baseline, CDPN,
Pix2Pose, EPOS, ZebraPose, DPOD) turn predicted object coordinates into a pose.  Everything stays on the device, through one
entry of include/slhip.h: slhip_pose_pnp, one workgroup per set.  There is no CPU path; `solve_host` and `p3p_host` run the
library's host twin of the same rules for tests and need no device.

    points = batch.points(buffers, n_points=256)                          # [n, K] pixels and object coordinates
    pnp = batch.pose_pnp(points, coord=predicted)                         # or sl.pose_pnp.solve(points, intrinsics=...)
    pnp.pose, pnp.n_inliers, pnp.rms, pnp.best, pnp.flags, pnp.inlier_mask()
    err = batch.pose_errors(pnp.dense(B, O, points.scene_global, points.slot), bank)

DESIGN.md "Pose PnP" states the rules operation by operation."""
import ctypes as C

import numpy as np
import torch

from . import _abi, _device, _record_set

__all__ = ["OUTPUTS", "FLAGS", "PosePnP", "make_params", "check_params", "solve", "solve_host", "p3p_host"]

NAME = "pose_pnp"
FLAGS = {"insufficient": _abi.PNP_INSUFFICIENT, "no_model": _abi.PNP_NO_MODEL, "refine_stopped": _abi.PNP_REFINE_STOPPED,
         "refine_rejected": _abi.PNP_REFINE_REJECTED}
n_words = _record_set.n_words


class PosePnP(_record_set.InlierPoseSet):
    """The pose of every set (torch tensors on the device from `solve`, numpy arrays from `solve_host`; those not asked for
    are None):
        pose       float32 [M, 3, 4] object to camera       n_inliers  int32 [M]
        rms        float32 [M] reprojection RMS of the inliers in pixels
        inliers    uint32 words [M, ceil(K / 32)] (held as int32 on the device), bit j & 31 of word j >> 5
        best       int32 [M] the winning hypothesis (-1: the initial pose, -2: none)
        flags      int32 [M] bits of FLAGS
    A set with fewer than 4 valid correspondences (`insufficient`) or without a hypothesis of min_inliers (`no_model`) has a
    NaN pose, 0 inliers, a NaN rms, best -2 and no inlier bit -- never an identity pose."""
    NAME, RECORD, FAILED = NAME, _abi.PosePnpOut, _abi.PNP_INSUFFICIENT | _abi.PNP_NO_MODEL
    TABLE = (("pose", _abi.PNP_OUT_POSE, (3, 4), np.float32), ("n_inliers", _abi.PNP_OUT_N_INLIERS, (), np.int32),
             ("rms", _abi.PNP_OUT_RMS, (), np.float32), ("inliers", _abi.PNP_OUT_INLIERS, ("words",), np.uint32),
             ("best", _abi.PNP_OUT_BEST, (), np.int32), ("flags", _abi.PNP_OUT_FLAGS, (), np.int32))


OUTPUTS = PosePnP.OUTPUTS
_ALL = tuple(OUTPUTS)


def make_params(intrinsics, n_sets, n_points, n_hypotheses=256, threshold_px=2.0, refine_iters=4, min_inliers=4, outputs=_ALL,
                seed=0, set_id_base=0):
    """One slhip_pose_pnp_params record (numpy).  `intrinsics`: (fx, fy, cx, cy) of every set without a row of its own;
    `outputs`: names or the bit mask; `seed`: an integer, or the (lo, hi) pair of a Philox key."""
    p = np.zeros((), _abi.POSE_PNP_PARAMS_DTYPE)
    p["fx"], p["fy"], p["cx"], p["cy"] = (np.float32(v) for v in intrinsics)
    p["n_sets"], p["n_points"], p["n_hypotheses"] = int(n_sets), int(n_points), int(n_hypotheses)
    p["threshold_px"], p["refine_iters"], p["min_inliers"] = np.float32(threshold_px), int(refine_iters), int(min_inliers)
    _record_set.set_key(p, seed, set_id_base, "set_id_base")
    p["outputs"] = outputs if isinstance(outputs, int) else _record_set.output_bits(outputs, OUTPUTS)
    return p


def check_params(params):
    """Raises SlhipError when the record breaks a rule of slhip_pose_pnp_check_params.  Needs no device."""
    rec = np.ascontiguousarray(np.asarray(params, dtype=_abi.POSE_PNP_PARAMS_DTYPE).reshape(1))
    _abi.check(_abi.lib().slhip_pose_pnp_check_params(rec.ctypes.data), "slhip_pose_pnp")
    return rec


def solve_host(uv, xyz, intrinsics, per_set_intrinsics=None, init=None, **kw):
    """slhip_pose_pnp_host on host arrays: a PosePnP of numpy arrays.  uv [M, K, 2]; xyz [M, K, 4] (point and weight);
    `intrinsics` (fx, fy, cx, cy); per_set_intrinsics [M, 4] or None; init [M, 3, 4] or None; `kw`: the other arguments of
    make_params.  Needs no device: the CPU tests' handle."""
    uv = np.ascontiguousarray(uv, np.float32)
    xyz = np.ascontiguousarray(xyz, np.float32)
    M, K = uv.shape[:2]
    if uv.shape != (M, K, 2) or xyz.shape != (M, K, 4):
        raise ValueError("pose_pnp: uv must be [M, K, 2] and xyz [M, K, 4]")
    rec = check_params(make_params(intrinsics, M, K, **kw))
    k4 = None if per_set_intrinsics is None else np.ascontiguousarray(per_set_intrinsics, np.float32).reshape(M, 4)
    t0 = None if init is None else np.ascontiguousarray(init, np.float32).reshape(M, 3, 4)
    res = PosePnP(K, **PosePnP.empty((M,), int(rec["outputs"][0]), words=n_words(K)))
    st = _abi.lib().slhip_pose_pnp_host(rec.ctypes.data, uv.ctypes.data, xyz.ctypes.data, None if k4 is None else k4.ctypes.data,
                                        None if t0 is None else t0.ctypes.data, C.byref(res.record()))
    _abi.check(st, "slhip_pose_pnp_host")
    return res


def p3p_host(uv, xyz, intrinsics):
    """slhip_pose_pnp_p3p_host: the minimal solver alone on three correspondences (uv [3, 2], xyz [3, 3]): float32 [n, 3, 4],
    the n <= 4 solutions it keeps.  Needs no device."""
    uv = np.ascontiguousarray(uv, np.float32).reshape(3, 2)
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(3, 3)
    k4 = np.ascontiguousarray(intrinsics, np.float32).reshape(4)
    out = np.zeros((4, 3, 4), np.float32)
    n = _abi.lib().slhip_pose_pnp_p3p_host(uv.ctypes.data, xyz.ctypes.data, k4.ctypes.data, out.ctypes.data)
    if n < 0:
        _abi.check(n, "slhip_pose_pnp_p3p_host")
    return out[:n]


def solve(uv, xyz=None, intrinsics=None, per_set_intrinsics=None, init=None, coord=None, **kw):
    """The pose of every set of correspondences: a PosePnP.

    uv                  float32 [M, K, 2] pixel positions on the device (the centre of pixel (x, y) is (x + 0.5, y + 0.5)), or
                        an ObjectPoints with its `pixel` and `coord` outputs: uv = pixel + 0.5, xyz = its coord
    xyz                 float32 [M, K, 4]: the object-frame point and a weight word; a correspondence counts when all five of
                        u, v, x, y, z are finite and w > 0
    coord               with an ObjectPoints: float32 [M, K, 4] coordinates that replace the rendered ones (a network's)
    intrinsics          (fx, fy, cx, cy) of every set
    per_set_intrinsics  float32 [M, 4] on the device: a row per set (the `K` of an ObjectCrops), or None
    init                float32 [M, 3, 4] on the device: a pose that competes with the sampled hypotheses as index -1 and wins
                        ties; with n_hypotheses=0 the call is a pure refinement
    kw                  n_hypotheses=256, threshold_px=2.0, refine_iters=4, min_inliers=4, outputs, seed, set_id_base

    Asynchronous on the current stream."""
    if intrinsics is None:
        raise TypeError("pose_pnp: `intrinsics` (fx, fy, cx, cy) is required")
    if hasattr(uv, "pixel") and hasattr(uv, "coord"):      # an ObjectPoints
        points = uv
        if xyz is not None:
            raise TypeError("pose_pnp: with an ObjectPoints pass replacement coordinates as `coord`, not `xyz`")
        xyz = points.coord if coord is None else coord
        if points.pixel is None or xyz is None:
            raise RuntimeError("pose_pnp: the ObjectPoints need their `pixel` and `coord` outputs")
        if not points.pixel.is_cuda:
            raise _abi.SlhipError(_device.no_cpu(NAME))
        uv = points.pixel.to(torch.float32) + 0.5
    elif coord is not None:
        raise TypeError("pose_pnp: `coord` goes with an ObjectPoints")
    tensors = [t for t in (uv, xyz, per_set_intrinsics, init) if t is not None]
    dev = _device.require_cuda(NAME, tensors, "uv, xyz, intrinsics and the initial poses", "uv and xyz must be torch tensors")
    if uv.dtype != torch.float32 or uv.dim() != 3 or uv.shape[2] != 2 or not uv.is_contiguous():
        raise ValueError("pose_pnp: uv must be a contiguous float32 [M, K, 2] tensor")
    M, K = int(uv.shape[0]), int(uv.shape[1])
    if xyz.dtype != torch.float32 or tuple(xyz.shape) != (M, K, 4) or not xyz.is_contiguous():
        raise ValueError("pose_pnp: xyz must be a contiguous float32 [%d, %d, 4] tensor" % (M, K))
    if per_set_intrinsics is not None and (per_set_intrinsics.dtype != torch.float32 or tuple(per_set_intrinsics.shape) != (M, 4)
                                           or not per_set_intrinsics.is_contiguous()):
        raise ValueError("pose_pnp: per_set_intrinsics must be a contiguous float32 [%d, 4] tensor" % M)
    if init is not None and (init.dtype != torch.float32 or tuple(init.shape) != (M, 3, 4) or not init.is_contiguous()):
        raise ValueError("pose_pnp: init must be a contiguous float32 [%d, 3, 4] tensor" % M)
    rec = check_params(make_params(intrinsics, M, K, **kw))
    res = PosePnP(K, **PosePnP.empty((M,), int(rec["outputs"][0]), dev, words=n_words(K)))
    out = res.record()
    with torch.cuda.device(dev):
        st = _abi.lib().slhip_pose_pnp(rec.ctypes.data, C.c_void_p(uv.data_ptr()), C.c_void_p(xyz.data_ptr()),
                                       C.c_void_p(_device.ptr(per_set_intrinsics)), C.c_void_p(_device.ptr(init)), C.byref(out),
                                       _device.stream_ptr(dev))
    _abi.check(st, "slhip_pose_pnp")
    res._keepalive = (uv, xyz, per_set_intrinsics, init)      # the launch is asynchronous: its inputs live as long as its outputs
    return res
