"""Robust alignment -- this project's addition (the reference has no counterpart): the pose of every set of K 3D-3D
correspondences that has the most inliers, by Horn's fit of three picked pairs inside RANSAC and the rigid fit on the inliers.
It is to `sl.pose_fit` what `sl.pose_pnp` is to a plain PnP: the pose from predicted object coordinates plus depth (Pix2Pose,
CDPN, EPOS with depth, the 3D-3D stage of NOCS-style decoders) or from voted 3D keypoints (PVN3D) when some of them are wrong
by the size of the object, which ruins a least-squares fit.  Rigid motions only: no similarity scale is estimated.  Everything
stays on the device, through one entry of include/slhip.h: slhip_pose_align, one workgroup per set.  There is no CPU path;
`solve_host` runs the library's host twin of the same rules for tests and needs no device.

    points = batch.points(buffers, n_points=256)                           # [n, K] object coordinates and camera points
    align = batch.pose_align(points, coord=predicted, threshold=2e-3)      # or sl.pose_align.solve(src, dst, threshold=...)
    align = batch.pose_align(votes3, bank=bank, threshold=5e-3)            # bank keypoints onto voted ones
    align.pose, align.n_inliers, align.rms, align.best, align.flags, align.found, align.inlier_mask()
    icp = batch.pose_icp(points, align, bank)

DESIGN.md "Robust alignment" states the rules operation by operation."""
import ctypes as C

import numpy as np
import torch

from . import _abi, _device, _record_set

__all__ = ["OUTPUTS", "FLAGS", "PoseAlign", "make_params", "check_params", "solve", "solve_host"]

NAME = "pose_align"
FLAGS = {"insufficient": _abi.ALIGN_INSUFFICIENT, "no_model": _abi.ALIGN_NO_MODEL, "refine_stopped": _abi.ALIGN_REFINE_STOPPED,
         "refine_rejected": _abi.ALIGN_REFINE_REJECTED}
n_words = _record_set.n_words


class PoseAlign(_record_set.InlierPoseSet):
    """The pose of every set (torch tensors on the device from `solve`, numpy arrays from `solve_host`; those not asked for
    are None):
        pose       float32 [M, 3, 4] object to camera       n_inliers  int32 [M]
        rms        float32 [M] root mean square of |R src + t - dst| over the inliers, in the unit of the points
        inliers    uint32 words [M, ceil(K / 32)] (held as int32 on the device), bit j & 31 of word j >> 5
        best       int32 [M] the winning hypothesis (-1: the initial pose, -2: none)
        flags      int32 [M] bits of FLAGS
        found      bool [M]: the set has a pose
    A set with fewer than 3 valid correspondences (`insufficient`) or without a hypothesis of min_inliers (`no_model`) has a
    NaN pose, 0 inliers, a NaN rms, best -2 and no inlier bit -- never an identity pose and never the initial one."""
    NAME, RECORD, FAILED = NAME, _abi.PoseAlignOut, _abi.ALIGN_INSUFFICIENT | _abi.ALIGN_NO_MODEL
    TABLE = (("pose", _abi.ALIGN_OUT_POSE, (3, 4), np.float32), ("n_inliers", _abi.ALIGN_OUT_N_INLIERS, (), np.int32),
             ("rms", _abi.ALIGN_OUT_RMS, (), np.float32), ("inliers", _abi.ALIGN_OUT_INLIERS, ("words",), np.uint32),
             ("best", _abi.ALIGN_OUT_BEST, (), np.int32), ("flags", _abi.ALIGN_OUT_FLAGS, (), np.int32))


OUTPUTS = PoseAlign.OUTPUTS
_ALL = tuple(OUTPUTS)


def make_params(n_sets, n_points, threshold, n_hypotheses=256, refine_iters=4, min_gap=1e-6, min_inliers=3, outputs=_ALL, seed=0,
                set_id_base=0):
    """One slhip_pose_align_params record (numpy).  `threshold`: the largest |R src + t - dst| of an inlier, in the unit of the
    points; it has no default, because it depends on that unit and on the noise of the correspondences.  `min_gap`: as
    sl.pose_fit's, for the samples and the refits (the default of 1e-6 is a convenience, not a measured value).  `outputs`: names
    or the bit mask; `seed`: an integer, or the (lo, hi) pair of a Philox key."""
    p = np.zeros((), _abi.POSE_ALIGN_PARAMS_DTYPE)
    p["n_sets"], p["n_points"], p["n_hypotheses"] = int(n_sets), int(n_points), int(n_hypotheses)
    p["threshold"], p["min_gap"] = np.float32(threshold), np.float32(min_gap)
    p["refine_iters"], p["min_inliers"] = int(refine_iters), int(min_inliers)
    _record_set.set_key(p, seed, set_id_base, "set_id_base")
    p["outputs"] = outputs if isinstance(outputs, int) else _record_set.output_bits(outputs, OUTPUTS)
    return p


def check_params(params):
    """Raises SlhipError when the record breaks a rule of slhip_pose_align_check_params.  Needs no device."""
    rec = np.ascontiguousarray(np.asarray(params, dtype=_abi.POSE_ALIGN_PARAMS_DTYPE).reshape(1))
    _abi.check(_abi.lib().slhip_pose_align_check_params(rec.ctypes.data), "slhip_pose_align")
    return rec


def solve_host(src, dst, init=None, **kw):
    """slhip_pose_align_host on host arrays: a PoseAlign of numpy arrays.  src, dst float32 [M, K, 4]; init [M, 3, 4] or None;
    `kw`: the other arguments of make_params (`threshold` is required).  Needs no device: the CPU tests' handle."""
    src = np.ascontiguousarray(src, np.float32)
    dst = np.ascontiguousarray(dst, np.float32)
    if src.ndim != 3 or src.shape[2] != 4 or dst.shape != src.shape:
        raise ValueError("pose_align: src and dst must both be [M, K, 4]")
    M, K = src.shape[:2]
    rec = check_params(make_params(M, K, **kw))
    t0 = None if init is None else np.ascontiguousarray(init, np.float32).reshape(M, 3, 4)
    res = PoseAlign(K, **PoseAlign.empty((M,), int(rec["outputs"][0]), words=n_words(K)))
    if M:
        st = _abi.lib().slhip_pose_align_host(rec.ctypes.data, src.ctypes.data, dst.ctypes.data,
                                              None if t0 is None else t0.ctypes.data, C.byref(res.record()))
        _abi.check(st, "slhip_pose_align_host")
    return res


def solve(src, dst=None, init=None, coord=None, **kw):
    """The pose of every set of correspondences: a PoseAlign.

    src     float32 [M, K, 4] on the device: points in the object frame and a weight word; or an ObjectPoints with its `coord`
            and `camera` outputs: src = its coord, dst = its camera
    dst     float32 [M, K, 4] on the device: the same points in the camera frame and a validity word; a correspondence counts
            when src.w > 0, dst.w != 0 and all six coordinates are finite
    coord   with an ObjectPoints: float32 [M, K, 4] coordinates that replace the rendered ones (a network's)
    init    float32 [M, 3, 4] on the device: a pose that competes with the sampled hypotheses as index -1 and wins ties; with
            n_hypotheses=0 the call is a pure refit on the inliers of that pose
    kw      threshold (required), n_hypotheses=256, refine_iters=4, min_gap=1e-6, min_inliers=3, outputs, seed, set_id_base

    Asynchronous on the current stream."""
    if hasattr(src, "coord") and hasattr(src, "camera"):      # an ObjectPoints
        points = src
        if dst is not None:
            raise TypeError("pose_align: with an ObjectPoints pass replacement coordinates as `coord`, not `dst`")
        src, dst = points.coord if coord is None else coord, points.camera
        if src is None or dst is None:
            raise RuntimeError("pose_align: the ObjectPoints need their `coord` and `camera` outputs")
    elif coord is not None:
        raise TypeError("pose_align: `coord` goes with an ObjectPoints")
    elif dst is None:
        raise TypeError("pose_align: `dst` is required with a `src` tensor")
    tensors = [t for t in (src, dst, init) if t is not None]
    dev = _device.require_cuda(NAME, tensors, "src, dst and the initial poses", "src and dst must be torch tensors")
    if src.dtype != torch.float32 or src.dim() != 3 or src.shape[2] != 4 or not src.is_contiguous():
        raise ValueError("pose_align: src must be a contiguous float32 [M, K, 4] tensor")
    M, K = int(src.shape[0]), int(src.shape[1])
    if dst.dtype != torch.float32 or tuple(dst.shape) != (M, K, 4) or not dst.is_contiguous():
        raise ValueError("pose_align: dst must be a contiguous float32 [%d, %d, 4] tensor" % (M, K))
    if init is not None and (init.dtype != torch.float32 or tuple(init.shape) != (M, 3, 4) or not init.is_contiguous()):
        raise ValueError("pose_align: init must be a contiguous float32 [%d, 3, 4] tensor" % M)
    rec = check_params(make_params(M, K, **kw))
    res = PoseAlign(K, **PoseAlign.empty((M,), int(rec["outputs"][0]), dev, words=n_words(K)))
    if M:
        with torch.cuda.device(dev):
            st = _abi.lib().slhip_pose_align(rec.ctypes.data, C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()),
                                             C.c_void_p(_device.ptr(init)), C.byref(res.record()), _device.stream_ptr(dev))
        _abi.check(st, "slhip_pose_align")
    res._keepalive = (src, dst, init)      # the launch is asynchronous: its inputs live as long as its outputs
    return res
