"""Rigid fit -- this project's addition (the reference has no counterpart): the pose of every set of N 3D-3D correspondences in
the least-squares sense (Horn / Kabsch), the last step of PVN3D / FFB6D (the bank's keypoints onto the voted ones) and the pose
from predicted object coordinates plus depth (`points.coord` onto `points.camera`), the depth counterpart of `sl.pose_pnp`.
Horn's unit quaternion from a fixed number of Jacobi sweeps on a 4 x 4: always a proper rotation, flat point sets included.
Everything stays on the device, through one entry of include/slhip.h: slhip_pose_fit, one workgroup per set.  There is no CPU
path; `solve_host` runs the library's host twin of the same rules for tests and needs no device.

    fit = batch.pose_fit(votes3, bank=bank)                               # or sl.pose_fit.solve(src, dst)
    fit = batch.pose_fit(points.coord, points.camera)                     # object coordinates onto camera points
    fit.pose, fit.n_used, fit.rms, fit.flags, fit.found
    err = batch.pose_errors(fit.dense(B, O, points.scene_global, points.slot), bank)

DESIGN.md "Rigid fit" states the rules operation by operation."""
import ctypes as C

import numpy as np
import torch

from . import _abi, _device, _record_set

__all__ = ["OUTPUTS", "FLAGS", "PoseFit", "make_params", "check_params", "solve", "solve_host"]

NAME = "pose_fit"
FLAGS = {"insufficient": _abi.FIT_INSUFFICIENT, "degenerate": _abi.FIT_DEGENERATE}


class PoseFit(_record_set.PoseSet):
    """The pose of every set (torch tensors on the device from `solve`, numpy arrays from `solve_host`; those not asked for are
    None):
        pose    float32 [M, 3, 4] object to camera       n_used  int32 [M] the correspondences that counted
        rms     float32 [M] root mean square of |R src + t - dst| over them, in the unit of the points
        flags   int32 [M] bits of FLAGS
        found   bool [M]: the set has a pose
    A set with fewer than 3 correspondences that count (`insufficient`) or with collinear or coincident points (`degenerate`)
    has a NaN pose and rms -- never an identity pose."""
    NAME, RECORD, FAILED = NAME, _abi.PoseFitOut, _abi.FIT_INSUFFICIENT | _abi.FIT_DEGENERATE
    TABLE = (("pose", _abi.FIT_OUT_POSE, (3, 4), np.float32), ("n_used", _abi.FIT_OUT_N_USED, (), np.int32),
             ("rms", _abi.FIT_OUT_RMS, (), np.float32), ("flags", _abi.FIT_OUT_FLAGS, (), np.int32))

    def __init__(self, pose=None, n_used=None, rms=None, flags=None):
        super().__init__(pose=pose, n_used=n_used, rms=rms, flags=flags)


OUTPUTS = PoseFit.OUTPUTS
_ALL = tuple(OUTPUTS)


def make_params(n_sets, n_points, min_gap=1e-6, outputs=_ALL):
    """One slhip_pose_fit_params record (numpy).  `min_gap`: a set is `degenerate` (collinear or coincident points) when the two
    largest eigenvalues of Horn's matrix differ by no more than min_gap times the sum of the four absolute eigenvalues; the
    default of 1e-6 is a convenience, not a measured value.  `outputs`: names or the bit mask."""
    p = np.zeros((), _abi.POSE_FIT_PARAMS_DTYPE)
    p["n_sets"], p["n_points"], p["min_gap"] = int(n_sets), int(n_points), np.float32(min_gap)
    p["outputs"] = outputs if isinstance(outputs, int) else _record_set.output_bits(outputs, OUTPUTS)
    return p


def check_params(params):
    """Raises SlhipError when the record breaks a rule of slhip_pose_fit_check_params.  Needs no device."""
    rec = np.ascontiguousarray(np.asarray(params, dtype=_abi.POSE_FIT_PARAMS_DTYPE).reshape(1))
    _abi.check(_abi.lib().slhip_pose_fit_check_params(rec.ctypes.data), "slhip_pose_fit")
    return rec


def solve_host(src, dst, **kw):
    """slhip_pose_fit_host on host arrays: a PoseFit of numpy arrays.  src, dst float32 [M, N, 4]; `kw`: the other arguments of
    make_params.  Needs no device: the CPU tests' handle."""
    src = np.ascontiguousarray(src, np.float32)
    dst = np.ascontiguousarray(dst, np.float32)
    if src.ndim != 3 or src.shape[2] != 4 or dst.shape != src.shape:
        raise ValueError("pose_fit: src and dst must both be [M, N, 4]")
    M, N = src.shape[:2]
    rec = check_params(make_params(M, N, **kw))
    res = PoseFit(**PoseFit.empty((M,), int(rec["outputs"][0])))
    if M:
        _abi.check(_abi.lib().slhip_pose_fit_host(rec.ctypes.data, src.ctypes.data, dst.ctypes.data, C.byref(res.record())),
                   "slhip_pose_fit_host")
    return res


def solve(src, dst, **kw):
    """The pose of every set of correspondences: a PoseFit.

    src   float32 [M, N, 4] on the device: points in the object frame and a weight word
    dst   float32 [M, N, 4] on the device: the same points in the camera frame and a validity word; a correspondence counts
          when src.w > 0, dst.w != 0 and all six coordinates are finite
    kw    min_gap=1e-6 (a convenience, not a measured value), outputs

    Asynchronous on the current stream."""
    dev = _device.require_cuda(NAME, [src, dst], "src and dst", "src and dst must be torch tensors")
    if src.dtype != torch.float32 or src.dim() != 3 or src.shape[2] != 4 or not src.is_contiguous():
        raise ValueError("pose_fit: src must be a contiguous float32 [M, N, 4] tensor")
    M, N = int(src.shape[0]), int(src.shape[1])
    if dst.dtype != torch.float32 or tuple(dst.shape) != (M, N, 4) or not dst.is_contiguous():
        raise ValueError("pose_fit: dst must be a contiguous float32 [%d, %d, 4] tensor" % (M, N))
    rec = check_params(make_params(M, N, **kw))
    res = PoseFit(**PoseFit.empty((M,), int(rec["outputs"][0]), dev))
    if M:
        with torch.cuda.device(dev):
            st = _abi.lib().slhip_pose_fit(rec.ctypes.data, C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()),
                                           C.byref(res.record()), _device.stream_ptr(dev))
        _abi.check(st, "slhip_pose_fit")
    res._keepalive = (src, dst)      # the launch is asynchronous: its inputs live as long as its outputs
    return res
