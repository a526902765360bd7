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
OUTPUTS = {"pose": _abi.FIT_OUT_POSE, "n_used": _abi.FIT_OUT_N_USED, "rms": _abi.FIT_OUT_RMS, "flags": _abi.FIT_OUT_FLAGS}
FLAGS = {"insufficient": _abi.FIT_INSUFFICIENT, "degenerate": _abi.FIT_DEGENERATE}
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


class PoseFit:
    """The pose of every set (torch tensors on the device from `solve`, numpy arrays from `solve_host`; those not asked for are
    None):
        pose    float32 [M, 3, 4] object to camera       n_used  int32 [M] the correspondences that counted
        rms     float32 [M] root mean square of |R src + t - dst| over them, in the unit of the points
        flags   int32 [M] bits of FLAGS
    A set with fewer than 3 correspondences that count (`insufficient`) or with collinear or coincident points (`degenerate`)
    has a NaN pose and rms -- never an identity pose."""

    def __init__(self, pose=None, n_used=None, rms=None, flags=None):
        self.pose, self.n_used, self.rms, self.flags = pose, n_used, rms, flags
        self._keepalive = ()

    def __len__(self):
        for k in _ALL:
            if getattr(self, k) is not None:
                return int(getattr(self, k).shape[0])
        return 0

    @property
    def found(self):
        """bool [M]: the set has a pose"""
        if self.flags is not None:
            return self.flags == 0
        if self.pose is None:
            raise RuntimeError("pose_fit: `found` reads the `flags` or `pose` output, and neither was asked for")
        return self.pose[:, 0, 0] == self.pose[:, 0, 0]

    def dense(self, B, O, scene, slot):
        """float32 [B, O, 3, 4]: the pose of set i at [scene[i], slot[i] - 1], NaN where a (scene, slot) has no set -- the shape
        SceneBatch.pose_errors and SceneBatch.pose_vsd take.  `slot` counts from 1 as the renders' instance indices do."""
        if self.pose is None:
            raise RuntimeError("pose_fit: the `pose` output was not asked for")
        if isinstance(self.pose, np.ndarray):
            out = np.full((int(B), int(O), 3, 4), np.nan, np.float32)
            out[np.asarray(scene, np.int64), np.asarray(slot, np.int64) - 1] = self.pose
            return out
        out = torch.full((int(B), int(O), 3, 4), float("nan"), dtype=torch.float32, device=self.pose.device)
        out[torch.as_tensor(scene, device=out.device).long(), torch.as_tensor(slot, device=out.device).long() - 1] = self.pose
        return out


def _record(ptrs):
    return _abi.PoseFitOut(*(ptrs.get(k) for k in _ALL))


def solve_host(src, dst, **kw):
    """slhip_pose_fit_host on host arrays: a PoseFit of numpy arrays.  src, dst float32 [M, N, 4]; `kw`: the other arguments of
    make_params.  Needs no device: the CPU tests' handle."""
    src = np.ascontiguousarray(src, np.float32)
    dst = np.ascontiguousarray(dst, np.float32)
    if src.ndim != 3 or src.shape[2] != 4 or dst.shape != src.shape:
        raise ValueError("pose_fit: src and dst must both be [M, N, 4]")
    M, N = src.shape[:2]
    rec = check_params(make_params(M, N, **kw))
    mask = int(rec["outputs"][0])
    spec = (("pose", (M, 3, 4), np.float32), ("n_used", (M,), np.int32), ("rms", (M,), np.float32), ("flags", (M,), np.int32))
    outs = {k: np.zeros(shape, dt) for k, shape, dt in spec if mask & OUTPUTS[k]}
    o = _record({k: v.ctypes.data for k, v in outs.items()})
    if M:
        _abi.check(_abi.lib().slhip_pose_fit_host(rec.ctypes.data, src.ctypes.data, dst.ctypes.data, C.byref(o)), "slhip_pose_fit_host")
    return PoseFit(**outs)


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
    mask = int(rec["outputs"][0])
    res = PoseFit(**_record_set.empty_outputs(M, mask, dev, (
        ("pose", _abi.FIT_OUT_POSE, (3, 4), torch.float32), ("n_used", _abi.FIT_OUT_N_USED, (), torch.int32),
        ("rms", _abi.FIT_OUT_RMS, (), torch.float32), ("flags", _abi.FIT_OUT_FLAGS, (), torch.int32))))
    if M:
        out = _record({k: _device.ptr(getattr(res, k)) for k in _ALL})
        with torch.cuda.device(dev):
            st = _abi.lib().slhip_pose_fit(rec.ctypes.data, C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), C.byref(out),
                                           _device.stream_ptr(dev))
        _abi.check(st, "slhip_pose_fit")
    res._keepalive = (src, dst)      # the launch is asynchronous: its inputs live as long as its outputs
    return res
