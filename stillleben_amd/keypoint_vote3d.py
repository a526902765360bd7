"""Keypoint voting in 3D -- this project's addition (the reference has no counterpart): per-point predicted 3D offsets to one
camera-frame position per (object, keypoint) with an uncertainty, the decoder of PVN3D / FFB6D -- the step between the offset
target of `ObjectKeypoints.offsets` and `sl.pose_fit`.  The candidates camera_j + offset_jk of a (set, keypoint) are clustered by
mean shift and the mode with the most support is returned.  Everything stays on the device, through one entry of
include/slhip.h: slhip_keypoint_vote3d, one workgroup per (set, keypoint), a lane per seed.  There is no CPU path; `vote_host`
runs the library's host twin of the same rules for tests and needs no device.

    points = batch.points(buffers, n_points=1024, outputs=("camera",))    # [n, K] camera-frame points of every visible object
    votes3 = batch.keypoint_votes3d(points, predicted_offsets)            # or sl.keypoint_vote3d.vote(points, offsets, ...)
    votes3.xyz, votes3.n_support, votes3.best, votes3.iters, votes3.flags, votes3.mean, votes3.cov3x3(), votes3.support_mask()
    fit = batch.pose_fit(votes3, bank=bank)                               # sl.pose_fit.solve(*votes3.correspondences(bank))

DESIGN.md "Keypoint voting in 3D" states the rules operation by operation."""
import ctypes as C

import numpy as np
import torch

from . import _abi, _device, _record_set

__all__ = ["OUTPUTS", "FLAGS", "KeypointVotes3D", "make_params", "check_params", "vote", "vote_host"]

NAME = "keypoint_vote3d"
_TABLE = (("xyz", _abi.VOTE3D_OUT_XYZ, (3,), np.float32), ("n_support", _abi.VOTE3D_OUT_N_SUPPORT, (), np.int32),
          ("best", _abi.VOTE3D_OUT_BEST, (), np.int32), ("iters", _abi.VOTE3D_OUT_ITERS, (), np.int32),
          ("flags", _abi.VOTE3D_OUT_FLAGS, (), np.int32), ("mean", _abi.VOTE3D_OUT_MEAN, (3,), np.float32),
          ("cov", _abi.VOTE3D_OUT_COV, (6,), np.float32), ("support", _abi.VOTE3D_OUT_SUPPORT, ("words",), np.uint32))
OUTPUTS = {name: bit for name, bit, _, _ in _TABLE}
FLAGS = {"insufficient": _abi.VOTE3D_INSUFFICIENT, "no_model": _abi.VOTE3D_NO_MODEL, "not_converged": _abi.VOTE3D_NOT_CONVERGED}
_ALL = tuple(OUTPUTS)


def make_params(n_sets, n_points, n_keypoints, n_seeds=128, bandwidth=0.05, max_iters=32, tol=1e-4, min_support=1, outputs=_ALL):
    """One slhip_keypoint_vote3d_params record (numpy).  `bandwidth`: the radius h of the mean-shift kernel, in the unit of the
    camera points (metres); `tol`: a seed stops when it moves by no more than this; `outputs`: names or the bit mask.  The
    defaults (128 seeds, h = 0.05, 32 steps, tol = 1e-4, min_support = 1) are conveniences, not measured values: choose h for
    the objects' size and the network's error at hand."""
    p = np.zeros((), _abi.KEYPOINT_VOTE3D_PARAMS_DTYPE)
    p["n_sets"], p["n_points"], p["n_keypoints"], p["n_seeds"] = int(n_sets), int(n_points), int(n_keypoints), int(n_seeds)
    p["bandwidth"], p["max_iters"], p["tol"], p["min_support"] = np.float32(bandwidth), int(max_iters), np.float32(tol), int(min_support)
    p["outputs"] = outputs if isinstance(outputs, int) else _record_set.output_bits(outputs, OUTPUTS)
    return p


def check_params(params):
    """Raises SlhipError when the record breaks a rule of slhip_keypoint_vote3d_check_params.  Needs no device."""
    rec = np.ascontiguousarray(np.asarray(params, dtype=_abi.KEYPOINT_VOTE3D_PARAMS_DTYPE).reshape(1))
    _abi.check(_abi.lib().slhip_keypoint_vote3d_check_params(rec.ctypes.data), "slhip_keypoint_vote3d")
    return rec


n_words = _record_set.n_words


class KeypointVotes3D(_record_set.OutputSet):
    """The position of every keypoint of every set (torch tensors on the device from `vote`, numpy arrays from `vote_host`; those
    not asked for are None):
        xyz        float32 [M, Kp, 3] the winning mode in the camera frame                  n_support  int32 [M, Kp]
        best       int32 [M, Kp] the winning seed (-2: none)                                iters      int32 [M, Kp] its steps
        flags      int32 [M, Kp] bits of FLAGS
        mean, cov  float32 [M, Kp, 3] and [M, Kp, 6] (xx, xy, xz, yy, yz, zz): mean and covariance of the winner's supporters
        support    uint32 words [M, Kp, ceil(K / 32)] (held as int32 on the device), bit j & 31 of word j >> 5
        found      bool [M, Kp]: the keypoint has a position
    A keypoint without a valid voter (`insufficient`) or without a mode of min_support (`no_model`) has NaN xyz, mean and cov,
    0 supporters, best -2 and no support bit -- never a zero position.  `classes`: the class of every set's object
    (SceneBatch.keypoint_votes3d fills it), what `correspondences` looks the bank up with."""

    NAME, TABLE, RECORD, FAILED = NAME, _TABLE, _abi.KeypointVote3dOut, _abi.VOTE3D_INSUFFICIENT | _abi.VOTE3D_NO_MODEL

    def __init__(self, n_points, xyz=None, n_support=None, best=None, iters=None, flags=None, mean=None, cov=None, support=None,
                 classes=None):
        super().__init__(xyz=xyz, n_support=n_support, best=best, iters=iters, flags=flags, mean=mean, cov=cov, support=support)
        self.n_points, self.classes = int(n_points), classes

    def support_mask(self):
        """bool [M, Kp, K]: voter j of a set supports the keypoint's position"""
        if self.support is None:
            raise RuntimeError("keypoint_vote3d: the `support` output was not asked for")
        return _record_set.bit_mask(self.support, self.n_points)

    def cov3x3(self):
        """float32 [M, Kp, 3, 3]: the covariance as a symmetric matrix"""
        if self.cov is None:
            raise RuntimeError("keypoint_vote3d: the `cov` output was not asked for")
        c = self.cov
        order = [0, 1, 2, 1, 3, 4, 2, 4, 5]
        if isinstance(c, np.ndarray):
            return c[..., order].reshape(c.shape[:-1] + (3, 3))
        return c[..., order].reshape(tuple(c.shape[:-1]) + (3, 3))

    def correspondences(self, bank, classes=None):
        """(src [M, Kp, 4], dst [M, Kp, 4]): every keypoint's point of `bank` (a KeypointBank or a float32 [A, Kp, 4] tensor) in
        the object frame, and its voted position xyz with dst.w = 1 where the keypoint was found and 0 elsewhere (there
        xyz is NaN, and the fit skips it) -- what sl.pose_fit.solve(src, dst) takes.  `classes`: the class of every set's object,
        integers [M]; default: what SceneBatch.keypoint_votes3d filled in."""
        if self.xyz is None:
            raise RuntimeError("keypoint_vote3d: the `xyz` output was not asked for")
        classes = self.classes if classes is None else classes
        if classes is None:
            raise TypeError("keypoint_vote3d: correspondences needs the class of every set (`classes`)")
        pts = bank.points if hasattr(bank, "points") else bank
        found = self.found
        if isinstance(self.xyz, np.ndarray):
            pts = pts.cpu().numpy() if isinstance(pts, torch.Tensor) else np.asarray(pts, np.float32)
            src = np.ascontiguousarray(pts[np.asarray(classes, np.int64)], np.float32)
            if src.shape[:2] != self.xyz.shape[:2]:
                raise ValueError("keypoint_vote3d: the bank holds %d keypoints per class, the votes %d" % (src.shape[1], self.xyz.shape[1]))
            dst = np.zeros(self.xyz.shape[:2] + (4,), np.float32)
            dst[..., :3] = self.xyz
            dst[..., 3] = found.astype(np.float32)
            return src, dst
        src = pts.to(self.xyz.device)[torch.as_tensor(classes, device=self.xyz.device).long()].contiguous()
        if tuple(src.shape[:2]) != tuple(self.xyz.shape[:2]):
            raise ValueError("keypoint_vote3d: the bank holds %d keypoints per class, the votes %d" % (src.shape[1], self.xyz.shape[1]))
        dst = torch.zeros(tuple(self.xyz.shape[:2]) + (4,), dtype=torch.float32, device=self.xyz.device)
        dst[..., :3] = self.xyz
        dst[..., 3] = found.to(torch.float32)
        return src, dst


def vote_host(camera, offsets, **kw):
    """slhip_keypoint_vote3d_host on host arrays: a KeypointVotes3D of numpy arrays.  camera float32 [M, K, 4]; offsets float32
    [M, K, Kp, 3]; `kw`: the other arguments of make_params.  Needs no device: the CPU tests' handle."""
    camera = np.ascontiguousarray(camera, np.float32)
    offsets = np.ascontiguousarray(offsets, np.float32)
    if camera.ndim != 3 or camera.shape[2] != 4:
        raise ValueError("keypoint_vote3d: camera must be [M, K, 4]")
    M, K = camera.shape[:2]
    if offsets.ndim != 4 or offsets.shape[:2] != (M, K) or offsets.shape[3] != 3:
        raise ValueError("keypoint_vote3d: offsets must be [%d, %d, Kp, 3]" % (M, K))
    Kp = offsets.shape[2]
    rec = check_params(make_params(M, K, Kp, **kw))
    res = KeypointVotes3D(K, **KeypointVotes3D.empty((M, Kp), int(rec["outputs"][0]), words=n_words(K)))
    if M:
        st = _abi.lib().slhip_keypoint_vote3d_host(rec.ctypes.data, camera.ctypes.data, offsets.ctypes.data, C.byref(res.record()))
        _abi.check(st, "slhip_keypoint_vote3d_host")
    return res


def vote(points_or_camera, offsets, **kw):
    """The position of every keypoint of every set of voters: a KeypointVotes3D.

    points_or_camera  float32 [M, K, 4] camera-frame points (x, y, z, w) on the device, a voter counts when w != 0; or an
                      ObjectPoints with its `camera` output
    offsets           float32 [M, K, Kp, 3] on the device: a network's prediction in the layout of ObjectKeypoints.offsets
    kw                n_seeds=128, bandwidth=0.05, max_iters=32, tol=1e-4, min_support=1 (conveniences, not measured values),
                      outputs

    Asynchronous on the current stream."""
    camera = points_or_camera
    if hasattr(points_or_camera, "camera") and hasattr(points_or_camera, "records"):      # an ObjectPoints
        camera = points_or_camera.camera
        if camera is None:
            raise RuntimeError("keypoint_vote3d: the ObjectPoints need their `camera` output")
    dev = _device.require_cuda(NAME, [camera, offsets], "camera points and offsets", "camera points and offsets must be torch tensors")
    if camera.dtype != torch.float32 or camera.dim() != 3 or camera.shape[2] != 4 or not camera.is_contiguous():
        raise ValueError("keypoint_vote3d: camera must be a contiguous float32 [M, K, 4] tensor")
    M, K = int(camera.shape[0]), int(camera.shape[1])
    if (offsets.dtype != torch.float32 or offsets.dim() != 4 or tuple(offsets.shape[:2]) != (M, K) or offsets.shape[3] != 3
            or not offsets.is_contiguous()):
        raise ValueError("keypoint_vote3d: offsets must be a contiguous float32 [%d, %d, Kp, 3] tensor" % (M, K))
    Kp = int(offsets.shape[2])
    rec = check_params(make_params(M, K, Kp, **kw))
    res = KeypointVotes3D(K, **KeypointVotes3D.empty((M, Kp), int(rec["outputs"][0]), dev, words=n_words(K)))
    if M:
        out = res.record()
        with torch.cuda.device(dev):
            st = _abi.lib().slhip_keypoint_vote3d(rec.ctypes.data, C.c_void_p(camera.data_ptr()), C.c_void_p(offsets.data_ptr()),
                                                  C.byref(out), _device.stream_ptr(dev))
        _abi.check(st, "slhip_keypoint_vote3d")
    res._keepalive = (camera, offsets)      # the launch is asynchronous: its inputs live as long as its outputs
    return res
