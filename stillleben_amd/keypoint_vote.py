"""Keypoint voting -- this project's addition (the reference has no counterpart): a predicted field of per-pixel unit vectors to
one 2D position per (object, keypoint) with an uncertainty, PVNet's RANSAC voting layer -- the step between the vector-field
target of `sl.object_keypoints` and `sl.pose_pnp`.  Everything stays on the device, through one entry of include/slhip.h:
slhip_keypoint_vote, one workgroup per (set, keypoint).  There is no CPU path; `vote_host` runs the library's host twin of the same
rules for tests and needs no device.

    points = batch.points(buffers, n_points=1024, outputs=("pixel",))     # [n, K] pixels of every visible object
    votes = batch.keypoint_votes(points, predicted_field)                 # or sl.keypoint_vote.vote(points, field=..., ...)
    votes.uv, votes.n_inliers, votes.best, votes.flags, votes.mean, votes.cov2x2(), votes.inlier_mask(), votes.found
    pnp = batch.pose_pnp(*votes.correspondences(bank))                    # uv [n, Kp, 2], xyz [n, Kp, 4]

DESIGN.md "Keypoint voting" states the rules operation by operation."""
import ctypes as C

import numpy as np
import torch

from . import _abi, _device, _record_set

__all__ = ["OUTPUTS", "FLAGS", "KeypointVotes", "make_params", "check_params", "vote", "vote_host"]

NAME = "keypoint_vote"
_TABLE = (("uv", _abi.VOTE_OUT_UV, (2,), np.float32), ("n_inliers", _abi.VOTE_OUT_N_INLIERS, (), np.int32),
          ("best", _abi.VOTE_OUT_BEST, (), np.int32), ("flags", _abi.VOTE_OUT_FLAGS, (), np.int32),
          ("mean", _abi.VOTE_OUT_MEAN, (2,), np.float32), ("cov", _abi.VOTE_OUT_COV, (3,), np.float32),
          ("inliers", _abi.VOTE_OUT_INLIERS, ("words",), np.uint32))
OUTPUTS = {name: bit for name, bit, _, _ in _TABLE}
FLAGS = {"insufficient": _abi.VOTE_INSUFFICIENT, "no_model": _abi.VOTE_NO_MODEL, "refine_stopped": _abi.VOTE_REFINE_STOPPED,
         "refine_rejected": _abi.VOTE_REFINE_REJECTED}
_ALL = tuple(OUTPUTS)
ANY_SIZE = (32768, 32768)      # the picture of gathered vectors when none is named: every pixel with x, y >= 0 lies inside


def make_params(size, n_sets, n_points, n_keypoints, n_hypotheses=128, inlier_cos=0.99, min_inliers=2, min_sin=1e-3, outputs=_ALL,
                seed=0, set_id_base=0):
    """One slhip_keypoint_vote_params record (numpy).  `size`: (W, H) of the picture the pixels lie in; `inlier_cos`: the smallest
    cosine between a voter's vector and the direction from its pixel to the position (0.99 is PVNet's customary value: a
    convenience, not a measured one); `min_sin`: the smallest |d_a x d_b| of a sampled pair; `outputs`: names or the bit mask;
    `seed`: an integer, or the (lo, hi) pair of a Philox key."""
    p = np.zeros((), _abi.KEYPOINT_VOTE_PARAMS_DTYPE)
    p["W"], p["H"] = int(size[0]), int(size[1])
    p["n_sets"], p["n_points"], p["n_keypoints"], p["n_hypotheses"] = int(n_sets), int(n_points), int(n_keypoints), int(n_hypotheses)
    p["inlier_cos"], p["min_inliers"], p["min_sin"] = np.float32(inlier_cos), int(min_inliers), np.float32(min_sin)
    _record_set.set_key(p, seed, set_id_base, "set_id_base")
    p["outputs"] = outputs if isinstance(outputs, int) else _record_set.output_bits(outputs, OUTPUTS)
    return p


def check_params(params):
    """Raises SlhipError when the record breaks a rule of slhip_keypoint_vote_check_params.  Needs no device."""
    rec = np.ascontiguousarray(np.asarray(params, dtype=_abi.KEYPOINT_VOTE_PARAMS_DTYPE).reshape(1))
    _abi.check(_abi.lib().slhip_keypoint_vote_check_params(rec.ctypes.data), "slhip_keypoint_vote")
    return rec


n_words = _record_set.n_words


class KeypointVotes(_record_set.OutputSet):
    """The position of every keypoint of every set (torch tensors on the device from `vote`, numpy arrays from `vote_host`; those
    not asked for are None):
        uv         float32 [M, Kp, 2] pixel position (pixel index x covers [x, x + 1))     n_inliers  int32 [M, Kp]
        best       int32 [M, Kp] the winning hypothesis (-2: none)                          flags      int32 [M, Kp] bits of FLAGS
        mean, cov  float32 [M, Kp, 2] and [M, Kp, 3] (xx, xy, yy): the hypotheses' weighted mean and covariance
        inliers    uint32 words [M, Kp, ceil(K / 32)] (held as int32 on the device), bit j & 31 of word j >> 5
        found      bool [M, Kp]: the keypoint has a position
    A keypoint with fewer than 2 valid voters (`insufficient`) or without a hypothesis of min_inliers (`no_model`) has NaN uv,
    mean and cov, 0 inliers, best -2 and no inlier bit -- never a zero position.  `classes`: the class of every set's object
    (SceneBatch.keypoint_votes fills it), what `correspondences` looks the bank up with."""

    NAME, TABLE, RECORD, FAILED = NAME, _TABLE, _abi.KeypointVoteOut, _abi.VOTE_INSUFFICIENT | _abi.VOTE_NO_MODEL

    def __init__(self, n_points, uv=None, n_inliers=None, best=None, flags=None, mean=None, cov=None, inliers=None, classes=None):
        super().__init__(uv=uv, n_inliers=n_inliers, best=best, flags=flags, mean=mean, cov=cov, inliers=inliers)
        self.n_points, self.classes = int(n_points), classes

    def inlier_mask(self):
        """bool [M, Kp, K]: voter j of a set agrees with the keypoint's position"""
        if self.inliers is None:
            raise RuntimeError("keypoint_vote: the `inliers` output was not asked for")
        return _record_set.bit_mask(self.inliers, self.n_points)

    def cov2x2(self):
        """float32 [M, Kp, 2, 2]: the covariance as a symmetric matrix"""
        if self.cov is None:
            raise RuntimeError("keypoint_vote: the `cov` output was not asked for")
        c = self.cov
        if isinstance(c, np.ndarray):
            return np.stack([c[..., 0], c[..., 1], c[..., 1], c[..., 2]], -1).reshape(c.shape[:-1] + (2, 2))
        return torch.stack([c[..., 0], c[..., 1], c[..., 1], c[..., 2]], -1).reshape(tuple(c.shape[:-1]) + (2, 2))

    def correspondences(self, bank, classes=None):
        """(uv [M, Kp, 2], xyz [M, Kp, 4]): every keypoint's position and its point of `bank` (a KeypointBank or a float32
        [A, Kp, 4] tensor) in the object frame, xyz.w = 1 where the keypoint was found and 0 elsewhere -- what
        sl.pose_pnp.solve(uv, xyz, ...) takes.  `classes`: the class of every set's object, integers [M]; default: what
        SceneBatch.keypoint_votes filled in."""
        if self.uv is None:
            raise RuntimeError("keypoint_vote: the `uv` output was not asked for")
        classes = self.classes if classes is None else classes
        if classes is None:
            raise TypeError("keypoint_vote: correspondences needs the class of every set (`classes`)")
        pts = bank.points if hasattr(bank, "points") else bank
        found = self.found
        if isinstance(self.uv, np.ndarray):
            pts = pts.cpu().numpy() if isinstance(pts, torch.Tensor) else np.asarray(pts, np.float32)
            xyz = pts[np.asarray(classes, np.int64)].astype(np.float32)
            xyz[..., 3] = found.astype(np.float32)
            return self.uv, xyz
        xyz = pts.to(self.uv.device)[torch.as_tensor(classes, device=self.uv.device).long()].clone()
        if tuple(xyz.shape[:2]) != tuple(self.uv.shape[:2]):
            raise ValueError("keypoint_vote: the bank holds %d keypoints per class, the votes %d" % (xyz.shape[1], self.uv.shape[1]))
        xyz[..., 3] = found.to(torch.float32)
        return self.uv, xyz.contiguous()


def _size_of(field, size):
    if size is not None:
        return int(size[0]), int(size[1])
    return (int(field.shape[2]), int(field.shape[1])) if field is not None else ANY_SIZE


def vote_host(pixel, field=None, scene=None, vectors=None, size=None, **kw):
    """slhip_keypoint_vote_host on host arrays: a KeypointVotes of numpy arrays.  pixel int16 [M, K, 2]; either `field` float32
    [B, H, W, Kp, 2] with `scene` int32 [M], or `vectors` float32 [M, K, Kp, 2]; `size` (W, H), default: the field's, or with
    vectors a picture that holds every pixel; `kw`: the other arguments of make_params.  Needs no device: the CPU tests' handle."""
    pixel = np.ascontiguousarray(pixel, np.int16)
    if pixel.ndim != 3 or pixel.shape[2] != 2:
        raise ValueError("keypoint_vote: pixel must be [M, K, 2]")
    M, K = pixel.shape[:2]
    if (field is None) == (vectors is None):
        raise TypeError("keypoint_vote: pass either `field` (with `scene`) or `vectors`")
    if field is not None:
        vec = np.ascontiguousarray(field, np.float32)
        if vec.ndim != 5 or vec.shape[4] != 2 or scene is None:
            raise ValueError("keypoint_vote: field must be [B, H, W, Kp, 2] and comes with `scene` [M]")
        sc = np.ascontiguousarray(scene, np.int32).reshape(M)
        Kp, B = vec.shape[3], vec.shape[0]
    else:
        vec = np.ascontiguousarray(vectors, np.float32)
        if vec.ndim != 4 or vec.shape[:2] != (M, K) or vec.shape[3] != 2:
            raise ValueError("keypoint_vote: vectors must be [%d, %d, Kp, 2]" % (M, K))
        sc, Kp, B = None, vec.shape[2], 0
    size = _size_of(vec if field is not None else None, size)
    if field is not None and (size[1], size[0]) != vec.shape[1:3]:
        raise ValueError("keypoint_vote: size %r is not the field's" % (size,))
    rec = check_params(make_params(size, M, K, Kp, **kw))
    res = KeypointVotes(K, **KeypointVotes.empty((M, Kp), int(rec["outputs"][0]), words=n_words(K)))
    st = _abi.lib().slhip_keypoint_vote_host(rec.ctypes.data, pixel.ctypes.data, vec.ctypes.data, None if sc is None else sc.ctypes.data,
                                             B, C.byref(res.record()))
    _abi.check(st, "slhip_keypoint_vote_host")
    return res


def vote(points_or_pixel, field=None, scene=None, vectors=None, size=None, **kw):
    """The position of every keypoint of every set of voters: a KeypointVotes.

    points_or_pixel  int16 [M, K, 2] pixels (x, y) on the device, or an ObjectPoints with its `pixel` output
    field            float32 [B, H, W, Kp, 2] on the device: a network's prediction in the layout of ObjectKeypoints.field;
                     voter j of set m is read at (scene[m], y, x) and nowhere else
    scene            integers [M], the picture of every set in `field`; default: the ObjectPoints' `scene`.  A scene outside
                     the field leaves its set without valid voters (`insufficient`)
    vectors          instead of field: float32 [M, K, Kp, 2] on the device, the vectors already gathered (networks on crops)
    size             (W, H) of the picture the pixels lie in; default: the field's, or with `vectors` one that holds every pixel
    kw               n_hypotheses=128, inlier_cos=0.99, min_inliers=2, min_sin=1e-3, outputs, seed, set_id_base

    Asynchronous on the current stream."""
    pixel = points_or_pixel
    if hasattr(points_or_pixel, "pixel") and hasattr(points_or_pixel, "records"):      # an ObjectPoints
        pixel = points_or_pixel.pixel
        if pixel is None:
            raise RuntimeError("keypoint_vote: the ObjectPoints need their `pixel` output")
        if scene is None and field is not None:
            scene = points_or_pixel.scene
    if (field is None) == (vectors is None):
        raise TypeError("keypoint_vote: pass either `field` (with `scene`) or `vectors`")
    if field is not None and scene is None:
        raise TypeError("keypoint_vote: a dense `field` needs the `scene` of every set")
    if field is None and scene is not None:
        raise TypeError("keypoint_vote: `scene` goes with a dense `field`")
    vec = field if field is not None else vectors
    tensors = [t for t in (pixel, vec, scene) if t is not None]
    dev = _device.require_cuda(NAME, tensors, "pixels, vectors and scenes", "pixels, vectors and scenes must be torch tensors")
    if pixel.dtype != torch.int16 or pixel.dim() != 3 or pixel.shape[2] != 2 or not pixel.is_contiguous():
        raise ValueError("keypoint_vote: pixel must be a contiguous int16 [M, K, 2] tensor")
    M, K = int(pixel.shape[0]), int(pixel.shape[1])
    if field is not None:
        if vec.dtype != torch.float32 or vec.dim() != 5 or vec.shape[4] != 2 or not vec.is_contiguous():
            raise ValueError("keypoint_vote: field must be a contiguous float32 [B, H, W, Kp, 2] tensor")
        B, Kp = int(vec.shape[0]), int(vec.shape[3])
        if scene.dim() != 1 or int(scene.shape[0]) != M or scene.dtype not in (torch.int16, torch.int32, torch.int64):
            raise ValueError("keypoint_vote: scene must be an integer [%d] tensor" % M)
        scene = scene.to(torch.int32).contiguous()
    else:
        if vec.dtype != torch.float32 or vec.dim() != 4 or tuple(vec.shape[:2]) != (M, K) or vec.shape[3] != 2 or not vec.is_contiguous():
            raise ValueError("keypoint_vote: vectors must be a contiguous float32 [%d, %d, Kp, 2] tensor" % (M, K))
        B, Kp = 0, int(vec.shape[2])
    size = _size_of(field, size)
    if field is not None and (size[1], size[0]) != tuple(vec.shape[1:3]):
        raise ValueError("keypoint_vote: size %r is not the field's" % (size,))
    rec = check_params(make_params(size, M, K, Kp, **kw))
    res = KeypointVotes(K, **KeypointVotes.empty((M, Kp), int(rec["outputs"][0]), dev, words=n_words(K)))
    out = res.record()
    with torch.cuda.device(dev):
        st = _abi.lib().slhip_keypoint_vote(rec.ctypes.data, C.c_void_p(pixel.data_ptr()), C.c_void_p(vec.data_ptr()),
                                            C.c_void_p(_device.ptr(scene)), B, C.byref(out), _device.stream_ptr(dev))
    _abi.check(st, "slhip_keypoint_vote")
    res._keepalive = (pixel, vec, scene)      # the launch is asynchronous: its inputs live as long as its outputs
    return res
