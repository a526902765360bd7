"""ICP pose refinement -- this project's addition (the reference has no counterpart): the pose of every set of K camera points
refined against the points of its class in a model bank, point to point, from an initial pose -- the step that DenseFusion, PVN3D,
FFB6D, PoseCNN+ICP and the BOP baselines run after their estimate.  Per iteration: every camera point goes into the object frame
of the current pose and takes the nearest bank point (the walk of the pose errors' ADD-S), then Horn's closed-form fit of the
pairs (sl.pose_fit's rules, unchanged) gives the new absolute pose.  Everything stays on the device, through one entry of
include/slhip.h: slhip_pose_icp, one workgroup per set with the class's points in LDS.  There is no CPU path; `solve_host` runs the
library's host twin of the same rules for tests and needs no device.

    surf = sl.pose_vsd.surface(table)
    pts, cnt = sl.pose_icp.surface_points(surf, 2048)                     # vertex banks are useless on low-poly classes
    bank = sl.pose_error.bank(table, points=pts, count=cnt)               # once: a ModelBank
    icp = batch.pose_icp(points, fit, bank, max_dist=0.05)                # or sl.pose_icp.solve(camera, init, classes, bank)
    icp.pose, icp.n_pairs, icp.rms, icp.iters, icp.flags, icp.nearest, icp.found, icp.converged
    err = batch.pose_errors(icp.dense(B, O, points.scene_global, points.slot), bank)

DESIGN.md "ICP" states the rules operation by operation."""
import ctypes as C

import numpy as np
import torch

from . import _abi, _device, _record_set
from . import pose_error as _pe

__all__ = ["OUTPUTS", "FLAGS", "FAILED", "PoseICP", "make_params", "check_params", "solve", "solve_host", "surface_points"]

NAME = "pose_icp"
FLAGS = {"bad_class": _abi.ICP_BAD_CLASS, "no_init": _abi.ICP_NO_INIT, "insufficient": _abi.ICP_INSUFFICIENT,
         "degenerate": _abi.ICP_DEGENERATE, "converged": _abi.ICP_CONVERGED}
FAILED = _abi.ICP_FAILED      # the failure bits: every flag but `converged`


class PoseICP(_record_set.PoseSet):
    """The refined pose of every set (torch tensors on the device from `solve`, numpy arrays from `solve_host`; those not asked
    for are None):
        pose     float32 [M, 3, 4] object to camera       n_pairs  int32 [M] the pairs of the last association
        rms      float32 [M] root mean square of |R p + t - c| over the pairs of the last fit, in the unit of the points
        iters    int32 [M] the fits done                   flags    int32 [M] bits of FLAGS
        nearest  int32 [M, K] the bank point every camera point was paired with in the last association, -1 without a pair
        found    bool [M]: the set has a pose (no failure bit)
    A set whose class lies outside the bank (`bad_class`), whose initial pose is not finite (`no_init`), with fewer than
    min_pairs pairs (`insufficient`) or whose pairs' bank points are collinear or coincident (`degenerate`) has a NaN pose and
    rms -- never an identity pose, never the initial one.  `converged` is not a failure."""
    NAME, RECORD, FAILED = NAME, _abi.PoseIcpOut, FAILED
    TABLE = (("pose", _abi.ICP_OUT_POSE, (3, 4), np.float32), ("n_pairs", _abi.ICP_OUT_N_PAIRS, (), np.int32),
             ("rms", _abi.ICP_OUT_RMS, (), np.float32), ("iters", _abi.ICP_OUT_ITERS, (), np.int32),
             ("flags", _abi.ICP_OUT_FLAGS, (), np.int32), ("nearest", _abi.ICP_OUT_NEAREST, ("K",), np.int32))

    def __init__(self, pose=None, n_pairs=None, rms=None, iters=None, flags=None, nearest=None):
        super().__init__(pose=pose, n_pairs=n_pairs, rms=rms, iters=iters, flags=flags, nearest=nearest)

    @property
    def converged(self):
        """bool [M]: the loop ended because the pose stood still"""
        if self.flags is None:
            raise RuntimeError("pose_icp: `converged` reads the `flags` output, which was not asked for")
        return (self.flags & _abi.ICP_CONVERGED) != 0


OUTPUTS = PoseICP.OUTPUTS
_ALL = tuple(OUTPUTS)


def make_params(n_sets, n_points, max_iters=20, max_dist=float("inf"), dist_scale=1.0, min_dist=0.0, min_pairs=6, min_gap=1e-6,
                tol_rot=1e-6, tol_trans=1e-6, outputs=_ALL):
    """One slhip_pose_icp_params record (numpy).
        max_iters   1..64 fits at the most
        max_dist    the gate of the first association: a pair counts when its distance is at most the gate; +inf: no gate
        dist_scale  in (0, 1]: after every fit the gate becomes max(gate * dist_scale, min_dist)
        min_pairs   >= 3: fewer pairs make the set `insufficient`
        min_gap     sl.pose_fit's: the pairs' bank points are `degenerate` (collinear, coincident) below it
        tol_rot, tol_trans   the loop ends (`converged`) when no rotation entry moved by more than tol_rot and no translation
                    entry by more than tol_trans
    Every default is a convenience, not a measured value.  `outputs`: names or the bit mask."""
    p = np.zeros((), _abi.POSE_ICP_PARAMS_DTYPE)
    p["n_sets"], p["n_points"], p["max_iters"], p["min_pairs"] = int(n_sets), int(n_points), int(max_iters), int(min_pairs)
    p["max_dist"], p["dist_scale"], p["min_dist"] = np.float32(max_dist), np.float32(dist_scale), np.float32(min_dist)
    p["min_gap"], p["tol_rot"], p["tol_trans"] = np.float32(min_gap), np.float32(tol_rot), np.float32(tol_trans)
    p["outputs"] = outputs if isinstance(outputs, int) else _record_set.output_bits(outputs, OUTPUTS)
    return p


def check_params(params):
    """Raises SlhipError when the record breaks a rule of slhip_pose_icp_check_params.  Needs no device."""
    rec = np.ascontiguousarray(np.asarray(params, dtype=_abi.POSE_ICP_PARAMS_DTYPE).reshape(1))
    _abi.check(_abi.lib().slhip_pose_icp_check_params(rec.ctypes.data), "slhip_pose_icp")
    return rec


def solve_host(camera, init, classes, bank, **kw):
    """slhip_pose_icp_host on host arrays: a PoseICP of numpy arrays.  camera float32 [M, K, 4], init float32 [M, 3, 4], classes
    int32 [M], bank = (points float32 [A, N, 4], count int32 [A]); `kw`: the other arguments of make_params.  Needs no device:
    the CPU tests' handle."""
    camera = np.ascontiguousarray(camera, np.float32)
    if camera.ndim != 3 or camera.shape[2] != 4:
        raise ValueError("pose_icp: camera must be [M, K, 4]")
    M, K = camera.shape[:2]
    init = np.ascontiguousarray(init, np.float32)
    if init.shape != (M, 3, 4):
        raise ValueError("pose_icp: init must be [%d, 3, 4]" % M)
    classes = np.ascontiguousarray(classes, np.int32)
    if classes.shape != (M,):
        raise ValueError("pose_icp: classes must be [%d]" % M)
    points, count = bank
    points = np.asarray(points, np.float32)
    if points.ndim != 3 or points.shape[2] != 4:
        raise ValueError("pose_icp: the bank's points must be [A, N, 4]")
    brec, keep = _pe._bank_record(points, count)
    rec = check_params(make_params(M, K, **kw))
    res = PoseICP(**PoseICP.empty((M,), int(rec["outputs"][0]), K=K))
    if M:
        _abi.check(_abi.lib().slhip_pose_icp_host(rec.ctypes.data, camera.ctypes.data, init.ctypes.data, classes.ctypes.data, C.byref(brec),
                                                  C.byref(res.record())), "slhip_pose_icp_host")
    return res


def solve(camera, init, classes, bank, **kw):
    """The refined pose of every set of camera points: a PoseICP.

    camera   float32 [M, K, 4] on the device, the layout of ObjectPoints.camera: a point counts when its w != 0 and x, y, z are
             finite
    init     float32 [M, 3, 4] on the device: the initial pose of every set, object to camera
    classes  int32 [M] on the device: the class of every set's object, a row of the bank
    bank     a ModelBank (sl.pose_error.bank(table, ...)); its symmetries are not read
    kw       max_iters=20, max_dist=inf, dist_scale=1, min_dist=0, min_pairs=6, min_gap=1e-6, tol_rot=1e-6, tol_trans=1e-6
             (conveniences, not measured values), outputs

    Asynchronous on the current stream; the result keeps its inputs alive."""
    if not isinstance(bank, _pe.ModelBank):
        raise TypeError("pose_icp: `bank` must be a ModelBank (sl.pose_error.bank(table, ...))")
    dev = _device.require_cuda(NAME, (camera, init, classes) + bank.tensors(), "camera, init, classes and the bank",
                               "camera, init and classes must be torch tensors")
    if camera.dtype != torch.float32 or camera.dim() != 3 or camera.shape[2] != 4 or not camera.is_contiguous():
        raise ValueError("pose_icp: camera must be a contiguous float32 [M, K, 4] tensor")
    M, K = int(camera.shape[0]), int(camera.shape[1])
    if init.dtype != torch.float32 or tuple(init.shape) != (M, 3, 4) or not init.is_contiguous():
        raise ValueError("pose_icp: init must be a contiguous float32 [%d, 3, 4] tensor" % M)
    if classes.dtype != torch.int32 or tuple(classes.shape) != (M,) or not classes.is_contiguous():
        raise ValueError("pose_icp: classes must be a contiguous int32 [%d] tensor" % M)
    rec = check_params(make_params(M, K, **kw))
    res = PoseICP(**PoseICP.empty((M,), int(rec["outputs"][0]), dev, K=K))
    if M:
        out = res.record()
        brec = bank.record()
        with torch.cuda.device(dev):
            st = _abi.lib().slhip_pose_icp(rec.ctypes.data, C.c_void_p(camera.data_ptr()), C.c_void_p(init.data_ptr()),
                                           C.c_void_p(classes.data_ptr()), C.byref(brec), C.byref(out), _device.stream_ptr(dev))
        _abi.check(st, "slhip_pose_icp")
    res._keepalive = (camera, init, classes) + bank.tensors()      # the launch is asynchronous: its inputs live as long as its outputs
    return res


# ---- surface-sampled banks -------------------------------------------------------------------------------------------------------
_PLASTIC = 1.32471795724474602596      # the real root of x^3 = x + 1: the generator of the R2 low-discrepancy sequence


def surface_points(surface, n_points):
    """(points float32 [A, n, 4], count int32 [A]) on the surface's device: n = n_points points on the triangles of every class
    of a SurfaceBank (sl.pose_vsd.surface(table)), for sl.pose_error.bank(table, points=..., count=...).  A vertex bank is
    useless for ICP on a low-poly class (a box has 8 vertices); this one covers the faces.

    The rule, deterministic and unseeded (float64 on the host, rounded to float32 at the end; set-up work, once per table):
      * the triangles of a class in their order, area_t = |(v1 - v0) x (v2 - v0)| / 2, cum_t = area_0 + ... + area_t;
      * sample k = 0 .. n-1 takes the first triangle t with cum_t > (k + 0.5) / n * cum_last (stratified: triangle t gets
        n * area_t / cum_last samples to within 1; a triangle without area gets none);
      * (r1, r2) = the fractional parts of 0.5 + (k + 1) / g and 0.5 + (k + 1) / g^2, g = 1.3247179572447460 (the R2
        sequence), s = sqrt(r1), barycentrics (1 - s, s (1 - r2), s r2): uniform over the triangle (the square-root map);
      * the point is b0 v0 + b1 v1 + b2 v2, its w is 1.
    A class without triangles, or whose triangles have no area, has count 0 and a row of zeros."""
    n = int(n_points)
    if not 1 <= n <= _abi.POSE_POINTS_MAX:
        raise ValueError("pose_icp: n_points %d must be in [1, %d]" % (n, _abi.POSE_POINTS_MAX))
    dev = surface.vertices.device
    verts = surface.vertices.detach().cpu().numpy().astype(np.float64)[:, :3]
    tris = surface.triangles.detach().cpu().numpy().astype(np.int64)
    begin, cnt = surface.tri_begin.detach().cpu().numpy(), surface.tri_count.detach().cpu().numpy()
    A = len(begin)
    points, count = np.zeros((A, n, 4), np.float32), np.zeros(A, np.int32)
    k = np.arange(n, dtype=np.float64)
    r1, r2 = np.modf(0.5 + (k + 1.0) / _PLASTIC)[0], np.modf(0.5 + (k + 1.0) / (_PLASTIC * _PLASTIC))[0]
    s = np.sqrt(r1)
    b = np.stack([1.0 - s, s * (1.0 - r2), s * r2], 1)      # [n, 3]
    for a in range(A):
        t = tris[int(begin[a]):int(begin[a]) + int(cnt[a])]
        if not len(t):
            continue
        v = verts[t]      # [T, 3, 3]
        cum = np.cumsum(0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1))
        if not cum[-1] > 0.0 or not np.isfinite(cum[-1]):
            continue
        pick = np.minimum(np.searchsorted(cum, (k + 0.5) / n * cum[-1], side="right"), len(t) - 1)
        points[a, :, :3] = (b[:, :, None] * v[pick]).sum(1)
        points[a, :, 3] = 1.0
        count[a] = n
    return torch.from_numpy(points).to(dev), torch.from_numpy(count).to(dev)
