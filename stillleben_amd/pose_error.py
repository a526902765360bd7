"""Pose errors -- this project's addition (the reference has no counterpart): ADD, ADD-S (PoseCNN, DenseFusion), BOP's MSSD and
MSPD of pose estimates against a batch's ground truth, with the symmetries of every class.  The arg-min of MSSD names the
symmetric equivalent of the ground truth nearest the estimate: the target of symmetry-aware losses (CosyPose, GDR-Net, EPOS).
Everything stays on the device, through two entries of include/slhip.h: slhip_pose_error_diameter (once per asset table) and
slhip_pose_error (all pairs and the symmetry sweep per scene, object and hypothesis).  There is no CPU path.

    sym = {3: sl.pose_error.symmetry_transforms(continuous=[{"axis": [0, 0, 1], "offset": [0, 0, 0]}])}
    bank = sl.pose_error.bank(table, n_points=1024, symmetries=sym)      # once: a ModelBank
    batch.place(object_to_camera=True)
    err = batch.pose_errors(estimates, bank)                             # estimates [B, O, Hy, 3, 4] or [B, O, 3, 4]
    err.add, err.adds, err.mssd, err.mspd, err.mssd_sym, err.mspd_sym
    err.add_auto(bank); err.recall("add", [0.1], bank); err.closest_gt(batch.object_to_camera, bank)

DESIGN.md "Pose errors" states the rules operation by operation."""
import ctypes as C
import math

import numpy as np
import torch

from . import _abi, _device

__all__ = ["OUTPUTS", "ModelBank", "PoseErrors", "make_params", "check_params", "sample_indices", "sample_points", "sample",
           "symmetry_transforms", "bank", "diameters", "diameter_host", "evaluate", "evaluate_host"]

NAME = "pose_error"
OUTPUTS = {"add": _abi.POSE_OUT_ADD, "adds": _abi.POSE_OUT_ADDS, "mssd": _abi.POSE_OUT_MSSD, "mspd": _abi.POSE_OUT_MSPD}


def output_mask(outputs):
    if isinstance(outputs, int):
        return outputs
    mask = 0
    for name in outputs:
        if name not in OUTPUTS:
            raise ValueError("outputs: unknown %r (known: %s)" % (name, ", ".join(OUTPUTS)))
        mask |= OUTPUTS[name]
    return mask


def make_params(intrinsics, n_objects, n_hypotheses, outputs=("add", "adds", "mssd", "mspd")):
    """One slhip_pose_error_params record (numpy).  `intrinsics`: (fx, fy, cx, cy) of MSPD; `outputs`: names or the bit mask."""
    p = np.zeros((), _abi.POSE_ERROR_PARAMS_DTYPE)
    p["fx"], p["fy"], p["cx"], p["cy"] = (np.float32(v) for v in intrinsics)
    p["n_objects"], p["n_hypotheses"], p["outputs"] = int(n_objects), int(n_hypotheses), output_mask(outputs)
    return p


def check_params(params):
    """Raises SlhipError when the record breaks a rule of slhip_pose_error_check_params.  Needs no device."""
    rec = np.ascontiguousarray(np.asarray(params, dtype=_abi.POSE_ERROR_PARAMS_DTYPE).reshape(1))
    _abi.check(_abi.lib().slhip_pose_error_check_params(rec.ctypes.data), "slhip_pose_error")
    return rec


# ---- the model bank --------------------------------------------------------------------------------------------------------------
class ModelBank:
    """One record per class, all tensors on one device:
        points      float32 [A, N, 4]  (x, y, z, 1) in the object frame (the frame of the `coord` target); zeros past count
        count       int32 [A]          1 <= count <= N <= 4096
        symmetries  float32 [A, S, 3, 4]  entry 0 of every class the identity, unused entries too
        n_sym       int32 [A]          1 <= n_sym <= S <= 1024
        diameter    float32 [A]        the largest distance between two of the class's points (BOP's `diameter`)"""

    def __init__(self, points, count, symmetries, n_sym, diameter=None):
        self.points, self.count, self.symmetries, self.n_sym, self.diameter = points, count, symmetries, n_sym, diameter
        A = int(points.shape[0]) if points.dim() == 3 else -1
        if points.dtype != torch.float32 or points.dim() != 3 or points.shape[2] != 4 or not points.is_contiguous():
            raise ValueError("ModelBank: points must be a contiguous float32 [A, N, 4] tensor")
        if (symmetries.dtype != torch.float32 or symmetries.dim() != 4 or tuple(symmetries.shape[2:]) != (3, 4)
                or symmetries.shape[0] != A or not symmetries.is_contiguous()):
            raise ValueError("ModelBank: symmetries must be a contiguous float32 [A, S, 3, 4] tensor")
        for t, what in ((count, "count"), (n_sym, "n_sym")):
            if t.dtype != torch.int32 or tuple(t.shape) != (A,) or not t.is_contiguous():
                raise ValueError("ModelBank: %s must be a contiguous int32 [A] tensor" % what)
        if not 1 <= points.shape[1] <= _abi.POSE_POINTS_MAX:
            raise ValueError("ModelBank: a class holds 1 to %d points, not %d" % (_abi.POSE_POINTS_MAX, points.shape[1]))
        if not 1 <= symmetries.shape[1] <= _abi.POSE_SYMMETRIES_MAX:
            raise ValueError("ModelBank: a class holds 1 to %d symmetries, not %d" % (_abi.POSE_SYMMETRIES_MAX, symmetries.shape[1]))

    def __len__(self):
        return int(self.points.shape[0])

    def tensors(self):
        return (self.points, self.count, self.symmetries, self.n_sym)

    def record(self):
        """the slhip_pose_bank record over the tensors' memory"""
        A, N, S = int(self.points.shape[0]), int(self.points.shape[1]), int(self.symmetries.shape[1])
        return _abi.PoseBank(self.points.data_ptr(), self.count.data_ptr(), self.symmetries.data_ptr(), self.n_sym.data_ptr(), A, N, S, 0)


def sample_indices(V, n):
    """The vertices a class of V vertices contributes to a bank row of n: all of them when V <= n, else vertex floor(k V / n)
    for k = 0 .. n-1 (integers)."""
    V, n = int(V), int(n)
    if V <= n:
        return np.arange(V, dtype=np.int64)
    return (np.arange(n, dtype=np.int64) * V) // n


def sample_points(positions, records, templates, n):
    """positions: float32 [V, 4] tensor (the pool's positions, any device); records, templates: the table's slhip_asset and
    slhip_draw records (numpy).  Returns (points float32 [A, N, 4], count int32 [A]) on the positions' device, N = the largest
    count: every class's sample_indices vertices under its mesh_to_object, rows ((m0 x + m1 y) + m2 z) + m3."""
    n = int(n)
    if not 1 <= n <= _abi.POSE_POINTS_MAX:
        raise ValueError("pose_error: n_points %d must be in [1, %d]" % (n, _abi.POSE_POINTS_MAX))
    dev, A = positions.device, len(records)
    picks = []
    for a in records:
        if int(a["draw_count"]) == 0 or int(a["n_verts"]) == 0 or int(a["draw_begin"]) >= len(templates):
            picks.append(np.zeros(0, np.int64))
            continue
        base, V = int(templates[int(a["draw_begin"])]["vtx_base"]), int(a["n_verts"])
        picks.append(base + sample_indices(V, n) if base + V <= positions.shape[0] else np.zeros(0, np.int64))
    N = max(1, max(len(p) for p in picks))
    points = torch.zeros((A, N, 4), dtype=torch.float32, device=dev)
    for c, (a, idx) in enumerate(zip(records, picks)):
        if not len(idx):
            continue
        v = positions[torch.from_numpy(idx).to(dev)]
        m = torch.from_numpy(np.ascontiguousarray(a["mesh_to_object"], dtype=np.float32).reshape(4, 4)).to(dev)
        x, y, z = v[:, 0], v[:, 1], v[:, 2]
        for r in range(3):
            points[c, :len(idx), r] = ((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3]
        points[c, :len(idx), 3] = 1.0
    count = torch.tensor([len(p) for p in picks], dtype=torch.int32, device=dev)
    return points, count


def sample(table, n):
    """sample_points of an sl.AssetTable on its device: (points float32 [A, N, 4], count int32 [A])."""
    eng, d_pos, _, _ = _device.table_on_device(table)
    return sample_points(d_pos.view(-1, 4), table.records, table.templates, n)


def _rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], np.float64)
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


def symmetry_transforms(discrete=(), continuous=(), max_step=0.01, scale=1.0, name=None):
    """One class's symmetry list, float32 [S, 3, 4], from the fields of BOP's models_info.json: `discrete` = symmetries_discrete
    (16 numbers each, row-major 4 x 4), `continuous` = symmetries_continuous ({"axis": .., "offset": ..}).  A continuous axis
    becomes n = ceil(pi / max_step) rotations by 2 pi k / n about it; with offset c the translation is c - R c.  The list is
    every product cont * disc (disc over the identity and the discrete ones, cont over the rotations), the identity first.
    Built in float64, rounded at the end.  Translations are multiplied by `scale` (0.001: BOP's millimetres into metres).
    More than 1024 entries raises a ValueError that names the class (`name`)."""
    if not max_step > 0:
        raise ValueError("pose_error: max_step must be positive")
    discs = [np.eye(4)]
    for d in discrete:
        m = np.asarray(d, np.float64).reshape(4, 4).copy()
        m[:3, 3] *= scale
        discs.append(m)
    conts = [np.eye(4)]
    for c in continuous:
        n = int(math.ceil(math.pi / max_step))
        axis, off = np.asarray(c["axis"], np.float64), np.asarray(c.get("offset", (0, 0, 0)), np.float64) * scale
        rots = []
        for k in range(n):
            m = np.eye(4)
            if k:
                m[:3, :3] = _rotation(axis, 2.0 * math.pi * k / n)
                m[:3, 3] = off - m[:3, :3] @ off
            rots.append(m)
        conts = [a @ r for a in conts for r in rots]
        if len(conts) * len(discs) > _abi.POSE_SYMMETRIES_MAX:
            break
    total = len(conts) * len(discs)
    if total > _abi.POSE_SYMMETRIES_MAX:
        raise ValueError("pose_error: class %s has more than %d symmetry transforms (%d discrete x %s rotations): raise max_step"
                         % ("?" if name is None else name, _abi.POSE_SYMMETRIES_MAX, len(discs), len(conts)))
    out = np.stack([(c @ d)[:3] for d in discs for c in conts]).astype(np.float32)
    return out


def _symmetry_tensor(A, symmetries, obj_ids, max_step, scale, dev):
    lists = [np.eye(4, dtype=np.float32)[None, :3] for _ in range(A)]
    if symmetries:
        for c in range(A):
            if obj_ids is not None:      # a models_info dict, keyed by object id (int or str)
                oid = obj_ids.get(c) if hasattr(obj_ids, "get") else obj_ids[c]
                info = symmetries.get(oid, symmetries.get(str(oid))) if oid is not None else None
                if info is not None:
                    lists[c] = symmetry_transforms(info.get("symmetries_discrete", ()), info.get("symmetries_continuous", ()),
                                                   max_step, scale, name="%d (object %s)" % (c, oid))
            elif c in symmetries:
                m = np.asarray(symmetries[c], np.float64)
                m = m.reshape(-1, 4, 4)[:, :3] if m.size % 16 == 0 and m.shape[-2:] != (3, 4) else m.reshape(-1, 3, 4)
                if len(m) > _abi.POSE_SYMMETRIES_MAX:
                    raise ValueError("pose_error: class %d has more than %d symmetry transforms: raise max_step" % (c, _abi.POSE_SYMMETRIES_MAX))
                if not len(m) or not np.array_equal(m[0], np.eye(4)[:3]):
                    m = np.concatenate([np.eye(4)[None, :3], m])      # entry 0 is the identity
                lists[c] = m.astype(np.float32)
    S = max(len(l) for l in lists)
    sym = np.tile(np.eye(4, dtype=np.float32)[:3], (A, S, 1, 1))
    for c, l in enumerate(lists):
        sym[c, :len(l)] = l
    n_sym = np.array([len(l) for l in lists], np.int32)
    return torch.from_numpy(sym).to(dev), torch.from_numpy(n_sym).to(dev)


def _bank_record(points, count, symmetries=None, n_sym=None):
    """(record, arrays kept alive) of host arrays"""
    points = np.ascontiguousarray(points, np.float32)
    A = points.shape[0]
    count = np.ascontiguousarray(count, np.int32).reshape(A)
    symmetries = np.tile(np.eye(4, dtype=np.float32)[:3], (A, 1, 1, 1)) if symmetries is None else np.ascontiguousarray(symmetries, np.float32)
    n_sym = np.ones(A, np.int32) if n_sym is None else np.ascontiguousarray(n_sym, np.int32).reshape(A)
    rec = _abi.PoseBank(points.ctypes.data, count.ctypes.data, symmetries.ctypes.data, n_sym.ctypes.data, A, points.shape[1],
                        symmetries.shape[1], 0)
    return rec, (points, count, symmetries, n_sym)


def diameter_host(points, count):
    """slhip_pose_error_diameter_host on host arrays (points float32 [A, N, 4], count [A]): float32 [A].  Needs no device."""
    rec, keep = _bank_record(points, count)
    out = np.zeros(rec.n_assets, np.float32)
    _abi.check(_abi.lib().slhip_pose_error_diameter_host(C.byref(rec), out.ctypes.data), "slhip_pose_error_diameter_host")
    return out


def diameters(model_bank):
    """The diameter of every class of a ModelBank on its device: float32 [A].  Asynchronous on the current stream."""
    dev = _device.require_cuda(NAME, model_bank.tensors(), "the bank's tensors")
    out = torch.empty((len(model_bank),), dtype=torch.float32, device=dev)
    rec = model_bank.record()
    with torch.cuda.device(dev):
        st = _abi.lib().slhip_pose_error_diameter(C.byref(rec), C.c_void_p(out.data_ptr()), _device.stream_ptr(dev))
    _abi.check(st, "slhip_pose_error_diameter")
    out._keepalive = model_bank.tensors()      # the launch is asynchronous
    return out


def bank(table, n_points=1024, symmetries=None, diameter=None, obj_ids=None, max_step=0.01, scale=1.0, points=None, count=None):
    """The ModelBank of an sl.AssetTable on its device.

    n_points    points per class (sample(table, n_points)); or pass `points` float32 [A, N, 4] and `count` int32 [A] device
                tensors of your own (the FPS points of sl.object_regions, say) -- `table` may then be None
    symmetries  None; a dict class index -> list of 4 x 4 (or 3 x 4) transforms in the table's unit; or, with `obj_ids` (class
                index -> object id), the dict of BOP's models_info.json, whose symmetries_discrete / symmetries_continuous go
                through symmetry_transforms(max_step=..., scale=...)
    diameter    None: computed on the device from the bank's points; or a dict class index -> value, or [A] values, that
                override it (a dataset's models_info diameter, in the table's unit)"""
    if points is None:
        points, count = sample(table, n_points)
    A, dev = int(points.shape[0]), points.device
    sym, n_sym = _symmetry_tensor(A, symmetries, obj_ids, max_step, scale, dev)
    out = ModelBank(points.contiguous(), count.to(torch.int32).contiguous(), sym, n_sym)
    if diameter is not None and not hasattr(diameter, "items"):
        out.diameter = torch.as_tensor(np.asarray(diameter, np.float32).reshape(A)).to(dev)
    else:
        out.diameter = diameters(out)
        for c, v in (diameter or {}).items():
            out.diameter[int(c)] = float(v)
    return out


# ---- the errors ------------------------------------------------------------------------------------------------------------------
class PoseErrors:
    """The errors of every (scene, object, hypothesis): float32 add, adds, mssd (the table's unit), mspd (pixels) and int32
    mssd_sym, mspd_sym, each [B, O, Hy] ([B, O] when the estimates had no hypothesis axis); those not asked for are None.
    +inf and -1: a class outside the bank or without points (and mspd with a point not in front of the camera); NaN and -1: an
    estimate that is not finite.  `classes`: int32 [B, O], the class of every object."""

    def __init__(self, classes, add=None, adds=None, mssd=None, mssd_sym=None, mspd=None, mspd_sym=None):
        self.classes = classes
        self.add, self.adds, self.mssd, self.mssd_sym, self.mspd, self.mspd_sym = add, adds, mssd, mssd_sym, mspd, mspd_sym
        self._keepalive = ()

    def _metric(self, name):
        v = getattr(self, name, None) if name in OUTPUTS else None
        if v is None:
            raise RuntimeError("pose_error: the `%s` output was not asked for" % name)
        return v

    def _per_class(self, values, like):
        """values [A] gathered by class and shaped to broadcast against `like`; (gathered, class inside the bank)"""
        cls = self.classes.long()
        inside = (cls >= 0) & (cls < values.shape[0])
        got = values[cls.clamp(0, values.shape[0] - 1)]
        while got.dim() < like.dim():
            got, inside = got[..., None], inside[..., None]
        return got, inside

    def add_auto(self, bank):
        """The usual "ADD(-S)": adds where the class has symmetries (n_sym > 1), add elsewhere."""
        add, adds = self._metric("add"), self._metric("adds")
        n_sym, inside = self._per_class(bank.n_sym, add)
        return torch.where(inside & (n_sym > 1), adds, add)

    def closest_gt(self, object_to_camera, bank):
        """float32 [B, O, Hy, 3, 4] = T_g S_{mssd_sym}: the symmetric equivalent of the ground truth nearest the estimate, the
        ground truth itself where the index is -1.  Plain torch."""
        if self.mssd_sym is None:
            raise RuntimeError("pose_error: closest_gt needs the `mssd` output")
        idx = self.mssd_sym.long()
        n_sym, inside = self._per_class(bank.n_sym, idx)
        cls = self.classes.long().clamp(0, len(bank) - 1)
        while cls.dim() < idx.dim():
            cls = cls[..., None]
        use = inside & (idx >= 0) & (idx < n_sym)
        S = bank.symmetries[cls.expand_as(idx), idx.clamp(0, bank.symmetries.shape[1] - 1)]      # [.., 3, 4]
        eye = torch.eye(4, dtype=torch.float32, device=S.device)[:3]
        S = torch.where(use[..., None, None], S, eye)
        g = object_to_camera
        while g.dim() < S.dim():
            g = g.unsqueeze(-3)
        R = g[..., :3] @ S[..., :3]
        t = g[..., :3] @ S[..., 3:] + g[..., 3:]
        return torch.cat([R, t], dim=-1)

    def recall(self, metric, thresholds, bank=None):
        """float32 [T]: the share of the finite entries of `metric` ("add", "adds", "mssd", "mspd") at or below each threshold;
        with `bank`, thresholds are fractions of the class's diameter (ADD's "0.1 d").  Plain torch."""
        v = self._metric(metric)
        thr = torch.as_tensor(thresholds, dtype=torch.float32, device=v.device).reshape(-1)
        thr = thr.view((-1,) + (1,) * v.dim())
        if bank is not None:
            d, inside = self._per_class(bank.diameter, v)
            thr = thr * torch.where(inside, d, torch.zeros_like(d))
        finite = torch.isfinite(v)
        hit = (v[None] <= thr) & finite[None]
        return hit.flatten(1).sum(dim=1).float() / finite.sum().clamp(min=1).float()


def _host_call(params, rec, classes, stride, gt, est, n_scenes, shape, mask):
    outs = {k: np.zeros(shape, np.float32) for k in ("add", "adds", "mssd", "mspd")}
    outs.update({k: np.zeros(shape, np.int32) for k in ("mssd_sym", "mspd_sym")})
    o = _abi.PoseErrorOut(*(outs[k].ctypes.data for k in ("add", "adds", "mssd", "mssd_sym", "mspd", "mspd_sym")))
    st = _abi.lib().slhip_pose_error_host(params.ctypes.data, C.byref(rec), classes.ctypes.data, stride, gt.ctypes.data,
                                          est.ctypes.data, n_scenes, C.byref(o))
    _abi.check(st, "slhip_pose_error_host")
    named = {"add": ("add",), "adds": ("adds",), "mssd": ("mssd", "mssd_sym"), "mspd": ("mspd", "mspd_sym")}
    return {k: outs[k] for name, bit in OUTPUTS.items() if mask & bit for k in named[name]}


def evaluate_host(object_to_camera, estimates, classes, points, count, symmetries, n_sym, intrinsics,
                  outputs=("add", "adds", "mssd", "mspd")):
    """slhip_pose_error_host on host arrays: a dict of the outputs asked for, each [B, O, Hy].  classes int32 [B, O];
    object_to_camera [B, O, 3, 4]; estimates [B, O, Hy, 3, 4].  Needs no device: the CPU tests' handle."""
    gt = np.ascontiguousarray(object_to_camera, np.float32)
    est = np.ascontiguousarray(estimates, np.float32)
    B, O, Hy = est.shape[:3]
    cls = np.ascontiguousarray(classes, np.int32).reshape(B, O)
    rec, keep = _bank_record(points, count, symmetries, n_sym)
    p = make_params(intrinsics, O, Hy, outputs).reshape(1)
    return _host_call(p, rec, cls, 1, gt, est, B, (B, O, Hy), int(p["outputs"][0]))


def evaluate(object_to_camera, estimates, objects, bank, intrinsics, outputs=("add", "adds", "mssd", "mspd")):
    """The errors of pose estimates against the ground truth: a PoseErrors.

    object_to_camera  float32 [B, O, 3, 4] on the device (SceneBatch.place(object_to_camera=True))
    estimates         float32 [B, O, Hy, 3, 4], or [B, O, 3, 4] (one hypothesis; the outputs lose that axis again)
    objects           the slhip_synth_object records of the B * O objects as a uint8 device tensor (SceneBatch.d_objects), read
                      in place, or the class of every object as an integer tensor [B, O]
    bank              a ModelBank (sl.pose_error.bank(table, ...))
    intrinsics        (fx, fy, cx, cy) of MSPD
    outputs           names among "add", "adds", "mssd", "mspd"

    Asynchronous on the current stream."""
    if not isinstance(bank, ModelBank):
        raise TypeError("pose_error: `bank` must be a ModelBank (sl.pose_error.bank(table, ...))")
    o2c, est = object_to_camera, estimates
    dev = _device.require_cuda(NAME, (o2c, est) + bank.tensors(), "object_to_camera, estimates and the bank",
                               "object_to_camera and estimates must be torch tensors")
    if o2c.dtype != torch.float32 or o2c.dim() != 4 or tuple(o2c.shape[2:]) != (3, 4) or not o2c.is_contiguous():
        raise ValueError("pose_error: object_to_camera must be a contiguous float32 [B, O, 3, 4] tensor")
    B, O = int(o2c.shape[0]), int(o2c.shape[1])
    squeeze = est.dim() == 4
    if squeeze:
        est = est[:, :, None]
    if (est.dtype != torch.float32 or est.dim() != 5 or tuple(est.shape[:2]) != (B, O) or tuple(est.shape[3:]) != (3, 4)
            or not est.is_contiguous()):
        raise ValueError("pose_error: estimates must be a contiguous float32 [%d, %d, Hy, 3, 4] (or [%d, %d, 3, 4]) tensor" % (B, O, B, O))
    Hy = int(est.shape[2])
    if isinstance(objects, torch.Tensor) and objects.dtype in (torch.int16, torch.int64):
        objects = objects.to(torch.int32).contiguous()
    keep, p_classes, stride, O_ = _device.object_classes(NAME, objects, B, dev, O)
    if O_ != O:
        raise ValueError("pose_error: `objects` holds %d objects per scene, object_to_camera %d" % (O_, O))
    classes = _device.class_tensor(keep, O)[:B] if keep.dtype == torch.uint8 else keep
    rec = check_params(make_params(intrinsics, O, Hy, outputs))
    mask = int(rec["outputs"][0])
    shape = (B, O, Hy)

    def new(bit, dtype):
        return torch.empty(shape, dtype=dtype, device=dev) if mask & bit else None

    res = PoseErrors(classes, new(_abi.POSE_OUT_ADD, torch.float32), new(_abi.POSE_OUT_ADDS, torch.float32),
                     new(_abi.POSE_OUT_MSSD, torch.float32), new(_abi.POSE_OUT_MSSD, torch.int32),
                     new(_abi.POSE_OUT_MSPD, torch.float32), new(_abi.POSE_OUT_MSPD, torch.int32))
    names = ("add", "adds", "mssd", "mssd_sym", "mspd", "mspd_sym")
    if B:
        out = _abi.PoseErrorOut(*(_device.ptr(getattr(res, k)) for k in names))
        brec = bank.record()
        with torch.cuda.device(dev):
            st = _abi.lib().slhip_pose_error(rec.ctypes.data, C.byref(brec), C.c_void_p(p_classes), stride, C.c_void_p(o2c.data_ptr()),
                                             C.c_void_p(est.data_ptr()), B, C.byref(out), _device.stream_ptr(dev))
        _abi.check(st, "slhip_pose_error")
    if squeeze:
        for k in names:
            if getattr(res, k) is not None:
                setattr(res, k, getattr(res, k)[:, :, 0])
    res._keepalive = (o2c, est, keep) + bank.tensors()      # the launch is asynchronous: its inputs live as long as its outputs
    return res
