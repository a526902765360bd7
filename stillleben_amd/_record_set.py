"""What sl.object_crops and sl.object_points share: the record-set class behind ObjectCrops and ObjectPoints and the select step
of their extract() -- statistics (and mask records) to a compact array of records in ascending (scene, slot) order.  And what the
pose family shares (pose_fit, pose_icp, pose_pnp, pose_align, keypoint_vote, keypoint_vote3d): OutputSet, the class behind their
results, which derives the outputs' names, arrays and ctypes record from one table per module, and set_key, the seed of a
parameter record."""
import ctypes as C

import numpy as np
import torch

from . import _abi, _device


class RecordSet:
    """n records of a select pass and the tensors gathered for them.  `records`: int32 [n, words], scene and slot its first two
    words.  A subclass names its tensors in `_TENSORS` (records first) and one item in `_ITEM`, and builds an empty set of its
    kind round new records in `_like`."""
    _TENSORS = ("records",)
    _ITEM = "record"

    def __init__(self, records, scene_global=None, object_to_camera=None):
        self.records = records
        self.scene_global, self.object_to_camera = scene_global, object_to_camera
        self._keepalive = ()

    @property
    def scene(self):
        return self.records[..., 0]

    @property
    def slot(self):
        return self.records[..., 1]

    def map(self, fn):
        """A new set of the same kind with fn applied to every tensor (indexing, .cpu(), .clone(), ...)."""
        out = self._like(fn(self.records))
        for name in self._TENSORS[1:]:
            t = getattr(self, name)
            setattr(out, name, None if t is None else fn(t))
        out._keepalive = self._keepalive
        return out

    def __len__(self):
        if self.records.dim() != 2:
            raise TypeError("a single %s has no length" % self._ITEM)
        return self.records.shape[0]

    def __getitem__(self, i):
        """Item i (the leading dimension is dropped) or the items of a slice."""
        if self.records.dim() != 2:
            raise TypeError("a single %s cannot be indexed" % self._ITEM)
        if not isinstance(i, slice):
            i = range(len(self))[i]
        return self.map(lambda t: t[i])


def output_bits(outputs, known):
    """The bits of `outputs` (a name or names) among `known` = {name: bit}."""
    bits = 0
    for name in (outputs,) if isinstance(outputs, str) else outputs:
        if name not in known:
            raise ValueError("outputs: unknown %r (known: %s)" % (name, ", ".join(known)))
        bits |= known[name]
    return bits


def set_key(p, seed, id_base, base_field="scene_id_base"):
    """seed_lo, seed_hi and the id base (`base_field`) of a params record.  `seed`: an integer, or the (lo, hi) pair of a Philox
    key."""
    lo, hi = seed if isinstance(seed, (tuple, list)) else (int(seed), int(seed) >> 32)
    p["seed_lo"], p["seed_hi"], p[base_field] = int(lo) & 0xFFFFFFFF, int(hi) & 0xFFFFFFFF, int(id_base) & 0xFFFFFFFF


def rendered(name, buffers, need):
    """The targets of `buffers` that `need` = [(target, wanted), ...] wants; RuntimeError for one that was not rendered."""
    for target, wanted in need:
        if wanted and getattr(buffers, target, None) is None:
            raise RuntimeError("%s: the `%s` target was not rendered, and the requested outputs read it" % (name, target))
    return [getattr(buffers, target) for target, wanted in need if wanted]


def select(entry, rec, inputs, B, S, extra, words, dev):
    """The select step: `entry`(params, *inputs, B, S, *extra, records, capacity, scratch, n_out, stream) of the library with
    room for every slot but the background's.  Returns (int32 [n, words] records, the scratch to keep alive).  Synchronises the
    current stream once."""
    capacity = B * max(S - 1, 0)
    records = torch.empty((max(capacity, 1), words), dtype=torch.int32, device=dev)
    scratch = _device.scratch_for(entry.replace("_select", "_scratch_bytes"), dev, B)
    n_out = C.c_uint64(0)
    with torch.cuda.device(dev):
        st = getattr(_abi.lib(), entry)(rec.ctypes.data, *(C.c_void_p(t.data_ptr()) for t in inputs), B, S, *extra,
                                        C.c_void_p(records.data_ptr()), capacity, C.c_void_p(scratch.data_ptr()), C.byref(n_out),
                                        _device.stream_ptr(dev))
    _abi.check(st, entry)
    return records[:int(n_out.value)], scratch


def empty_outputs(n, bits, dev, spec):
    """{name: a tensor [n, *shape] for every (name, bit, shape, dtype) of `spec` whose bit is in `bits`, None for the others}"""
    return {name: torch.empty((n,) + shape, dtype=dtype, device=dev) if bits & bit else None for name, bit, shape, dtype in spec}


def n_words(K):
    """The 32-bit words of K bits."""
    return (int(K) + 31) // 32


def bit_mask(words, K):
    """bool [..., K] of uint32 words [..., n_words(K)] (numpy, or int32 on the device): bit j & 31 of word j >> 5."""
    if isinstance(words, np.ndarray):
        j = np.arange(K)
        return ((words.view(np.uint32)[..., j >> 5] >> (j & 31).astype(np.uint32)) & 1).astype(bool)
    j = torch.arange(K, device=words.device)
    return ((words[..., j >> 5] >> (j & 31).to(torch.int32)) & 1).bool()


_TORCH = {np.float32: torch.float32, np.int32: torch.int32, np.uint32: torch.int32}      # (bit words are int32 on the device)


class OutputSet:
    """The result of a pose-family module (pose_fit, pose_icp, pose_pnp, keypoint_vote, keypoint_vote3d): one optional array per
    output, torch tensors on the device or numpy arrays from the host twin; those not asked for are None.  A subclass states
        NAME    its module, for messages
        TABLE   ((name, bit of `outputs`, shape of one item, numpy dtype), ...) in the field order of RECORD; a dimension is a
                number or the name of a size that `empty` is given.  The first row is the result itself, NaN for an item without one
        RECORD  the ctypes record of the output pointers (_abi)
        FAILED  the bits of `flags` that leave an item without a result
    and gets OUTPUTS = {name: bit} from the table."""
    NAME, TABLE, RECORD, FAILED = "", (), None, 0

    def __init_subclass__(cls):
        if cls.RECORD is not None:
            assert [row[0] for row in cls.TABLE] == [f[0] for f in cls.RECORD._fields_], cls.NAME
        cls.OUTPUTS = {name: bit for name, bit, _, _ in cls.TABLE}

    def __init__(self, **outs):
        for name in self.OUTPUTS:
            setattr(self, name, outs.pop(name, None))
        if outs:
            raise TypeError("%s: unknown output %r" % (self.NAME, sorted(outs)[0]))
        self._keepalive = ()

    @classmethod
    def empty(cls, lead, bits, dev=None, **sizes):
        """{name: an array [*lead, *item shape] for every output of TABLE in `bits`}: numpy zeros, or torch tensors on `dev`."""
        outs = {}
        for name, bit, shape, dtype in cls.TABLE:
            if bits & bit:
                full = tuple(lead) + tuple(sizes[d] if isinstance(d, str) else d for d in shape)
                outs[name] = np.zeros(full, dtype) if dev is None else torch.empty(full, dtype=_TORCH[dtype], device=dev)
        return outs

    def record(self):
        """The ctypes record of the arrays' addresses, null for an output that is None."""
        def address(a):
            return None if a is None else a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()
        return self.RECORD(*(address(getattr(self, name)) for name in self.OUTPUTS))

    def __len__(self):
        for name in self.OUTPUTS:
            if getattr(self, name) is not None:
                return int(getattr(self, name).shape[0])
        return 0

    @property
    def found(self):
        """bool, one per item: it has a result.  Read from `flags` (no bit of FAILED), without them from `best` (-2: none),
        without both from the result itself (NaN: none)."""
        if self.flags is not None:
            return (self.flags & self.FAILED) == 0
        if getattr(self, "best", None) is not None:
            return self.best != -2
        name, _, shape, _ = self.TABLE[0]
        value = getattr(self, name)
        if value is None:
            reads = ", ".join("`%s`" % n for n in ("flags", "best", name) if n in self.OUTPUTS)
            raise RuntimeError("%s: `found` reads one of the outputs %s, and none of them was asked for" % (self.NAME, reads))
        first = value[(Ellipsis,) + (0,) * len(shape)]
        return first == first


class PoseSet(OutputSet):
    """An OutputSet with one `pose` float32 [M, 3, 4] per set."""

    def dense(self, B, O, scene, slot):
        """float32 [B, O, 3, 4]: the pose of set i at [scene[i], slot[i] - 1], NaN where a (scene, slot) has no set -- the shape
        SceneBatch.pose_errors and SceneBatch.pose_vsd take.  `slot` counts from 1 as the renders' instance indices do."""
        if self.pose is None:
            raise RuntimeError("%s: the `pose` output was not asked for" % self.NAME)
        if isinstance(self.pose, np.ndarray):
            out = np.full((int(B), int(O), 3, 4), np.nan, np.float32)
            out[np.asarray(scene, np.int64), np.asarray(slot, np.int64) - 1] = self.pose
            return out
        out = torch.full((int(B), int(O), 3, 4), float("nan"), dtype=torch.float32, device=self.pose.device)
        out[torch.as_tensor(scene, device=out.device).long(), torch.as_tensor(slot, device=out.device).long() - 1] = self.pose
        return out


class InlierPoseSet(PoseSet):
    """A PoseSet of sets of K correspondences with inlier bits (pose_pnp, pose_align); `n_points`: K."""

    def __init__(self, n_points, pose=None, n_inliers=None, rms=None, inliers=None, best=None, flags=None):
        super().__init__(pose=pose, n_inliers=n_inliers, rms=rms, inliers=inliers, best=best, flags=flags)
        self.n_points = int(n_points)

    def inlier_mask(self):
        """bool [M, K]: correspondence j of a set is an inlier of its pose"""
        if self.inliers is None:
            raise RuntimeError("%s: the `inliers` output was not asked for" % self.NAME)
        return bit_mask(self.inliers, self.n_points)
