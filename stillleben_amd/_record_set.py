"""What sl.object_crops and sl.object_points share: the record-set class behind ObjectCrops and ObjectPoints and the select step
of their extract() -- statistics (and mask records) to a compact array of records in ascending (scene, slot) order."""
import ctypes as C

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


def set_key(p, seed, scene_id_base):
    """seed_lo, seed_hi and scene_id_base of a params record.  `seed`: an integer, or the (lo, hi) pair of a Philox key."""
    lo, hi = seed if isinstance(seed, (tuple, list)) else (int(seed), int(seed) >> 32)
    p["seed_lo"], p["seed_hi"], p["scene_id_base"] = int(lo) & 0xFFFFFFFF, int(hi) & 0xFFFFFFFF, int(scene_id_base) & 0xFFFFFFFF


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
