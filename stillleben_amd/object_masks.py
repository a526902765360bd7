"""sl.ObjectMasks: per-object masks of a render (slhip_render_object_masks, include/slhip.h) -- of every object the whole
silhouette as if nothing occluded it (kind "all", BOP's mask/) and the visible part (kind "visib", BOP's mask_visib/).

Slot i of a scene is instance index i; slot 0 (the background plane, unindexed draws) is always empty.  Both kinds live on the
device in two forms:
    bit tiles    .words, one int64 word per 8 x 8-pixel tile of a slot's tile box, laid out by .records; dense() expands them
    run lengths  .runs, int32: COCO's uncompressed RLE ({"counts": [...], "size": [H, W]}, what the BOP toolkit writes into
                 scene_gt_coco.json and pycocotools accepts); rle() / rles() copy a mask's or a scene's lengths to the host

The RLE in executable form -- rle_encode() / rle_decode(), plain numpy on the host: the mask is read column by column (pixel
(x, y) at position x * H + y), `counts` are the lengths of the runs of zeros and ones in turn, zeros first (a first count of 0
when pixel (0, 0) is set); they sum to H * W, and an empty mask is [H * W]."""
import ctypes as C

import numpy as np
import torch

from . import _abi, _device

KINDS = {"all": 0, "visib": 1}


def rle_encode(mask):
    """{"counts": [int, ...], "size": [H, W]} of a 2-D mask (anything numpy reads as [H, W]; non-zero = set)."""
    m = np.asarray(mask)
    if m.ndim != 2:
        raise ValueError("rle_encode needs a 2-D mask [H, W]")
    H, W = m.shape
    flat = np.concatenate([[0], (m != 0).ravel(order="F").astype(np.int8)])      # the run of zeros that opens every RLE
    edges = np.flatnonzero(flat[1:] != flat[:-1])                                # positions whose pixel differs from the one before
    bounds = np.concatenate([[0], edges, [H * W]])
    return {"counts": [int(v) for v in np.diff(bounds)], "size": [int(H), int(W)]}


def rle_decode(rle):
    """bool [H, W] of {"counts": [...], "size": [H, W]}."""
    H, W = (int(v) for v in rle["size"])
    counts = np.asarray(rle["counts"], dtype=np.int64)
    if counts.ndim != 1 or (counts < 0).any() or int(counts.sum()) != H * W:
        raise ValueError("counts must be non-negative and sum to H * W = %d" % (H * W))
    values = (np.arange(len(counts)) & 1).astype(bool)
    return np.repeat(values, counts).reshape((H, W), order="F")


def _kind(kind):
    if kind not in KINDS:
        raise ValueError("kind must be 'all' (the whole silhouette) or 'visib' (the visible part), not %r" % (kind,))
    return KINDS[kind]


class ObjectMasks:
    """stats    the ObjectStats of the same call
    records  int32 [B, S, 14]: the device view of the slhip_object_mask array (host_records() gives it with field names)
    words    int64 [...]: the bit tiles of both kinds
    runs     int32 [...]: the run lengths of both kinds
    size     (H, W);  n_slots  S
    A single scene's view (RenderPassResult.object_masks(), masks[b]) drops the scene argument and dimension everywhere."""

    def __init__(self, stats, records, words, runs, size, single=False):
        self.stats = stats
        self.records = records
        self.words = words
        self.runs = runs
        self.size = (int(size[0]), int(size[1]))
        self._single = bool(single)
        self._host = None

    @property
    def n_slots(self):
        return self.records.shape[-2]

    @property
    def n_scenes(self):
        return 1 if self._single else self.records.shape[0]

    def __getitem__(self, b):
        """The masks of scene b as a single scene's view (the pools are shared, nothing is copied)."""
        if self._single:
            raise TypeError("a single scene's masks have no scene index")
        b = range(self.n_scenes)[b]
        return ObjectMasks(self.stats[b], self.records[b], self.words, self.runs, self.size, single=True)

    def host_records(self):
        """The records on the host, a numpy array [B, S] of _abi.OBJECT_MASK_DTYPE (copied once and kept)."""
        if self._host is None:
            raw = self.records.detach().cpu().contiguous().numpy()
            self._host = raw.view(_abi.OBJECT_MASK_DTYPE).reshape(-1, self.n_slots)
        return self._host

    # ---- dense masks ---------------------------------------------------------------------------------------------------
    def dense(self, kind="visib", scenes=None, slots=None):
        """torch.bool [len(scenes), len(slots), H, W] on the device (slhip_object_masks_expand; [len(slots), H, W] for a single
        scene's view).  Defaults: all scenes, slots 1..S-1.  One byte per pixel and mask: asking for everything costs
        B * (S - 1) * H * W bytes per kind -- 1.6 GB for 256 scenes of 20 objects at 640 x 480 -- so select."""
        k = _kind(kind)
        if self._single:
            if scenes is not None:
                raise TypeError("a single scene's masks take no `scenes`")
            scenes = [0]
        elif scenes is None:
            scenes = range(self.n_scenes)
        scenes = [int(s) for s in scenes]
        slots = [int(s) for s in (range(1, self.n_slots) if slots is None else slots)]
        for s in scenes:
            if not 0 <= s < self.n_scenes:
                raise IndexError("scene %d of %d" % (s, self.n_scenes))
        for s in slots:
            if not 0 <= s < self.n_slots:
                raise IndexError("slot %d of %d" % (s, self.n_slots))
        H, W = self.size
        if not self.words.is_cuda:
            raise RuntimeError("dense() runs on the device: these masks live on the host")
        dev = self.words.device
        out = torch.empty((len(scenes), len(slots), H, W), dtype=torch.uint8, device=dev)
        if out.numel():
            sel = np.array([(b, i) for b in scenes for i in slots], dtype=np.uint32)
            d_sel = torch.from_numpy(sel.view(np.int32)).to(dev)
            with torch.cuda.device(dev):
                st = _abi.lib().slhip_object_masks_expand(C.c_void_p(self.records.data_ptr()), C.c_void_p(self.words.data_ptr()),
                                                          self.n_scenes, self.n_slots, W, H, k, C.c_void_p(d_sel.data_ptr()),
                                                          len(sel), C.c_void_p(out.data_ptr()), _device.stream_ptr(dev))
            _abi.check(st, "slhip_object_masks_expand")
        out = out.view(torch.bool)
        return out[0] if self._single else out

    # ---- run lengths ---------------------------------------------------------------------------------------------------
    def _args(self, args, n, what):
        if len(args) != n - (1 if self._single else 0):
            raise TypeError("%s of %s" % (what, "a single scene's view takes no scene index" if self._single else "batched masks needs a scene index"))
        return ((0,) + tuple(args)) if self._single else tuple(args)

    def rle(self, *args, kind="visib"):
        """rle(b, i, kind) -- rle(i, kind) for a single scene's view: {"counts": [int, ...], "size": [H, W]} of slot i of scene b
        on the host; only that mask's run lengths are copied."""
        if args and isinstance(args[-1], str):
            kind, args = args[-1], args[:-1]
        b, i = self._args(args, 2, "rle()")
        k = _kind(kind)
        r = self.host_records()[range(self.n_scenes)[b], range(self.n_slots)[i]]
        o, n = int(r["rle_offset"][k]), int(r["rle_count"][k])
        return {"counts": self.runs[o:o + n].cpu().tolist(), "size": list(self.size)}

    def rles(self, *args, kind="visib"):
        """rles(b, kind) -- rles(kind) for a single scene's view: the RLEs of slots 1..S-1 of scene b, with a single copy (the
        scene's run lengths of both kinds lie in one piece of the pool)."""
        if args and isinstance(args[-1], str):
            kind, args = args[-1], args[:-1]
        (b,) = self._args(args, 1, "rles()")
        k = _kind(kind)
        rec = self.host_records()[range(self.n_scenes)[b]]
        if self.n_slots < 2:
            return []
        lo = int(rec[1]["rle_offset"][0])
        hi = int(rec[-1]["rle_offset"][1]) + int(rec[-1]["rle_count"][1])
        piece = self.runs[lo:hi].cpu().numpy()
        out = []
        for i in range(1, self.n_slots):
            o, n = int(rec[i]["rle_offset"][k]) - lo, int(rec[i]["rle_count"][k])
            out.append({"counts": piece[o:o + n].tolist(), "size": list(self.size)})
        return out

    def __repr__(self):
        return "ObjectMasks(%s%d slots, %d x %d)" % ("" if self._single else "%d scenes, " % self.n_scenes, self.n_slots,
                                                      self.size[1], self.size[0])
