"""sl.ObjectStats: per-object visibility statistics of a render (slhip_render_object_stats, include/slhip.h) -- the numbers the
BOP toolkit records in scene_gt_info for every object of every picture.

Slot i of a scene is instance index i; slot 0 (the background plane, unindexed draws) is always empty.
    px_count_visib  int32 [B, S]     pixels whose instance output is i
    px_count_all    int32 [B, S]     pixels the visibility pass covers with object i drawn alone (same camera and viewport)
    bbox_visib      int32 [B, S, 4]  (x, y, w, h) of the visible pixels, (-1, -1, -1, -1) when there are none
    bbox_obj        int32 [B, S, 4]  (x, y, w, h) of the whole silhouette
    visib_fract     float32 [B, S]   px_count_visib / px_count_all, 0.0 when px_count_all == 0 (BOP's rule)
"""
import torch

_FIELDS = ("px_count_visib", "px_count_all", "bbox_visib", "bbox_obj", "visib_fract")


class ObjectStats:
    def __init__(self, px_count_visib, px_count_all, bbox_visib, bbox_obj, visib_fract=None):
        self.px_count_visib = px_count_visib
        self.px_count_all = px_count_all
        self.bbox_visib = bbox_visib
        self.bbox_obj = bbox_obj
        if visib_fract is None:
            visib_fract = self.fraction(px_count_visib, px_count_all)
        self.visib_fract = visib_fract

    @staticmethod
    def fraction(visib, all_):
        """float32 visib / all, 0.0 where all == 0."""
        a = all_.to(torch.float32)
        return torch.where(all_ > 0, visib.to(torch.float32) / torch.where(all_ > 0, a, torch.ones_like(a)), torch.zeros_like(a))

    @classmethod
    def from_records(cls, rec):
        """From the int32 [B, S, 10] view of slhip_object_stats records (px_visib, px_all, bbox_visib[4], bbox_obj[4])."""
        return cls(rec[..., 0], rec[..., 1], rec[..., 2:6], rec[..., 6:10])

    def records(self):
        """int32 [B, S, 10]: the slhip_object_stats array of batched statistics (assembled on their device, 40 bytes per slot)."""
        pv, pa, bv, bo = self.px_count_visib, self.px_count_all, self.bbox_visib, self.bbox_obj
        if pv.dim() != 2:
            raise ValueError("object_crops: batched statistics [B, S] expected, got %s" % (tuple(pv.shape),))
        return torch.cat([pv.unsqueeze(-1), pa.unsqueeze(-1), bv, bo], dim=-1).to(torch.int32).contiguous()

    @property
    def n_slots(self):
        return self.px_count_all.shape[-1]

    def map(self, fn):
        """A new ObjectStats with fn applied to every tensor (indexing, .cpu(), .clone(), ...)."""
        return ObjectStats(*(fn(getattr(self, f)) for f in _FIELDS))

    def __getitem__(self, b):
        """The statistics of scene b: tensors [S], [S, 4]."""
        return self.map(lambda t: t[b])

    def to_bop(self, b=None):
        """scene_gt_info entries of scene b (omit b for a single scene's [S] view): one dict per object slot 1..S-1, in slot
        order, with BOP's keys.  Slots that hold no object in any sense (nothing drawn, nothing visible) are included as well:
        BOP lists every object of scene_gt, and slot i is the object with instance index i."""
        s = self if b is None else self[b]
        if s.px_count_all.dim() != 1:
            raise ValueError("to_bop() needs a scene index for batched statistics")
        cols = [t.detach().cpu() for t in (s.px_count_all, s.px_count_visib, s.visib_fract, s.bbox_obj, s.bbox_visib)]
        pa, pv, vf, bo, bv = cols
        return [{
            "bbox_obj": [int(v) for v in bo[i].tolist()],
            "bbox_visib": [int(v) for v in bv[i].tolist()],
            "px_count_all": int(pa[i]),
            "px_count_visib": int(pv[i]),
            "visib_fract": float(vf[i]),
        } for i in range(1, pa.shape[0])]

    def __repr__(self):
        return "ObjectStats(%s slots)" % (tuple(self.px_count_all.shape),)
