#!/usr/bin/env python3
"""Developer tool (GPU box): the cost of the object regions (slhip_object_regions_centres, _vertices, _label), timed with the HIP
events of slhip_object_regions_timing_enable:
  bank     centres and vertices of the YCB-mini table (synthetic.ycb_like_meshes, 21 classes) at R = 64 and 255
  label    a render chunk of the bench's scene mix (20 objects per scene, 640 x 480) at R = 64 and 255: `region` only, with
           `local`, with `histogram`, with both; ms, and the bytes the kernel must move over that time
and the torch formulation a user would write today, in the same run on the same render: per class, gather the pixels of the
class, a [P, R] plane of squared distances, argmin.  Prints one JSON line.
    python tools/time_object_regions.py [scenes=16] [repeats=20]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import stillleben_amd as sl  # noqa: E402
from stillleben_amd import _abi, synthetic  # noqa: E402
from stillleben_amd import object_regions as og  # noqa: E402

import _step_timing  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
REP = max(3, int(sys.argv[2]) if len(sys.argv) > 2 else 20)
OBJ, RES, K4 = 20, (640, 480), (1066.778, 1067.487, 312.9869, 241.3109)      # bench.py's N_OBJECTS, RESOLUTION, INTRINSICS
sl.init_cuda(0)
dev = torch.device("cuda", 0)


def timed(fn, which, warm=3):
    return _step_timing.timed_step("object_regions", 3, which, fn, REP, warm)


table = sl.AssetTable(synthetic.ycb_like_meshes(seed=0, tex_size=64))
batch = sl.SceneBatch(table, B, OBJ, resolution=RES, seed=20261019, render_chunk=B)
batch.set_camera_intrinsics(*K4)
batch.stage()
batch.settle()
batch.place()
bufs = batch.render(0)
torch.cuda.synchronize()
inst = bufs.instance.view(B, RES[1], RES[0])
coord = bufs.coord
nb = OBJ * _abi.SYNTH_OBJECT_DTYPE.itemsize
records = batch.d_objects[:B * nb]
classes = records.view(torch.int32).view(B, OBJ, 4)[..., 0].contiguous()
pixels = B * RES[0] * RES[1]
own = (inst >= 1) & (inst <= OBJ)
object_pixels = int(own.sum())
result = {"metric": "object regions, ms (median of %d, HIP events); label: %d scenes x %d objects at %d x %d" % (REP, B, OBJ, RES[0], RES[1]),
          "pixels": pixels, "object_share": round(object_pixels / pixels, 4), "classes": len(table),
          "max_verts": int(table.records["n_verts"].max()), "pool_vertices": int(batch.eng.pool.n_vertices)}


def torch_label(cen):
    """what a user writes today: per class, gather its pixels, [P, R] squared distances, argmin"""
    i = inst.long()
    obj = torch.where(own, i - 1, torch.zeros_like(i))
    cls = classes.long()[torch.arange(B, device=dev)[:, None, None], obj]
    region = torch.full((B, RES[1], RES[0]), 255, dtype=torch.uint8, device=dev)
    for c in cls[own].unique().tolist():
        at = own & (cls == c)
        pts = coord[at][:, :3]
        d2 = ((pts[:, None, :] - cen[c, :, :3][None]) ** 2).sum(dim=-1)
        region[at] = d2.argmin(dim=1).to(torch.uint8)
    return region


for R in (64, 255):
    (cen, _), centres_ms, _ = timed(lambda: og.centres(table, R), 0)
    _, vertices_ms, _ = timed(lambda: og.vertices(table, cen), 1)
    row = {"centres_ms": round(centres_ms, 4), "vertices_ms": round(vertices_ms, 4)}
    for name, kw in (("region", {}), ("local", dict(local=True)), ("histogram", dict(histogram=True)),
                     ("local_histogram", dict(local=True, histogram=True))):
        out, ms, every = timed(lambda: og.label(inst, coord, records, cen, n_objects=OBJ, **kw), 2)
        # what must move: 2 B of instance and 1 B of region per pixel, 16 B of coord per object pixel, 16 B of local per pixel
        moved = pixels * 3 + object_pixels * 16 + (pixels * 16 if "local" in kw else 0)
        row["label_%s_ms" % name] = round(ms, 4)
        row["label_%s_ms_min_max" % name] = [round(min(every), 4), round(max(every), 4)]
        row["label_%s_GBps" % name] = round(moved / (ms * 1e-3) / 1e9, 1)
    mine = og.label(inst, coord, records, cen, n_objects=OBJ).region
    torch_label(cen)                               # warm-up
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch_ms = []
    for r in range(max(3, REP // 4)):
        ev[0].record()
        base = torch_label(cen)
        ev[1].record()
        torch.cuda.synchronize()
        torch_ms.append(ev[0].elapsed_time(ev[1]))
    row["torch_ms"] = round(statistics.median(torch_ms), 3)
    row["torch_over_label_region"] = round(row["torch_ms"] / row["label_region_ms"], 1)
    # torch's sum of squares is not the rule's parenthesisation and its argmin not its tie rule: a count, not a bit test
    row["pixels_torch_labels_differently"] = int((mine != base).sum())
    row["regions_seen_per_object"] = round(float((og.label(inst, coord, records, cen, n_objects=OBJ, histogram=True).histogram > 0)
                                                 .sum(dim=2).float().mean()), 2)
    result["R%d" % R] = row
print(json.dumps(result))
