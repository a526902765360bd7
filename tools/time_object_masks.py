#!/usr/bin/env python3
"""Developer tool (GPU box): the cost of the per-object masks (slhip_render_object_masks) on one render chunk of C2 scenes
through SceneBatch, against the two things one could do before them --
  * the chunk's render sequence with object_stats=True (the numbers alone) and with object_masks=True, alternated, timed with
    HIP events on the render stream;
  * one extra render per object, alone and without the plane (how the tests obtain a whole silhouette), for a handful of
    scenes handed over to the per-scene API: wall-clock per scene, and scaled to the chunk.
Also the sizes of the two pools of the masks call.  Prints one JSON line.
    python tools/time_object_masks.py [scenes=256] [repeats=10] [alone_scenes=4]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import stillleben_amd as sl  # noqa: E402
from stillleben_amd import _abi, synthetic  # noqa: E402
from stillleben_amd._context import engine  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
REP = max(4, int(sys.argv[2]) if len(sys.argv) > 2 else 10)
ALONE = int(sys.argv[3]) if len(sys.argv) > 3 else 4
N_OBJECTS = 20
sl.init_cuda(0)
table = sl.AssetTable(synthetic.ycb_like_meshes(seed=0, tex_size=1024))
batch = sl.SceneBatch(table, B, N_OBJECTS, resolution=bench.RESOLUTION, seed=20260929, render_chunk=B)
batch.set_camera_intrinsics(*bench.INTRINSICS)
batch.stage()
batch.settle()
batch.check_settled()
batch.place()
eng = engine()
buf = batch.render(0, _abi.OUT_GT6, ssao=True)
for _ in range(2):      # warm-up: scratch, pools, code objects
    buf = batch.render(0, _abi.OUT_GT6, ssao=True, buffers=buf, object_stats=True)
    buf = batch.render(0, _abi.OUT_GT6, ssao=True, buffers=buf, object_masks=True)
    buf.object_masks = None
torch.cuda.synchronize()


def timed(**kw):
    global buf
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    buf = batch.render(0, _abi.OUT_GT6, ssao=True, buffers=buf, **kw)
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


plain, stats, masks = [], [], []
for r in range(REP):
    # rotate the order so that no form always follows the same other
    order = [(plain, {}), (stats, {"object_stats": True}), (masks, {"object_masks": True})]
    for lst, kw in order[r % 3:] + order[:r % 3]:
        lst.append(timed(**kw))
        buf.object_masks = None          # (the pools of a finished masks call are not kept over the next timing)
buf = batch.render(0, _abi.OUT_GT6, ssao=True, buffers=buf, object_masks=True)
torch.cuda.synchronize()
om = buf.object_masks
calls = eng.last_masks_calls
rec = om.host_records()

# the only way to a whole silhouette without the masks: the object alone, no plane, one render each
alone_ms = []
for index in range(min(ALONE, B)):
    scene = batch.scene(index)
    scene._background_plane_size = np.zeros(2, np.float32)
    objs = scene.objects
    for i, o in enumerate(objs):
        o.instance_index = i + 1
    eng.render([scene], _abi.OUT_INSTANCE, ssao=False, shadows=False, predicate=lambda o: o.instance_index == 1)   # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(1, len(objs) + 1):
        m = eng.render([scene], _abi.OUT_INSTANCE, ssao=False, shadows=False, predicate=lambda o, i=i: o.instance_index == i)
        m = (m.instance[0, ..., 0] == i)
    torch.cuda.synchronize()
    alone_ms.append((time.perf_counter() - t0) * 1e3)

m_plain, m_stats, m_masks = (statistics.median(v) for v in (plain, stats, masks))
per_scene = statistics.median(alone_ms) if alone_ms else None
worst_w, worst_r = C.c_uint64(0), C.c_uint64(0)
W, H = bench.RESOLUTION
_abi.lib().slhip_render_object_masks_bytes(B, N_OBJECTS + 1, W, H, C.byref(worst_w), C.byref(worst_r))
print(json.dumps({
    "metric": "object masks cost per %d-scene C2 render chunk (median of %d rotated repetitions, HIP events)" % (B, REP),
    "render_ms": round(m_plain, 3), "render_with_stats_ms": round(m_stats, 3), "render_with_masks_ms": round(m_masks, 3),
    "stats_ms": round(m_stats - m_plain, 3), "masks_ms": round(m_masks - m_plain, 3),
    "masks_over_stats_ms": round(m_masks - m_stats, 3),
    "render_with_stats_ms_all": [round(x, 3) for x in stats], "render_with_masks_ms_all": [round(x, 3) for x in masks],
    "alone_renders_ms_per_scene": None if per_scene is None else round(per_scene, 3),
    "alone_renders_ms_per_scene_all": [round(x, 3) for x in alone_ms],
    "alone_renders_ms_per_chunk": None if per_scene is None else round(per_scene * B, 1),
    "words_needed": calls[-1][2], "words_bytes": calls[-1][2] * 8, "runs_needed": calls[-1][4], "runs_bytes": calls[-1][4] * 4,
    "worst_case_words_bytes": worst_w.value * 8, "worst_case_runs_bytes": worst_r.value * 4,
    "dense_bytes_both_kinds": 2 * B * N_OBJECTS * W * H,
    "runs_per_mask_mean": round(float(rec["rle_count"][:, 1:].mean()), 2), "runs_per_mask_max": int(rec["rle_count"].max()),
    "masks_calls_last": len(calls),
}))
