#!/usr/bin/env python3
"""Developer tool (GPU box): the cost of the per-object visibility statistics (slhip_render_object_stats) on one render chunk
of C2 scenes through SceneBatch -- the chunk's render sequence with statistics off and on, alternated, timed with HIP events
on the render stream.  Prints one JSON line.   python tools/time_object_stats.py [scenes=512] [repeats=10]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
import stillleben_amd as sl  # noqa: E402
from stillleben_amd import _abi, synthetic  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 512
REP = max(10, int(sys.argv[2]) if len(sys.argv) > 2 else 10)
sl.init_cuda(0)
table = sl.AssetTable(synthetic.ycb_like_meshes(seed=0, tex_size=1024))
batch = sl.SceneBatch(table, B, 20, resolution=bench.RESOLUTION, seed=20260929, render_chunk=B)
batch.set_camera_intrinsics(*bench.INTRINSICS)
batch.stage()
batch.settle()
batch.check_settled()
batch.place()
buf = batch.render(0, _abi.OUT_GT6, ssao=True)
for _ in range(2):      # warm-up: scratch, word pool, code objects
    buf = batch.render(0, _abi.OUT_GT6, ssao=True, buffers=buf, object_stats=True)
    buf = batch.render(0, _abi.OUT_GT6, ssao=True, buffers=buf)
torch.cuda.synchronize()


def timed(stats):
    global buf
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    buf = batch.render(0, _abi.OUT_GT6, ssao=True, buffers=buf, object_stats=stats)
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


off, on = [], []
for r in range(REP):
    # alternate the order so that neither form always follows the other
    if r % 2 == 0:
        off.append(timed(False))
        on.append(timed(True))
    else:
        on.append(timed(True))
        off.append(timed(False))
buf = batch.render(0, _abi.OUT_GT6, ssao=True, buffers=buf, object_stats=True)
st = buf.object_stats
m_off, m_on = statistics.median(off), statistics.median(on)
print(json.dumps({
    "metric": "object statistics cost per %d-scene C2 render chunk (median of %d alternated repetitions, HIP events)" % (B, REP),
    "render_ms": round(m_off, 3), "render_with_stats_ms": round(m_on, 3), "stats_ms": round(m_on - m_off, 3),
    "stats_fraction_of_render": round((m_on - m_off) / m_off, 4),
    "render_ms_all": [round(x, 3) for x in off], "render_with_stats_ms_all": [round(x, 3) for x in on],
    "objects_visible": int((st.px_count_visib > 0).sum()), "objects_drawn": int((st.px_count_all > 0).sum()),
    "mean_visib_fract": round(float(st.visib_fract[:, 1:].mean()), 4),
}))
