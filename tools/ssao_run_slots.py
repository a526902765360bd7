#!/usr/bin/env python3
"""Developer tool (GPU box): the runs of the SSAO tap kernel over one isolated render chunk of C2 scenes (the scenes of
tools/time_render.py), counted under SLHIP_SSAO_DEBUG=3 with the per-wave drain (SLHIP_SSAO_POOL=0) and with the pooled one:
full runs and end-of-band runs, the tap lane-slots each kind issued (taps of the run's list x 64) and those its pixels needed (each
running lane's own list), per scene.   python tools/ssao_run_slots.py [scenes=512]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
import stillleben_amd as sl  # noqa: E402
from stillleben_amd import _abi, synthetic  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 512
sl.init_cuda(0)
table = sl.AssetTable(synthetic.ycb_like_meshes(seed=0, tex_size=1024))
batch = sl.SceneBatch(table, B, 20, resolution=bench.RESOLUTION, seed=20260929, render_chunk=B)
batch.set_camera_intrinsics(*bench.INTRINSICS)
batch.stage()
batch.settle()
batch.check_settled()
batch.place()
W, H = bench.RESOLUTION
buf = None
for name, pool in (("per-wave drain (SLHIP_SSAO_POOL=0)", "0"), ("pooled drain", "1")):
    os.environ["SLHIP_SSAO_DEBUG"], os.environ["SLHIP_SSAO_POOL"] = "3", pool
    buf = batch.render(0, _abi.OUT_GT6, ssao=True, buffers=buf)
    torch.cuda.synchronize()
    tiles, runs, mixed = batch.eng.ssao_levels(buf, W, H)
    full_runs, full_slots, drain_issued, drain_needed = batch.eng.ssao_run_slots(buf, W, H)
    issued = full_slots + drain_issued
    print("%s, B=%d, per scene:" % (name, B))
    print("  tiles per level 0..5: " + " ".join("%.1f" % (t / B) for t in tiles))
    print("  full runs        %9.1f   lane-slots issued %11.0f   needed %11.0f" % (full_runs / B, full_slots / B, full_slots / B))
    print("  end-of-band runs %9.1f   lane-slots issued %11.0f   needed %11.0f   (runs with levels mixed %.1f)"
          % (runs / B, drain_issued / B, drain_needed / B, mixed / B))
    print("  end-of-band share of the issued lane-slots %.3f; issued / needed over all runs %.3f"
          % (drain_issued / max(issued, 1), issued / max(full_slots + drain_needed, 1)))
