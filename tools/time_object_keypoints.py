#!/usr/bin/env python3
"""Developer tool (GPU box): the cost of the object keypoints (slhip_object_keypoints_fps, _project, _field), timed with the HIP
events of slhip_object_keypoints_timing_enable:
  fps      the YCB-mini table (synthetic.ycb_like_meshes, 21 classes) and the Stanford bunny alone, n_fps = 8
  project  64 scenes x 20 objects, Kp = 9, against a depth plane
  field    the same at 640 x 480, unit mode, 16 scenes per call (the slice a user takes: 353.9 MB): ms, GB/s written (the kernel's
           only traffic but 2 bytes of instance per 72 written) and the share of the 6.29 TB/s a float4 copy reaches on the MI355X
and the torch formulation of the field a user would write today, in the same run on the same inputs: a gather of uv by
instance, a subtract and a normalise.  The picture is made on the device from a seed.  Prints one JSON line.
    python tools/time_object_keypoints.py [scenes=64] [repeats=20] [slice=16]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import scenes as S  # noqa: E402
import stillleben_amd as sl  # noqa: E402
from stillleben_amd import synthetic  # noqa: E402
from stillleben_amd import object_keypoints as ok  # noqa: E402

import _step_timing  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
REP = max(3, int(sys.argv[2]) if len(sys.argv) > 2 else 20)
SLICE = min(B, int(sys.argv[3]) if len(sys.argv) > 3 else 16)
OBJ, W, H, N_FPS = 20, 640, 480, 8
K4 = (1066.778, 1067.487, 312.9869, 241.3109)
HBM_COPY_TBPS = 6.29      # measured float4 copy on the MI355X, the roof of a streaming kernel
sl.init_cuda(0)
dev = torch.device("cuda", 0)


def timed(fn, which, warm=2):
    return _step_timing.timed_step("object_keypoints", 3, which, fn, REP, warm)


# ---- fps
ycb = sl.AssetTable(synthetic.ycb_like_meshes(seed=0, tex_size=64))
bunny_mesh = sl.Mesh(S.BUNNY)
bunny_mesh.center_bbox()
bunny_mesh.scale_to_bbox_diagonal(0.25)
bunny = sl.AssetTable([bunny_mesh])
_, fps_ycb_ms, _ = timed(lambda: ok.fps(ycb, N_FPS), 0)
_, fps_bunny_ms, _ = timed(lambda: ok.fps(bunny, N_FPS), 0)
bank = ok.bank(ycb, N_FPS)                       # centre + 8: Kp = 9
Kp = len(bank)

# ---- a picture and poses from a seed: 20 rectangles per scene painted back to front, objects 0.5 .. 1.5 m in front
g = torch.Generator(device=dev)
g.manual_seed(20261019)
S1 = OBJ + 1
bw, bh = (torch.randint(60, 161, (B, S1), generator=g, device=dev) for _ in range(2))
bx = (torch.rand((B, S1), generator=g, device=dev) * (W - bw)).long()
by = (torch.rand((B, S1), generator=g, device=dev) * (H - bh)).long()
xx, yy = torch.arange(W, device=dev)[None, None, :], torch.arange(H, device=dev)[None, :, None]
inst = torch.zeros((B, H, W), dtype=torch.int16, device=dev)
for i in range(1, S1):
    m = (xx >= bx[:, i, None, None]) & (xx < (bx + bw)[:, i, None, None]) & (yy >= by[:, i, None, None]) & (yy < (by + bh)[:, i, None, None])
    inst[m] = i
o2c = torch.zeros((B, OBJ, 3, 4), device=dev)
q = torch.randn((B, OBJ, 4), generator=g, device=dev)
q = q / q.norm(dim=-1, keepdim=True)
x, y, z, w = q.unbind(-1)
o2c[..., :3, :3] = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                                2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], dim=-1).view(B, OBJ, 3, 3)
o2c[..., 2, 3] = 0.5 + torch.rand((B, OBJ), generator=g, device=dev)
o2c[..., 0, 3] = (torch.rand((B, OBJ), generator=g, device=dev) - 0.5) * 0.5
o2c[..., 1, 3] = (torch.rand((B, OBJ), generator=g, device=dev) - 0.5) * 0.4
ids = torch.randint(0, len(ycb), (B, OBJ), generator=g, device=dev, dtype=torch.int32)
depth = 0.5 + torch.rand((B, H, W), generator=g, device=dev)
kps, project_ms, _ = timed(lambda: ok.project(o2c, ids, bank, K4, (W, H), depth=depth), 1)

# ---- field: SLICE scenes per call into one buffer, the slices of the chunk in turn
out = torch.empty((SLICE, H, W, Kp, 2), dtype=torch.float32, device=dev)
firsts = list(range(0, B - SLICE + 1, SLICE))
turn = [0]


def field_call():
    f = firsts[turn[0] % len(firsts)]
    turn[0] += 1
    return kps.field(inst, mode="unit", scenes=(f, SLICE), out=out)


_, field_ms, field_all = timed(field_call, 2, warm=len(firsts))
written = SLICE * H * W * Kp * 8
read = SLICE * H * W * 2


def torch_field(first):
    """what a user writes today: gather uv by instance, subtract the pixel centres, normalise"""
    i = inst[first:first + SLICE].long()
    own = (i >= 1) & (i <= OBJ)
    obj = torch.where(own, i - 1, torch.zeros_like(i))
    b = torch.arange(first, first + SLICE, device=dev)[:, None, None]
    at = kps.uv[b, obj]                                                     # [S, H, W, Kp, 2]
    live = own[..., None] & kps.in_front[b, obj]
    centre = torch.stack([xx.expand(1, H, W).float() + 0.5, yy.expand(1, H, W).float() + 0.5], dim=-1)[:, :, :, None, :]
    d = at - centre
    n = d.norm(dim=-1, keepdim=True)
    d = torch.where(n > 0, d / n, torch.zeros_like(d))
    return torch.where(live[..., None], d, torch.zeros_like(d))


torch_field(0)                                     # warm-up
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
torch_ms = []
for r in range(max(3, REP // 4)):
    ev[0].record()
    base = torch_field(firsts[r % len(firsts)])
    ev[1].record()
    torch.cuda.synchronize()
    torch_ms.append(ev[0].elapsed_time(ev[1]))
last = firsts[(max(3, REP // 4) - 1) % len(firsts)]
mine = kps.field(inst, mode="unit", scenes=(last, SLICE))
torch.cuda.synchronize()
gap = float((mine - base).abs().max())             # torch's norm and divide are not the rule's roundings: a distance, not a bit test
torch_med = statistics.median(torch_ms)
print(json.dumps({
    "metric": "object keypoints, ms (median of %d, HIP events); field: %d of %d scenes x %d objects at %d x %d, Kp = %d, unit mode"
              % (REP, SLICE, B, OBJ, W, H, Kp),
    "fps_ycb_ms": round(fps_ycb_ms, 4), "fps_ycb_classes": len(ycb), "fps_ycb_max_verts": int(ycb.records["n_verts"].max()),
    "fps_bunny_ms": round(fps_bunny_ms, 4), "fps_bunny_verts": int(bunny.records["n_verts"].max()),
    "project_ms": round(project_ms, 4), "project_keypoints": B * OBJ * Kp,
    "field_ms": round(field_ms, 4), "field_ms_min_max": [round(min(field_all), 4), round(max(field_all), 4)],
    "field_bytes_written": written, "field_bytes_read": read,
    "field_GBps_written": round(written / (field_ms * 1e-3) / 1e9, 1),
    "field_share_of_hbm_copy": round((written + read) / (field_ms * 1e-3) / (HBM_COPY_TBPS * 1e12), 3),
    "field_ms_whole_chunk": round(field_ms * B / SLICE, 3),
    "torch_field_ms": round(torch_med, 3), "torch_over_field": round(torch_med / field_ms, 1), "torch_max_abs_gap": gap,
    "inside": round(float(kps.inside.float().mean()), 4), "unoccluded": round(float(kps.unoccluded.float().mean()), 4)}))
