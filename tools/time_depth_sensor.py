#!/usr/bin/env python3
"""Developer tool (GPU box): the cost of the depth sensor model (slhip_depth_sensor) on one chunk of 640 x 480 images, per
pass, timed with the HIP events of slhip_depth_sensor_timing_enable -- once reading z and n.v in place from the w of
[n,H,W,4] buffers (what a render leaves, stride 4) and once from dense planes (stride 1), alternated.  The images are a
tilted plane with boxes in front of it, made on the device from a seed; every output (f32, uint16, flags) is written.
Also the bytes the two passes must move per image, and the rate that makes.  Prints one JSON line.
    python tools/time_depth_sensor.py [images=512] [repeats=10] [window_radius=4]"""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import stillleben_amd as sl  # noqa: E402
from stillleben_amd import _abi  # noqa: E402
from stillleben_amd import depth_sensor as ds  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 512
REP = max(4, int(sys.argv[2]) if len(sys.argv) > 2 else 10)
RADIUS = int(sys.argv[3]) if len(sys.argv) > 3 else 4
W, H = 640, 480
sl.init_cuda(0)
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev)
g.manual_seed(20261018)
coord = torch.zeros((N, H, W, 4), dtype=torch.float32, device=dev)
normals = torch.zeros((N, H, W, 4), dtype=torch.float32, device=dev)
z = coord[..., 3]
z[:] = 1.2 + 0.002 * torch.arange(H, device=dev, dtype=torch.float32)[None, :, None]
for _ in range(8):                               # boxes 0.3 .. 0.9 m in front of the plane, the same in every image
    x0, y0 = (int(torch.randint(0, v - 120, (1,), generator=g, device=dev)) for v in (W, H))
    z[:, y0:y0 + 110, x0:x0 + 110] -= 0.3 + 0.6 * float(torch.rand(1, generator=g, device=dev))
z.clamp_(min=0.45)
z[:, :40] = 3000.0                               # background
normals[..., 3] = torch.rand((N, H, W), generator=g, device=dev)
z_dense, c_dense = z.contiguous(), normals[..., 3].contiguous()
params = [ds.make_params(580.0, window_radius=RADIUS, min_support=(2 * RADIUS + 1) ** 2 // 2, seed=i) for i in range(N)]
L = _abi.lib()
_abi.check(L.slhip_depth_sensor_timing_enable(1), "slhip_depth_sensor_timing_enable")


def timed(zz, cc):
    out = ds.process_batch(zz, params, ndotv=cc, out="both", flags=True)
    ms = (C.c_float * 2)()
    _abi.check(L.slhip_depth_sensor_timings(C.byref(ms)), "slhip_depth_sensor_timings")
    return (ms[0], ms[1]), out


for _ in range(2):                               # warm-up: code objects, allocator
    timed(z, normals[..., 3])
    timed(z_dense, c_dense)
strided, dense = [], []
for r in range(REP):
    order = [(strided, z, normals[..., 3]), (dense, z_dense, c_dense)]
    for lst, zz, cc in order[r % 2:] + order[:r % 2]:
        t, out = timed(zz, cc)
        lst.append(t)
valid_share = float((out[2] == 0).float().mean())
_abi.check(L.slhip_depth_sensor_timing_enable(0), "slhip_depth_sensor_timing_enable")
px = W * H
# bytes per image: pass 1 reads z and n.v (4 B each; from the w of a float4 buffer the whole 16 B come in with the line) and
# writes disparity (4) + flags (1); pass 2 reads them back (5, the halo comes from cache) and writes f32 + u16 + flags (7)
bytes_p1 = {"stride4": px * (32 + 5), "dense": px * (8 + 5)}
bytes_p2 = px * (5 + 7)


def med(lst, k):
    return statistics.median(t[k] for t in lst)


res = {"metric": "depth sensor model, ms per %d images of %d x %d, window_radius %d (median of %d alternated repetitions, HIP events)"
       % (N, W, H, RADIUS, REP), "valid_share": round(valid_share, 4)}
for name, lst in (("stride4", strided), ("dense", dense)):
    p1, p2 = med(lst, 0), med(lst, 1)
    res[name] = {"pass1_ms": round(p1, 3), "pass2_ms": round(p2, 3), "total_ms": round(p1 + p2, 3),
                 "pass1_ms_all": [round(t[0], 3) for t in lst], "pass2_ms_all": [round(t[1], 3) for t in lst],
                 "pass1_bytes_per_image": bytes_p1[name], "pass2_bytes_per_image": bytes_p2,
                 "pass1_TBps": round(N * bytes_p1[name] / (p1 * 1e-3) / 1e12, 3), "pass2_TBps": round(N * bytes_p2 / (p2 * 1e-3) / 1e12, 3)}
print(json.dumps(res))
