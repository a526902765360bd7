#!/usr/bin/env python3
"""Developer tool (GPU box): the cost of the pose VSD (slhip_pose_vsd, slhip_pose_depth), timed with the HIP events of
slhip_pose_vsd_timing_enable, at 640 x 480:
  vsd    1024 scenes x 20 objects x 1 hypothesis   (a batch's ground truth against one estimate each)
  vsd    1 x 64 x 32                               (the sl.diff shape: many hypotheses of few objects)
  depth  1 x 64 x 32                               (the raster alone, dense planes)
The bank is 21 icospheres of 1280 triangles, 0.08 to 0.28 across, the poses 0.6 to 1.5 in front of the camera (about 30 to 250
px), the estimates a few centimetres and degrees off; the scene's depth is a tilted plane through the objects.  Everything is
made from a seed.  Prints one JSON line.
    python tools/time_pose_vsd.py [repeats=10] [scenes=1024]
With --libs a.so,b.so,... [--rounds R] the tool instead runs itself once per library and round in a child process (SLHIP_LIB
selects the build), taking the libraries in turn, and prints per library the median and the min - max over all repetitions of
all rounds: how the band_pixels candidates (builds with -DSLHIP_VSD_BAND_PIXELS=4096 / 8192 / 16384) are compared."""
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def compare(libs, rounds, rest):
    rows = {lib: {} for lib in libs}
    for r in range(rounds):
        for lib in libs:      # in turn: a drift of the box hits every build alike
            env = dict(os.environ, SLHIP_LIB=os.path.abspath(lib))
            out = subprocess.run([sys.executable, os.path.abspath(__file__)] + rest, env=env, check=True, capture_output=True, text=True, timeout=600)
            line = json.loads(out.stdout.strip().splitlines()[-1])
            print(json.dumps({"round": r, "lib": lib, **line}), flush=True)
            rows[lib].setdefault("band_pixels", line["band_pixels"])
            for k, v in line["ms_all"].items():
                rows[lib].setdefault(k, []).extend(v)
    for lib in libs:
        print(json.dumps({"lib": lib, "band_pixels": rows[lib]["band_pixels"],
                          **{k: {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)} for k, v in rows[lib].items() if k != "band_pixels"}}))


if "--libs" in sys.argv:
    i = sys.argv.index("--libs")
    libs = sys.argv[i + 1].split(",")
    rest = sys.argv[1:i] + sys.argv[i + 2:]
    rounds = 3
    if "--rounds" in rest:
        j = rest.index("--rounds")
        rounds = int(rest[j + 1])
        rest = rest[:j] + rest[j + 2:]
    compare(libs, rounds, rest)
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import stillleben_amd as sl  # noqa: E402
from stillleben_amd import pose_vsd as pv  # noqa: E402

import _step_timing  # noqa: E402

REP = max(3, int(sys.argv[1]) if len(sys.argv) > 1 else 10)
B = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
OBJ, A, W, H = 20, 21, 640, 480
K4 = (1066.778 / 2, 1067.487 / 2, 312.9869, 241.3109)
sl.init_cuda(0)
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev)
g.manual_seed(20261020)


def timed(fn, rep, warm=2):
    return _step_timing.timed("pose_vsd", 2, fn, rep, warm)


def icosphere(levels):
    t = (1.0 + math.sqrt(5.0)) / 2.0
    v = [np.array(p, np.float64) / math.sqrt(1 + t * t) for p in
         [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(levels):
        mid, nf = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v), np.array(f)


def make_surface():
    sv, sf = icosphere(3)
    verts, tris = [], []
    for c in range(A):
        r = 0.04 + 0.005 * c
        verts.append(np.concatenate([sv * r * np.array([1.0, 0.8, 0.6]), np.ones((len(sv), 1))], axis=1))
        tris.append(sf + c * len(sv))
    as_t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)      # noqa: E731
    return pv.surface(vertices=as_t(np.concatenate(verts), torch.float32), triangles=as_t(np.concatenate(tris), torch.int32),
                      tri_begin=as_t(np.arange(A) * len(sf), torch.int32), tri_count=as_t(np.full(A, len(sf)), torch.int32),
                      diameter=[2 * (0.04 + 0.005 * c) for c in range(A)])


def poses(shape):
    q = torch.randn(shape + (4,), generator=g, device=dev)
    q = q / q.norm(dim=-1, keepdim=True)
    x, y, z, w = q.unbind(-1)
    T = torch.zeros(shape + (3, 4), device=dev)
    T[..., 0, 0], T[..., 0, 1], T[..., 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)
    T[..., 1, 0], T[..., 1, 1], T[..., 1, 2] = 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)
    T[..., 2, 0], T[..., 2, 1], T[..., 2, 2] = 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)
    u = torch.rand(shape + (3,), generator=g, device=dev)
    T[..., 2, 3] = 0.6 + 0.9 * u[..., 2]
    T[..., 0, 3] = (u[..., 0] - 0.5) * 0.9 * T[..., 2, 3]
    T[..., 1, 3] = (u[..., 1] - 0.5) * 0.65 * T[..., 2, 3]
    return T


def near(gt, Hy):
    est = gt[:, :, None].repeat(1, 1, Hy, 1, 1).contiguous()
    est[..., 3] += (torch.rand(est.shape[:-1], generator=g, device=dev) - 0.5) * 0.04
    est[..., :3] += (torch.rand(est.shape[:-1] + (3,), generator=g, device=dev) - 0.5) * 0.05      # a few degrees, not re-orthonormalised
    return est


def scene_depth(n):
    py, px = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    return (1.0 + 0.001 * (px - W / 2) - 0.0007 * (py - H / 2)).float()[None].repeat(n, 1, 1).contiguous()


surf = make_surface()
result = {"tool": "time_pose_vsd", "band_pixels": pv.band_pixels(), "repeats": REP, "size": [W, H], "ms": {}, "ms_all": {}, "minmax": {}}


def record(name, times, which):
    ms = [t[which] for t in times]
    result["ms"][name] = statistics.median(ms)
    result["minmax"][name] = [min(ms), max(ms)]
    result["ms_all"][name] = ms


for name, (b, o, hy) in (("vsd_%dx%dx1" % (B, OBJ), (B, OBJ, 1)), ("vsd_1x64x32", (1, 64, 32))):
    classes = torch.randint(0, A, (b, o), generator=g, device=dev, dtype=torch.int32)
    gt = poses((b, o))
    est, depth = near(gt, hy), scene_depth(b)
    out, times = timed(lambda: pv.evaluate(gt, est, classes, surf, depth, K4), REP)
    torch.cuda.synchronize()
    record(name, times, 0)
    result.setdefault("mean_union", {})[name] = float(out.counts[..., 3].float().mean())
    if b == 1:
        planes, times = timed(lambda: pv.render_depth(est, classes, surf, K4, (W, H)), REP)
        torch.cuda.synchronize()
        record("depth_1x64x32", times, 1)
print(json.dumps(result))
