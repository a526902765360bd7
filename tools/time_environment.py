#!/usr/bin/env python3
"""Developer tool (GPU box): what an environment bank costs a SceneBatch on the C2 shape (20 objects, 640x480, 6-channel GT,
shadows + SSAO) -- place() of the whole batch and the render sequence of one chunk, for
    none        no bank (slhip_synth_place, one drawn light)
    ibl1        every scene with a one-light map
    ibl3        every scene with a three-light map (three shadow maps per scene)
    ibl3+bg+tex every scene with a three-light map, a background image and a plane texture
timed with HIP events on the stream, the variants taken in turn with a rotating start so that none always follows the same
other.  All variants share ONE settled batch (same seed; the settled bodies are copied), so they differ in the environment only.
Prints one JSON line.   python tools/time_environment.py [scenes=2048] [chunk=512] [repeats=10]

With SLHIP_LIB naming a build without slhip_synth_place_env (the parent commit's library) only `none` is run: that is how
place() is compared across commits."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import stillleben_amd as sl  # noqa: E402
from stillleben_amd import _abi, synthetic  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
CHUNK = int(sys.argv[2]) if len(sys.argv) > 2 else 512
REP = max(5, int(sys.argv[3]) if len(sys.argv) > 3 else 10)
sl.init_cuda(0)
has_env = hasattr(_abi.lib(), "slhip_synth_place_env")
table = sl.AssetTable(synthetic.ycb_like_meshes(seed=0, tex_size=1024))


def sky(H, W, seed):
    """a smooth sky over a darker ground with a sun (f32 [H,W,3], row 0 = top)"""
    rng = np.random.default_rng(seed)
    v = (np.arange(H, dtype=np.float32)[:, None] + 0.5) / H
    u = (np.arange(W, dtype=np.float32)[None, :] + 0.5) / W
    img = np.stack([0.3 + 0.5 * (1 - v) + 0.05 * np.sin(12 * u), 0.4 + 0.4 * (1 - v) + 0 * u, 0.6 + 0.3 * (1 - v) + 0.05 * np.cos(9 * u)], axis=2)
    img[v[:, 0] > 0.55] *= np.array([0.35, 0.3, 0.25], np.float32)
    img += 30.0 * np.exp(-(((u - 0.3) * 2 * W / H) ** 2 + (v - 0.25) ** 2) * 400.0)[..., None] * np.array([1.0, 0.9, 0.7], np.float32)
    return (img + 0.02 * rng.random((H, W, 3))).astype(np.float32)


variants = {"none": None}
if has_env:
    rng = np.random.default_rng(1)
    lm = sl.LightMap(sky(512, 1024, 0))                          # the reference's texture sizes (light_map.DEFAULT_SIZES)
    lights = [((0.3, -0.2, -0.93), (3.0, 2.8, 2.5)), ((-0.5, 0.4, -0.77), (1.0, 1.2, 1.5)), ((0.1, 0.7, -0.7), (0.8, 0.6, 0.5))]
    bgs = [sl.Texture(torch.from_numpy((rng.random((480, 640, 4)) * 255).astype(np.uint8))) for _ in range(4)]
    pts = [sl.Texture2D(torch.from_numpy((rng.random((1024, 1024, 4)) * 255).astype(np.uint8) | np.uint8(1))) for _ in range(4)]
    for name, n_lights, rest in (("ibl1", 1, False), ("ibl3", 3, False), ("ibl3+bg+tex", 3, True)):
        bank = sl.EnvironmentBank(backgrounds=bgs if rest else (), plane_textures=pts if rest else ())
        bank.add_light_map(lm, directions=[d for d, _ in lights[:n_lights]], colors=[c for _, c in lights[:n_lights]])
        variants[name] = bank

batches = {}
for name, bank in variants.items():
    b = sl.SceneBatch(table, N, 20, resolution=bench.RESOLUTION, seed=20261016, render_chunk=CHUNK, environment=bank)
    b.set_camera_intrinsics(*bench.INTRINSICS)
    if batches:
        first = next(iter(batches.values()))
        for t in ("d_bodies", "d_settle_scenes", "d_objects", "d_scenes"):
            getattr(b, t).copy_(getattr(first, t))
    else:
        b.stage()
        b.settle()
        b.check_settled()
    batches[name] = b
bufs = {}
for _ in range(2):            # warm-up: code objects, bank upload, scratch
    for name, b in batches.items():
        b.place()
        bufs[name] = b.render(0, _abi.OUT_GT6, ssao=True, buffers=bufs.get(name))
torch.cuda.synchronize()


def timed(fn):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    e.record()
    e.synchronize()
    return a.elapsed_time(e)


def render(name):
    bufs[name] = batches[name].render(0, _abi.OUT_GT6, ssao=True, buffers=bufs[name])


names = list(batches)
place = {n: [] for n in names}
rend = {n: [] for n in names}
for r in range(REP):
    order = names[r % len(names):] + names[:r % len(names)]
    for n in order:
        place[n].append(timed(batches[n].place))
    for n in order:
        rend[n].append(timed(lambda: render(n)))


def summary(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


env = batches[names[-1]].host_env()
try:
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
except OSError:
    commit = ""
print(json.dumps({
    "metric": "environment bank cost, C2 shape: place() of %d scenes and the render sequence of one %d-scene chunk "
              "(HIP events, %d repetitions per variant, taken in turn)" % (N, CHUNK, REP),
    "commit": commit, "library": os.path.basename(os.path.dirname(_abi.lib_path())) + "/" + os.path.basename(_abi.lib_path()),
    "place": {n: summary(place[n]) for n in names}, "render": {n: summary(rend[n]) for n in names},
    "render_vs_none": {n: round(statistics.median(rend[n]) / statistics.median(rend["none"]), 4) for n in names},
    "scenes_with_light_map_background_plane_texture": [int((env[:, k] >= 0).sum()) for k in range(3)],
}))
