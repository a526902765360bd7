#!/usr/bin/env python3
"""Developer tool (GPU box): the cost of the object points (slhip_object_points_select + slhip_object_points_gather) at the
workload's shape -- one chunk of 512 scenes x 20 objects at 640 x 480, K = 1024 points per object, pixel + camera + coord --
timed with the HIP events of slhip_object_points_timing_enable, and the same result made by a torch formulation on the same
device: ObjectMasks.dense for the visible masks, nonzero, the rank rule as tensor arithmetic, and fancy-indexing gathers, 16
scenes at a time.  (The torch formulation takes the pixels of a mask in row-major order of the picture, not in tile order: the
same amount of work, other pixels; the tool therefore compares against it only what does not depend on the order.)
The picture is made on the device from a seed: 20 rectangles per scene painted back to front, statistics and bit tiles to match
(one tile box over the whole picture per slot, the hardest case for the gather: 4800 words per set).  Prints one JSON line.
    python tools/time_object_points.py [scenes=512] [repeats=10] [points=1024]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import stillleben_amd as sl  # noqa: E402
from stillleben_amd import object_points as op  # noqa: E402

import _step_timing  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 512
REP = max(3, int(sys.argv[2]) if len(sys.argv) > 2 else 10)
K = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
OBJ, W, H = 20, 640, 480
S = OBJ + 1
K4 = (1066.778, 1067.487, 312.9869, 241.3109)
KW = dict(n_points=K, outputs=("pixel", "camera", "coord"), seed=7)
sl.init_cuda(0)
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev)
g.manual_seed(20261018)


def rand(lo, hi):
    return torch.randint(lo, hi, (B, S), generator=g, device=dev)


# rectangles 60 .. 160 px wide and high, anywhere in the picture; slot 0 empty
bw, bh = rand(60, 161), rand(60, 161)
bx, by = (torch.rand((B, S), generator=g, device=dev) * (W - bw)).long(), (torch.rand((B, S), generator=g, device=dev) * (H - bh)).long()
xx = torch.arange(W, device=dev)[None, None, :]
yy = torch.arange(H, device=dev)[None, :, None]
inst = torch.zeros((B, H, W), dtype=torch.int16, device=dev)
for i in range(1, S):
    m = (xx >= bx[:, i, None, None]) & (xx < (bx + bw)[:, i, None, None]) & (yy >= by[:, i, None, None]) & (yy < (by + bh)[:, i, None, None])
    inst[m] = i
px_visib = torch.stack([torch.zeros(B, dtype=torch.int64, device=dev)] + [(inst == i).sum(dim=(1, 2)) for i in range(1, S)], dim=1)
box = torch.stack([bx, by, bw, bh], dim=-1)
box[:, 0] = -1
rec = torch.cat([px_visib[..., None], (bw * bh)[..., None], box, box], dim=-1).to(torch.int32)
rec[:, 0, :2] = 0
stats = sl.ObjectStats.from_records(rec)
# kind-1 bit tiles from the instance picture: word(tile) = sum over the tile's pixels of [inst == slot] << ((y & 7) * 8 + (x & 7))
TX, TY = W // 8, H // 8
shift = ((torch.arange(8, device=dev)[:, None] * 8 + torch.arange(8, device=dev)[None, :])).view(1, 1, 8, 1, 8)
tiles = inst.view(B, TY, 8, TX, 8)
words = torch.zeros((B, S, TY, TX), dtype=torch.int64, device=dev)
for i in range(1, S):
    words[:, i] = ((tiles == i).long() << shift).sum(dim=(2, 4))      # (bit 63 wraps into the sign: the same 64 bits)
mrec = torch.zeros((B, S, 14), dtype=torch.int32, device=dev)
mrec[..., 2], mrec[..., 3] = TX - 1, TY - 1
mrec[:, 0, 2], mrec[:, 0, 3] = -1, -1
offs = (torch.arange(B * S, device=dev, dtype=torch.int64) * (TX * TY)).view(B, S)
for k in (0, 1):                                   # (kind 0 shares the words of kind 1: the tool reads kind 1 only)
    mrec[..., 4 + 2 * k], mrec[..., 5 + 2 * k] = (offs & 0xFFFFFFFF).to(torch.int32), (offs >> 32).to(torch.int32)
masks = sl.ObjectMasks(stats, mrec, words.view(-1), torch.zeros(1, dtype=torch.int32, device=dev), (H, W))
buffers = type("Buffers", (), {})()
buffers.coord = torch.rand((B, H, W, 4), generator=g, device=dev) + 0.5
buffers.rgb, buffers.normals, buffers.instance = None, None, inst.view(B, H, W, 1)
buffers.object_stats, buffers.object_masks = stats, masks

points, times = _step_timing.timed("object_points", 2, lambda: op.extract(buffers, K4, **KW), REP)
n = len(points)
# every point is a visible pixel of its object
hit = inst[points.scene.long()[:, None], points.pixel[..., 1].long(), points.pixel[..., 0].long()] == points.slot[:, None]
written = n * K * (4 + 16 + 16)
read_words = n * TX * TY * 8                       # pass A reads every word of the set's box once; pass B re-reads a few from cache
read_points = n * K * (16 + 4)                     # coord (whose w is the depth) ... one 64-byte line per point at the least
fx, fy, cx, cy = K4


def torch_formulation():
    """The same outputs with stock operators, 16 scenes at a time: dense masks, nonzero per object, the rank rule with
    torch.rand for the draw, gathers.  One host synchronisation per object (nonzero), as a user's loop would have."""
    outs = []
    j = torch.arange(K, device=dev, dtype=torch.int64)
    for s0 in range(0, B, 16):
        scenes = range(s0, min(B, s0 + 16))
        dense = masks.dense("visib", scenes=scenes)
        for b in scenes:
            for i in range(1, S):
                ys, xs = torch.nonzero(dense[b - s0, i - 1], as_tuple=True)
                m = ys.numel()
                if m == 0:
                    continue
                lo, hi = j * m // K, (j + 1) * m // K
                rank = lo + (torch.rand(K, device=dev, dtype=torch.float64) * (hi - lo)).long()
                x, y = xs[rank], ys[rank]
                c = buffers.coord[b, y, x]
                z = c[:, 3]
                cam = torch.stack([((x.float() + 0.5) - cx) * z / fx, ((y.float() + 0.5) - cy) * z / fy, z, torch.ones_like(z)], dim=1)
                outs.append((torch.stack([x, y], dim=1).to(torch.int16), cam, c))
    return outs


torch_formulation()                                # warm-up
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
ev[0].record()
base = torch_formulation()
ev[1].record()
torch.cuda.synchronize()
base_ms = ev[0].elapsed_time(ev[1])
sel_ms, gat_ms = (statistics.median(t[k] for t in times) for k in (0, 1))
print(json.dumps({
    "metric": "object points, ms per %d scenes x %d objects at %d x %d, K = %d, pixel + camera + coord (median of %d, HIP events)"
              % (B, OBJ, W, H, K, REP),
    "sets": n, "sets_torch": len(base), "select_ms": round(sel_ms, 4), "gather_ms": round(gat_ms, 3),
    "gather_ms_all": [round(t[1], 3) for t in times], "points_per_s": round(n * K / ((sel_ms + gat_ms) * 1e-3)),
    "words_per_set": TX * TY, "bytes_written": written, "bytes_read_words": read_words, "bytes_read_points": read_points,
    "gather_GBps": round((written + read_words + read_points) / (gat_ms * 1e-3) / 1e9, 1),
    "points_on_their_object": round(float(hit.float().mean()), 5), "valid": round(float(points.valid.float().mean()), 5),
    "torch_formulation_ms": round(base_ms, 1), "speedup": round(base_ms / (sel_ms + gat_ms), 1)}))
