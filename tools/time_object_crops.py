#!/usr/bin/env python3
"""Developer tool (GPU box): the cost of the object crops (slhip_object_crops_select + slhip_object_crops_gather) at the
workload's shape -- one chunk of 512 scenes x 20 objects at 640 x 480, windows of 128 x 128, rgb + coord + mask -- timed with
the HIP events of slhip_object_crops_timing_enable, against the bytes the kernels must move:
    written  per output pixel 4 (rgb) + 16 (coord) + 1 (mask) = 21 B of the 39 B of all five outputs
    read     per output pixel at most 16 (rgb, four taps) + 16 (coord) + 2 (instance) + 8 (mask word); neighbouring output pixels
             share source pixels and cache lines, so a window asks the caches for about its source area inside the picture,
             (4 + 16 + 2) B + 1 bit per source pixel; windows of one scene overlap, so HBM delivers at most every source pixel of
             the chunk once -- the smaller of the two is the HBM model the achieved GB/s is computed with
and the same crops made by a torch composition on the same device: index_select of the source images + grid_sample per channel
group, ObjectMasks.dense for the amodal masks.  The picture is made on the device from a seed: 20 rectangles per scene painted
back to front, statistics and bit tiles to match (one tile box over the whole picture per slot).  Prints one JSON line.
    python tools/time_object_crops.py [scenes=512] [repeats=10] [size=128]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as TF  # noqa: E402

import stillleben_amd as sl  # noqa: E402
from stillleben_amd import object_crops as oc  # noqa: E402

import _step_timing  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 512
REP = max(3, int(sys.argv[2]) if len(sys.argv) > 2 else 10)
N = int(sys.argv[3]) if len(sys.argv) > 3 else 128
OBJ, W, H = 20, 640, 480
S = OBJ + 1
K = (1066.778, 1067.487, 312.9869, 241.3109)
KW = dict(size=N, box="obj", pad=1.4, jitter_scale=0.25, jitter_shift=0.25, outputs=("rgb", "coord", "mask"), seed=7)
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
# bit tiles of the rectangles: word(tx, ty) = OR over the tile's rows r of ybit(r) * (xbits << 8 r)
TX, TY = W // 8, H // 8


def bits(lo, hi, n_tiles):
    pos = torch.arange(n_tiles * 8, device=dev)[None, None, :]
    inside = ((pos >= lo[..., None]) & (pos < hi[..., None])).view(B, S, n_tiles, 8).long()
    return (inside << torch.arange(8, device=dev)).sum(dim=-1)


xb, yb = bits(bx, bx + bw, TX), bits(by, by + bh, TY)
xb[:, 0], yb[:, 0] = 0, 0
words = torch.zeros((B, S, TY, TX), dtype=torch.int64, device=dev)
for r in range(8):
    words |= ((yb >> r) & 1)[..., None] * (xb << (8 * r))[:, :, None, :]
mrec = torch.zeros((B, S, 14), dtype=torch.int32, device=dev)
mrec[..., 2], mrec[..., 3] = TX - 1, TY - 1
offs = (torch.arange(B * S, device=dev, dtype=torch.int64) * (TX * TY)).view(B, S)
for k in (0, 1):                                   # (kind 1 shares the words of kind 0: the tool reads kind 0 only)
    mrec[..., 4 + 2 * k], mrec[..., 5 + 2 * k] = (offs & 0xFFFFFFFF).to(torch.int32), (offs >> 32).to(torch.int32)
masks = sl.ObjectMasks(stats, mrec, words.view(-1), torch.zeros(1, dtype=torch.int32, device=dev), (H, W))
buffers = type("Buffers", (), {})()
buffers.rgb = torch.randint(0, 256, (B, H, W, 4), generator=g, device=dev, dtype=torch.uint8)
buffers.coord = torch.rand((B, H, W, 4), generator=g, device=dev)
buffers.normals, buffers.instance = None, inst.view(B, H, W, 1)
buffers.object_stats, buffers.object_masks = stats, masks

crops, times = _step_timing.timed("object_crops", 2, lambda: oc.extract(buffers, K, **KW), REP)
n = len(crops)
bx0, by0, side = (crops.box[:, k].double() for k in (0, 1, 2))
area = ((bx0 + side).clamp(0, W) - bx0.clamp(0, W)) * ((by0 + side).clamp(0, H) - by0.clamp(0, H))      # the part inside the picture
written = n * N * N * (4 + 16 + 1)
PX = 4 + 16 + 2 + 1.0 / 8.0                        # source bytes per pixel: rgb, coord, instance, one bit of a tile
read_windows = float(area.sum()) * PX              # what the windows ask of the caches
read = min(read_windows, B * H * W * PX)           # what must come from HBM: overlapping windows share their pixels


def torch_composition():
    """The same windows with stock operators; 16 scenes at a time."""
    u = (torch.arange(N, device=dev, dtype=torch.float32) + 0.5)
    outs = []
    for s0 in range(0, B, 16):
        sel = ((crops.scene >= s0) & (crops.scene < s0 + 16)).nonzero()[:, 0]
        if not len(sel):
            continue
        sc, slot, bxs = crops.scene[sel].long(), crops.slot[sel].long(), crops.box[sel]
        sx = bxs[:, 0, None] + u[None, :] * bxs[:, 3, None]
        sy = bxs[:, 1, None] + u[None, :] * bxs[:, 3, None]
        grid = torch.stack([(sx / W * 2 - 1)[:, None, :].expand(-1, N, -1), (sy / H * 2 - 1)[:, :, None].expand(-1, -1, N)], dim=-1)
        rgb = TF.grid_sample(buffers.rgb.index_select(0, sc).permute(0, 3, 1, 2).float(), grid, mode="bilinear", align_corners=False)
        rgb = (rgb + 0.5).floor().clamp(max=255).to(torch.uint8).permute(0, 2, 3, 1)
        near = TF.grid_sample(torch.cat([buffers.coord.index_select(0, sc).permute(0, 3, 1, 2),
                                         inst.index_select(0, sc)[:, None].float()], dim=1), grid, mode="nearest", align_corners=False)
        dense = masks.dense("all", scenes=range(s0, min(B, s0 + 16)))
        amodal = TF.grid_sample(dense[sc - s0, slot - 1][:, None].float(), grid, mode="nearest", align_corners=False)[:, 0] > 0
        visible = near[:, 4] == slot[:, None, None]
        coord = (near[:, :4] * visible[:, None]).permute(0, 2, 3, 1)
        outs.append((rgb, coord, visible.to(torch.uint8) | (amodal.to(torch.uint8) << 1)))
    return outs


torch_composition()                                # warm-up
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
ev[0].record()
base = torch_composition()
ev[1].record()
torch.cuda.synchronize()
base_ms = ev[0].elapsed_time(ev[1])
agree = float(torch.cat([b[2].reshape(-1) for b in base]).eq(crops.mask.reshape(-1)).float().mean())
sel_ms, gat_ms = (statistics.median(t[k] for t in times) for k in (0, 1))
print(json.dumps({
    "metric": "object crops, ms per %d scenes x %d objects at %d x %d, %d x %d windows, rgb + coord + mask (median of %d, HIP events)"
              % (B, OBJ, W, H, N, N, REP),
    "crops": n, "select_ms": round(sel_ms, 4), "gather_ms": round(gat_ms, 3),
    "gather_ms_all": [round(t[1], 3) for t in times], "crops_per_s": round(n / ((sel_ms + gat_ms) * 1e-3)),
    "mean_step": round(float(crops.box[:, 3].mean()), 3), "bytes_written": written, "bytes_read_windows": int(read_windows),
    "bytes_read_hbm_model": int(read), "write_GBps": round(written / (gat_ms * 1e-3) / 1e9, 1),
    "gather_GBps": round((written + read) / (gat_ms * 1e-3) / 1e9, 1), "share_of_8TBps": round((written + read) / (gat_ms * 1e-3) / 8e12, 3),
    "cache_level_GBps": round((written + read_windows) / (gat_ms * 1e-3) / 1e9, 1),
    "torch_composition_ms": round(base_ms, 1), "speedup": round(base_ms / (sel_ms + gat_ms), 1),
    "mask_agreement_with_torch": round(agree, 5)}))
