#!/usr/bin/env python3
"""Developer tool (GPU box): the cost of the render flow (slhip_render_flow) at 512 scenes of 640 x 480 with 20 objects, against
the plain torch route of the same arithmetic -- what a user would write today: a gather of the motion by instance, the
projection, four gathers of picture b, a dozen elementwise passes, in slices of 32 scenes so that its temporaries fit.  The two
are timed in three alternating runs each (kernel, torch, kernel, torch, ...) with device events round every call; nobody has
promised a time for this kernel, so the tool reports and asserts nothing; how far the two routes agree on the last slice is part
of the report.  Per run one JSON line, then a summary:
the kernel's median ms for the depth as planes and as coord targets, the bytes of the model below over that time as a share of
the 6.29 TB/s a float4 copy reaches on the MI355X, and the torch route's ms.

Bytes per pixel of the model (every plane swept once; the footprint gathers of picture b hit lines that its sweep brings in):
    depth a 4 (plane) or 16 (the w of a coord target drags its line in), instance a 2, the same for picture b,
    flow 8, flags 1, scene flow 12 when asked for; the motion table and the counts are noise.

    python tools/time_render_flow.py [scenes=512] [repeats=10]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import stillleben_amd as sl  # noqa: E402
from stillleben_amd import render_flow as rf  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 512
REP = max(3, int(sys.argv[2]) if len(sys.argv) > 2 else 10)
OBJ, W, H, SLICE, RUNS = 20, 640, 480, 32, 3
S1 = OBJ + 1
K4 = (1066.778, 1067.487, 312.9869, 241.3109)
TOL, REL, MAX_DEPTH = 0.005, 0.01, 3000.0
HBM_COPY_TBPS = 6.29      # measured float4 copy on the MI355X, the roof of a streaming kernel
sl.init_cuda(0)
dev = torch.device("cuda", 0)

# ---- two pictures from a seed: 20 rectangles per scene painted back to front on a plane, every slot with a small rigid motion
g = torch.Generator(device=dev)
g.manual_seed(20261021)
xx, yy = torch.arange(W, device=dev)[None, None, :], torch.arange(H, device=dev)[None, :, None]


def picture(shift):
    bw, bh = (torch.randint(60, 161, (B, S1), generator=g, device=dev) for _ in range(2))
    bx = (torch.rand((B, S1), generator=g, device=dev) * (W - bw)).long() + shift
    by = (torch.rand((B, S1), generator=g, device=dev) * (H - bh)).long()
    inst = torch.zeros((B, H, W), dtype=torch.int16, device=dev)
    depth = torch.full((B, H, W), 2.0, device=dev)
    for i in range(1, S1):
        m = (xx >= bx[:, i, None, None]) & (xx < (bx + bw)[:, i, None, None]) & (yy >= by[:, i, None, None]) & (yy < (by + bh)[:, i, None, None])
        inst[m] = i
        depth = torch.where(m, torch.full_like(depth, 2.0 - 0.06 * i), depth)
    depth[:, :24] = MAX_DEPTH                           # a strip of background
    return depth + 0.01 * torch.rand((B, H, W), generator=g, device=dev), inst


g_state = g.get_state()
depth_a, inst_a = picture(0)
g.set_state(g_state)
depth_b, inst_b = picture(6)                            # the same rectangles six pixels to the right
angle = 0.02 * (torch.rand((B, S1, 3), generator=g, device=dev) - 0.5)
table = torch.zeros((B, S1, 3, 4), device=dev)
table[..., 0, 0] = table[..., 1, 1] = table[..., 2, 2] = 1.0
table[..., 0, 1], table[..., 1, 0] = -angle[..., 2], angle[..., 2]
table[..., 0, 2], table[..., 2, 0] = angle[..., 1], -angle[..., 1]
table[..., 1, 2], table[..., 2, 1] = -angle[..., 0], angle[..., 0]
table[..., 0, 3] = 6.0 * 2.0 / K4[0] + 0.004 * (torch.rand((B, S1), generator=g, device=dev) - 0.5)
table[..., 1, 3] = 0.004 * (torch.rand((B, S1), generator=g, device=dev) - 0.5)


def coord_of(depth):
    c = torch.zeros((B, H, W, 4), device=dev)
    c[..., 3] = depth
    return c


def kernel_planes(outputs):
    return rf.compute(depth_a, inst_a, table, K4, depth_b, inst_b, MAX_DEPTH, TOL, REL, True, outputs)


def torch_slice(first):
    """the same arithmetic in plain torch on scenes [first, first + SLICE): (flow, flags)"""
    fx, fy, cx, cy = K4
    sl_ = slice(first, first + SLICE)
    z, i = depth_a[sl_], inst_a[sl_].long() & 0xFFFF
    b = torch.arange(SLICE, device=dev)[:, None, None]
    tab, zb_all, ib_all = table[sl_], depth_b[sl_], inst_b[sl_].long() & 0xFFFF
    M = tab[b, i.clamp(max=S1 - 1)]
    px, py = xx.float() + 0.5, yy.float() + 0.5
    X, Y = ((px - cx) * z) / fx, ((py - cy) * z) / fy
    Xp, Yp, Zp = (((M[..., r, 0] * X + M[..., r, 1] * Y) + M[..., r, 2] * z) + M[..., r, 3] for r in range(3))
    valid = (torch.isfinite(z) & (z > 0) & (z < MAX_DEPTH) & (i < S1) & torch.isfinite(M).all(-1).all(-1)
             & torch.isfinite(Xp) & torch.isfinite(Yp) & torch.isfinite(Zp) & (Zp > 0))
    u, v = (fx * Xp) / Zp + cx, (fy * Yp) / Zp + cy
    inside = valid & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    x0 = torch.where(inside, torch.floor(u - 0.5), torch.zeros_like(u)).long()
    y0 = torch.where(inside, torch.floor(v - 0.5), torch.zeros_like(v)).long()
    tol = TOL + REL * Zp
    visible = torch.zeros_like(inside)
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        x1, y1 = x0 + dx, y0 + dy
        inb = (x1 >= 0) & (x1 < W) & (y1 >= 0) & (y1 < H)
        xc, yc = x1.clamp(0, W - 1), y1.clamp(0, H - 1)
        zb = zb_all[b, yc, xc]
        visible |= inside & inb & (ib_all[b, yc, xc] == i) & torch.isfinite(zb) & (zb > 0) & (Zp <= zb + tol)
    flow = torch.where(valid[..., None], torch.stack([u - px, v - py], dim=-1), torch.zeros((), device=dev))
    return flow, valid.to(torch.uint8) + 2 * inside.to(torch.uint8) + 4 * visible.to(torch.uint8)


def torch_all():
    for first in range(0, B - SLICE + 1, SLICE):
        out = torch_slice(first)
    return out


def timed(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        keep = fn()
        b.record()
    torch.cuda.synchronize()
    del keep
    return [a.elapsed_time(b) for a, b in ev]


pixels = B * H * W
DEFAULT, EVERYTHING = ("flow", "flags", "counts"), ("flow", "scene_flow", "flags", "counts")
model = {"planes": (4 + 2) * 2 + 8 + 1, "planes_all": (4 + 2) * 2 + 8 + 1 + 12, "coord": (16 + 2) * 2 + 8 + 1}
coord_a, coord_b = coord_of(depth_a), coord_of(depth_b)
cases = {"planes": lambda: kernel_planes(DEFAULT), "planes_all": lambda: kernel_planes(EVERYTHING),
         "coord": lambda: rf.compute(coord_a, inst_a, table, K4, coord_b, inst_b, MAX_DEPTH, TOL, REL, True, DEFAULT)}
for fn in cases.values():                              # warm-up: code objects, the allocator's blocks
    timed(fn, 2)
timed(torch_all, 1)

# agreement first: faster and different is not faster
mine = kernel_planes(EVERYTHING)
last = B - SLICE
want_flow, want_flags = torch_slice(last)
torch.cuda.synchronize()
gap = float((mine.flow[last:] - want_flow).abs().max())
flag_diff = int((mine.flags[last:] != want_flags).sum())
counts = mine.counts.sum(dim=(0, 1)).tolist()

ms = {k: [] for k in list(cases) + ["torch"]}
for run in range(RUNS):                                # alternating: the neighbours on the machine change over a run
    line = {"run": run}
    for name, fn in cases.items():
        t = timed(fn, REP)
        ms[name] += t
        line[name + "_ms"] = round(statistics.median(t), 4)
    t = timed(torch_all, max(1, REP // 5))
    ms["torch"] += t
    line["torch_ms"] = round(statistics.median(t), 3)
    print(json.dumps(line), flush=True)

med = {k: statistics.median(v) for k, v in ms.items()}
summary = {"metric": "render flow, ms per call (median over %d runs x %d calls, device events): %d scenes x %d slots at %d x %d" % (RUNS, REP, B, S1, W, H),
           "torch_ms": round(med["torch"], 3), "torch_ms_min_max": [round(min(ms["torch"]), 3), round(max(ms["torch"]), 3)],
           "torch_over_planes": round(med["torch"] / med["planes"], 1),
           "torch_max_abs_flow_gap_px": gap, "torch_flag_mismatches": flag_diff,
           "pixels_valid_inside_visible": counts}
for name in cases:
    nbytes = model[name] * pixels
    summary[name] = {"ms": round(med[name], 4), "ms_min_max": [round(min(ms[name]), 4), round(max(ms[name]), 4)],
                     "model_bytes_per_pixel": model[name], "model_GBps": round(nbytes / (med[name] * 1e-3) / 1e9, 1),
                     "share_of_hbm_copy": round(nbytes / (med[name] * 1e-3) / (HBM_COPY_TBPS * 1e12), 3)}
print(json.dumps(summary))
