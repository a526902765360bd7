#!/usr/bin/env python3
"""Developer tool (GPU box): the cost of the keypoint voting in 3D (slhip_keypoint_vote3d), timed with the HIP events of
slhip_keypoint_vote3d_timing_enable, at
  M = 1280 sets (20 scenes x 64 objects), Kp = 9 keypoints, K = 1024 voters, S = 128 seeds, h = 0.05 m, tol = 1e-4 m,
  offsets with 5 mm of Gaussian noise, 30 % of them replaced by vectors of up to half a metre
and the torch formulation of the same rules on the same device -- for every (set, keypoint) an [S, K] tensor of squared distances
per iteration, every seed stepped until all have stopped -- on a slice of 32 sets, the most whose intermediates fit comfortably,
timed with torch's events and scaled to M sets; then the rigid fit (slhip_pose_fit) of the voted keypoints onto the true ones.
The sets are made on the device from a seed; the tool reads nothing outside the repository.  Prints one JSON line per shape.
    python tools/time_keypoint_vote3d.py [repeats=10] [sets=1280]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import stillleben_amd as sl  # noqa: E402
from stillleben_amd import _abi  # noqa: E402
from stillleben_amd import keypoint_vote3d as kv  # noqa: E402
from stillleben_amd import pose_fit as pf  # noqa: E402

import _step_timing  # noqa: E402

REP = max(3, int(sys.argv[1]) if len(sys.argv) > 1 else 10)
M = int(sys.argv[2]) if len(sys.argv) > 2 else 1280
KP, K, S, H, TOL, ITERS, SLICE = 9, 1024, 128, 0.05, 1e-4, 32, 32
sl.init_cuda(0)
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev)
g.manual_seed(20261020)


def timed(fn, entry, rep=REP, warm=2):
    return _step_timing.timed_step(entry, 1, 0, fn, rep, warm)


def sets():
    """(camera [M, K, 4], offsets [M, K, Kp, 3], keypoints [M, Kp, 3])"""
    centre = torch.tensor([0.0, 0.0, 1.0], device=dev) + (torch.rand((M, 1, 3), generator=g, device=dev) - 0.5) * 0.6
    cam = torch.ones((M, K, 4), device=dev)
    cam[..., :3] = centre + (torch.rand((M, K, 3), generator=g, device=dev) - 0.5) * 0.2
    kps = centre + (torch.rand((M, KP, 3), generator=g, device=dev) - 0.5) * 0.25
    off = kps[:, None] - cam[:, :, None, :3] + 0.005 * torch.randn((M, K, KP, 3), generator=g, device=dev)
    wild = torch.rand((M, K, KP, 1), generator=g, device=dev) < 0.3
    off = torch.where(wild, torch.rand((M, K, KP, 3), generator=g, device=dev) - 0.5, off)
    return cam.contiguous(), off.contiguous(), kps


def torch_vote(cam, off):
    """the same rules in torch on m sets: (modes [m, Kp, 3], steps taken); the [m, Kp, S, K] intermediates are what limits m"""
    m = cam.shape[0]
    c = (cam[:, :, None, :3] + off).permute(0, 2, 1, 3).contiguous()             # [m, Kp, K, 3]
    rank = ((2 * torch.arange(S, device=cam.device) + 1) * K) // (2 * S)
    x = c[:, :, rank]                                                            # [m, Kp, S, 3]
    live = torch.ones((m, KP, S), dtype=torch.bool, device=cam.device)
    steps = 0
    for steps in range(1, ITERS + 1):
        d = c[:, :, None] - x[:, :, :, None]                                     # [m, Kp, S, K, 3]
        t = (d * d).sum(-1) / (H * H)
        w = torch.where(t < 1.0, 1.0 - t, torch.zeros_like(t))
        shift = (w[..., None] * d).sum(3) / w.sum(3)[..., None]
        x = torch.where(live[..., None], x + shift, x)
        live = live & ((shift * shift).sum(-1) > TOL * TOL)
        if not bool(live.any()):
            break
    support = (((c[:, :, None] - x[:, :, :, None]) ** 2).sum(-1) <= H * H).sum(-1)      # [m, Kp, S]
    best = support.argmax(-1)
    return torch.gather(x, 2, best[..., None, None].expand(-1, -1, 1, 3))[:, :, 0], steps


cam, off, kps = sets()
kw = dict(n_seeds=S, bandwidth=H, tol=TOL, max_iters=ITERS)
res, ms, all_ms = timed(lambda: kv.vote(cam, off, **kw), "keypoint_vote3d")
torch.cuda.synchronize()
print(json.dumps({"shape": "vote3d_M%d_Kp%d_K%d_S%d" % (M, KP, K, S), "ms": round(ms, 4), "ms_min_max": [round(min(all_ms), 4), round(max(all_ms), 4)],
                  "repeats": REP, "found": int(res.found.sum()), "of": M * KP, "median_support": int(res.n_support.median()),
                  "median_iters": int(res.iters.median()), "max_iters": int(res.iters.max()),
                  "not_converged": int(((res.flags & _abi.VOTE3D_NOT_CONVERGED) != 0).sum()),
                  "median_error_m": float((res.xyz - kps).norm(dim=-1)[res.found].median())}))

start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
t_ms, steps = [], 0
for r in range(2 + REP):
    start.record()
    xyz, steps = torch_vote(cam[:SLICE], off[:SLICE])
    stop.record()
    torch.cuda.synchronize()
    if r >= 2:
        t_ms.append(start.elapsed_time(stop))
med = statistics.median(t_ms)
print(json.dumps({"shape": "torch_M%d_Kp%d_K%d_S%d" % (SLICE, KP, K, S), "ms": round(med, 4), "ms_min_max": [round(min(t_ms), 4), round(max(t_ms), 4)],
                  "repeats": REP, "steps": steps, "scaled_to_sets": M, "ms_scaled": round(med * M / SLICE, 2),
                  "intermediate_elements": SLICE * KP * S * K * 3,
                  "worst_distance_from_the_kernel_m": float((xyz - res.xyz[:SLICE]).norm(dim=-1).max())}))

src = torch.ones((M, KP, 4), device=dev)
src[..., :3] = (torch.rand((1, KP, 3), generator=g, device=dev) - 0.5) * 0.25
dst = torch.cat([res.xyz, res.found.float()[..., None]], -1).contiguous()
fit, ms, all_ms = timed(lambda: pf.solve(src, dst), "pose_fit")
torch.cuda.synchronize()
print(json.dumps({"shape": "fit_M%d_N%d" % (M, KP), "ms": round(ms, 4), "ms_min_max": [round(min(all_ms), 4), round(max(all_ms), 4)], "repeats": REP}))
big_src = torch.ones((M, K, 4), device=dev)
big_src[..., :3] = torch.rand((M, K, 3), generator=g, device=dev) - 0.5
fit, ms, all_ms = timed(lambda: pf.solve(big_src, cam), "pose_fit")
torch.cuda.synchronize()
print(json.dumps({"shape": "fit_M%d_N%d" % (M, K), "ms": round(ms, 4), "ms_min_max": [round(min(all_ms), 4), round(max(all_ms), 4)], "repeats": REP}))
