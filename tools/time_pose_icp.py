#!/usr/bin/env python3
"""Developer tool (GPU box): the cost of the ICP refinement (slhip_pose_icp), timed with the HIP events of
slhip_pose_icp_timing_enable: ms per launch at
  n in {1024, 16384} sets, K in {256, 1024} camera points per set, banks of 1024 and 4096 points per class (8 classes),
  5 fits per set (max_iters = 5 with tolerances of 0, so that every set runs them all), no gate
on sets made on the device from a seed: the bank's points lie on lumpy ellipsoids of 0.1 m, the camera points are a random
subset of the class's points under a random pose a metre away with 1 mm of noise, the initial pose is turned by 5 degrees and
shifted by 5 mm.  The cost model of DESIGN.md "ICP" -- K * count dist2 evaluations per iteration and set -- is printed beside
every measurement as evaluations per second.  The tool reads nothing outside the repository and ends after one pass.
Prints one JSON line per shape.
    python tools/time_pose_icp.py [repeats=5]"""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import stillleben_amd as sl  # noqa: E402
from stillleben_amd import pose_icp as pi  # noqa: E402

import _step_timing  # noqa: E402

REP = max(3, int(sys.argv[1]) if len(sys.argv) > 1 else 5)
A, ITERS = 8, 5
sl.init_cuda(0)
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev)
g.manual_seed(20261021)


def timed(fn, rep=REP, warm=1):
    return _step_timing.timed_step("pose_icp", 1, 0, fn, rep, warm)


def rotations(n, max_angle):
    """n rotations [n, 3, 3] by up to max_angle about random axes (Rodrigues)"""
    axis = torch.randn((n, 3), generator=g, device=dev)
    axis = axis / axis.norm(dim=1, keepdim=True)
    a = torch.rand((n,), generator=g, device=dev) * max_angle
    Kx = torch.zeros((n, 3, 3), device=dev)
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0], Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0], -axis[:, 1], axis[:, 0]
    return torch.eye(3, device=dev)[None] + torch.sin(a)[:, None, None] * Kx + (1 - torch.cos(a))[:, None, None] * (Kx @ Kx)


def model_bank(n_bank):
    u = torch.randn((A, n_bank, 3), generator=g, device=dev)
    u = u / u.norm(dim=2, keepdim=True)
    radii = 0.03 + 0.04 * torch.rand((A, 1, 3), generator=g, device=dev)
    lump = 1.0 + 0.2 * torch.sin(7.0 * u[..., :1]) * torch.cos(5.0 * u[..., 1:2])
    points = torch.ones((A, n_bank, 4), device=dev)
    points[..., :3] = u * radii * lump
    count = torch.full((A,), n_bank, dtype=torch.int32, device=dev)
    return sl.pose_error.bank(None, points=points.contiguous(), count=count)


def sets(bank, n, K):
    """(camera [n, K, 4], init [n, 3, 4], classes [n], truth [n, 3, 4])"""
    n_bank = bank.points.shape[1]
    classes = torch.randint(0, A, (n,), generator=g, device=dev, dtype=torch.int32)
    pick = torch.randint(0, n_bank, (n, K), generator=g, device=dev)
    p = bank.points[classes.long()[:, None], pick][..., :3]                             # [n, K, 3]
    Rg = rotations(n, math.pi)
    tg = torch.tensor([0.0, 0.0, 1.0], device=dev) + (torch.rand((n, 3), generator=g, device=dev) - 0.5) * 0.6
    cam = torch.ones((n, K, 4), device=dev)
    cam[..., :3] = p @ Rg.transpose(1, 2) + tg[:, None] + 0.001 * torch.randn((n, K, 3), generator=g, device=dev)
    Ri = Rg @ rotations(n, math.radians(5.0))
    shift = torch.randn((n, 3), generator=g, device=dev)
    ti = tg + 0.005 * shift / shift.norm(dim=1, keepdim=True)
    return (cam.contiguous(), torch.cat([Ri, ti[:, :, None]], 2).contiguous(), classes, torch.cat([Rg, tg[:, :, None]], 2))


for n_bank in (1024, 4096):
    bank = model_bank(n_bank)
    for n in (1024, 16384):
        for K in (256, 1024):
            cam, init, classes, truth = sets(bank, n, K)
            kw = dict(max_iters=ITERS, tol_rot=0.0, tol_trans=0.0)
            res, ms, all_ms = timed(lambda: pi.solve(cam, init, classes, bank, **kw))
            torch.cuda.synchronize()
            fits = int(res.iters.sum())
            before = (init - truth).flatten(1).norm(dim=1).median()
            after = (res.pose - truth).flatten(1).norm(dim=1)[res.found].median()
            print(json.dumps({"shape": "icp_n%d_K%d_bank%d" % (n, K, n_bank), "ms": round(ms, 4),
                              "ms_min_max": [round(min(all_ms), 4), round(max(all_ms), 4)], "repeats": REP, "found": int(res.found.sum()),
                              "fits": fits, "ms_per_fit_and_1024_sets": round(ms * 1024 / max(fits, 1), 5),
                              "dist2_per_s": round(fits * K * n_bank / (ms * 1e-3), 0), "lds_bytes": (3 * n_bank + K) * 4,
                              "median_pose_difference_before": float(before), "median_pose_difference_after": float(after)}), flush=True)
            del cam, init, classes, truth, res
