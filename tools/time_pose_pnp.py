#!/usr/bin/env python3
"""Developer tool (GPU box): the cost of the pose from correspondences (slhip_pose_pnp), timed with the HIP events of
slhip_pose_pnp_timing_enable, one shape per line:
  M = 2048 sets, K = 256 and K = 1024 correspondences, Hy = 256 hypotheses, 4 refinement steps, 30 % outliers, half a pixel of noise
  the same with Hy = 0 and the true pose as the initial one (the refinement and the final pass alone)
and for the first two the scoring stage's share of the VALU issue rate for its instruction count -- the arithmetic of the "Pose
errors" table in DESIGN.md: M * Hy * K point tests of SCORE_VALU instructions each (counted in the kernel's ISA, see DESIGN.md
"Pose PnP"), one instruction per lane and cycle on 256 CUs x 4 SIMDs x 16 lanes at 2.4 GHz.  The sets are made on the device from
a seed; the tool reads nothing outside the repository.  Prints one JSON line per shape.
    python tools/time_pose_pnp.py [repeats=10] [sets=2048]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import stillleben_amd as sl  # noqa: E402
from stillleben_amd import pose_pnp as pnp  # noqa: E402

import _step_timing  # noqa: E402

REP = max(3, int(sys.argv[1]) if len(sys.argv) > 1 else 10)
M = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
K4 = (572.4, 572.4, 320.0, 240.0)
SCORE_VALU = 53                            # VALU instructions of one point test: 213 per 4 tests in the main score loop (DESIGN.md "Pose PnP")
LANE_RATE = 256 * 4 * 16 * 2.4e9           # lane-instructions per second of the device
sl.init_cuda(0)
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev)
g.manual_seed(20261020)


def timed(fn, which, rep=REP, warm=2):
    return _step_timing.timed_step("pose_pnp", 2, which, fn, rep, warm)


def poses(n):
    q = torch.randn((n, 4), generator=g, device=dev)
    x, y, z, w = (q / q.norm(dim=-1, keepdim=True)).unbind(-1)
    T = torch.zeros((n, 3, 4), device=dev)
    T[:, :, :3] = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                               2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], dim=-1).view(n, 3, 3)
    T[:, 2, 3] = 0.4 + 1.1 * torch.rand(n, generator=g, device=dev)
    T[:, 0, 3] = (torch.rand(n, generator=g, device=dev) - 0.5) * 0.8 * T[:, 2, 3]
    T[:, 1, 3] = (torch.rand(n, generator=g, device=dev) - 0.5) * 0.6 * T[:, 2, 3]
    return T


def sets(K):
    """(uv [M, K, 2], xyz [M, K, 4], the true poses): a 0.1 m cube of points, 30 % of them replaced, half a pixel of noise"""
    T = poses(M)
    P = (torch.rand((M, K, 3), generator=g, device=dev) - 0.5) * 0.1
    X = P @ T[:, :, :3].transpose(1, 2) + T[:, None, :, 3]
    uv = torch.stack([K4[0] * X[..., 0] / X[..., 2] + K4[2], K4[1] * X[..., 1] / X[..., 2] + K4[3]], dim=-1)
    uv = uv + 0.5 * torch.randn(uv.shape, generator=g, device=dev)
    swap = torch.rand((M, K), generator=g, device=dev) < 0.3
    P = torch.where(swap[..., None], (torch.rand((M, K, 3), generator=g, device=dev) - 0.5) * 0.1, P)
    xyz = torch.cat([P, torch.ones((M, K, 1), device=dev)], dim=-1)
    return uv.contiguous(), xyz.contiguous(), T.contiguous()


for K in (256, 1024):
    uv, xyz, T = sets(K)
    for Hy in (256, 0):
        kw = dict(intrinsics=K4, n_hypotheses=Hy, threshold_px=2.0, refine_iters=4, seed=7)
        res, ms, all_ms = timed(lambda: pnp.solve(uv, xyz, init=T if Hy == 0 else None, **kw), 0)
        torch.cuda.synchronize()
        ok = res.flags == 0
        dt = (res.pose[:, :, 3] - T[:, :, 3]).norm(dim=-1)
        line = {"shape": "M%d_K%d_Hy%d_refine4" % (M, K, Hy), "ms": round(ms, 4), "ms_min_max": [round(min(all_ms), 4), round(max(all_ms), 4)],
                "repeats": REP, "sets_without_flags": int(ok.sum()), "median_inliers": int(res.n_inliers.median()),
                "median_translation_error_m": float(dt[ok].median()) if bool(ok.any()) else None}
        if Hy:
            tests = M * Hy * K
            line.update({"point_tests": tests, "score_valu_per_test": SCORE_VALU,
                         "score_share_of_valu_issue_rate": round(tests * SCORE_VALU / LANE_RATE / (ms * 1e-3), 3)})
        print(json.dumps(line))
