#!/usr/bin/env python3
"""Developer tool (GPU box): the cost of the pose errors (slhip_pose_error, slhip_pose_error_diameter), timed with the HIP events
of slhip_pose_error_timing_enable:
  evaluate  all four outputs (add, adds, mssd, mspd) at
              1024 scenes x 20 objects x 1 hypothesis, N = 1024 points, S = 1 symmetry
              the same with S = 315 (one continuous axis at max_step 0.01)
              1 x 64 x 32 (the sl.diff shape), N = 1024, S = 1
  diameter  21 classes at N = 4096
and beside each the plain-torch formulation of the same quantities a user would write today, in the same run on the same
inputs: torch.cdist in chunks of pose pairs that fit memory for ADD-S, a [chunk, S, N] distance tensor for MSSD and MSPD.  The
bank and the poses are made on the device from a seed.  Prints one JSON line.
    python tools/time_pose_error.py [repeats=10] [scenes=1024] [torch_repeats=2]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import stillleben_amd as sl  # noqa: E402
from stillleben_amd import pose_error as pe  # noqa: E402

import _step_timing  # noqa: E402

REP = max(3, int(sys.argv[1]) if len(sys.argv) > 1 else 10)
B = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
TORCH_REP = max(1, int(sys.argv[3]) if len(sys.argv) > 3 else 2)
OBJ, A, N = 20, 21, 1024
K4 = (1066.778, 1067.487, 312.9869, 241.3109)
sl.init_cuda(0)
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev)
g.manual_seed(20261019)


def timed(fn, which, rep=REP, warm=2):
    return _step_timing.timed_step("pose_error", 2, which, fn, rep, warm)


def torch_timed(fn, rep=TORCH_REP):
    fn()                                           # warm-up
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out, ms = None, []
    for _ in range(rep):
        ev[0].record()
        out = fn()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    return out, statistics.median(ms)


def make_bank(n_points, n_sym):
    points = torch.ones((A, n_points, 4), device=dev)
    points[..., :3] = (torch.rand((A, n_points, 3), generator=g, device=dev) - 0.5) * 0.2
    count = torch.full((A,), n_points, dtype=torch.int32, device=dev)
    sym = {c: pe.symmetry_transforms(continuous=[{"axis": [0, 0, 1], "offset": [0, 0, 0]}]) for c in range(A)} if n_sym > 1 else None
    return pe.bank(None, symmetries=sym, points=points, count=count)


def poses(shape, near=None):
    q = torch.randn(shape + (4,), generator=g, device=dev)
    q = q / q.norm(dim=-1, keepdim=True)
    x, y, z, w = q.unbind(-1)
    T = torch.zeros(shape + (3, 4), device=dev)
    T[..., :3] = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                              2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], dim=-1).view(shape + (3, 3))
    T[..., 2, 3] = 0.6 + torch.rand(shape, generator=g, device=dev)
    T[..., 0, 3] = (torch.rand(shape, generator=g, device=dev) - 0.5) * 0.5
    T[..., 1, 3] = (torch.rand(shape, generator=g, device=dev) - 0.5) * 0.4
    return T


def estimates(gt, Hy):
    """the ground truth moved by a few centimetres and degrees"""
    est = gt[:, :, None].repeat(1, 1, Hy, 1, 1)
    est = est + torch.randn(est.shape, generator=g, device=dev) * 0.02
    return est.contiguous()


def torch_errors(gt, est, classes, bank, chunk):
    """what a user writes today, a chunk of pose pairs at a time: (add, adds, mssd, mspd), each [P]"""
    Bq, O, Hy = est.shape[:3]
    P = Bq * O * Hy
    G = gt[:, :, None].expand(Bq, O, Hy, 3, 4).reshape(P, 3, 4)
    E = est.reshape(P, 3, 4)
    cls = classes.long()[:, :, None].expand(Bq, O, Hy).reshape(P)
    fx, fy, cx, cy = K4
    outs = [torch.empty(P, device=dev) for _ in range(4)]

    def proj(X):
        return torch.stack([fx * X[..., 0] / X[..., 2] + cx, fy * X[..., 1] / X[..., 2] + cy], dim=-1)

    for a in range(0, P, chunk):
        s = slice(a, a + chunk)
        p = bank.points[cls[s], :, :3]                                          # [c, N, 3]
        xe = p @ E[s, :, :3].transpose(1, 2) + E[s, None, :, 3]
        xg = p @ G[s, :, :3].transpose(1, 2) + G[s, None, :, 3]
        outs[0][s] = (xe - xg).norm(dim=-1).mean(dim=1)
        outs[1][s] = torch.cdist(xe, xg).min(dim=2).values.mean(dim=1)
        S = bank.symmetries[cls[s]]                                             # [c, S, 3, 4]
        ps = torch.einsum("csij,cnj->csni", S[..., :3], p) + S[:, :, None, :, 3]
        xs = torch.einsum("cij,csnj->csni", G[s, :, :3], ps) + G[s, None, None, :, 3]
        outs[2][s] = (xe[:, None] - xs).norm(dim=-1).max(dim=2).values.min(dim=1).values
        outs[3][s] = (proj(xe)[:, None] - proj(xs)).norm(dim=-1).max(dim=2).values.min(dim=1).values
    return outs


def shape_run(name, Bq, O, Hy, n_sym, chunk):
    bank = make_bank(N, n_sym)
    gt = poses((Bq, O))
    est = estimates(gt, Hy)
    classes = torch.randint(0, A, (Bq, O), generator=g, device=dev, dtype=torch.int32)
    err, ms, all_ms = timed(lambda: pe.evaluate(gt, est, classes, bank, K4), 1)
    base, torch_ms = torch_timed(lambda: torch_errors(gt, est, classes, bank, chunk))
    torch.cuda.synchronize()
    gaps = {}
    for k, b in zip(("add", "adds", "mssd", "mspd"), base):
        v = getattr(err, k).reshape(-1)
        ok = torch.isfinite(v) & torch.isfinite(b)
        gaps[k] = float((v[ok] - b[ok]).abs().max())      # torch's matmuls and norms are not the rule's roundings: a distance
    return {name + "_ms": round(ms, 4), name + "_ms_min_max": [round(min(all_ms), 4), round(max(all_ms), 4)],
            name + "_torch_ms": round(torch_ms, 3), name + "_torch_over_ours": round(torch_ms / ms, 1), name + "_max_abs_gap": gaps,
            name + "_pose_pairs": Bq * O * Hy, name + "_symmetries": int(bank.n_sym.max())}


result = {"metric": "pose errors, ms (median of %d, HIP events of the entry); torch: median of %d, torch events" % (REP, TORCH_REP),
          "points": N, "classes": A}
result.update(shape_run("b%dx%dx1_s1" % (B, OBJ), B, OBJ, 1, 1, 2048))
result.update(shape_run("b%dx%dx1_s315" % (B, OBJ), B, OBJ, 1, 315, 64))
result.update(shape_run("b1x64x32_s1", 1, 64, 32, 1, 2048))

big = make_bank(4096, 1)
_, diameter_ms, diameter_all = timed(lambda: pe.diameters(big), 0)


def torch_diameter():
    return torch.stack([torch.cdist(big.points[a, :, :3], big.points[a, :, :3]).max() for a in range(A)])


base, torch_diameter_ms = torch_timed(torch_diameter)
torch.cuda.synchronize()
result.update({"diameter_n4096_ms": round(diameter_ms, 4), "diameter_n4096_ms_min_max": [round(min(diameter_all), 4), round(max(diameter_all), 4)],
               "diameter_torch_ms": round(torch_diameter_ms, 3), "diameter_torch_over_ours": round(torch_diameter_ms / diameter_ms, 1),
               "diameter_max_abs_gap": float((pe.diameters(big) - base).abs().max())})
print(json.dumps(result))
