#!/usr/bin/env python3
"""Developer tool (GPU box): the cost of the keypoint voting (slhip_keypoint_vote), timed with the HIP events of
slhip_keypoint_vote_timing_enable, one shape per line:
  M = 2048 sets, Kp = 9 keypoints, K = 1024 voters, Hy = 128 hypotheses, 30 % of the vectors replaced, half a degree of noise,
  once on gathered vectors [M, K, Kp, 2] and once on a dense field [16, 480, 640, Kp, 2] (128 sets per picture)
  the same at K = 256
and the torch formulation of the same step (pairs, meeting points, the [m, Kp, Hy, K] score, arg-max, one least-squares step) on a
slice of 32 sets, the most whose intermediates fit comfortably, timed with torch's events and scaled to M sets.  The sets are made on
the device from a seed; the tool reads nothing outside the repository.  Prints one JSON line per shape.
    python tools/time_keypoint_vote.py [repeats=10] [sets=2048]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import stillleben_amd as sl  # noqa: E402
from stillleben_amd import _abi  # noqa: E402
from stillleben_amd import keypoint_vote as kv  # noqa: E402

import _step_timing  # noqa: E402

REP = max(3, int(sys.argv[1]) if len(sys.argv) > 1 else 10)
M = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
KP, HY, SIZE, SCENES, SLICE = 9, 128, (640, 480), 16, 32
COS = 0.99
sl.init_cuda(0)
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev)
g.manual_seed(20261020)


def timed(fn, which, rep=REP, warm=2):
    return _step_timing.timed_step("keypoint_vote", 2, which, fn, rep, warm)


def sets(K):
    """(pixel int16 [M, K, 2], vectors [M, K, Kp, 2], keypoints [M, Kp, 2]): K distinct pixels of a 64 x 64 window, unit vectors
    towards keypoints in and round it, half a degree of noise, 30 % of them replaced by uniform directions"""
    x0 = torch.randint(0, SIZE[0] - 64, (M, 1), generator=g, device=dev)
    y0 = torch.randint(0, SIZE[1] - 64, (M, 1), generator=g, device=dev)
    cells = torch.rand((M, 4096), generator=g, device=dev).argsort(dim=1)[:, :K]
    pixel = torch.stack([x0 + cells % 64, y0 + cells // 64], dim=-1).to(torch.int16).contiguous()
    kps = torch.stack([x0, y0], dim=-1).float() + (torch.rand((M, KP, 2), generator=g, device=dev) * 1.4 - 0.2) * 64.0
    to = kps[:, None] - (pixel.float() + 0.5)[:, :, None]
    ang = torch.atan2(to[..., 1], to[..., 0]) + 0.5 * torch.pi / 180.0 * torch.randn((M, K, KP), generator=g, device=dev)
    swap = torch.rand((M, K, KP), generator=g, device=dev) < 0.3
    ang = torch.where(swap, torch.rand((M, K, KP), generator=g, device=dev) * (2.0 * torch.pi), ang)
    return pixel, torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1).contiguous(), kps


def torch_vote(pixel, vec):
    """the same step in torch on m sets: positions [m, Kp, 2]; the [m, Kp, Hy, K] intermediates are what limits m"""
    m, K = pixel.shape[:2]
    p = pixel.float() + 0.5                                                      # [m, K, 2]
    d = vec.permute(0, 2, 1, 3)                                                  # [m, Kp, K, 2]
    ab = torch.randint(0, K, (m, KP, HY, 2), device=pixel.device)
    pa, pb = (torch.gather(p[:, None].expand(-1, KP, -1, -1), 2, ab[..., i:i + 1].expand(-1, -1, -1, 2)) for i in (0, 1))
    da, db = (torch.gather(d, 2, ab[..., i:i + 1].expand(-1, -1, -1, 2)) for i in (0, 1))
    det = da[..., 0] * db[..., 1] - da[..., 1] * db[..., 0]
    s = ((pb[..., 0] - pa[..., 0]) * db[..., 1] - (pb[..., 1] - pa[..., 1]) * db[..., 0]) / det
    q = pa + s[..., None] * da                                                   # [m, Kp, Hy, 2]
    q = torch.where((det.abs() > 1e-3)[..., None], q, torch.full_like(q, float("nan")))
    e = q[:, :, :, None] - p[:, None, None]                                      # [m, Kp, Hy, K, 2]
    dot = (e * d[:, :, None]).sum(-1)
    inl = (dot > 0) & (dot * dot >= COS * COS * (e * e).sum(-1))
    best = inl.sum(-1).argmax(-1)                                                # [m, Kp]
    qb = torch.gather(q, 2, best[..., None, None].expand(-1, -1, 1, 2))[:, :, 0]
    w = torch.gather(inl, 2, best[..., None, None].expand(-1, -1, 1, K))[:, :, 0].float()      # [m, Kp, K]
    n = torch.stack([-d[..., 1], d[..., 0]], -1)
    c = (n * (p[:, None] - qb[:, :, None])).sum(-1)
    A = torch.einsum("mpk,mpki,mpkj->mpij", w, n, n)
    b = torch.einsum("mpk,mpki,mpk->mpi", w, n, c)
    return qb + torch.linalg.solve(A, b[..., None])[..., 0]


for K in (1024, 256):
    pixel, vec, kps = sets(K)
    kw = dict(n_hypotheses=HY, inlier_cos=COS, seed=7)
    field = torch.randn((SCENES, SIZE[1], SIZE[0], KP, 2), generator=g, device=dev)
    scene = (torch.arange(M, device=dev) % SCENES).to(torch.int32)
    field[scene.long()[:, None], pixel[..., 1].long(), pixel[..., 0].long()] = vec      # (sets of one picture may overlap: timing only)
    for mode in ("gathered", "dense"):
        if mode == "gathered":
            res, ms, all_ms = timed(lambda: kv.vote(pixel, vectors=vec, size=SIZE, **kw), 0)
        else:
            res, ms, all_ms = timed(lambda: kv.vote(pixel, field=field, scene=scene, **kw), 1)
        torch.cuda.synchronize()
        line = {"shape": "M%d_Kp%d_K%d_Hy%d_%s" % (M, KP, K, HY, mode), "ms": round(ms, 4), "ms_min_max": [round(min(all_ms), 4), round(max(all_ms), 4)],
                "repeats": REP, "found": int(res.found.sum()), "of": M * KP, "median_inliers": int(res.n_inliers.median()),
                "refine_rejected": int(((res.flags & _abi.VOTE_REFINE_REJECTED) != 0).sum()),
                "voter_tests": M * KP * HY * K}
        if mode == "gathered":
            line["median_error_px"] = float((res.uv - kps).norm(dim=-1)[res.found].median())
        print(json.dumps(line))
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for r in range(2 + REP):
        start.record()
        uv = torch_vote(pixel[:SLICE], vec[:SLICE])
        stop.record()
        torch.cuda.synchronize()
        if r >= 2:
            ms.append(start.elapsed_time(stop))
    med = statistics.median(ms)
    print(json.dumps({"shape": "torch_M%d_Kp%d_K%d_Hy%d" % (SLICE, KP, K, HY), "ms": round(med, 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)],
                      "repeats": REP, "scaled_to_sets": M, "ms_scaled": round(med * M / SLICE, 2),
                      "intermediate_elements": SLICE * KP * HY * K, "median_error_px": float((uv - kps[:SLICE]).norm(dim=-1).nanmedian())}))
    del field
