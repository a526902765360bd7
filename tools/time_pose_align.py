#!/usr/bin/env python3
"""Developer tool (GPU box): the cost of the robust alignment (slhip_pose_align), timed with the HIP events of
slhip_pose_align_timing_enable, one shape per line:
  M = 1280 sets, K = 9, 256 and 1024 correspondences, 256 hypotheses, 4 refits, 30 % of the rows moved by 0.05 to 0.3 m, 0.2 mm of noise
  K = 4096 once (the raised-LDS path)
and, at the same shapes, the route a user has without it, in batched PyTorch on the device (timed with torch events round the
whole route): random triples, batched torch.linalg.svd with the determinant correction (Kabsch), scoring of every hypothesis
against every point in chunks of hypotheses (a cdist-style broadcast), the best hypothesis per set, then 4 Kabsch refits on its
inliers.  Its draws are torch's own, so the two routes do not pick the same triples; the comparison is of cost at equal work,
and of the inliers both find.  The sets are made on the device from a seed; the tool reads nothing outside the repository.
Prints one JSON line per shape and route.
    python tools/time_pose_align.py [repeats=10] [sets=1280]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import stillleben_amd as sl  # noqa: E402
from stillleben_amd import pose_align as pa  # noqa: E402

import _step_timing  # noqa: E402

REP = max(3, int(sys.argv[1]) if len(sys.argv) > 1 else 10)
M = int(sys.argv[2]) if len(sys.argv) > 2 else 1280
HY, REFITS, THR = 256, 4, 1e-3
sl.init_cuda(0)
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev)
g.manual_seed(20261021)


def sets(m, K):
    """(src [m, K, 4], dst [m, K, 4], clean bool [m, K]): a 0.1 m cube of points about a metre away under a random motion"""
    q = torch.randn((m, 4), generator=g, device=dev)
    x, y, z, w = (q / q.norm(dim=-1, keepdim=True)).unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                     2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], dim=-1).view(m, 3, 3)
    t = torch.tensor([0.1, -0.05, 1.0], device=dev) + 0.1 * torch.randn((m, 3), generator=g, device=dev)
    P = (torch.rand((m, K, 3), generator=g, device=dev) - 0.5) * 0.1
    X = P @ R.transpose(1, 2) + t[:, None] + 2e-4 * torch.randn((m, K, 3), generator=g, device=dev)
    hit = torch.rand((m, K), generator=g, device=dev) < 0.3
    way = torch.randn((m, K, 3), generator=g, device=dev)
    way = way / way.norm(dim=-1, keepdim=True) * (0.05 + 0.25 * torch.rand((m, K, 1), generator=g, device=dev))
    P = torch.where(hit[..., None], P + way, P)
    one = torch.ones((m, K, 1), device=dev)
    return torch.cat([P, one], -1).contiguous(), torch.cat([X, one], -1).contiguous(), ~hit


def kabsch(a, b, w=None):
    """the rigid motions of a [..., n, 3] onto b [..., n, 3] (weights w [..., n] or all one): R [..., 3, 3], t [..., 3]"""
    w = torch.ones(a.shape[:-1], device=a.device) if w is None else w
    n = w.sum(-1, keepdim=True).clamp_min(1.0)
    ca, cb = (a * w[..., None]).sum(-2) / n, (b * w[..., None]).sum(-2) / n
    H = ((a - ca[..., None, :]) * w[..., None]).transpose(-1, -2) @ (b - cb[..., None, :])
    U, _, Vh = torch.linalg.svd(H)
    V = Vh.transpose(-1, -2)
    d = torch.sign(torch.linalg.det(V @ U.transpose(-1, -2)))
    D = torch.diag_embed(torch.stack([torch.ones_like(d), torch.ones_like(d), d], -1))
    R = V @ D @ U.transpose(-1, -2)
    return R, cb - (R @ ca[..., None])[..., 0]


def torch_route(src, dst, chunk=32):
    """(inlier mask [m, K], R, t) by RANSAC in batched torch: HY triples, SVD Kabsch, broadcast scoring, REFITS refits"""
    m, K = src.shape[:2]
    a, b = src[..., :3], dst[..., :3]
    idx = torch.randint(0, K, (m, HY, 3), device=dev)
    rows = torch.arange(m, device=dev)[:, None, None]
    R, t = kabsch(a[rows, idx], b[rows, idx])                                           # [m, HY, 3, 3], [m, HY, 3]
    count = torch.empty((m, HY), dtype=torch.int32, device=dev)
    for h in range(0, HY, chunk):      # [m, chunk, K, 3] at a time: the whole [m, HY, K, 3] does not fit at K = 1024
        moved = a[:, None] @ R[:, h:h + chunk].transpose(-1, -2) + t[:, h:h + chunk, None]
        count[:, h:h + chunk] = ((moved - b[:, None]).norm(dim=-1) <= THR).sum(-1)
    best = count.argmax(1)
    R, t = R[rows[:, 0, 0], best], t[rows[:, 0, 0], best]
    for _ in range(REFITS):
        inl = ((a @ R.transpose(-1, -2) + t[:, None] - b).norm(dim=-1) <= THR).float()
        R, t = kabsch(a, b, inl)
    return (a @ R.transpose(-1, -2) + t[:, None] - b).norm(dim=-1) <= THR, R, t


def torch_timed(fn, rep=REP, warm=2):
    ms, out = [], None
    for r in range(warm + rep):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        if r >= warm:
            ms.append(e0.elapsed_time(e1))
    return out, statistics.median(ms), ms


for m, K in ((M, 9), (M, 256), (M, 1024), (M, 4096)):
    src, dst, clean = sets(m, K)
    res, ms, all_ms = _step_timing.timed_step("pose_align", 1, 0, lambda: pa.solve(src, dst, threshold=THR, n_hypotheses=HY, refine_iters=REFITS, seed=7), REP)
    torch.cuda.synchronize()
    shape = "M%d_K%d_Hy%d_refit%d" % (m, K, HY, REFITS)
    print(json.dumps({"route": "slhip_pose_align", "shape": shape, "ms": round(ms, 4), "ms_min_max": [round(min(all_ms), 4), round(max(all_ms), 4)],
                      "repeats": REP, "sets_found": int(res.found.sum()), "sets_with_exactly_the_untouched_rows": int((res.inlier_mask() == clean).all(1).sum()),
                      "point_tests": m * HY * K}))
    (mask, _, _), ms, all_ms = torch_timed(lambda: torch_route(src, dst))
    print(json.dumps({"route": "torch_svd_ransac", "shape": shape, "ms": round(ms, 4), "ms_min_max": [round(min(all_ms), 4), round(max(all_ms), 4)],
                      "repeats": REP, "sets_with_exactly_the_untouched_rows": int((mask == clean).all(1).sum())}))
