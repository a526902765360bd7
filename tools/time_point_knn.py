#!/usr/bin/env python3
"""Developer tool (GPU box): the cost of the point k-NN (slhip_point_knn), timed with the HIP events of
slhip_point_knn_timing_enable, against the torch route on the same device, shapes and run: torch.cdist + topk(largest=False),
over chunks of sets where cdist's [n, Q, R] matrix would pass 2 GiB, timed with HIP events round the whole route.  Shapes:
  objects   n = 1024 sets, Q = R = 1024, k = 16 (the point sets of a render batch, self-search)
  scene     n = 32 clouds, Q = R = 12288, k = 16 (FFB6D's clouds, level 0 of the pyramid)
  interp    n = 32, Q = 12288, R = 3072 (the first quarter of the same tensor), k = 1 (the up-sampling index)
  pyramid   n = 32, N = 12288, k = 16, ratios (4, 4, 4, 4): the 8 launches of sl.point_knn.pyramid, events round all of them
The two routes alternate within every repeat, after a warm-up of both; the medians and the spread are printed.  The cost model
of DESIGN.md "Point neighbours" -- n * Q * R dist2 evaluations -- is printed beside every measurement as evaluations per second.
The clouds are made on the device from a seed: uniform in a cube of side 1, in random order, w = 1.  The share of rows in which the torch
route names the same points in the same order is printed, not asserted: cdist rounds differently and breaks ties its own way.  The tool reads nothing outside the repository and ends after one pass.  Prints one JSON line per shape.
    python tools/time_point_knn.py [repeats=5]"""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import stillleben_amd as sl  # noqa: E402
from stillleben_amd import _abi  # noqa: E402
from stillleben_amd import point_knn as pk  # noqa: E402

REP = max(3, int(sys.argv[1]) if len(sys.argv) > 1 else 5)
WARM = 2
MATRIX_FLOATS = 1 << 29      # 2 GiB of cdist's matrix at a time
sl.init_cuda(0)
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev)
g.manual_seed(20261021)
L = _abi.lib()


def clouds(n, N):
    p = torch.ones((n, N, 4), device=dev)
    p[..., :3] = torch.rand((n, N, 3), generator=g, device=dev)
    return p.contiguous()


def torch_route(points, Q, R, k):
    """idx int64 [n, Q, k] by cdist + topk over chunks of sets"""
    n = points.shape[0]
    step = max(1, MATRIX_FLOATS // (Q * R))
    out = []
    for s in range(0, n, step):
        d = torch.cdist(points[s:s + step, :Q, :3], points[s:s + step, :R, :3])
        out.append(torch.topk(d, k, dim=2, largest=False).indices)
        del d
    return torch.cat(out)


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def kernel_ms():
    ms = (C.c_float * 1)()
    _abi.check(L.slhip_point_knn_timings(C.byref(ms)), "slhip_point_knn_timings")
    return float(ms[0])


def report(shape, evals, ours, theirs, extra):
    m_ours, m_torch = statistics.median(ours), statistics.median(theirs)
    print(json.dumps(dict(shape=shape, ms=round(m_ours, 4), ms_min_max=[round(min(ours), 4), round(max(ours), 4)], torch_ms=round(m_torch, 4),
                          torch_ms_min_max=[round(min(theirs), 4), round(max(theirs), 4)], torch_over_ours=round(m_torch / m_ours, 3),
                          repeats=REP, dist2_evaluations=evals, dist2_per_s=round(evals / (m_ours * 1e-3), 0),
                          torch_dist2_per_s=round(evals / (m_torch * 1e-3), 0), **extra)), flush=True)


def one_search(shape, points, Q, R, k):
    n = points.shape[0]
    ours, theirs = [], []
    _abi.check(L.slhip_point_knn_timing_enable(1), "slhip_point_knn_timing_enable")
    for rep in range(WARM + REP):      # the two routes alternate
        nb = pk.search(points, k=k, n_queries=Q, n_refs=R, outputs=("idx", "dist2"))
        t_ours = kernel_ms()
        ref, t_torch = events(lambda: torch_route(points, Q, R, k))
        if rep >= WARM:
            ours.append(t_ours)
            theirs.append(t_torch)
    _abi.check(L.slhip_point_knn_timing_enable(0), "slhip_point_knn_timing_enable")
    # the share of rows whose k distances are all different, and of rows where the two routes name the same points in the same order
    d = nb.dist2
    clear = (d[..., 1:] != d[..., :-1]).all(-1)
    agree = (nb.idx.long() == ref).all(-1)
    report(shape, n * Q * R, ours, theirs, dict(n=n, Q=Q, R=R, k=k, rows_equal_to_torch=round(float(agree.float().mean()), 6),
                                                rows_without_ties=round(float(clear.float().mean()), 6)))


def one_pyramid(shape, points, k, ratios):
    n, N = points.shape[:2]
    sizes = [N]
    for r in ratios:
        sizes.append(sizes[-1] // r)
    pairs = [(a, a, k) for a in sizes[:-1]] + [(a, b, 1) for a, b in zip(sizes[:-1], sizes[1:])]
    ours, theirs = [], []
    for rep in range(WARM + REP):
        pyr, t_ours = events(lambda: pk.pyramid(points, k=k, ratios=ratios))
        ref, t_torch = events(lambda: [torch_route(points, Q, R, kk) for Q, R, kk in pairs])
        if rep >= WARM:
            ours.append(t_ours)
            theirs.append(t_torch)
    report(shape, n * sum(Q * R for Q, R, _ in pairs), ours, theirs, dict(n=n, N=N, k=k, ratios=list(ratios), launches=len(pairs)))


objects = clouds(1024, 1024)
one_search("objects_n1024_Q1024_R1024_k16", objects, 1024, 1024, 16)
del objects
scene = clouds(32, 12288)
one_search("scene_n32_Q12288_R12288_k16", scene, 12288, 12288, 16)
one_search("interp_n32_Q12288_R3072_k1", scene, 12288, 3072, 1)
one_pyramid("pyramid_n32_N12288_k16_r4444", scene, 16, (4, 4, 4, 4))
