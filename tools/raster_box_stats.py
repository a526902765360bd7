#!/usr/bin/env python3
"""Developer tool (CPU only, no GPU call): what the two rasterisers of slhip_render.hip are asked to walk, from host records.

    python tools/raster_box_stats.py --poses DIR [--scenes 4]

DIR holds `object_poses.npy` [n, 20, 4, 4] and `camera_poses.npy` [n, 4, 4] as `bench.py --dump-outputs DIR` writes them: settled
object and camera poses of real benchmark scenes.  Every scene is rebuilt as an ordinary sl.Scene of the benchmark's shape
(bench.make_scene: 20 of the 21 YCB-like meshes, the 3 x 3 m plane, one light), the dumped poses are set, a light direction is
drawn with the scene's own choose_random_light_direction(), and the batch goes through the normal host path
(_batch.build_batch: scene, draw and chunk records, shadow matrices).  The dump does not say which class sits at which pose and
not where the light was: both are drawn afresh here -- the meshes are all of 8 k vertices / 16 k triangles and 0.1 - 0.25 m, so
box statistics carry over, single triangles do not.

The casters are then projected with `shadow_mat` and set up as setup_finish() does it -- snap to 1/256 px, signed area and
facing, pixel box, clamp to the 2048^2 map -- in numpy; the vertex transform is a float32 matrix product here and a MFMA product
in k_vertex_xform, so a vertex may land one sub-pixel beside the kernel's.  Per scene it prints

  * triangles, the share that draws nothing (light-facing, zero area, off the map, box without a texel centre), the share queued
    (box > kSmallArea texels);
  * box-texel visits of the in-place triangles against the texels they cover (the exact inside test, top-left rule included);
  * the distribution of ex * ey (vertex extents in sub-pixels) and the share of in-place / queued triangles under the narrow
    bound of slhip_raster_walk.h;
  * per chunk (256 consecutive triangles of a draw): chunks that walk nothing, and the union box of the walked triangles against
    the 64 x 64 LDS window of k_shadow_raster -- what a sized clear / flush would touch against 4096 texels;
  * the same figures for the camera view (no facing cull there).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SMALL_AREA = 256                 # kSmallArea of slhip_render.hip
WINDOW = 64                      # SLHIP_SHADOW_WINDOW
NARROW_MAX = 1 << 29             # slhip_raster::kNarrowMax
SHADOW_RES = 2048


def snap(w):
    """snap() of slhip_render.hip on a float32 array."""
    s = np.floor(w.astype(np.float32) * np.float32(256.0) + np.float32(0.5))      # fmaf: exact here up to the last bit
    s = np.where(np.isnan(s), np.float32(0.0), s)
    return np.clip(s, -67108864.0, 67108864.0).astype(np.int64)


def window_coords(M, pos, half_w, half_h):
    """screen_vertex() of every vertex: clip = M pos (float32), X / Y snapped.  Returns X, Y (int64) and `front`, the inside
    test of clip_near()."""
    clip = (pos.astype(np.float32) @ M.astype(np.float32).T).astype(np.float32)
    w = clip[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        xn, yn = clip[:, 0] / w, clip[:, 1] / w
    X = snap(xn * np.float32(half_w) + np.float32(half_w))
    Y = snap(yn * np.float32(half_h) + np.float32(half_h))
    return X, Y, clip[:, 2] >= -w


def setup(X, Y, W, H):
    """setup_finish() of T triangles: X, Y [T, 3] int64.  Returns a dict of arrays; `ok` = it returns true."""
    area2 = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
    flipped = area2 < 0
    xmn, xmx, ymn, ymx = X.min(1), X.max(1), Y.min(1), Y.max(1)
    x0, x1 = np.maximum((xmn - 128 + 255) >> 8, 0), np.minimum((xmx - 128) >> 8, W - 1)
    y0, y1 = np.maximum((ymn - 128 + 255) >> 8, 0), np.minimum((ymx - 128) >> 8, H - 1)
    ok = (area2 != 0) & (x0 <= x1) & (y0 <= y1)
    ex, ey = xmx - xmn, ymx - ymn
    narrow = (256 * np.maximum(ex, ey) <= NARROW_MAX) & (ex * ey <= NARROW_MAX)
    bias = np.zeros((len(X), 3), np.int64)
    for i in range(3):
        a, b = (i + 1) % 3, (i + 2) % 3
        dx, dy = X[:, b] - X[:, a], Y[:, b] - Y[:, a]
        dx, dy = np.where(flipped, -dx, dx), np.where(flipped, -dy, dy)
        bias[:, i] = np.where((dy < 0) | ((dy == 0) & (dx < 0)), 0, -1)
    return dict(area2=np.abs(area2), flipped=flipped, ok=ok, xmin=x0, xmax=x1, ymin=y0, ymax=y1, ex=ex, ey=ey, narrow=narrow,
                bias=bias, n=np.where(ok, (x1 - x0 + 1) * (y1 - y0 + 1), 0))


def covered_texels(X, Y, t, sel):
    """Texels of the boxes of the triangles `sel` (indices) that pass the biased inside test: the walk of raster_bbox()."""
    total = 0
    for lo in range(0, len(sel), 20000):           # bounded memory: at most 20 000 boxes of <= kSmallArea texels at a time
        s = sel[lo:lo + 20000]
        n = t["n"][s]
        owner = np.repeat(np.arange(len(s)), n)
        k = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
        bw = (t["xmax"][s] - t["xmin"][s] + 1)[owner]
        cx = 256 * (t["xmin"][s][owner] + k % bw) + 128
        cy = 256 * (t["ymin"][s][owner] + k // bw) + 128
        inside = np.ones(len(owner), bool)
        Xs, Ys, fl, bias = X[s][owner], Y[s][owner], t["flipped"][s][owner], t["bias"][s][owner]
        for i in range(3):
            a, b = (i + 1) % 3, (i + 2) % 3
            e = (Xs[:, b] - Xs[:, a]) * (cy - Ys[:, a]) - (Ys[:, b] - Ys[:, a]) * (cx - Xs[:, a])
            inside &= np.where(fl, -e, e) + bias[:, i] >= 0
        total += int(inside.sum())
    return total


def pct(a, qs=(50, 90, 99, 100)):
    return "/".join("%d" % v for v in np.percentile(a, qs)) if len(a) else "-"


def view_stats(label, X, Y, tri_chunk, n_chunks, W, H, cull_flipped, windowed):
    """X, Y [T, 3]; tri_chunk [T]: the chunk of every triangle."""
    t = setup(X, Y, W, H)
    drawn = t["ok"] & ~(t["flipped"] if cull_flipped else False)
    queued = drawn & (t["n"] > SMALL_AREA)
    walked = drawn & ~queued
    T = len(X)
    sel = np.nonzero(walked)[0]
    visits = int(t["n"][sel].sum())
    cov = covered_texels(X, Y, t, sel)
    print("  %s: %d triangles in %d chunks; nothing drawn %.1f %%, queued %.2f %%, walked in place %.1f %%"
          % (label, T, n_chunks, 100.0 * (1 - drawn.mean()), 100.0 * queued.mean(), 100.0 * walked.mean()))
    print("    in-place walk: %d box texels visited, %d covered (%.1f %%); box texels per triangle p50/p90/p99/max %s"
          % (visits, cov, 100.0 * cov / max(visits, 1), pct(t["n"][sel])))
    exey = (t["ex"] * t["ey"])
    print("    ex*ey of the walked triangles p50/p90/p99/max %s (bound %d); under the narrow bound: walked %.3f %%, queued %.3f %%"
          % (pct(exey[sel]), NARROW_MAX, 100.0 * t["narrow"][sel].mean() if len(sel) else 0.0,
             100.0 * t["narrow"][queued].mean() if queued.any() else 0.0))
    if windowed is None:
        return
    big = np.iinfo(np.int64).max
    ux0 = np.full(n_chunks, big); uy0 = np.full(n_chunks, big); ux1 = np.full(n_chunks, -1); uy1 = np.full(n_chunks, -1)
    c = tri_chunk[sel]
    np.minimum.at(ux0, c, t["xmin"][sel]); np.minimum.at(uy0, c, t["ymin"][sel])
    np.maximum.at(ux1, c, t["xmax"][sel]); np.maximum.at(uy1, c, t["ymax"][sel])
    any_drawn = np.zeros(n_chunks, bool)
    any_drawn[tri_chunk[drawn]] = True
    has = ux1 >= 0
    w, h = (ux1 - ux0 + 1)[has], (uy1 - uy0 + 1)[has]
    wc, hc = np.minimum(w, WINDOW), np.minimum(h, WINDOW)
    cols = np.where(wc > 1, 1 << np.ceil(np.log2(np.maximum(wc, 1))).astype(np.int64), 1)
    touched = hc * cols
    print("    chunks: %.1f %% walk nothing (%.1f %% draw nothing at all); union box of the walked triangles w p50/p90/p99/max %s, "
          "h %s" % (100.0 * (1 - has.mean()), 100.0 * (1 - any_drawn.mean()), pct(w), pct(h)))
    print("    union box n 64x64 window: more than half the window in %.1f %% of the walking chunks; texels cleared and scanned "
          "(rows x columns rounded up to a power of two) mean %.0f of 4096, over ALL chunks %.0f"
          % (100.0 * (wc * hc > WINDOW * WINDOW // 2).mean() if len(w) else 0.0, touched.mean() if len(w) else 0.0,
             touched.sum() / max(n_chunks, 1)))


def scene_stats(si, srec, drec, crec, pos, idx, W, H):
    from stillleben_amd import _abi

    s = srec[si]
    chunks = crec[crec["scene"] == si]
    for view in ("light 0", "camera"):
        Xs, Ys, cs, n_chunks = [], [], [], 0
        for d_i in np.unique(chunks["draw"]):
            d = drec[d_i]
            if view != "camera" and not (int(d["flags"]) & _abi.DRAW_CASTS_SHADOW):
                continue
            T1 = (d["object_to_world"].reshape(4, 4).astype(np.float32) @ d["mesh_to_object"].reshape(4, 4).astype(np.float32)).astype(np.float32)
            if view == "camera":
                Mv = (s["proj"].reshape(4, 4) @ (s["world_to_cam"].reshape(4, 4) @ T1).astype(np.float32)).astype(np.float32)
                hw, hh = 0.5 * W, 0.5 * H
            else:
                Mv = (s["shadow_mat"][0].reshape(4, 4) @ T1).astype(np.float32)
                hw = hh = 0.5 * SHADOW_RES
            v = pos[int(d["vtx_base"]):int(d["vtx_base"]) + int(d["n_verts"])]
            X, Y, front = window_coords(Mv, v, hw, hh)
            tri = idx[int(d["idx_base"]):int(d["idx_base"]) + 3 * int(d["n_tris"])].reshape(-1, 3).astype(np.int64)
            keep = front[tri].all(axis=1)                 # (the few near-clipped triangles of the camera view are left out)
            chunk_of = np.zeros(len(tri), np.int64)
            for ch in chunks[chunks["draw"] == d_i]:
                chunk_of[int(ch["first_tri"]):int(ch["first_tri"]) + int(ch["count"])] = n_chunks
                n_chunks += 1
            Xs.append(X[tri][keep]); Ys.append(Y[tri][keep]); cs.append(chunk_of[keep])
        X, Y, c = np.concatenate(Xs), np.concatenate(Ys), np.concatenate(cs)
        if view == "camera":
            view_stats(view, X, Y, c, n_chunks, W, H, cull_flipped=False, windowed=None)
        else:
            view_stats(view, X, Y, c, n_chunks, SHADOW_RES, SHADOW_RES, cull_flipped=True, windowed=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--poses", required=True, help="directory of bench.py --dump-outputs (object_poses.npy, camera_poses.npy)")
    ap.add_argument("--scenes", type=int, default=4, help="scenes of the dump to look at (the first N)")
    args = ap.parse_args()

    import torch

    import bench
    import stillleben_amd as sl
    from stillleben_amd import synthetic
    from stillleben_amd._batch import HostPool, build_batch

    sl.init()
    obj_poses = np.load(os.path.join(args.poses, "object_poses.npy"))
    cam_poses = np.load(os.path.join(args.poses, "camera_poses.npy"))
    n = min(args.scenes, len(obj_poses))
    meshes = synthetic.ycb_like_meshes(seed=0, tex_size=64)        # geometry only: small textures
    scenes = []
    for i in range(n):
        sc = bench.make_scene(sl, meshes, 1000 + i)
        for o, pose in zip(sc.objects, obj_poses[i]):
            o.set_pose(torch.from_numpy(pose.astype(np.float32)))
        sc.set_camera_pose(torch.from_numpy(cam_poses[i].astype(np.float32)))
        sc.choose_random_light_direction()
        scenes.append(sc)
    pool = HostPool()
    srec, drec, crec = build_batch(scenes, pool, with_shadows=True)
    arrays = pool.arrays()
    pos, idx = arrays[0], arrays[4]
    W, H = bench.RESOLUTION
    print("raster_box_stats: %d scenes of %s, %d draws, %d chunks (%.0f per scene); shadow map %d^2, window %d^2, kSmallArea %d"
          % (n, args.poses, len(drec), len(crec), len(crec) / n, SHADOW_RES, WINDOW, SMALL_AREA))
    for i in range(n):
        print("scene %d" % i)
        scene_stats(i, srec, drec, crec, pos, idx, W, H)


if __name__ == "__main__":
    main()
