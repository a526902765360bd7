#!/usr/bin/env python3
"""Developer tool: SHA-256 digests of every output array of slhip_pose_pnp and slhip_pose_align on seeded inputs -- the "same
bytes" evidence of a refactor of the RANSAC pose family (profiles/r21, r22, r23).  One line per array:
    pose_pnp[K,variant].output (shape) sha256
  K         3 (align only), 4, 5, 63, 64, 65, 257, 1024, 4096: the 16-byte tail of the score walk, one wave and one past it, one
            past the 256 stride, the raised-LDS path
  sets      five per call: clean, 20 % and 40 % of the rows replaced, one with too few valid rows (insufficient) and one of
            unrelated rows (no model; min_inliers is max(the module's least, K / 8), which chance does not reach)
  variant   plain (64 hypotheses, 4 refinement steps), init (the same with initial poses), refit (a pure refinement, 0 hypotheses),
            deep (4096 hypotheses, 16 refinement steps); for PnP each also with per-set intrinsics (a `k` behind the name)
The inputs come from the fixed seed below, so the lines can be made again by any later tree.
    python tools/pose_digests.py host                     the host twins of the library in use (SLHIP_LIB, or this tree's); no device
    python tools/pose_digests.py device                   the kernels, through solve() on cuda:0
    python tools/pose_digests.py host|device [--out DIR] NAME=LIB [NAME=LIB ...]
                                                          one child process per library (SLHIP_LIB=LIB), its lines written to
                                                          DIR/pose_digests_<mode>_<NAME>.txt; says whether all files are equal and
                                                          exits with 1 when they are not"""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

SEED = 20261023
KS = (3, 4, 5, 63, 64, 65, 257, 1024, 4096)
K4 = (572.4, 572.4, 320.0, 240.0)
F = np.float32
VARIANTS = (("plain", dict(n_hypotheses=64, refine_iters=4), False), ("init", dict(n_hypotheses=64, refine_iters=4), True),
            ("refit", dict(n_hypotheses=0, refine_iters=4), True), ("deep", dict(n_hypotheses=4096, refine_iters=16), False))
OUTPUTS = ("pose", "n_inliers", "rms", "inliers", "best", "flags")
M = 5      # clean, 20 %, 40 %, insufficient, no model


def motions(rng, n):
    """float64 [n, 3, 4]: random rotations, the object 0.5 to 1.5 m in front of the camera"""
    q = rng.standard_normal((n, 4))
    x, y, z, w = (q / np.linalg.norm(q, axis=-1, keepdims=True)).T
    T = np.zeros((n, 3, 4))
    T[:, :, :3] = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                            2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(n, 3, 3)
    T[:, 2, 3] = 0.5 + rng.random(n)
    T[:, :2, 3] = (rng.random((n, 2)) - 0.5) * 0.3 * T[:, 2:3, 3]
    return T


def case(K, min_valid):
    """The inputs of both modules at K rows: object points P [M, K, 4], camera points X [M, K, 4], per-set intrinsics k4 [M, 4],
    pixels under K4 and under k4, and initial poses near the true ones."""
    rng = np.random.default_rng([SEED, K])
    T = motions(rng, M)
    P = (rng.random((M, K, 3)) - 0.5) * 0.1
    X = P @ T[:, :, :3].transpose(0, 2, 1) + T[:, None, :, 3]
    k4 = np.asarray(K4) * (1.0 + 0.05 * (rng.random((M, 4)) - 0.5))

    def pixels(k):
        k = np.broadcast_to(np.asarray(k, np.float64), (M, 4))[:, None]
        uv = np.stack([k[..., 0] * X[..., 0] / X[..., 2] + k[..., 2], k[..., 1] * X[..., 1] / X[..., 2] + k[..., 3]], -1)
        return uv + 0.3 * np.random.default_rng([SEED, K, 1]).standard_normal(uv.shape)

    uv, uv_k = pixels(K4), pixels(k4)
    X = X + 2e-4 * rng.standard_normal(X.shape)
    junk = (rng.random((M, K, 3)) - 0.5) * 0.1
    swap = rng.random((M, K)) < np.array([0.0, 0.2, 0.4, 0.0, 1.0])[:, None]      # the last set keeps no row of its own
    P = np.where(swap[..., None], junk, P)
    w = np.ones((M, K, 1))
    w[3, min_valid - 1:] = 0.0                                                    # one row short of a model
    init = T.copy()
    init[:, :, 3] += 2e-4 * rng.standard_normal((M, 3))
    c = lambda a: np.ascontiguousarray(a, F)      # noqa: E731
    return dict(src=c(np.concatenate([P, w], -1)), dst=c(np.concatenate([X, np.ones_like(w)], -1)), uv=c(uv), uv_k=c(uv_k), k4=c(k4),
                init=c(init))


def calls(mode):
    """(name, the module's result) of every case, solved as the generator advances"""
    from stillleben_amd import pose_align as pa
    from stillleben_amd import pose_pnp as pnp
    if mode == "device":
        import torch

        import stillleben_amd as sl
        sl.init_cuda(0)
        put = lambda a: None if a is None else torch.from_numpy(a).to("cuda:0")      # noqa: E731
    else:
        put = lambda a: a      # noqa: E731
    for K in KS:
        for module, min_valid in (("pose_pnp", 4), ("pose_align", 3)):
            if K < min_valid:
                continue
            c = case(K, min_valid)
            few = max(min_valid, K // 8)      # min_inliers: more than unrelated rows reach by chance, fewer than a damaged set keeps
            for variant, kw, with_init in VARIANTS:
                init = put(c["init"]) if with_init else None
                common = dict(init=init, min_inliers=few, seed=7, **kw)
                if module == "pose_align":
                    solve = pa.solve if mode == "device" else pa.solve_host
                    yield "pose_align[%d,%s]" % (K, variant), solve(put(c["src"]), put(c["dst"]), threshold=1e-3, **common)
                    continue
                solve = pnp.solve if mode == "device" else pnp.solve_host
                yield "pose_pnp[%d,%s]" % (K, variant), solve(put(c["uv"]), put(c["src"]), intrinsics=K4, **common)
                yield "pose_pnp[%d,%sk]" % (K, variant), solve(put(c["uv_k"]), put(c["src"]), intrinsics=K4, per_set_intrinsics=put(c["k4"]),
                                                                **common)


def digests(mode):
    for name, res in calls(mode):
        for out in OUTPUTS:
            a = getattr(res, out)
            a = a if isinstance(a, np.ndarray) else a.cpu().numpy()
            print("%s.%s %s %s" % (name, out, tuple(a.shape), hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()), flush=True)


def main(argv):
    if not argv or argv[0] not in ("host", "device"):
        sys.exit(__doc__)
    mode, args, out_dir = argv[0], argv[1:], "."
    if args[:1] == ["--out"]:
        out_dir, args = args[1], args[2:]
    if not args:
        return digests(mode)
    os.makedirs(out_dir, exist_ok=True)
    texts = []
    for arg in args:      # a fresh child per library: a process keeps the library it loaded first
        name, lib = arg.split("=", 1)
        env = dict(os.environ, SLHIP_LIB=os.path.abspath(lib))
        text = subprocess.run([sys.executable, os.path.abspath(__file__), mode], env=env, check=True, stdout=subprocess.PIPE).stdout
        with open(os.path.join(out_dir, "pose_digests_%s_%s.txt" % (mode, name)), "wb") as f:
            f.write(text)
        texts.append(text)
    same = all(t == texts[0] for t in texts)
    print("%s: %d libraries, %d lines each: %s" % (mode, len(texts), texts[0].count(b"\n"), "the same bytes" if same else "DIFFERENT"))
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main(sys.argv[1:])
