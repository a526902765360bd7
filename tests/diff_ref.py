"""NumPy restatement of sl.diff (rows D1..D4 and D6), written from the semantics of the reference's CPU loops
(python/src/bridge_diff.cpp) and torch chain (python/stillleben/diff.py), whole-array operations only:

  sobel_valid, dilate, image_gradients   exact (the gradients are float32 elementwise, one rounded operation per NumPy call)
  pose_backward                          float64 from the float32 inputs and the float32 image gradients; also returns A, the sum
                                         of the absolute per-pixel contributions to each output (the scale of the summation error)
  vertex_backward                        float32 in the operation order csrc/slhip_diff.hip documents for D6: bit-exact

and `synth_gbuffer` / `synth_case`, adversarial G-buffers from fixed seeds: ragged instance maps, tied depths, coordinates that
differ at every pixel, so that "which neighbour", "< or <=" and "whose pixel" all show in the results."""
import itertools
from types import SimpleNamespace

import numpy as np

F = np.float32

# (H, W, n_obj, cell): the sizes at which a 256-thread block per 256 pixels can go wrong
SHAPES = [
    (1, 1, 1, 1), (2, 9, 2, 2), (3, 3, 2, 1),    # no interior, or a single interior pixel
    (5, 7, 3, 2),                                # smallest real case
    (16, 17, 4, 3),                              # 272 pixels: a last block of 16
    (17, 31, 5, 4), (37, 53, 7, 5),              # ragged both ways
    (9, 257, 6, 4), (257, 3, 3, 2),              # a row longer than a block, a column image
    (33, 40, 256, 2),                            # the LDS accumulators at their full extent
]

NEIGHBOURS = [(x, y) for x in (-1, 0, 1) for y in (-1, 0, 1)]      # the scan order of the reference's 3x3 loops


def _nb(a, x, y):
    """the (x, y) neighbour of every interior pixel: a[h + x, w + y] for h in 1..H-2, w in 1..W-2"""
    H, W = a.shape[:2]
    return a[1 + x:H - 1 + x, 1 + y:W - 1 + y]


def _occluded(inst, depth, closer):
    """interior pixels of an object with a 3x3 neighbour of another object for which closer(neighbour depth, own depth)"""
    cur, cd = _nb(inst, 0, 0), _nb(depth, 0, 0)
    occ = np.zeros(cur.shape, bool)
    for x, y in NEIGHBOURS:
        o = _nb(inst, x, y)
        occ |= (o != cur) & (o != 0) & closer(_nb(depth, x, y), cd)
    return occ & (cur != 0)


def sobel_valid(inst, depth):
    """D1: bool[H,W], unset where a 3x3 neighbour belongs to another object and is strictly closer; the border stays set."""
    inst, depth = np.asarray(inst), np.asarray(depth, F)
    H, W = inst.shape
    valid = np.ones((H, W), bool)
    if H >= 3 and W >= 3:
        valid[1:-1, 1:-1] = ~_occluded(inst, depth, np.less)
    return valid


def dilate(mask, valid, coords3):
    """D2: (bool[H,W], float32[H,W,3]).  An interior pixel outside the mask joins it when its 3x3 holds a mask pixel and no
    invalid pixel; it takes the coordinates of the LAST mask pixel of the 3x3 in row-major scan order.  Border: zero."""
    mask, valid, coords3 = np.asarray(mask, bool), np.asarray(valid, bool), np.asarray(coords3, F)
    H, W = mask.shape
    out_mask, out_c = np.zeros((H, W), bool), np.zeros((H, W, 3), F)
    if H < 3 or W < 3:
        return out_mask, out_c
    own = _nb(mask, 0, 0)
    any_obj, all_valid = np.zeros(own.shape, bool), np.ones(own.shape, bool)
    last = np.zeros(own.shape + (3,), F)
    for x, y in NEIGHBOURS:
        m = _nb(mask, x, y)
        any_obj |= m
        all_valid &= _nb(valid, x, y)
        last = np.where(m[..., None], _nb(coords3, x, y), last)
    grown = ~own & any_obj & all_valid
    out_mask[1:-1, 1:-1] = own | grown
    out_c[1:-1, 1:-1] = np.where(grown[..., None], last, _nb(coords3, 0, 0))
    return out_mask, out_c


def image_gradients(rgb, valid):
    """D3: (grad_x, grad_y) float32[3,H,W] = -((right - left) * (W / 4)), -((down - up) * (H / 4)) of float32(byte) / 255 with
    zero padding, zero where !valid."""
    rgb, valid = np.asarray(rgb, np.uint8), np.asarray(valid, bool)
    H, W = valid.shape
    f = np.zeros((3, H + 2, W + 2), F)
    f[:, 1:-1, 1:-1] = np.moveaxis(rgb[:, :, :3].astype(F) / F(255.0), 2, 0)
    sx, sy = F(W) / F(4.0), F(H) / F(4.0)
    gx = -((f[:, 1:-1, 2:] - f[:, 1:-1, :-2]) * sx)
    gy = -((f[:, 2:, 1:-1] - f[:, :-2, 1:-1]) * sy)
    return np.where(valid, gx, F(0.0)), np.where(valid, gy, F(0.0))


def pose_backward(rgb, coord, inst, grad, P, poses, obj_inst):
    """D4: (out float64[n,6], A float64[n,6]).  Per object: dilate its mask, and over the dilated pixels sum
    grad_in[1x3] . g_xy[3x2] . d proj / d world [2x3] . d world / d (alpha, beta, gamma, a, b, c) [3x6]."""
    coord, inst = np.asarray(coord, F), np.asarray(inst)
    P = np.asarray(P, F).reshape(4, 4).astype(np.float64)
    poses = np.asarray(poses, F).reshape(-1, 4, 4).astype(np.float64)
    H, W = inst.shape
    valid = sobel_valid(inst, coord[:, :, 3])
    gx, gy = image_gradients(rgb, valid)
    gi = np.asarray(grad, F).astype(np.float64)
    s = np.zeros((2, H, W))
    for c in range(3):
        s[0] += gi[c] * gx[c].astype(np.float64)
        s[1] += gi[c] * gy[c].astype(np.float64)
    out, A = np.zeros((len(poses), 6)), np.zeros((len(poses), 6))
    for o, (T, idx) in enumerate(zip(poses, obj_inst)):
        dm, dc = dilate(inst == np.int16(idx), valid, coord[:, :, :3])
        if not dm.any():
            continue
        X = dc[dm].astype(np.float64).T                                   # [3, n]
        X = np.concatenate([X, np.ones((1, X.shape[1]))])
        y = T[:, 0, None] * X[0] + T[:, 1, None] * X[1] + T[:, 2, None] * X[2] + T[:, 3, None] * X[3]
        Py = P[:3, 0, None] * y[0] + P[:3, 1, None] * y[1] + P[:3, 2, None] * y[2] + P[:3, 3, None] * y[3]
        inv, ninv2 = 1.0 / Py[2], -1.0 / (Py[2] * Py[2])
        s0, s1 = s[0][dm], s[1][dm]
        r3 = [s0 * (P[0, i] * inv + (P[2, i] * ninv2) * Py[0]) + s1 * (P[1, i] * inv + (P[2, i] * ninv2) * Py[1]) for i in range(3)]
        z, one = np.zeros_like(X[0]), X[3]
        GX = [(z, -X[2], X[1], z), (X[2], z, -X[0], z), (-X[1], X[0], z, z), (one, z, z, z), (z, one, z, z), (z, z, one, z)]
        for k in range(6):
            g = np.zeros_like(s0)
            for i in range(3):
                g = g + r3[i] * (T[i, 0] * GX[k][0] + T[i, 1] * GX[k][1] + T[i, 2] * GX[k][2] + T[i, 3] * GX[k][3])
            out[o, k], A[o, k] = g.sum(), np.abs(g).sum()
    return out, A


def pose_bound(ref, A):
    """|hip - ref| <= 2^-23 |ref| + 1e-9 A: the final cast to float32 (2^-24 |ref|, doubled) and the order of a float64 sum whose
    terms add up to A in magnitude."""
    return 2.0 ** -23 * np.abs(ref) + 1e-9 * A


def vertex_backward(rgb, coord, inst, bary, grad, P, poses, obj_inst):
    """D6 dense form: (grad_vertices, grad_colors) float32[H,W,3,3], -bary_k * dL/dX and -bary_k * dL/dI at the pixels of the
    objects, zero elsewhere; float32, every product and sum rounded once, in the kernel's order."""
    coord, inst, bary = np.asarray(coord, F), np.asarray(inst), np.asarray(bary, F)
    P, poses = np.asarray(P, F).reshape(4, 4), np.asarray(poses, F).reshape(-1, 4, 4)
    H, W = inst.shape
    valid = sobel_valid(inst, coord[:, :, 3])
    gx, gy = image_gradients(rgb, valid)
    gl = np.asarray(grad, F)
    obj = np.full((H, W), -1, np.int64)
    for k in reversed(range(len(poses))):                                  # the first object of an id wins
        obj[inst == np.int16(obj_inst[k])] = k
    # M = proj * pose per object, rows 0..2
    Mo = np.zeros((max(len(poses), 1), 3, 4), F)
    for k, T in enumerate(poses):
        for r in range(3):
            Mo[k, r] = ((P[r, 0] * T[0] + P[r, 1] * T[1]) + P[r, 2] * T[2]) + P[r, 3] * T[3]
    M = Mo[np.maximum(obj, 0)]                                             # [H, W, 3, 4]
    X = coord[:, :, :3]
    PX = [((M[:, :, r, 0] * X[:, :, 0] + M[:, :, r, 1] * X[:, :, 1]) + M[:, :, r, 2] * X[:, :, 2]) + M[:, :, r, 3] * F(1.0) for r in range(3)]
    with np.errstate(all="ignore"):                                        # pixels of no object are discarded below
        den = PX[2] * PX[2]
        g3 = []
        for j in range(3):
            gxw = (PX[2] * M[:, :, 0, j] - PX[0] * M[:, :, 2, j]) / den
            gyw = (PX[2] * M[:, :, 1, j] - PX[1] * M[:, :, 2, j]) / den
            a = np.zeros((H, W), F)
            for c in range(3):
                a = a + gl[c] * (gx[c] * gxw + gy[c] * gyw)
            g3.append(a)
        gv, gc = np.zeros((H, W, 3, 3), F), np.zeros((H, W, 3, 3), F)
        for k in range(3):
            for j in range(3):
                gv[:, :, k, j] = -(bary[:, :, k] * g3[j])
                gc[:, :, k, j] = -(bary[:, :, k] * gl[j])
    none = obj < 0
    gv[none], gc[none] = F(0.0), F(0.0)
    return gv, gc


# ---- synthetic G-buffers ----------------------------------------------------------------------------
def _random_rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def synth_gbuffer(rng, H, W, n_obj, cell):
    """One G-buffer with everything sl.diff reads.  Instance ids 0 (background) .. n_obj in cells of cell x cell pixels at a random
    offset, about 5 % of the pixels flipped to a random id; where the interior has the room, every id owns an interior pixel.
    Depth in steps of 1/8 so that it ties across instance edges.  The objects are listed in a shuffled order."""
    g = SimpleNamespace(H=H, W=W, n_obj=n_obj, cell=cell)
    oy, ox = rng.integers(0, cell, 2)
    cells = rng.integers(0, n_obj + 1, ((H + cell) // cell + 1, (W + cell) // cell + 1))
    hh, ww = np.mgrid[0:H, 0:W]
    inst = cells[(hh + oy) // cell, (ww + ox) // cell]
    flip = rng.random((H, W)) < 0.05
    inst = np.where(flip, rng.integers(0, n_obj + 1, (H, W)), inst)
    n_int = max(H - 2, 0) * max(W - 2, 0)
    if n_int >= 2 * n_obj:
        at = rng.permutation(n_int)[:n_obj]
        inst[1 + at // (W - 2), 1 + at % (W - 2)] = np.arange(1, n_obj + 1)
    g.inst = inst.astype(np.int16)
    g.obj_inst = rng.permutation(np.arange(1, n_obj + 1)).astype(np.int32)
    depth = 1.0 + rng.choice([-1] + [0] * 10 + [1], (H, W)) / 8.0
    g.coord = np.concatenate([rng.uniform(-0.1, 0.1, (H, W, 3)), depth[..., None]], axis=2).astype(F)
    g.rgb = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    g.grad = rng.standard_normal((3, H, W)).astype(F)
    g.bary = rng.dirichlet([1.0, 1.0, 1.0], (H, W)).astype(F)
    g.vidx = rng.integers(1, 1000, (H, W, 4)).astype(np.int32)
    poses = np.tile(np.eye(4), (n_obj, 1, 1))
    for T in poses:
        T[:3, :3] = _random_rotation(rng)
        T[:3, 3] = [rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(0.8, 1.5)]
    g.poses = poses.astype(F)
    fx, fy = rng.uniform(1.5, 2.5, 2)
    g.P = np.array([[fx, 0.02, rng.uniform(-0.1, 0.1), 0.01], [-0.03, fy, rng.uniform(-0.1, 0.1), -0.02],
                    [0.01, -0.02, 1.0, 0.05], [0.0, 0.0, 1.0, 0.0]], F)
    return g


def hard_enough(g):
    """None when the case holds every stencil edge case, else what it lacks (cases with H, W >= 5)."""
    depth = g.coord[:, :, 3]
    valid = sobel_valid(g.inst, depth)
    bad = 1.0 - valid.mean()
    if not 0.05 <= bad <= 0.70:
        return "%.0f %% invalid pixels" % (100 * bad)
    seen = np.unique(g.inst[1:-1, 1:-1][valid[1:-1, 1:-1]])
    if np.count_nonzero(seen) < 0.85 * g.n_obj:
        return "only %d of %d objects own a valid interior pixel" % (np.count_nonzero(seen), g.n_obj)
    claims = np.zeros((g.H, g.W), int)
    grown_any = several = False
    for idx in range(1, g.n_obj + 1):
        mask = g.inst == idx
        dm, _ = dilate(mask, valid, g.coord[:, :, :3])
        grown = dm & ~mask
        grown_any |= bool(grown.any())
        claims += grown & (g.inst == 0)
        n_in = sum(_nb(mask, x, y).astype(int) for x, y in NEIGHBOURS)
        several |= bool((grown[1:-1, 1:-1] & (n_in >= 2)).any())
    if not grown_any:
        return "no dilated pixel"
    if not (claims >= 2).any():
        return "no background pixel claimed by two objects"
    if not several:
        return "no dilated pixel with two pixels of the object in its 3x3"
    # an edge between two objects with the same depth on both sides that only `<` keeps valid
    if not (_occluded(g.inst, depth, np.less_equal) & ~_occluded(g.inst, depth, np.less)).any():
        return "no instance edge with equal depths"
    return None


def synth_case(H, W, n_obj, cell, seed=0):
    """synth_gbuffer from the first seed >= `seed` whose case is hard enough (always the same one: nothing here is random)."""
    for s in itertools.count(seed):
        g = synth_gbuffer(np.random.default_rng([s, H, W, n_obj]), H, W, n_obj, cell)
        g.seed = s
        why = hard_enough(g) if min(H, W) >= 5 else None
        if why is None:
            return g
        assert s < seed + 200, "no hard case at %dx%d with %d objects: %s" % (H, W, n_obj, why)
