"""Float64 definition of the geometric G-buffer -- instance, class, vertex ids, barycentrics, object coordinates + depth, camera
coordinates, normals -- by casting one ray per pixel centre against every triangle, plus the small scenes it is held against.
Written from DESIGN.md, include/slhip.h and the public classes (Scene, Object, Mesh); it imports nothing of stillleben_amd/csrc or
oracle/, builds no render records and shares no code with either.  tests/test_oracle_raster_known.py holds the CPU oracle to it,
tests/test_gpu_raster_known.py the kernels.  What it reads of a scene: positions, normals, indices, Mesh.pretransform,
Object.pose(), Scene.camera_pose(), Scene.projection_matrix(), Scene.viewport, instance and class indices -- the record
builders and the float32 matrix chains are part of what is being checked.

Conventions (and where they come from)
  camera    x right, y DOWN, z forward.  projection_matrix() P gives fx = P00 W / 2, fy = P11 H / 2, cx = (P02 + 1) W / 2,
            cy = (P12 + 1) H / 2; near 0.1, far 10 (Scene.set_camera_intrinsics).  Pixel (column i, row j) is sampled at
            (u, v) = (i + 0.5, j + 0.5); its ray is ((u - cx) / fx, (v - cy) / fy, 1), so the ray parameter IS the camera z.
  vertices  object = pretransform . position, camera = inverse(camera_pose) . pose . object, in float64 from the float32 inputs.
  hit       the nearest intersection with camera z in [near, far] over all triangles of all objects; no culling.  Of two
            triangles with the SAME camera-space vertices in the same order (coincident objects of one mesh) the one drawn first
            is the hit and the other is no competitor: the depth test is LESS and the earlier draw wins the tie (rule R6).
  channels  instance / cls: the object's and the mesh's indices.  vertex_idx: the triangle's indices + 1 in index-buffer order,
            w = 0.  bary: the 3D barycentrics of the hit in the ORIGINAL triangle (also when the near plane cuts it), w = 0.
            coord: xyz the barycentric combination of the object-frame vertices, w the camera z.  cam_coord: the hit, w = 1.
            Background: 0 everywhere but coord and cam_coord, which are 3000.
  normals   n_i = normalize(N . vertex normal i) with N the inverse transpose of the 3x3 of pose . pretransform (a pretransform
            is a rotation and a uniform scale, a pose is rigid: N is the rotation over the scale, and the scale drops out);
            n = sum b_i n_i, NOT renormalised, negated on a back face; xyz = normalize(R_world->camera n),
            w = n . normalize(camera position - world hit).  A face is a BACK face when the geometric normal of its index-order
            winding, (v1 - v0) x (v2 - v0) in the camera frame, points away from the camera (its dot with the hit is positive).
            In window coordinates (x, row) such a triangle has positive signed area: counter-clockwise with the row axis up, as
            OpenGL's window has it -- front is FrontFace = CW.  _facing_of_a_hand_made_triangle (scene 5a) pins this by hand.
  peel      second layer: given the first layer's coord.w (the picture under test), the nearest hit with camera z > w + 1e-5.
            The first layer's own fragment recomputes the same bits and is rejected whatever its float64 z: its triangle is no
            candidate.  A pixel whose nearest remaining hit lies within PEEL_MARGIN plus that hit's own snapping envelope of the
            threshold is left out (the envelope is what the hit's float32 z may differ by from the one computed here, up to
            1e-4 m in these scenes: without it the margin of 2e-5 alone would not cover the comparison it is there for).

What is left out of the value comparison (decided here, never from the picture under test)
  (a) pixels whose centre is within EDGE_MARGIN = 1/128 px of a projected edge segment of ANY triangle, hidden or not (rule R3
      moves a vertex by at most 1/512 px per axis, an edge by less than 0.003 px; 1/128 is 2.8 times that);
  (b) pixels whose two nearest hits are closer in camera z than four steps of the 24-bit window depth, dz = z^2 (f - n) / (f n)
      2^-24 each, plus both hits' snapping envelopes;
  (c) pixels within 1/128 px of the line in which a triangle crosses the near or the far plane (the projected edges of a triangle
      that crosses the near plane are those of the part in front of it, the crossing line among them).
There the picture must show the nearest or second-nearest hit's instance, an object with an edge within the margin, or background.

Bound on the kept pixels, per component: |out - ref| <= E_snap + 16 2^-23 M.  E_snap is the change of the component when the same
triangle's plane is evaluated at (u + 1/256, v) and at (u, v + 1/256), the two absolute changes added (a vertex moves by at most half
a snap step per axis).  M is the largest magnitude of the attribute among the triangle's three vertices (1 for barycentrics and
normals).  16 stands for the float32 chain of rule R5: two conversions, three products, a sum, a division and two fused
multiply-adds on differences."""
import math

import numpy as np

NEAR, FAR = 0.1, 10.0
BACKGROUND = 3000.0
SNAP = 1.0 / 256.0                 # rule R3: window coordinates are snapped to 1/256 px
EDGE_MARGIN = 1.0 / 128.0          # (a), (c): 2.8 x the largest move of an edge under R3
DEPTH_STEPS = 4.0                  # (b): steps of the 24-bit window depth
PEEL_EPS, PEEL_MARGIN = 1e-5, 2e-5
F32_OPS, F32_EPS = 16.0, 2.0 ** -23
LEFT_OUT_CAP, SLIVER_CAP, MIN_COVERED = 0.05, 0.15, 0.03
FLOAT_CHANNELS = ("coord", "cam_coord", "bary", "normals")
INT_CHANNELS = ("instance", "cls", "vertex_idx")


# ---- the triangles of a scene, in draw order --------------------------------------------------------------------------------------
class Soup:
    """cam, obj [T, 3, 3] camera- and object-frame vertices, nrm [T, 3, 3] unit world normals (None: no normals channel),
    vid [T, 3] vertex ids, inst, cls [T]; fx, fy, cx, cy, W, H; cam_to_world 4x4 (None: no normals channel)."""


def intrinsics(P, W, H):
    P = np.asarray(P, np.float64)
    return P[0, 0] * W / 2.0, P[1, 1] * H / 2.0, (P[0, 2] + 1.0) * W / 2.0, (P[1, 2] + 1.0) * H / 2.0


def _np64(t):
    return (t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)).astype(np.float64)


def soup_from_parts(parts, intr, size, cam_to_world=None):
    """parts: (mesh, mesh-object-frame -> camera 4x4, instance index, object -> world 4x4 or None) per object, in draw order."""
    s = Soup()
    s.W, s.H = int(size[0]), int(size[1])
    s.fx, s.fy, s.cx, s.cy = (float(x) for x in intr)
    s.cam_to_world = None if cam_to_world is None else np.asarray(cam_to_world, np.float64)
    cam, obj, nrm, vid, inst, cls = [], [], [], [], [], []
    for mesh, o2c, instance, o2w in parts:
        m2o = _np64(mesh.pretransform)
        pos, idx = _np64(mesh.points), _np64(mesh.faces).astype(np.int64).reshape(-1, 3)
        po = pos @ m2o[:3, :3].T + m2o[:3, 3]
        o2c = np.asarray(o2c, np.float64)
        pc = po @ o2c[:3, :3].T + o2c[:3, 3]
        cam.append(pc[idx])
        obj.append(po[idx])
        if o2w is not None:
            N = np.linalg.inv((np.asarray(o2w, np.float64) @ m2o)[:3, :3]).T
            nw = _np64(mesh.normals) @ N.T
            nw /= np.linalg.norm(nw, axis=1, keepdims=True)
            nrm.append(nw[idx])
        vid.append(idx + 1)
        inst.append(np.full(len(idx), int(instance), np.int64))
        cls.append(np.full(len(idx), int(mesh.class_index), np.int64))
    s.cam = np.concatenate(cam) if cam else np.zeros((0, 3, 3))
    s.obj = np.concatenate(obj) if obj else np.zeros((0, 3, 3))
    s.nrm = np.concatenate(nrm) if nrm and s.cam_to_world is not None else None
    s.vid = np.concatenate(vid) if vid else np.zeros((0, 3), np.int64)
    s.inst = np.concatenate(inst) if inst else np.zeros(0, np.int64)
    s.cls = np.concatenate(cls) if cls else np.zeros(0, np.int64)
    return s


def soup_from_scene(scene):
    W, H = scene.viewport
    c2w = _np64(scene.camera_pose())
    w2c = np.linalg.inv(c2w)
    parts = []
    for o in scene.objects:
        o2w = _np64(o.pose())
        parts.append((o.mesh, w2c @ o2w, o.instance_index, o2w))
    return soup_from_parts(parts, intrinsics(_np64(scene.projection_matrix()), W, H), (W, H), c2w)


# ---- geometry ---------------------------------------------------------------------------------------------------------------------
def _clip(poly, sign, plane):
    """Sutherland-Hodgman of a camera-space polygon against sign * (z - plane) >= 0."""
    out = []
    n = len(poly)
    for i in range(n):
        a, b = poly[i], poly[(i + 1) % n]
        da, db = sign * (a[2] - plane), sign * (b[2] - plane)
        if da >= 0:
            out.append(a)
        if (da >= 0) != (db >= 0):
            t = da / (da - db)
            out.append(a + t * (b - a))
    return out


def _window(lo, hi, n):
    a = max(0, int(math.floor(lo - 1.5)))
    b = min(n, int(math.ceil(hi + 1.5)))
    return a, b


def _segment_distance(U, V, p, q):
    d = q - p
    L2 = float(d @ d)
    if L2 == 0.0:
        return np.hypot(U - p[0], V - p[1])
    t = np.clip(((U - p[0]) * d[0] + (V - p[1]) * d[1]) / L2, 0.0, 1.0)
    return np.hypot(U - (p[0] + t * d[0]), V - (p[1] + t * d[1]))


def _project(s, poly):
    p = np.asarray(poly)
    return np.stack([s.fx * p[:, 0] / p[:, 2] + s.cx, s.fy * p[:, 1] / p[:, 2] + s.cy], 1)


def _planes(s, tri, rx, ry, affine=False):
    """Everything the plane of triangle tri[k] gives ray k, also outside the triangle's edges: dict of [P, 4] channels.  `affine`:
    the WRONG interpolation -- screen-space barycentrics applied to the attributes -- which a scene that tells the two apart must
    fail (test_steep_perspective_tells_affine_apart)."""
    A, B, C = s.cam[tri, 0], s.cam[tri, 1], s.cam[tri, 2]
    e1, e2 = B - A, C - A
    g = np.cross(e1, e2)
    d = np.stack([rx, ry, np.ones_like(rx)], -1)
    with np.errstate(all="ignore"):
        z = (A * g).sum(-1) / (d * g).sum(-1)
        hit = z[:, None] * d
        r = hit - A
        gg = (g * g).sum(-1)
        b1 = (np.cross(r, e2) * g).sum(-1) / gg
        b2 = (np.cross(e1, r) * g).sum(-1) / gg
        b = np.stack([1.0 - b1 - b2, b1, b2], -1)
        if affine:
            pa, pb, pc = (np.stack([s.fx * X[:, 0] / X[:, 2], s.fy * X[:, 1] / X[:, 2]], 1) for X in (A, B, C))
            q = np.stack([s.fx * rx, s.fy * ry], 1)
            den = (pb[:, 0] - pa[:, 0]) * (pc[:, 1] - pa[:, 1]) - (pb[:, 1] - pa[:, 1]) * (pc[:, 0] - pa[:, 0])
            l1 = ((q[:, 0] - pa[:, 0]) * (pc[:, 1] - pa[:, 1]) - (q[:, 1] - pa[:, 1]) * (pc[:, 0] - pa[:, 0])) / den
            l2 = ((pb[:, 0] - pa[:, 0]) * (q[:, 1] - pa[:, 1]) - (pb[:, 1] - pa[:, 1]) * (q[:, 0] - pa[:, 0])) / den
            b = np.stack([1.0 - l1 - l2, l1, l2], -1)
            hit = np.einsum("pk,pkc->pc", b, s.cam[tri])
            z = hit[:, 2]
        zero, one = np.zeros_like(z), np.ones_like(z)
        out = {"bary": np.concatenate([b, zero[:, None]], 1),
               "coord": np.concatenate([np.einsum("pk,pkc->pc", b, s.obj[tri]), z[:, None]], 1),
               "cam_coord": np.concatenate([hit, one[:, None]], 1)}
        if s.nrm is not None:
            n = np.einsum("pk,pkc->pc", b, s.nrm[tri])
            back = (g * hit).sum(-1) > 0.0
            n = np.where(back[:, None], -n, n)
            R, t = s.cam_to_world[:3, :3], s.cam_to_world[:3, 3]
            nc = n @ R                                   # R_world->camera = R^T: (R^T n) as a row is n R
            nc = nc / np.linalg.norm(nc, axis=1, keepdims=True)
            view = -(hit @ R.T)                          # camera position - world hit = -(R hit)
            view = view / np.linalg.norm(view, axis=1, keepdims=True)
            out["normals"] = np.concatenate([nc, (n * view).sum(-1)[:, None]], 1)
    return out


class Reference:
    """Per pixel [H, W]: tri (-1: background), covered, keep, the INT_CHANNELS and FLOAT_CHANNELS, tol[channel] [H, W, 4] the bound,
    inst2 the second-nearest hit's instance, edge_near[instance] / any_hit[instance] bool maps, edge_distance."""


def cast(s, peel=None, affine=False):
    """The reference of one scene.  peel = (first layer's Reference, the picture's first-layer coord.w [H, W]): the second layer."""
    W, H, T = s.W, s.H, len(s.cam)
    U, V = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    RX, RY = (U - s.cx) / s.fx, (V - s.cy) / s.fy
    # the two nearest hits per pixel: depth, envelope, triangle (equal depths stay in draw order)
    zs, ezs = np.full((2, H, W), np.inf), np.zeros((2, H, W))
    ts = np.zeros((2, H, W), np.int64)
    edge = np.full((H, W), np.inf)
    instances = sorted(set(s.inst.tolist()))
    edge_of = {i: np.full((H, W), np.inf) for i in instances}
    any_hit = {i: np.zeros((H, W), bool) for i in instances}
    if peel is not None:
        first, w = peel
        L = np.asarray(w, np.float64) + PEEL_EPS
    seen = set()
    for t in range(T):
        tri = s.cam[t]
        front = _clip([tri[0], tri[1], tri[2]], 1.0, NEAR)
        if len(front) < 3:
            continue
        polys = [front]
        if any(p[2] > FAR for p in front):
            polys.append(_clip(front, -1.0, FAR))         # (c): the far plane's crossing line
        for poly in polys:
            if len(poly) < 3:
                continue
            pp = _project(s, poly)
            for k in range(len(pp)):
                p, q = pp[k], pp[(k + 1) % len(pp)]
                x0, x1 = _window(min(p[0], q[0]), max(p[0], q[0]), W)
                y0, y1 = _window(min(p[1], q[1]), max(p[1], q[1]), H)
                if x0 >= x1 or y0 >= y1:
                    continue
                dist = _segment_distance(U[y0:y1, x0:x1], V[y0:y1, x0:x1], p, q)
                edge[y0:y1, x0:x1] = np.minimum(edge[y0:y1, x0:x1], dist)
                e = edge_of[int(s.inst[t])]
                e[y0:y1, x0:x1] = np.minimum(e[y0:y1, x0:x1], dist)
        pp = _project(s, front)
        x0, x1 = _window(pp[:, 0].min(), pp[:, 0].max(), W)
        y0, y1 = _window(pp[:, 1].min(), pp[:, 1].max(), H)
        if x0 >= x1 or y0 >= y1:
            continue
        A, e1, e2 = tri[0], tri[1] - tri[0], tri[2] - tri[0]
        g = np.cross(e1, e2)
        gg = float(g @ g)
        if gg == 0.0:
            continue
        win = (slice(y0, y1), slice(x0, x1))
        rx, ry = RX[win], RY[win]
        with np.errstate(all="ignore"):
            num = float(A @ g)
            z = num / (rx * g[0] + ry * g[1] + g[2])
            r = np.stack([z * rx - A[0], z * ry - A[1], z - A[2]], -1)
            b1 = (np.cross(r, e2) * g).sum(-1) / gg
            b2 = (np.cross(e1, r) * g).sum(-1) / gg
            inside = (b1 >= 0) & (b2 >= 0) & (b1 + b2 <= 1) & (z >= NEAR) & (z <= FAR)
            ez = np.abs(num / ((rx + SNAP / s.fx) * g[0] + ry * g[1] + g[2]) - z) \
                + np.abs(num / (rx * g[0] + (ry + SNAP / s.fy) * g[1] + g[2]) - z)
        any_hit[int(s.inst[t])][win] |= inside
        key = tri.tobytes()
        if key in seen:                                   # the same triangle drawn again: the earlier one wins the tie (R6)
            continue
        seen.add(key)
        if peel is not None:                              # behind the threshold, or too close to it to say; not the first layer's own
            inside &= (first.tri[win] != t) & (z > L[win] - (PEEL_MARGIN + ez))
        if not inside.any():
            continue
        z = np.where(inside, z, np.inf)
        tt = np.full(z.shape, t, np.int64)
        for k in range(2):
            sw = z < zs[k][win]
            zk, ek, tk = zs[k][win].copy(), ezs[k][win].copy(), ts[k][win].copy()
            zs[k][win], ezs[k][win], ts[k][win] = np.where(sw, z, zk), np.where(sw, ez, ek), np.where(sw, tt, tk)
            z, ez, tt = np.where(sw, zk, z), np.where(sw, ek, ez), np.where(sw, tk, tt)

    (z1, z2), (ez1, ez2), (t1, t2) = zs, ezs, ts
    covered = np.isfinite(z1)
    left_peel = np.zeros((H, W), bool)
    if peel is not None:
        left_peel = (covered & (z1 <= L + PEEL_MARGIN + ez1)) | ~first.keep
    with np.errstate(all="ignore"):
        step = z1 * z1 * (FAR - NEAR) / (FAR * NEAR) * 2.0 ** -24
        left_depth = covered & np.isfinite(z2) & (z2 - z1 < DEPTH_STEPS * step + ez1 + ez2)
    left_edge = edge <= EDGE_MARGIN

    ref = Reference()
    ref.soup, ref.W, ref.H = s, W, H
    ref.covered = covered
    ref.tri = np.where(covered, t1, -1)
    ref.keep = ~(left_edge | left_depth | left_peel)
    ref.left = {"edge": left_edge, "depth": left_depth, "peel": left_peel}
    ref.edge_distance = edge
    ref.edge_near = {i: e <= EDGE_MARGIN for i, e in edge_of.items()}
    ref.any_hit = any_hit
    ref.instance = np.where(covered, s.inst[t1] if T else 0, 0)
    ref.inst2 = np.where(np.isfinite(z2), s.inst[t2] if T else 0, 0)
    ref.cls = np.where(covered, s.cls[t1] if T else 0, 0)
    ref.vertex_idx = np.zeros((H, W, 4), np.int64)
    if T:
        ref.vertex_idx[..., :3] = np.where(covered[..., None], s.vid[t1], 0)
    bg = {"coord": BACKGROUND, "cam_coord": BACKGROUND, "bary": 0.0, "normals": 0.0}
    ref.tol = {}
    names = [c for c in FLOAT_CHANNELS if c != "normals" or s.nrm is not None]
    ref.channels = names
    for c in names:
        setattr(ref, c, np.full((H, W, 4), bg[c]))
        ref.tol[c] = np.zeros((H, W, 4))
    if covered.any():
        tri, rx, ry = t1[covered], RX[covered], RY[covered]
        at = _planes(s, tri, rx, ry, affine)
        dx = _planes(s, tri, rx + SNAP / s.fx, ry, affine)
        dy = _planes(s, tri, rx, ry + SNAP / s.fy, affine)
        m_obj = np.abs(s.obj[tri]).max(axis=(1, 2))
        m_cam = np.abs(s.cam[tri]).max(axis=(1, 2))
        one = np.ones_like(m_obj)
        M = {"coord": np.stack([m_obj, m_obj, m_obj, m_cam], 1), "cam_coord": np.stack([m_cam] * 4, 1),
             "bary": np.stack([one] * 4, 1), "normals": np.stack([one] * 4, 1)}
        for c in names:
            getattr(ref, c)[covered] = at[c]
            ref.tol[c][covered] = np.abs(dx[c] - at[c]) + np.abs(dy[c] - at[c]) + F32_OPS * F32_EPS * M[c]
    return ref


# ---- the comparison both test files share -----------------------------------------------------------------------------------------
def channels_of(r, b=0):
    """{channel: numpy array of scene b} of an oracle RenderResult or of the engine's buffers (integers widened, unsigned)."""
    out = {}
    for c in INT_CHANNELS + FLOAT_CHANNELS:
        a = getattr(r, c, None)
        if a is None:
            continue
        a = a[b]
        a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
        if a.dtype == np.int16:
            a = a.view(np.uint16)
        if a.dtype == np.int32:
            a = a.view(np.uint32)
        out[c] = a.astype(np.int64) if a.dtype.kind in "iu" else a
    for c in ("instance", "cls"):
        if c in out:
            out[c] = out[c].reshape(out[c].shape[:2])
    return out


def compare(ref, out, cap=LEFT_OUT_CAP, min_covered=MIN_COVERED, label="", only=None, extra_left=None):
    """Asserts `out` (channels_of) against the reference and returns the figures: covered and left-out shares, the worst
    error-to-bound ratio per channel.  `only`: compare at these pixels alone (the others count as left out but need not show a
    permitted instance); `extra_left`: further rule-based exclusions, counted against the cap."""
    keep = ref.keep.copy()
    if extra_left is not None:
        keep &= ~extra_left
    region = np.ones_like(keep) if only is None else only
    keep &= region
    cov = ref.covered & region
    n_cov = int(cov.sum())
    n_left = int((region & ~keep).sum())                  # a silhouette's outer margin counts too
    fig = {"covered": n_cov / keep.size, "left_out": n_left / max(1, n_cov), "ratio": {}}
    # integer channels and the background: exact
    for c in INT_CHANNELS:
        if c in out:
            want = getattr(ref, c)
            bad = keep & ((out[c] != want).any(-1) if want.ndim == 3 else (out[c] != want))
            assert not bad.any(), "%s %s: %d kept pixels differ, first (row, col) %s: got %s, want %s" % (
                label, c, bad.sum(), np.argwhere(bad)[0], out[c][tuple(np.argwhere(bad)[0])], want[tuple(np.argwhere(bad)[0])])
    kept_cov, kept_bg = keep & ref.covered, keep & ~ref.covered
    worst = {}
    for c in ref.channels:
        if c not in out:
            continue
        got, want = out[c].astype(np.float64), getattr(ref, c)
        assert np.array_equal(got[kept_bg], want[kept_bg]), "%s %s: background differs" % (label, c)
        with np.errstate(all="ignore"):
            ratio = np.abs(got - want)[kept_cov] / ref.tol[c][kept_cov]
        assert not np.isnan(ratio).any(), "%s %s: NaN" % (label, c)
        for k, name in enumerate(("xyz", "xyz", "xyz", "w")):
            key = c + "." + name
            if ratio.size:
                worst[key] = max(worst.get(key, 0.0), float(ratio[:, k].max()))
    fig["ratio"] = worst
    # left-out pixels: one of the permitted owners
    if "instance" in out:
        left = region & ~keep
        got = out["instance"]
        ok = (got == 0) | (got == ref.instance) | (got == ref.inst2)
        for i, near in ref.edge_near.items():
            ok |= near & (got == i)
        if ref.left["peel"].any():                        # a peeled layer: any object the ray meets
            for i, h in ref.any_hit.items():
                ok |= h & (got == i)
        bad = left & ~ok
        assert not bad.any(), "%s: left-out pixel %s shows instance %d" % (label, np.argwhere(bad)[0], got[tuple(np.argwhere(bad)[0])])
    assert fig["covered"] >= min_covered, "%s: only %.2f %% of the picture is covered" % (label, 100 * fig["covered"])
    assert fig["left_out"] <= cap, "%s: %.2f %% of the covered pixels are left out" % (label, 100 * fig["left_out"])
    return fig


def assert_within(fig, label=""):
    over = {k: v for k, v in fig["ratio"].items() if not v <= 1.0}
    assert not over, "%s: error over the bound (ratio > 1): %s" % (label, over)


def report(label, fig):
    print("%-28s covered %5.1f %%  left out %5.2f %%  worst error / bound: %s" % (
        label, 100 * fig["covered"], 100 * fig["left_out"], "  ".join("%s %.2f" % kv for kv in sorted(fig["ratio"].items()))))


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
def make_mesh(sl, positions, normals, triangles, name):
    from stillleben_amd import _loaders

    cm = _loaders.ConsolidatedMesh()
    cm.positions = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    n = np.asarray(normals, np.float64).reshape(-1, 3)
    cm.normals = np.ascontiguousarray(n / np.linalg.norm(n, axis=1, keepdims=True), np.float32)
    V = len(cm.positions)
    cm.uvs = np.zeros((V, 2), np.float32)
    cm.colors = np.ones((V, 4), np.float32)
    cm.indices = np.ascontiguousarray(triangles, np.uint32).reshape(-1)
    cm.textures = []
    cm._tex_alpha = []
    cm.materials = [_loaders.Material(base_color=(0.8, 0.8, 0.8, 1))]
    cm.submeshes = [_loaders.SubMesh(0, len(cm.indices), 0)]
    return sl.Mesh.from_data(cm, hulls=[], filename="memory://" + name)


def rotation(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = math.radians(deg)
    return np.eye(3) + math.sin(r) * K + (1 - math.cos(r)) * (K @ K)


def pose(R=None, t=(0, 0, 0)):
    import torch

    P = np.eye(4)
    if R is not None:
        P[:3, :3] = R
    P[:3, 3] = t
    return torch.from_numpy(P.astype(np.float32))


def add(sl, scene, mesh, P=None, instance=None):
    o = sl.Object(mesh)
    if P is not None:
        o.set_pose(P)
    if instance is not None:
        o.instance_index = instance
    scene.add_object(o)
    return o


def clutter(sl, seed, size=(160, 120)):
    """1: the oblique heap of cubes."""
    import scenes as S

    return S.clutter_scene(sl, seed, n_objects=6, size=size, plane=False)


def icosphere(subdivisions=2):
    p = (1 + math.sqrt(5)) / 2
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p),
         (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v), np.array(f)


def smooth_scene(sl, size=(150, 100)):
    """2: an icosphere of 2 subdivisions, squeezed to an ellipsoid in the mesh while its vertex normals stay the sphere's radial
    ones (normals that are not positions), in an oblique pose off the optical axis, seen with an off-centre principal point."""
    v, f = icosphere(2)
    mesh = make_mesh(sl, v * np.array([0.11, 0.07, 0.05]), v, f, "ellipsoid")
    mesh.class_index = 7
    scene = sl.Scene(size)
    scene.set_camera_intrinsics(300.0, 310.0, 70.3, 52.6)
    add(sl, scene, mesh, pose(rotation((1, 2, -1), 51.0), (0.03, -0.02, 0.47)), instance=5)
    return scene


QUAD = np.array([(-0.07, -0.03, 0.15), (-0.07, 0.03, 0.15), (2.0, 1.2, 6.0), (2.0, -1.2, 6.0)])
QUAD_NORMALS = np.array([(-1, 0.2, -0.3), (-0.8, -0.5, 0.1), (-0.3, 0.1, -1), (-0.6, 0.6, -0.4)])


def quad_mesh(sl):
    """A planar quad that runs from 0.15 m to 6 m deep across the picture (camera frame = world frame = object frame), two
    triangles, four different vertex normals."""
    return make_mesh(sl, QUAD, QUAD_NORMALS, [(0, 1, 2), (0, 2, 3)], "quad")


def steep_scene(sl, size=(160, 120)):
    """3: screen-space instead of perspective-correct interpolation is off by tens of percent of the attribute's range here."""
    scene = sl.Scene(size)
    add(sl, scene, quad_mesh(sl))
    return scene


def clip_scene(sl, size=(160, 120)):
    """4: the quad pushed through the near plane; a triangle with one and one with two vertices behind the camera (negative
    clip w); one entirely behind it; one beyond the far plane.  Five objects, instances 1..5."""
    scene = sl.Scene(size)
    add(sl, scene, quad_mesh(sl), pose(None, (0.0, 0.0, -0.1)))
    nr = [(0.2, -0.1, -1), (-0.3, 0.2, -1), (0.1, 0.4, -1)]
    tris = [[(-0.3, -0.28, 1.0), (0.3, -0.30, 1.2), (0.05, -0.2, -0.5)],          # one vertex behind: leaves through the top
            [(0.0, 0.3, 1.0), (0.4, 0.2, -0.2), (-0.4, 0.25, -0.3)],             # two behind: a wedge towards the bottom
            [(-0.2, 0.1, -0.5), (0.2, 0.1, -0.6), (0.0, -0.2, -1.0)],            # all behind
            [(-3.0, -2.0, 11.0), (3.0, -2.0, 12.0), (0.0, 2.5, 11.5)]]           # beyond the far plane
    for k, t in enumerate(tris):
        add(sl, scene, make_mesh(sl, t, nr, [(0, 1, 2)], "clip%d" % k))
    return scene


FACING_NORMAL = (0.0, 0.0, -1.0)


def facing_triangles_scene(sl, size=(96, 64)):
    """5a: one triangle twice, side by side, 1 m in front of the camera (camera frame = world frame), vertex normals towards the
    camera.  Instance 1 lists its vertices (left, top) -> (right, top) -> (middle, bottom) in the picture; instance 2 in the
    opposite order."""
    scene = sl.Scene(size)
    t = np.array([(-0.12, -0.1, 1.0), (0.12, -0.1, 1.0), (0.01, 0.13, 1.0)])
    for k, order in enumerate([(0, 1, 2), (0, 2, 1)]):
        m = make_mesh(sl, t + np.array([(-0.15, 0, 0), (0.15, 0.01, 0)][k]), [FACING_NORMAL] * 3, [order], "facing%d" % k)
        add(sl, scene, m)
    return scene


def inside_cube_scene(sl, size=(96, 64)):
    """5b: a closed cube seen from inside, obliquely: every face is a back face."""
    import scenes as S

    scene = sl.Scene(size)
    add(sl, scene, S.mesh(sl, S.CUBE), pose(rotation((1, -2, 0.5), 33.0), (0.1, -0.05, 0.2)))
    return scene


def sliver_scene(sl, size=(160, 120)):
    """6: a fan of 32 slivers about a common vertex that lies off the pixel grid, tilted (instance 1; at 12 px from the hub a sliver
    is 3 px wide, the disc's radius is 45 px), and 16 x 16 separate triangles of about 0.3 px (instance 2), most of which cover no
    pixel centre."""
    scene = sl.Scene(size)
    ang = np.linspace(0, 2 * math.pi, 33)[:-1] + 0.0371
    ring = np.stack([0.31 * np.cos(ang), 0.31 * np.sin(ang), np.zeros(32)], 1)
    pos = np.concatenate([[(0.0, 0.0, 0.0)], ring])
    fan = make_mesh(sl, pos, np.tile([(0.1, -0.2, -1.0)], (33, 1)), [(0, 1 + k, 1 + (k + 1) % 32) for k in range(32)], "fan")
    add(sl, scene, fan, pose(rotation((1, 1, 0), 28.0), (-0.1917, 0.0047, 1.0)))
    px = 1.0 / (size[0] / (2.0 * math.tan(math.radians(58.0) / 2.0)))       # one pixel at 1 m
    gi, gj = np.meshgrid(np.arange(16), np.arange(16))
    org = np.stack([gi.ravel() * 1.13 * px, gj.ravel() * 1.07 * px, np.zeros(256)], 1)
    t0 = np.array([(0.0, 0.0, 0.0), (0.45, 0.05, 0.0), (0.1, 0.4, 0.0)]) * px * 1.8
    tiny = make_mesh(sl, (org[:, None] + t0[None]).reshape(-1, 3), np.tile([(0.0, 0.0, -1.0)], (768, 1)),
                     np.arange(768).reshape(-1, 3), "tiny")
    add(sl, scene, tiny, pose(rotation((0, 0, 1), 9.0), (0.3512, -0.2031, 1.0)))
    return scene


def _small_cube(sl):
    import scenes as S

    m = sl.Mesh(S.CUBE, physics=False)
    m.center_bbox()
    m.scale_to_bbox_diagonal(0.2)
    return m


def interpenetrating_scene(sl, size=(160, 120)):
    """7a: two cubes that intersect; the winner changes along the intersection line."""
    import torch

    scene = sl.Scene(size)
    m = _small_cube(sl)
    add(sl, scene, m, pose(rotation((0.2, 1, 0.4), 20.0), (0.0, 0.0, 0.0)))
    add(sl, scene, m, pose(rotation((1, 0.3, -0.5), 40.0), (-0.05, 0.03, 0.03)))
    scene.set_camera_look_at(torch.tensor([0.33, 0.2, 0.27]), torch.tensor([0.02, 0.015, 0.01]))
    return scene


def coincident_scene(sl, size=(160, 120)):
    """7b: two cubes of one mesh in one pose: the earlier object owns every pixel."""
    import torch

    scene = sl.Scene(size)
    m = _small_cube(sl)
    P = pose(rotation((0.2, 1, 0.4), 20.0), (0.0, 0.0, 0.0))
    add(sl, scene, m, P)
    add(sl, scene, m, P)
    scene.set_camera_look_at(torch.tensor([0.33, 0.2, 0.27]), torch.tensor([0.0, 0.0, 0.0]))
    return scene


def borders_scene(sl, size=(160, 120)):
    """8: a triangle larger than the viewport with all three vertices far outside it (the large-triangle path), oblique, behind
    four cubes each half outside one border of the picture."""
    scene = sl.Scene(size)
    big = make_mesh(sl, [(-9.0, -6.0, 2.0), (10.0, -5.0, 4.5), (0.5, 14.0, 3.0)], [(0.3, 0.1, -1), (-0.2, 0.2, -1), (0.1, -0.3, -1)],
                    [(0, 1, 2)], "big")
    add(sl, scene, big)
    m = _small_cube(sl)
    W, H = size
    fx = W / (2.0 * math.tan(math.radians(58.0) / 2.0))
    z = 0.8
    for k, (x, y) in enumerate([(-W / 2 / fx * z, 0.04), (W / 2 / fx * z, -0.05), (0.06, -H / 2 / fx * z), (-0.07, H / 2 / fx * z)]):
        add(sl, scene, m, pose(rotation((1, k + 1, 2), 25.0 + 20 * k), (x, y, z)))
    return scene


# ---- the scenes by name, and what each is looked at for beyond the comparison -----------------------------------------------------
# scene 8: per size a clutter seed whose picture keeps the caps by the reference alone.  At 1 x 1 the only pixel has to be a covered
# one off every edge, at 7 x 5 (two or three covered pixels) none may be left out: seed 33 is the first that does it at all three
# small sizes
SIZES = {(1, 1): 33, (7, 5): 33, (33, 9): 33, (130, 98): 3}
SCENES = {
    "clutter3": lambda sl: clutter(sl, 3), "clutter21": lambda sl: clutter(sl, 21), "clutter8": lambda sl: clutter(sl, 8),
    "smooth": smooth_scene, "steep": steep_scene, "clip": clip_scene, "facing": facing_triangles_scene,
    "inside_cube": inside_cube_scene, "sliver": sliver_scene, "interpenetrating": interpenetrating_scene,
    "coincident": coincident_scene, "borders": borders_scene,
}
for _size, _seed in SIZES.items():
    SCENES["clutter%d@%dx%d" % ((_seed,) + _size)] = lambda sl, size=_size, seed=_seed: clutter(sl, seed, size)

# scene 10: scenes 1, 2 and 4 at one common size, for one launch
BATCH = ("clutter3@150x100", "smooth", "clip@150x100")
SCENES[BATCH[0]] = lambda sl: clutter(sl, 3, (150, 100))
SCENES[BATCH[2]] = lambda sl: clip_scene(sl, (150, 100))

_cache = {}


def reference(sl, name):
    """(scene, Reference) of a named scene, computed once per session and shared: nothing changes either."""
    if name not in _cache:
        scene = SCENES[name](sl)
        _cache[name] = (scene, cast(soup_from_scene(scene)))
    return _cache[name]


def _near_clip_keeps_the_original_triangle(ref, out):
    """Scene 4: where the near plane cuts a triangle, bary and vertex_idx are still the ORIGINAL triangle's: the cut triangles
    show pixels, their vertex ids are the three of the index buffer in its order, and bary reproduces coord from the original
    object-frame vertices (two float32 interpolations apart: twice the float32 term of the bound).  The triangle behind the
    camera and the one beyond the far plane show nothing."""
    assert set(np.unique(out["instance"]).tolist()) == {0, 1, 2, 3}
    s = ref.soup
    for i in (1, 2, 3):
        m = ref.keep & (ref.instance == i)
        assert m.sum() > 30, (i, m.sum())
        tri = ref.tri[m]
        assert (s.cam[tri][:, :, 2].min(axis=1) < NEAR).all()            # every one of them is cut by the near plane
        assert np.array_equal(out["vertex_idx"][m][:, :3], s.vid[tri])
        recon = np.einsum("pk,pkc->pc", out["bary"][m][:, :3].astype(np.float64), s.obj[tri])
        assert np.abs(recon - out["coord"][m][:, :3]).max() <= 2 * F32_OPS * F32_EPS * np.abs(s.obj[tri]).max()


def _facing_of_a_hand_made_triangle(ref, out):
    """Scene 5a, by hand and without the reference's facing rule: vertices listed (left, top) -> (right, top) -> (middle, bottom)
    in the picture have positive signed area in window coordinates (x, row), i.e. counter-clockwise in OpenGL's window whose y
    axis is the row axis; with FrontFace = CW that is a BACK face, and the vertex normal (0, 0, -1) comes out negated.  The
    opposite order is a front face and keeps it."""
    for i, sign in ((1, -1.0), (2, 1.0)):
        m = ref.keep & (ref.instance == i)
        assert m.sum() > 100
        n = out["normals"][m]
        want = sign * np.array(FACING_NORMAL)
        assert np.abs(n[:, :3] - want).max() <= F32_OPS * F32_EPS        # the camera frame is the world frame here
        # n . v: towards the camera for the front face only; the farthest corner is 0.27 m and 0.13 m off the axis at 1 m:
        # cos >= 1 / sqrt(1 + 0.27^2 + 0.13^2) = 0.958
        assert (sign * n[:, 3] > 0.95).all()


def _inside_of_a_closed_cube_faces_the_camera(ref, out):
    """Scene 5b: every face is a back face, every normal is turned towards the camera."""
    m = ref.keep & ref.covered
    assert m.mean() > 0.9
    assert (out["normals"][m][:, 3] > 0).all()


def _slivers_and_tiny_triangles(ref, out):
    """Scene 6: a kept pixel is background or the triangle the ray hits -- never a triangle the reference does not hit; the tiny
    triangles are mostly uncovered, and some are covered."""
    k = ref.keep
    assert np.array_equal(out["vertex_idx"][k][:, :3], ref.vertex_idx[k][:, :3])
    assert not (out["instance"][k & ~ref.covered] != 0).any()
    assert 3 <= len(np.unique(ref.tri[(ref.instance == 2) & k])) < 128


def _interpenetration_changes_the_winner(ref, out):
    """Scene 7a: each cube owns kept pixels that the other one's rays meet too, and margin (b) is in use along their line."""
    both = ref.any_hit[1] & ref.any_hit[2] & ref.keep
    assert (out["instance"][both] == 1).sum() > 50 and (out["instance"][both] == 2).sum() > 50
    assert ref.left["depth"].sum() > 0


def _coincident_cubes_go_to_the_first(ref, out):
    """Scene 7b: rule R6's tie.  Both cubes are hit at the same depth everywhere; every pixel, kept or not, shows the first."""
    assert np.array_equal(ref.any_hit[1], ref.any_hit[2])
    assert set(np.unique(out["instance"]).tolist()) == {0, 1}
    assert (out["instance"][ref.keep & ref.covered] == 1).all()


def _borders(ref, out):
    """Scene 8: the large triangle fills the picture behind four cubes that each leave it through another border."""
    assert ref.covered.all()
    for i, edge in ((2, ref.instance[:, 0]), (3, ref.instance[:, -1]), (4, ref.instance[0]), (5, ref.instance[-1])):
        assert (edge == i).sum() > 5 and (ref.instance == i).sum() > 100


ALSO = {"clip": _near_clip_keeps_the_original_triangle, "facing": _facing_of_a_hand_made_triangle,
        "inside_cube": _inside_of_a_closed_cube_faces_the_camera, "sliver": _slivers_and_tiny_triangles,
        "interpenetrating": _interpenetration_changes_the_winner, "coincident": _coincident_cubes_go_to_the_first,
        "borders": _borders}


def check(name, ref, out, label=None, **kw):
    """compare + report + the bound + the scene's own assertions; returns the figures."""
    label = label or name
    kind = name.split("@")[0]
    fig = compare(ref, out, cap=SLIVER_CAP if kind == "sliver" else LEFT_OUT_CAP, label=label, **kw)
    report(label, fig)
    assert_within(fig, label)
    if kind in ALSO:
        ALSO[kind](ref, out)
    return fig
