"""The raster passes of slhip_render give the same bits whichever way a triangle is walked: the default (32-bit edge walk where a
triangle qualifies, sized shadow window), SLHIP_RASTER_WIDE=1 (the 64-bit walk everywhere) and SLHIP_SHADOW_SMALL=0
SLHIP_RASTER_SMALL=0 (every triangle through the tile-queue kernels), rendered in one process.  The scenes are built from small
OBJ files so that the light-space pixel boxes -- recomputed here in numpy from the scene record's shadow_mat -- sit on the
thresholds of the kernels: the in-place / queue limit kSmallArea, the narrow bound of slhip_raster_walk.h, the 64 x 64 LDS window
of k_shadow_raster, chunks of 1 / 63 / 64 / 65 / 256 triangles.

Geometry is laid out in the light's frame (x, y: the map's axes), so a right-angled triangle with legs along them has a box of
its legs.  A `frame` object of four corner triangles fixes the fit of the shadow matrix (it clamps x / y to the objects' bounding
spheres), hence the texel size -- about 0.75 mm with the 0.4 m frame below; it is measured from the shadow matrix of the frame
alone (`calibrate`) before the other meshes are written.

(The packed emission of the in-place walk -- case (f) of the issue that asked for these tests -- was not built; there is no
queue of covered texels to drain, so there is no case for it.)"""
import os
import sys

import numpy as np
import pytest
import torch

from stillleben_amd import _abi
from stillleben_amd._batch import HostPool, build_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import raster_box_stats as RB  # noqa: E402   (the numpy restatement of snap / setup_finish)

pytestmark = pytest.mark.gpu

S = 2048                    # the engine's shadow map (_engine.SHADOW_RES)
SMALL = 256                 # kSmallArea
MODES = ({}, {"SLHIP_RASTER_WIDE": "1"}, {"SLHIP_SHADOW_SMALL": "0", "SLHIP_RASTER_SMALL": "0"})
LIGHT = np.array([-0.3, 0.2, -1.0]) / np.linalg.norm([-0.3, 0.2, -1.0])
FRAME = 0.4                 # half side of the frame, metres
TEXEL = 2.0 * FRAME * np.sqrt(2.0) / S       # metres per texel along the map's axes: a first guess, then what calibrate() measured


def light_axes(d=LIGHT):
    """x, y, z of the light's frame in world coordinates (shadow_matrix of slhip_records.cpp)."""
    z = d / np.linalg.norm(d)
    x = np.cross(z, [0.0, 0.0, 1.0]); x /= np.linalg.norm(x)
    y = np.cross(z, x); y /= np.linalg.norm(y)
    return x, y, z


def to_world(p_light, origin=(0.0, 0.0, 0.15)):
    """Points given in the light's frame (metres) about `origin`."""
    x, y, z = light_axes()
    p = np.asarray(p_light, np.float64)
    return np.asarray(origin) + p[:, :1] * x + p[:, 1:2] * y + p[:, 2:3] * z


class Soup:
    """Triangles in the light's frame, one vertex triple each."""

    def __init__(self):
        self.v, self.f = [], []

    def tri(self, a, b, c, both=False):
        n = len(self.v)
        self.v += [a, b, c]
        self.f.append((n, n + 1, n + 2))
        if both:
            self.f.append((n, n + 2, n + 1))
        return self

    def right(self, x, y, lx, ly, z=0.0, both=True, drawn=True):
        """Right angle at (x, y), legs lx / ly along the map's axes, all in TEXELS.  drawn=False: the winding the shadow pass
        culls (its light-space area2 is negative)."""
        a, b, c = (x * TEXEL, y * TEXEL, z), ((x + lx) * TEXEL, y * TEXEL, z), (x * TEXEL, (y + ly) * TEXEL, z)
        return self.tri(a, b, c, both) if (drawn or both) else self.tri(a, c, b)

    def mesh(self, sl, path, origin=(0.0, 0.0, 0.15)):
        V = to_world(np.array(self.v), origin)
        with open(path, "w") as fh:
            for p in V:
                fh.write("v %.9g %.9g %.9g\n" % tuple(p))
            for t in self.f:
                fh.write("f %d %d %d\n" % (t[0] + 1, t[1] + 1, t[2] + 1))
        return sl.Mesh(str(path), physics=False)


def map_axes(scene, origin=(0.0, 0.0, 0.15)):
    """(ax, bx, ay, by): texel = a * (light-frame coordinate in metres about `origin`) + b, from the scene's shadow_mat."""
    pool = HostPool()
    srec, _, _ = build_batch([scene], pool, with_shadows=True)
    M = srec[0]["shadow_mat"][0].reshape(4, 4).astype(np.float64)
    P = np.concatenate([to_world(np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), origin), np.ones((3, 1))], axis=1)
    t = ((P @ M.T)[:, :2] * 0.5 + 0.5) * S
    return t[1, 0] - t[0, 0], t[0, 0], t[2, 1] - t[0, 1], t[0, 1]


def calibrate(sl, tmp_path):
    """Sets TEXEL to what the frame alone makes of it (the other objects lie inside the frame's bounding sphere)."""
    global TEXEL
    ax, _, ay, _ = map_axes(scene_of(sl, tmp_path, [("frame", frame_soup())], (128, 96)))
    assert ax > 0 and ay > 0 and abs(ax / ay - 1.0) < 1e-4
    TEXEL = 1.0 / ax


def frame_soup():
    s = Soup()
    for sx in (-1, 1):
        for sy in (-1, 1):
            cx, cy = sx * FRAME / TEXEL, sy * FRAME / TEXEL
            s.right(cx, cy, -sx * 40.0, -sy * 40.0)
    return s


def ladder_soup():
    """(a): legs of 0.2 k texels, k = 1 .. 130, on a 12-column grid (boxes 1 x 1 .. 27 x 27 = 729 > 2 kSmallArea), then legs of
    30 .. 110 texels: past the narrow bound (8192 texels of vertex extent) as well."""
    s = Soup()
    for k in range(1, 131):
        col, row = (k - 1) % 12, (k - 1) // 12
        s.right(-330.0 + 30.0 * col + 0.37, -330.0 + 30.0 * row + 0.41, 0.2 * k, 0.2 * k, z=0.0)
    for j, leg in enumerate(range(30, 111, 10)):
        s.right(-330.0 + 115.0 * (j % 5) + 0.3, 60.0 + 120.0 * (j // 5) + 0.2, float(leg), float(leg), z=0.0)
    return s


def sheet_soup(n_tris, x0, y0, cell=6.0, cols=16, z=0.0, pattern="drawn"):
    """(b): n_tris triangles in one draw = one chunk (or a full one and a rest): two per grid cell.  pattern: `drawn`, `culled`
    (every triangle faces the light) or `mixed` (drawn, culled, zero area in turn)."""
    s = Soup()
    for i in range(n_tris):
        c = i // 2
        x, y = x0 + cell * (c % cols), y0 + cell * (c // cols)
        kind = {"drawn": 0, "culled": 1, "mixed": i % 3}[pattern]
        if kind == 2:                                         # zero area: three points on a line
            s.tri((x * TEXEL, y * TEXEL, z), ((x + 2) * TEXEL, (y + 2) * TEXEL, z), ((x + 4) * TEXEL, (y + 4) * TEXEL, z))
        elif i % 2 == 0:
            s.right(x, y, cell, cell, z=z, both=False, drawn=kind == 0)
        else:
            s.right(x + cell, y + cell, -cell, -cell, z=z, both=False, drawn=kind == 0)
    return s


def scene_of(sl, tmp_path, soups, size, lights=1, cam_height=1.8):
    sc = sl.Scene(size)
    for i, (name, soup) in enumerate(soups):
        o = sl.Object(soup.mesh(sl, tmp_path / ("%s_%d.obj" % (name, i))))
        o.metallic, o.roughness = 0.0, 1.0
        sc.add_object(o)
    sc.background_plane_size = torch.tensor([3.0, 3.0])
    sc.set_camera_look_at(torch.tensor([0.0, 0.0, cam_height]), torch.tensor([0.0, 0.0, 0.0]), up=(0.0, 1.0, 0.0))
    dirs = [LIGHT.tolist(), [0.5, 0.1, -1.0], [-0.1, -0.6, -1.0]]
    cols = [[3.0, 3.0, 3.0], [2.0, 1.0, 0.5], [0.5, 1.0, 2.0]]
    sc.light_directions = torch.tensor([dirs[i] if i < lights else [0.0] * 3 for i in range(3)])
    sc.light_colors = torch.tensor([cols[i] if i < lights else [0.0] * 3 for i in range(3)])
    sc.ambient_light = torch.tensor([0.1, 0.1, 0.1])
    sc.manual_exposure = 1.0
    return sc


def main_soups():
    two_sheets = Soup()                                         # (d) lanes of ONE wave: far and near triangle over the same texels, in turn
    for c in range(24):
        x, y = 150.0 + 9.0 * (c % 6), -300.0 + 9.0 * (c // 6)
        two_sheets.right(x, y, 8.0, 8.0, z=0.0, both=False)
        two_sheets.right(x, y, 8.0, 8.0, z=-0.02, both=False)     # 2 cm nearer to the light
    straddle = Soup()                                           # (e) one chunk whose boxes leave its 64 x 64 window on every side
    straddle.right(0.0, -200.0, 6.0, 6.0)
    for k, (dx, dy) in enumerate(((58.0, 0.0), (0.0, 58.0), (60.5, 60.5), (63.0, 3.0), (3.0, 63.0), (90.0, 20.0), (20.0, 90.0))):
        straddle.right(dx, -200.0 + dy, 12.0, 12.0 + (k % 3))
    return [("frame", frame_soup()), ("ladder", ladder_soup()),
            ("one", sheet_soup(1, -100.0, -250.0)), ("c63", sheet_soup(63, -60.0, -250.0)),
            ("facing64", sheet_soup(64, 40.0, -250.0, pattern="culled")), ("c65", sheet_soup(65, -200.0, -250.0)),
            ("mixed256", sheet_soup(256, -330.0, 330.0 - 60.0, cols=40, pattern="mixed")),
            # (d) different chunks: a sheet under the drawn 63 and the culled 64, 3 cm farther from the light
            ("under", sheet_soup(128, -60.0, -250.0, cols=40, z=0.03)),
            ("two_sheets", two_sheets), ("straddle", straddle)]


def strip_soups(axes=None):
    """(c): triangles far longer than the camera's footprint, which is what bounds the map here: they cross every edge of it.
    Triangles that poke a corner of a few texels into a corner of the map from far outside (walked in place, vertex extents far
    beyond the narrow bound) share their waves with ordinary small triangles.  axes: map_axes() of the scene without the
    pokers -- they lie inside the strips' bounding box, so the fit stays what it was."""
    far = 60.0                                                   # metres
    ax, bx, ay, by = axes if axes is not None else (1.0 / TEXEL, S / 2, 1.0 / TEXEL, S / 2)
    tx, ty = 1.0 / ax, 1.0 / ay                                  # metres per texel of THIS map
    s = Soup()
    for k in range(40):
        x, y = (-20.0 + 7.0 * (k % 8)) * tx, (-20.0 + 7.0 * (k // 8)) * ty
        s.tri((x, y, 0.0), (x + 5.0 * tx, y, 0.0), (x, y + 6.0 * ty, 0.0), both=True)       # small, narrow
        if k % 4 == 0:
            c = (k - 20) * 9.0
            s.tri((-far, c * ty, 0.0), (far, (c + 3.0) * ty, 0.0), (far, (c - 3.0) * ty, 0.0), both=True)   # crosses left and right
            s.tri((c * tx, -far, 0.0), ((c + 3.0) * tx, far, 0.0), ((c - 3.0) * tx, far, 0.0), both=True)   # crosses top and bottom
        if axes is not None and k % 5 == 0:                      # the corner pokers, spread over the waves
            j = k // 5
            sx, sy = (1, -1)[j & 1], (1, -1)[(j >> 1) & 1]
            depth = 6.3 + 2.0 * (j >> 2)                          # texels inside the map's corner
            px = ((0.0 if sx > 0 else S) + sx * depth - bx) * tx
            py = ((0.0 if sy > 0 else S) + sy * depth - by) * ty
            s.tri((px, py, 0.0), (px - sx * far, py, 0.0), (px, py - sy * far, 0.0), both=True)
    return [("strip", s), ("c65", sheet_soup(65, -50.0, 40.0))]


def strip_scene(sl, tmp_path, cam_height):
    first = scene_of(sl, tmp_path, strip_soups(), (130, 98), cam_height=cam_height)
    axes = map_axes(first)
    scene = scene_of(sl, tmp_path, strip_soups(axes), (130, 98), cam_height=cam_height)
    assert np.allclose(map_axes(scene), axes, rtol=1e-6)
    return scene


def caster_boxes(scene, light=0, size=S):
    """Per caster draw: the numpy set-up (tools/raster_box_stats.py) of its triangles in the light's map."""
    pool = HostPool()
    srec, drec, crec = build_batch([scene], pool, with_shadows=True)
    arrays = pool.arrays()
    pos, idx = arrays[0], arrays[4]
    out = []
    for d in drec:
        if not int(d["flags"]) & _abi.DRAW_CASTS_SHADOW:
            continue
        T1 = (d["object_to_world"].reshape(4, 4) @ d["mesh_to_object"].reshape(4, 4)).astype(np.float32)
        M = (srec[0]["shadow_mat"][light].reshape(4, 4) @ T1).astype(np.float32)
        X, Y, _ = RB.window_coords(M, pos[int(d["vtx_base"]):int(d["vtx_base"]) + int(d["n_verts"])], 0.5 * size, 0.5 * size)
        tri = idx[int(d["idx_base"]):int(d["idx_base"]) + 3 * int(d["n_tris"])].reshape(-1, 3).astype(np.int64)
        t = RB.setup(X[tri], Y[tri], size, size)
        t["drawn"] = t["ok"] & ~t["flipped"]
        out.append(t)
    return out, crec


def queue_items(boxes):
    n = 0
    for t in boxes:
        d = t["drawn"]
        n += int((((t["xmax"][d] >> 3) - (t["xmin"][d] >> 3) + 1) * ((t["ymax"][d] >> 3) - (t["ymin"][d] >> 3) + 1)).sum())
    return n


@pytest.fixture(scope="module")
def eng(sl):
    from stillleben_amd._context import engine

    return engine()


def render_modes(eng, scenes):
    """OUT_ALL plus the kept HDR image of `scenes`, once per mode, as dicts of numpy arrays."""
    W, H = scenes[0].viewport
    outs = []
    saved = {k: os.environ.get(k) for m in MODES for k in m}
    try:
        for mode in MODES:
            for k in saved:
                os.environ.pop(k, None)
            os.environ.update(mode)
            bufs = eng.render(scenes, _abi.OUT_ALL, ssao=True, shadows=True, keep_hdr=True)
            torch.cuda.synchronize()
            out = {}
            for name in ("rgb", "instance", "cls", "vertex_idx", "coord", "bary", "cam_coord", "normals"):
                t = getattr(bufs, name, None)
                if t is not None:
                    out[name] = t.cpu().numpy().copy()
            n = 2 * len(scenes) * H * W * 4
            out["hdr"] = bufs._keepalive[0]["hdr"].view(torch.float32)[:n].cpu().numpy().copy()
            outs.append((bufs, out))
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return outs


def assert_modes_equal(outs):
    ref = outs[0][1]
    assert {"rgb", "instance", "coord", "normals", "hdr"} <= set(ref)
    for mode, (_, out) in zip(MODES[1:], outs[1:]):
        assert set(out) == set(ref)
        for name, a in ref.items():
            b = out[name]
            same = a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
            assert same, "%s differs under %s at %d values" % (name, mode, int((a != b).sum()))


def shadowed_share(outs, H, W):
    """Share of the plane's pixels whose HDR value is below the frame's median: the casters' shadows reach the picture."""
    hdr = outs[0][1]["hdr"][: H * W * 4].reshape(H, W, 4)[..., 0]
    plane = outs[0][1]["instance"].reshape(H, W, -1)[..., 0] == 0
    v = hdr[plane]
    return float((v < 0.8 * np.median(v)).mean())


@pytest.fixture(scope="module", autouse=True)
def calibrated(sl, tmp_path_factory):
    calibrate(sl, tmp_path_factory.mktemp("raster_frame"))


@pytest.fixture(scope="module")
def main_scene(sl, tmp_path_factory):
    return scene_of(sl, tmp_path_factory.mktemp("raster_main"), main_soups(), (128, 96))


def test_main_scene_boxes_sit_on_the_thresholds(sl, main_scene):
    """The numpy side of cases (a), (b), (d), (e): the scene asks of the kernels what its docstrings say.  (Needs no GPU call of
    its own; it is marked with the rest of the module because it vouches for the renders below.)"""
    boxes, crec = caster_boxes(main_scene)
    names = [n for n, _ in main_soups()]
    by = dict(zip(names, boxes))
    # (a) the ladder: from 1 x 1 past 2 kSmallArea in steps of at most one texel per side, then past the narrow bound
    t = by["ladder"]
    d = t["drawn"]
    assert not t["drawn"][1::2].any() and t["drawn"][260::2].all()      # one winding of every triangle, all of the large ones
    small = np.nonzero(d[:260])[0]                              # (the smallest legs may miss every texel centre)
    assert len(small) >= 120
    w, h = (t["xmax"] - t["xmin"] + 1)[small], (t["ymax"] - t["ymin"] + 1)[small]
    order = np.lexsort((w, w + h))
    assert (w[order][0], h[order][0]) == (1, 1) and w.max() * h.max() > 2 * SMALL
    assert np.abs(np.diff(w[order])).max() <= 1 and np.abs(np.diff(h[order])).max() <= 1
    area = w * h
    assert (area <= SMALL).sum() > 50 and (area > SMALL).sum() > 10 and (np.abs(area - SMALL) <= 32).any()
    assert t["narrow"][small].all()
    big = t["narrow"][260::2]
    assert (t["xmax"] - t["xmin"] + 1)[260::2].max() in (110, 111)      # the texel is what calibrate() measured
    assert big.any() and not big.all()                          # the narrow / wide boundary lies inside the large ones
    # (b) chunk sizes, the light-facing chunk, the mixed one
    counts = sorted(int(c["count"]) for c in crec)
    assert {1, 63, 64, 65, 256} <= set(counts), counts
    assert by["facing64"]["ok"].all() and not by["facing64"]["drawn"].any()
    m = by["mixed256"]
    assert m["drawn"].sum() > 60 and (m["ok"] & m["flipped"]).sum() > 60 and (~m["ok"]).sum() > 60
    assert by["c63"]["drawn"].all() and by["one"]["drawn"].all() and by["c65"]["drawn"].all()
    # (d) the sheet `under` lies behind the 63 and the 64 in the same texels
    u = by["under"]
    assert u["xmin"][u["drawn"]].min() <= by["c63"]["xmin"].min() and u["xmax"][u["drawn"]].max() >= by["c63"]["xmax"].max()
    # (e) one chunk, boxes inside and outside the window at its corner, one across each edge
    s = by["straddle"]
    d = s["drawn"]
    x0, y0 = s["xmin"][d].min(), s["ymin"][d].min()
    rx0, rx1, ry0, ry1 = s["xmin"][d] - x0, s["xmax"][d] - x0, s["ymin"][d] - y0, s["ymax"][d] - y0
    assert (s["n"][d] <= SMALL).all()
    assert ((rx0 < 64) & (rx1 >= 64) & (ry1 < 64)).any() and ((ry0 < 64) & (ry1 >= 64) & (rx1 < 64)).any()
    assert ((rx0 < 64) & (rx1 >= 64) & (ry0 < 64) & (ry1 >= 64)).any() and ((rx0 >= 64) | (ry0 >= 64)).any()
    # the queue-only rendering must not overflow the engine's 2^20 items (light map; the camera view is 128 x 96: 384 tiles at most
    # per triangle and a few thousand triangles)
    assert queue_items(boxes) < (1 << 20) // 8
    assert sum(len(t["ok"]) for t in boxes) * 192 < (1 << 20)


@pytest.mark.parametrize("lights,size", [(1, (128, 96)), (3, (130, 98))])
def test_three_walks_one_picture(sl, eng, tmp_path, lights, size):
    """Cases (a), (b), (d), (e) under one light at 128 x 96 (the tiled placement of k_shade) and (g) under three lights with
    different directions at 130 x 98 (the untiled one): every output and the float image, bit for bit, across the three modes."""
    scene = scene_of(sl, tmp_path, main_soups(), size, lights=lights)
    for l in range(lights):
        boxes, _ = caster_boxes(scene, l)
        assert queue_items(boxes) < (1 << 20) // 8
    outs = render_modes(eng, [scene])
    assert_modes_equal(outs)
    W, H = size
    inst = outs[0][1]["instance"].reshape(H, W, -1)[..., 0]
    assert len(np.unique(inst)) >= 8                            # the objects are in the picture
    assert shadowed_share(outs, H, W) > 0.002                   # ... and so are their shadows


def test_strip_across_the_map_edges(sl, eng, tmp_path):
    """Case (c), two scenes in one batch: clamped boxes, vertex extents far beyond the narrow bound, qualifying and
    non-qualifying lanes in one wave -- in the light's map and in the camera view."""
    scenes = [strip_scene(sl, tmp_path, h) for h in (0.9, 1.3)]
    for sc in scenes:
        boxes, _ = caster_boxes(sc)
        t = boxes[0]
        d = t["drawn"]
        walked = d & (t["n"] <= SMALL)
        assert (walked & t["narrow"]).sum() >= 30 and (walked & ~t["narrow"]).sum() >= 6      # mixed lanes, walked in place
        assert (walked & ~t["narrow"])[:64].any() and (walked & t["narrow"])[:64].any()        # ... in the first wave already
        assert (d & (t["n"] > SMALL) & ~t["narrow"]).sum() >= 8                                # ... and queued wide ones
        assert t["xmin"][d].min() == 0 and t["ymin"][d].min() == 0 and t["xmax"][d].max() == S - 1 and t["ymax"][d].max() == S - 1
        assert (t["ex"][d].max() >> 8) > 8 * S                  # vertex extents many maps wide
        assert queue_items(boxes) < (1 << 20) // 8
    outs = render_modes(eng, scenes)
    assert_modes_equal(outs)
    assert shadowed_share(outs, 98, 130) > 0.002


def test_default_walk_against_the_oracle(sl, oracle, eng, main_scene):
    """The main scene of the default mode against oracle.render, at the bar of tests/test_gpu_render.py: geometry bit for bit,
    8-bit colour within 1 LSB on all but 1e-4 of the values."""
    from stillleben_amd import _engine
    from test_gpu_render import assert_geometry_equal, assert_rgb_close

    W, H = main_scene.viewport
    bufs = eng.render([main_scene], _abi.OUT_ALL, ssao=True, shadows=True)
    torch.cuda.synchronize()
    pool = HostPool()
    srec, drec, _ = build_batch([main_scene], pool, with_shadows=True)
    flags = _abi.OUT_ALL | _abi.RENDER_SSAO | _abi.RENDER_SHADOWS
    ref = oracle.render(pool.arrays(), srec, drec, W, H, flags, shadow_res=_engine.SHADOW_RES)
    assert_geometry_equal(bufs, ref)
    assert_rgb_close(bufs, ref)
