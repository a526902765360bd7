"""Seeded scene builders shared by the CPU (oracle) tests and the GPU parity tests."""
import math
import os

import numpy as np
import torch

FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fixtures")
CUBE = os.path.join(FIXTURES, "cube.glb")
BUNNY = os.path.join(FIXTURES, "stanford_bunny", "scene.gltf")

_mesh_cache = {}


def mesh(sl, path, physics=False):
    key = (path, physics)
    if key not in _mesh_cache:
        _mesh_cache[key] = sl.Mesh(path, physics=physics)
    return _mesh_cache[key]


def cube_lookat_scene(sl, size=(640, 480)):
    """reference tests/basic.cpp:375-453: cube seen from (4,0,0) looking at the origin."""
    m = sl.Mesh(CUBE, physics=False)
    scene = sl.Scene(size)
    obj = sl.Object(m)
    scene.add_object(obj)
    scene.set_camera_look_at(torch.tensor([4.0, 0.0, 0.0]), torch.tensor([0.0, 0.0, 0.0]))
    return scene


def random_rotation(rng):
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    x, y, z, w = q
    return np.array([
        [1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
        [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
        [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)],
    ], dtype=np.float32)


def clutter_scene(sl, seed, n_objects=6, size=(320, 240), with_bunny=False, plane=True, light=True):
    """Random heap of cubes (and optionally a bunny) on a plane, camera looking down at it."""
    rng = np.random.default_rng(seed)
    scene = sl.Scene(size, seed=seed)
    cube = sl.Mesh(CUBE, physics=False)
    cube.center_bbox()
    cube.scale_to_bbox_diagonal(0.2)
    meshes = [cube]
    if with_bunny:
        b = sl.Mesh(BUNNY, physics=False)
        b.center_bbox()
        b.scale_to_bbox_diagonal(0.3)
        b.class_index = 2
        meshes.append(b)
    for i in range(n_objects):
        m = meshes[i % len(meshes)]
        obj = sl.Object(m)
        pose = np.eye(4, dtype=np.float32)
        pose[:3, :3] = random_rotation(rng)
        pose[:3, 3] = [rng.uniform(-0.25, 0.25), rng.uniform(-0.25, 0.25), rng.uniform(0.05, 0.3)]
        obj.set_pose(torch.from_numpy(pose))
        obj.metallic = float(rng.uniform(0, 1))
        obj.roughness = float(rng.uniform(0, 1))
        scene.add_object(obj)
    az = rng.uniform(-math.pi, math.pi)
    cam = np.array([1.2 * math.cos(az), 1.2 * math.sin(az), 0.9], dtype=np.float32)
    scene.set_camera_look_at(torch.from_numpy(cam), torch.tensor([0.0, 0.0, 0.1]))
    if plane:
        scene.background_plane_size = torch.tensor([3.0, 3.0])
    if light:
        scene.choose_random_light_direction()
    scene.ambient_light = torch.tensor([0.1, 0.1, 0.1])
    return scene


def delaunay_sheet(sl, n_points, seed, reverse=False, half=1.0):
    """A watertight flat sheet in the mesh's z = 0 plane: `n_points` random interior points plus a dense border, Delaunay
    triangulated (every interior edge is shared by exactly two triangles).  `reverse` keeps the geometry and submits the
    triangles in the opposite order -- on a fronto-parallel sheet every triangle has the SAME depth, so the depth test
    (LESS, earlier triangle wins) makes any pixel that two triangles both claim change its owner."""
    from scipy.spatial import Delaunay

    from stillleben_amd import _loaders

    rng = np.random.default_rng(seed)
    nb = max(8, int(math.sqrt(n_points)))
    t = np.linspace(-half, half, nb, endpoint=False)
    border = np.concatenate([np.stack([t, np.full(nb, -half)], 1), np.stack([np.full(nb, half), t], 1),
                             np.stack([-t, np.full(nb, half)], 1), np.stack([np.full(nb, -half), -t], 1)])
    pts = np.concatenate([border, rng.uniform(-half, half, (n_points, 2))]).astype(np.float32)
    tri = Delaunay(pts.astype(np.float64)).simplices.astype(np.uint32)
    a, b, c = pts[tri[:, 0]], pts[tri[:, 1]], pts[tri[:, 2]]
    cw = ((b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])) < 0
    tri[cw] = tri[cw][:, ::-1]                      # counter-clockwise seen from +z
    if reverse:
        tri = tri[::-1]
    cm = _loaders.ConsolidatedMesh()
    cm.positions = np.concatenate([pts, np.zeros((len(pts), 1), np.float32)], 1)
    cm.normals = np.tile(np.array([[0, 0, 1]], np.float32), (len(pts), 1))
    cm.uvs = (pts * 0.5 + 0.5).astype(np.float32)
    cm.colors = np.ones((len(pts), 4), np.float32)
    cm.indices = np.ascontiguousarray(tri).reshape(-1).astype(np.uint32)
    cm.textures = []
    cm._tex_alpha = []
    cm.materials = [_loaders.Material(base_color=(0.8, 0.8, 0.8, 1))]
    cm.submeshes = [_loaders.SubMesh(0, len(cm.indices), 0)]
    return sl.Mesh.from_data(cm, hulls=[], filename="memory://sheet%d" % seed)


def sheet_scene(sl, mesh, roll_deg=17.0, tilt_deg=0.0, distance=4.0, size=(320, 240)):
    """The sheet in front of the camera (camera at the origin looking along its optical axis): rolled about the optical
    axis so that no edge is pixel-aligned, optionally tilted (then depths differ across the sheet)."""
    scene = sl.Scene(size)
    obj = sl.Object(mesh)
    r, t = math.radians(roll_deg), math.radians(tilt_deg)
    Rz = np.array([[math.cos(r), -math.sin(r), 0], [math.sin(r), math.cos(r), 0], [0, 0, 1]])
    Ry = np.array([[math.cos(t), 0, math.sin(t)], [0, 1, 0], [-math.sin(t), 0, math.cos(t)]])
    cam = scene.camera_pose().numpy().astype(np.float64)          # camera-to-world; the camera looks along its +z
    P = np.eye(4)
    P[:3, :3] = Ry @ Rz @ np.diag([1.0, -1.0, -1.0])              # sheet normal towards the camera
    P[:3, 3] = [0.0, 0.0, distance]
    obj.set_pose(torch.from_numpy((cam @ P).astype(np.float32)))
    scene.add_object(obj)
    return scene


# ---- settle scenes whose solver list has a known row structure (tests of the per-scene list capacities) -------------------------
# A cube face-down on the table or on another cube is a patch of four points behind its centre row: five rows in the list; a cube
# on one of its edges is a patch of two points without a centre row.  The table's patches come first, in body order, then the
# hull pairs'.  The sliders keep sliding for the first frames: a wrong friction row would change their velocities.
CUT_TABLE = 0.04
CUT_ROWS = {"sliders": 25, "edge": 17, "long": 40, "grid": 500, "row": 25}    # rows each of the first steps offers
CUT_PAIRS = {"sliders": 1, "edge": 2, "long": 2, "grid": 0, "row": 2}          # hull pairs = touching body pairs (a cube is one hull)
CUT_VELOCITY = (1.2, 0.6, 0.0)                                      # of the sliders of variant 0
_cut_cube = {}


def _cut_pose(x, y, z, yaw=0.0, roll=0.0):
    cy, sy, cr, sr = math.cos(yaw), math.sin(yaw), math.cos(roll), math.sin(roll)
    p = np.eye(4, dtype=np.float32)
    p[:3, :3] = np.array([[cy, -sy, 0.0], [sy, cy, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[1.0, 0.0, 0.0], [0.0, cr, -sr], [0.0, sr, cr]])
    p[:3, 3] = (x, y, z)
    return p


def cut_scene(sl, kind, variant=0):
    """kind "sliders": three yawed cubes sliding face-down on the table + a column of two (four table patches and one face patch,
    five rows each: 25); "edge": a cube sliding on one edge (2 rows) + a column of three (5 + 2 x 5: 17); "long": five sliders + a
    column of three (40); "grid": 100 sliders, 10 x 10 (500); "row": three cubes side by side on the table, sliding across the row
    (three table patches and two side patches: 25; every body has a table group).  `variant` turns the yaws and the direction of
    sliding: the same rows."""
    if sl not in _cut_cube:
        m = sl.Mesh(CUBE)
        m.center_bbox()
        m.scale_to_bbox_diagonal(0.2)
        _cut_cube[sl] = m
    h = 0.2 / math.sqrt(3.0) / 2.0
    z0 = CUT_TABLE + h + 0.0015                                         # resting on the table (rest offset)
    a = 0.7 * variant
    v = CUT_VELOCITY if variant == 0 else (1.35 * math.cos(0.46 + a), 1.35 * math.sin(0.46 + a), 0.0)
    items = []
    if kind in ("sliders", "long"):
        n = 3 if kind == "sliders" else 5
        items += [(_cut_pose(-0.6 + 0.3 * k, 0.4, z0, yaw=0.3 + 0.25 * k + a), v) for k in range(n)]
    if kind == "edge":
        items.append((_cut_pose(-0.4, 0.0, CUT_TABLE + h * math.sqrt(2.0) + 0.0015, yaw=a, roll=math.pi / 4),
                      (1.2 * math.cos(a), 1.2 * math.sin(a), 0.0)))                  # sliding along its edge
    if kind == "row":
        c, s_ = math.cos(a), math.sin(a)
        items += [(_cut_pose(k * (2 * h + 0.001) * c, k * (2 * h + 0.001) * s_, z0, yaw=a), (-1.2 * s_, 1.2 * c, 0.0)) for k in (-1, 0, 1)]
    if kind == "grid":
        items += [(_cut_pose(0.3 * (i - 5), 0.3 * (j - 5), z0, yaw=0.1 + 0.05 * (10 * i + j) + a), v) for i in range(10) for j in range(10)]
    column = {"sliders": 2, "edge": 3, "long": 3, "grid": 0, "row": 0}[kind]
    items += [(_cut_pose(0.3, -0.3, z0 + k * (2 * h + 0.003), yaw=0.2 + a), None) for k in range(column)]
    scene = sl.Scene((64, 48))
    for p, vel in items:
        o = sl.Object(_cut_cube[sl])
        scene.add_object(o)
        o.set_pose(torch.from_numpy(p))
        if vel is not None:
            o.linear_velocity = torch.tensor(vel, dtype=torch.float32)
    return scene
