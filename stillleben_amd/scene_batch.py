"""Batched scene synthesis: the GPU counterpart of the reference's per-scene host loop
(examples/ycb.py:36-80 -- build a scene from random meshes, `simulate_tabletop_scene`,
`choose_random_light_direction`, `RenderPass.render`) for MANY scenes at once, with every per-scene
step on the device (slhip_synth_stage -> slhip_settle -> slhip_synth_place -> slhip_render,
include/slhip.h).  The host describes the batch once (an asset table built from sl.Mesh objects, the
camera intrinsics, light colour, seed); per scene nothing crosses PCIe.

    table = sl.AssetTable(meshes)                       # once
    batch = sl.SceneBatch(table, n_scenes=4096, n_objects=20, resolution=(640, 480), seed=1)
    batch.set_camera_intrinsics(1066.778, 1067.487, 312.9869, 241.3109)
    batch.stage(); batch.settle(); batch.place()
    for chunk in batch.render_chunks(): ...             # RenderBuffers, [chunk, H, W, C] tensors in HBM
    scene = batch.scene(17)                             # an ordinary sl.Scene rebuilt from the device records

Domain randomisation of the picture (examples/ycb.py --ibl / --plane-texture, Scene.background_image): an
sl.EnvironmentBank of light maps, background images and plane textures, handed out per scene by the place step:

    bank = sl.EnvironmentBank(light_maps, backgrounds, plane_textures)          # once
    batch = sl.SceneBatch(table, 4096, 20, environment=bank, p_light_map=0.5)

Several pictures of one settled scene (a BOP scene: one pile, many images; sl.bop writes the entries):

    for v, chunk, buffers in batch.views(8): ...        # view 0 = the camera of place(); v >= 1 further drawn cameras
    batch.place(camera_poses=poses)                      # or the caller's cameras, [n_scenes, 4, 4] on the device
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _abi
from . import _settle_batch as SB
from ._batch import object_draws
from ._context import engine
from ._math import f32

PLANE_HALF_Z = 0.04   # BOX_HALF_EXTENTS.z (scene.cpp:638)


def _dev(arr, device):
    raw = np.frombuffer(np.ascontiguousarray(arr).tobytes(), dtype=np.uint8)
    if raw.size == 0:
        raw = np.zeros(16, np.uint8)
    return torch.from_numpy(raw.copy()).to(device)


def check_view_arguments(view, camera_poses, n_scenes, device):
    """The argument errors of SceneBatch.place(view=, camera_poses=): raised before anything is asked of the device."""
    if isinstance(view, bool) or int(view) != view or not 0 <= int(view) <= 0xFFFFFFFF:
        raise ValueError("view must be an integer in [0, 2^32)")
    if camera_poses is None:
        return
    if not isinstance(camera_poses, torch.Tensor) or camera_poses.dtype != torch.float32:
        raise ValueError("camera_poses must be a float32 torch tensor")
    if tuple(camera_poses.shape) != (int(n_scenes), 4, 4) or not camera_poses.is_contiguous():
        raise ValueError("camera_poses must be a contiguous [n_scenes, 4, 4] = [%d, 4, 4] tensor" % n_scenes)
    if camera_poses.device != torch.device(device):
        raise ValueError("camera_poses must live on the batch's device (%s), not on %s" % (device, camera_poses.device))


class AssetTable:
    """slhip_asset records + sub-mesh draw templates of a list of sl.Mesh objects (built once; the meshes'
    vertices, textures and hulls are registered with the process-wide pools)."""

    def __init__(self, meshes, mesh_pool=None, hull_pool=None):
        """`mesh_pool` / `hull_pool`: host pools to register with instead of the device engine's (the CPU tests
        build the records for the oracle that way); a table built on explicit pools cannot drive a SceneBatch."""
        from .object import Object

        if not meshes:
            raise ValueError("AssetTable needs at least one mesh")
        if len(meshes) > _abi.SYNTH_MAX_ASSETS:
            raise ValueError("at most %d classes per asset table" % _abi.SYNTH_MAX_ASSETS)
        self.meshes = list(meshes)
        if mesh_pool is None or hull_pool is None:
            from . import physics

            self.eng = engine()
            self.se = physics.settle_engine()
            mesh_pool, hull_pool = self.eng.pool, self.se.pool
        else:
            self.eng = self.se = None
        self.mesh_pool, self.hull_pool = mesh_pool, hull_pool
        recs = np.zeros(len(meshes), dtype=_abi.ASSET_DTYPE)
        templates = []
        self.n_hulls, self.n_hull_verts, self.n_draws, self.n_chunks, self.n_clip = [], [], [], [], []
        for i, mesh in enumerate(self.meshes):
            obj = Object(mesh)                               # the defaults of sl.Object (material, flags)
            draws = object_draws(obj, mesh_pool)
            hb, he, bc, br = hull_pool.register(mesh)
            p = obj._props()
            r = recs[i]
            r["mesh_to_object"] = mesh._pretransform.reshape(-1)
            bbox = mesh.bbox
            r["bbox_min"][:3], r["bbox_max"][:3] = bbox._min, bbox._max
            r["com"][:3] = p.com
            ii = np.zeros((3, 4), np.float32)
            ii[:, :3] = p.inv_inertia
            r["inv_inertia"] = ii.reshape(-1)
            r["mass"] = p.mass
            r["mu_s"], r["mu_d"], r["restitution"] = obj._static_friction, obj._dynamic_friction, obj._restitution
            r["bsphere"][:3], r["bsphere"][3] = bc, br
            r["hull_begin"], r["hull_end"] = hb, he
            r["draw_begin"], r["draw_count"] = len(templates), len(draws)
            r["n_verts"] = draws[0]["n_verts"] if draws else 0
            chunks = sum((int(d["n_tris"]) + _abi.CHUNK_TRIS - 1) // _abi.CHUNK_TRIS for d in draws)
            r["n_chunks"] = chunks
            for d in draws:
                d["mesh_to_object"] = 0.0
                d["object_to_world"] = 0.0
                d["normal_to_world"] = 0.0
                d["instance_index"] = 0
                templates.append(d)
            hulls = hull_pool.hulls[hb:he]
            self.n_hulls.append(he - hb)
            self.n_hull_verts.append(int(sum(int(h["vtx_count"]) for h in hulls)))
            self.n_draws.append(len(draws))
            self.n_chunks.append(chunks)
            self.n_clip.append(int(r["n_verts"]) * len(draws))
        self.records = recs
        self.templates = np.array(templates, dtype=_abi.DRAW_DTYPE)
        self._dev = None

    def __len__(self):
        return len(self.meshes)

    def device(self):
        if self.eng is None:
            raise _abi.SlhipError("this AssetTable was built on host pools (test helper); build it without them to use the device")
        if self._dev is None:
            d = self.eng.device
            self._dev = (_dev(self.records, d), _dev(self.templates, d))
        return self._dev

    def bound(self, per_asset, n_objects, distinct):
        """Largest possible per-scene sum of a per-class quantity: the n_objects largest classes when classes are
        drawn without replacement, n_objects times the largest otherwise."""
        v = sorted(per_asset, reverse=True)
        return int(sum(v[:n_objects])) if distinct else int(v[0]) * n_objects


class SceneBatch:
    """n_scenes tabletop scenes of n_objects objects each, resident in HBM.  `asset_ids` ([n_scenes, n_objects]
    class indices into the table) fixes every scene's objects; without it each scene draws n_objects DISTINCT
    classes (examples/ycb.py:60).  `random_pbr`: metallic / roughness ~ U(0,1) per object (examples/ycb.py:63-64).

    `environment`: an sl.EnvironmentBank.  place() then gives every scene a light map with probability `p_light_map`, a
    background image with `p_background` and a plane texture with `p_plane_texture`, each picked uniformly from the bank
    with the batch's counter-based random streams (stream 4 of include/slhip.h; the probability of a kind the bank has no
    entry of is not used) -- or exactly what `env_ids` ([n_scenes, 3] = light set, background, plane texture; -1 = none)
    names.  A scene with a light map is lit by the map and the map's lights, without ambient term, as `scene.light_map`
    does it on the per-scene path; the others keep the drawn light.  host_env() tells what every scene got.

    Memory: the render scratch holds one 2048 x 2048 f32 shadow map per scene and LIGHT, 16.8 MB each, and a batch on a bank
    renders with as many as the bank's largest light set has (at least 1): a 512-scene render chunk takes 8.6 GB of shadow
    maps with one-light maps and 25.8 GB with three-light maps.  The engine checks the free memory before it allocates;
    choose `render_chunk` accordingly.  Further views (place(view=...), views()) overwrite the one record set and render into
    the same scratch: they add nothing to this, object_to_camera 48 bytes per object."""

    def __init__(self, table, n_scenes, n_objects, resolution=(640, 480), seed=0, asset_ids=None, random_pbr=True,
                 shadows=True, render_chunk=None, plane_size=(3.0, 3.0), light_color=(300.0, 300.0, 300.0),
                 ambient=(0.05, 0.05, 0.05), manual_exposure=-1.0, scene_id_base=0, pair_contact_budget=SB.PAIR_CONTACT_BUDGET,
                 environment=None, p_light_map=1.0, p_background=1.0, p_plane_texture=1.0, env_ids=None):
        from .scene import Scene

        if not 1 <= n_objects <= 64:      # SLHIP_SYNTH_MAX_OBJECTS: the synthesis kernels map an object to a lane of one wave
            raise ValueError("n_objects must be in [1, 64]")
        self.table, self.eng, self.se = table, table.eng, table.se
        self.n_scenes, self.n_objects = int(n_scenes), int(n_objects)
        self.resolution = tuple(resolution)
        self._proto = Scene(self.resolution)                 # projection bookkeeping of sl.Scene (scene.cpp:222-271)
        distinct = asset_ids is None
        if distinct and len(table) < n_objects:
            raise ValueError("drawing %d distinct classes needs an asset table of at least that size" % n_objects)
        self.asset_ids = None
        if asset_ids is not None:
            ids = np.ascontiguousarray(asset_ids, dtype=np.uint16).reshape(self.n_scenes, self.n_objects)
            if ids.max(initial=0) >= len(table):
                raise ValueError("asset id out of range")
            self.asset_ids = ids
        has_plane = float(plane_size[0]) ** 2 + float(plane_size[1]) ** 2 > 0
        p = np.zeros((), dtype=_abi.SYNTH_PARAMS_DTYPE)
        p["n_scenes"], p["n_objects"], p["n_assets"] = self.n_scenes, self.n_objects, len(table)
        p["flags"] = ((_abi.SYNTH_SAMPLE_DISTINCT if distinct else 0) | (_abi.SYNTH_RANDOM_PBR if random_pbr else 0)
                      | (_abi.SYNTH_SHADOWS if shadows else 0))
        p["seed_lo"], p["seed_hi"] = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
        p["scene_id_base"] = scene_id_base
        p["render_chunk"] = self.n_scenes if render_chunk is None else int(render_chunk)
        p["max_draws_per_scene"] = table.bound(table.n_draws, n_objects, distinct) + (1 if has_plane else 0)
        p["max_chunks_per_scene"] = table.bound(table.n_chunks, n_objects, distinct) + (1 if has_plane else 0)
        p["max_clip_verts_per_scene"] = table.bound(table.n_clip, n_objects, distinct) + (4 if has_plane else 0)
        p["plane_z"] = PLANE_HALF_Z
        p["plane_size"] = plane_size
        p["manual_exposure"] = manual_exposure
        p["light_color"][:3] = light_color
        p["ambient"][:3] = ambient
        self.params = p
        self.shadows = bool(shadows)
        self._set_projection()
        # settle parameters with the sizing hints of the WORST scene the table can produce (no read-back)
        sp = SB.default_params(tabletop=True, pair_contact_budget=int(pair_contact_budget))   # (0: every point, as in PhysX; > 0: the compound manifold reduction of slhip.h)
        sp["max_bodies_per_scene"] = self.n_objects
        sp["max_hulls_per_scene"] = table.bound(table.n_hulls, n_objects, distinct)
        sp["max_hull_verts_per_scene"] = table.bound(table.n_hull_verts, n_objects, distinct)
        # list capacities of the scratch: no scene may lose a hull pair or a contact (settle_caps() says if one did).  The bound on
        # the pairs is what the table's hull counts allow, capped where 16384 scenes of the 21 YCB-like classes never got (the most
        # ever seen: 3 168 candidate pairs in a step -- mug in bowl on banana; 664 contacts with the default pair_contact_budget)
        h = int(sp["max_hulls_per_scene"])
        sp["max_hull_pairs_per_scene"] = max(64, min(4096, h * h // 2))
        # (32768 C2 scenes: at most 2 191 contacts in a step with every point in the solver, 543 with a pair budget of 32)
        sp["max_contacts_per_scene"] = 4096 if int(pair_contact_budget) == 0 else 1024
        for key, env in (("max_hull_pairs_per_scene", "SLHIP_PAIR_CAP"), ("max_contacts_per_scene", "SLHIP_CONTACT_CAP"),
                         ("pair_contact_budget", "SLHIP_PAIR_BUDGET")):      # developer knobs (tools/probes)
            if os.environ.get(env):
                sp[key] = int(os.environ[env])
        self.settle_params = sp
        dev = self.eng.device
        nb = self.n_scenes * self.n_objects

        def buf(n):
            return torch.empty(max(16, int(n)), dtype=torch.uint8, device=dev)

        self.d_bodies = buf(nb * SB.BODY_DTYPE.itemsize)
        self.d_settle_scenes = buf(self.n_scenes * SB.SETTLE_SCENE_DTYPE.itemsize)
        self.d_objects = buf(nb * _abi.SYNTH_OBJECT_DTYPE.itemsize)
        self.d_scenes = buf(self.n_scenes * _abi.SYNTH_SCENE_DTYPE.itemsize)
        self.d_srec = buf(self.n_scenes * _abi.SCENE_DTYPE.itemsize)
        self.d_drec = buf(self.n_scenes * int(p["max_draws_per_scene"]) * _abi.DRAW_DTYPE.itemsize)
        self.d_crec = buf(self.n_scenes * int(p["max_chunks_per_scene"]) * _abi.CHUNK_DTYPE.itemsize)
        self.d_asset_ids = None if self.asset_ids is None else torch.from_numpy(self.asset_ids.view(np.int16).copy()).to(dev)
        # environment bank (slhip_synth_place_env)
        self.environment, self.env_ids, self.d_env_ids, self.d_env_out = environment, None, None, None
        if environment is None:
            if env_ids is not None:
                raise ValueError("env_ids needs an environment bank")
        else:
            if environment.eng is not self.eng:
                raise ValueError("the environment bank and the asset table must live on the same device engine")
            counts = environment.counts()
            probs = [float(p_light_map), float(p_background), float(p_plane_texture)]
            for name, pr in zip(("p_light_map", "p_background", "p_plane_texture"), probs):
                if not 0.0 <= pr <= 1.0:             # (false for NaN)
                    raise ValueError("%s must be in [0, 1]" % name)
            self.env_probs = tuple(pr if n else 0.0 for pr, n in zip(probs, counts))
            if env_ids is not None:
                ids = np.ascontiguousarray(env_ids, dtype=np.int32).reshape(self.n_scenes, 3)
                if (ids < -1).any() or (ids >= np.array(counts, np.int32)[None, :]).any():
                    raise ValueError("environment id out of range")
                self.env_ids = ids
                self.d_env_ids = torch.from_numpy(ids.copy()).to(dev)
            self.d_env_out = torch.full((self.n_scenes, 3), -1, dtype=torch.int32, device=dev)
        self.view, self.object_to_camera, self._view_keep = 0, None, None      # place(view=...)
        self._object_to_camera_placed = False      # object_to_camera belongs to the view last placed (keypoints())

    # ---- camera (shared by all scenes of the batch; sl.Scene's setters) --------------------------------------
    def _set_projection(self):
        P = self._proto._projection.astype(np.float32)
        self.params["proj"] = P.reshape(-1)
        self.params["proj_inv"] = np.linalg.inv(P.astype(np.float64)).astype(np.float32).reshape(-1)   # render_pass.cpp:73

    def set_camera_intrinsics(self, fx, fy, cx, cy):
        self._proto.set_camera_intrinsics(fx, fy, cx, cy)
        self._set_projection()

    def set_camera_hfov(self, hfov):
        self._proto.set_camera_hfov(hfov)
        self._set_projection()

    # ---- the four steps -----------------------------------------------------------------------------------------
    def _p(self):
        self._prm = np.array(self.params)       # kept alive: the launch copies it by value
        return C.c_void_p(self._prm.ctypes.data)

    @staticmethod
    def _a(t):
        return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)

    def stage(self, scene_id_base=None):
        """Tabletop set-up of every scene (scene.cpp:612-678) on the current stream."""
        if scene_id_base is not None:
            self.params["scene_id_base"] = scene_id_base
        d_assets, _ = self.table.device()
        self.se.hulls_dev()
        stream = torch.cuda.current_stream(self.eng.device).cuda_stream
        with torch.cuda.device(self.eng.device):
            st = self.eng.L.slhip_synth_stage(self._p(), self._a(d_assets), self._a(self.d_asset_ids), self._a(self.d_bodies),
                                              self._a(self.d_settle_scenes), self._a(self.d_objects), self._a(self.d_scenes),
                                              C.c_void_p(stream))
        _abi.check(st, "slhip_synth_stage")

    def settle(self, frames=None):
        """slhip_settle of the whole batch (scene.cpp:720-756) on the current stream."""
        eng, se = self.eng, self.se
        d_hulls, d_verts = se.hulls_dev()
        prm = self.settle_params if frames is None else self.settle_params.copy()
        if frames is not None:
            prm["frames"] = frames
        prm = np.ascontiguousarray(prm)
        stream = torch.cuda.current_stream(eng.device).cuda_stream
        scratch = se.scratch(self.n_scenes, stream, prm)
        with torch.cuda.device(eng.device):
            st = eng.L.slhip_settle(self._a(self.d_settle_scenes), self.n_scenes, self._a(self.d_bodies), self._a(d_hulls),
                                    self._a(d_verts), C.c_void_p(prm.ctypes.data), self._a(scratch), scratch.numel(),
                                    C.c_void_p(stream))
        _abi.check(st, "slhip_settle")
        self._settle_keep = prm
        self._settle_stream = stream

    def check_settled(self):
        """Synchronises the settle stream; raises if the kernel refused a scene (sizing hints) or if a step of some scene offered
        more hull pairs / contacts / body pairs than the lists of the scratch hold (slhip.h: nothing is ever dropped silently --
        the reference has no caps, scene.cpp:738-739).  A caller that gets the second error settles again with larger
        `settle_params` capacities (the batch is staged from counters, so stage() + settle() reproduce it)."""
        self.se.check_status(self.n_scenes, self._settle_stream)
        caps = self.settle_caps()
        if caps["scenes_dropped"]:
            raise RuntimeError("SceneBatch.settle: %d scene(s) lost hull pairs / contacts / body pairs to the list capacities "
                               "(max_hull_pairs_per_scene %d, max_contacts_per_scene %d; the most a step offered: %d / %d): raise "
                               "them in settle_params and settle again (%r)"
                               % (caps["scenes_dropped"], int(self._settle_keep["max_hull_pairs_per_scene"]),
                                  int(self._settle_keep["max_contacts_per_scene"]), caps["max_hull_pairs"], caps["max_contacts"], caps))

    def settle_caps(self):
        """What the list capacities cost the last settle() (slhip_settle_caps, SettleEngine.caps; synchronises the settle stream)."""
        return self.se.caps(self.n_scenes, self._settle_stream, self._settle_keep)

    def _env(self):
        d_ls, d_bg, d_pt = self.environment.device()
        e = _abi.SynthEnv()
        e.d_light_sets, e.d_backgrounds, e.d_plane_textures = d_ls.data_ptr(), d_bg.data_ptr(), d_pt.data_ptr()
        e.d_env_ids = self.d_env_ids.data_ptr() if self.d_env_ids is not None else None
        e.n_light_sets, e.n_backgrounds, e.n_plane_textures = self.environment.counts()
        e.p_light_map, e.p_background, e.p_plane_texture = self.env_probs
        return e

    def place(self, view=0, camera_poses=None, object_to_camera=False):
        """Camera pose, light direction, shadow matrix and the render records of every scene; with an environment bank also
        every scene's light map / background image / plane texture and the shadow matrices of all its lights.

        A view is another camera on the SAME physical scene: poses, world-space lights, environment and every draw / chunk
        record keep their bits, only the camera and what hangs on it (world_to_cam, cam_position, the shadow matrices,
        camera_pose of the scene records) are the view's.  `view` = 0 is the batch's camera; `view` = v >= 1 draws azimuth
        and elevation as view 0 does, from the Philox key of view v (include/slhip.h, "Randomness"), and fits the camera to
        the pile the same way.  `camera_poses`: a float32 device tensor [n_scenes, 4, 4] of camera-to-world matrices taken
        as they are (no draw, no fit; `view` only names them); a pose with a non-finite entry leaves that scene empty.
        `object_to_camera`: also keep world_to_cam * pose of every object, float32 [n_scenes, n_objects, 3, 4], in
        `batch.object_to_camera` (sl.bop.scene_gt_entries).  The records are overwritten in place: a view costs no memory."""
        check_view_arguments(view, camera_poses, self.n_scenes, self.eng.device)
        d_assets, d_templates = self.table.device()
        stream = torch.cuda.current_stream(self.eng.device).cuda_stream
        if view != 0 or camera_poses is not None or object_to_camera:
            v = _abi.SynthView()
            v.view = int(view)
            v.d_camera_poses = camera_poses.data_ptr() if camera_poses is not None else None
            if object_to_camera:
                if self.object_to_camera is None:
                    self.object_to_camera = torch.empty((self.n_scenes, self.n_objects, 3, 4), dtype=torch.float32,
                                                        device=self.eng.device)
                v.d_object_to_camera = self.object_to_camera.data_ptr()
            e = self._env() if self.environment is not None else None
            with torch.cuda.device(self.eng.device):
                st = self.eng.L.slhip_synth_place_view(self._p(), C.byref(e) if e is not None else None, C.byref(v),
                                                       self._a(d_assets), self._a(d_templates), self._a(self.d_bodies),
                                                       self._a(self.d_objects), self._a(self.d_scenes), self._a(self.d_srec),
                                                       self._a(self.d_drec), self._a(self.d_crec), self._a(self.d_env_out),
                                                       C.c_void_p(stream))
            _abi.check(st, "slhip_synth_place_view")
            self._view_keep = camera_poses          # alive until the next place(): the launch reads it on the stream
        elif self.environment is not None:
            e = self._env()
            with torch.cuda.device(self.eng.device):
                st = self.eng.L.slhip_synth_place_env(self._p(), C.byref(e), self._a(d_assets), self._a(d_templates),
                                                      self._a(self.d_bodies), self._a(self.d_objects), self._a(self.d_scenes),
                                                      self._a(self.d_srec), self._a(self.d_drec), self._a(self.d_crec),
                                                      self._a(self.d_env_out), C.c_void_p(stream))
            _abi.check(st, "slhip_synth_place_env")
        else:
            with torch.cuda.device(self.eng.device):
                st = self.eng.L.slhip_synth_place(self._p(), self._a(d_assets), self._a(d_templates), self._a(self.d_bodies),
                                                  self._a(self.d_objects), self._a(self.d_scenes), self._a(self.d_srec),
                                                  self._a(self.d_drec), self._a(self.d_crec), C.c_void_p(stream))
            _abi.check(st, "slhip_synth_place")
        self.view = int(view)
        self._object_to_camera_placed = bool(object_to_camera)

    def views(self, n, mask=_abi.OUT_GT6, ssao=True, object_stats=False, object_to_camera=False, object_masks=False):
        """n pictures of every scene: places view v = 0 .. n - 1 in turn and yields (v, chunk, buffers) for every render chunk
        of it, view-major.  The records of a view are gone once the next one is placed: read what is needed of them
        (host_cameras(), object_to_camera) while the view's items are being consumed."""
        for v in range(int(n)):
            self.place(view=v, object_to_camera=object_to_camera)
            for c in range(self.n_render_chunks()):
                yield v, c, self.render(c, mask, ssao, object_stats=object_stats, object_masks=object_masks)

    @property
    def render_chunk(self):
        return int(self.params["render_chunk"])

    def n_render_chunks(self):
        return (self.n_scenes + self.render_chunk - 1) // self.render_chunk

    def render(self, chunk=0, mask=_abi.OUT_GT6, ssao=True, buffers=None, object_stats=False, object_masks=False):
        """slhip_render of render chunk `chunk` (scenes [chunk * render_chunk, ...)) on the current stream.  `object_stats`: also
        the per-object visibility statistics (the returned buffers' .object_stats; slot i = object i - 1 of a scene).
        `object_masks`: the statistics and the per-object masks (.object_masks, an ObjectMasks; the same slots)."""
        rc = self.render_chunk
        s0 = chunk * rc
        B = min(rc, self.n_scenes - s0)
        if B <= 0:
            raise IndexError("render chunk %d out of range" % chunk)
        md, mk, mv = (int(self.params[k]) for k in ("max_draws_per_scene", "max_chunks_per_scene", "max_clip_verts_per_scene"))
        W, H = self.resolution
        self.eng.pool_abi()
        return self.eng.render_device(
            self.d_srec.data_ptr() + s0 * _abi.SCENE_DTYPE.itemsize,
            self.d_drec.data_ptr() + s0 * md * _abi.DRAW_DTYPE.itemsize,
            self.d_crec.data_ptr() + s0 * mk * _abi.CHUNK_DTYPE.itemsize,
            B, B * md, B * mk, B * mv, W, H, mask, ssao=ssao, shadows=self.shadows, buffers=buffers,
            # the synthesised scenes have one light, or as many as the largest light set of the bank (k_synth_place)
            shadow_lights=1 if self.environment is None else max(1, self.environment.max_lights),
            object_stats=object_stats, n_slots=self.n_objects + 1,   # instance index = object + 1 (k_synth_place)
            object_masks=object_masks)

    def render_chunks(self, mask=_abi.OUT_GT6, ssao=True, object_stats=False, object_masks=False):
        for c in range(self.n_render_chunks()):
            yield self.render(c, mask, ssao, object_stats=object_stats, object_masks=object_masks)

    def intrinsics(self):
        """(fx, fy, cx, cy) of the batch's camera, read back from its projection (Scene.set_camera_intrinsics' convention)."""
        P = self._proto._projection.astype(np.float64)
        W, H = (float(v) for v in self.resolution)
        return (P[0, 0] * W / 2.0, P[1, 1] * H / 2.0, (P[0, 2] + 1.0) * W / 2.0, (P[1, 2] + 1.0) * H / 2.0)

    def _chunk_range(self, chunk, held=None):
        """(first scene, scenes) of render chunk `chunk`.  `held`: the scenes that a caller's buffers hold, which must cover it."""
        s0 = int(chunk) * self.render_chunk
        B = min(self.render_chunk, self.n_scenes - s0)
        if B <= 0 or (held is not None and held < B):
            raise IndexError("render chunk %d out of range%s" % (chunk, ", or `buffers` holds fewer scenes than it" if held is not None else ""))
        return s0, B

    def _extract(self, what, extract, buffers, chunk, kw):
        """`extract` (sl.object_crops.extract, sl.object_points.extract) with the batch's intrinsics, the chunk's scene ids and
        the key of the view last placed; scene_global and object_to_camera attached to the result"""
        for name in ("intrinsics", "seed", "scene_id_base"):
            if name in kw:
                raise TypeError("SceneBatch.%s sets `%s` itself" % (what, name))
        s0 = int(chunk) * self.render_chunk
        key = _abi.view_key(int(self.params["seed_lo"]), int(self.params["seed_hi"]), self.view)
        out = extract(buffers, self.intrinsics(), seed=key, scene_id_base=int(self.params["scene_id_base"]) + s0, **kw)
        out.scene_global = out.scene + s0
        if self.object_to_camera is not None:
            out.object_to_camera = self.object_to_camera[out.scene_global.long(), (out.slot - 1).long()]
        return out

    def crops(self, buffers, chunk=0, **kw):
        """sl.object_crops.extract on the render of chunk `chunk` (`buffers` = what render(chunk, object_stats=True) or
        render(chunk, object_masks=True) returned) with the batch's intrinsics, the scene ids of the chunk and the Philox key
        of the view last placed -- every view of a pile gets its own jitter.  The result also carries `scene_global`
        (= scene + chunk * render_chunk) and, when place(object_to_camera=True) keeps it, `object_to_camera` [n, 3, 4] of every
        crop's object.  `kw`: the other arguments of extract (size, box, pad, jitter_scale, jitter_shift, ...)."""
        from . import object_crops

        return self._extract("crops", object_crops.extract, buffers, chunk, kw)

    def points(self, buffers, chunk=0, **kw):
        """sl.object_points.extract on the render of chunk `chunk` (`buffers` = what render(chunk, object_masks=True) returned)
        with the batch's intrinsics, the scene ids of the chunk and the Philox key of the view last placed -- every view of a
        pile gets its own draw.  The result also carries `scene_global` (= scene + chunk * render_chunk) and, when
        place(object_to_camera=True) keeps it, `object_to_camera` [n, 3, 4] of every set's object.  `kw`: the other arguments
        of extract (n_points, min_px, min_visib_fract, outputs, depth)."""
        from . import object_points

        return self._extract("points", object_points.extract, buffers, chunk, kw)

    def keypoints(self, buffers, chunk=0, bank=None, depth=None, **kw):
        """sl.object_keypoints.project for the render of chunk `chunk` (`buffers` = what render(chunk, ...) returned; only its
        size is used) with the batch's intrinsics, its object records and the chunk's slice of `object_to_camera`: an
        ObjectKeypoints whose scene b is scene b of the chunk.  `bank`: a KeypointBank of the batch's table
        (sl.object_keypoints.bank(table, ...)) or a [A, Kp, 4] tensor.  `depth`: a float32 [B, H, W] plane, or True for the
        ideal depth (the w of buffers.coord): enables the `unoccluded` flag.  `kw`: depth_tol.  Needs
        place(object_to_camera=True) for the view last placed: the keypoints are projected with that camera."""
        from . import object_keypoints

        for name in ("intrinsics", "size", "object_to_camera", "objects"):
            if name in kw:
                raise TypeError("SceneBatch.keypoints sets `%s` itself" % name)
        if bank is None:
            raise TypeError("SceneBatch.keypoints needs a bank (sl.object_keypoints.bank(table, ...))")
        if self.object_to_camera is None or not self._object_to_camera_placed:
            raise RuntimeError("SceneBatch.keypoints needs object_to_camera of the view last placed: call "
                               "place(object_to_camera=True) (the last place() did not keep it)")
        s0, B = self._chunk_range(chunk)
        if depth is True:
            depth = buffers.coord
            if depth is None:
                raise RuntimeError("object_keypoints: the `coord` target was not rendered, and depth=True reads it")
        nb = self.n_objects * _abi.SYNTH_OBJECT_DTYPE.itemsize
        out = object_keypoints.project(self.object_to_camera[s0:s0 + B], self.d_objects[s0 * nb:(s0 + B) * nb], bank,
                                       self.intrinsics(), self.resolution, depth=depth, **kw)
        out.scene0 = s0      # scene b of the result is scene s0 + b of the batch (offsets() pairs it with points.scene_global)
        return out

    def regions(self, buffers, chunk=0, bank=None, **kw):
        """sl.object_regions.label for the render of chunk `chunk` (`buffers` = what render(chunk, ...) returned, with the
        `instance` and `coord` targets) with the batch's object records, read in place: an ObjectRegions whose picture b is
        scene b of the chunk.  `bank`: a RegionBank of the batch's table (sl.object_regions.bank(table, ...)) or a [A, R, 4]
        tensor.  `kw`: local, histogram."""
        from . import object_regions

        for name in ("classes", "n_objects"):
            if name in kw:
                raise TypeError("SceneBatch.regions sets `%s` itself" % name)
        if bank is None:
            raise TypeError("SceneBatch.regions needs a bank (sl.object_regions.bank(table, ...))")
        if buffers.instance is None or buffers.coord is None:
            raise RuntimeError("object_regions: the `instance` and `coord` targets were not rendered")
        s0, B = self._chunk_range(chunk, int(buffers.instance.shape[0]))
        nb = self.n_objects * _abi.SYNTH_OBJECT_DTYPE.itemsize
        return object_regions.label(buffers.instance[:B], buffers.coord[:B], self.d_objects[s0 * nb:(s0 + B) * nb], bank,
                                    n_objects=self.n_objects, **kw)

    def view_state(self):
        """What flow() needs of the view last placed once another one is placed or the pile is settled further: an
        sl.render_flow.ViewState with clones of `object_to_camera` [n_scenes, O, 3, 4] and of rows 0-2 of every scene's
        world_to_cam [n_scenes, 3, 4], read from the scene records on the device (no host round trip).  Needs
        place(object_to_camera=True) for the view last placed.  Asynchronous on the current stream."""
        from . import render_flow

        if self.object_to_camera is None or not self._object_to_camera_placed:
            raise RuntimeError("SceneBatch.view_state needs object_to_camera of the view last placed: call "
                               "place(object_to_camera=True) (the last place() did not keep it)")
        size, at = _abi.SCENE_DTYPE.itemsize, _abi.SCENE_DTYPE.fields["world_to_cam"][1]
        rec = self.d_srec[:self.n_scenes * size].view(self.n_scenes, size)
        w2c = rec[:, at:at + 48].contiguous().view(torch.float32).view(self.n_scenes, 3, 4)      # (contiguous(): the clone)
        return render_flow.ViewState(self.object_to_camera.clone(), w2c, self.view)

    def flow(self, buffers_a, state_a, buffers_b=None, state_b=None, chunk=0, **kw):
        """sl.render_flow.compute from the render `buffers_a` of chunk `chunk` under the view `state_a` (a view_state()) to
        the render `buffers_b` of the same chunk under `state_b` -- None: the view now placed -- with the batch's intrinsics:
        a RenderFlow whose picture b is scene b of the chunk.  The motion table [B, O + 1, 3, 4] is built on the device:
        slot 0 = motion(world_to_cam of a, of b), the plane and the background; slot o + 1 = motion(object_to_camera[o] of
        a, of b).  It serves another camera on the same pile and equally the same camera after the pile was settled further
        (place() again after settle()).  Both renders need the `coord` and `instance` targets; without `buffers_b` nothing
        is `visible`.  `kw`: the other arguments of compute (max_depth, depth_tol, depth_rel, match_instance, outputs)."""
        from . import render_flow

        for name in ("intrinsics", "motion"):
            if name in kw:
                raise TypeError("SceneBatch.flow sets `%s` itself" % name)
        if state_b is None:
            state_b = self.view_state()
        for buffers in (buffers_a,) + (() if buffers_b is None else (buffers_b,)):
            if buffers.instance is None or buffers.coord is None:
                raise RuntimeError("render_flow: the `instance` and `coord` targets were not rendered")
        held = min(int(b.instance.shape[0]) for b in (buffers_a, buffers_b) if b is not None)
        s0, B = self._chunk_range(chunk, held)
        table = torch.cat([render_flow.motion(state_a.world_to_cam[s0:s0 + B], state_b.world_to_cam[s0:s0 + B])[:, None],
                           render_flow.motion(state_a.object_to_camera[s0:s0 + B], state_b.object_to_camera[s0:s0 + B])], dim=1)
        b_planes = (None, None) if buffers_b is None else (buffers_b.coord[:B], buffers_b.instance[:B])
        out = render_flow.compute(buffers_a.coord[:B], buffers_a.instance[:B], table, self.intrinsics(), *b_planes, **kw)
        out.scene0 = s0
        return out

    def pose_errors(self, estimates, bank, chunk=None, **kw):
        """sl.pose_error.evaluate of pose estimates against the batch's own ground truth: its `object_to_camera`, its object
        records (read in place) and its intrinsics.  `estimates`: float32 [B, O, Hy, 3, 4] or [B, O, 3, 4] for all scenes of the
        batch, or with `chunk` for the scenes of that render chunk.  `bank`: a ModelBank of the batch's table
        (sl.pose_error.bank(table, ...)).  `kw`: outputs.  Needs place(object_to_camera=True) for the view last placed."""
        from . import pose_error

        for name in ("intrinsics", "object_to_camera", "objects"):
            if name in kw:
                raise TypeError("SceneBatch.pose_errors sets `%s` itself" % name)
        if self.object_to_camera is None or not self._object_to_camera_placed:
            raise RuntimeError("SceneBatch.pose_errors needs object_to_camera of the view last placed: call "
                               "place(object_to_camera=True) (the last place() did not keep it)")
        s0, B = (0, self.n_scenes) if chunk is None else self._chunk_range(chunk)
        nb = self.n_objects * _abi.SYNTH_OBJECT_DTYPE.itemsize
        return pose_error.evaluate(self.object_to_camera[s0:s0 + B], estimates, self.d_objects[s0 * nb:(s0 + B) * nb], bank,
                                   self.intrinsics(), **kw)

    def pose_vsd(self, estimates, surface, buffers, chunk=None, **kw):
        """sl.pose_vsd.evaluate of pose estimates against the batch's own ground truth: its `object_to_camera`, its object records
        (read in place), its intrinsics, and the scene's depth from the w of `buffers.coord` (`buffers` = what render(chunk, ...)
        returned).  `estimates`: float32 [B, O, Hy, 3, 4] or [B, O, 3, 4] for the scenes of render chunk `chunk`; None: the
        buffers hold every scene of the batch.  `surface`: a SurfaceBank of the batch's table (sl.pose_vsd.surface(table)).
        `kw`: taus, delta, normalized, z_near, outputs.  Needs place(object_to_camera=True) for the view last placed."""
        from . import pose_vsd

        for name in ("intrinsics", "object_to_camera", "objects", "depth"):
            if name in kw:
                raise TypeError("SceneBatch.pose_vsd sets `%s` itself" % name)
        if self.object_to_camera is None or not self._object_to_camera_placed:
            raise RuntimeError("SceneBatch.pose_vsd needs object_to_camera of the view last placed: call "
                               "place(object_to_camera=True) (the last place() did not keep it)")
        if buffers.coord is None:
            raise RuntimeError("pose_vsd: the `coord` target was not rendered, and the scene's depth is its w")
        held = int(buffers.coord.shape[0])
        s0, B = (0, self.n_scenes) if chunk is None else self._chunk_range(chunk, held)
        if held < B:
            raise ValueError("pose_vsd: the buffers hold %d scenes, the estimates are for %d" % (held, B))
        nb = self.n_objects * _abi.SYNTH_OBJECT_DTYPE.itemsize
        return pose_vsd.evaluate(self.object_to_camera[s0:s0 + B], estimates, self.d_objects[s0 * nb:(s0 + B) * nb], surface,
                                 buffers.coord[:B], self.intrinsics(), **kw)

    def pose_pnp(self, points, coord=None, **kw):
        """sl.pose_pnp.solve on the point sets of a render (`points` = what points(...) returned, with its `pixel` and `coord`
        outputs) with the batch's intrinsics, the Philox key of the view last placed and the first scene id of the batch as the
        set id base: a PosePnP with one pose per set.  `coord`: float32 [n, K, 4] coordinates that replace the rendered ones
        (a network's prediction; a correspondence counts when its w > 0).  `kw`: n_hypotheses, threshold_px, refine_iters,
        min_inliers, outputs, init.  pose_pnp(...).dense(B, O, points.scene_global, points.slot) is the [B, O, 3, 4] that
        pose_errors and pose_vsd take."""
        from . import pose_pnp

        for name in ("intrinsics", "seed", "set_id_base", "xyz", "per_set_intrinsics"):
            if name in kw:
                raise TypeError("SceneBatch.pose_pnp sets `%s` itself" % name)
        key = _abi.view_key(int(self.params["seed_lo"]), int(self.params["seed_hi"]), self.view)
        return pose_pnp.solve(points, coord=coord, intrinsics=self.intrinsics(), seed=key,
                              set_id_base=int(self.params["scene_id_base"]), **kw)

    def keypoint_votes(self, points, field, scenes=None, **kw):
        """sl.keypoint_vote.vote on the point sets of a render (`points` = what points(...) returned, with its `pixel` output)
        and a predicted vector field float32 [count, H, W, Kp, 2] in the layout of ObjectKeypoints.field, with the Philox key
        of the view last placed and the first scene id of the batch as the set id base: a KeypointVotes with one position per
        (set, keypoint).  `scenes`: the (first, count) the field was made for -- picture 0 of the field is scene `first` of the
        points' render chunk; default: the field starts at the chunk's first scene.  The result carries the class of every
        set's object from the batch's object records, so votes.correspondences(bank) is what pose_pnp takes.  `kw`:
        n_hypotheses, inlier_cos, min_inliers, min_sin, outputs."""
        from . import keypoint_vote

        for name in ("seed", "set_id_base", "scene", "vectors", "size"):
            if name in kw:
                raise TypeError("SceneBatch.keypoint_votes sets `%s` itself" % name)
        if points.pixel is None:
            raise RuntimeError("keypoint_vote: the ObjectPoints need their `pixel` output")
        first = 0 if scenes is None else int(scenes[0])
        key = _abi.view_key(int(self.params["seed_lo"]), int(self.params["seed_hi"]), self.view)
        out = keypoint_vote.vote(points, field=field, scene=points.scene - first, seed=key,
                                 set_id_base=int(self.params["scene_id_base"]), **kw)
        if points.scene_global is not None:
            nb = self.n_scenes * self.n_objects * _abi.SYNTH_OBJECT_DTYPE.itemsize
            asset = self.d_objects[:nb].view(torch.int32).view(self.n_scenes, self.n_objects, -1)[..., 0]
            out.classes = asset[points.scene_global.long(), (points.slot - 1).long()]
        return out

    def keypoint_votes3d(self, points, offsets, **kw):
        """sl.keypoint_vote3d.vote on the point sets of a render (`points` = what points(...) returned, with its `camera`
        output) and predicted offsets float32 [n, K, Kp, 3] in the layout of ObjectKeypoints.offsets: a KeypointVotes3D with one
        camera-frame position per (set, keypoint).  The result carries the class of every set's object from the batch's object
        records, so pose_fit(votes3, bank=bank) has what it needs.  `kw`: n_seeds, bandwidth, max_iters, tol, min_support,
        outputs."""
        from . import keypoint_vote3d

        if "classes" in kw:
            raise TypeError("SceneBatch.keypoint_votes3d sets `classes` itself")
        if getattr(points, "camera", None) is None:
            raise RuntimeError("keypoint_vote3d: the ObjectPoints need their `camera` output")
        out = keypoint_vote3d.vote(points, offsets, **kw)
        if points.scene_global is not None:
            nb = self.n_scenes * self.n_objects * _abi.SYNTH_OBJECT_DTYPE.itemsize
            asset = self.d_objects[:nb].view(torch.int32).view(self.n_scenes, self.n_objects, -1)[..., 0]
            out.classes = asset[points.scene_global.long(), (points.slot - 1).long()]
        return out

    def pose_fit(self, src, dst=None, bank=None, **kw):
        """sl.pose_fit.solve: a PoseFit with one pose (object to camera) per set.  Either a pair of float32 [n, N, 4] tensors --
        pose_fit(points.coord, points.camera) fits predicted or rendered object coordinates to the camera points -- or a
        KeypointVotes3D with `bank=` (a KeypointBank or a float32 [A, Kp, 4] tensor): the bank's keypoints of every set's class
        onto the voted ones, the PVN3D pose.  `kw`: min_gap, outputs.  pose_fit(...).dense(B, O, points.scene_global,
        points.slot) is the [B, O, 3, 4] that pose_errors and pose_vsd take."""
        from . import keypoint_vote3d, pose_fit

        if isinstance(src, keypoint_vote3d.KeypointVotes3D):
            if dst is not None or bank is None:
                raise TypeError("SceneBatch.pose_fit takes a KeypointVotes3D with `bank=` and without `dst`")
            src, dst = src.correspondences(bank)
        elif bank is not None or dst is None:
            raise TypeError("SceneBatch.pose_fit takes either (src, dst) tensors or a KeypointVotes3D with `bank=`")
        return pose_fit.solve(src, dst, **kw)

    def pose_align(self, src, dst=None, bank=None, coord=None, **kw):
        """sl.pose_align.solve with the Philox key of the view last placed and the first scene id of the batch as the set id
        base: a PoseAlign with one pose (object to camera) per set, the one with the most inliers, refitted on them.  Either an
        ObjectPoints with its `coord` and `camera` outputs (`coord=`: float32 [n, K, 4] coordinates that replace the rendered
        ones, a network's prediction), or a KeypointVotes3D with `bank=` (a KeypointBank or a float32 [A, Kp, 4] tensor: the
        bank's keypoints of every set's class onto the voted ones), or a pair of float32 [n, K, 4] tensors.  `kw`: threshold
        (required, in the unit of the points), n_hypotheses, refine_iters, min_gap, min_inliers, outputs, init.
        pose_align(...).dense(B, O, points.scene_global, points.slot) is the [B, O, 3, 4] that pose_errors and pose_vsd take."""
        from . import keypoint_vote3d, pose_align

        for name in ("seed", "set_id_base"):
            if name in kw:
                raise TypeError("SceneBatch.pose_align sets `%s` itself" % name)
        if isinstance(src, keypoint_vote3d.KeypointVotes3D):
            if dst is not None or bank is None or coord is not None:
                raise TypeError("SceneBatch.pose_align takes a KeypointVotes3D with `bank=` and without `dst` and `coord`")
            src, dst = src.correspondences(bank)
        elif bank is not None:
            raise TypeError("SceneBatch.pose_align takes an ObjectPoints, (src, dst) tensors or a KeypointVotes3D with `bank=`")
        key = _abi.view_key(int(self.params["seed_lo"]), int(self.params["seed_hi"]), self.view)
        return pose_align.solve(src, dst, coord=coord, seed=key, set_id_base=int(self.params["scene_id_base"]), **kw)

    def pose_icp(self, points, init, bank, **kw):
        """sl.pose_icp.solve on the point sets of a render (`points` = what points(...) returned, with its `camera` output): a
        PoseICP with one refined pose (object to camera) per set.  `init`: the initial poses as float32 [n, 3, 4], a PoseFit,
        PoseAlign or PosePnP (its `.pose`), or float32 [B, O, 3, 4] for all scenes of the batch, gathered by points.scene_global and
        points.slot.  `bank`: a ModelBank of the batch's table (sl.pose_error.bank(table, ...); surface-sampled points from
        sl.pose_icp.surface_points serve low-poly classes).  The class of every set's object comes from the batch's object
        records.  `kw`: max_iters, max_dist, dist_scale, min_dist, min_pairs, min_gap, tol_rot, tol_trans, outputs.
        pose_icp(...).dense(B, O, points.scene_global, points.slot) is the [B, O, 3, 4] that pose_errors and pose_vsd take."""
        from . import _device, pose_icp

        if "classes" in kw:
            raise TypeError("SceneBatch.pose_icp sets `classes` itself")
        if getattr(points, "camera", None) is None:
            raise RuntimeError("pose_icp: the ObjectPoints need their `camera` output")
        if points.scene_global is None:
            raise RuntimeError("pose_icp: the ObjectPoints carry no scene_global (they do not come from this batch's points())")
        if not isinstance(init, torch.Tensor):
            init = getattr(init, "pose", None)
            if init is None:
                raise TypeError("SceneBatch.pose_icp: `init` must be a tensor, or a PoseFit / PoseAlign / PosePnP with its `pose` output")
        scene, slot = points.scene_global.long(), (points.slot - 1).long()
        if init.dim() == 4:
            if not init.is_cuda:
                raise _abi.SlhipError(_device.no_cpu("pose_icp"))
            init = init[scene, slot]
        nb = self.n_scenes * self.n_objects * _abi.SYNTH_OBJECT_DTYPE.itemsize
        asset = self.d_objects[:nb].view(torch.int32).view(self.n_scenes, self.n_objects, -1)[..., 0]
        if not init.is_cuda or not points.camera.is_cuda:
            raise _abi.SlhipError(_device.no_cpu("pose_icp"))
        return pose_icp.solve(points.camera, init.contiguous(), asset[scene, slot].contiguous(), bank, **kw)

    def point_graph(self, points, k=16, space="camera", **kw):
        """sl.point_knn on the point sets of a render (`points` = what points(...) returned): the k nearest points of every
        point within its own set, in the camera frame (`space="camera"`, the `camera` output) or the object frame
        (`space="coord"`, the `coord` output).  Without `ratios=` a PointNeighbours (sl.point_knn.search; `kw`: max_dist,
        skip_same, n_queries, n_refs, outputs); with `ratios=` the PointPyramid of every set (sl.point_knn.pyramid; `kw`:
        ratios, interp).  A padded point (w == 0) has no neighbours and is nobody's neighbour."""
        from . import point_knn

        if space not in ("camera", "coord"):
            raise ValueError("point_knn: `space` must be \"camera\" or \"coord\", not %r" % (space,))
        cloud = getattr(points, space, None)
        if cloud is None:
            raise RuntimeError("point_knn: the ObjectPoints need their `%s` output" % space)
        if "ratios" in kw:
            return point_knn.pyramid(cloud, k=k, **kw)
        return point_knn.search(cloud, k=k, **kw)

    # ---- host views (tests, inspection, hand-over to the per-scene API) ---------------------------------------
    def _host(self, t, dtype, count):
        return np.frombuffer(t.cpu().numpy().tobytes()[:count * dtype.itemsize], dtype=dtype).copy()

    def host_bodies(self):
        return self._host(self.d_bodies, SB.BODY_DTYPE, self.n_scenes * self.n_objects)

    def host_settle_scenes(self):
        return self._host(self.d_settle_scenes, SB.SETTLE_SCENE_DTYPE, self.n_scenes)

    def host_objects(self):
        return self._host(self.d_objects, _abi.SYNTH_OBJECT_DTYPE, self.n_scenes * self.n_objects)

    def host_scenes(self):
        return self._host(self.d_scenes, _abi.SYNTH_SCENE_DTYPE, self.n_scenes)

    def host_render_records(self):
        md, mk = int(self.params["max_draws_per_scene"]), int(self.params["max_chunks_per_scene"])
        return (self._host(self.d_srec, _abi.SCENE_DTYPE, self.n_scenes),
                self._host(self.d_drec, _abi.DRAW_DTYPE, self.n_scenes * md),
                self._host(self.d_crec, _abi.CHUNK_DTYPE, self.n_scenes * mk))

    def host_cameras(self):
        """[n_scenes, 4, 4] float32: camera-to-world of every scene in the view last placed (Scene.camera_pose)."""
        return self.host_scenes()["camera_pose"].reshape(self.n_scenes, 4, 4).copy()

    def host_env(self):
        """[n_scenes, 3] int32: the (light set, background, plane texture) of the bank every scene got at place(); -1 = none."""
        if self.environment is None:
            return np.full((self.n_scenes, 3), -1, np.int32)
        return self.d_env_out.cpu().numpy().copy()

    def scene(self, index, _cache=None):
        """Scene `index` as an ordinary sl.Scene (objects, poses, velocities, camera, light, plane, and the light map /
        background image / plane texture it got from the environment bank) rebuilt from the device records -- the hand-over
        to the per-scene API (serialize, render with other settings, ...).  The camera is read from the records, so the scene
        is handed over with the camera of the view last placed (`batch.view`)."""
        from .object import Object
        from .scene import Scene

        c = _cache or {}
        bodies = c.get("bodies") if "bodies" in c else self.host_bodies()
        objs = c.get("objects") if "objects" in c else self.host_objects()
        scs = c.get("scenes") if "scenes" in c else self.host_scenes()
        srec = c.get("srec") if "srec" in c else self._host(self.d_srec, _abi.SCENE_DTYPE, self.n_scenes)
        scene = Scene(self.resolution)
        scene._projection = self._proto._projection.copy()
        for o in range(self.n_objects):
            k = index * self.n_objects + o
            obj = Object(self.table.meshes[int(objs[k]["asset"])])
            if objs[k]["metallic"] >= 0:
                obj._metallic = f32(objs[k]["metallic"])
            if objs[k]["roughness"] >= 0:
                obj._roughness = f32(objs[k]["roughness"])
            scene.add_object(obj)
            obj._pose = bodies[k]["pose"].reshape(4, 4).copy()
            obj._linear_velocity = bodies[k]["lin_vel"][:3].copy()
            obj._angular_velocity = bodies[k]["ang_vel"][:3].copy()
            obj._separation = f32(bodies[k]["separation"])
        scene._background_plane_pose = scs[index]["plane_pose"].reshape(4, 4).copy()
        scene._background_plane_size = np.asarray(self.params["plane_size"], np.float32).copy()
        scene._camera_pose = scs[index]["camera_pose"].reshape(4, 4).copy()
        scene._light_directions[0] = torch.from_numpy(srec[index]["light_dir"][0][:3].copy())
        scene._light_colors[0] = torch.from_numpy(np.asarray(self.params["light_color"][:3], np.float32).copy())
        scene._ambient_light = np.asarray(self.params["ambient"][:3], np.float32).copy()
        scene._manual_exposure = f32(self.params["manual_exposure"])
        if self.environment is not None:
            ids = c.get("env") if "env" in c else self.host_env()
            li, bi, ti = (int(v) for v in ids[index])
            scene._light_map = self.environment.light_map(li)
            scene._background_image = self.environment.background(bi)
            scene._background_plane_texture = self.environment.plane_texture(ti)
        return scene
