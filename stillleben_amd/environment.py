"""sl.EnvironmentBank -- the light maps, background images and plane textures a SceneBatch hands out to its scenes on
the device: the batch-path counterpart of `scene.light_map = sl.LightMap(...)` (reference examples/ycb.py:64-67),
`scene.background_plane_texture = sl.Texture2D(...)` (examples/ycb.py:73-74) and `scene.background_image = sl.Texture(...)`
(python/src/py_scene.cpp:131-140).  Like the asset table it is described once; slhip_synth_place_env (include/slhip.h) gives
every scene its environment from the batch's counter-based random streams, or as the caller names it.

    bank = sl.EnvironmentBank(light_maps=[sl.LightMap(p) for p in ibl_files],
                              backgrounds=[sl.Texture(img) for img in photos],
                              plane_textures=[sl.Texture2D(p) for p in texture_files])
    batch = sl.SceneBatch(table, 4096, 20, environment=bank, p_background=0.5)
"""
import copy

import numpy as np

from . import _abi


class EnvironmentBank:
    """`light_maps`: sl.LightMap objects (each contributes its map and the lights its .ibl file names); `backgrounds`:
    sl.Texture (rectangle textures, one level); `plane_textures`: sl.Texture2D (stored with their mip chain).

    The textures are registered with the engine's texel pool by the calls the per-scene path makes
    (`HostPool.add_texture`), so a texture that is also bound to an sl.Scene is stored once.  The pool addresses texels with
    32-bit offsets: a bank that would take it beyond 4 GiB is refused with the pool's own RuntimeError.

    `pool`: a host pool to register with instead of the device engine's (tests build the records that way; such a bank cannot
    drive a SceneBatch)."""

    def __init__(self, light_maps=(), backgrounds=(), plane_textures=(), pool=None):
        if pool is None:
            from ._context import engine

            self.eng = engine()
            pool = self.eng.pool
        else:
            self.eng = None
        self.pool = pool
        self._light_sets, self._backgrounds, self._plane_textures = [], [], []   # records
        self._light_maps, self._bg_objects, self._pt_objects = [], [], []        # the objects SceneBatch.scene() hands over
        self._dev = None
        for lm in light_maps:
            self.add_light_map(lm)
        for t in backgrounds:
            self.add_background(t)
        for t in plane_textures:
            self.add_plane_texture(t)

    # ---- building ------------------------------------------------------------------------------------------------
    def add_light_map(self, lm, directions=None, colors=None):
        """Adds `lm` with its own lights, or -- `directions` and `colors` given -- the same map with other lights.  Lights
        beyond NUM_LIGHTS are cut as the renderer cuts them (render_pass.cpp:417-418).  Returns the light set's index."""
        if not all(hasattr(lm, a) for a in ("_slot", "light_directions", "light_colors")):
            raise TypeError("expected an sl.LightMap")
        if (directions is None) != (colors is None):
            raise ValueError("give both directions and colors, or neither")
        if directions is not None:
            shared = lm
            lm = copy.copy(shared)           # shares the map's textures and slot, carries the set's lights
            lm.light_directions = [np.array(d, dtype=np.float32).reshape(3) for d in directions]
            lm.light_colors = [np.array(c, dtype=np.float32).reshape(3) for c in colors]
        rec = np.zeros((), dtype=_abi.ENV_LIGHT_SET_DTYPE)
        rec["light_map"] = lm._slot + 1
        lights = list(zip(lm.light_directions, lm.light_colors))[:_abi.NUM_LIGHTS]
        rec["n_lights"] = len(lights)
        for i, (d, c) in enumerate(lights):
            rec["light_dir"][i, :3], rec["light_color"][i, :3] = d, c
        self._light_sets.append(rec)
        self._light_maps.append(lm)
        self._dev = None
        return len(self._light_sets) - 1

    def _texture(self, tex, mips):
        if not hasattr(tex, "_rgba"):
            raise TypeError("expected an sl.Texture / sl.Texture2D")
        off, w, h = self.pool.add_texture(tex._rgba, mips=mips)
        rec = np.zeros((), dtype=_abi.ENV_TEXTURE_DTYPE)
        rec["offset"], rec["w"], rec["h"], rec["sampler"] = off, w, h, _abi.SAMPLER_DEFAULT
        return rec

    def add_background(self, tex):
        self._backgrounds.append(self._texture(tex, mips=False))
        self._bg_objects.append(tex)
        self._dev = None
        return len(self._backgrounds) - 1

    def add_plane_texture(self, tex):
        self._plane_textures.append(self._texture(tex, mips=True))
        self._pt_objects.append(tex)
        self._dev = None
        return len(self._plane_textures) - 1

    # ---- records -------------------------------------------------------------------------------------------------
    @property
    def light_sets(self):
        return np.array(self._light_sets, dtype=_abi.ENV_LIGHT_SET_DTYPE)

    @property
    def backgrounds(self):
        return np.array(self._backgrounds, dtype=_abi.ENV_TEXTURE_DTYPE)

    @property
    def plane_textures(self):
        return np.array(self._plane_textures, dtype=_abi.ENV_TEXTURE_DTYPE)

    def counts(self):
        return len(self._light_sets), len(self._backgrounds), len(self._plane_textures)

    @property
    def max_lights(self):
        """Largest n_lights of the bank's light sets (0 without one): the shadow maps per scene a batch on this bank needs."""
        return min(_abi.NUM_LIGHTS, max((int(r["n_lights"]) for r in self._light_sets), default=0))

    def device(self):
        """The three record arrays in HBM (uploaded once, again after an add_*)."""
        if self.eng is None:
            raise _abi.SlhipError("this EnvironmentBank was built on a host pool (test helper); build it without one to use the device")
        if self._dev is None:
            from .scene_batch import _dev

            d = self.eng.device
            self._dev = tuple(_dev(a, d) for a in (self.light_sets, self.backgrounds, self.plane_textures))
        return self._dev

    # ---- hand-over (SceneBatch.scene) --------------------------------------------------------------------------------
    def light_map(self, i):
        return self._light_maps[i] if i >= 0 else None

    def background(self, i):
        return self._bg_objects[i] if i >= 0 else None

    def plane_texture(self, i):
        return self._pt_objects[i] if i >= 0 else None
