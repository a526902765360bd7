"""CPU tests of the environment bank of the batch path (sl.EnvironmentBank, slhip_synth_place_env): a numpy mirror of the
Philox4x32-10 streams described in include/slhip.h ("Randomness") -- proven on the draws oracle/synth_ref.c makes, then the
reference for the environment stream --, the bank's records against HostPool.add_texture, the argument errors of the C-ABI
entry (refused before any launch, so no device is needed), and the condition on the seed of tests/test_gpu_environment.py
that keeps its checks from passing vacuously."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from stillleben_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the batch of tests/test_gpu_environment.py (its seed is checked below)
GPU_SEED, GPU_SCENE_ID_BASE, GPU_N_SCENES = 20261016, 256, 64
GPU_PROBS, GPU_COUNTS = (0.5, 0.5, 0.5), (3, 3, 3)

STREAM_SCENE, STREAM_ENV = 0, 4


# ---- the mirror -------------------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    c0, c1, c2, c3 = (int(v) for v in counter)
    k0, k1 = (int(v) for v in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def draw4(seed, scene_id, stream, index):
    """counter (scene id, stream, index, 0x51DE5EED), key (seed_lo, seed_hi)"""
    return philox4x32_10((scene_id & 0xFFFFFFFF, stream, index, 0x51DE5EED), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def u01(x):
    """((float)(x >> 8) + 0.5f) * 2^-24 in float32: the sum rounds (to even) above 2^23, as on the device"""
    return (np.float32(x >> 8) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def env_choice(seed, scene_id, counts, probs):
    """(light set, background, plane texture) of a scene, -1 = none: stream 4 of include/slhip.h; decisions in float32"""
    x, y = draw4(seed, scene_id, STREAM_ENV, 0), draw4(seed, scene_id, STREAM_ENV, 1)
    out = []
    for gate, pick, n, p in zip((x[0], x[2], y[0]), (x[1], x[3], y[1]), counts, probs):
        take = n > 0 and bool(u01(gate) < np.float32(p))
        out.append(min(n - 1, int(np.uint32(u01(pick) * np.float32(n)))) if take else -1)
    return out


def env_choices(seed, scene_id_base, n_scenes, counts, probs):
    return np.array([env_choice(seed, scene_id_base + s, counts, probs) for s in range(n_scenes)], np.int32)


def test_mirror_reproduces_the_oracles_draws(oracle):
    """Azimuth / elevation of oracle.synth_draws to 1 ulp (numpy has no fmaf: the product is formed exactly in float64 and
    rounded once more; a wrong counter or key layout gives unrelated numbers)."""
    seed = (77 << 32) | 12345
    p = np.zeros((), dtype=_abi.SYNTH_PARAMS_DTYPE)
    p["n_scenes"], p["n_objects"], p["n_assets"] = 4096, 2, 4
    p["seed_lo"], p["seed_hi"], p["scene_id_base"] = seed & 0xFFFFFFFF, seed >> 32, 1000
    two_pi, pi, span = np.float32(6.28318530717958647692), np.float32(3.14159265358979323846), np.float32(0.52359877559829887308)
    for s in (0, 1, 2, 3, 7, 64, 65, 500, 1023, 2048, 4000, 4095):
        ref = oracle.synth_draws(p, s)
        x = draw4(seed, 1000 + s, STREAM_SCENE, 0)
        for name, got in (("yaw", np.float32(float(u01(x[0])) * float(two_pi) - float(pi))),
                          ("azimuth", np.float32(float(u01(x[1])) * float(two_pi) - float(pi))),
                          ("elevation", np.float32(float(u01(x[2])) * float(span) + float(span)))):
            assert abs(float(got) - float(ref[name])) <= float(np.spacing(np.abs(np.float32(ref[name])))), (s, name, got, ref[name])


def test_u01_is_float32_arithmetic():
    assert u01(0) == np.float32(0.5 / 16777216.0) and u01(0xFFFFFFFF) == np.float32(1.0)    # 2^24 - 0.5 rounds to 2^24
    assert u01(0x800000FF) == np.float32(0.5)                       # 2^23 + 0.5 is a tie: to even, 2^23
    assert u01(0x800001FF) == np.float32((2 ** 23 + 2) * 2.0 ** -24)    # 2^23 + 1.5 is a tie: to even, 2^23 + 2
    assert 0.0 < float(u01(0x00000100)) < float(u01(0x00000200))


def picture_scenes(ids):
    """6 scenes that between them cover: the three-light map (light set 1), a one-light map, a background, a plane texture,
    all three kinds at once, nothing at all."""
    wants = [lambda r: r[0] == 1, lambda r: r[0] == 0, lambda r: r[1] >= 0 and r[0] < 0, lambda r: r[2] >= 0,
             lambda r: (r >= 0).all(), lambda r: (r < 0).all()]
    out = []
    for want in wants:
        hit = [s for s in range(len(ids)) if want(ids[s]) and s not in out]
        assert hit, "the seed does not offer such a scene"
        out.append(hit[0])
    return out


# ---- the bank's records -----------------------------------------------------------------------------------------------
class FakeLightMap:
    """What EnvironmentBank reads of an sl.LightMap (building a real one needs the device)."""

    def __init__(self, slot, directions, colors):
        self._slot = slot
        self.light_directions = [np.array(d, np.float32) for d in directions]
        self.light_colors = [np.array(c, np.float32) for c in colors]


def test_bank_records(sl):
    from stillleben_amd._batch import HostPool, effective_lights

    rng = np.random.default_rng(3)
    pool = HostPool()
    pool.add_texture((rng.random((8, 8, 4)) * 255).astype(np.uint8))          # something in front: offsets are not zero
    bg = [sl.Texture((rng.random((h, w, 4)) * 255).astype(np.uint8)) for h, w in ((30, 40), (17, 9))]
    pt = [sl.Texture2D((rng.random((h, w, 3)) * 255).astype(np.uint8)) for h, w in ((16, 16), (12, 20))]
    lm1 = FakeLightMap(4, [(0.3, -0.2, -0.93)], [(3.0, 2.8, 2.5)])
    lm5 = FakeLightMap(2, [(0, 0, -1), (1, 0, -1), (0, 1, -1), (1, 1, -1), (-1, 0, -1)], [(k + 1.0, 1.0, 0.5) for k in range(5)])
    lm0 = FakeLightMap(0, [], [])
    bank = sl.EnvironmentBank([lm1, lm5, lm0], bg, pt, pool=pool)
    assert bank.counts() == (3, 2, 2) and bank.max_lights == 3
    # textures: the pool's own answers for the same arrays; backgrounds one level, plane textures with the mip chain
    before = pool.n_tex_bytes
    for rec, t in zip(bank.backgrounds, bg):
        assert (int(rec["offset"]), int(rec["w"]), int(rec["h"])) == pool.add_texture(t._rgba, mips=False)
        assert (int(rec["w"]), int(rec["h"])) == (t._rgba.shape[1], t._rgba.shape[0])
    for rec, t in zip(bank.plane_textures, pt):
        assert (int(rec["offset"]), int(rec["w"]), int(rec["h"])) == pool.add_texture(t._rgba, mips=True)
        assert int(rec["sampler"]) == _abi.SAMPLER_DEFAULT
    assert pool.n_tex_bytes == before                          # nothing was stored again
    assert int(bank.backgrounds[1]["offset"]) - int(bank.backgrounds[0]["offset"]) == 30 * 40 * 4      # one level
    assert int(bank.plane_textures[1]["offset"]) - int(bank.plane_textures[0]["offset"]) == 4 * (256 + 64 + 16 + 4 + 1)
    # a texture added twice is stored once, in the bank and against the per-scene path's call
    assert bank.add_background(bg[0]) == 2 and pool.n_tex_bytes == before
    assert bank.backgrounds[2] == bank.backgrounds[0]
    assert bank.add_plane_texture(pt[1]) == 2 and pool.n_tex_bytes == before
    # light sets: slot + 1, the map's lights, cut at NUM_LIGHTS as effective_lights cuts them
    ls = bank.light_sets
    assert list(ls["light_map"]) == [5, 3, 1] and list(ls["n_lights"]) == [1, 3, 0]

    class FakeScene:
        pass

    for rec, lm in zip(ls, (lm1, lm5, lm0)):
        sc = FakeScene()
        sc._light_map = lm
        ld, lc, amb = effective_lights(sc)
        assert np.array_equal(rec["light_dir"][:, :3], ld) and np.array_equal(rec["light_color"][:, :3], lc)
        assert (rec["light_dir"][:, 3] == 0).all() and (rec["light_color"][:, 3] == 0).all() and (amb == 0).all()
    # the same map with other lights: a shallow copy that shares the slot
    k = bank.add_light_map(lm1, directions=[(0, 0, -1), (0, 1, -1)], colors=[(1, 1, 1), (2, 2, 2)])
    assert k == 3 and int(bank.light_sets[k]["light_map"]) == 5 and int(bank.light_sets[k]["n_lights"]) == 2
    other = bank.light_map(k)
    assert other is not lm1 and other._slot == lm1._slot and len(lm1.light_directions) == 1 and len(other.light_directions) == 2
    assert bank.light_map(0) is lm1 and bank.light_map(-1) is None and bank.background(1) is bg[1] and bank.plane_texture(-1) is None
    with pytest.raises(ValueError):
        bank.add_light_map(lm1, directions=[(0, 0, -1)])
    with pytest.raises(TypeError):
        bank.add_background(np.zeros((4, 4, 4), np.uint8))
    with pytest.raises(_abi.SlhipError):
        bank.device()                                          # a host-pool bank cannot drive a batch


def test_abi_struct_sizes_match_the_header():
    src = open(os.path.join(ROOT, "stillleben_amd", "csrc", "slhip_synth.hip")).read()
    sizes = {n: int(v) for n, v in re.findall(r"static_assert\(sizeof\((slhip_\w+)\) == (\d+)", src)}
    assert sizes["slhip_env_light_set"] == _abi.ENV_LIGHT_SET_DTYPE.itemsize == 112
    assert sizes["slhip_env_texture"] == _abi.ENV_TEXTURE_DTYPE.itemsize == 16
    assert sizes["slhip_synth_env"] == C.sizeof(_abi.SynthEnv) == 56
    assert sizes["slhip_synth_params"] == _abi.SYNTH_PARAMS_DTYPE.itemsize == 224       # untouched
    hdr = open(os.path.join(ROOT, "include", "slhip.h")).read()
    for name, size in (("slhip_env_light_set", 112), ("slhip_env_texture", 16), ("slhip_synth_env", 56)):
        assert re.search(r"\}\s*%s;\s*/\* %d bytes \*/" % (name, size), hdr), name
    assert "#define SLHIP_ABI_VERSION 5" in hdr or _abi.ABI_VERSION == 5
    # field offsets of the ctypes mirror = the C layout (4 pointers, 3 counts, 3 floats)
    assert [getattr(_abi.SynthEnv, f).offset for f, _ in _abi.SynthEnv._fields_] == [0, 8, 16, 24, 32, 36, 40, 44, 48, 52]


def test_place_env_refuses_malformed_banks():
    """Everything the host can see is refused with a message before any launch (the pointers below are never followed)."""
    import __graft_entry__ as g

    g.build()
    L = _abi.lib()
    p = np.zeros((), dtype=_abi.SYNTH_PARAMS_DTYPE)
    p["n_scenes"], p["n_objects"], p["n_assets"] = 4, 2, 3
    p["max_draws_per_scene"], p["max_chunks_per_scene"], p["max_clip_verts_per_scene"] = 3, 3, 100
    dummy = np.zeros(64, np.uint8)
    ptr = C.c_void_p(dummy.ctypes.data)

    def call(env, env_out=ptr, params=p):
        prm = np.array(params)
        return L.slhip_synth_place_env(C.c_void_p(prm.ctypes.data), C.byref(env) if env is not None else None,
                                       ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, env_out, C.c_void_p(0))

    def env(**kw):
        e = _abi.SynthEnv()
        e.d_light_sets = e.d_backgrounds = e.d_plane_textures = dummy.ctypes.data
        e.n_light_sets = e.n_backgrounds = e.n_plane_textures = 2
        e.p_light_map = e.p_background = e.p_plane_texture = 0.5
        for k, v in kw.items():
            setattr(e, k, v)
        return e

    def refused(e, word, **kw):
        assert call(e, **kw) != 0
        msg = L.slhip_last_error().decode()
        assert "slhip_synth_place_env" in msg and word in msg, msg

    refused(None, "null environment")
    for bank, name in (("d_light_sets", "light_sets"), ("d_backgrounds", "backgrounds"), ("d_plane_textures", "plane_textures")):
        refused(env(**{bank: None}), name + " / p_")                       # a null bank with a non-zero count
        assert "null bank" in L.slhip_last_error().decode()
    for prob in ("p_light_map", "p_background", "p_plane_texture"):
        for bad in (-0.1, 1.5, float("nan"), float("inf"), -float("inf")):
            refused(env(**{prob: bad}), "[0, 1]")
            assert prob in L.slhip_last_error().decode()
    for count, prob in (("n_light_sets", "p_light_map"), ("n_backgrounds", "p_background"), ("n_plane_textures", "p_plane_texture")):
        refused(env(**{count: 0}), "not empty")                             # a probability above zero for an empty bank
        assert prob in L.slhip_last_error().decode()
    refused(env(), "d_env_out", env_out=None)
    bad = p.copy()
    bad["n_objects"] = 0
    refused(env(), "n_objects", params=bad)
    # the plain entry is as it was
    assert L.slhip_synth_place(C.c_void_p(np.array(bad).ctypes.data), ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, C.c_void_p(0)) != 0
    assert "slhip_synth_place:" in L.slhip_last_error().decode()


def test_public_surface(sl):
    from stillleben_amd import scene_batch

    import inspect

    sig = inspect.signature(scene_batch.SceneBatch.__init__).parameters
    assert [sig[k].default for k in ("environment", "p_light_map", "p_background", "p_plane_texture", "env_ids")] == [None, 1.0, 1.0, 1.0, None]
    assert sl.EnvironmentBank is __import__("stillleben").EnvironmentBank


# ---- the input of the GPU test ------------------------------------------------------------------------------------------
def test_gpu_test_seed_exercises_every_kind():
    ids = env_choices(GPU_SEED, GPU_SCENE_ID_BASE, GPU_N_SCENES, GPU_COUNTS, GPU_PROBS)
    for k in range(3):
        took = int((ids[:, k] >= 0).sum())
        assert took >= 8 and GPU_N_SCENES - took >= 8, (k, took)
        assert set(ids[:, k].tolist()) == {-1, 0, 1, 2}, k                # every entry of the 3-entry bank is picked
    chosen = picture_scenes(ids)                                          # (asserts that every wanted kind of scene exists)
    assert len(set(chosen)) == 6
    assert any((ids[s] >= 0).all() and ids[s, 0] == 1 for s in range(GPU_N_SCENES))    # the three-light map with everything bound
