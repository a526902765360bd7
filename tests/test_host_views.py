"""CPU tests of the views of the batch path (SceneBatch.place(view=...), slhip_synth_place_view, sl.bop): the Philox key of a
view against the draws oracle/synth_ref.c makes under that key, the BOP entries on hand-made values, the argument errors of
place() and of the C-ABI entry (all refused before anything is asked of a device), the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from stillleben_amd import _abi
from test_host_environment import STREAM_SCENE, philox4x32_10, u01

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_view_key_wraps_at_32_bits():
    assert _abi.view_key(5, 77, 0) == (5, 77)
    assert _abi.view_key(5, 77, 1) == (5 + 0x9E3779B9, 77 + 0xBB67AE85)
    assert _abi.view_key(0xFFFFFFFF, 0xFFFFFFFF, 1) == (0x9E3779B8, 0xBB67AE84)
    assert _abi.view_key(5, 77, 2) == ((5 + 2 * 0x9E3779B9) % 2 ** 32, (77 + 2 * 0xBB67AE85) % 2 ** 32)
    assert _abi.view_key(5, 77, 7) == ((5 + 7 * 0x9E3779B9) % 2 ** 32, (77 + 7 * 0xBB67AE85) % 2 ** 32)
    assert _abi.view_key(0, 0, 0xFFFFFFFF) == ((-0x9E3779B9) % 2 ** 32, (-0xBB67AE85) % 2 ** 32)
    keys = {_abi.view_key(5, 77, v) for v in range(64)}
    assert len(keys) == 64 and all(0 <= k < 2 ** 32 for key in keys for k in key)


def test_view_draws_are_the_oracles_draws_under_the_view_key(oracle):
    """Azimuth / elevation of view v from the mirror of tests/test_host_environment.py keyed with the view's key = what
    oracle.synth_draws gives for params whose seed is that key (to 1 ulp: numpy has no fmaf, the product is formed exactly in
    float64 and rounded once more), and they differ from view to view."""
    seed_lo, seed_hi = 0xFFFFFF05, 77             # seed_lo wraps from view 1 on
    two_pi, pi, span = np.float32(6.28318530717958647692), np.float32(3.14159265358979323846), np.float32(0.52359877559829887308)
    seen = set()
    for v in (0, 1, 2, 7, 1000):
        k0, k1 = _abi.view_key(seed_lo, seed_hi, v)
        p = np.zeros((), dtype=_abi.SYNTH_PARAMS_DTYPE)
        p["n_scenes"], p["n_objects"], p["n_assets"] = 64, 2, 4
        p["seed_lo"], p["seed_hi"], p["scene_id_base"] = k0, k1, 1000
        for s in (0, 1, 36, 63):
            ref = oracle.synth_draws(p, s)
            x = philox4x32_10((1000 + s, STREAM_SCENE, 0, 0x51DE5EED), (k0, k1))
            for name, got in (("azimuth", np.float32(float(u01(x[1])) * float(two_pi) - float(pi))),
                              ("elevation", np.float32(float(u01(x[2])) * float(span) + float(span)))):
                assert abs(float(got) - float(ref[name])) <= float(np.spacing(np.abs(np.float32(ref[name])))), (v, s, name)
            seen.add((float(ref["azimuth"]), float(ref["elevation"])))
    assert len(seen) == 5 * 4


def test_bop_scene_camera_entry(sl):
    # camera at (1, 2, 3) m looking along world +x: camera x, y, z = world -y, -z, +x (scene.cpp:489-493)
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3] = np.array([[0, 0, 1], [-1, 0, 0], [0, -1, 0]], np.float32)
    pose[:3, 3] = (1.0, 2.0, 3.0)
    e = sl.bop.scene_camera_entry((1066.778, 1067.487, 312.9869, 241.3109), pose)
    assert e["cam_K"] == [1066.778, 0.0, 312.9869, 0.0, 1067.487, 241.3109, 0.0, 0.0, 1.0]
    assert e["cam_R_w2c"] == [0.0, -1.0, 0.0, 0.0, 0.0, -1.0, 1.0, 0.0, 0.0]            # row-major transpose
    assert np.allclose(e["cam_t_w2c"], [2000.0, 3000.0, -1000.0], atol=1e-9)             # -R^T t, millimetres
    assert e["depth_scale"] == 1.0 and set(e) == {"cam_K", "cam_R_w2c", "cam_t_w2c", "depth_scale"}
    K = np.array([[500.0, 0, 160], [0, 510.0, 120], [0, 0, 1]])
    e = sl.bop.scene_camera_entry(K, torch.from_numpy(pose), depth_scale=0.1)
    assert e["cam_K"] == [500.0, 0.0, 160.0, 0.0, 510.0, 120.0, 0.0, 0.0, 1.0] and e["depth_scale"] == 0.1
    # a world point in front of the camera lands where K [R | t] says
    X = np.array([4.0, 2.0, 3.0])
    xc = np.array(e["cam_R_w2c"]).reshape(3, 3) @ (X * 1000.0) + np.array(e["cam_t_w2c"])
    assert np.allclose(xc, [0.0, 0.0, 3000.0], atol=1e-9)
    with pytest.raises(ValueError):
        sl.bop.scene_camera_entry((1.0, 2.0, 3.0), pose)
    with pytest.raises(ValueError):
        sl.bop.scene_camera_entry(K, pose[:3])


def test_bop_scene_gt_entries(sl):
    o2c = np.zeros((3, 3, 4), np.float32)
    o2c[0, :, :3], o2c[0, :, 3] = np.eye(3), (0.1, -0.2, 0.75)
    o2c[1, :, :3], o2c[1, :, 3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]], (0.0, 0.0, 1.5)
    o2c[2, :, :3], o2c[2, :, 3] = [[1, 0, 0], [0, 0, -1], [0, 1, 0]], (-0.5, 0.25, 2.0)
    m2o = np.stack([np.eye(4)] * 3)
    m2o[1, :3, 3] = (0.01, 0.02, 0.03)              # a centring pretransform
    gt = sl.bop.scene_gt_entries(o2c, m2o, [5, 2, 9])
    assert [g["obj_id"] for g in gt] == [5, 2, 9]                                        # slot order, class indices
    assert all(set(g) == {"cam_R_m2c", "cam_t_m2c", "obj_id"} and len(g["cam_R_m2c"]) == 9 and len(g["cam_t_m2c"]) == 3 for g in gt)
    assert gt[0]["cam_R_m2c"] == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    assert np.allclose(gt[0]["cam_t_m2c"], [100.0, -200.0, 750.0], atol=1e-4)
    assert gt[1]["cam_R_m2c"] == [0, -1, 0, 1, 0, 0, 0, 0, 1]                            # row-major
    assert np.allclose(gt[1]["cam_t_m2c"], [-20.0, 10.0, 1530.0], atol=1e-4)             # R * pretranslation + t, millimetres
    assert gt[2]["cam_R_m2c"] == [1, 0, 0, 0, 0, -1, 0, 1, 0]
    same = sl.bop.scene_gt_entries(torch.from_numpy(o2c), None, [5, 2, 9])
    assert same[0] == gt[0] and same[2] == gt[2] and np.allclose(same[1]["cam_t_m2c"], [0.0, 0.0, 1500.0])
    one = sl.bop.scene_gt_entries(o2c, m2o[1], [1, 1, 1])
    assert one[1]["cam_t_m2c"] == gt[1]["cam_t_m2c"] and [g["obj_id"] for g in one] == [1, 1, 1]
    with pytest.raises(ValueError):
        sl.bop.scene_gt_entries(o2c, m2o, [5, 2])
    with pytest.raises(ValueError):
        sl.bop.scene_gt_entries(o2c.reshape(3, 12), m2o, [5, 2, 9])
    import stillleben

    assert stillleben.bop is sl.bop


def test_place_refuses_bad_view_arguments_before_any_device_call():
    """SceneBatch.place() checks its arguments first: on a batch whose every other attribute is missing, the ValueError is
    what comes out (anything later would be an AttributeError), and the checker never touches the device."""
    from stillleben_amd import scene_batch
    from stillleben_amd.scene_batch import SceneBatch, check_view_arguments

    dev = torch.device("cuda", 0)
    good = torch.zeros((37, 4, 4), dtype=torch.float32)                 # (on the host: right for a batch on "cpu" only)
    check_view_arguments(0, None, 37, dev)
    check_view_arguments(7, good, 37, torch.device("cpu"))
    for view in (-1, -7, 1.5, 2 ** 32, True):
        with pytest.raises(ValueError):
            check_view_arguments(view, None, 37, dev)
    for bad in (torch.zeros((37, 16)), torch.zeros((36, 4, 4)), torch.zeros((37, 4, 4), dtype=torch.float64),
                torch.zeros((37, 4, 4), dtype=torch.float16), np.zeros((37, 4, 4), np.float32), torch.zeros((4, 4, 37)).permute(2, 0, 1)):
        with pytest.raises(ValueError):
            check_view_arguments(0, bad, 37, torch.device("cpu"))
    with pytest.raises(ValueError, match="device"):
        check_view_arguments(0, good, 37, dev)                           # a host tensor for a batch on the GPU

    class Eng:
        device = dev

    b = object.__new__(SceneBatch)
    b.n_scenes, b.eng = 37, Eng()
    with pytest.raises(ValueError):
        b.place(view=-1)
    with pytest.raises(ValueError):
        b.place(camera_poses=good)
    with pytest.raises(ValueError):
        b.place(camera_poses=torch.zeros((37, 3, 4)))
    import inspect

    sig = inspect.signature(SceneBatch.place).parameters
    assert [sig[k].default for k in ("view", "camera_poses", "object_to_camera")] == [0, None, False]
    assert scene_batch.SceneBatch.views and scene_batch.SceneBatch.host_cameras


def test_header_declares_the_entry_and_the_version_stays():
    hdr = open(os.path.join(ROOT, "include", "slhip.h")).read()
    assert "#define SLHIP_ABI_VERSION 5 " in hdr and _abi.ABI_VERSION == 5
    assert re.search(r"\bint slhip_synth_place_view\(const slhip_synth_params\* params, const slhip_synth_env\* env, "
                     r"const slhip_synth_view\* view,", hdr)
    assert re.search(r"\}\s*slhip_synth_view;\s*/\* 24 bytes \*/", hdr)
    assert "0x9E3779B9" in hdr and "0xBB67AE85" in hdr                   # the "Randomness" paragraph names the view key
    src = open(os.path.join(ROOT, "stillleben_amd", "csrc", "slhip_synth.hip")).read()
    assert "static_assert(sizeof(slhip_synth_view) == 24" in src and C.sizeof(_abi.SynthView) == 24
    assert [getattr(_abi.SynthView, f).offset for f, _ in _abi.SynthView._fields_] == [0, 4, 8, 16]


def test_place_view_refuses_before_any_launch():
    """A null view, the refusals of slhip_synth_place_env when an environment is given, d_env_out without env and env without
    d_env_out: refused with a message (the pointers below are never followed)."""
    import __graft_entry__ as g

    g.build()
    L = _abi.lib()
    p = np.zeros((), dtype=_abi.SYNTH_PARAMS_DTYPE)
    p["n_scenes"], p["n_objects"], p["n_assets"] = 4, 2, 3
    p["max_draws_per_scene"], p["max_chunks_per_scene"], p["max_clip_verts_per_scene"] = 3, 3, 100
    dummy = np.zeros(64, np.uint8)
    ptr = C.c_void_p(dummy.ctypes.data)
    view = _abi.SynthView()
    view.view = 1

    def env(**kw):
        e = _abi.SynthEnv()
        e.d_light_sets = e.d_backgrounds = e.d_plane_textures = dummy.ctypes.data
        e.n_light_sets = e.n_backgrounds = e.n_plane_textures = 2
        e.p_light_map = e.p_background = e.p_plane_texture = 0.5
        for k, v in kw.items():
            setattr(e, k, v)
        return e

    def refused(word, e=None, v=view, env_out=None, params=p, first=ptr):
        prm = np.array(params)
        st = L.slhip_synth_place_view(C.c_void_p(prm.ctypes.data), C.byref(e) if e is not None else None,
                                      C.byref(v) if v is not None else None, first, ptr, ptr, ptr, ptr, ptr, ptr, ptr, env_out,
                                      C.c_void_p(0))
        assert st != 0
        msg = L.slhip_last_error().decode()
        assert "slhip_synth_place_view" in msg and word in msg, msg

    refused("null view", v=None)
    refused("null view", e=env(), v=None, env_out=ptr)
    refused("d_env_out", env_out=ptr)                                     # d_env_out without an environment
    refused("d_env_out", e=env())                                         # an environment without d_env_out
    refused("null bank", e=env(d_backgrounds=None), env_out=ptr)
    refused("[0, 1]", e=env(p_light_map=float("nan")), env_out=ptr)
    refused("not empty", e=env(n_plane_textures=0), env_out=ptr)
    refused("null argument", first=None)
    bad = p.copy()
    bad["n_objects"] = 65
    refused("n_objects", params=bad)
    bad = p.copy()
    bad["max_draws_per_scene"] = 0
    refused("record strides", params=bad)
