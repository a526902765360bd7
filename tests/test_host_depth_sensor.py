"""Host tests of the depth sensor model: the known answers of the NumPy restatement (tests/depth_sensor_ref.py, the reference
the GPU tests compare slhip_depth_sensor against) and the host side of the feature -- record layout against include/slhip.h,
the limits, the scratch size, the BOP depth scale.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import depth_sensor_ref as R
from conftest import ROOT
from stillleben_amd import _abi, bop
from stillleben_amd import depth_sensor as ds

F = np.float32


def test_shadow_known_answer():
    z, c = R.rectangle_scene()
    p = R.known_answer_params(ds.make_params)
    assert float(p["fb"]) == 32.0
    zf, zu, fl = R.reference(z, p, c)
    shadow = np.zeros(z.shape, bool)
    shadow[6:18, 24:40] = True                      # width d_front - d_back = 32 - 16, on the side away from the projector
    assert np.array_equal((fl & R.SHADOW) != 0, shadow) and int(shadow.sum()) == 192
    support = np.zeros(z.shape, bool)
    for y, x in ((0, 0), (0, 95), (23, 0), (23, 95), (6, 40), (6, 63), (17, 40), (17, 63)):
        support[y, x] = True
    assert np.array_equal((fl & R.SUPPORT) != 0, support)
    assert not (fl & (R.RANGE | R.GRAZING | R.DROPOUT)).any()
    valid = fl == 0
    assert round(100.0 * valid.mean(), 1) == 91.3
    assert np.array_equal(zf[valid].view(np.uint32), z[valid].view(np.uint32))      # integer disparities survive the quantisation
    assert (zf[~valid] == 0).all() and (zu[~valid] == 0).all()
    assert np.array_equal(zu[valid], (z[valid] * 1000).astype(np.uint16))


def test_quantisation():
    """A ramp z = 1 + 0.01 x under the parameters of the shadow scene: |z_out - z| <= z^2 / (2 fb q) at every pixel, fewer
    distinct depths than columns, and no flag -- but for SUPPORT at the four image corners, which the model gives every image
    under r = 1, min_support = 6 (a corner's window holds 4 pixels; the shadow known answer lists them too).  With
    min_support = 4 no flag is left at all and the bound holds on the whole image."""
    z = R.ramp_scene()
    fb, q = 32.0, 8.0
    bound = z.astype(np.float64) ** 2 / (2 * fb * q)
    corners = np.zeros(z.shape, np.uint8)
    corners[0, 0] = corners[0, -1] = corners[-1, 0] = corners[-1, -1] = R.SUPPORT
    for min_support, expect in ((6, corners), (4, np.zeros(z.shape, np.uint8))):
        zf, _, fl = R.reference(z, R.known_answer_params(ds.make_params, min_support=min_support), np.ones_like(z))
        assert np.array_equal(fl, expect)
        err = np.abs(zf.astype(np.float64) - z)[fl == 0]
        print("max |z_out - z| = %.4f, largest bound %.4f" % (err.max(), bound.max()))
        assert (err <= bound[fl == 0]).all()
        assert len(np.unique(zf[fl == 0])) < z.shape[1]


def test_grazing_plane_still_shadows():
    z, _ = R.rectangle_scene()
    c = np.ones_like(z)
    c[6:18, 40:64] = 0.1                              # the rectangle is seen at a grazing angle
    p = R.known_answer_params(ds.make_params, cos_min=0.2)
    _, _, fl = R.reference(z, p, c)
    assert (fl[6:18, 40:64] == R.GRAZING).all() and int(((fl & R.GRAZING) != 0).sum()) == 12 * 24
    assert ((fl[6:18, 24:40] & R.SHADOW) != 0).all()   # it blocks the projector all the same
    assert int(((fl & R.SHADOW) != 0).sum()) == 192
    # the stage is off at cos_min = 0 and without an n.v plane
    for kw, cc in ((dict(cos_min=0.0), c), (dict(cos_min=0.2), None)):
        assert not (R.reference(z, R.known_answer_params(ds.make_params, **kw), cc)[2] & R.GRAZING).any()


def test_range_and_uint16():
    z = np.full((8, 32), 2.0, F)
    z[1, 3], z[2, 5], z[3, 7], z[4, 9] = 3000.0, np.nan, 0.0, -1.0
    p = R.known_answer_params(ds.make_params, window_radius=0, min_support=1, depth_scale=0.025)
    zf, zu, fl = R.reference(z, p, None)
    for y, x in ((1, 3), (2, 5), (3, 7), (4, 9)):
        assert fl[y, x] == R.RANGE and zf[y, x] == 0 and zu[y, x] == 0
    assert int((fl != 0).sum()) == 4
    assert (zu[fl == 0] == 65535).all()               # 2000 mm / 0.025 = 80000 units: saturated
    zu1 = R.reference(z, R.known_answer_params(ds.make_params, window_radius=0, min_support=1), None)[1]
    assert (zu1[fl == 0] == 2000).all()


def _header():
    return open(os.path.join(ROOT, "include", "slhip.h")).read()


def test_record_layout_matches_the_header():
    m = re.search(r"typedef struct \{([^}]*)\} slhip_depth_sensor_params;\s*/\* (\d+) bytes \*/", _header())
    assert m, "slhip_depth_sensor_params not found in include/slhip.h"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), {"float": np.float32, "uint32_t": np.uint32}[ctype]) for n in names.split(",")]
    dt = _abi.DEPTH_SENSOR_DTYPE
    assert [n for n, _ in fields] == list(dt.names)
    assert all(dt[n] == np.dtype(t) for n, t in fields)
    assert dt.itemsize == int(m.group(2)) == 60 and [dt.fields[n][1] for n in dt.names] == list(range(0, 60, 4))
    p = ds.make_params(580.0)
    assert p.dtype == dt and p.nbytes == 60
    assert float(p["fb"]) == float(F(580.0 * 0.075)) and int(p["subpixel"]) == 8      # the documented defaults
    with pytest.raises(TypeError):
        ds.make_params()                              # fx has no default


def test_ctypes_signatures_match_the_header():
    hdr = _header()
    L = _abi.lib()
    for name in ("slhip_depth_sensor", "slhip_depth_sensor_scratch_bytes", "slhip_depth_sensor_check_params"):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        at = getattr(L, name).argtypes
        assert len(at) == len(args), name
        for a, t in zip(args, at):
            want = C.c_void_p if "*" in a else {"uint32_t": C.c_uint32, "int": C.c_int}[a.split()[0]]
            assert t is want or (want is C.c_void_p and issubclass(t, C._Pointer)), (name, a)
    assert L.slhip_abi_version() == 5 == _abi.ABI_VERSION


def test_scratch_bytes_and_limits_need_no_gpu():
    assert ds.scratch_bytes(512, 640, 480) == 512 * 640 * 480 * 5
    assert ds.scratch_bytes(0, 640, 480) == 0
    with pytest.raises(_abi.SlhipError):
        ds.scratch_bytes(1, 0, 480)
    ok = ds.make_params(580.0)                        # Dmax = ceil(43.5 / 0.4) = 109
    ds.check_params([ok, ok], 640)
    ds.check_params([ok], 4096 - 109)
    with pytest.raises(_abi.SlhipError, match="exceeds 4096"):
        ds.check_params([ok, ok], 4096 - 108)
    with pytest.raises(_abi.SlhipError, match="exceeds 4096"):
        ds.check_params([ds.make_params(580.0, z_min=0.01)], 640)     # Dmax = 4350
    with pytest.raises(ValueError):
        ds.make_params(580.0, window_radius=5)
    bad = ok.copy()
    bad["window_radius"] = 5                          # a record no make_params would write
    with pytest.raises(_abi.SlhipError, match="window_radius 5"):
        ds.check_params([ok, bad], 640)
    for field, value in (("z_min", 0.0), ("fb", -1.0), ("depth_scale", 0.0), ("z_max", 0.1)):
        bad = ok.copy()
        bad[field] = value
        with pytest.raises(_abi.SlhipError):
            ds.check_params([bad], 640)


def test_public_interface_on_the_host():
    import torch

    import stillleben_amd as sl

    assert sl.depth_sensor is ds and "depth_sensor" in sl.__all__
    with pytest.raises(_abi.SlhipError, match="cuda tensor"):
        ds.process_batch(torch.ones(1, 8, 8), [ds.make_params(580.0)])
    s = bop.depth_image_scale(4.0)
    assert s == 4000.0 / 65535.0 and np.floor(F(4.0) * F(1000) / F(s) + F(0.5)) == 65535
    p = ds.make_params(512.0, baseline=0.0625, z_min=0.25, z_max=4.0, window_radius=0, min_support=1, sigma_lateral=0.0,
                       sigma_disparity=0.0, subpixel=0, dropout_p=0.0, depth_scale=s, seed=0)
    zu = R.reference(np.array([[4.0, 2.0, 0.25]], F), p)[1]
    assert zu.tolist() == [[65535, 32768, 4096]]          # z_max on the last unit; no valid depth saturates below it
    assert bop.scene_camera_entry((500, 500, 320, 240), np.eye(4), depth_scale=s)["depth_scale"] == s
