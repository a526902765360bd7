"""The CPU oracle's geometric G-buffer against the float64 ray cast of tests/raster_ref.py: every channel, per pixel, from a
definition that shares nothing with oracle/render_ref.c or the kernels.  tests/test_gpu_raster_known.py holds the kernels to the
same reference with the same helpers (raster_ref.check and the per-scene assertions behind it); this file is where the
exclusions' caps and the tolerances are shown to hold without a GPU.

Exclusions, caps and the bound |out - ref| <= E_snap + 16 2^-23 M are raster_ref.py's (derivations in its docstring): edge and
clip-line margin 1/128 px, depth margin four 24-bit steps plus both snapping envelopes, left-out pixels at most 5 % of the covered
ones (15 % in the sliver scene), covered pixels at least 3 % of the picture.  Run with -s for the figures of every scene.

Worst |out - ref| / bound on the kept pixels, per scene and channel, as this file measures them on the oracle (the kernels give
the same figures; the w of bary and cam_coord is exact everywhere).  A throw-away prototype of this comparison measured at most
0.45 on the clutter scenes; the largest here is 0.49 (barycentrics on the ellipsoid), so the bound's factor of 1 on the snapping
envelope leaves 2x:

  scene                    covered left out    bary cam_coord coord.xyz coord.w normals.xyz normals.w
  borders                   100.0%    0.06%    0.36      0.39      0.36    0.31        0.07      0.29
  clip                       66.7%    1.02%    0.37      0.37      0.37    0.37        0.37      0.37
  clip@150x100               69.8%    0.12%    0.42      0.42      0.42    0.42        0.40      0.39
  clutter21                   5.9%    1.67%    0.43      0.44      0.39    0.44        0.04      0.40
  clutter3                    5.2%    1.61%    0.41      0.41      0.41    0.37        0.04      0.35
  clutter33@1x1             100.0%    0.00%    0.25      0.25      0.25    0.20        0.01      0.19
  clutter33@33x9             16.5%    4.08%    0.41      0.44      0.41    0.37        0.05      0.36
  clutter33@7x5               8.6%    0.00%    0.32      0.32      0.32    0.28        0.03      0.28
  clutter3@130x98             5.2%    1.52%    0.43      0.43      0.42    0.41        0.04      0.41
  clutter3@150x100            5.9%    2.16%    0.44      0.42      0.44    0.42        0.04      0.41
  clutter8                    6.2%    1.77%    0.42      0.44      0.42    0.44        0.06      0.42
  coincident                 11.0%    0.57%    0.44      0.45      0.44    0.38        0.04      0.37
  facing                      6.9%    0.94%    0.43      0.42      0.42    0.00        0.00      0.28
  inside_cube               100.0%    0.00%    0.40      0.42      0.40    0.42        0.02      0.35
  interpenetrating           16.2%    0.64%    0.39      0.44      0.40    0.37        0.06      0.37
  sliver                     27.9%    0.60%    0.44      0.43      0.43    0.37        0.02      0.38
  smooth                     52.5%    1.00%    0.49      0.43      0.45    0.42        0.48      0.44
  steep                      34.7%    0.00%    0.37      0.36      0.36    0.36        0.37      0.37
  interpenetrating peeled    16.2%    0.67%    0.42      0.41      0.40    0.38        0.06      0.37
  smooth peeled              52.5%    1.00%    0.47      0.42      0.46    0.42        0.48      0.46
"""
import numpy as np
import pytest

import raster_ref as R
from stillleben_amd import _abi
from test_oracle_render import oracle_render

GEOMETRY = _abi.OUT_ALL & ~_abi.OUT_RGB


@pytest.mark.parametrize("name", sorted(R.SCENES))
def test_scene_against_ray_cast(sl, oracle, name):
    scene, ref = R.reference(sl, name)
    R.check(name, ref, R.channels_of(oracle_render(oracle, [scene], flags=GEOMETRY)))


def test_steep_perspective_tells_affine_apart(sl, oracle):
    """Scene 3 discriminates: the reference's own screen-space (affine) variant is off by more than 100 bounds in every
    interpolated channel, and the oracle's picture fails against it."""
    scene, ref = R.reference(sl, "steep")
    wrong = R.cast(R.soup_from_scene(scene), affine=True)
    keep = ref.keep & ref.covered
    for c in R.FLOAT_CHANNELS:
        ratio = (np.abs(getattr(wrong, c) - getattr(ref, c))[keep] / ref.tol[c][keep])
        n = 4 if c in ("coord", "normals") else 3
        assert ratio[:, :n].max() > 100.0, (c, ratio[:, :n].max())
    out = R.channels_of(oracle_render(oracle, [scene], flags=GEOMETRY))
    with pytest.raises(AssertionError):
        R.assert_within(R.compare(wrong, out, label="affine"), "affine")


@pytest.mark.parametrize("name", ["interpenetrating", "smooth"])
def test_depth_peel_second_layer(sl, oracle, name):
    """Scene 9: the layer behind the first one against the reference's definition of it."""
    scene, first = R.reference(sl, name)
    r0 = oracle_render(oracle, [scene], flags=GEOMETRY)
    r1 = oracle_render(oracle, [scene], flags=GEOMETRY, depth_peel=r0.coord)
    ref = R.cast(R.soup_from_scene(scene), peel=(first, r0.coord[0, :, :, 3]))
    R.check(name + " peeled", ref, R.channels_of(r1))
    assert (ref.covered & ref.keep & (ref.tri != first.tri)).sum() > 300
