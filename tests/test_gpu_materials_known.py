"""GPU: the kernels' material stage (k_shade of slhip_render.hip: texture2D, sRGB decode, normal maps, metallic-roughness /
emissive / occlusion channels, the sticker, the direct-light lobe) against the float64 definition of tests/material_ref.py -- no
oracle involved.  The scenes, the checks and the bound |got - ref| <= 1e-3 |ref| + S + 1e-6 are those of
tests/test_oracle_materials.py, whose docstring records the measured shares of both sides."""
import os

import numpy as np
import pytest
import torch

import material_ref as R
import test_oracle_materials as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def light_map(sl):
    import ibl_analytic as A

    return sl.LightMap(T.constant_equirect(), sizes=A.SIZES_COARSE)


def gpu_pictures(sl, cases, light_map=None):
    """[(case, scene, hdr, normals, instance, coord)]: one render of the whole list, the float image kept."""
    from test_gpu_ibl import render_hdr

    scenes = [R.build_scene(sl, c, light_map if c.light_map else None) for c in cases]
    bufs, hdr = render_hdr(scenes)
    normals, inst, coord = bufs.normals.cpu().numpy(), bufs.instance.cpu().numpy(), bufs.coord.cpu().numpy()
    return [(c, s, hdr[k], normals[k], inst[k, :, :, 0], coord[k]) for k, (c, s) in enumerate(zip(cases, scenes))]


@pytest.mark.parametrize("size", R.SIZES, ids=["%dx%d" % s for s in R.SIZES])
def test_texture_sizes_and_wraps(sl, size):
    T.hold_to_reference(gpu_pictures(sl, R.size_cases(*size)))


@pytest.mark.parametrize("placement", ["exact", "oblique"])
def test_filters_and_levels(sl, placement):
    T.check_lambda_ranges(T.hold_to_reference(gpu_pictures(sl, R.filter_cases(placement))), placement)


def test_chain_ends_and_uneven_chains(sl):
    T.check_chain_ends(T.hold_to_reference(gpu_pictures(sl, R.chain_cases())))


def test_orientation_known_answer(sl):
    pics = gpu_pictures(sl, [R.orientation_case()])
    T.check_orientation(pics[0][2], pics[0][4])
    T.hold_to_reference(pics)


def test_srgb_decode_known_answer(sl):
    pics = gpu_pictures(sl, [R.srgb_case()])
    T.check_srgb(pics[0][2], pics[0][4])
    T.hold_to_reference(pics)


def test_normal_maps(sl):
    T.check_normal_maps_act(T.hold_to_reference(gpu_pictures(sl, R.normal_cases())))


def test_metallic_roughness_and_emissive(sl):
    T.hold_to_reference(gpu_pictures(sl, R.channel_cases()))


def test_occlusion_scales_the_light_map_part(sl, light_map):
    T.check_occlusion(gpu_pictures(sl, R.occlusion_cases(), light_map))


def test_sticker(sl):
    T.check_sticker_in_view(T.hold_to_reference(gpu_pictures(sl, R.sticker_cases())))


def test_lobe_off_the_axis(sl):
    T.check_lobe_geometry(T.hold_to_reference(gpu_pictures(sl, R.lobe_cases())))


def test_two_shading_forms_give_the_same_bits_on_textured_cases(sl):
    """The default and the reference form of k_shade (SLHIP_SHADE_REFERENCE, tests/test_gpu_shade_paths.py) on textured quads:
    nearest and trilinear base textures, a normal map, the channels and the sticker -- float image and normals, bit for bit."""
    cases = [R.size_cases(5, 6)[0], R.filter_cases("oblique")[5], R.normal_cases()[9], R.channel_cases()[2], R.sticker_cases()[1]]
    saved = os.environ.pop("SLHIP_SHADE_REFERENCE", None)
    try:
        default = gpu_pictures(sl, cases)
        os.environ["SLHIP_SHADE_REFERENCE"] = "1"
        reference = gpu_pictures(sl, cases)
    finally:
        os.environ.pop("SLHIP_SHADE_REFERENCE", None)
        if saved is not None:
            os.environ["SLHIP_SHADE_REFERENCE"] = saved
    for a, b in zip(default, reference):
        assert (a[4] == 1).sum() >= R.MIN_COMPARED
        for k in (2, 3, 4, 5):
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (a[0].name, k)
    torch.cuda.synchronize()
