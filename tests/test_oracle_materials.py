"""CPU: the ORACLE's material stage (texture2D, sRGB decode, normal maps, metallic-roughness / emissive / occlusion channels, the
sticker, the direct-light lobe of oracle/render_ref.c) against the float64 definition of tests/material_ref.py, which shares no code
with it.  Every case checks every covered pixel of the float image (rgb and alpha) and of the normals output against
|got - ref| <= 1e-3 |ref| + S + 1e-6 (material_ref's docstring derives S) and prints the share of that bound its worst pixel uses
and the share of pixels left out as near-ties; tests/test_gpu_materials_known.py holds the kernels to the same bound.

Measured: share of the bound used by the worst pixel of a group (near-ties as a share of the covered pixels), the oracle on the
CPU / the kernels on an MI355X -- the two sides agree to the last digit shown:
  texture sizes and wraps (42 cases)        0.013 / 0.013   (0 %)
  filters and levels, exact (24)            0.053 / 0.053   (0 %)
  filters and levels, oblique (12)          0.669 / 0.669   (at most 0.58 %)
  chain ends and uneven chains (17)         0.359 / 0.359   (0 %)
  orientation, sRGB                         0.000 / 0.000   (sRGB closed form: 7e-8 / 1e-8 relative)
  normal maps (14)                          0.267 / 0.267   (0 %)
  metallic-roughness, emissive (3)          0.031 / 0.031   (0 %)
  occlusion                                 0.000 / 0.000
  sticker (2)                               0.007 / 0.007   (0 %)
  lobe (14)                                 0.034 / 0.034   (0 %)
A first run had "normal oblique (128, 40, 200) w +1" at 1.74: there the mapped normal stands at right angles to the view (N'.V =
4e-5) and the corner snap of the oblique placement, which moves the point on the face and with it the view vector, is all the
value consists of.  The derivation had moved uv alone; material_ref now moves the world point with it (its docstring).  Likewise
the 1e-5 m sanity check of the object coordinates allows for that move on the oblique placement (1.8e-5 m was measured).
Deliberate errors in a scratch copy of render_ref.c, each caught: g and b of the metallic-roughness texel swapped
(test_metallic_roughness_and_emissive), v -> 1 - v (12 tests, test_orientation_known_answer among them), the negative remainder
not wrapped (11), tangent.w ignored (test_normal_maps), ^2.2 before filtering (13), k = r^2 / 2 (test_normal_maps,
test_metallic_roughness_and_emissive, test_lobe_off_the_axis).
"""
import numpy as np
import pytest

import material_ref as R
from stillleben_amd import _abi
from stillleben_amd._batch import HostPool, build_batch


class HostLightMap:
    """What the host builder reads of an sl.LightMap (tests/test_oracle_ibl.py): slot 0 of the oracle's pool, no lights."""
    _slot = 0
    light_directions = []
    light_colors = []


def constant_equirect():
    return np.broadcast_to(np.asarray(R.LIGHT_MAP_RADIANCE, np.float32), (4, 8, 3)).copy()


@pytest.fixture(scope="module")
def light_map(oracle):
    import ibl_analytic as A

    return oracle.light_map_build(constant_equirect(), A.SIZES_COARSE), A.SIZES_COARSE


def oracle_pictures(sl, oracle, cases, light_map=None):
    """[(case, scene, hdr, normals, instance, coord)]: one oracle render of the whole list."""
    scenes = [R.build_scene(sl, c, HostLightMap() if c.light_map else None) for c in cases]
    pool = HostPool()
    srec, drec, _ = build_batch(scenes, pool, with_shadows=False)
    r = oracle.render(pool.arrays(), srec, drec, R.W, R.H, _abi.OUT_ALL, want_hdr=True, light_maps=[light_map] if light_map else None)
    return [(c, s, r.hdr[k], r.normals[k], r.instance[k, :, :, 0], r.coord[k]) for k, (c, s) in enumerate(zip(cases, scenes))]


def hold_to_reference(pictures):
    """Compares every picture with the definition; all figures are printed before the first assertion."""
    figs = []
    print()
    for case, scene, hdr, normals, instance, coord in pictures:
        ref = R.evaluate(case, scene)
        figs.append((case, ref, R.compare(case, ref, hdr, normals, instance, coord)))
    for _, _, fig in figs:
        R.check(fig)
    return figs


# ---- the definition's own parts ---------------------------------------------------------------------------------------------------
def test_wrap_modes_for_any_integer():
    i = np.arange(-13, 14)
    assert list(R.wrap(i, 3, R.REPEAT)) == [(k % 3 + 3) % 3 for k in i]
    assert list(R.wrap(i, 3, R.CLAMP)) == [min(max(k, 0), 2) for k in i]
    period = [0, 1, 2, 2, 1, 0]
    assert list(R.wrap(i, 3, R.MIRROR)) == [period[(k % 6 + 6) % 6] for k in i]
    assert list(R.wrap([-1, 0, 1], 1, R.MIRROR)) == [0, 0, 0]


def all_case_textures():
    cases = [c for s in R.SIZES for c in R.size_cases(*s)] + R.filter_cases("exact") + R.chain_cases() + R.normal_cases() + \
        R.channel_cases() + R.occlusion_cases() + R.sticker_cases() + [R.orientation_case(), R.srgb_case()]
    seen = {}
    for c in cases:
        for img, _ in c.tex.values():
            seen[img.shape[:2], img.tobytes()] = img
    return list(seen.values())


def test_chain_is_what_the_host_pool_lays_out():
    imgs = all_case_textures()
    assert {(i.shape[1], i.shape[0]) for i in imgs} >= set(R.SIZES) | {(2, 1), (2, 2), (3, 2)}
    for img in imgs:
        levels = R.mip_chain(img)
        assert len(levels) == 1 + int(np.floor(np.log2(max(img.shape[:2]))))
        R.check_chain_layout(img, levels)
    # the sizes at which the axes reach one texel at different levels
    assert [lv.shape[:2] for lv in R.mip_chain(R.distinct_texture(7, 2))] == [(2, 7), (1, 3), (1, 1)]
    assert [lv.shape[:2] for lv in R.mip_chain(R.distinct_texture(1, 4))] == [(4, 1), (2, 1), (1, 1)]


def test_distinct_textures_are_distinct():
    for w, h in R.SIZES[1:]:
        t = R.distinct_texture(w, h).reshape(-1, 4)
        for c in range(4):                                         # (alpha has 116 values to give, the 16 x 16 texture 256 texels)
            assert len(set(t[:, c])) >= min(w * h, 100)
        assert len({tuple(x) for x in t}) == w * h and t[:, 3].min() >= 140


# ---- the oracle against it ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", R.SIZES, ids=["%dx%d" % s for s in R.SIZES])
def test_texture_sizes_and_wraps(sl, oracle, size):
    figs = hold_to_reference(oracle_pictures(sl, oracle, R.size_cases(*size)))
    for case, ref, _ in figs:
        g = ref["geometry"]
        assert g["u"].min() < -1.0 and g["u"].max() > 1.0 and g["v"].min() < -1.0          # negative indices and a second period


def check_lambda_ranges(figs, placement):
    for case, ref, _ in figs:
        lam = ref["lambda"]["base"][ref["inside"]]
        if placement == "oblique":
            assert lam.min() < 0.0 and lam.max() >= 2.0, (case.name, lam.min(), lam.max())
        elif "magnified" in case.name:
            assert lam.max() < 0.0
        else:
            assert lam.min() > 1.0


@pytest.mark.parametrize("placement", ["exact", "oblique"])
def test_filters_and_levels(sl, oracle, placement):
    figs = hold_to_reference(oracle_pictures(sl, oracle, R.filter_cases(placement)))
    check_lambda_ranges(figs, placement)


def check_chain_ends(figs):
    for case, ref, _ in figs:
        lam, top = ref["lambda"]["base"][ref["inside"]], len(case.chains["base"]) - 1
        if case.name.startswith("beyond"):
            assert lam.min() > top + 1.0                                     # the clamp to the last level is what is read
        elif "oblique" not in case.name:
            assert 0.0 < lam.min() and lam.max() < top + 1.5


def test_chain_ends_and_uneven_chains(sl, oracle):
    check_chain_ends(hold_to_reference(oracle_pictures(sl, oracle, R.chain_cases())))


def check_orientation(hdr, instance):
    """Known answer, no sampler of the definition involved.  Texel row 0 (red, green) lies at v < 0.5, which is the quad's y < 0:
    with the quad's +y up in the picture that is the LOWER half of the screen; u < 0.5 is the left half."""
    assert (instance[:, 16:80] == 1).all()
    quadrant = {"lower left": (hdr[32:, 16:48], (1, 0, 0)), "lower right": (hdr[32:, 48:80], (0, 1, 0)),
                "upper left": (hdr[:32, 16:48], (0, 0, 1)), "upper right": (hdr[:32, 48:80], (1, 1, 0))}
    for name, (px, colour) in quadrant.items():
        assert (px == np.array(colour + (1,), np.float32)).all(), name


def test_orientation_known_answer(sl, oracle):
    pics = oracle_pictures(sl, oracle, [R.orientation_case()])
    check_orientation(pics[0][2], pics[0][4])
    hold_to_reference(pics)


def check_srgb(hdr, instance):
    want = np.array(R.AMBIENT) * np.array(R.SRGB_BASE[:3]) * (128.0 / 255.0) ** 2.2
    err = np.abs(hdr[instance == 1][:, :3] - want) / want
    print("sRGB decode: largest relative error %.3g" % err.max())
    assert err.max() <= R.RTOL and (hdr[instance == 1][:, 3] == 1.0).all()


def test_srgb_decode_known_answer(sl, oracle):
    pics = oracle_pictures(sl, oracle, [R.srgb_case()])
    check_srgb(pics[0][2], pics[0][4])
    hold_to_reference(pics)


def check_normal_maps_act(figs):
    """The cases are no no-ops: the two signs of tangent.w give different normals unless the map's y is (nearly) zero, and the
    blend of the 2 x 1 map is normalised after filtering (the two texels' own unit normals, blended, would differ)."""
    by_name = {c.name: ref for c, ref, _ in figs}
    for placement in ("exact", "oblique"):
        for texel in R.NORMAL_TEXELS:
            a = by_name["normal %s %s w %+g" % (placement, texel, 1.0)]["normals"]
            b = by_name["normal %s %s w %+g" % (placement, texel, -1.0)]["normals"]
            assert (np.abs(a - b).max() > 0.1) == (texel[1] != 128), texel


def test_normal_maps(sl, oracle):
    check_normal_maps_act(hold_to_reference(oracle_pictures(sl, oracle, R.normal_cases())))


def test_metallic_roughness_and_emissive(sl, oracle):
    hold_to_reference(oracle_pictures(sl, oracle, R.channel_cases()))


def check_occlusion(pictures):
    """The light-map part with a constant occlusion texture of value o 255 is o times the part without the texture."""
    (_, _, plain, _, inst, _), (_, _, lit, _, _, _), (_, _, occluded, _, _, _) = pictures
    m = inst == 1
    part, part_o = (lit.astype(np.float64) - plain)[m][:, :3], (occluded.astype(np.float64) - plain)[m][:, :3]
    assert m.sum() >= R.MIN_COMPARED and part.min() > 0.05                      # the map lights the face
    want = (R.OCCLUSION_VALUE / 255.0) * part
    # both parts are differences of float32 pictures: each picture's rounding (2^-24 relative) enters the bound
    slack = 2.0 ** -23 * (np.abs(lit[m][:, :3]) + np.abs(occluded[m][:, :3]) + 2 * np.abs(plain[m][:, :3]))
    share = (np.abs(part_o - want) / (R.RTOL * want + slack + R.ATOL)).max()
    print("\nocclusion: share of bound %.3f, pixels %d" % (share, m.sum()))
    assert share <= 1.0
    assert (lit[m][:, 3] == 1.0).all() and (occluded[m][:, 3] == 1.0).all()


def test_occlusion_scales_the_light_map_part(sl, oracle, light_map):
    check_occlusion(oracle_pictures(sl, oracle, R.occlusion_cases(), light_map))


def check_sticker_in_view(figs):
    import copy

    import stillleben_amd as sl

    for case, ref, _ in figs:
        # part of the face lies inside the range and part outside; transparent and half-transparent texels make alpha vary
        bare = copy.copy(case)
        bare.sticker = None
        changed = (np.abs(ref["hdr"] - R.evaluate(bare, R.build_scene(sl, bare))["hdr"]).max(-1) > 1e-3)[ref["inside"]]
        assert 0.25 < changed.mean() < 0.75, changed.mean()
        assert len(np.unique(np.round(ref["hdr"][ref["inside"]][:, 3], 3))) > 20


def test_sticker(sl, oracle):
    check_sticker_in_view(hold_to_reference(oracle_pictures(sl, oracle, R.sticker_cases())))


def check_lobe_geometry(figs):
    """Where the issue's constraints on the lights are verified: on the two lowest roughness values N.H <= 0.995 everywhere; the
    grazing case reaches the 0.001 floor of the denominator; the back face has its normal negated."""
    for case, ref, _ in figs:
        g = ref["geometry"]
        V = R._unit(g["cam_position"] - g["world"])[ref["inside"]]
        N = ref["normals"][ref["inside"]][:, :3] @ g["world_to_cam"]            # back to the world frame
        for d, _ in case.lights:
            L = -d / np.linalg.norm(d)
            NoH = np.sum(N * R._unit(V + L), -1)
            if case.roughness <= 0.3:
                assert NoH.max() <= 0.995, case.name
            if case.name == "lobe grazing":
                assert (4 * np.sum(N * V, -1) * (N @ L)).max() < 0.001 and (N @ L).min() > 0
        assert (np.sum(N * V, -1) > 0).all()
        if case.placement == "back":
            assert (N @ (g["o2w"][:3, :3] @ np.array([0.0, 0.0, 1.0])) < -0.999).all()


def test_lobe_off_the_axis(sl, oracle):
    check_lobe_geometry(hold_to_reference(oracle_pictures(sl, oracle, R.lobe_cases())))
