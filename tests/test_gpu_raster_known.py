"""The kernels' geometric G-buffer against the float64 ray cast of tests/raster_ref.py, with no oracle in the loop: the same
scenes, exclusions, caps, bound and per-scene assertions as tests/test_oracle_raster_known.py (raster_ref.check), on what
Engine.render returns.  Beyond that file: several scenes in one launch, the amodal masks and their pixel counts against the
reference's any-hit masks, and the device-built records of a SceneBatch against rays cast from its object_to_camera.

The worst error-to-bound ratios (run with -s) are those of the CPU file: kernels and oracle are bit-equal on these channels
(tests/test_gpu_render.py), so a ratio that differs from the CPU file's is itself a finding."""
import numpy as np
import pytest
import torch

import raster_ref as R
from stillleben_amd import _abi

pytestmark = pytest.mark.gpu

GEOMETRY = _abi.OUT_ALL & ~_abi.OUT_RGB
TABLE_BAND = 0.002        # batch path: hits this close to the table's plane, which the reference does not hold, are left out


@pytest.fixture(scope="module")
def eng(sl):
    from stillleben_amd._context import engine

    return engine()


def render(eng, scene_list, **kw):
    bufs = eng.render(scene_list, GEOMETRY, ssao=False, shadows=False, **kw)
    torch.cuda.synchronize()
    return bufs


@pytest.mark.parametrize("name", sorted(R.SCENES))
def test_scene_against_ray_cast(sl, eng, name):
    scene, ref = R.reference(sl, name)
    R.check(name, ref, R.channels_of(render(eng, [scene])))


@pytest.mark.parametrize("name", ["interpenetrating", "smooth"])
def test_depth_peel_second_layer(sl, eng, name):
    """Scene 9: the layer behind the first one against the reference's definition of it."""
    scene, first = R.reference(sl, name)
    b0 = render(eng, [scene])
    layer0 = R.channels_of(b0)                                         # on the host before the buffers are rendered into again
    R.check(name, first, layer0)
    b1 = render(eng, [scene], depth_peel=b0.coord.clone())
    ref = R.cast(R.soup_from_scene(scene), peel=(first, layer0["coord"][:, :, 3]))
    R.check(name + " peeled", ref, R.channels_of(b1))
    assert (ref.covered & ref.keep & (ref.tri != first.tri)).sum() > 300


def test_several_scenes_in_one_launch(sl, eng):
    """Scene 10: scenes 1, 2 and 4 at one size as one batch, each against its own reference."""
    pairs = [R.reference(sl, name) for name in R.BATCH]
    assert len({scene.viewport for scene, _ in pairs}) == 1
    bufs = render(eng, [scene for scene, _ in pairs])
    for b, (name, (_, ref)) in enumerate(zip(R.BATCH, pairs)):
        R.check(name, ref, R.channels_of(bufs, b), label="%s (scene %d of the batch)" % (name, b))


@pytest.mark.parametrize("name", ["clutter3", "clutter21", "clutter8", "interpenetrating", "coincident"])
def test_amodal_masks_against_any_hit(sl, eng, name):
    """Scenes 1 and 7 with object_masks: off the object's own projected edges (margin (a)) the "all" mask of every object is the
    reference's any-hit mask of it -- every pixel whose ray meets the object between the near and the far plane, hidden or not;
    the "visib" mask is instance == slot of the same picture; px_count_all lies between the any-hit count without and with the
    margin pixels."""
    scene, ref = R.reference(sl, name)
    bufs = render(eng, [scene], object_masks=True)
    om = bufs.object_masks
    inst = R.channels_of(bufs)["instance"]
    slots = sorted(ref.any_hit)
    assert slots == [o.instance_index for o in scene.objects] and om.n_slots == slots[-1] + 1
    whole = om.dense("all", scenes=[0], slots=slots)[0].cpu().numpy()
    visib = om.dense("visib", scenes=[0], slots=slots)[0].cpu().numpy()
    count = om.stats.px_count_all[0].cpu().numpy()
    hidden = 0
    for k, i in enumerate(slots):
        hit, near = ref.any_hit[i], ref.edge_near[i]
        bad = (whole[k] != hit) & ~near
        assert not bad.any(), "%s: the whole mask of object %d differs from the any-hit mask at (row, col) %s" % (name, i, np.argwhere(bad)[0])
        assert np.array_equal(visib[k], inst == i)
        assert (hit & ~near).sum() <= count[i] <= (hit | near).sum(), (i, (hit & ~near).sum(), count[i], (hit | near).sum())
        assert near.sum() <= R.LEFT_OUT_CAP * hit.sum()
        hidden += int((hit & ~near & (ref.instance != i) & ref.keep).sum())
    assert hidden > 50                                                 # amodal: the masks hold pixels another object owns


def test_scene_batch_records_against_object_to_camera(sl, eng):
    """The device-built records (slhip_synth_place) against the pictures: 3 scenes x 4 cubes of test_gpu_synth.small_table,
    settled for 5 frames; the reference casts rays from batch.object_to_camera, the table's meshes and the batch's intrinsics
    alone (no world frame: no normals).  The objects are the table's three cubes: the reference walks the triangles one by one,
    and the table's fourth mesh has 69 451 of them.  The table's plane is drawn and is not in the reference: compared are the
    pixels the reference gives to an object; those whose hit lies within 2 mm of the plane (whose height and camera are the
    batch's) are left out and count against the cap.  So do hits MORE than 2 mm under the plane's top -- a corner that the short
    settle leaves sunk into the table: the camera is above the table, the table hides them, and the picture must show the table
    (instance 0) there."""
    from test_gpu_synth import small_table

    table = small_table(sl)
    ids = np.array([[0, 1, 2, 0], [1, 2, 0, 1], [2, 0, 1, 2]])
    batch = sl.SceneBatch(table, 3, 4, resolution=(320, 240), seed=11, asset_ids=ids)
    batch.stage()
    batch.settle(frames=5)
    batch.check_settled()
    batch.place(object_to_camera=True)
    bufs = batch.render(0, mask=GEOMETRY, ssao=False)
    torch.cuda.synchronize()
    o2c = batch.object_to_camera.cpu().numpy().astype(np.float64)
    cams = batch.host_cameras().astype(np.float64)
    plane_z = float(batch.params["plane_z"])
    W, H = batch.resolution
    for b in range(3):
        parts = []
        for k in range(4):
            m = np.eye(4)
            m[:3] = o2c[b, k]
            parts.append((table.meshes[ids[b, k]], m, k + 1, None))
        ref = R.cast(R.soup_from_parts(parts, batch.intrinsics(), (W, H)))
        world_z = ref.cam_coord[..., :3] @ cams[b][2, :3] + cams[b][2, 3]
        assert cams[b][2, 3] > plane_z + 0.1                            # the camera looks down on the table
        band = ref.covered & (np.abs(world_z - plane_z) <= TABLE_BAND)
        sunk = ref.covered & (world_z < plane_z - TABLE_BAND)
        out = R.channels_of(bufs, b)
        assert (out["instance"][sunk & ref.keep] == 0).all()
        fig = R.compare(ref, out, label="batch scene %d" % b, only=ref.covered, extra_left=band | sunk)
        R.report("batch scene %d" % b, fig)
        R.assert_within(fig, "batch scene %d" % b)
