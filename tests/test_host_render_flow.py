"""Render flow on the host (slhip_render_flow_host, slhip_render_flow_motion_host, sl.render_flow) against the NumPy restatement
tests/render_flow_ref.py -- bit for bit in float32 -- and against known answers in float64.

The float tolerance cannot be derived in closed form; as for the rigid fit it is measured on the RESTATEMENT, not on the library:
over all seeded known-answer cases below (320 x 240, the intrinsics of the device tests' batch, depths of 0.4 .. 3 m) the float32
restatement deviates from the float64 answer by at most
    flow        3.7e-4 px      (MEASURED_FLOW;   the library is held to 4 x that, T_FLOW)
    scene flow  3.6e-7 m       (MEASURED_SCENE;  T_SCENE)
    motion      4.1e-7         (MEASURED_MOTION, entries of the 3 x 4; T_MOTION)
test_the_bounds_are_four_times_the_restatements_worst recomputes the three and holds the constants to them."""
import os
import re

import numpy as np
import pytest

import render_flow_ref as R
from stillleben_amd import _abi
from stillleben_amd import render_flow as rf

F = np.float32
MEASURED_FLOW, MEASURED_SCENE, MEASURED_MOTION = 3.7e-4, 3.6e-7, 4.1e-7
T_FLOW, T_SCENE, T_MOTION = 4 * MEASURED_FLOW, 4 * MEASURED_SCENE, 4 * MEASURED_MOTION
ALL = ("flow", "scene_flow", "flags", "counts")
INTRINSICS, SIZE = (533.4, 533.7, 156.5, 120.6), (320, 240)      # the batch of the device tests
POISON = 0x5B


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(bits(got), bits(want))


def rigid(rng, angle, shift, n=None):
    """float64 [n, 3, 4] (or [3, 4]): rotations by up to `angle` rad about random axes, translations up to `shift`"""
    m = 1 if n is None else n
    axis = rng.normal(size=(m, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    a = rng.uniform(-angle, angle, m)
    K = np.zeros((m, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 2] = -axis[:, 2], axis[:, 1], -axis[:, 0]
    K -= np.swapaxes(K, 1, 2)
    Rm = np.eye(3) + np.sin(a)[:, None, None] * K + (1 - np.cos(a))[:, None, None] * (K @ K)
    out = np.concatenate([Rm, rng.uniform(-shift, shift, (m, 3, 1))], axis=2)
    return out[0] if n is None else out


def seeded_case(W, H, S, B=3, seed=0):
    """Everything the rules branch on, at random: (depth_a, instance_a, table, depth_b, instance_b), float32 / int16.  Scene 1
    (when there is one) has a NaN row in its motion table."""
    rng = np.random.default_rng(1000 * seed + 7 * W + H + S)
    depth_a = rng.uniform(0.5, 3.0, (B, H, W)).astype(F)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -1.0, 3000.0, 2999.0, 1e30], F)
    hit = rng.random((B, H, W)) < 0.1
    depth_a[hit] = rng.choice(special, int(hit.sum()))
    instance_a = rng.integers(0, S + 2, (B, H, W)).astype(np.int16)
    instance_a[rng.random((B, H, W)) < 0.03] = -1
    table = rigid(rng, 0.05, 0.15, B * S).reshape(B, S, 3, 4).astype(F)
    if B > 1:
        table[1, S // 2, 1, 2] = np.nan
    depth_b = (depth_a + rng.normal(0, 0.05, (B, H, W))).astype(F)
    depth_b[rng.random((B, H, W)) < 0.05] = np.nan
    instance_b = np.where(rng.random((B, H, W)) < 0.7, instance_a, rng.integers(0, S + 1, (B, H, W))).astype(np.int16)
    return depth_a, instance_a, table, depth_b, instance_b


def as_coord(depth, seed=1):
    """the plane as the w of a coord target whose xyz is noise"""
    c = np.random.default_rng(seed).normal(size=depth.shape + (4,)).astype(F)
    c[..., 3] = depth
    return c


def edge_case():
    """8 x 8 at depth 1 with fx = fy = 64, cx = cy = 4: every product is exact.  Slot s moves its pixels by half a pixel:
    0 left, 1 right, 2 down, 3 up.  Columns 0 and 7 and rows 0 and 7 land exactly on u = 0, u = W, v = H and v = 0."""
    W = H = 8
    depth = np.ones((1, H, W), F)
    inst = np.zeros((1, H, W), np.int16)
    inst[0, :, 4:] = 1                     # the right half moves right: x = 7 lands on u = 8 = W
    inst[0, 6:, 2:6] = 2                   # the bottom rows move down: y = 7 lands on v = 8 = H
    inst[0, :2, 2:6] = 3                   # the top rows move up: y = 0 lands on v = 0
    table = np.zeros((1, 4, 3, 4), F)
    table[..., :3] = np.eye(3)
    table[0, 0, 0, 3], table[0, 1, 0, 3], table[0, 2, 1, 3], table[0, 3, 1, 3] = -1 / 128, 1 / 128, 1 / 128, -1 / 128
    return (64.0, 64.0, 4.0, 4.0), depth, inst, table


def occlusion_case():
    """64 x 32, fx = fy = 64, cx = 32, cy = 16: a plane at depth 2 (instance 0, static camera), a square of 16 x 16 pixels at depth
    1 (instance 1) that moves by 0.25 m = 16 px to the right, and a square of 8 x 8 pixels at depth 1 in the bottom right corner
    (instance 2) that moves the same way, out of the picture.  Powers of two throughout: every product is exact."""
    W, H = 64, 32
    depth_a, inst_a = np.full((1, H, W), 2.0, F), np.zeros((1, H, W), np.int16)
    depth_a[0, 8:24, 16:32], inst_a[0, 8:24, 16:32] = 1.0, 1
    depth_a[0, 24:32, 56:64], inst_a[0, 24:32, 56:64] = 1.0, 2
    depth_b, inst_b = np.full((1, H, W), 2.0, F), np.zeros((1, H, W), np.int16)
    depth_b[0, 8:24, 32:48], inst_b[0, 8:24, 32:48] = 1.0, 1
    table = np.zeros((1, 3, 3, 4), F)
    table[..., :3] = np.eye(3)
    table[0, 1:, 0, 3] = 0.25
    return (64.0, 64.0, 32.0, 16.0), depth_a, inst_a, table, depth_b, inst_b


def params_of(intrinsics, depth, table, **kw):
    return rf.check_params(rf.make_params(intrinsics, (depth.shape[2], depth.shape[1]), table.shape[1], **kw))[0]


# ---- 1. the host twin is the restatement, bit for bit ----------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,S", [(1, 1, 1), (70, 37, 3), (256, 1, 256), (33, 9, 256)])
def test_host_twin_equals_the_restatement(W, H, S):
    depth_a, inst_a, table, depth_b, inst_b = seeded_case(W, H, S)
    intr = (64.0, 61.5, W / 2 + 0.25, H / 2 - 0.125)
    # (the depth as the coord target, a depth of b, an instance plane of b, the instance condition)
    for coord, with_b, with_ib, match in ((False, True, True, True), (True, True, True, False), (True, False, False, True),
                                          (False, True, False, True)):
        kw = dict(max_depth=3000.0, depth_tol=0.01, depth_rel=0.02, match_instance=match, outputs=ALL)
        da = as_coord(depth_a) if coord else depth_a
        db = (as_coord(depth_b, 2) if coord else depth_b) if with_b else None
        ib = inst_b if with_ib else None
        got = rf.compute_host(da, inst_a, table, intr, db, ib, **kw)
        want = R.flow(got.params, da, inst_a, table, db, ib)
        for name, w in zip(ALL, want):
            assert same(getattr(got, name), w), (name, coord, with_b, with_ib, match)
        f = got.flags
        assert (f[(f & 2) != 0] & 1).all() and (f[(f & 4) != 0] & 2).all()      # visible -> inside -> valid
        assert not got.flow[f == 0].any() and not got.scene_flow[f == 0].any()
        if (W, H) == (70, 37):
            assert got.counts[:, :, 1].sum() > 1000 and got.counts[:, :, 2].sum() > 500 and (not with_b or got.counts[:, :, 3].sum() > 100)
        if not with_b:
            assert not (f & 4).any() and not got.counts[:, :, 3].any()
        if S == 3:
            assert got.counts[1, 1].tolist()[1:] == [0, 0, 0] and got.counts[1, 1, 0] > 0      # the NaN row: pixels, none valid


def test_counts_are_the_bincount_of_the_flags():
    depth_a, inst_a, table, depth_b, inst_b = seeded_case(70, 37, 3, seed=2)
    got = rf.compute_host(depth_a, inst_a, table, (64.0, 64.0, 35.0, 18.5), depth_b, inst_b, outputs=ALL)
    i = inst_a.view(np.uint16).astype(np.int64)
    for b in range(3):
        for col, bit in enumerate((0, 1, 2, 4)):
            pick = (i[b] < 3) & ((got.flags[b] & bit) != 0 if bit else True)
            assert np.array_equal(got.counts[b, :, col], np.bincount(i[b][pick], minlength=3))
    cov = got.covisibility()
    assert cov.shape == (3, 3) and np.isnan(cov[1, 1]) and np.allclose(cov[0], got.counts[0, :, 3] / got.counts[0, :, 1])


def test_motion_twin_equals_the_restatement():
    rng = np.random.default_rng(5)
    a, b = rigid(rng, 3.0, 2.0, 200).astype(F), rigid(rng, 3.0, 2.0, 200).astype(F)
    a[3, 1, 2], b[9, 2, 3], a[11, 0, 0] = np.nan, np.inf, -np.inf
    got = rf.motion_host(a, b)
    assert same(got, R.motion(a, b))
    assert np.isnan(got[[3, 9, 11]]).all() and np.isfinite(np.delete(got, [3, 9, 11], axis=0)).all()
    four = np.concatenate([a, np.broadcast_to(np.array([[[0, 0, 0, 1]]], F), (200, 1, 4))], axis=1)      # [.., 4, 4]: rows 0-2 taken
    assert same(rf.motion_host(four.reshape(10, 20, 4, 4), b.reshape(10, 20, 3, 4)), got.reshape(10, 20, 3, 4))
    assert rf.motion_host(a[:0], b[:0]).shape == (0, 3, 4)


# ---- 2. known answers in float64 -------------------------------------------------------------------------------------------------
def known_cases():
    """(name, depth [1, H, W] f32, the motion float32 [3, 4], answer(px, py, z) -> (u, v) in float64 from the float32 motion's
    own entries, or None)"""
    W, H = SIZE
    fx, fy, cx, cy = (float(F(v)) for v in INTRINSICS)
    rng = np.random.default_rng(11)
    eye = np.eye(3, 4, dtype=F)
    bumpy = rng.uniform(0.4, 3.0, (1, H, W)).astype(F)
    out = [("identity", bumpy, eye, lambda px, py, z: (px, py))]
    for Z, tx, ty in ((0.75, 0.03, -0.02), (2.5, -0.11, 0.07)):
        m = eye.copy()
        m[0, 3], m[1, 3] = tx, ty
        out.append(("plane %g" % Z, np.full((1, H, W), Z, F), m,
                    lambda px, py, z, Z=float(F(Z)), tx=float(m[0, 3]), ty=float(m[1, 3]): (px + fx * tx / Z, py + fy * ty / Z)))
    for th in (0.02, -0.3):
        m = eye.copy()
        c, s = np.cos(th), np.sin(th)
        m[:2, :2] = [[c, -s], [s, c]]
        q = m.astype(np.float64)
        out.append(("roll %g" % th, bumpy, m, lambda px, py, z, q=q: (q[0, 0] * (px - cx) + q[0, 1] * (py - cy) * fx / fy + cx,
                                                                     q[1, 0] * (px - cx) * fy / fx + q[1, 1] * (py - cy) + cy)))
    for tz in (0.1, -0.2):
        m = eye.copy()
        m[2, 3] = tz
        out.append(("dolly %g" % tz, bumpy, m, lambda px, py, z, tz=float(m[2, 3]): ((px - cx) * z / (z + tz) + cx, (py - cy) * z / (z + tz) + cy)))
    out.append(("general", bumpy, rigid(rng, 0.1, 0.1).astype(F), None))
    return out


def pixel_centres():
    W, H = SIZE
    return (np.arange(W) + 0.5)[None, None, :], (np.arange(H) + 0.5)[None, :, None]


def same_frame_twice():
    """motion(T, T) of seeded rigid frames two metres off is the identity up to rounding: (depth, instances, the frames)"""
    W, H = SIZE
    rng = np.random.default_rng(12)
    frames = rigid(rng, 3.0, 2.0, 8)
    depth = rng.uniform(0.4, 3.0, (1, H, W)).astype(F)
    inst = rng.integers(0, 8, (1, H, W)).astype(np.int16)
    return depth, inst, frames.astype(F)


def deviations(flow_of, motion_of):
    """The worst deviation from the float64 answers over all seeded cases of `flow_of(depth, inst, table32, **kw)` -> (flow,
    scene_flow, flags) and `motion_of(from32, to32)`: (flow px, scene flow m, motion entries)."""
    px, py = pixel_centres()
    worst_f = worst_s = 0.0
    for name, depth, table, answer in known_cases():
        inst = np.zeros(depth.shape, np.int16)
        t32 = table[None, None]
        fl, sf, flags = flow_of(depth, inst, t32)
        # the float64 answer of the float32 inputs: the table as the library gets it
        want_f, want_s, want_flags, _ = R.flow(params_of(INTRINSICS, depth, t32, outputs=ALL), depth, inst, t32.astype(np.float64), T=np.float64)
        assert (flags & 1).all() and (want_flags & 1).all(), name
        if answer is not None:
            u, v = np.broadcast_arrays(*answer(px, py, depth.astype(np.float64)), depth)[:2]
            assert np.abs(want_f - np.stack([u - px, v - py], axis=-1)).max() < 1e-9, name
        worst_f = max(worst_f, float(np.abs(fl - want_f).max()))
        worst_s = max(worst_s, float(np.abs(sf - want_s).max()))
    depth, inst, frames = same_frame_twice()
    fl, sf, flags = flow_of(depth, inst, motion_of(frames, frames)[None])
    assert (flags & 1).all()
    worst_f, worst_s = max(worst_f, float(np.abs(fl).max())), max(worst_s, float(np.abs(sf).max()))
    rng = np.random.default_rng(13)
    a, b = rigid(rng, 3.0, 2.0, 500), rigid(rng, 3.0, 2.0, 500)
    a4 = np.concatenate([a.astype(F).astype(np.float64), np.broadcast_to([[[0.0, 0, 0, 1]]], (500, 1, 4))], axis=1)
    want_m = b.astype(F).astype(np.float64) @ np.linalg.inv(a4)
    worst_m = float(np.abs(motion_of(a.astype(F), b.astype(F)) - want_m).max())
    return worst_f, worst_s, worst_m


def ref_flow(depth, inst, table):
    return R.flow(params_of(INTRINSICS, depth, table, outputs=ALL), depth, inst, table)[:3]


def lib_flow(depth, inst, table):
    r = rf.compute_host(depth, inst, table, INTRINSICS, outputs=ALL)
    return r.flow, r.scene_flow, r.flags


def test_the_bounds_are_four_times_the_restatements_worst():
    worst = deviations(ref_flow, R.motion)
    print("restatement vs float64: flow %.3g px, scene flow %.3g m, motion %.3g" % worst)
    for w, m in zip(worst, (MEASURED_FLOW, MEASURED_SCENE, MEASURED_MOTION)):
        assert 0.9 * m <= w <= m, (worst, "the header's numbers are the restatement's worst, to two digits, rounded up")


def test_known_answers():
    """identity, fronto-parallel planes under a sideways camera, rolls about the optical axis, dollies along it (radial flow),
    a general motion and the same frame twice, all against float64; motion() against float64 to @ inv(from)"""
    worst = deviations(lib_flow, rf.motion_host)
    print("library vs float64: flow %.3g px, scene flow %.3g m, motion %.3g" % worst)
    assert worst[0] <= T_FLOW and worst[1] <= T_SCENE and worst[2] <= T_MOTION, worst


def test_closed_forms():
    """what the answers say, on the library's flow: constant under a sideways camera, radial from (cx, cy) under a dolly"""
    px, py = pixel_centres()
    fx, fy, cx, cy = (float(F(v)) for v in INTRINSICS)
    for name, depth, table, answer in known_cases():
        if answer is None:
            continue
        fl = lib_flow(depth, np.zeros(depth.shape, np.int16), table[None, None])[0].astype(np.float64)
        if name.startswith("plane"):
            Z, tx, ty = float(depth[0, 0, 0]), float(table[0, 3]), float(table[1, 3])
            assert np.abs(fl - [fx * tx / Z, fy * ty / Z]).max() <= T_FLOW, name
        if name.startswith("dolly"):
            cross = fl[..., 0] * (py - cy) - fl[..., 1] * (px - cx)            # parallel to the ray from the principal point
            assert np.abs(cross).max() <= T_FLOW * (np.hypot(*SIZE)), name
            away = fl[..., 0] * (px - cx) + fl[..., 1] * (py - cy)
            assert (away < 0).all() if table[2, 3] > 0 else (away > 0).all(), name      # a camera moving back shrinks the picture
        if name == "identity":
            assert np.abs(fl).max() <= T_FLOW


def test_identity_with_b_equal_a_sees_everything():
    depth, inst, _ = same_frame_twice()
    depth[0, :5, :7] = np.nan
    eye = np.zeros((1, 8, 3, 4), F)
    eye[..., :3] = np.eye(3)
    r = rf.compute_host(depth, inst, eye, INTRINSICS, depth, inst, depth_tol=0.0, depth_rel=0.0, outputs=ALL)
    assert np.array_equal(r.valid, np.isfinite(depth)) and np.array_equal(r.visible, r.valid) and not r.occluded.any()
    assert np.array_equal(r.counts[0, :, 1], r.counts[0, :, 3]) and np.nanmin(r.covisibility()) == 1.0


def test_exact_occlusion():
    """Written out by hand.  The plane (instance 0, depth 2, identity): u = px exactly, flow 0, footprint x .. x + 1, y .. y + 1.
    Picture b has the square on columns 32 .. 47, rows 8 .. 23, so the plane pixels whose whole footprint lies on it -- columns
    32 .. 46, rows 8 .. 22: 15 x 15 = 225 -- are occluded (the plane at 2 lies behind the square at 1 by more than depth_tol =
    0.125), and every other plane pixel sees the plane in its footprint.  The square (instance 1, 256 pixels at depth 1):
    X' = X + 0.25, u = px + 16 exactly, it lands on itself in b.  The corner square (instance 2, 64 pixels): u = px + 16 >= 72.5:
    valid, not inside."""
    intr, depth_a, inst_a, table, depth_b, inst_b = occlusion_case()
    for match in (True, False):
        r = rf.compute_host(depth_a, inst_a, table, intr, depth_b, inst_b, depth_tol=0.125, depth_rel=0.0, match_instance=match, outputs=ALL)
        flow = np.zeros((1, 32, 64, 2), F)
        flow[0, 8:24, 16:32, 0] = 16.0
        flow[0, 24:32, 56:64, 0] = 16.0
        scene = np.zeros((1, 32, 64, 3), F)
        scene[..., 0] = flow[..., 0] / F(64.0)                                 # 0.25 m in x where the flow is 16 px
        flags = np.full((1, 32, 64), 7, np.uint8)
        flags[0, 8:23, 32:47] = 3                                              # the plane under the square in b: occluded
        flags[0, 24:32, 56:64] = 1                                             # left the picture
        assert same(r.flow, flow) and same(r.scene_flow, scene) and same(r.flags, flags)
        assert r.counts.tolist() == [[[1728, 1728, 1728, 1503], [256, 256, 256, 256], [64, 64, 0, 0]]]
        assert int(r.occluded.sum()) == 225 and r.covisibility().tolist() == [[F(1503) / F(1728), 1.0, 0.0]]
    # the instance condition alone: with a tolerance that lets the plane through the square, only the instances occlude
    r = rf.compute_host(depth_a, inst_a, table, intr, depth_b, inst_b, depth_tol=1.0, depth_rel=0.0, outputs=ALL)
    assert r.counts[0, 0].tolist() == [1728, 1728, 1728, 1503]
    r = rf.compute_host(depth_a, inst_a, table, intr, depth_b, inst_b, depth_tol=1.0, depth_rel=0.0, match_instance=False, outputs=ALL)
    assert r.counts[0, 0].tolist() == [1728, 1728, 1728, 1728]
    r = rf.compute_host(depth_a, inst_a, table, intr, depth_b, None, depth_tol=0.0, depth_rel=0.5, outputs=ALL)      # 2 <= 1 + 0.5 * 2
    assert r.counts[0, 0].tolist() == [1728, 1728, 1728, 1728]


def test_landings_on_the_border():
    """u = 0 and v = 0 are inside with a footprint clipped at -1; u = W and v = H are outside"""
    intr, depth, inst, table = edge_case()
    r = rf.compute_host(depth, inst, table, intr, depth, inst, depth_tol=0.0, depth_rel=0.0, outputs=ALL)
    want = np.full((1, 8, 8), 7, np.uint8)
    want[0, :, 7] = 1                          # u = 8 = W
    want[0, 7, 2:6] = 1                        # v = 8 = H
    assert same(r.flags, want)
    assert r.flow[0, 3, 0].tolist() == [-0.5, 0.0] and r.flow[0, 3, 7].tolist() == [0.5, 0.0]      # u = 0: inside, x0 = -1
    assert r.flow[0, 0, 3].tolist() == [0.0, -0.5] and r.flow[0, 7, 3].tolist() == [0.0, 0.5]      # v = 0: inside, y0 = -1


# ---- 3. invalid inputs give zeros and flag 0 -------------------------------------------------------------------------------------
def one_bad_pixel(**change):
    depth = np.full((1, 2, 3), 1.5, F)
    inst = np.array([[[0, 1, 2], [2, 1, 0]]], np.int16)
    table = rigid(np.random.default_rng(3), 0.01, 0.002, 3).astype(F)[None]      # a tenth of a pixel
    depth[0, 1, 1] = change.get("z", 1.5)
    inst[0, 1, 1] = change.get("i", 1)
    if "row" in change:
        table[0, 1] = change["row"]
    r = rf.compute_host(depth, inst, table, (64.0, 64.0, 1.5, 1.0), depth, inst, max_depth=change.get("max_depth", 3000.0), outputs=ALL)
    good = np.ones((1, 2, 3), bool)
    good[0, 1, 1] = False
    if "row" in change:
        good &= inst != 1
    assert (r.flags[good] & 1).all() and r.flow[good].any()
    assert not r.flags[~good].any() and not bits(r.flow[~good]).any() and not bits(r.scene_flow[~good]).any()      # +0.0, not -0.0
    return r


@pytest.mark.parametrize("z", [np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, 3000.0, 4000.0])
def test_a_bad_depth_is_not_valid(z):
    r = one_bad_pixel(z=z)
    assert r.counts[0, 1].tolist() == [2, 1, 1, 1]


def test_max_depth_is_exclusive_and_may_be_infinite():
    assert one_bad_pixel(z=2.0, max_depth=2.0).counts[0, 1, 1] == 1
    r = rf.compute_host(np.full((1, 1, 1), 1e30, F), np.zeros((1, 1, 1), np.int16), np.eye(3, 4, dtype=F)[None, None], (64.0, 64.0, 0.5, 0.5),
                        max_depth=np.inf, outputs=ALL)
    assert r.flags[0, 0, 0] == 3


@pytest.mark.parametrize("i", [3, 4, 255, 256, 32767, -1, -32768])
def test_an_instance_outside_the_table_is_not_valid(i):
    r = one_bad_pixel(i=i)
    assert r.counts[0].tolist() == [[2, 2, 2, 2], [1, 1, 1, 1], [2, 2, 2, 2]]      # and it is counted nowhere


@pytest.mark.parametrize("k", range(12))
def test_a_nan_in_the_motion_row_is_not_valid(k):
    row = rigid(np.random.default_rng(4), 0.01, 0.002).astype(F)
    row.reshape(-1)[k] = np.nan if k % 2 else np.inf
    r = one_bad_pixel(row=row)
    assert r.counts[0, 1].tolist() == [2, 0, 0, 0]


def test_a_point_moved_behind_the_camera_is_not_valid():
    row = np.eye(3, 4, dtype=F)
    row[2, 3] = -1.5                                                           # Z' = 1.5 - 1.5 = 0: not in front
    assert one_bad_pixel(row=row).counts[0, 1].tolist() == [2, 0, 0, 0]
    row[2, 3] = -5.0
    assert one_bad_pixel(row=row).counts[0, 1].tolist() == [2, 0, 0, 0]


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------
BAD_FIELDS = [("fx", 0.0), ("fx", -1.0), ("fx", np.nan), ("fx", np.inf), ("fy", 0.0), ("fy", np.nan), ("cx", np.nan), ("cx", np.inf),
              ("cy", -np.inf), ("cy", np.nan), ("W", 0), ("W", -3), ("W", 32769), ("H", 0), ("H", 32769), ("n_slots", 0), ("n_slots", 257),
              ("max_depth", 0.0), ("max_depth", -1.0), ("max_depth", np.nan), ("depth_tol", -1e-6), ("depth_tol", np.nan),
              ("depth_tol", np.inf), ("depth_rel", -1.0), ("depth_rel", np.nan), ("depth_rel", np.inf), ("outputs", 0), ("outputs", 16),
              ("outputs", 31), ("flags", 2), ("flags", 3)]


@pytest.mark.parametrize("field,value", BAD_FIELDS)
def test_check_params_names_the_broken_rule(field, value):
    p = rf.make_params((64.0, 64.0, 4.0, 4.0), (8, 8), 4)
    rf.check_params(p)
    p[field] = value
    with pytest.raises(_abi.SlhipError) as e:
        rf.check_params(p)
    word = {"fx": "intrinsics", "fy": "intrinsics", "cx": "intrinsics", "cy": "intrinsics", "W": "picture size", "H": "picture size",
            "depth_rel": "depth_tol"}.get(field, field)
    assert word in str(e.value)
    assert _abi.lib().slhip_render_flow_check_params(None) < 0


def test_the_limits_themselves_pass():
    for field, value in (("n_slots", 1), ("n_slots", 256), ("W", 32768), ("max_depth", np.inf), ("depth_tol", 0.0), ("outputs", 15), ("flags", 0)):
        p = rf.make_params((64.0, 64.0, 4.0, 4.0), (8, 8), 4)
        p[field] = value
        rf.check_params(p)


def host_call(null=(), B=1, outputs=15, stride_a=1, stride_b=1, **fields):
    """slhip_render_flow_host on the edge case with poisoned outputs: (status, the four outputs)"""
    intr, depth, inst, table = edge_case()
    p = rf.make_params(intr, (8, 8), 4, outputs=outputs).reshape(1)
    for k, v in fields.items():
        p[k] = v
    out = dict(flow=np.full((1, 8, 8, 2), np.nan, F), scene=np.full((1, 8, 8, 3), np.nan, F), flags=np.full((1, 8, 8), POISON, np.uint8),
               counts=np.full((1, 4, 4), -7, np.int32))
    arg = dict(params=p, depth_a=depth, inst_a=inst.view(np.uint16), table=table, depth_b=depth.copy(), inst_b=inst.view(np.uint16).copy(), **out)
    ptr = {k: (None if k in null else v.ctypes.data) for k, v in arg.items()}
    st = _abi.lib().slhip_render_flow_host(ptr["params"], ptr["depth_a"], stride_a, ptr["inst_a"], ptr["table"], ptr["depth_b"], stride_b,
                                           ptr["inst_b"], B, ptr["flow"], ptr["scene"], ptr["flags"], ptr["counts"])
    return st, out


def poisoned(out, names=("flow", "scene", "flags", "counts")):
    want = dict(flow=lambda a: np.isnan(a).all(), scene=lambda a: np.isnan(a).all(), flags=lambda a: (a == POISON).all(),
                counts=lambda a: (a == -7).all())
    return all(want[n](out[n]) for n in names)


REFUSALS = [dict(null=("params",)), dict(null=("depth_a",)), dict(null=("inst_a",)), dict(null=("table",)), dict(null=("flow",)),
            dict(null=("scene",)), dict(null=("flags",)), dict(null=("counts",)), dict(stride_a=0), dict(stride_b=0), dict(B=65536),
            dict(n_slots=0), dict(n_slots=257), dict(outputs=0), dict(outputs=16), dict(W=0), dict(fx=0.0), dict(flags=2)]


@pytest.mark.parametrize("kw", REFUSALS, ids=[str(sorted(k.items())) for k in REFUSALS])
def test_entries_refuse_bad_arguments(kw):
    st, out = host_call(**kw)
    assert st < 0 and _abi.lib().slhip_last_error() and poisoned(out)


def test_no_scenes_succeed_and_write_nothing():
    st, out = host_call(B=0)
    assert st == 0 and poisoned(out)
    st, out = host_call(B=0, null=("depth_a", "flow"))                         # nothing is read either
    assert st == 0 and poisoned(out)
    r = rf.compute_host(np.zeros((0, 4, 5), F), np.zeros((0, 4, 5), np.int16), np.zeros((0, 2, 3, 4), F), (64.0, 64.0, 2.5, 2.0), outputs=ALL)
    assert r.flow.shape == (0, 4, 5, 2) and r.counts.shape == (0, 2, 4)


@pytest.mark.parametrize("mask", range(1, 16))
def test_outputs_not_named_stay_poison(mask):
    names = ("flow", "scene", "flags", "counts")
    st, out = host_call(outputs=mask, null=tuple(n for k, n in enumerate(names) if not mask >> k & 1))      # and may be NULL
    assert st == 0
    st, out = host_call(outputs=mask)
    assert st == 0 and poisoned(out, [n for k, n in enumerate(names) if not mask >> k & 1])
    full = host_call()[1]
    for k, n in enumerate(names):
        if mask >> k & 1:
            assert same(out[n], full[n])
    st, out = host_call(null=("depth_b", "inst_b"))                            # no picture b: nothing visible
    assert st == 0 and not (out["flags"] & 4).any() and not out["counts"][..., 3].any() and (out["flags"] & 1).all()


# ---- 5. the Python surface -------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries_and_abi_stays_5():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "slhip.h")).read()
    for name in ("slhip_render_flow_check_params", "slhip_render_flow", "slhip_render_flow_host", "slhip_render_flow_motion",
                 "slhip_render_flow_motion_host"):
        assert re.search(r"\bint %s\(" % name, text), name
        assert hasattr(_abi.lib(), name)
    assert "Render flow" in text and _abi.ABI_VERSION == 5 and _abi.lib().slhip_abi_version() == 5
    for name, value in (("SLHIP_FLOW_SLOTS_MAX", _abi.FLOW_SLOTS_MAX), ("SLHIP_FLOW_VALID", _abi.FLOW_VALID), ("SLHIP_FLOW_INSIDE", _abi.FLOW_INSIDE),
                        ("SLHIP_FLOW_VISIBLE", _abi.FLOW_VISIBLE), ("SLHIP_FLOW_OUT_FLOW", _abi.FLOW_OUT_FLOW),
                        ("SLHIP_FLOW_OUT_SCENE", _abi.FLOW_OUT_SCENE), ("SLHIP_FLOW_OUT_FLAGS", _abi.FLOW_OUT_FLAGS),
                        ("SLHIP_FLOW_OUT_COUNTS", _abi.FLOW_OUT_COUNTS), ("SLHIP_FLOW_MATCH_INSTANCE", _abi.FLOW_MATCH_INSTANCE)):
        assert re.search(r"#define %s\s+%du?\b" % (name, value), text), name


def test_the_module_is_exported():
    import stillleben as alias
    import stillleben_amd as sl

    assert sl.render_flow is rf and alias.render_flow is rf and sl.RenderFlow is rf.RenderFlow and alias.RenderFlow is rf.RenderFlow
    assert "render_flow" in sl.__all__ and "RenderFlow" in sl.__all__
    assert hasattr(sl.SceneBatch, "flow") and hasattr(sl.SceneBatch, "view_state")


def test_cpu_tensors_are_refused():
    import torch

    d, i, m = torch.ones((1, 4, 5)), torch.zeros((1, 4, 5), dtype=torch.int16), torch.zeros((1, 2, 3, 4))
    with pytest.raises(_abi.SlhipError) as e:
        rf.compute(d, i, m, (64.0, 64.0, 2.5, 2.0))
    assert "no CPU path" in str(e.value)
    with pytest.raises(_abi.SlhipError):
        rf.motion(m, m)
    with pytest.raises(ValueError):
        rf.make_params((64.0, 64.0, 2.5, 2.0), (5, 4), 2, outputs=("flow", "colour"))
    r = rf.RenderFlow(flow=np.zeros((1, 1, 1, 2), F))
    with pytest.raises(RuntimeError):
        r.valid
    with pytest.raises(RuntimeError):
        r.covisibility()
