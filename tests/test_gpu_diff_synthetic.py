"""sl.diff on the GPU against tests/diff_ref.py (NumPy) and the C oracle at synthetic G-buffers: pixel counts that are no multiple
of the 256-thread block, images without an interior, 256 objects, junctions of several objects with tied depths, one gradient
image per pose hypothesis, and the limits of the entries.  The stencils, the image gradients and the vertex backward are exact; the
atomically summed pose gradient is held to diff_ref.pose_bound."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import diff_ref as R
from stillleben_amd import _abi
from test_gpu_diff import _Obj, _ResultVB, _Scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(sl):
    from stillleben_amd._context import engine

    return engine()


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _scene(g, poses=None, obj_inst=None):
    poses, obj_inst = g.poses if poses is None else poses, g.obj_inst if obj_inst is None else obj_inst
    return _Scene(g.P, [_Obj(p, i) for p, i in zip(poses, obj_inst)])


def _result(g):
    return _ResultVB(g.rgb, g.coord, g.inst, g.bary, g.vidx)


@pytest.fixture(scope="module", params=R.SHAPES, ids=lambda s: "%dx%d_%d" % s[:3])
def case(request):
    """the G-buffer of one shape with its NumPy answers, computed once for the tests below"""
    g = R.synth_case(*request.param)
    g.valid = R.sobel_valid(g.inst, g.coord[:, :, 3])
    g.gx, g.gy = R.image_gradients(g.rgb, g.valid)
    g.pose, g.A = R.pose_backward(g.rgb, g.coord, g.inst, g.grad, g.P, g.poses, g.obj_inst)
    g.gv, g.gc = R.vertex_backward(g.rgb, g.coord, g.inst, g.bary, g.grad, g.P, g.poses, g.obj_inst)
    return g


def test_stencils_and_image_gradients_exact(sl, oracle, case):
    g = case
    depth, c3 = g.coord[:, :, 3].copy(), g.coord[:, :, :3].copy()
    valid = sl.diff.generate_sobel_valid_mask(torch.from_numpy(g.inst), torch.from_numpy(depth))
    assert valid.dtype == torch.bool and np.array_equal(valid.numpy(), g.valid)
    assert np.array_equal(g.valid, oracle.sobel_valid(g.inst, depth))
    for idx in g.obj_inst[:8]:
        m, c = sl.diff.dilate_object_mask(torch.from_numpy(g.inst == idx), valid, torch.from_numpy(c3))
        rm, rc = R.dilate(g.inst == idx, g.valid, c3)
        om, oc = oracle.dilate(g.inst == idx, g.valid, c3)
        assert np.array_equal(m.numpy(), rm) and np.array_equal(u32(c.numpy()), u32(rc))
        assert np.array_equal(m.numpy(), om) and np.array_equal(u32(c.numpy()), u32(oc))
    gx, gy, v = sl.diff.compute_image_space_gradients(_scene(g), _result(g))
    ogx, ogy = oracle.image_gradients(g.rgb, g.valid)
    assert np.array_equal(v.numpy(), g.valid)
    assert np.array_equal(u32(gx.numpy()), u32(g.gx)) and np.array_equal(u32(gy.numpy()), u32(g.gy))
    assert np.array_equal(u32(gx.numpy()), u32(ogx)) and np.array_equal(u32(gy.numpy()), u32(ogy))


def test_pose_backward_within_the_bound(sl, case):
    g = case
    got = sl.diff.backpropagate_gradient_to_poses(_scene(g), _result(g), torch.from_numpy(g.grad)).numpy().astype(np.float64)
    assert got.shape == (g.n_obj, 6)
    bound = R.pose_bound(g.pose, g.A)
    err = np.abs(got - g.pose)
    print("D4 hip vs diff_ref at %dx%d, %d objects: worst ratio to the bound %.3f"
          % (g.H, g.W, g.n_obj, float(np.max(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)))))
    assert (err <= bound).all()
    if g.n_obj == 256:
        assert np.count_nonzero(got.any(axis=1)) >= 200          # the LDS accumulators at their full extent, nearly all of them in use


def test_vertex_backward_bit_exact(sl, oracle, case):
    g = case
    vi, gv, gc = sl.diff.bp_to_vertices_and_colors(_scene(g), _result(g), torch.from_numpy(g.grad))
    ogv, ogc = oracle.vertex_backward(g.rgb, g.coord, g.inst, g.bary, g.grad, g.P, g.poses, g.obj_inst)
    seen = [o for o in g.obj_inst if (g.inst == o).any()]
    assert len(vi) == len(gv) == len(gc) == len(seen)
    for o, v, a, c in zip(seen, vi, gv, gc):
        m = g.inst == o
        assert np.array_equal(v.numpy(), g.vidx[m][:, :3].reshape(-1))
        for got, ref, orc in ((a, g.gv, ogv), (c, g.gc, ogc)):
            assert np.array_equal(u32(got.numpy()), u32(ref[m].reshape(-1, 3)))
            assert np.array_equal(u32(got.numpy()), u32(orc[m].reshape(-1, 3)))


def test_native_stencils_take_views_and_device_tensors(sl, eng):
    """coord[:, :, 3] and coord[:, :, :3] as the strided views they are, and the same on the device: the same answers, on
    the device of the first argument."""
    g = R.synth_case(17, 31, 5, 4)
    inst, coord = torch.from_numpy(g.inst), torch.from_numpy(g.coord)
    assert not coord[:, :, 3].is_contiguous() and not coord[:, :, :3].is_contiguous()
    ref_valid = R.sobel_valid(g.inst, g.coord[:, :, 3])
    idx = int(g.obj_inst[0])
    ref_m, ref_c = R.dilate(g.inst == idx, ref_valid, g.coord[:, :, :3])
    assert (ref_m & (g.inst != idx)).any()
    for dev in (torch.device("cpu"), eng.device):
        i, c = inst.to(dev), coord.to(dev)
        valid = sl.diff.generate_sobel_valid_mask(i, c[:, :, 3])
        m, c3 = sl.diff.dilate_object_mask(i == idx, valid, c[:, :, :3])
        assert valid.device == i.device and m.device == i.device and c3.device == i.device
        assert np.array_equal(valid.cpu().numpy(), ref_valid)
        assert np.array_equal(m.cpu().numpy(), ref_m) and np.array_equal(u32(c3.cpu().numpy()), u32(ref_c))


def test_batch_with_one_gradient_image_per_hypothesis(sl, eng):
    """K different G-buffers with different poses through sl.diff.pose_backward_batch_on_buffers: row k is hypothesis k under its
    own gradient image -- a gradient stride of 0 would give rows 1 and 2 the image of hypothesis 0."""
    H, W, n, K = 17, 31, 5, 3
    gs = [R.synth_case(H, W, n, 4, seed=1000 * k) for k in range(K)]
    assert len({g.seed for g in gs}) == K
    ids = gs[0].obj_inst
    scene = SimpleNamespace(objects=[_Obj(p, i) for p, i in zip(gs[0].poses, ids)], viewport=(W, H),
                            projection_matrix=lambda: torch.from_numpy(gs[0].P))
    buf = SimpleNamespace(rgb=torch.from_numpy(np.stack([g.rgb for g in gs])).to(eng.device),
                          coord=torch.from_numpy(np.stack([g.coord for g in gs])).to(eng.device),
                          instance=torch.from_numpy(np.stack([g.inst for g in gs])).to(eng.device))
    hyp = np.stack([g.poses for g in gs])
    grads = np.stack([g.grad for g in gs])
    shared = sl.diff.pose_backward_batch_on_buffers(scene, buf, hyp, torch.from_numpy(grads[0]).to(eng.device))
    own = sl.diff.pose_backward_batch_on_buffers(scene, buf, hyp, torch.from_numpy(grads).to(eng.device))
    assert tuple(shared.shape) == tuple(own.shape) == (K, n, 6) and own.device == eng.device
    shared, own = shared.cpu().numpy().astype(np.float64), own.cpu().numpy().astype(np.float64)

    def held(rows, image_of):
        for k, g in enumerate(gs):
            ref, A = R.pose_backward(g.rgb, g.coord, g.inst, grads[image_of(k)], gs[0].P, g.poses, ids)
            assert np.abs(ref).max() > 0
            assert (np.abs(rows[k] - ref) <= R.pose_bound(ref, A)).all()

    held(shared, lambda k: 0)
    held(own, lambda k: k)
    assert not np.array_equal(own[1], shared[1]) and not np.array_equal(own[2], shared[2])
    # the [K,H,W,1] form of the renderer's instance target is the same image
    buf.instance = buf.instance.unsqueeze(-1)
    held(sl.diff.pose_backward_batch_on_buffers(scene, buf, hyp, torch.from_numpy(grads).to(eng.device)).cpu().numpy().astype(np.float64),
         lambda k: k)
    with pytest.raises(ValueError, match="grad_objective_wrt_rnd_img"):
        sl.diff.pose_backward_batch_on_buffers(scene, buf, hyp, torch.from_numpy(grads[:2]).to(eng.device))
    buf.instance = buf.instance[0]
    with pytest.raises(ValueError, match="instance"):
        sl.diff.pose_backward_batch_on_buffers(scene, buf, hyp, torch.from_numpy(grads).to(eng.device))


def test_257_objects_are_refused_by_name(sl, eng):
    """kMaxDiffObjects = 256 sizes the LDS accumulators: one more is an error that names the limit, from the single and from the
    batch entry (256 objects run in the 33x40 case above)."""
    g = R.synth_case(5, 7, 3, 2)
    poses, ids = np.tile(g.poses[:1], (257, 1, 1)), np.arange(1, 258, dtype=np.int32)
    scene = _scene(g, poses, ids)
    with pytest.raises(_abi.SlhipError, match="at most 256 objects"):
        sl.diff.backpropagate_gradient_to_poses(scene, _result(g), torch.from_numpy(g.grad))
    scene.viewport = (g.W, g.H)
    buf = SimpleNamespace(rgb=torch.from_numpy(g.rgb[None]).to(eng.device), coord=torch.from_numpy(g.coord[None]).to(eng.device),
                          instance=torch.from_numpy(g.inst[None]).to(eng.device))
    with pytest.raises(_abi.SlhipError, match="at most 256 objects"):
        sl.diff.pose_backward_batch_on_buffers(scene, buf, poses[None], torch.from_numpy(g.grad).to(eng.device))


def test_entries_refuse_an_empty_image(sl, eng):
    """H = 0 (a grid of zero blocks) and a coordinate stride below 3: a status and a message from every entry, no launch."""
    L = eng.L
    d = torch.zeros(1024, dtype=torch.uint8, device=eng.device)
    p, P, st = C.c_void_p(d.data_ptr()), np.eye(4, dtype=np.float32), C.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)
    hp = C.c_void_p(P.ctypes.data)
    for H, W in ((0, 4), (4, 0), (-1, 4)):
        calls = {
            "slhip_diff_dilate": lambda: L.slhip_diff_dilate(p, p, p, 3, H, W, p, p, st),
            "slhip_diff_image_gradients": lambda: L.slhip_diff_image_gradients(p, p, H, W, p, p, st),
            "slhip_diff_pose_backward": lambda: L.slhip_diff_pose_backward(p, p, p, p, hp, p, p, 1, H, W, p, p, p, st),
            "slhip_diff_pose_backward_batch": lambda: L.slhip_diff_pose_backward_batch(p, p, p, p, 0, hp, p, p, 1, 1, H, W, p, p, p, st),
            "slhip_diff_sobel_valid": lambda: L.slhip_diff_sobel_valid(p, p, 1, H, W, p, st),
            "slhip_diff_vertex_backward": lambda: L.slhip_diff_vertex_backward(p, p, p, p, p, hp, p, p, 1, H, W, p, p, p, st),
        }
        for name, call in calls.items():
            assert call() != 0
            assert name.encode() in L.slhip_last_error()
    assert L.slhip_diff_dilate(p, p, p, 2, 2, 2, p, p, st) != 0
    assert b"coord_stride" in L.slhip_last_error()
    torch.cuda.synchronize(eng.device)
    assert int(d.sum()) == 0                                   # nothing ran on the buffer
