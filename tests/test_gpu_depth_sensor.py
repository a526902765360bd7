"""GPU tests of the depth sensor model (slhip_depth_sensor through sl.depth_sensor): flags and both outputs bit-exact against
the NumPy restatement tests/depth_sensor_ref.py wherever the arithmetic is IEEE add, mul, div, floor and compare; the stages
that go through the normal draws of the RNG (logf, cosf) by moments here, and draw by draw against the restated generator
(tests/sensor_rng_ref.py) in tests/test_gpu_sensor_rng.py."""
import numpy as np
import pytest
import torch

import depth_sensor_ref as R
from stillleben_amd import _abi
from stillleben_amd import depth_sensor as ds

pytestmark = pytest.mark.gpu

F = np.float32


def run(z, params, c=None):
    """process_batch on host arrays [n,H,W]: (depth f32, depth u16, flags u8) as numpy."""
    zt = torch.from_numpy(np.ascontiguousarray(z)).cuda()
    ct = None if c is None else torch.from_numpy(np.ascontiguousarray(c)).cuda()
    return tuple(t.cpu().numpy() for t in ds.process_batch(zt, params, ndotv=ct, out="both", flags=True))


def assert_bit_exact(got, ref, what=""):
    for name, g, r in zip(("flags", "depth f32", "depth u16"), (got[2], got[0].view(np.uint32), got[1]),
                          (ref[2], ref[0].view(np.uint32), ref[1])):
        assert g.dtype == r.dtype and g.shape == r.shape, (what, name)
        assert np.array_equal(g, r), "%s %s: %d of %d pixels differ" % (what, name, int((g != r).sum()), g.size)


def test_known_answers(sl):
    """The rectangle and the ramp of tests/test_host_depth_sensor.py in one launch of two images."""
    zr, c = R.rectangle_scene()
    z = np.stack([zr, R.ramp_scene()])
    params = [R.known_answer_params(ds.make_params)] * 2
    got = run(z, params, np.stack([c, c]))
    assert_bit_exact(got, R.reference_batch(z, params, np.stack([c, c])))
    fl = got[2]
    assert int(((fl[0] & R.SHADOW) != 0).sum()) == 192 and ((fl[0, 6:18, 24:40] & R.SHADOW) != 0).all()
    assert int(((fl[0] & R.SUPPORT) != 0).sum()) == 8 and int((fl[1] != 0).sum()) == 4
    valid = fl[0] == 0
    assert np.array_equal(got[0][0][valid].view(np.uint32), zr[valid].view(np.uint32))


def test_synthetic_batch_dense_and_strided(sl):
    z, c, params = R.synthetic_batch(ds.make_params)
    assert [z.shape[2] + R.dmax_of(p) for p in params] == [288, 285, 280]
    ref = R.reference_batch(z, params, c)
    for bit in (R.RANGE, R.GRAZING, R.SHADOW, R.SUPPORT):                  # the scene exercises every deterministic stage
        assert ((ref[2] & bit) != 0).any(), bit
    assert (ref[2] == 0).mean() > 0.3 and (ref[1] == 65535).any()
    assert_bit_exact(run(z, params, c), ref, "dense")
    # the same planes as the 4th float of [n,H,W,4] buffers, read in place
    z4 = torch.full(z.shape + (4,), float("nan"), dtype=torch.float32).cuda()
    c4 = torch.full(z.shape + (4,), 7.0, dtype=torch.float32).cuda()
    z4[..., 3], c4[..., 3] = torch.from_numpy(z).cuda(), torch.from_numpy(c).cuda()
    zv, cv = z4[..., 3], c4[..., 3]
    assert ds._pixel_stride(zv, "depth")[0].data_ptr() == zv.data_ptr() and ds._pixel_stride(zv, "depth")[1] == 4
    strided = tuple(t.cpu().numpy() for t in ds.process_batch(zv, params, ndotv=cv, out="both", flags=True))
    assert_bit_exact(strided, ref, "stride 4")
    # single outputs are the same planes; no n.v plane = no grazing stage
    assert np.array_equal(ds.process_batch(zv, params, ndotv=cv, out="uint16").cpu().numpy(), ref[1])
    f_only = ds.process_batch(zv, params, ndotv=cv)
    assert f_only.dtype == torch.float32 and np.array_equal(f_only.cpu().numpy().view(np.uint32), ref[0].view(np.uint32))
    assert_bit_exact(run(z, params), R.reference_batch(z, params), "no n.v")


def test_longest_projector_line(sl):
    """W + Dmax = 4096, the whole LDS line: fb / z_min = 3936 with W = 160, disparities up to Dmax itself."""
    rng = np.random.default_rng(7)
    z = rng.uniform(0.25, 3.0, (1, 5, 160)).astype(F)
    z[0, :, ::7] = 0.25                                                    # d = Dmax: the far end of the line
    p = ds.make_params(984.0, baseline=1.0, z_min=0.25, z_max=10.0, shadow_margin=1.0, cos_min=0.0, window_radius=1,
                       window_tol=50.0, min_support=2, sigma_lateral=0.0, sigma_disparity=0.0, subpixel=8, dropout_p=0.0, seed=0)
    assert z.shape[2] + R.dmax_of(p) == 4096
    assert_bit_exact(run(z, [p]), R.reference_batch(z, [p]))


def test_real_render(sl):
    """2 scenes of the small table at 320 x 240: process_buffers on the render's own buffers, noise off, against the
    restatement on the downloaded coord and normals; the objects throw projector shadows onto the plane."""
    from test_gpu_synth import small_table

    batch = sl.SceneBatch(small_table(sl), 2, 3, resolution=(320, 240), seed=(77 << 32) | 5, render_chunk=2, manual_exposure=1.0)
    batch.set_camera_intrinsics(533.4, 533.7, 156.5, 120.6)
    batch.stage()
    batch.settle(frames=5)
    batch.check_settled()
    batch.place()
    buf = batch.render(0)
    params = [ds.make_params(533.4, z_min=0.3, z_max=10.0, window_radius=2, min_support=12, sigma_lateral=0.0, sigma_disparity=0.0,
                             dropout_p=0.0, seed=i) for i in range(2)]
    got = tuple(t.cpu().numpy() for t in ds.process_buffers(buf, params, out="both", flags=True))
    z, c = buf.coord[..., 3].cpu().numpy(), buf.normals[..., 3].cpu().numpy()
    assert_bit_exact(got, R.reference_batch(z, params, c))
    inst = buf.instance[..., 0].cpu().numpy()
    for s in range(2):
        assert (inst[s] > 0).any()                                         # an object stands in front of the plane
        on_plane = (inst[s] == 0) & (z[s] < 100.0)
        assert on_plane.any() and (((got[2][s] & R.SHADOW) != 0) & on_plane).any()
        assert ((got[2][s] & R.RANGE) != 0)[z[s] > 10.0].all()             # the background at 3000
    valid = got[2] == 0
    # a valid depth is the input's disparity rounded to 1/8 px: half a step off at the most (+ f32 rounding)
    fb = float(params[0]["fb"])
    assert valid.mean() > 0.2 and np.abs(fb / got[0][valid].astype(np.float64) - fb / z[valid]).max() <= 1.0 / 16 + 1e-4


def _flat(sigma_disparity=0.25, subpixel=0, dropout_p=0.0, seed=1234, n=1, **kw):
    z = np.full((n, 256, 256), 1.5, F)
    ps = [ds.make_params(800.0, baseline=0.075, z_min=0.3, z_max=10.0, window_radius=0, min_support=1, sigma_lateral=0.0,
                         sigma_disparity=sigma_disparity, subpixel=subpixel, dropout_p=dropout_p,
                         seed=seed if np.isscalar(seed) else seed[i], **kw) for i in range(n)]
    return run(z, ps), F(60.0) / F(1.5)


def test_noise_moments(sl):
    sigma, N = 0.25, 256 * 256
    (zf, _, fl), d0 = _flat(sigma)
    assert not fl.any()
    err = 60.0 / zf.astype(np.float64) - float(d0)
    print("disparity error: mean %.5f, std %.5f (sigma %.3f)" % (err.mean(), err.std(), sigma))
    assert abs(err.mean()) < 5 * sigma / np.sqrt(N)                        # 5 standard errors of the mean
    assert abs(err.std() / sigma - 1.0) < 0.05
    # dropout: a binomial share
    p_drop = 0.1
    (zd, _, fd), _ = _flat(sigma, dropout_p=p_drop)
    share = ((fd & R.DROPOUT) != 0).mean()
    print("dropout share %.5f of %.2f" % (share, p_drop))
    assert set(np.unique(fd)) <= {0, R.DROPOUT}
    assert abs(share - p_drop) < 3 * np.sqrt(p_drop * (1 - p_drop) / N)
    # the fixed draw order: switching the dropout off leaves the noise of the surviving pixels as it was
    keep = fd == 0
    assert np.array_equal(zd[keep].view(np.uint32), zf[keep].view(np.uint32)) and (zd[~keep] == 0).all()
    # quantised output lies on the 1/8 px lattice (two f32 roundings of ~2^-24 on 8 d = 320: far below 1e-3)
    (zq, _, fq), _ = _flat(0.5, subpixel=8)
    steps = 60.0 / zq.astype(np.float64) * 8
    assert not fq.any() and np.abs(steps - np.round(steps)).max() < 1e-3 and len(np.unique(np.round(steps))) > 8


def test_seeds(sl):
    (a, _, _), _ = _flat(seed=1234)
    (b, _, _), _ = _flat(seed=1234)
    (c, _, _), _ = _flat(seed=1235)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and not np.array_equal(a, c)
    (m, _, _), _ = _flat(seed=(1234, 99, 1235), n=3)
    assert np.array_equal(m[0].view(np.uint32), a[0].view(np.uint32))       # image 0 of a batch = the image alone
    assert not np.array_equal(m[0], m[1]) and not np.array_equal(m[1], m[2]) and not np.array_equal(m[0], m[2])


def test_lateral_jitter(sl):
    """sigma_lateral = 0.5 on the rectangle scene: every output pixel is the deterministic outcome (value and flags) of
    some pixel within +-2 of it, clamped to the image -- and not always of itself."""
    z, c = R.rectangle_scene()
    det_f, _, det_flags = R.reference(z, R.known_answer_params(ds.make_params), c)
    zf, _, fl = (a[0] for a in run(z[None], [R.known_answer_params(ds.make_params, sigma_lateral=0.5, seed=42)], c[None]))
    H, W = z.shape
    ys, xs = np.mgrid[0:H, 0:W]
    found = np.zeros((H, W), bool)
    for jy in range(-2, 3):
        for jx in range(-2, 3):
            sy, sx = np.clip(ys + jy, 0, H - 1), np.clip(xs + jx, 0, W - 1)
            found |= (det_flags[sy, sx] == fl) & (det_f[sy, sx].view(np.uint32) == zf.view(np.uint32))
    assert found.all()
    assert (zf[fl == 0] > 0).all() and (zf[fl != 0] == 0).all()
    moved = (fl != det_flags) | (zf != det_f)
    assert moved.any()                                                     # (only pixels next to an edge can tell)


def test_public_interface(sl):
    from test_gpu_synth import small_table

    with pytest.raises(_abi.SlhipError):
        ds.process_batch(torch.ones(1, 8, 8), [ds.make_params(500.0)])
    with pytest.raises(ValueError):
        ds.process_batch(torch.ones(2, 8, 8).cuda(), [ds.make_params(500.0)])          # one record per image
    with pytest.raises(_abi.SlhipError, match="exceeds 4096"):
        ds.process_batch(torch.ones(1, 8, 8).cuda(), [ds.make_params(500.0, z_min=0.005)])
    batch = sl.SceneBatch(small_table(sl), 2, 3, resolution=(320, 240), seed=3, render_chunk=2)
    batch.set_camera_intrinsics(533.4, 533.7, 156.5, 120.6)
    batch.stage()
    batch.settle(frames=5)
    batch.place()
    params = [ds.make_params(533.4, seed=i) for i in range(2)]
    buf = batch.render(0, _abi.OUT_COORD)                                    # no normals: the grazing stage is off
    zu, fl = sl.depth_sensor.process_buffers(buf, params, out="uint16", flags=True)
    assert zu.dtype == torch.uint16 and fl.dtype == torch.uint8 and tuple(zu.shape) == (2, 240, 320) and zu.is_cuda
    fl = fl.cpu().numpy()
    assert not (fl & R.GRAZING).any() and (fl == 0).any()
    assert ((zu.cpu().numpy() > 0) == (fl == 0)).all()
    with pytest.raises(RuntimeError, match="coord"):
        sl.depth_sensor.process_buffers(batch.render(0, _abi.OUT_RGB | _abi.OUT_NORMALS), params)
