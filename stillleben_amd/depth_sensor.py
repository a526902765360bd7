"""Depth sensor model -- this project's addition, the depth sibling of ``camera_model`` (the reference has no counterpart).

The renderer's depth (``RenderPassResult.depth()``, ``buffers.coord[..., 3]``) is the exact camera z: dense, noise-free, valid
up to every silhouette, 3000 on the background.  ``process_batch`` / ``process_buffers`` turn it into what a rectified
structured-light or active-stereo sensor with its projector at +baseline along camera x delivers (``slhip_depth_sensor`` of
include/slhip.h, two HIP kernels; there is no CPU path): range limits, holes at grazing angles, the projector's shadow band
beside every object, holes where the matching window straddles a discontinuity, lateral jitter, disparity noise, disparity
quantised to 1/subpixel px (so the depth step grows with z squared), random dropout.  DESIGN.md "Depth sensor model" states
the model step by step.

    params = [sl.depth_sensor.make_params(fx, seed=s) for s in range(buffers.B)]
    depth_mm, flags = sl.depth_sensor.process_buffers(buffers, params, out="uint16", flags=True)      # BOP's depth/

Flags (uint8 per pixel, 0 = valid): RANGE 1, GRAZING 2, SHADOW 4, SUPPORT 8, DROPOUT 16."""
import ctypes as C

import numpy as np
import torch

from . import _abi, _device

__all__ = ["RANGE", "GRAZING", "SHADOW", "SUPPORT", "DROPOUT", "make_params", "check_params", "scratch_bytes", "process_batch",
           "process_buffers"]

RANGE, GRAZING, SHADOW, SUPPORT, DROPOUT = 1, 2, 4, 8, 16
MAX_LINE, MAX_RADIUS = 4096, 4      # SLHIP_DEPTH_SENSOR_MAX_LINE / _MAX_RADIUS


def make_params(fx, baseline=0.075, z_min=0.4, z_max=4.0, shadow_margin=0.5, cos_min=0.15, window_radius=4, window_tol=1.0,
                min_support=40, sigma_lateral=0.4, sigma_disparity=1.0 / 6.0, subpixel=8, dropout_p=0.002, depth_scale=1.0,
                seed=None):
    """One slhip_depth_sensor_params record (numpy).  `fx`: focal length in px of the rendered image (no default).  The other
    defaults describe a PrimeSense-class device (Kinect v1, Xtion): 75 mm between projector and camera, a working range of
    0.4 .. 4 m, a 9 x 9 matching window (`window_radius` 4) of which about half (`min_support` 40 of 81) must lie within
    `window_tol` 1 px of disparity of the centre, disparity in 1/8 px steps (`subpixel` 8) with a noise of 1/6 px, returns lost
    below |n.v| = `cos_min` 0.15 (about 81 degrees off the normal), a shadow wherever an occluder is more than
    `shadow_margin` 0.5 px of disparity in front, edges that wander by `sigma_lateral` 0.4 px, 0.2 % random holes.
    `depth_scale`: millimetres per unit of the uint16 output (sl.bop.depth_image_scale).  `seed`: the image's noise key;
    None draws one from torch's generator."""
    p = np.zeros((), _abi.DEPTH_SENSOR_DTYPE)
    p["fb"] = np.float32(float(fx) * float(baseline))        # rounded once
    p["z_min"], p["z_max"] = np.float32(z_min), np.float32(z_max)
    p["shadow_margin"], p["cos_min"] = np.float32(shadow_margin), np.float32(cos_min)
    if not 0 <= int(window_radius) <= MAX_RADIUS:
        raise ValueError("window_radius must be in [0, %d]" % MAX_RADIUS)
    p["window_radius"], p["window_tol"], p["min_support"] = int(window_radius), np.float32(window_tol), int(min_support)
    p["sigma_lateral"], p["sigma_disparity"] = np.float32(sigma_lateral), np.float32(sigma_disparity)
    p["subpixel"], p["dropout_p"], p["depth_scale"] = int(subpixel), np.float32(dropout_p), np.float32(depth_scale)
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())   # follows torch.manual_seed
    p["seed_lo"], p["seed_hi"] = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    return p


def _records(params):
    return np.ascontiguousarray(np.stack([np.asarray(p, dtype=_abi.DEPTH_SENSOR_DTYPE) for p in params]).reshape(-1))


def check_params(params, width):
    """Raises SlhipError when a record cannot run on images `width` px wide (slhip_depth_sensor_check_params: positive fb,
    z_min and depth_scale, z_max >= z_min, window_radius <= 4, width + ceil(fb / z_min) <= 4096).  Needs no device."""
    rec = _records(params)
    _abi.check(_abi.lib().slhip_depth_sensor_check_params(rec.ctypes.data, len(rec), int(width)), "slhip_depth_sensor")
    return rec


def scratch_bytes(n_images, width, height):
    n = C.c_uint64(0)
    _abi.check(_abi.lib().slhip_depth_sensor_scratch_bytes(int(n_images), int(width), int(height), C.byref(n)),
               "slhip_depth_sensor_scratch_bytes")
    return n.value


def _pixel_stride(t, what):
    """The stride in floats of a [n,H,W] float32 tensor laid out as pixel (i, y, x) at ((i * H + y) * W + x) * stride; a
    tensor of any other layout is copied to a dense one.  Returns (tensor, stride)."""
    if t.dim() != 3:
        raise ValueError("%s: a [n,H,W] tensor expected, got %s" % (what, tuple(t.shape)))
    if not t.is_cuda:
        raise _abi.SlhipError("depth_sensor runs on the HIP device: pass a cuda tensor (there is no CPU path)")
    if t.dtype != torch.float32:
        t = t.float()
    n, H, W = t.shape
    s = t.stride(2)
    if not (s >= 1 and t.stride(1) == W * s and t.stride(0) == H * W * s):
        t, s = t.contiguous(), 1
    return t, s


def process_batch(depth, params, ndotv=None, out="float", flags=False):
    """depth: f32 [n,H,W] on a HIP device, camera z in metres -- dense, or a strided view such as ``buffers.coord[..., 3]``,
    which is read in place.  params: one make_params record per image.  ndotv: the same for n.v (``buffers.normals[..., 3]``);
    None runs without the grazing stage.  Returns, in this order, what was asked for (a single tensor when it is one thing):
    out="float": f32 [n,H,W] metres, 0 where invalid; out="uint16": uint16 [n,H,W] in units of depth_scale mm, 0 where
    invalid; out="both": the two; flags=True: uint8 [n,H,W] of RANGE | GRAZING | SHADOW | SUPPORT | DROPOUT."""
    if out not in ("float", "uint16", "both"):
        raise ValueError('out: "float", "uint16" or "both"')
    z, zs = _pixel_stride(depth, "depth")
    n, H, W = z.shape
    c, cs = None, 0
    if ndotv is not None:
        if tuple(ndotv.shape) != (n, H, W):
            raise ValueError("ndotv: shape %s expected" % ((n, H, W),))
        c, cs = _pixel_stride(ndotv, "ndotv")
        if c.device != z.device:
            raise ValueError("depth and ndotv are on different devices")
    if len(params) != n:
        raise ValueError("one parameter record per image")
    rec = check_params(params, W)
    L = _abi.lib()
    dev = z.device
    d_params = torch.from_numpy(np.frombuffer(rec.tobytes(), dtype=np.uint8).copy()).to(dev)
    o_f = torch.empty((n, H, W), dtype=torch.float32, device=dev) if out in ("float", "both") else None
    o_u = torch.empty((n, H, W), dtype=torch.uint16, device=dev) if out in ("uint16", "both") else None
    o_g = torch.empty((n, H, W), dtype=torch.uint8, device=dev) if flags else None
    scratch = _device.scratch(scratch_bytes(n, W, H), dev)

    def ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)

    with torch.cuda.device(dev):
        st = L.slhip_depth_sensor(ptr(z), zs, ptr(c), cs, n, H, W, ptr(d_params), ptr(o_f), ptr(o_u), ptr(o_g), ptr(scratch),
                                  _device.stream_ptr(dev))
    _abi.check(st, "slhip_depth_sensor")
    res = [t for t in (o_f, o_u, o_g) if t is not None]
    for t in res:                                   # the launch is asynchronous: its inputs live as long as its outputs
        t._keepalive = (d_params, scratch, z, c)
    return res[0] if len(res) == 1 else tuple(res)


def process_buffers(buffers, params, out="float", flags=False):
    """The model on the result of a render: `buffers` is what SceneBatch.render / RenderPass.render_batch return (every image of
    it) or a RenderPassResult (its one image).  z is the w of `coord`, read in place; n.v the w of `normals`.  Raises when
    `coord` was not rendered; runs without the grazing stage when `normals` was not."""
    sel = slice(None)
    if hasattr(buffers, "_buffers"):                # RenderPassResult
        if buffers._buffers is None:
            raise RuntimeError("RenderPassResult is empty: render something first")
        sel, buffers = slice(buffers._index, buffers._index + 1), buffers._buffers
    if getattr(buffers, "coord", None) is None:
        raise RuntimeError("depth_sensor needs the `coord` output of the render (OUT_COORD): its w is the camera z")
    normals = getattr(buffers, "normals", None)
    return process_batch(buffers.coord[sel][..., 3], params, ndotv=None if normals is None else normals[sel][..., 3], out=out,
                         flags=flags)
