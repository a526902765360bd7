"""What the host and the GPU tests of the sensor models' noise share, on top of the restated generator
(tests/sensor_rng_ref.py): the noise stage of k_camera_stage1 and the four draws of k_depth_measure restated with its streams, the
inputs of the per-pixel comparisons, and the check that reads the draws back out of a camera image."""
import numpy as np

import sensor_rng_ref as S

F = np.float32

# ---- the noise stage of k_camera_stage1 and how a test reads its draws back out of an image ------------------------------------
HUE_ROUND_TRIP = 6.6e-7             # the most the hue round trip at hue_shift = 0 moves a value in [0, 1]


# (noise_a, noise_b, lowest input, highest input) of the per-pixel comparisons; the rate of a draw is input / noise_a.
POISSON_SETS = [(2.0 ** -6, 0.0, 0.0, 0.125),        # rates 0 .. 8: the multiplication method
                (2.0 ** -6, 0.0, 0.078, 0.235),      # 5 .. 15: both methods, either side of 10
                (2.0 ** -9, 0.0, 0.039, 0.39),       # 20 .. 200
                (2.0 ** -14, 0.0, 0.061, 0.488)]     # 1000 .. 8000
NORMAL_SET = (0.0, 2.0 ** -6, 0.12, 0.24)
ORDER_SETS = [(2.0 ** -6, 2.0 ** -6, 0.0, 0.235), (2.0 ** -9, 2.0 ** -6, 0.039, 0.39)]
CAMERA_SHAPE = (2, 3, 20, 72)       # partial 32 x 8 tiles in both directions, two values of ctr1
CAMERA_SEED = (0x5EED0BAD << 32) | 0x00C0FFEE


def ramp(lo, hi, shape=CAMERA_SHAPE):
    """A smooth ramp over every pixel, channel and image: each draw has a rate of its own."""
    n = int(np.prod(shape))
    return (lo + (hi - lo) * np.arange(n, dtype=np.float64) / n).reshape(shape).astype(F)


def neutral_camera_params(noise_a, noise_b, seed, noise=True):
    """A camera record whose every stage but the noise is neutral: no blur, scaling 1, translation 0, exposure_deltaS 0,
    hue_shift 0, a delta as the post kernel."""
    from stillleben_amd import camera_model as cm

    p = cm.make_params(np.zeros((3, 2)), np.ones(3), 0.0, 0.0, noise, noise_a, noise_b, 0.0, seed=seed)
    delta = np.zeros(25, F)
    delta[12] = 1
    p["post_kernel"] = delta
    return p


def camera_noise_input(oracle, img):
    """v, the values that enter the noise stage: the oracle's stage 2 (the HIP path is held bit-equal to it elsewhere)."""
    return oracle.camera_model(img, [neutral_camera_params(0.0, 0.0, 0, noise=False)] * len(img), stage=2)


def camera_noise(v, noise_a, noise_b, seed, stream_cls=S.Stream):
    """The noise stage on v f32 [B,3,H,W], the values that enter it: per channel, R then G then B, the Poisson draw
    (noise_a > 0) and then the normal (noise_b > 0) of the pixel's stream.  Returns [B,3,H,W] arrays: k (counts), n (normals),
    tol (bound of |device n - n|), fragile, and out = clamp(k / chi + n * b, 0, 1), what goes into the hue round trip."""
    v = np.asarray(v, F)
    B, _, H, W = v.shape
    a, b = F(noise_a), F(noise_b)
    res = {"k": np.zeros(v.shape, F), "n": np.zeros(v.shape, F), "tol": np.zeros(v.shape), "fragile": np.zeros(v.shape, bool),
           "out": np.zeros(v.shape, F)}
    for i in range(B):
        s = stream_cls(seed, H, W, i)
        for c in range(3):
            pois, g = v[i, c], F(0)
            if a > 0:
                chi = F(1.0) / a
                res["k"][i, c], res["fragile"][i, c] = s.poisson(chi * v[i, c])
                pois = res["k"][i, c] / chi
            if b > 0:
                res["n"][i, c], res["fragile"][i, c], res["tol"][i, c] = s.normal()
                g = res["n"][i, c] * b
            res["out"][i, c] = np.minimum(np.maximum(pois + g, F(0)), F(1))
    return res


def check_camera_noise(out, v, noise_a, noise_b, seed, max_fragile=0.01, stream_cls=S.Stream):
    """Holds `out` f32 [B,3,H,W], the camera model's output with every other stage neutral (hue_shift 0, delta post kernel),
    to the restatement draw by draw; v as in camera_noise, noise_a a power of two or 0.  Raises AssertionError; returns the
    figures it checked.  Without the normal: out / noise_a lies within 0.05 of an integer, the count, which equals the
    restatement's on every draw that is not fragile; no value is clamped at 1.  With it: out is within
    noise_b * tol + HUE_ROUND_TRIP of clamp(k / chi + n * noise_b) on every draw that is not fragile.  With both, only that
    clamped sum is compared: where it clamps to 0 or 1 (small counts under a negative normal), a wrong count goes unseen; the
    counts themselves are held by the sets without the normal."""
    ref = camera_noise(v, noise_a, noise_b, seed, stream_cls=stream_cls)
    out64, ok = np.asarray(out, np.float64), ~ref["fragile"]
    res = {"fragile_share": float(ref["fragile"].mean())}
    assert res["fragile_share"] <= max_fragile, res
    if noise_b > 0:
        bound = float(noise_b) * ref["tol"] + HUE_ROUND_TRIP
        err = np.abs(out64 - ref["out"].astype(np.float64))
        res["max_normal_error"] = float((err[ok] / float(noise_b)).max())
        res["max_error_over_bound"] = float((err[ok] / bound[ok]).max())
        res["over_bound"] = int((err[ok] > bound[ok]).sum())
        assert res["over_bound"] == 0, res
        assert float(np.abs(ref["n"]).max()) > 3.0                  # (the comparison has a tail to look at)
        return res
    r = out64 / float(noise_a)
    k = np.rint(r)
    res["max_off_lattice"] = float(np.abs(r - k).max())
    res["clamped_share"] = float((np.asarray(out) >= 1.0).mean())
    res["mismatches"] = int((k != ref["k"])[ok].sum())
    res["mismatches_among_fragile"] = int((k != ref["k"])[~ok].sum())
    assert res["max_off_lattice"] <= 0.05, res
    assert res["clamped_share"] == 0.0, res
    assert res["mismatches"] == 0, res
    return res


def depth_sensor_draws(seed, H, W, image, stream_cls=S.Stream):
    """The four draws of k_depth_measure in their order: dict of ex, ey, u, en (f32 [H,W]) and tol_ex, tol_ey, tol_en."""
    s = stream_cls(seed, H, W, image)
    ex, _, tex = s.normal()
    ey, _, tey = s.normal()
    u = s.uniform()
    en, _, ten = s.normal()
    return {"ex": ex, "ey": ey, "u": u, "en": en, "tol_ex": tex, "tol_ey": tey, "tol_en": ten}


def near_integer(x, tol):
    """True where x lies within tol of an integer + rounding: a floorf(x) that an error of tol in x can move."""
    x = np.asarray(x, np.float64)
    return np.abs(x - np.rint(x)) <= tol
