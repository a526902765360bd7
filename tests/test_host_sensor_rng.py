"""Host tests of tests/sensor_rng_ref.py, the NumPy restatement of stillleben_amd/csrc/slhip_rng.h that
tests/test_gpu_sensor_rng.py holds the kernels to draw by draw: Random123's known answers for philox4x32-10, the restated
Poisson and normal samplers against their exact distributions (chi-square, fixed seeds: a pass is a pass forever),
independence across pixels, images and the halves of a block, and two deliberately wrong samplers that must fail."""
import math
from statistics import NormalDist

import numpy as np
import pytest

import sensor_noise_harness as Hn
import sensor_rng_ref as S

F = np.float32
H, W = 400, 512                     # N = 204 800 draws per field
N = H * W
SEED = (0x1234ABCD << 32) | 0x9E3779B1


def chi2_limit(bins, tail=1e-6):
    """Wilson-Hilferty upper quantile of chi-square with bins - 1 degrees of freedom."""
    df = bins - 1
    z = NormalDist().inv_cdf(1.0 - tail)
    return df * (1.0 - 2.0 / (9.0 * df) + z * math.sqrt(2.0 / (9.0 * df))) ** 3


def merged_chi2(counts, expect, least=10.0):
    """Chi-square of observed `counts` against `expect`, neighbouring bins merged until each expects at least `least`."""
    obs, exp, o, e = [], [], 0.0, 0.0
    for c, x in zip(counts, expect):
        o, e = o + c, e + x
        if e >= least:
            obs.append(o), exp.append(e)
            o, e = 0.0, 0.0
    obs[-1] += o                                                    # the remainder joins the last bin
    exp[-1] += e
    obs, exp = np.array(obs), np.array(exp)
    return float(((obs - exp) ** 2 / exp).sum()), len(obs)


def poisson_chi2(k, lam):
    """(statistic, bins) of the draws k against the exact probability mass function of Poisson(lam)."""
    k = np.asarray(k, np.int64).reshape(-1)
    assert k.min() >= 0
    top = int(max(k.max(), lam + 12.0 * math.sqrt(lam) + 20.0))
    ks = np.arange(top + 1, dtype=np.float64)
    pmf = np.exp(-lam + ks * math.log(lam) - S.lgamma64(ks + 1.0))
    expect = pmf * k.size
    expect[-1] += (1.0 - pmf.sum()) * k.size                        # (the mass beyond `top`: below 1e-30)
    return merged_chi2(np.bincount(k, minlength=top + 1), expect)


class RejectSlowPath(S.Stream):
    """Deliberately wrong: PTRS whose slow path always rejects -- only the squeeze's region is ever returned."""

    def _slow_accept(self, lhs, k, lam, mags):
        no = np.zeros(k.shape, bool)
        return no, no


class ForwardWords(S.Stream):
    """Deliberately wrong: the words of a block handed out front to back."""

    WORDS = (0, 1, 2, 3)


KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_known_answers():
    for ctr, key, out in KAT:
        assert tuple(int(w) for w in S.philox4x32_10(np.array(ctr, np.uint32), np.array(key, np.uint32))) == out
    # vectorised: the three at once, each with its own key
    got = S.philox4x32_10(np.array([c for c, _, _ in KAT], np.uint32), np.array([k for _, k, _ in KAT], np.uint32))
    assert np.array_equal(got, np.array([o for _, _, o in KAT], np.uint32))


def test_stream_layout_and_word_order():
    """ctr0 = y * W + x, ctr1 = image, c[2] = sub-block, c[3] = 0x5114EBE2, key = (seed_lo, seed_hi); words 3, 2, 1, 0."""
    h, w, image = 3, 5, 7
    s = S.Stream(SEED, h, w, image)
    words = np.stack([s.next_u32() for _ in range(9)])               # two blocks and the first word of a third
    key = np.array([SEED & 0xFFFFFFFF, SEED >> 32], np.uint32)
    assert key[1] != 0
    for y in range(h):
        for x in range(w):
            blocks = [S.philox4x32_10(np.array([y * w + x, image, sub, 0x5114EBE2], np.uint32), key) for sub in range(3)]
            expect = [blocks[0][3], blocks[0][2], blocks[0][1], blocks[0][0], blocks[1][3], blocks[1][2], blocks[1][1],
                      blocks[1][0], blocks[2][3]]
            assert [int(v) for v in words[:, y, x]] == [int(v) for v in expect]
    # a pixel that sits a draw out keeps its words
    s1, s2 = S.Stream(SEED, h, w, image), S.Stream(SEED, h, w, image)
    act = np.zeros((h, w), bool)
    act[1, 2] = True
    first = s1.next_u32(act)
    assert first[1, 2] == words[0, 1, 2] and not first[~act].any()
    assert np.array_equal(s1.next_u32()[~act], words[0][~act]) and s1.next_u32(act)[1, 2] == words[2, 1, 2]
    assert np.array_equal(s2.uniform(), S.uniform_of(words[0]))


def test_uniform_is_half_open_at_zero():
    """(0, 1]: exactly 1.0 for the word 0xffffffff (the + 0.5f rounds 2^24 - 0.5 up), never 0."""
    edge = S.uniform_of(np.array([0xFFFFFFFF, 0xFFFFFF00, 0xFFFFFEFF, 0, 0xFF, 0x100], np.uint32))
    assert edge.dtype == F
    assert edge[0] == F(1.0) and edge[1] == F(1.0) and edge[2] < F(1.0)
    assert edge[3] == F(2.0 ** -25) and edge[4] == edge[3] and edge[5] == F(1.5 * 2.0 ** -24)
    u = S.Stream(SEED, H, W, 0).uniform()
    assert u.min() > 0 and u.max() <= 1 and abs(float(u.mean()) - 0.5) < 5 * math.sqrt(1 / 12 / N)
    # a uniform of exactly 1.0 goes through all three samplers: log 0 = 0 draws a normal of 0, the multiplication method
    # keeps its product, PTRS's proposal has us = 0 and is rejected by the (us < 0.013 && V > us) test

    class Ones(S.Stream):
        def _next(self, act):
            return np.where(act, np.uint32(0xFFFFFFFF), np.uint32(0)).astype(np.uint32)

    ones = Ones(0, 1, 4, 0)
    n, _, _ = ones.normal()
    assert np.all(n == 0)
    k, _ = ones.poisson(np.array([[0.5, 5.0, 30.0, 900.0]], F))
    assert [float(v) for v in k[0]] == [200.0, 200.0, 30.0, 900.0]  # (the caps: 200 products, 64 proposals)


@pytest.mark.parametrize("lam", [0.05, 1.0, 9.99, 10.0, 10.5, 30.0, 900.0, 8192.0])
def test_poisson_against_exact_pmf(lam):
    k, _ = S.Stream(SEED + int(lam * 100), H, W, 0).poisson(F(lam))
    stat, bins = poisson_chi2(k, float(F(lam)))
    print("rate %g: chi-square %.1f over %d bins, limit %.1f; mean %.4f, var/lambda %.4f"
          % (lam, stat, bins, chi2_limit(bins), k.mean(), k.var() / lam))
    assert bins >= 2 and stat <= chi2_limit(bins)


def test_poisson_edges():
    s = S.Stream(SEED, 1, 6, 0)
    k, fr = s.poisson(np.array([[0.0, -1.0, np.nan, 1.0, 1.0, 1.0]], F))
    assert not k[0, :3].any() and not fr.any()
    assert (s.sub[:3] == 0).all() and (s.sub[3:] >= 1).all()         # a rate that is not positive consumes nothing


@pytest.mark.parametrize("lam", [30.0, 900.0])
def test_wrong_sampler_fails_chi2(lam):
    """The check can fail: PTRS with its slow path replaced by `reject`."""
    k, _ = RejectSlowPath(SEED + int(lam * 100), H, W, 0).poisson(F(lam))
    stat, bins = poisson_chi2(k, lam)
    print("rate %g, slow path rejects: chi-square %.1f over %d bins, limit %.1f" % (lam, stat, bins, chi2_limit(bins)))
    assert stat > chi2_limit(bins)


def test_normal_distribution():
    s = S.Stream(SEED + 1, H, W, 0)
    n = np.concatenate([s.normal()[0].reshape(-1), s.normal()[0].reshape(-1)]).astype(np.float64)
    edges = np.array([NormalDist().inv_cdf(i / 64.0) for i in range(1, 64)])
    counts = np.bincount(np.searchsorted(edges, n), minlength=64)
    stat, bins = merged_chi2(counts, np.full(64, n.size / 64.0))
    p4 = 2.0 * (1.0 - NormalDist().cdf(4.0))
    tail = int((np.abs(n) > 4.0).sum())
    print("normal: chi-square %.1f over %d bins, limit %.1f; |n| > 4: %d of %.1f expected; mean %.5f, var %.5f"
          % (stat, bins, chi2_limit(bins), tail, p4 * n.size, n.mean(), n.var()))
    assert bins == 64 and stat <= chi2_limit(64)
    assert abs(tail - p4 * n.size) <= 5.0 * math.sqrt(n.size * p4 * (1.0 - p4))


def corr(a, b):
    return float(np.corrcoef(np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1))[0, 1])


def test_independence():
    fields = {}
    for image in (0, 1):
        s = S.Stream(SEED + 2, H, W, image)
        n1, n2 = s.normal()[0], s.normal()[0]                        # the two halves of block 0
        fields[image] = (n1, n2, s.poisson(F(30.0))[0], s.uniform())
    pairs = {}
    for name, i in (("first normal", 0), ("second normal", 1), ("poisson(30)", 2), ("uniform", 3)):
        a, b = fields[0][i], fields[1][i]
        pairs[name + ", x and x+1"] = (a[:, :-1], a[:, 1:])
        pairs[name + ", y and y+1"] = (a[:-1], a[1:])
        pairs[name + ", images 0 and 1"] = (a, b)
    pairs["first and second normal of a pixel"] = (fields[0][0], fields[0][1])
    pairs["first normal and poisson of a pixel"] = (fields[0][0], fields[0][2])
    for name, (a, b) in pairs.items():
        r, limit = corr(a, b), 5.0 / math.sqrt(a.size)               # the pair's own N
        print("%-40s %+.5f (limit %.5f, N %d)" % (name, r, limit, a.size))
        assert abs(r) < limit, name
    assert corr(fields[0][0], fields[0][0]) > 0.999                   # (the statistic sees a dependence)


# ---- the per-pixel comparison of tests/test_gpu_sensor_rng.py, run on the CPU against the restatement itself ----------------
@pytest.mark.parametrize("noise_a,noise_b,lo,hi", Hn.POISSON_SETS + [Hn.NORMAL_SET] + Hn.ORDER_SETS)
def test_per_pixel_check_passes_on_itself_and_fails_on_forward_words(oracle, noise_a, noise_b, lo, hi):
    """The inputs of the GPU comparisons, with the restatement + the hue round trip of camera_model.color_jitter standing in
    for the kernel: the fragile share stays below 1 %, the check passes, and fails for words in forward order."""
    import torch
    from stillleben_amd import camera_model as cm

    v = Hn.camera_noise_input(oracle, Hn.ramp(lo, hi))
    assert abs(float(v.min()) - lo) < 2e-4 and abs(float(v.max()) - hi) < 2e-4

    def device(stream_cls):
        noisy = Hn.camera_noise(v, noise_a, noise_b, Hn.CAMERA_SEED, stream_cls=stream_cls)["out"]
        return np.stack([cm.color_jitter(torch.from_numpy(im), 0.0).numpy() for im in noisy])

    res = Hn.check_camera_noise(device(S.Stream), v, noise_a, noise_b, Hn.CAMERA_SEED)
    print(res)
    with pytest.raises(AssertionError):
        Hn.check_camera_noise(device(ForwardWords), v, noise_a, noise_b, Hn.CAMERA_SEED)


def test_fragile_marks_near_thresholds(monkeypatch):
    """With an absurd device error every decision is near its threshold; with the real one next to none is; a pixel that
    was fragile once stays so, because what it consumes next hangs on that decision."""
    lam = np.concatenate([np.full((8, 64), 3.0, F), np.full((8, 64), 300.0, F)])
    s = S.Stream(SEED, 16, 64, 0)
    assert s.poisson(lam)[1].mean() < 0.01
    monkeypatch.setattr(S, "ULP_BOUND", 2.0 ** 22)
    s = S.Stream(SEED, 16, 64, 0)
    k, fr = s.poisson(lam)
    assert fr[:8].mean() > 0.2 and 0.05 < fr[8:].mean() < 0.5        # PTRS: only the slow path decides by a logarithm
    assert np.array_equal(s.normal()[1], fr) and np.array_equal(s.poisson(F(0.0))[1], fr)


def test_make_params_refuses_unrepresentable_counts():
    from stillleben_amd import camera_model as cm

    args = (np.zeros((3, 2)), np.ones(3), 0.0, 0.0)
    for a in (2.0 ** -25, 1e-9):
        with pytest.raises(ValueError, match="noise_a"):
            cm.make_params(*args, True, a, 0.0, 0.0, seed=1)
        assert cm.make_params(*args, False, a, 0.0, 0.0, seed=1)["noise_enabled"] == 0     # noise off: nothing to refuse
    for a in (0.0, 2.0 ** -24, 2.0 ** -20, 0.04):
        assert cm.make_params(*args, True, a, 0.0, 0.0, seed=1)["noise_a"] == F(a)


@pytest.mark.parametrize("draws", [[1e-7], [0.9, 0.9, 1e-7, 0.5], [0.9, 0.9, 0.0, 0.5], [0.9, 0.9, 0.5, 0.5]])
def test_process_image_never_draws_a_refused_record(monkeypatch, draws):
    """process_image draws noise_a = random() * 0.04, which is above 0 and below 2^-24 about once in 670 000 images: such a
    draw counts as 0 and the record is made, noise on or off.  `draws`: what random.random returns, in turn, then its last."""
    from stillleben_amd import camera_model as cm

    seq = list(draws)
    monkeypatch.setattr(cm.random, "random", lambda: seq.pop(0) if len(seq) > 1 else seq[0])
    args = cm._random_parameters()
    assert args["do_noise"] == (draws[min(1, len(draws) - 1)] > 0.3)
    small = draws[min(2, len(draws) - 1)] * 0.04 < 2.0 ** -24
    assert args["noise_a"] == (0.0 if small else draws[2] * 0.04)
    p = cm.make_params(*(args[k] for k in ("chromatic_translation", "chromatic_scaling", "blur_sigma", "exposure_deltaS", "do_noise",
                                           "noise_a", "noise_b", "hue_shift")), seed=1)
    assert p["noise_a"] == F(args["noise_a"]) and (p["noise_a"] == 0 or p["noise_a"] >= F(2.0 ** -24))
