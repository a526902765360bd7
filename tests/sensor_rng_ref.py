"""CPU restatement of the sensor models' random number generator (stillleben_amd/csrc/slhip_rng.h): Philox4x32-10 keyed by the
image's seed, counted by (pixel, image, sub-block), with the uniform / normal / Poisson draws on top.  NumPy, vectorised over
the pixels of one image, float32 throughout, in the header's operation order.

What is exact and what is not.  The library is built with -ffp-contract=off and HIP's float32 divide and square root are
correctly rounded, so every + - * / sqrt floor of the samplers is reproduced bit for bit by NumPy float32.  Only expf, logf,
log1pf and cosf can differ from the device, by units in the last place; here they are evaluated in float64 and rounded once.
ROCm's installed documentation states no accuracy for the device's math functions, so ULP_BOUND falls back to 4 ulp for each of
them.  Next to every draw comes a `fragile` mask: True where a decision that hangs on such a function (the multiplication
method's `prod > limit`, PTRS's slow-path inequality) is closer to its threshold, evaluated in float64 from the same uniforms,
than that error explains.  Such a decision also sets how many words the pixel consumes, so once a pixel is fragile every later
draw of its stream is fragile too.  `uniform` is exact and never fragile by itself."""
import math

import numpy as np

F = np.float32
U32 = np.uint32
ULP_BOUND = 4                       # device ulp of expf, logf, log1pf, cosf (fallback: see the module docstring)
CTR3 = 0x5114EBE2
TWO_PI = F(6.28318530717958647692)

_lgamma = np.frompyfunc(math.lgamma, 1, 1)


def lgamma64(x):
    return _lgamma(np.asarray(x, np.float64)).astype(np.float64)


def ulp(x):
    """Spacing of float32 at |x|."""
    return np.spacing(np.abs(np.asarray(x)).astype(F)).astype(np.float64)


def philox4x32_10(counter, key):
    """counter uint32[...,4], key uint32[...,2] -> uint32[...,4]: ten rounds of Philox::round()."""
    c = np.asarray(counter, np.uint64) & np.uint64(0xFFFFFFFF)
    k = np.broadcast_to(np.asarray(key, np.uint64) & np.uint64(0xFFFFFFFF), c.shape[:-1] + (2,))
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = k[..., 0].copy(), k[..., 1].copy()
    m32, sh = np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        n0, n2 = (p1 >> sh) ^ c1 ^ k0, (p0 >> sh) ^ c3 ^ k1
        c0, c1, c2, c3 = n0, p1 & m32, n2, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack([c0, c1, c2, c3], -1).astype(U32)


def uniform_of(word):
    """Rng::uniform of one 32-bit word: in (0, 1] -- the largest 24-bit value rounds up to 2^24 when 0.5 is added."""
    return ((np.asarray(word, U32) >> U32(8)).astype(F) + F(0.5)) * F(1.0 / 16777216.0)


class Stream:
    """The Rng objects of every pixel of image `image` of an H x W launch with the key `seed` (seed_lo = its low 32 bits,
    seed_hi the next 32).  Every draw takes an optional bool mask [H,W] `active`: the pixels that draw; the others consume
    nothing and get 0.  Draws come back as [H,W] arrays."""

    WORDS = (3, 2, 1, 0)            # Rng::next hands a block out back to front (buf[--left])

    def __init__(self, seed, H, W, image):
        self.H, self.W, n = int(H), int(W), int(H) * int(W)
        self.key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], U32)
        self.ctr0 = np.arange(n, dtype=np.uint64).astype(U32)      # y * W + x
        self.ctr1 = int(image) & 0xFFFFFFFF
        self.sub = np.zeros(n, U32)
        self.buf = np.zeros((n, 4), U32)
        self.left = np.zeros(n, np.int64)
        self.tainted = np.zeros(n, bool)                           # a fragile decision has set what the pixel consumed
        self.words = np.array(self.WORDS, np.int64)

    # ---- flat [n] forms ----------------------------------------------------------------------------------------------
    def _mask(self, active):
        if active is None:
            return np.ones(self.H * self.W, bool)
        return np.broadcast_to(np.asarray(active, bool), (self.H, self.W)).reshape(-1)

    def _next(self, act):
        idx = np.nonzero(act & (self.left == 0))[0]
        if idx.size:
            ctr = np.empty((idx.size, 4), U32)
            ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = self.ctr0[idx], self.ctr1, self.sub[idx], CTR3
            self.buf[idx] = philox4x32_10(ctr, self.key)
            self.sub[idx] += U32(1)
            self.left[idx] = 4
        out = np.zeros(act.shape, U32)
        idx = np.nonzero(act)[0]
        out[idx] = self.buf[idx, self.words[4 - self.left[idx]]]
        self.left[idx] -= 1
        return out

    def _uniform(self, act):
        return np.where(act, uniform_of(self._next(act)), F(0)).astype(F)

    def _normal(self, act):
        u1, u2 = self._uniform(act), self._uniform(act)
        with np.errstate(divide="ignore", invalid="ignore"):
            lg = np.log(u1.astype(np.float64)).astype(F)
            r = np.sqrt(F(-2.0) * lg)
            n = r * np.cos((TWO_PI * u2).astype(np.float64)).astype(F)
        return np.where(act, n, F(0)).astype(F), np.where(act, r, F(0)).astype(F)

    # ---- the draws -----------------------------------------------------------------------------------------------------
    def _sq(self, a):
        return a.reshape(self.H, self.W)

    def next_u32(self, active=None):
        return self._sq(self._next(self._mask(active)))

    def uniform(self, active=None):
        return self._sq(self._uniform(self._mask(active)))

    def normal(self, active=None):
        """(n, fragile, tol): Box-Muller, sqrtf(-2 logf(u1)) * cosf(2 pi u2).  tol bounds |device - n|:
        ULP_BOUND * 2^-24 * (|n| + sqrt(-2 log u1))."""
        act = self._mask(active)
        n, r = self._normal(act)
        tol = (ULP_BOUND * 2.0 ** -24) * (np.abs(n).astype(np.float64) + r.astype(np.float64))
        return self._sq(n), self._sq(self.tainted & act), self._sq(tol)

    def poisson(self, lam, active=None):
        """(k, fragile): Rng::poisson(lam), lam float32 [H,W] or a scalar."""
        act = self._mask(active)
        lam = np.broadcast_to(np.asarray(lam, F), (self.H, self.W)).reshape(-1)
        with np.errstate(invalid="ignore"):
            pos = act & (lam > F(0))
            small, large = pos & (lam < F(10.0)), pos & ~(lam < F(10.0))
        k = np.zeros(act.shape, F)
        if small.any():
            self._poisson_small(lam, small, k)
        if large.any():
            self._poisson_ptrs(lam, large, k)
        return self._sq(k), self._sq(self.tainted & act)

    def _poisson_small(self, lam, go, k):
        """Multiplication method: k = number of uniforms whose running product stays above exp(-lam)."""
        lam64 = np.where(go, lam, F(1)).astype(np.float64)
        limit64 = np.exp(-lam64)
        limit = limit64.astype(F)
        margin = ULP_BOUND * ulp(limit)
        prod = self._uniform(go)
        go = go.copy()
        while True:
            self.tainted |= go & (np.abs(prod.astype(np.float64) - limit64) <= margin)
            go &= (prod > limit) & (k < F(200))
            if not go.any():
                return
            prod = np.where(go, prod * self._uniform(go), prod).astype(F)
            k[go] += F(1)

    @staticmethod
    def _log_weight(k, lam, f64):
        """Rng::log_weight in its operation order: float32 with each transcendental rounded once, or all in float64.  Also
        the largest magnitude among its terms, which scales its error."""
        T = np.float64 if f64 else F
        k, lam = k.astype(T), lam.astype(T)

        def fn(g, x):
            return g(np.asarray(x, np.float64)).astype(T)

        out, mag = np.zeros(k.shape, T), np.zeros(k.shape)
        lo = k < 10
        if lo.any():
            a, g = k[lo] * fn(np.log, lam[lo]), fn(lgamma64, k[lo] + T(1))
            out[lo] = -lam[lo] + a - g
            mag[lo] = np.maximum(np.maximum(lam[lo], np.abs(a)), np.abs(g))
        hi = ~lo
        if hi.any():
            kk, d = k[hi], lam[hi] - k[hi]
            ik = T(1) / kk
            series = ik * (T(F(0.0833333333)) - T(F(0.00277777778)) * (ik * ik))
            a, h = kk * fn(np.log1p, d * ik), T(0.5) * fn(np.log, T(TWO_PI) * kk)
            out[hi] = ((a - d) - h) - series
            mag[hi] = np.maximum(np.maximum(np.abs(a), np.abs(d)), np.maximum(h, np.abs(out[hi])))
        return out, mag

    def _slow_accept(self, lhs, k, lam, mags):
        """PTRS's slow path: (accept, fragile) of `lhs <= log_weight(k, lam)`.  The left-hand side is one logf of an argument
        that float32 arithmetic fixes: ULP_BOUND ulp of its magnitude `mags`, and one for the rounding here; the right
        one at most two transcendentals (log1pf and logf; below k = 10 logf and a table of log k!) and six roundings, each at
        most an ulp of the largest magnitude among its terms.  Fragile: the two sides, in float64 from the same float32
        inputs, lie closer than the sum of these, or the float32 and the float64 decision differ."""
        rhs, _ = self._log_weight(k, lam, False)
        rhs64, mag = self._log_weight(k, lam, True)
        margin = (ULP_BOUND + 1) * ulp(mags) + (2 * ULP_BOUND + 6) * ulp(mag)
        accept, d = lhs <= rhs, lhs.astype(np.float64) - rhs64
        return accept, (np.abs(d) <= margin) | (accept != (d <= 0.0))

    def _poisson_ptrs(self, lam, go, k_out):
        """Hoermann's transformed rejection with squeeze, at most 64 proposals, then floorf(lam + 0.5f)."""
        with np.errstate(all="ignore"):
            lam = np.where(go, lam, F(16)).astype(F)
            slam = np.sqrt(lam)
            b = F(0.931) + F(2.53) * slam
            a = F(-0.059) + F(0.02483) * b
            inv_alpha = F(1.1239) + F(1.1328) / (b - F(3.4))
            vr = F(0.9277) - F(3.6224) / (b - F(2.0))
            pending = go.copy()
            for _ in range(64):
                if not pending.any():
                    return
                U = self._uniform(pending) - F(0.5)
                V = self._uniform(pending)
                us = F(0.5) - np.abs(U)
                k = np.floor((F(2.0) * a / us + b) * U + lam + F(0.43))
                fast = pending & (us >= F(0.07)) & (V <= vr)
                k_out[fast] = k[fast]
                pending &= ~fast
                slow = pending & ~((k < F(0)) | ((us < F(0.013)) & (V > us)))
                idx = np.nonzero(slow)[0]
                if idx.size:
                    t = a[idx] / (us[idx] * us[idx]) + b[idx]
                    lhs = np.log((V[idx] * inv_alpha[idx] / t).astype(np.float64)).astype(F)
                    mags = np.abs(lhs)
                    acc, frag = self._slow_accept(lhs, k[idx], lam[idx], mags)
                    self.tainted[idx[frag]] = True
                    k_out[idx[acc]] = k[idx[acc]]
                    pending[idx[acc]] = False
            k_out[pending] = np.floor(lam[pending] + F(0.5))
