"""The step, noise and NLL kernels of csrc/misc.hip (posterior_kernel, vb_terms_kernel / vb_final_kernel, prior_bpd_kernel,
q_sample_kernel / q_sample_prev_kernel, randn_kernel) restated from the reference's source lines: in float64 on the float32 table
values the engine is handed, with the forward rounding bound of every output; in numpy float32 in the reference's operation order
(with seedable mistakes, for tests/test_step_nll_cpu.py); and the inputs both test files run on.  numpy only.

Bounds.  Every float32 operation is one relative error of 2^-24 on its result; the bound carries these through the expression as
an INTERVAL (class Iv): each operation maps the operands' intervals to the exact result's interval and widens it outward by 2^-24 of
its end points.  An interval holds the exact value of every partial expression as well as every rounded one, so a product that is
fused into the following sum (one rounding instead of two) lies inside the same interval: either rounding of `a x - b eps` is allowed.
Division by sqrt_recipm1 (smallest at t = 0: 0.0100 linear, 0.0064 cosine) and the radicand 1 - abp - sigma^2 are carried the same
way; a clamp maps both ends and cannot widen.  A device math call (expf, logf, tanhf, sincosf) gets K_ULP units in the last place.

K_ULP = 4 is an ASSUMPTION: no copy of the HIP math API's ULP table is installed with ROCm here.  The GPU tests print their largest
|error| / bound per kernel; a ratio above 1 where the float32 restatement is inside is a finding about the kernel, not about K_ULP.
"""
import numpy as np

U = 2.0 ** -24
K_ULP = 4
F = np.float32
_GROW = 1.0 + 2.0 ** -20            # second-order terms, and the float64 arithmetic the intervals themselves are computed in
CLAMP = float(F(1e-12))             # x.clamp(min=1e-12) on a float32 tensor
FMAX = 3.4028234e38

ROWS = dict(sr="sqrt_recip_alphas_cumprod", srm1="sqrt_recipm1_alphas_cumprod", c1="posterior_mean_coef1", c2="posterior_mean_coef2",
            ab="alphas_cumprod", abp="alphas_cumprod_prev", sa="sqrt_alphas_cumprod", s1="sqrt_one_minus_alphas_cumprod",
            tlv="posterior_log_variance_clipped", l1m="log_one_minus_alphas_cumprod")


def tables(diff):
    """name -> float32 row: the casts _extract_into_tensor yields (gather in float64, THEN .float()), which is elementwise.
    `lv` is the model's log variance (gaussian_diffusion.py:299-317).  diff: the diffusion object, or an oracle ScheduleRef."""
    get = lambda name: getattr(diff, name) if hasattr(diff, name) else np.log(1.0 - diff.alphas_cumprod)    # noqa: E731  (the oracle keeps no log_one_minus row)
    tab = {k: np.asarray(get(name), np.float64).astype(F) for k, name in ROWS.items()}
    lv = diff._model_log_variance() if hasattr(diff, "_model_log_variance") else diff.model_log_variance
    tab["lv"] = np.asarray(lv, np.float64).astype(F)
    tab["NT"] = int(diff.num_timesteps)
    return tab


# ------------------------------------------------------------------------------------------------------------ intervals
class Iv:
    """[lo, hi] of float64 arrays.  Every arithmetic method rounds: it widens the exact result's interval by 2^-24 of its ends."""
    __slots__ = ("lo", "hi")
    w = U * _GROW

    def __init__(self, lo, hi=None):
        self.lo = np.asarray(lo, np.float64)
        self.hi = self.lo if hi is None else np.asarray(hi, np.float64)

    @classmethod
    def _r(cls, lo, hi, k=1.0):
        return cls(lo - k * cls.w * np.abs(lo), hi + k * cls.w * np.abs(hi))

    @classmethod
    def of(cls, v):
        return v if isinstance(v, Iv) else cls(v)

    def __add__(self, o):
        o = self.of(o)
        return self._r(self.lo + o.lo, self.hi + o.hi)

    def __sub__(self, o):
        o = self.of(o)
        return self._r(self.lo - o.hi, self.hi - o.lo)

    def __mul__(self, o):
        o = self.of(o)
        p = [self.lo * o.lo, self.lo * o.hi, self.hi * o.lo, self.hi * o.hi]
        return self._r(np.minimum(np.minimum(p[0], p[1]), np.minimum(p[2], p[3])), np.maximum(np.maximum(p[0], p[1]), np.maximum(p[2], p[3])))

    __radd__ = __add__
    __rmul__ = __mul__

    def __rsub__(self, o):
        return self.of(o) - self

    def div_pos(self, o):
        """self / o for o > 0."""
        o = self.of(o)
        q = [self.lo / o.lo, self.lo / o.hi, self.hi / o.lo, self.hi / o.hi]
        return self._r(np.minimum(np.minimum(q[0], q[1]), np.minimum(q[2], q[3])), np.maximum(np.maximum(q[0], q[1]), np.maximum(q[2], q[3])))

    def sq(self):
        a, b = np.abs(self.lo), np.abs(self.hi)
        lo = np.where((self.lo <= 0) & (self.hi >= 0), 0.0, np.minimum(a, b)) ** 2
        return self._r(lo, np.maximum(a, b) ** 2)

    def sqrt(self):
        """correctly rounded; a radicand interval that reaches below 0 is cut there (the exact value is >= 0)."""
        return self._r(np.sqrt(np.maximum(self.lo, 0.0)), np.sqrt(np.maximum(self.hi, 0.0)))

    def exp(self):
        return self._r(np.exp(self.lo), np.exp(self.hi), 2.0 * K_ULP)

    # exact in float32: no widening
    def __neg__(self):
        return type(self)(-self.hi, -self.lo)

    def times_exact(self, c):
        """c >= 0 a power of two, 0 or 1 (per element)."""
        return type(self)(self.lo * c, self.hi * c)

    def clip(self, a, b):
        return type(self)(np.clip(self.lo, a, b), np.clip(self.hi, a, b))

    def nan_where_nonfinite(self, src):
        """where the exact value `src` is not finite the result is NaN: the engine neither clamps such an x_0 into range nor passes an
        infinity on (the reference's clamp would make it +-1)."""
        bad = ~np.isfinite(src)
        return type(self)(np.where(bad, np.nan, self.lo), np.where(bad, np.nan, self.hi))


class Ex(Iv):
    """The same expressions without rounding: lo == hi == the float64 value."""
    w = 0.0

    @classmethod
    def _r(cls, lo, hi, k=1.0):
        return cls(lo, hi)                                                   # (0 * inf would turn an infinite value into NaN)

    def exp(self):
        return type(self)(np.exp(self.lo), np.exp(self.hi))


def _hull(exact, iv):
    """(want, bound): the float64 value and the largest distance to an end of the interval."""
    want = exact.lo
    with np.errstate(invalid="ignore"):
        return want, np.maximum(iv.hi - want, want - iv.lo)


def ratio(got, want, bound):
    """Per element |got - want| / bound.  Where `want` is not finite `got` must be of the same kind (NaN, +inf, -inf): 0 or inf."""
    got, want, bound = np.broadcast_arrays(np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64))
    fin = np.isfinite(want)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(got - want)
        r = np.where(bound > 0, d / bound, np.where(d == 0, 0.0, np.inf))
    same = np.where(np.isnan(want), np.isnan(got), got == want)
    r = np.where(fin, r, np.where(same, 0.0, np.inf))
    return np.where(np.isnan(r), np.inf, r)                                 # got NaN where want is finite


def ratio_in(got, lo, hi):
    """Distance of `got` outside [lo, hi] in units of the interval's half width plus 1: <= 1 inside, > 1 outside."""
    got, lo, hi = np.broadcast_arrays(np.asarray(got, np.float64), np.asarray(lo, np.float64), np.asarray(hi, np.float64))
    inside = (got >= lo) & (got <= hi)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(half > 0, np.abs(got - mid) / half, np.where(got == mid, 0.0, np.inf))
    both_nan = np.isnan(lo) & np.isnan(got)
    return np.where(both_nan, 0.0, np.where(inside, np.minimum(r, 1.0), np.where(np.isnan(r), np.inf, np.maximum(r, 1.0 + 1e-12))))


def _rows(tab, t, wrap=False):
    """name -> (B, 1) float64 of the float32 row entries at t[b]; NaN for an index outside the table (IndexError in the reference)."""
    t = np.asarray(t, np.int64)
    NT = tab["NT"]
    if wrap:
        t = np.where(t < 0, t + NT, t)
    ok = (t >= 0) & (t < NT)
    tc = np.where(ok, t, 0)
    out = {k: np.where(ok, v[tc].astype(np.float64), np.nan)[:, None] for k, v in tab.items() if k != "NT"}
    out["ok"] = ok
    return out


# ------------------------------------------------------------------------------------------------------------ posterior
def _posterior(A, tab, x, src, t, mode, eta, clip, noise, given):
    c = _rows(tab, t)
    t = np.asarray(t, np.int64)
    X = A(x)
    with np.errstate(invalid="ignore", over="ignore"):
        if given:
            x0 = A(src)                                                       # process_xstart(denoised_fn(...)) handed back
        else:
            x0 = A(c["sr"]) * X - A(c["srm1"]) * A(src)                       # :374-382
        raw = c["sr"] * np.asarray(x, np.float64) - c["srm1"] * np.asarray(src, np.float64) if not given else np.asarray(src, np.float64) + 0.0 * c["sr"]
        if clip:
            x0 = x0.clip(-1.0, 1.0)                                           # :322-323
        x0 = x0.nan_where_nonfinite(raw)
        mean = A(c["c1"]) * x0 + A(c["c2"]) * X                               # :216-220
        nz = (t != 0).astype(np.float64)[:, None]                             # :438-440, :631
        if mode == 0:
            sd = A(c["lv"]).times_exact(0.5).exp()
            sample = mean + sd.times_exact(nz) * A(noise)                     # :441-443
        else:
            e = (A(c["sr"]) * X - x0).div_pos(c["srm1"])                      # :392-396
            ab, abp = A(c["ab"]), A(c["abp"])
            sigma = (A(float(F(eta))) * (1.0 - abp).div_pos(1.0 - ab).sqrt()) * (1.0 - ab.div_pos(abp)).sqrt()      # :625-626
            mean_pred = x0 * abp.sqrt() + ((1.0 - abp) - sigma.sq()).sqrt() * e                                    # :629-630
            sample = mean_pred + sigma.times_exact(nz) * A(noise)             # :633
    return dict(pred_xstart=x0, mean=mean, sample=sample)


def posterior_fp64(tab, x, src, t, mode, eta, clip, noise, given):
    """p_sample (mode 0: gaussian_diffusion.py:319-343,374-382,208-227,438-443) / ddim_sample (mode 1: :597-634) in float64.
    x, src, noise: (B, per) float32; src is eps, or with `given` the x_0 prediction; t: (B,).  -> dict of pred_xstart, mean, sample.
    Items whose t is outside the table are NaN."""
    return {k: v.lo for k, v in _posterior(Ex, tab, x, src, t, mode, eta, clip, noise, given).items()}


def posterior_bound(tab, x, src, t, mode, eta, clip, noise, given):
    """-> dict of (want, bound) per output: the float64 value and the forward rounding bound of a float32 evaluation."""
    ex, iv = (_posterior(A, tab, x, src, t, mode, eta, clip, noise, given) for A in (Ex, Iv))
    return {k: _hull(ex[k], iv[k]) for k in ex}


# ------------------------------------------------------------------------------------------------------------ q_sample
def _q_sample(A, tab, x0, t, noise):
    c = _rows(tab, t, wrap=True)                                              # a negative index counts from the end (:565-568 at t = 0)
    return A(c["sa"]) * A(x0) + A(c["s1"]) * A(noise)                         # :203-206


def q_sample_fp64(tab, x0, t, noise):
    return _q_sample(Ex, tab, x0, t, noise).lo


def q_sample_bound(tab, x0, t, noise):
    """(want, bound): three roundings (two products and a sum), fused or not."""
    return _hull(_q_sample(Ex, tab, x0, t, noise), _q_sample(Iv, tab, x0, t, noise))


# ------------------------------------------------------------------------------------------------------------ NLL terms
def _cdf(y):
    """losses.py:38-43 in float64."""
    return 0.5 * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (y + 0.044715 * y ** 3)))


def xstart_bound(tab, xt, src, t, clip, start_x):
    """(want, bound) of pred_xstart as _vb_terms_bpd's p_mean_variance forms it (:326-341)."""
    o = posterior_bound(tab, xt, src, t, 0, 0.0, clip, np.zeros_like(xt), bool(start_x))
    return o["pred_xstart"]


def vb_term_interval(tab, xs, xt, x0, t):
    """Per element, in nats and without the mask: (lo, hi) that the float32 term of _vb_terms_bpd (:769-787; losses.py:13-76) must lie
    in, given the float32 pred_xstart `x0` the same call returned.
    t > 0: the KL term as an interval of the kind above.
    t == 0: the decoder NLL is ill-conditioned where both CDFs saturate, so the interval follows the conditioning: the argument
    arg = inv_stdv (xs - mean +- 1/255) carries E_arg = inv_stdv 2^-23 (|xs| + |c1 x0| + |c2 xt| + 1/255) + K 2^-23 |arg|, the CDF value an
    absolute K 2^-24; both go through the float64 CDF (monotone), the branch is chosen by the float32 comparison against -0.999f /
    0.999f, and the term lies in [-log(max(d_hi, 1e-12)), -log(max(d_lo, 1e-12))] widened by logf's K ulp."""
    c = _rows(tab, t)
    t = np.asarray(t, np.int64)
    xs32, xs, xt, x0 = np.asarray(xs, F), np.asarray(xs, np.float64), np.asarray(xt, np.float64), np.asarray(x0, np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        # KL(q(x_{t-1} | x_t, x_0) || p(x_{t-1} | x_t)), losses.py:13-35 with mean1 = true mean, logvar1 = tlv, mean2 = mean, logvar2 = lv
        out = []
        for A in (Ex, Iv):
            mean = A(c["c1"]) * A(x0) + A(c["c2"]) * A(xt)
            tmean = A(c["c1"]) * A(xs) + A(c["c2"]) * A(xt)
            lv, tlv = A(c["lv"]), A(c["tlv"])
            kl = ((((-1.0 + lv) - tlv) + (tlv - lv).exp()) + (tmean - mean).sq() * (-lv).exp()).times_exact(0.5)
            out.append(kl)
        kl_lo, kl_hi = out[1].lo, out[1].hi
        # decoder NLL, losses.py:46-76 with log_scales = 0.5 lv
        inv = np.exp(-0.5 * c["lv"])
        c1x0, c2xt = c["c1"] * x0, c["c2"] * xt
        cx = xs - (c1x0 + c2xt)
        q = float(F(1.0 / 255.0))
        e_cdf = K_ULP * U
        ends = {}
        for name, sgn in (("plus", 1.0), ("min", -1.0)):
            arg = inv * (cx + sgn * q)
            e_arg = inv * 2.0 * U * (np.abs(xs) + np.abs(c1x0) + np.abs(c2xt) + q) + K_ULP * 2.0 * U * np.abs(arg)
            ends[name] = (_cdf(arg - e_arg) - e_cdf, _cdf(arg + e_arg) + e_cdf)
        low, high = xs32 < F(-0.999), xs32 > F(0.999)
        d_lo = np.where(low, ends["plus"][0], np.where(high, 1.0 - ends["min"][1], ends["plus"][0] - ends["min"][1]))
        d_hi = np.where(low, ends["plus"][1], np.where(high, 1.0 - ends["min"][0], ends["plus"][1] - ends["min"][0]))
        d_lo, d_hi = d_lo - U * np.abs(d_lo), d_hi + U * np.abs(d_hi)      # the subtraction's rounding
        n_lo, n_hi = -np.log(np.maximum(d_hi, CLAMP)), -np.log(np.maximum(d_lo, CLAMP))
        n_lo, n_hi = n_lo - K_ULP * 2.0 * U * np.abs(n_lo), n_hi + K_ULP * 2.0 * U * np.abs(n_hi)
    z = (t == 0)[:, None]
    lo, hi = np.where(z, n_lo, kl_lo), np.where(z, n_hi, kl_hi)
    bad = ~c["ok"][:, None]
    return np.where(bad, np.nan, lo), np.where(bad, np.nan, hi)


def mse_intervals(tab, xs, xt, x0, t, noise):
    """Per element (lo, hi) of (x0 - xs)^2 and of (_predict_eps_from_xstart(x_t, t, x0) - noise)^2 (:975-990, :392-396)."""
    c = _rows(tab, t)
    with np.errstate(invalid="ignore"):
        a = (Iv(x0) - Iv(xs)).sq()
        e = ((Iv(c["sr"]) * Iv(xt) - Iv(x0)).div_pos(c["srm1"]) - Iv(noise)).sq() if noise is not None else None
    return (a.lo, a.hi), (None if e is None else (e.lo, e.hi))


def elem_mask(mask, B, T, per):
    """(B, per) float64: mean_flat(tensor, mask) broadcasts the (B, T, 1, 1, 1) mask over a frame's per / T elements; None: ones."""
    if mask is None:
        return np.ones((B, per))
    return np.repeat(np.asarray(mask, np.float64).reshape(B, T), per // T, axis=1)


def item_mean(lo, hi, m, bits=False):
    """nn.py:73-77: (tensor * mask).mean over ALL elements.  The product with the mask rounds once (exactly, for 0, 1 and 0.5), the
    engine sums in float64, and the mean is cast to float32 once; `bits`: divided by ln 2 (a float32 constant: three more roundings
    allow for the reciprocal's own, the product's and the reference's division instead)."""
    lo, hi = lo * m, hi * m
    lo, hi = lo - U * np.abs(lo), hi + U * np.abs(hi)
    lo, hi = lo.mean(axis=1), hi.mean(axis=1)
    k = (4.0 if bits else 1.0) * U * _GROW
    s = 1.0 / np.log(2.0) if bits else 1.0
    lo, hi = lo * s, hi * s
    return lo - k * np.abs(lo), hi + k * np.abs(hi)


def _prior(A, tab, xs):
    NT = tab["NT"]
    sa, lv = float(tab["sa"][NT - 1]), float(tab["l1m"][NT - 1])
    mu = A(sa) * A(xs)                                                        # q_mean_variance, :174-188
    return ((((-1.0 + A(0.0)) - A(lv)) + A(lv).exp()) + mu.sq()).times_exact(0.5)     # normal_kl(mean, logvar, 0, 0)


def prior_bpd_fp64(tab, xs, m):
    """_prior_bpd (:909-926) in float64, bits per dimension per item.  xs: (B, per); m: elem_mask(...)."""
    return (_prior(Ex, tab, xs).lo * m).mean(axis=1) / np.log(2.0)


def prior_bpd_interval(tab, xs, m):
    iv = _prior(Iv, tab, xs)
    return item_mean(iv.lo, iv.hi, m, bits=True)


def posterior_ratios(tab, x, src, t, mode, eta, clip, noise, given, got):
    """name -> largest |got - want| / bound over the elements, for the outputs present in `got`."""
    b = posterior_bound(tab, x, src, t, mode, eta, clip, noise, given)
    return {k: float(ratio(v, *b[k]).max()) for k, v in got.items() if v is not None}


def vb_ratios(tab, xs, xt, src, t, clip, start_x, noise, m, got):
    """got: pred_xstart (B, per) and the per-item vb (bits), xstart_mse and, with `noise`, mse -> name -> largest ratio.  The term and
    the two squared errors are bounded on the float32 pred_xstart the same call returned; pred_xstart itself on `src`."""
    x0 = got["pred_xstart"]
    r = {"pred_xstart": float(ratio(x0, *xstart_bound(tab, xt, src, t, clip, start_x)).max())}
    r["vb"] = float(ratio_in(got["vb"], *item_mean(*vb_term_interval(tab, xs, xt, x0, t), m, bits=True)).max())
    a, e = mse_intervals(tab, xs, xt, x0, t, noise)
    r["xstart_mse"] = float(ratio_in(got["xstart_mse"], *item_mean(*a, m)).max())
    if noise is not None:
        r["mse"] = float(ratio_in(got["mse"], *item_mean(*e, m)).max())
    return r


# ------------------------------------------------------------------------------------------------------------ Philox4x32-10
M32 = 0xFFFFFFFF


def philox4x32_10(counter4, key2):
    """Philox4x32-10 (Salmon et al., SC'11) in plain integers: Python ints, or numpy uint64 arrays holding 32-bit words."""
    c0, c1, c2, c3 = counter4
    k0, k1 = key2
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def _u64(v):
    return np.asarray(v, np.uint64)


def philox_words(seed, offset, i):
    """(4, n) uint64: the block of element i -- counter {lo32(offset + i // 4), hi32, 0x5eed5eed, 0}, key {lo32(seed), hi32(seed)}."""
    i = np.asarray(i, np.uint64)
    ctr = (np.uint64(offset % 2 ** 64) + (i >> np.uint64(2)))                # wraps modulo 2^64 like the kernel's unsigned sum
    seed = int(seed) % 2 ** 64
    m, s32 = np.uint64(M32), np.uint64(32)
    r = philox4x32_10((ctr & m, ctr >> s32, np.full(i.shape, 0x5EED5EED, np.uint64), np.zeros(i.shape, np.uint64)),
                      (np.uint64(seed & M32), np.uint64(seed >> 32)))
    return np.stack([_u64(v) for v in r])


def _uniforms(seed, offset, i, pairs="adjacent", plus_one=True):
    """float32 (u1, angle) of element i, to the bit: conversions, one addition and exact or single multiplications only."""
    i = np.asarray(i, np.uint64)
    r = philox_words(seed, offset, i)
    cols = np.arange(i.size)
    pair = (i & np.uint64(2)).astype(np.int64)
    first, second = (pair, pair + 1) if pairs == "adjacent" else (pair // 2, pair // 2 + 2)      # the mistake: (0,2),(1,3)
    ra, rb = r[first, cols].astype(F), r[second, cols].astype(F)
    u1 = ((ra + F(1.0)) if plus_one else ra) * F(2.0 ** -32)
    return u1, F(6.283185307179586) * (rb * F(2.0 ** -32))


def normal_fp64(seed, offset, i):
    """Element i of the stream (seed, offset): Box-Muller on the float32 (u1, angle) in float64, cosine for even i, sine for odd.
    -> (value, rad)."""
    i = np.asarray(i, np.uint64)
    u1, ang = _uniforms(seed, offset, i)
    rad = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    a = ang.astype(np.float64)
    return rad * np.where((i & np.uint64(1)) == 1, np.sin(a), np.cos(a)), rad


def normal_bound(rad):
    """Generous on purpose: a wrong bit anywhere in Philox moves the value by order 1."""
    return 16.0 * U * np.maximum(1.0, rad)


def normal_f32(seed, offset, i, mistake=None):
    i = np.asarray(i, np.uint64)
    u1, ang = _uniforms(seed, offset, i, pairs="split" if mistake == "pairs_02_13" else "adjacent", plus_one=mistake != "u1_plus_one_dropped")
    with np.errstate(divide="ignore", invalid="ignore"):
        rad = np.sqrt(F(-2.0) * np.log(u1))
        out = rad * np.where((i & np.uint64(1)) == 1, np.sin(ang), np.cos(ang))
    assert out.dtype == F
    return out


RANDN_CASES = [(0, 0), (5, 7), (2 ** 63 + 11, 2 ** 32 - 2)]
# A fourth stream, found by a search over counters: Philox block 132087 of seed 5 has the word 526 in its first u1 slot, so element
# 2000 of the stream at offset 131587 draws u1 = 527 2^-32 with the +1 and 526 2^-32 without it (0.03 % in the radius of 5.6).  From
# 2^24 on the float32 sum r + 1 rounds back to r: a dropped +1 shows only at a small word, and none of the three streams above has
# one within 4099 elements.
RANDN_SMALL_U1 = (5, 131587, 2000, 526)
RANDN_N = 4099


# ------------------------------------------------------------------------------------------------------------ float32 restatement
def _f(v):
    return np.asarray(v, F)


def _muladd(a, b, c, d, fused):
    """a b + c d in float32; fused: the first product exact inside the sum (one rounding less), through float64."""
    a, b, c, d = _f(a), _f(b), _f(c), _f(d)
    cd = c * d
    if fused:
        return (a.astype(np.float64) * b.astype(np.float64) + cd.astype(np.float64)).astype(F)
    return a * b + cd


def _mulsub1(a, b, c, fused):
    """a b - c."""
    a, b, c = _f(a), _f(b), _f(c)
    if fused:
        return (a.astype(np.float64) * b.astype(np.float64) - c.astype(np.float64)).astype(F)
    return a * b - c


def _addmul(m, a, b, fused):
    """m + a b."""
    m, a, b = _f(m), _f(a), _f(b)
    if fused:
        return (m.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(F)
    return m + a * b


def _rows32(tab, t, wrap=False):
    return {k: (v if k == "ok" else v.astype(F)) for k, v in _rows(tab, t, wrap).items()}


def _xstart32(c, x, src, given, clip, fused, mistake, nan_bad=True):
    """nan_bad: posterior_kernel writes a non-finite x_0 as NaN; vb_terms_kernel leaves it as it is (and unclamped)."""
    x0 = _f(src) if given else _muladd(c["sr"], x, -c["srm1"], src, fused)
    if mistake == "clamp_before_nonfinite_test":
        x0 = np.clip(x0, F(-1), F(1)) if clip else x0
        bad = ~(np.abs(x0) <= F(FMAX))
    else:
        bad = ~(np.abs(x0) <= F(FMAX))
        if clip:
            x0 = np.where(bad, x0, np.clip(x0, F(-1), F(1)))
    if nan_bad:
        x0 = np.where(bad, F(np.nan), x0)
    return x0.astype(F), bad


def posterior_f32(tab, x, src, t, mode, eta, clip, noise, given, fused=False, mistake=None):
    """posterior_fp64's lines in numpy float32 (every operation rounded once; `fused`: products folded into the sums)."""
    t = np.asarray(t, np.int64)
    c = _rows32(tab, t)
    x, noise = _f(x), _f(noise)
    with np.errstate(invalid="ignore", over="ignore"):
        x0, _ = _xstart32(c, x, src, given, clip, fused, mistake)
        c1, c2 = (c["c2"], c["c1"]) if mistake == "coef1_coef2_swapped" else (c["c1"], c["c2"])
        mean = _muladd(c1, x0, c2, x, fused)
        nz = (t != 0) if mistake != "t0_switch_from_item0" else np.full(t.shape, t[0] != 0)
        nz = nz.astype(F)[:, None]
        if mode == 0:
            sample = _addmul(mean, nz * np.exp(F(0.5) * c["lv"]), noise, fused)
        else:
            e = _mulsub1(c["sr"], x, x0, fused) / c["srm1"]
            ab = c["ab"]
            abp = c["abp"] if mistake != "abp_read_at_t_minus_1" else tab["abp"][(t - 1) % tab["NT"]][:, None]
            et = F(1.0) if mistake == "eta_dropped_from_sigma" else F(eta)
            sigma = et * np.sqrt((F(1) - abp) / (F(1) - ab)) * np.sqrt(F(1) - ab / abp)
            rad = (F(1) - abp) - sigma * sigma if not fused else ((F(1) - abp).astype(np.float64) - sigma.astype(np.float64) ** 2).astype(F)
            mean_pred = _muladd(x0, np.sqrt(abp), np.sqrt(rad), e, fused)
            sample = _addmul(mean_pred, nz * sigma, noise, fused)
    out = dict(pred_xstart=x0, mean=mean, sample=sample)
    assert all(v.dtype == F for v in out.values())
    return out


def q_sample_f32(tab, x0, t, noise, fused=False, mistake=None):
    c = _rows32(tab, t, wrap=mistake != "index_minus_1_unwrapped")
    with np.errstate(invalid="ignore"):
        return _muladd(c["sa"], x0, c["s1"], noise, fused)


def _cdf32(y):
    return F(0.5) * (F(1.0) + np.tanh(F(0.7978845608028654) * (y + F(0.044715) * y * y * y)))


def vb_terms_f32(tab, xs, xt, src, t, clip, T, mask=None, start_x=False, noise=None, fused=False, mistake=None):
    """_vb_terms_bpd with the two squared errors of calc_bpd_loop_subsampled in numpy float32 -> dict: pred_xstart, term (per element,
    nats, unmasked) and the per-item vb (bits), xstart_mse, mse (float64 sums, one cast: the reduction is not what is restated)."""
    t = np.asarray(t, np.int64)
    c = _rows32(tab, t)
    xs, xt = _f(xs), _f(xt)
    B, per = xs.shape
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        x0, _ = _xstart32(c, xt, src, start_x, clip, fused, None, nan_bad=False)
        c1, c2 = (c["c2"], c["c1"]) if mistake == "coef1_coef2_swapped" else (c["c1"], c["c2"])
        lv, tlv = (c["tlv"], c["lv"]) if mistake == "logvar_and_post_logvar_exchanged" else (c["lv"], c["tlv"])
        mean, tmean = _muladd(c1, x0, c2, xt, fused), _muladd(c1, xs, c2, xt, fused)
        d = tmean - mean
        kl = F(0.5) * (F(-1.0) + lv - tlv + np.exp(tlv - lv) + _f(d * d) * np.exp(-lv))
        cx, inv, q = xs - mean, np.exp(F(-0.5) * lv), F(1.0 / 255.0)
        cp, cm = _cdf32(inv * (cx + q)), _cdf32(inv * (cx - q))
        thr = F(0.99) if mistake == "threshold_0.99" else F(0.999)
        eps12 = F(1e-12)
        low = np.log(np.maximum(cm if mistake == "cdf_min_in_low_branch" else cp, eps12))
        lp = np.where(xs < -thr, low, np.where(xs > thr, np.log(np.maximum(F(1.0) - cm, eps12)), np.log(np.maximum(cp - cm, eps12))))
        term = np.where((t == 0)[:, None], -lp, kl).astype(F)
        if mask is None:
            m = np.ones((B, per), F)
        else:
            fsz = per // T + (1 if mistake == "mask_index_fsz_plus_1" else 0)
            m = _f(mask).reshape(B, T)[:, np.minimum(np.arange(per) // fsz, T - 1)]
        den = m.astype(np.float64).sum(axis=1) if mistake == "mean_over_masked_count" else float(per)
        mean_of = lambda v: (_f(v).astype(np.float64).sum(axis=1) / den).astype(F)  # noqa: E731
        dx = x0 - xs
        out = dict(pred_xstart=x0, term=term, vb=mean_of(term * m) * F(1.4426950408889634), xstart_mse=mean_of(dx * dx * m))
        if noise is not None:
            e = _mulsub1(c["sr"], xt, x0, fused) / c["srm1"] - _f(noise)
            out["mse"] = mean_of(e * e * m)
    return out


def prior_bpd_f32(tab, xs, m, fused=False):
    NT = tab["NT"]
    sa, lv = tab["sa"][NT - 1], tab["l1m"][NT - 1]
    mu = sa * _f(xs)
    mu2 = mu * mu
    term = F(0.5) * (F(-1.0) - lv + np.exp(lv) + mu2) if not fused else \
        (0.5 * (np.float64(F(-1.0) - lv + np.exp(lv)) + mu.astype(np.float64) ** 2)).astype(F)
    return ((term * _f(m)).astype(np.float64).mean(axis=1)).astype(F) * F(1.4426950408889634)


# ------------------------------------------------------------------------------------------------------------ the inputs
SCHEDULES = [("linear_ddim250", dict(steps=1000, noise_schedule="linear", timestep_respacing="ddim250", sigma_small=False)),
             ("linear_1000", dict(steps=1000, noise_schedule="linear", timestep_respacing="", sigma_small=False)),
             ("cosine_1000_small", dict(steps=1000, noise_schedule="cosine", timestep_respacing="", sigma_small=True))]

POSTERIOR_COMBOS = [(0, 0.0)] + [(1, eta) for eta in (0.0, 0.5, 1.0)]         # (mode, eta)


def posterior_t(NT, B, variant=0):
    """Mixed per item, with 0, 1, NT - 2 and NT - 1."""
    pool = [[0, NT - 1, 1, NT - 2, NT // 2], [NT - 2, 0, NT // 2, 1, NT - 1]][variant]
    return np.array([pool[b % 5] for b in range(B)], np.int64)


def posterior_inputs(tab, t, per, seed):
    """x ~ N(0, 1); an x_0 target inside, at and outside +-1 (`given` hands it over as it is; eps = (sr x - target) / srm1 in float32
    brings the kernel's own x_0 to within rounding of it); noise ~ N(0, 1)."""
    rs = np.random.RandomState(seed)
    B = len(t)
    x = rs.randn(B, per).astype(F)
    target = rs.uniform(-1.5, 1.5, (B, per)).astype(F)
    target[:, ::7] = F(1.0)
    target[:, 3::7] = F(-1.0)
    target[:, 5::11] = np.nextafter(F(1.0), F(2.0))
    c = _rows32(tab, t)
    eps = ((c["sr"] * x - target) / c["srm1"]).astype(F)
    noise = rs.randn(B, per).astype(F)
    return x, target, eps, noise


XS_GRID = [F(-1.0), np.nextafter(F(-0.999), F(-2)), F(-0.999), np.nextafter(F(-0.999), F(0)), F(0.0), F(0.5),
           np.nextafter(F(0.999), F(0)), F(0.999), np.nextafter(F(0.999), F(2)), F(1.0)]
ERR_SIGMAS = [0.0] + [s * k for k in (0.5, 1, 3, 4, 5, 6, 7, 12, 40) for s in (1.0, -1.0)]
KL_ERRS = [0.0, 1e-3, -0.05, 0.4, -1.7]


def vb_grid(tab, start_x, seed=7):
    """One scalar scenario per batch item -> (xs, xt, src, noise, t), each (B,) (t: int64): the decoder grid at t = 0 (x_start at and
    next to the branch thresholds x prediction errors in units of sigma_0 = exp(lv[0] / 2)) and the KL grid at t in {1, 2, NT / 2,
    NT - 1}.  src is eps (float32 (sr x_t - target) / srm1) or, START_X, the target itself; x_t = q_sample(x_start, t, noise)."""
    NT = tab["NT"]
    rs = np.random.RandomState(seed)
    sig0 = float(np.exp(0.5 * np.float64(tab["lv"][0])))
    rows = [(xs, F(np.float64(xs) - k * sig0), 0) for xs in XS_GRID for k in ERR_SIGMAS]
    rows += [(xs, F(np.float64(xs) + e), tv) for tv in (1, 2, NT // 2, NT - 1) for xs in (F(-1.0), F(0.3), F(0.999)) for e in KL_ERRS]
    xs, target, t = _f([r[0] for r in rows]), _f([r[1] for r in rows]), np.array([r[2] for r in rows], np.int64)
    noise = rs.randn(len(rows)).astype(F)
    xt = q_sample_f32(tab, xs[:, None], t, noise[:, None])[:, 0]
    c = _rows32(tab, t)
    src = target if start_x else ((c["sr"][:, 0] * xt - target) / c["srm1"][:, 0]).astype(F)
    return xs, xt, src, noise, t


def masked_inputs(tab, B, T, per, seed):
    """Well-conditioned data for the masked sums: x_start in [-1, 1] with exact +-1 among it, t mixed with 0, decoder errors within
    3 sigma_0, per-frame masks drawn from {0, 1, 0.5} -> (xs, xt, eps, noise, t, mask (B, T))."""
    NT = tab["NT"]
    rs = np.random.RandomState(seed)
    t = np.array([[0, NT // 2, 1, NT - 1][b % 4] for b in range(B)], np.int64)
    xs = rs.uniform(-1, 1, (B, per)).astype(F)
    xs[:, ::13] = F(1.0)
    xs[:, 5::13] = F(-1.0)
    sig0 = float(np.exp(0.5 * np.float64(tab["lv"][0])))
    spread = np.where(t == 0, 3.0 * sig0, 0.1)[:, None]
    target = (xs + spread * rs.uniform(-1, 1, (B, per))).astype(F)
    noise = rs.randn(B, per).astype(F)
    xt = q_sample_f32(tab, xs, t, noise)
    c = _rows32(tab, t)
    eps = ((c["sr"] * xt - target) / c["srm1"]).astype(F)
    mask = rs.choice(np.array([0.0, 1.0, 0.5], F), size=(B, T)).astype(F)
    mask[:, 0], mask[:, -1] = F(1.0), F(0.5)                                # the first and the last frame always count
    return xs, xt, eps, noise, t, mask


def q_sample_inputs(NT, B, per, seed):
    rs = np.random.RandomState(seed)
    pool = [0, NT - 1, -1, NT // 2]
    t = np.array([pool[b % 4] for b in range(B)] if B != 3 else [-1, 0, NT - 1], np.int64)
    return rs.uniform(-1, 1, (B, per)).astype(F), t, rs.randn(B, per).astype(F)


SMALL = (3, 1001)                   # items unaligned to 256 and to 4
LARGE = (5, 250_003)                # more than 4096 * 256 elements: the grid-stride loop runs twice for some threads
VB_CALLS = [(clip, start_x, with_noise) for clip in (1, 0) for start_x in (False, True) for with_noise in (True, False)]


def posterior_cases(tab, large):
    """Argument tuples (x, src, t, mode, eta, clip, noise, given).  Small shape: every (mode, eta) x clip x eps / given x both t
    vectors; large shape: one p_sample call from eps and one DDIM call (eta = 0.5, clip off) on a given x_0."""
    NT = tab["NT"]
    if large:
        t = posterior_t(NT, LARGE[0])
        x, target, eps, noise = posterior_inputs(tab, t, LARGE[1], seed=11)
        yield (x, eps, t, 0, 0.0, 1, noise, False)
        yield (x, target, t, 1, 0.5, 0, noise, True)
        return
    for variant in (0, 1):
        t = posterior_t(NT, SMALL[0], variant)
        x, target, eps, noise = posterior_inputs(tab, t, SMALL[1], seed=3 + variant)
        for mode, eta in POSTERIOR_COMBOS:
            for clip in (1, 0):
                yield (x, eps, t, mode, eta, clip, noise, False)
                yield (x, target, t, mode, eta, clip, noise, True)


NONFINITE_AT = {"inf": (1, 17), "nan": (2, 900)}


def nonfinite_case(tab, kinds=("inf", "nan")):
    """The small shape with one eps element infinite and / or one NaN -> (x, eps, t, noise)."""
    t = posterior_t(tab["NT"], SMALL[0])
    x, _, eps, noise = posterior_inputs(tab, t, SMALL[1], seed=5)
    eps = eps.copy()
    for kind in kinds:
        eps[NONFINITE_AT[kind]] = np.inf if kind == "inf" else np.nan
    return x, eps, t, noise
