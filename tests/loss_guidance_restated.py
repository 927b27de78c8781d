"""Loss-guided sampling restated in numpy (no engine): the seed and final arithmetic of csrc/guide.hip in float32, exactly -- numpy's float32
products, sums and quotients are IEEE single roundings, the fused multiply-add is built from float64 (fma32) -- and the norm in float64
with the bound of its float32 value.

Per item b at index t, with a = sqrt_recip_alphas_cumprod[t], b = sqrt_recipm1_alphas_cumprod[t] as float32, on the frames with lat == 1:
    x_0r = a x_t - b eps                         two rounded products, one subtraction (xstart_from_eps)
    c_r  = cot where !clip or -1 <= x_0r <= 1, else 0
    d_eps = (-b) c_r,   d_x = a c_r              one rounding each
    g    = d_x + dx_net * inv_s                  inv_s a power of two: the product is exact, the sum rounds once
    n_b  = fp32(sqrt(sum g^2))                   the sum in float64
    m_b  = scale_b, or n_b == 0 ? 0 : fp32(scale_b / n_b)
    sample = fmaf(-m_b, g, sample')
and 0 (d_eps, d_x) / untouched (sample) on every other frame."""
import math

import numpy as np

F = np.float32
U = 2.0 ** -24


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays, exactly: the product is exact in float64, the sum's rounding error comes from TwoSum, and where the
    float64 sum lies on a float32 tie the error's sign decides."""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, F).astype(np.float64) for v in (a, b, c)))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    r = s.astype(F)
    lo, hi = np.nextafter(r, F(-np.inf)).astype(np.float64), np.nextafter(r, F(np.inf)).astype(np.float64)
    r64 = r.astype(np.float64)
    up = (s - r64 == (hi - r64) / 2) & (e > 0)
    down = (r64 - s == (r64 - lo) / 2) & (e < 0)
    return np.where(up, hi, np.where(down, lo, r64)).astype(F)


def rows(diff, t):
    """(a, b): (B, 1, 1, 1, 1) float32 of the two table rows at t[b]; NaN for an index outside the schedule."""
    t = np.asarray(t, np.int64)
    ok = (t >= 0) & (t < diff.num_timesteps)
    tc = np.where(ok, t, 0)
    cast = lambda row: np.where(ok, np.asarray(row, np.float64)[tc].astype(F), F(np.nan)).astype(F).reshape(-1, 1, 1, 1, 1)      # noqa: E731
    return cast(diff.sqrt_recip_alphas_cumprod), cast(diff.sqrt_recipm1_alphas_cumprod)


def xstart_r(a, b, xt, eps):
    """The unclamped x_0 of the sampler pass: a x_t - b eps with every operation rounded to float32, nothing fused."""
    return (a * np.asarray(xt, F)).astype(F) - (b * np.asarray(eps, F)).astype(F)


def _lat5(lat, shape):
    return np.broadcast_to(np.asarray(lat).reshape(shape[0], shape[1], 1, 1, 1) == 1, shape)


def seed_f32(a, b, xt, eps, cot, lat, clip):
    """(d_eps, d_x, x_0r) as float32 arrays: the bits guide_seed_kernel writes.  An item whose rows are NaN (t outside the schedule) is NaN
    on every frame."""
    xt, eps, cot = (np.asarray(v, F) for v in (xt, eps, cot))
    with np.errstate(invalid="ignore"):
        x0r = xstart_r(a, b, xt, eps)
        keep = (x0r >= F(-1)) & (x0r <= F(1)) if clip else np.ones(xt.shape, bool)
        cr = np.where(keep, cot, F(0)).astype(F)
        de, dx = ((-b) * cr).astype(F), (a * cr).astype(F)
    latent = _lat5(lat, xt.shape)
    bad = np.broadcast_to(np.isnan(a), xt.shape)
    de = np.where(bad, F(np.nan), np.where(latent, de, F(0))).astype(F)
    dx = np.where(bad, F(np.nan), np.where(latent, dx, F(0))).astype(F)
    return de, dx, x0r


def grad_f32(dxd, dx_net, inv_s):
    """g = d_x + dx_net * inv_s, the product and the sum each rounded to float32 (the product is exact for a power of two)."""
    return (np.asarray(dxd, F) + (np.asarray(dx_net, F) * F(inv_s)).astype(F)).astype(F)


def norm_fp64(g, lat):
    """(n, bound): per item sqrt(sum g^2) over the latent frames, exactly rounded to float64 (math.fsum of the exact squares), and the most
    the kernel's float32 value may differ from it: the float64 sum of N non-negative exact terms in any order is off by at most
    (N - 1) 2^-53 relative, the square root halves that and adds 2^-53, the cast to float32 adds 2^-24 -- (2^-24 + (N + 2) 2^-53) n, kept
    with a 2^-20 margin for the bound's own float64 arithmetic."""
    g = np.asarray(g, F).astype(np.float64)
    latent = _lat5(lat, g.shape)
    n, lim = np.zeros(g.shape[0]), np.zeros(g.shape[0])
    for b in range(g.shape[0]):
        v = g[b][latent[b]]
        n[b] = math.sqrt(math.fsum((v * v).tolist()))
        lim[b] = (U + (v.size + 2.0) * 2.0 ** -53) * n[b] * (1.0 + 2.0 ** -20)
    return n, lim


def multiplier_f32(scale, n=None):
    """m_b (B,) float32: scale_b, or with the float32 norms n the one float32 division scale_b / n_b, 0 where n_b == 0."""
    scale = np.asarray(scale, F)
    if n is None:
        return scale
    n = np.asarray(n, F)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(n == 0, F(0), (scale / n).astype(F)).astype(F)


def final_f32(m, g, plain, lat):
    """sample: fmaf(-m_b, g, sample') on the latent frames, the bits of sample' elsewhere."""
    g, plain = np.asarray(g, F), np.asarray(plain, F)
    mb = np.broadcast_to(np.asarray(m, F).reshape(-1, 1, 1, 1, 1), g.shape)
    return np.where(_lat5(lat, g.shape), fma32(-mb, g, plain), plain).astype(F)
