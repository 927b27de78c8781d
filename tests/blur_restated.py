"""Deblurring (csrc/blur.hip: blur_residual_kernel, blur_seed_kernel, blur_apply_kernel) restated: the convolution measurement A of
include/vd_amd.h: vd_deblur_step and its adjoint, and steps 2-4 of that step -- the x_0 head, r = y - A x_0 on the latent frames,
rho_b = ||r||_2 per item and the two cotangents d eps = -b q_r, d_x = a q_r with q = -(A^T r) / rho_b -- in float64 on the float32 values
the engine is handed, with the forward rounding bound of every output; and the same in numpy float32 in the kernel's documented order.
numpy only.

The operator.  w is (k, k), k odd, c = k // 2; a video is (B, T, 3, H, W) and every (H, W) plane is treated alike, zeros outside it:
    (A x)[i, j]   = sum_{a, b} w[a, b] x[i + a - c, j + b - c]            (torch.nn.functional.conv2d: correlation)
    (A^T r)[p, q] = sum_{a, b} w[a, b] r[p - a + c, q - b + c]
The kernel's order, both forms: acc = 0, a ascending, inside it b ascending, acc = fl(acc + fl(w[a, b] v)); a tap outside the plane takes
part with v = 0 (it adds +-0 and changes nothing).

Bound, with u = 2^-24 (step_nll_restated.U), n = k k, gamma_n = n u / (1 - n u), |A| and |A|^T the operators of the kernel |w|.  Every
line names the exact (float64) quantity on the left.
  s      = A z for float32 operands z.  The kernel's s^ is n rounded products and n - 1 rounded additions (the first addition, to 0, is
         exact): |s^ - s| <= gamma_n (|A| |z|) (Higham lemma 3.1 and 8.4; any order).  This alone is the bound of vd_op_blur, and of
         its adjoint with |A|^T.
  h      per element: the head's bound |x_0^ - x_0| (step_nll_restated.xstart_bound, with the step's clamp).
  s      = A x_0 in the residual pass: the kernel sums over its own x_0^, |x_0^| <= |x_0| + h:
             ds = |A| h + gamma_n |A| (|x_0| + h).
  r      = y - s, one rounding:   dr = ds + u (|r| + ds);  0 off the latent frames (the kernel writes and reads nothing there).
  rho    = ||r||_2 over the item's latent elements, as dps_restated:  D = sqrt(sum dr^2),  drho = D + (u + (N + 2) 2^-53) (rho + D).
  g      = A^T r: the kernel sums over its own r^, |r^| <= |r| + dr:     dg = |A|^T dr + gamma_n |A|^T (|r| + dr).
           delta r thus enters the seed through sum |w|.
  q      = -g / rho.  | g^ / rho^ - g / rho | <= e = (dg rho + |g| drho) / (rho (rho - drho)), then the division's one rounding:
             dq = e + u (|q| + e).
  q_r    = q where the clamp passes, 0 elsewhere; assert_unambiguous() keeps every latent |x_0r| further from 1 than the unclamped head's
         bound, so the kernel and this file decide alike.
  d eps  = (-b) q_r, d_x = a q_r, one rounding each:   b dq + u (|d eps| + b dq),   a dq + u (|d_x| + a dq).
Every bound is widened by step_nll_restated's _GROW and by (n + 1) 2^-149 (products and a result below fp32's normal range).  Frames
that are not latent, and items with rho = 0 or without a latent frame: 0, bound 0.  Nothing here is taken from what the kernel returns.
"""
import numpy as np

from step_nll_restated import F, U, _GROW, _rows, _rows32, _xstart32, xstart_bound

__all__ = ["blur_fp64", "blur_f32", "apply_bound", "deblur_fp64", "deblur_bound", "deblur_f32", "assert_unambiguous", "seed_inputs",
           "random_taps", "gaussian_taps", "one_hot_taps", "shifted", "RHO_MIN", "SHAPES"]

RHO_MIN = 1e-3
_TINY = 2.0 ** -149
# (H, W, k) of the operator-level tests and why; the last: three tiles of 32 in either tiled direction of the kernels as built
SHAPES = [(8, 8, 3), (8, 8, 15), (12, 8, 7), (6, 10, 5), (7, 7, 1), (16, 32, 9), (32, 32, 15), (64, 64, 15), (72, 68, 5)]


def _terms(x, w, adjoint):
    """The k k operand planes in the kernel's order: yields (w[a, b], v) with v shaped like x."""
    w = np.asarray(w)
    k = w.shape[0]
    c = k // 2
    H, W = x.shape[-2:]
    xp = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(c, c), (c, c)])
    for a in range(k):
        for b in range(k):
            i0, j0 = (2 * c - a, 2 * c - b) if adjoint else (a, b)             # x[i + a - c] -> xp[i + a];  r[p - a + c] -> xp[p + 2c - a]
            yield w[a, b], xp[..., i0:i0 + H, j0:j0 + W]


def blur_fp64(x, w, adjoint=False):
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    out = np.zeros_like(x)
    for t, v in _terms(x, w, adjoint):
        out += t * v
    return out


def blur_f32(x, w, adjoint=False):
    """The kernel's order in numpy float32: every product and every sum rounded once."""
    x, w = np.asarray(x, F), np.asarray(w, F)
    acc = np.zeros_like(x)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for t, v in _terms(x, w, adjoint):
            acc = (acc + (t * v).astype(F)).astype(F)
    return acc


def _gamma(w):
    n = np.asarray(w).size
    return n * U / (1.0 - n * U), n


def apply_bound(x, w, adjoint=False):
    """(want, bound) of vd_op_blur on float32 x and w."""
    g, n = _gamma(w)
    lim = g * blur_fp64(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)), adjoint)
    return blur_fp64(x, w, adjoint), lim * _GROW + (n + 1) * _TINY


def _flat(v):
    v = np.asarray(v)
    return v.reshape(v.shape[0], -1)


def _sel(lat, shape):
    B, T = shape[:2]
    return np.broadcast_to((np.asarray(lat).reshape(B, T, 1, 1, 1) == 1), shape)


def _head_fp64(tab, xt, eps, t, clip):
    c = _rows(tab, t)
    x0r = (c["sr"] * _flat(xt).astype(np.float64) - c["srm1"] * _flat(eps).astype(np.float64)).reshape(np.shape(xt))
    return x0r, (np.clip(x0r, -1.0, 1.0) if clip else x0r)


def _core(x0, y, lat, w):
    """From an exact x_0: r (0 off the latent frames), rho (B,), g = A^T r, q (0 where rho = 0 and off the latent frames)."""
    B = x0.shape[0]
    sel = _sel(lat, x0.shape)
    r = np.where(sel, np.asarray(y, np.float64) - blur_fp64(x0, w), 0.0)
    rho = np.sqrt((r * r).reshape(B, -1).sum(axis=1))
    g = blur_fp64(r, w, adjoint=True)
    rho5 = rho.reshape(B, 1, 1, 1, 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(sel & (rho5 > 0), -g / rho5, 0.0)
    return r, rho, g, q


def deblur_fp64(tab, xt, eps, t, y, lat, w, clip):
    """Steps 2-4 in float64 -> dict x0, x0r, r, rho, q, mask, deps, dxd."""
    x0r, x0 = _head_fp64(tab, xt, eps, t, clip)
    r, rho, _, q = _core(x0, y, lat, w)
    mask = ((x0r >= -1.0) & (x0r <= 1.0)) if clip else np.ones(x0r.shape, bool)
    qr = np.where(mask, q, 0.0)
    c = _rows(tab, t)
    a, b = (c[k].reshape(-1, 1, 1, 1, 1) for k in ("sr", "srm1"))
    return dict(x0=x0, x0r=x0r, r=r, rho=rho, q=q, mask=mask, deps=-b * qr, dxd=a * qr)


def seed_bound(x0, h, y, lat, w):
    """From an exact x_0 and the per-element bound h of the float32 x_0 the kernel works on: dict of (want, bound) for `rho` (B,), `r` and
    `q` (per element, before the clamp's mask)."""
    x0 = np.asarray(x0, np.float64)
    B = x0.shape[0]
    gam, n = _gamma(w)
    aw = np.abs(np.asarray(w, np.float64))
    sel = _sel(lat, x0.shape)
    r, rho, g, q = _core(x0, y, lat, w)
    ds = blur_fp64(h, aw) + gam * blur_fp64(np.abs(x0) + h, aw) + n * _TINY
    dr = np.where(sel, ds + U * (np.abs(r) + ds), 0.0)
    D = np.sqrt((dr * dr).reshape(B, -1).sum(axis=1))
    N = sel.reshape(B, -1).sum(axis=1).astype(np.float64)
    drho = D + (U + (N + 2.0) * 2.0 ** -53) * (rho + D)
    dg = blur_fp64(dr, aw, adjoint=True) + gam * blur_fp64(np.abs(r) + dr, aw, adjoint=True) + n * _TINY
    rho5, drho5 = (v.reshape(B, 1, 1, 1, 1) for v in (rho, drho))
    ok = (rho5 > 0) & (rho5 > drho5)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.where(ok, (dg * rho5 + np.abs(g) * drho5) / (rho5 * (rho5 - drho5)), np.where(rho5 > 0, np.inf, 0.0))
    e = np.where(sel, e, 0.0)
    dq = e + U * (np.abs(q) + e)
    return dict(rho=(rho, np.where(N > 0, drho * _GROW + _TINY, 0.0)), r=(r, np.where(sel, dr * _GROW + _TINY, 0.0)),
                q=(q, np.where(sel, dq * _GROW + _TINY, 0.0)))


def deblur_bound(tab, xt, eps, t, y, lat, w, clip):
    """dict of (want, bound) for deps, dxd (per element) and rho (B,)."""
    ex = deblur_fp64(tab, xt, eps, t, y, lat, w, clip)
    _, h = xstart_bound(tab, _flat(xt), _flat(eps), t, bool(clip), False)
    sb = seed_bound(ex["x0"], h.reshape(np.shape(xt)), y, lat, w)
    _, dq = sb["q"]
    dq = np.where(ex["mask"], dq, 0.0)
    c = _rows(tab, t)
    out = dict(rho=sb["rho"])
    for k, row in (("deps", "srm1"), ("dxd", "sr")):
        co = np.abs(c[row]).reshape(-1, 1, 1, 1, 1)
        lim = co * dq + U * (np.abs(ex[k]) + co * dq)
        out[k] = (ex[k], np.where(dq > 0, lim * _GROW + _TINY, 0.0))
    return out


def assert_unambiguous(tab, xt, eps, t, y, lat, w, clip):
    """The inputs keep the clamp -- in the head and in the seed's mask -- and the division out of the rounding question: no element of
    any frame has |x_0r| within the unclamped head's bound of 1 (only asked with the clamp on), and rho of every item with a latent frame
    is at least RHO_MIN."""
    ex = deblur_fp64(tab, xt, eps, t, y, lat, w, clip)
    B, T = np.shape(xt)[:2]
    if clip:
        _, hr = xstart_bound(tab, _flat(xt), _flat(eps), t, False, False)
        near = np.abs(np.abs(ex["x0r"]) - 1.0) <= hr.reshape(np.shape(xt))
        assert not near.any(), f"{int(near.sum())} elements have |x_0r| within the head's bound of 1"
    has = (np.asarray(lat).reshape(B, T) == 1).any(axis=1)
    assert (ex["rho"][has] >= RHO_MIN).all(), f"rho {ex['rho']} below {RHO_MIN} on an item with latent frames"


def deblur_f32(tab, xt, eps, t, y, lat, w, clip):
    """The kernels' order in numpy float32 -> dict x0, r, rho, deps, dxd.  x_0 as dps_restated.dps_f32; s = A x_0 by blur_f32, r = y - s;
    rho: the squares and their sum in float64, one root, one rounding; g = A^T r by blur_f32 on the latent frames' r, q = -(g / rho),
    d eps = (-b) q_r, d_x = a q_r, one rounding each."""
    shape = np.shape(xt)
    B = shape[0]
    c32 = _rows32(tab, t)
    with np.errstate(invalid="ignore", over="ignore"):
        x0, _ = _xstart32(c32, _flat(xt).astype(F), _flat(eps).astype(F), False, bool(clip), False, None, nan_bad=False)
        x0r, _ = _xstart32(c32, _flat(xt).astype(F), _flat(eps).astype(F), False, False, False, None, nan_bad=False)
    x0, x0r = x0.reshape(shape), x0r.reshape(shape)
    sel = _sel(lat, shape)
    r = np.where(sel, (np.asarray(y, F) - blur_f32(x0, w)).astype(F), F(0))
    rho = np.sqrt((r.astype(np.float64) ** 2).reshape(B, -1).sum(axis=1)).astype(F)
    g = blur_f32(r, w, adjoint=True)
    rho5 = rho.reshape(B, 1, 1, 1, 1)
    live = sel & (rho5 != 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(live, (-g / rho5).astype(F), F(0))
    mask = ((x0r >= F(-1)) & (x0r <= F(1))) if clip else np.ones(shape, bool)
    qr = np.where(mask, q, F(0))
    a, b = (c32[k].reshape(-1, 1, 1, 1, 1) for k in ("sr", "srm1"))
    return dict(x0=x0, r=r, rho=rho, deps=np.where(live, ((-b) * qr).astype(F), F(0)), dxd=np.where(live, (a * qr).astype(F), F(0)))


def seed_inputs(tab, B, T, H, W, w, clip, seed, t=None, noise_sd=0.1):
    """dps_restated.seed_inputs for a plane of H x W and the blur: (xt, eps, t, y, lat) float32 / int64; frame 1 not latent; eps solved
    so that x_0r lands on chosen targets -- three quarters inside [-0.9, 0.9], with the clamp on a quarter at 1.1 .. 1.6 beyond +-1 --;
    y = A clamp(target) plus noise, so rho is far from 0.  The restatement alone decides that they are unambiguous."""
    g = np.random.default_rng(seed)
    shape = (B, T, 3, H, W)
    NT = tab["NT"]
    t = np.asarray([(7 + 23 * b) % NT for b in range(B)] if t is None else t, np.int64)
    c = _rows(tab, t)
    a, b = (c[k].reshape(-1, 1, 1, 1, 1) for k in ("sr", "srm1"))
    xt = g.standard_normal(shape).astype(F)
    target = g.uniform(-0.9, 0.9, shape)
    if clip:
        out = g.random(shape) < 0.25
        target = np.where(out, np.sign(target) * g.uniform(1.1, 1.6, shape), target)
    eps = ((a * xt.astype(np.float64) - target) / b).astype(F)
    lat = np.ones((B, T), F)
    if T > 1:
        lat[:, 1] = 0
    ycl = blur_fp64(np.clip(target, -1, 1) if clip else target, w)
    y = (ycl + noise_sd * g.standard_normal(ycl.shape)).astype(F)
    return xt, eps, t, y, lat


def random_taps(k, seed):
    """Signed, asymmetric, not normalised: what a motion-blur kernel may be."""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (k, k)).astype(F)


def gaussian_taps(k, sigma=None):
    """gaussian_diffusion.gaussian_kernel's arithmetic: normalised in float64, rounded once."""
    sigma = max(k / 4.0, 0.5) if sigma is None else sigma
    ax = np.arange(k, dtype=np.float64) - k // 2
    g1 = np.exp(-(ax * ax) / (2.0 * sigma ** 2))
    w2 = g1[:, None] * g1[None, :]
    return (w2 / w2.sum()).astype(F)


def one_hot_taps(k, a, b):
    w = np.zeros((k, k), F)
    w[a, b] = 1
    return w


def shifted(x, di, dj):
    """out[..., i, j] = x[..., i + di, j + dj], 0 where that lies outside the plane: A for one_hot_taps(k, c + di, c + dj), and A^T for
    one_hot_taps(k, c - di, c - dj).  Copies bits; no arithmetic."""
    x = np.asarray(x)
    H, W = x.shape[-2:]
    out = np.zeros_like(x)
    i0, i1 = max(0, -di), min(H, H - di)
    j0, j1 = max(0, -dj), min(W, W - dj)
    if i0 < i1 and j0 < j1:
        out[..., i0:i1, j0:j1] = x[..., i0 + di:i1 + di, j0 + dj:j1 + dj]
    return out
