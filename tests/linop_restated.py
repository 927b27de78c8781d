"""Separable linear measurements (csrc/linop.hip: linop_apply_kernel, linop_residual_kernel, linop_project_kernel, linop_seed_kernel)
restated: the two-sided product Z = L X R^T of include/vd_amd.h, the residual r = y - A_h x_0 A_w^T on the latent frames, rho_b = ||r||_2
per item, the projection x_0' = x_0 + P_h r P_w^T and the two cotangents d eps = -b q_r, d_x = a q_r with q = -(A_h^T r A_w) / rho_b -- in
float64 on the float32 values the engine is handed, with the forward rounding bound of every output; and the same in numpy float32 in the
kernel's documented order.  numpy only.

The product.  L is (P, Q), X (..., Q, U), R (S, U); the right factor goes first:
    tmp[q, s] = sum_u X[q, u] R[s, u]        acc = 0, u ascending, acc = fl(acc + fl(X[q, u] R[s, u]))
    Z[p, s]   = sum_q L[p, q] tmp[q, s]      acc = 0, q ascending, acc = fl(acc + fl(L[p, q] tmp[q, s]))
tmp is a float32 value between the two sums.  Forward: L = A_h, R = A_w; adjoint: L = A_h^T, R = A_w^T; back-projection: L = P_h, R = P_w.

Bound, with u = 2^-24 (step_nll_restated.U), gamma_n = n u / (1 - n u), |M| the matrix of absolute values.  Every line names the exact
(float64) quantity on the left.
  tmp    = X R^T for float32 operands: U rounded products and U - 1 rounded additions, |tmp^ - tmp| <= gamma_U |X| |R|^T (Higham lemma
         3.1 and 8.4; any order), so |tmp^| <= (1 + gamma_U) |X| |R|^T.
  Z      = L tmp.  The kernel sums over its own tmp^: |Z^ - L tmp^| <= gamma_Q |L| |tmp^| and |L tmp^ - L tmp| <= gamma_U |L| |X| |R|^T:
             dZ = G |L| |X| |R|^T,   G = gamma_U + gamma_Q (1 + gamma_U).
         This alone is the bound of vd_op_linop in all three uses.  An operand that carries an error itself, |X^ - X| <= h per element:
             dZ = |L| h |R|^T + G |L| (|X| + h) |R|^T.                                                              (two_bound)
  h      per element: the head's bound |x_0^ - x_0| (step_nll_restated.xstart_bound, with the step's clamp); 0 for an x_0 handed in.
  s      = A_h x_0 A_w^T in the residual pass:  ds = two_bound(A_h, x_0, A_w, h).
  r      = y - s, one rounding:   dr = ds + u (|r| + ds);  0 off the latent frames (the kernel writes and reads nothing there).
  rho    = ||r||_2 over the item's latent elements, as blur_restated:  D = sqrt(sum dr^2),  drho = D + (u + (N + 2) 2^-53) (rho + D).
  x_0'   = x_0 + P_h r P_w^T, one rounding:   dz = two_bound(P_h, r, P_w, dr),  dx' = h + dz + u (|x_0'| + h + dz); off the latent
         frames x_0' = x_0 with bound h.
  A x_0' = y + (K_h r K_w^T - r) with K = A P of either axis, in exact arithmetic.  For the float32 x_0'^ the kernel returns, A applied to
         it in float64:   |A x_0'^ - y| <= |A_h| dx' |A_w|^T + |K_h - I| |r| |K_w|^T + |r| |K_w - I|^T,
         K formed in float64 from the actual float32 matrices: what a truncated or rounded pseudo-inverse leaves is part of the bound,
         not of the tolerance.                                                                                       (identity_bound)
  g      = A_h^T r A_w: the kernel works on its own r^:   dg = two_bound(A_h^T, r, A_w^T, dr).
  q      = -g / rho.  | g^ / rho^ - g / rho | <= e = (dg rho + |g| drho) / (rho (rho - drho)), then the division's one rounding:
             dq = e + u (|q| + e).
  q_r    = q where the clamp passes, 0 elsewhere; assert_unambiguous() keeps every latent |x_0r| further from 1 than the unclamped head's
         bound, so the kernel and this file decide alike.
  d eps  = (-b) q_r, d_x = a q_r, one rounding each:   b dq + u (|d eps| + b dq),   a dq + u (|d_x| + a dq).
Every bound is widened by step_nll_restated's _GROW and by the subnormal term (Q (U max|L| + 1) + 1) 2^-149 (products and results below
fp32's normal range).  Frames that are not latent, and items with rho = 0 or without a latent frame: 0, bound 0.  Nothing here is taken
from what the kernel returns.
"""
import numpy as np

from step_nll_restated import F, U, _GROW, _rows, _rows32, _xstart32, xstart_bound

__all__ = ["two_fp64", "two_f32", "two_bound", "apply_bound", "forward", "adjoint", "linop_fp64", "linop_bound", "linop_f32", "project_fp64",
           "project_bound", "project_f32", "identity_bound", "assert_unambiguous", "seed_inputs", "random_operator", "RHO_MIN", "SHAPES"]

RHO_MIN = 1e-3
_TINY = 2.0 ** -149
# (H, W, Mh, Mw) of the operator-level tests: the smallest sides, a single output row, odd and non-square sides, sides not divisible by
# 4 (the scalar load form), more than one chunk of 32 output columns, and the largest LDS footprint and the longest sums
SHAPES = [(8, 8, 2, 2), (8, 8, 8, 8), (7, 7, 1, 1), (12, 8, 5, 3), (6, 10, 6, 4), (32, 32, 8, 8), (64, 64, 16, 16), (72, 68, 9, 17),
          (128, 128, 32, 32), (128, 128, 128, 128)]


def two_fp64(L, X, R):
    """Z = L X R^T in float64 on every trailing (Q, U) plane of X."""
    L, X, R = (np.asarray(v, np.float64) for v in (L, X, R))
    return L @ (X @ R.T)


def two_f32(L, X, R):
    """The kernel's order in numpy float32: every product and every sum rounded once, tmp a float32 value."""
    L, X, R = (np.asarray(v, F) for v in (L, X, R))
    Q, Un = X.shape[-2:]
    tmp = np.zeros(X.shape[:-1] + (R.shape[0],), F)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for u in range(Un):
            tmp = (tmp + (X[..., :, u, None] * R[None, :, u]).astype(F)).astype(F)
        Z = np.zeros(X.shape[:-2] + (L.shape[0], R.shape[0]), F)
        for q in range(Q):
            Z = (Z + (L[:, q, None] * tmp[..., q, None, :]).astype(F)).astype(F)
    return Z


def _gam(n):
    return n * U / (1.0 - n * U)


def two_bound(L, X, R, h=None):
    """(want, bound) of the kernel's Z for float32 L and R and an operand X known to |X^ - X| <= h per element (None: exact)."""
    L, X, R = (np.asarray(v, np.float64) for v in (L, X, R))
    Q, Un = X.shape[-2:]
    G = _gam(Un) + _gam(Q) * (1.0 + _gam(Un))
    aL, aR = np.abs(L), np.abs(R)
    hh = np.zeros_like(X) if h is None else np.asarray(h, np.float64)
    lim = two_fp64(aL, hh, aR) + G * two_fp64(aL, np.abs(X) + hh, aR)
    return two_fp64(L, X, R), lim * _GROW + (Q * (Un * max(float(aL.max()), 1.0) + 1.0) + 1.0) * _TINY


apply_bound = two_bound


def forward(A_h, A_w):
    return np.asarray(A_h), np.asarray(A_w)


def adjoint(A_h, A_w):
    return np.ascontiguousarray(np.asarray(A_h).T), np.ascontiguousarray(np.asarray(A_w).T)


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


def _core(x0, y, lat, A_h, A_w):
    """From an exact x_0: r (0 off the latent frames), rho (B,), g = A_h^T r A_w, q (0 where rho = 0 and off the latent frames)."""
    B = x0.shape[0]
    y = np.asarray(y, np.float64)
    sel_y, sel_x = _sel(lat, y.shape), _sel(lat, x0.shape)
    r = np.where(sel_y, y - two_fp64(A_h, x0, A_w), 0.0)
    rho = np.sqrt((r * r).reshape(B, -1).sum(axis=1))
    At = adjoint(A_h, A_w)
    g = two_fp64(At[0], r, At[1])
    rho5 = rho.reshape(B, 1, 1, 1, 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(sel_x & (rho5 > 0), -g / rho5, 0.0)
    return r, rho, g, q


def linop_fp64(tab, xt, eps, t, y, lat, A_h, A_w, clip):
    """The residual and seed passes in float64 -> dict x0, x0r, r, rho, q, mask, deps, dxd."""
    x0r, x0 = _head_fp64(tab, xt, eps, t, clip)
    r, rho, _, q = _core(x0, y, lat, A_h, A_w)
    mask = ((x0r >= -1.0) & (x0r <= 1.0)) if clip else np.ones(x0r.shape, bool)
    qr = np.where(mask, q, 0.0)
    c = _rows(tab, t)
    a, b = (c[k].reshape(-1, 1, 1, 1, 1) for k in ("sr", "srm1"))
    return dict(x0=x0, x0r=x0r, r=r, rho=rho, q=q, mask=mask, deps=-b * qr, dxd=a * qr)


def residual_bound(x0, h, y, lat, A_h, A_w):
    """From an exact x_0 and the per-element bound h of the float32 x_0 the kernel works on: (r, dr, rho, drho, N), dr and drho not yet
    widened; dr is 0 off the latent frames."""
    x0 = np.asarray(x0, np.float64)
    B = x0.shape[0]
    r, rho, _, _ = _core(x0, y, lat, A_h, A_w)
    sel = _sel(lat, r.shape)
    _, ds = two_bound(A_h, x0, A_w, h)
    dr = np.where(sel, ds + U * (np.abs(r) + ds), 0.0)
    D = np.sqrt((dr * dr).reshape(B, -1).sum(axis=1))
    N = sel.reshape(B, -1).sum(axis=1).astype(np.float64)
    drho = D + (U + (N + 2.0) * 2.0 ** -53) * (rho + D)
    return r, dr, rho, drho, N


def seed_bound(x0, h, y, lat, A_h, A_w):
    """dict of (want, bound) for `rho` (B,), `r` and `q` (per element, before the clamp's mask)."""
    x0 = np.asarray(x0, np.float64)
    B = x0.shape[0]
    r, dr, rho, drho, N = residual_bound(x0, h, y, lat, A_h, A_w)
    _, _, g, q = _core(x0, y, lat, A_h, A_w)
    sel_y, sel_x = _sel(lat, r.shape), _sel(lat, x0.shape)
    At = adjoint(A_h, A_w)
    _, dg = two_bound(At[0], r, At[1], dr)
    rho5, drho5 = (v.reshape(B, 1, 1, 1, 1) for v in (rho, drho))
    ok = (rho5 > 0) & (rho5 > drho5)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.where(ok, (dg * rho5 + np.abs(g) * drho5) / (rho5 * (rho5 - drho5)), np.where(rho5 > 0, np.inf, 0.0))
    e = np.where(sel_x, e, 0.0)
    dq = e + U * (np.abs(q) + e)
    return dict(rho=(rho, np.where(N > 0, drho * _GROW + _TINY, 0.0)), r=(r, np.where(sel_y, dr * _GROW + _TINY, 0.0)),
                q=(q, np.where(sel_x, dq * _GROW + _TINY, 0.0)))


def linop_bound(tab, xt, eps, t, y, lat, A_h, A_w, clip):
    """dict of (want, bound) for deps, dxd (per element), r (per element of y) and rho (B,)."""
    ex = linop_fp64(tab, xt, eps, t, y, lat, A_h, A_w, clip)
    _, h = xstart_bound(tab, _flat(xt), _flat(eps), t, bool(clip), False)
    sb = seed_bound(ex["x0"], h.reshape(np.shape(xt)), y, lat, A_h, A_w)
    _, dq = sb["q"]
    dq = np.where(ex["mask"], dq, 0.0)
    c = _rows(tab, t)
    out = dict(rho=sb["rho"], r=sb["r"])
    for k, row in (("deps", "srm1"), ("dxd", "sr")):
        co = np.abs(c[row]).reshape(-1, 1, 1, 1, 1)
        lim = co * dq + U * (np.abs(ex[k]) + co * dq)
        out[k] = (ex[k], np.where(dq > 0, lim * _GROW + _TINY, 0.0))
    return out


def assert_unambiguous(tab, xt, eps, t, y, lat, A_h, A_w, clip):
    """The inputs keep the clamp -- in the head and in the seed's mask -- and the division out of the rounding question: no element of
    any frame has |x_0r| within the unclamped head's bound of 1 (only asked with the clamp on), and rho of every item with a latent frame
    is at least RHO_MIN."""
    ex = linop_fp64(tab, xt, eps, t, y, lat, A_h, A_w, clip)
    B, T = np.shape(xt)[:2]
    if clip:
        _, hr = xstart_bound(tab, _flat(xt), _flat(eps), t, False, False)
        near = np.abs(np.abs(ex["x0r"]) - 1.0) <= hr.reshape(np.shape(xt))
        assert not near.any(), f"{int(near.sum())} elements have |x_0r| within the head's bound of 1"
    has = (np.asarray(lat).reshape(B, T) == 1).any(axis=1)
    assert (ex["rho"][has] >= RHO_MIN).all(), f"rho {ex['rho']} below {RHO_MIN} on an item with latent frames"


def linop_f32(tab, xt, eps, t, y, lat, A_h, A_w, clip):
    """The kernels' order in numpy float32 -> dict x0, r, rho, deps, dxd.  x_0 as blur_restated.deblur_f32; s by two_f32, r = y - s;
    rho: the squares and their sum in float64, one root, one rounding; g = A_h^T r A_w by two_f32 on the latent frames' r,
    q = -(g / rho), d eps = (-b) q_r, d_x = a q_r, one rounding each."""
    shape = np.shape(xt)
    B = shape[0]
    c32 = _rows32(tab, t)
    with np.errstate(invalid="ignore", over="ignore"):
        x0, _ = _xstart32(c32, _flat(xt).astype(F), _flat(eps).astype(F), False, bool(clip), False, None, nan_bad=False)
        x0r, _ = _xstart32(c32, _flat(xt).astype(F), _flat(eps).astype(F), False, False, False, None, nan_bad=False)
    x0, x0r = x0.reshape(shape), x0r.reshape(shape)
    y = np.asarray(y, F)
    sel_y, sel = _sel(lat, y.shape), _sel(lat, shape)
    r = np.where(sel_y, (y - two_f32(A_h, x0, A_w)).astype(F), F(0))
    rho = np.sqrt((r.astype(np.float64) ** 2).reshape(B, -1).sum(axis=1)).astype(F)
    At = adjoint(A_h, A_w)
    g = two_f32(At[0], r, At[1])
    rho5 = rho.reshape(B, 1, 1, 1, 1)
    live = sel & (rho5 != 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(live, (-g / rho5).astype(F), F(0))
    mask = ((x0r >= F(-1)) & (x0r <= F(1))) if clip else np.ones(shape, bool)
    qr = np.where(mask, q, F(0))
    a, b = (c32[k].reshape(-1, 1, 1, 1, 1) for k in ("sr", "srm1"))
    return dict(x0=x0, r=r, rho=rho, deps=np.where(live, ((-b) * qr).astype(F), F(0)), dxd=np.where(live, (a * qr).astype(F), F(0)))


# ------------------------------------------------------------------------------------------------------------ the projection
def project_fp64(x0, y, lat, A_h, A_w, P_h, P_w, clip=False):
    """x_0' in float64 from a float32 x_0 handed in (through the clamp when clip): x_0 + P_h (y - A x_0) P_w^T on the latent frames."""
    x0 = np.asarray(x0, np.float64)
    x0 = np.clip(x0, -1.0, 1.0) if clip else x0
    y = np.asarray(y, np.float64)
    r = np.where(_sel(lat, y.shape), y - two_fp64(A_h, x0, A_w), 0.0)
    return np.where(_sel(lat, x0.shape), x0 + two_fp64(P_h, r, P_w), x0)


def project_bound(x0, y, lat, A_h, A_w, P_h, P_w, clip=False, h=None):
    """(want, bound) per element of the projected x_0, for an x_0 (float64: the exact one) the kernel knows to h per element (None: it
    is handed the float32 values themselves; the clamp is then exact)."""
    x0 = np.asarray(x0, np.float64)
    x0 = np.clip(x0, -1.0, 1.0) if clip else x0
    hh = np.zeros_like(x0) if h is None else np.asarray(h, np.float64)
    want = project_fp64(x0, y, lat, A_h, A_w, P_h, P_w)
    r, dr, _, _, _ = residual_bound(x0, hh, y, lat, A_h, A_w)
    _, dz = two_bound(P_h, r, P_w, dr)
    sel = _sel(lat, x0.shape)
    lim = np.where(sel, hh + dz + U * (np.abs(want) + hh + dz), hh)
    return want, np.where(lim > 0, lim * _GROW + _TINY, 0.0)


def project_f32(x0, y, lat, A_h, A_w, P_h, P_w, clip=False):
    """The two kernels' order in numpy float32 on a float32 x_0."""
    x0 = np.asarray(x0, F)
    x0 = np.clip(x0, F(-1), F(1)) if clip else x0
    y = np.asarray(y, F)
    r = np.where(_sel(lat, y.shape), (y - two_f32(A_h, x0, A_w)).astype(F), F(0))
    return np.where(_sel(lat, x0.shape), (x0 + two_f32(P_h, r, P_w)).astype(F), x0)


def identity_bound(x0, y, lat, A_h, A_w, P_h, P_w, clip=False, h=None):
    """Per element of y on the latent frames: the bound of |A x_0'^ - y| for the kernel's float32 x_0'^, A applied to it in float64 --
    the projection's own rounding carried through |A|, plus what A P - I leaves of r (K formed in float64 from the float32 matrices)."""
    x0 = np.asarray(x0, np.float64)
    x0c = np.clip(x0, -1.0, 1.0) if clip else x0
    _, dx = project_bound(x0, y, lat, A_h, A_w, P_h, P_w, clip, h)
    y = np.asarray(y, np.float64)
    r = np.where(_sel(lat, y.shape), y - two_fp64(A_h, x0c, A_w), 0.0)
    Ah, Aw, Ph, Pw = (np.asarray(v, np.float64) for v in (A_h, A_w, P_h, P_w))
    Kh, Kw = Ah @ Ph, Aw @ Pw
    Eh, Ew = np.abs(Kh - np.eye(Kh.shape[0])), np.abs(Kw - np.eye(Kw.shape[0]))
    left = two_fp64(Eh, np.abs(r), np.abs(Kw)) + np.abs(r) @ Ew.T
    lim = two_fp64(np.abs(Ah), dx, np.abs(Aw)) + left
    return np.where(_sel(lat, y.shape), lim * _GROW + _TINY, 0.0)


# ------------------------------------------------------------------------------------------------------------ inputs
def random_operator(H, W, Mh, Mw, seed):
    """Signed, dense, not normalised float32 matrices (Mh, H) and (Mw, W) with entries of order 1 / sqrt(n): what a blur with a signed
    kernel or a random projection may be."""
    g = np.random.default_rng(seed)
    return (g.uniform(-1.0, 1.0, (Mh, H)) / np.sqrt(H)).astype(F), (g.uniform(-1.0, 1.0, (Mw, W)) / np.sqrt(W)).astype(F)


def seed_inputs(tab, B, T, H, W, A_h, A_w, clip, seed, t=None, noise_sd=0.1):
    """blur_restated.seed_inputs for this operator: (xt, eps, t, y, lat) float32 / int64; frame 1 not latent; eps solved so that x_0r
    lands on chosen targets -- three quarters inside [-0.9, 0.9], with the clamp on a quarter at 1.1 .. 1.6 beyond +-1 --;
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
    ycl = two_fp64(A_h, np.clip(target, -1, 1) if clip else target, A_w)
    y = (ycl + noise_sd * g.standard_normal(ycl.shape)).astype(F)
    return xt, eps, t, y, lat
