"""Diffusion posterior sampling (csrc/dps.hip: dps_residual_kernel, dps_seed_kernel; DPS, Chung et al. 2023) restated: steps 2-4 of
include/vd_amd.h: vd_dps_step -- the x_0 head, the residual r = y - A x_0 on the latent frames, rho_b = ||r||_2 per item and the two
cotangents d eps = -b q_r, d_x = a q_r with q = -r_cell / (rho_b n_c) -- in float64 on the float32 values the engine is handed, with the
forward rounding bound of every output; and the same in numpy float32 in the kernel's summation order.  numpy only.

Layout as tests/measurement_restated.py: a video is (B, T, 3, H, W), `lat` (B, T), a cell is s x s pixels of one channel plane (gray:
of the three planes of its frame), n = s s (gray: 3 s s) elements, y is (B, T, Cy, H / s, W / s).

Bound, with u = 2^-24 (step_nll_restated.U), gamma_n = n u / (1 - n u).  Every line names the exact (float64) quantity on the left.
  h      per element: the head's bound |x_0^ - x_0| (step_nll_restated.xstart_bound, with the step's clamp; 0 where x_0 is handed in).
  m      the cell mean.  The kernel's m^ = fl(sum^ / n) over its own x_0^: |m^ - mean(x_0^)| <= gamma_n mean_cell|x_0^| (any order of
         summation, Higham lemma 3.1 and 4.2, as measurement_restated) and |mean(x_0^) - m| <= mean_cell(h):
             dm = mean_cell(h) + gamma_n (mean_cell|x_0| + mean_cell(h)).
  r      = y - m, one rounding:   dr = dm + u (|r| + dm).
  rho    = ||r||_2 over the item's latent cells.  | ||r^|| - ||r|| | <= ||r^ - r|| <= D = sqrt(sum dr^2).  The kernel squares in fp64
         (exact: 24 x 24 bits), folds N terms in fp64 (relative N 2^-53 at most, any order), takes the fp64 root (2^-53) and rounds once
         to fp32 (u):            drho = D + (u + (N + 2) 2^-53) (rho + D).
  den    = rho n.  n is a power of two without gray -- fl(rho^ n) is exact --, with gray it is one rounding:
             dden = n drho + [gray] u (den + n drho).
  q      = -r / den.  | r^ / den^ - r / den | <= (dr den + |r| dden) / (den (den - dden)), then one rounding of the division:
             dq = e + u (|q| + e),  e = that quotient.
  q_r    = q where the clamp passes, 0 elsewhere.  The kernel decides on its own x_0r^; assert_unambiguous() keeps every latent |x_0r|
         further from 1 than the unclamped head's bound, so both decide alike and the mask adds no error.
  d eps  = (-b) q_r, d_x = a q_r, one rounding each:   b dq + u (|d eps| + b dq),   a dq + u (|d_x| + a dq).
Every bound is widened by step_nll_restated's _GROW (second-order terms and the float64 arithmetic the bound itself is computed in) and
by 2^-149 (a result below fp32's normal range).  Frames that are not latent, and items with rho = 0 or without a latent frame: 0, bound 0.
Nothing here is taken from what the kernel returns.
"""
import numpy as np

from measurement_restated import _sel, _tree, measure_fp64, replicate
from step_nll_restated import F, U, _GROW, _rows, _rows32, _xstart32, xstart_bound

__all__ = ["dps_fp64", "dps_bound", "dps_f32", "seed_bound", "assert_unambiguous", "seed_inputs", "RHO_MIN"]

RHO_MIN = 1e-3
_TINY = 2.0 ** -149


def _flat(v):
    v = np.asarray(v)
    return v.reshape(v.shape[0], -1)


def _head_fp64(tab, xt, eps, t, clip):
    """x_0r and x_0 in float64, shaped like xt."""
    c = _rows(tab, t)
    x0r = (c["sr"] * _flat(xt).astype(np.float64) - c["srm1"] * _flat(eps).astype(np.float64)).reshape(np.shape(xt))
    return x0r, (np.clip(x0r, -1.0, 1.0) if clip else x0r)


def _item_sum(v, lat):
    """sum over the cells of the latent frames, per item: (B,)"""
    B, T = v.shape[:2]
    w = (np.asarray(lat).reshape(B, T) == 1).astype(np.float64).reshape(B, T, 1, 1, 1)
    return (v * w).reshape(B, -1).sum(axis=1)


def _core(x0, y, lat, s, gray):
    """From an exact x_0 (float64): r per cell (0 off the latent frames), rho (B,), q per element (0 where rho = 0)."""
    B, T = x0.shape[:2]
    latc = (np.asarray(lat).reshape(B, T, 1, 1, 1) == 1)
    r = np.where(latc, np.asarray(y, np.float64) - measure_fp64(x0, s, gray), 0.0)
    rho = np.sqrt(_item_sum(r * r, lat))
    n = s * s * (3 if gray else 1)
    den = (rho * n).reshape(B, 1, 1, 1, 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        qc = np.where(den > 0, -r / den, 0.0)
    return r, rho, replicate(qc, s, gray, x0.shape)


def dps_fp64(tab, xt, eps, t, y, lat, s, gray, clip):
    """Steps 2-4 in float64 -> dict x0, x0r, r, rho, q, mask, deps, dxd (arrays shaped like xt; r like y; rho (B,))."""
    x0r, x0 = _head_fp64(tab, xt, eps, t, clip)
    r, rho, q = _core(x0, y, lat, s, gray)
    mask = ((x0r >= -1.0) & (x0r <= 1.0)) if clip else np.ones(x0r.shape, bool)
    qr = np.where(mask, q, 0.0)
    c = _rows(tab, t)
    a, b = (c[k].reshape(-1, 1, 1, 1, 1) for k in ("sr", "srm1"))
    return dict(x0=x0, x0r=x0r, r=r, rho=rho, q=q, mask=mask, deps=-b * qr, dxd=a * qr)


def seed_bound(x0, h, y, lat, s, gray):
    """From an exact x_0 and the per-element bound h of the float32 x_0 the kernel works on: dict of (want, bound) for `rho` (B,) and `q`
    (per element, before the clamp's mask)."""
    x0 = np.asarray(x0, np.float64)
    B, T = x0.shape[:2]
    n = s * s * (3 if gray else 1)
    gamma = n * U / (1.0 - n * U)
    r, rho, q = _core(x0, y, lat, s, gray)
    latc = (np.asarray(lat).reshape(B, T, 1, 1, 1) == 1)
    mh = measure_fp64(h, s, gray)
    dm = mh + gamma * (measure_fp64(np.abs(x0), s, gray) + mh)
    dr = np.where(latc, dm + U * (np.abs(r) + dm), 0.0)
    D = np.sqrt(_item_sum(dr * dr, lat))
    N = _item_sum(np.ones_like(r), lat)
    drho = D + (U + (N + 2.0) * 2.0 ** -53) * (rho + D)
    den, dden = rho * n, n * drho
    if gray:
        dden = dden + U * (den + dden)
    den5, dden5, ok = (v.reshape(B, 1, 1, 1, 1) for v in (den, dden, (rho > 0) & (den > dden)))
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.where(ok, (dr * den5 + np.abs(r) * dden5) / (den5 * (den5 - dden5)), np.where(den5 > 0, np.inf, 0.0))
        e = np.where(latc, e, 0.0)
    e = replicate(e, s, gray, x0.shape)
    dq = e + U * (np.abs(q) + e)
    return dict(rho=(rho, np.where(N > 0, drho * _GROW + _TINY, 0.0)), q=(q, np.where(_sel(lat, x0.shape), dq * _GROW + _TINY, 0.0)))


def dps_bound(tab, xt, eps, t, y, lat, s, gray, clip):
    """dict of (want, bound) for deps, dxd (per element) and rho (B,)."""
    ex = dps_fp64(tab, xt, eps, t, y, lat, s, gray, clip)
    _, h = xstart_bound(tab, _flat(xt), _flat(eps), t, bool(clip), False)
    sb = seed_bound(ex["x0"], h.reshape(np.shape(xt)), y, lat, s, gray)
    _, dq = sb["q"]
    dq = np.where(ex["mask"], dq, 0.0)
    c = _rows(tab, t)
    out = dict(rho=sb["rho"])
    for k, row in (("deps", "srm1"), ("dxd", "sr")):
        co = np.abs(c[row]).reshape(-1, 1, 1, 1, 1)
        lim = co * dq + U * (np.abs(ex[k]) + co * dq)
        out[k] = (ex[k], np.where(dq > 0, lim * _GROW + _TINY, 0.0))
    return out


def assert_unambiguous(tab, xt, eps, t, y, lat, s, gray, clip):
    """The inputs keep the clamp's mask and the division out of the rounding question: no latent element has |x_0r| within the unclamped
    head's bound of 1 (only asked with the clamp on), and rho of every item with a latent frame is at least RHO_MIN."""
    ex = dps_fp64(tab, xt, eps, t, y, lat, s, gray, clip)
    B, T = np.shape(xt)[:2]
    if clip:
        _, hr = xstart_bound(tab, _flat(xt), _flat(eps), t, False, False)
        near = (np.abs(np.abs(ex["x0r"]) - 1.0) <= hr.reshape(np.shape(xt))) & _sel(lat, np.shape(xt))
        assert not near.any(), f"{int(near.sum())} latent elements have |x_0r| within the head's bound of 1"
    has = (np.asarray(lat).reshape(B, T) == 1).any(axis=1)
    assert (ex["rho"][has] >= RHO_MIN).all(), f"rho {ex['rho']} below {RHO_MIN} on an item with latent frames"


def dps_f32(tab, xt, eps, t, y, lat, s, gray, clip):
    """The kernels' order in numpy float32 -> dict x0, r, rho, deps, dxd.  x_0: two rounded products and one subtraction, then the clamp
    (step_nll_restated._xstart32).  A cell: a lane's row segment of min(s, 4) elements left to right, its channels' segment sums in
    channel order, the butterfly over the cell's lanes (measurement_restated.project_f32); m = sum / n, r = y - m.  rho: the squares
    and their sum in float64 -- the kernel's fold order moves that sum by parts in 2^53, below what the one rounding to float32
    sees but for a tie -- then q = -r / (rho n), d eps = (-b) q_r, d_x = a q_r, one rounding each."""
    shape = np.shape(xt)
    B, T, _, H, W = shape
    c32 = _rows32(tab, t)
    with np.errstate(invalid="ignore", over="ignore"):
        x0, _ = _xstart32(c32, _flat(xt).astype(F), _flat(eps).astype(F), False, bool(clip), False, None, nan_bad=False)
        x0r, _ = _xstart32(c32, _flat(xt).astype(F), _flat(eps).astype(F), False, False, False, None, nan_bad=False)
    x0, x0r = x0.reshape(shape), x0r.reshape(shape)
    seg = min(s, 4)
    hx = s // seg
    v = x0.reshape(B, T, 3, H // s, s, W // s, hx, seg)
    q = v[..., 0]
    for j in range(1, seg):
        q = (q + v[..., j]).astype(F)
    p = ((q[:, :, 0] + q[:, :, 1]).astype(F) + q[:, :, 2]).astype(F)[:, :, None] if gray else q
    p = p.transpose(0, 1, 2, 3, 5, 4, 6).reshape(B, T, p.shape[2], H // s, W // s, s * hx)
    n = F(s * s * (3 if gray else 1))
    m = (_tree(p) / n).astype(F)
    latc = (np.asarray(lat).reshape(B, T, 1, 1, 1) == 1)
    r = np.where(latc, (np.asarray(y, F) - m).astype(F), F(0))
    rho = np.sqrt((r.astype(np.float64) ** 2).reshape(B, -1).sum(axis=1)).astype(F)
    den = (rho * n).astype(F).reshape(B, 1, 1, 1, 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        qc = np.where(den > 0, (-r / den).astype(F), F(0))
    qe = replicate(qc, s, gray, shape).astype(F)
    mask = ((x0r >= F(-1)) & (x0r <= F(1))) if clip else np.ones(shape, bool)
    qr = np.where(mask, qe, F(0))
    a, b = (c32[k].reshape(-1, 1, 1, 1, 1) for k in ("sr", "srm1"))
    live = _sel(lat, shape) & (rho != 0).reshape(B, 1, 1, 1, 1)                  # elsewhere the kernel writes +0 without a product
    return dict(x0=x0, r=r, rho=rho, deps=np.where(live, ((-b) * qr).astype(F), F(0)), dxd=np.where(live, (a * qr).astype(F), F(0)))


def seed_inputs(tab, B, T, H, s, gray, clip, seed, t=None, noise_sd=0.1):
    """(xt, eps, t, y, lat) float32 / int64 for the seed passes: frame 1 not latent; eps solved so that x_0r lands on chosen targets --
    three quarters inside [-0.9, 0.9], with the clamp on a quarter at 1.1 .. 1.6 beyond +-1 --; y = A clamp(target) plus noise, so rho
    is far from 0.  The restatement alone decides that they are unambiguous (assert_unambiguous)."""
    g = np.random.default_rng(seed)
    shape = (B, T, 3, H, H)
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
    ycl = measure_fp64(np.clip(target, -1, 1) if clip else target, s, gray)
    y = (ycl + noise_sd * g.standard_normal(ycl.shape)).astype(F)
    return xt, eps, t, y, lat
