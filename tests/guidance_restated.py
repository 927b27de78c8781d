"""Float64 restatements of the two guidance operators (csrc/guidance.hip; include/vd_amd.h: vd_set_guidance_rescale), numpy only.  They
are the definition the kernels are tested against.

Tensors are (B, T, frame_elems); `lat` is the (B, T) latent mask.  "Item" is one batch element and every statistic runs over the
elements of its frames with lat == 1; the other frames pass through (rescale) or get the static clamp (threshold).

Guidance rescale (Lin et al. 2023, 3.4), on the float32 guided output out_g the combine pass produced and the conditional output out_c:
    sigma_c, sigma_g = population standard deviations (about the mean) over the item's latent elements, in float64
    f = 1 + phi (sigma_c / sigma_g - 1)      float64;  1 where sigma_g == 0 or the item has no latent frame
    out = out_g * float32(f)                 on latent frames (the kernel: one float32 product), out_g elsewhere
Bounds, derived: the kernel rounds f once to float32 (2^-24 relative; its float64 sums differ from the two-pass ones here by parts in
10^13 at most, far below that), and the product once more: |out - out_g f| <= (2^-24 + 2^-24 + 2^-48) |out_g f| < 1.01 2^-23 |out_g f|.

Dynamic thresholding (Saharia et al. 2022, 2.3), on the float32 x_0 prediction:
    n = latent elements, a = sorted |x_0|, h = (n - 1) p, k = floor(h)
    s = a[k] + (h - k) (a[min(k + 1, n - 1)] - a[k])     float64, each operation rounded (no fused multiply-add), then float32(s)
    s = max(s, 1);  NaN when a latent x_0 is not finite;  1 for an item without latent frame
    out = clamp(x_0, -s, s) / s              on latent frames (NaN for a poisoned item), clamp(x_0, -1, 1) elsewhere (a non-finite
                                             value there stays as it is)
`p` is used as given: a caller that compares with the engine passes the float32 value the C ABI carries.
"""
import numpy as np


def _latent(lat, shape):
    lat = np.asarray(lat).reshape(shape[0], shape[1])
    return lat == 1


def rescale_factor_fp64(out_c, out_g, lat, phi):
    """f per item, float64 (not yet rounded to float32)."""
    out_c, out_g = np.asarray(out_c, np.float64), np.asarray(out_g, np.float64)
    m = _latent(lat, out_g.shape)
    f = np.ones(out_g.shape[0], np.float64)
    for b in range(out_g.shape[0]):
        if not m[b].any():
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            sc, sg = out_c[b][m[b]].std(), out_g[b][m[b]].std()
        if sg != 0:
            f[b] = 1.0 + np.float64(phi) * (sc / sg - 1.0)
    return f


def rescale_fp64(out_c, out_g, lat, phi):
    """(out in float64 with the factor rounded to float32 as the kernel rounds it, f in float64)."""
    g = np.asarray(out_g, np.float64)
    m = _latent(lat, g.shape)
    f = rescale_factor_fp64(out_c, out_g, lat, phi)
    out = g.copy()
    for b in range(g.shape[0]):
        out[b][m[b]] = g[b][m[b]] * np.float64(np.float32(f[b]))
    return out, f


def threshold_s_fp64(x0, lat, p):
    """(s before max(., 1) in float64 -- NaN for a poisoned item, 1 for an item without latent frame --, float32 threshold max(s, 1))."""
    x0 = np.asarray(x0, np.float32)
    m = _latent(lat, x0.shape)
    s = np.ones(x0.shape[0], np.float64)
    for b in range(x0.shape[0]):
        if not m[b].any():
            continue
        a = np.abs(x0[b][m[b]].ravel())
        if not np.isfinite(a).all():
            s[b] = np.nan
            continue
        a = np.sort(a).astype(np.float64)
        n = a.size
        h = np.float64(n - 1) * np.float64(p)
        k = int(np.floor(h))
        a0, a1 = a[k], a[min(k + 1, n - 1)]
        s[b] = a0 + (h - np.float64(k)) * (a1 - a0)
    with np.errstate(invalid="ignore"):
        s32 = np.where(np.isnan(s), np.float32(np.nan), np.maximum(s.astype(np.float32), np.float32(1))).astype(np.float32)
    return s, s32


def threshold_fp64(x0, lat, p):
    """(out in float64, float32 thresholds)."""
    x = np.asarray(x0, np.float32).astype(np.float64)
    m = _latent(lat, x.shape)
    _, s32 = threshold_s_fp64(x0, lat, p)
    out = x.copy()
    for b in range(x.shape[0]):
        rest = out[b][~m[b]]
        fin = np.isfinite(rest)
        rest[fin] = np.clip(rest[fin], -1.0, 1.0)
        out[b][~m[b]] = rest
        if m[b].any():
            s = np.float64(s32[b])
            out[b][m[b]] = np.nan if np.isnan(s) else np.clip(x[b][m[b]], -s, s) / s
    return out, s32
