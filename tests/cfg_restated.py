"""Float64 restatement of the cfg_scale combine pass (csrc/misc.hip: cfg_combine_kernel; include/vd_amd.h: vd_set_cfg_scale), numpy only.

    d     = out_c - out_u          formed in float32, as the kernel forms it (one subtraction)
    out_g = out_u + w d            the kernel's one fused multiply-add, here in float64

The bound is derived, not measured: with d given, the kernel's fma rounds its exact result once, an error of at most 2^-24 of that
result, which is at most 2^-24 (|out_u| + |w d|); the bound allows twice that, and 2^-126 (the smallest normal float32) on top
covers a result in the subnormal range flushed to zero.  Where d is not finite the kernel writes NaN and there is nothing to bound.
"""
import numpy as np


def difference_f32(out_c, out_u):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(out_c, np.float32) - np.asarray(out_u, np.float32)


def combine_fp64(out_c, out_u, w):
    """(out_g in float64, d in float32, mask of the elements whose d is finite)."""
    d = difference_f32(out_c, out_u)
    ok = np.isfinite(d)
    with np.errstate(over="ignore", invalid="ignore"):
        g = np.asarray(out_u, np.float64) + np.float64(np.float32(w)) * d.astype(np.float64)
    return g, d, ok


def rounding_bound(out_u, w, d):
    with np.errstate(over="ignore", invalid="ignore"):
        return 2.0 ** -23 * (np.abs(np.asarray(out_u, np.float64)) + np.abs(np.float64(np.float32(w)) * d.astype(np.float64))) + 2.0 ** -126
