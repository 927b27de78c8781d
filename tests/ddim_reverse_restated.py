"""ddim_reverse_sample's arithmetic behind pred_xstart (gaussian_diffusion.py:658-666 of the reference), restated in float64 on the
float32 values the step reads, with the rounding bound the GPU test holds the kernel to.  numpy only.

    e      = (a x - x0) / b            a = float32(sqrt_recip_alphas_cumprod[t]), b = float32(sqrt_recipm1_alphas_cumprod[t])
    abn    = float32(alphas_cumprod_next[t]),  alphas_cumprod_next = append(alphas_cumprod[1:], 0.0)
    sample = x0 sqrt(abn) + sqrt(1 - abn) e
"""
import numpy as np


def tables(diff, t):
    """(a, b, abn) at index t: float64 numbers holding the float32 casts the reference's _extract_into_tensor yields."""
    f = lambda row: float(np.float32(row[t]))  # noqa: E731
    return f(diff.sqrt_recip_alphas_cumprod), f(diff.sqrt_recipm1_alphas_cumprod), f(diff.alphas_cumprod_next)


def sample_fp64(x, x0, a, b, abn):
    """The three lines in float64 -> (sample, e).  x, x0: float32 arrays, x_t and the step's own float32 pred_xstart."""
    x, x0 = np.asarray(x, np.float64), np.asarray(x0, np.float64)
    e = (a * x - x0) / b
    return x0 * np.sqrt(abn) + np.sqrt(1.0 - abn) * e, e


def rounding_bound(x, x0, a, b, abn):
    """Per element, the most a float32 evaluation may differ from sample_fp64: at most eight roundings of 2^-24 on every term
    (a x, the subtraction, the quotient, sqrt(abn), 1 - abn, its root, the two products and the sum; division and square root
    are correctly rounded), i.e. 2^-21 times the magnitudes that carry them:
        (|a x| + |x0|) / b * s     the numerator's roundings, carried through the quotient into the sample
        |x0| r                     the first product
        s |e|                      the quotient's own rounding, the second product, the sum
    with r = sqrt(abn), s = sqrt(1 - abn)."""
    _, e = sample_fp64(x, x0, a, b, abn)
    ax, ax0 = np.abs(a * np.asarray(x, np.float64)), np.abs(np.asarray(x0, np.float64))
    r, s = np.sqrt(abn), np.sqrt(1.0 - abn)
    return 2.0 ** -21 * ((ax + ax0) / b * s + ax0 * r + s * np.abs(e))
