"""Zero-shot restoration (csrc/measure.hip: measurement_project_kernel; DDNM, Wang, Yu, Zhang 2022) restated: the cell-mean operator
A, its pseudo-inverse A^+ and the projection x + A^+(y - A x) in float64 on the float32 values the engine is handed, with the forward
rounding bound of every projected element; and the same in numpy float32 in the kernel's summation order.  numpy only.

Layout.  A video is (B, T, 3, H, W), `lat` is (B, T).  A cell is s x s pixels of one channel plane, or with gray of the three planes
of its frame: n = s s (gray: 3 s s) elements.  y = A x is (B, T, Cy, H / s, W / s), Cy = 3 (gray: 1).  A^+ replicates a cell's value
over the cell, so A A^+ = I.  The projection acts on the frames with lat == 1; every other frame keeps its bits.

Bound, with u = 2^-24 (step_nll_restated.U) and gamma_n = n u / (1 - n u).  The kernel computes m = fl(sum / n) -- n - 1 additions in
some order and one division: |m - mean| <= gamma_n mean_cell|x| (Higham, Accuracy and Stability, lemma 3.1 and 4.2: any order of
summation) --, d = fl(y - m): one rounding of |y - m|, and out = fl(x + d): one rounding of |out|.  So
    |out - exact| <= gamma_n mean_cell|x| + u |y - m| + u |out|
with m, out the exact values.  Nothing here is taken from what the kernel gives.  Where x_0 is formed inside the kernel from (x_t, eps),
the bound of that head (step_nll_restated.xstart_bound) is added by the caller.

What follows from it, for the tests.  A(out) - y is the cell mean of out - exact (A(exact) = y), so |A(out) - y| <= the cell mean
of the bound.  A second application to out gives exactly out + A^+(y - A out): it moves an element by at most that cell mean, plus its
own bound on the input `out`.
"""
import numpy as np

from step_nll_restated import F, U

__all__ = ["OPERATORS", "served", "cells", "uncells", "measure_fp64", "replicate", "project_fp64", "project_bound", "project_f32",
           "cell_mean_of", "second_application_bound"]

# (scale, gray) of every operator the engine serves
OPERATORS = [(2, False), (4, False), (8, False), (1, True), (2, True), (4, True), (8, True)]


def served(scale, gray):
    return (scale, bool(gray)) in OPERATORS


def cells(x, s, gray):
    """(B, T, 3, H, W) -> (B, T, Cy, H/s, W/s, n): the elements of every cell, channel-major, then row, then column."""
    B, T, C, H, W = x.shape
    assert C == 3 and H % s == 0 and W % s == 0
    v = x.reshape(B, T, 3, H // s, s, W // s, s).transpose(0, 1, 2, 3, 5, 4, 6).reshape(B, T, 3, H // s, W // s, s * s)
    if gray:
        v = v.transpose(0, 1, 3, 4, 2, 5).reshape(B, T, 1, H // s, W // s, 3 * s * s)
    return v


def uncells(v, s, gray, shape):
    """The inverse of cells()."""
    B, T, _, H, W = shape
    if gray:
        v = v.reshape(B, T, H // s, W // s, 3, s * s).transpose(0, 1, 4, 2, 3, 5)
    return v.reshape(B, T, 3, H // s, W // s, s, s).transpose(0, 1, 2, 3, 5, 4, 6).reshape(B, T, 3, H, W)


def measure_fp64(x, s, gray):
    """A x in float64."""
    return cells(np.asarray(x, np.float64), s, gray).mean(axis=-1)


def replicate(y, s, gray, shape):
    """A^+ y: every cell's value over its cell."""
    n = s * s * (3 if gray else 1)
    return uncells(np.repeat(np.asarray(y)[..., None], n, axis=-1), s, gray, shape)


def cell_mean_of(v, s, gray):
    """Per element, the mean of v over the element's cell (float64)."""
    return replicate(measure_fp64(v, s, gray), s, gray, v.shape)


def _sel(lat, shape):
    B, T = shape[:2]
    return np.broadcast_to((np.asarray(lat).reshape(B, T, 1, 1, 1) == 1), shape)


def project_fp64(x, y, lat, s, gray):
    x64 = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        out = x64 + replicate(np.asarray(y, np.float64) - measure_fp64(x64, s, gray), s, gray, x.shape)
    return np.where(_sel(lat, x.shape), out, x64)


def project_bound(x, y, lat, s, gray):
    """(want, bound) per element; bound 0 (bit equality) on the frames that are not latent."""
    n = s * s * (3 if gray else 1)
    gamma = n * U / (1.0 - n * U)
    x64 = np.asarray(x, np.float64)
    want = project_fp64(x, y, lat, s, gray)
    with np.errstate(invalid="ignore", over="ignore"):
        mean_abs = cell_mean_of(np.abs(x64), s, gray)
        d = replicate(np.abs(np.asarray(y, np.float64) - measure_fp64(x64, s, gray)), s, gray, x.shape)
        bound = gamma * mean_abs + U * d + U * np.abs(want)
    return want, np.where(_sel(lat, x.shape), bound, 0.0)


def second_application_bound(out, y, lat, s, gray, first_bound):
    """(want, bound) of the projection applied to `out`, itself a projection onto y computed inside first_bound: the exact second
    application moves an element by y_cell - mean_cell(out), at most the cell mean of first_bound; `want` is `out` itself."""
    _, again = project_bound(out, y, lat, s, gray)
    return np.asarray(out, np.float64), np.where(_sel(lat, out.shape), again + cell_mean_of(first_bound, s, gray), 0.0)


def _tree(p):
    """Pairwise float32 tree over the last axis (a power of two long): the xor butterfly at lane distance 1, 2, 4, ..."""
    while p.shape[-1] > 1:
        p = (p[..., 0::2] + p[..., 1::2]).astype(F)
    return p[..., 0]


def project_f32(x, y, lat, s, gray):
    """The kernel's order in numpy float32.  A lane owns a row segment of min(s, 4) elements per channel: it adds the segment left to
    right, then its channels' segment sums in channel order; the lanes of a cell -- row-major, s = 8: two segments per row -- are
    reduced by the butterfly.  m = sum / n, d = y - m, out = x + d."""
    x = np.asarray(x, F)
    B, T, _, H, W = x.shape
    seg = min(s, 4)
    hx = s // seg
    # (B, T, 3, H/s, row, W/s, half, seg)
    v = x.reshape(B, T, 3, H // s, s, W // s, hx, seg)
    q = v[..., 0]
    for j in range(1, seg):
        q = (q + v[..., j]).astype(F)
    if gray:
        p = ((q[:, :, 0] + q[:, :, 1]).astype(F) + q[:, :, 2]).astype(F)[:, :, None]
    else:
        p = q
    # lanes of a cell: (row, half) row-major -> last axis
    p = p.transpose(0, 1, 2, 3, 5, 4, 6).reshape(B, T, p.shape[2], H // s, W // s, s * hx)
    n = F(s * s * (3 if gray else 1))
    with np.errstate(invalid="ignore", over="ignore"):
        m = (_tree(p) / n).astype(F)
        d = (np.asarray(y, F) - m).astype(F)
        out = (x + replicate(d, s, gray, x.shape).astype(F)).astype(F)
    return np.where(_sel(lat, x.shape), out, x)
