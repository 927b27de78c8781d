"""Pixel-mask inpainting (csrc/known.hip: known_merge_kernel, q_jump_kernel; respace.repaint_schedule) restated: the merge and the jump
in float64 on the float32 values the engine is handed, with the forward rounding bound of every merged element from the interval
helpers of tests/step_nll_restated.py; the same in numpy float32 in the kernels' operation order; and the schedule from the RePaint
paper's loop (Lugmayr et al. 2022, algorithm 1 with jump length j and r resamplings).  numpy only.

Layout.  Tensors are (B, T, 3, hw); the mask is (B, T, hw), broadcast over the three channels; `lat` is (B, T).  An element is merged
iff lat == 1 and mask != 0.  The merge at index t is q_sample(known_src, t - 1, z) for t >= 1 and known_src itself for t == 0; an item
whose t lies outside the schedule is NaN throughout.  Philox: element i (flat over the whole tensor) of the merge's noise is element i
of the stream at offset + (B per) // 4, per = T 3 hw; of the jump's, element i at offset.
"""
import numpy as np

from step_nll_restated import Ex, F, Iv, _hull, normal_f32, q_sample_bound, q_sample_fp64

__all__ = ["merged", "known_merge_fp64", "known_merge_f32", "known_merge_bound", "merge_noise_f32", "jump_rows", "q_jump_fp64",
           "q_jump_f32", "q_jump_bound", "jump_noise_f32", "repaint_schedule_ref", "repaint_steps"]


def merged(mask, lat):
    """(B, T, 3, hw) bool: the elements the merge overwrites."""
    B, T, hw = mask.shape
    m = (np.asarray(mask) != 0) & (np.asarray(lat).reshape(B, T, 1) == 1)
    return np.broadcast_to(m[:, :, None, :], (B, T, 3, hw)).copy()


def _t_ok(tab, t):
    t = np.asarray(t, np.int64)
    return (t >= 0) & (t < tab["NT"])


def _merge(fn, tab, g, k, mask, lat, t, z, dtype):
    """fn(tab, k2, t - 1, z2) on (B, per) arrays is the q_sample of the restatement in use."""
    B = g.shape[0]
    t = np.asarray(t, np.int64)
    ok = _t_ok(tab, t)
    tq = np.where(ok & (t >= 1), t - 1, 0)                                   # a valid index; the result is used where t >= 1 only
    with np.errstate(invalid="ignore"):
        q = np.asarray(fn(tab, k.reshape(B, -1), tq, z.reshape(B, -1))).reshape(g.shape)
    sel = (t >= 1).reshape(B, 1, 1, 1)
    out = np.where(merged(mask, lat), np.where(sel, q, k.astype(dtype)), g.astype(dtype))
    return np.where(ok.reshape(B, 1, 1, 1), out, np.nan).astype(dtype)


def known_merge_fp64(tab, g, k, mask, lat, t, z):
    return _merge(q_sample_fp64, tab, g, k, mask, lat, t, z, np.float64)


def known_merge_f32(tab, g, k, mask, lat, t, z):
    """The kernel's order: fmaf(s1[t-1], z, sa[t-1] * k) -- the product sa k rounded, the other one exact inside the sum."""
    def q(tab_, k2, tq, z2):
        sa, s1 = tab_["sa"][tq][:, None], tab_["s1"][tq][:, None]
        p = (sa * k2.astype(F)).astype(F)
        return (s1.astype(np.float64) * z2.astype(np.float64) + p.astype(np.float64)).astype(F)
    return _merge(q, tab, g, k, mask, lat, t, z, F)


def known_merge_bound(tab, g, k, mask, lat, t, z):
    """(want, bound) per element: q_sample_bound at t - 1 on the merged elements of items with t >= 1, 0 (bit equality) elsewhere."""
    B = g.shape[0]
    t = np.asarray(t, np.int64)
    want = known_merge_fp64(tab, g, k, mask, lat, t, z)
    tq = np.where(_t_ok(tab, t) & (t >= 1), t - 1, 0)
    _, lim = q_sample_bound(tab, k.reshape(B, -1), tq, z.reshape(B, -1))
    lim = np.where(merged(mask, lat) & (t >= 1).reshape(B, 1, 1, 1), lim.reshape(g.shape), 0.0)
    return want, lim


def merge_noise_f32(seed, offset, shape):
    """The merge's in-kernel draws for a (B, T, 3, hw) tensor: normal_f32 at offset + (B per) // 4."""
    n = int(np.prod(shape))
    return normal_f32(seed, offset + n // 4, np.arange(n)).reshape(shape)


# ------------------------------------------------------------------------------------------------------------ the jump
def jump_rows(betas):
    """(sqrt_alpha, sqrt_beta) float32: casts of the float64 sqrt(1 - betas), sqrt(betas)."""
    b = np.asarray(betas, np.float64)
    return np.sqrt(1.0 - b).astype(F), np.sqrt(b).astype(F)


def _jump(A, rows, x, lat, t, z):
    B, T = x.shape[:2]
    t = np.asarray(t, np.int64)
    ok = (t >= 0) & (t < len(rows[0]))
    tc = np.where(ok, t, 0)
    sa = rows[0][tc].astype(np.float64).reshape(B, 1, 1, 1)
    sb = rows[1][tc].astype(np.float64).reshape(B, 1, 1, 1)
    return A(sa) * A(x) + A(sb) * A(z), ok


def _jump_select(val, x, lat, ok, dtype):
    B, T = x.shape[:2]
    out = np.where((np.asarray(lat).reshape(B, T, 1, 1) == 1), val, x.astype(dtype))
    return np.where(ok.reshape(B, 1, 1, 1), out, np.nan).astype(dtype)


def q_jump_fp64(rows, x, lat, t, z):
    v, ok = _jump(Ex, rows, x, lat, t, z)
    return _jump_select(v.lo, x, lat, ok, np.float64)


def q_jump_bound(rows, x, lat, t, z):
    """(want, bound): two products and a sum, fused or not, on the latent frames; 0 (bit equality) on the others."""
    B, T = x.shape[:2]
    (ex, ok), (iv, _) = _jump(Ex, rows, x, lat, t, z), _jump(Iv, rows, x, lat, t, z)
    _, lim = _hull(ex, iv)
    lim = np.where(np.asarray(lat).reshape(B, T, 1, 1) == 1, lim, 0.0)
    return _jump_select(ex.lo, x, lat, ok, np.float64), lim


def q_jump_f32(rows, x, lat, t, z):
    """The kernel's order: fmaf(sqrt_beta[t], z, sqrt_alpha[t] * x)."""
    B = x.shape[0]
    t = np.asarray(t, np.int64)
    ok = (t >= 0) & (t < len(rows[0]))
    tc = np.where(ok, t, 0)
    sa, sb = rows[0][tc].reshape(B, 1, 1, 1), rows[1][tc].reshape(B, 1, 1, 1)
    p = (sa * x.astype(F)).astype(F)
    v = (sb.astype(np.float64) * z.astype(np.float64) + p.astype(np.float64)).astype(F)
    return _jump_select(v, x, lat, ok, F)


def jump_noise_f32(seed, offset, shape):
    n = int(np.prod(shape))
    return normal_f32(seed, offset, np.arange(n)).reshape(shape)


# ------------------------------------------------------------------------------------------------------------ the schedule
def repaint_schedule_ref(t_start, jump_length, n_resample):
    """The walk written from the paper's nested loops rather than from the project's while-loop: descend from t_start; each time the
    distance from t_start reaches a multiple of jump_length (and the level is still >= 0), go back up jump_length levels and redo the
    stretch, n_resample - 1 extra times per such level."""
    ops = []

    def descend(frm, to):                   # steps at frm, frm - 1, ..., to + 1: leaves the chain at level `to`
        for level in range(frm, to, -1):
            ops.append(("step", level))

    level = t_start
    while level >= 0:
        nxt = level - jump_length           # the level this stretch ends at
        if nxt < 0:                         # the last, short stretch: straight down to -1
            descend(level, -1)
            break
        descend(level, nxt)
        for _ in range(n_resample - 1):
            for up in range(nxt + 1, level + 1):
                ops.append(("jump", up))
            descend(level, nxt)
        level = nxt
    return ops


def repaint_steps(t_start, jump_length, n_resample):
    return t_start + 1 + (n_resample - 1) * jump_length * (t_start // jump_length)
