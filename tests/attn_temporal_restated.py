"""Restatement of the temporal attention operator (csrc/attn_temporal.hip, csrc/attn_temporal_long.hip; vd_op_attn_temporal),
torch-CPU only, in float64 by default.

    q' = q * scale,  scale = F^-1/2                                              unet.py:487
    w[t,s]  = q'_t . k_s                                                         unet.py:489
    w[t,s] += q'_t . Rk[t,s]                                                     unet.py:502, einsum of :362-366
    w[t,s] += (k_s * scale) . Rq[s,t]        the rpe_q term is TRANSPOSED        unet.py:506-509
    ok[t,s] = m_t m_s (+ (1 - m_t)(1 - m_s) if allow, else ok[t,t] = 1);  w[t,s] = -inf where ok[t,s] == 0      unet.py:511-524
    a = softmax_s(w);  o_t = sum_s a[t,s] (v_s + Rv[t,s])                        unet.py:525-534, einsum of :374-378

Layouts are the operator's: qkv [B][T][HW][3C] (q | k | v, each heads x F), R* [B][T][T][C], mask [B][T] (1 = real frame), out
[B][T][HW][C].

row_scale() is the unit the per-element tests measure an error in: an output row (b, t, pixel, head) is a convex combination of the
vectors v_s + Rv[t,s] over the allowed s, so no feature of it exceeds S = max over allowed s and the head's features of
|v_s + Rv[t,s]| (max |v_s| without relative positions).
"""
import torch


def allowed_pairs(m, allow, B, T):
    """bool [B][T][T]: may query frame t attend to key frame s (unet.py:511-521); all True without a mask."""
    if m is None:
        return torch.ones(B, T, T, dtype=torch.bool)
    m = m.double()
    ok = m.view(B, 1, T) * m.view(B, T, 1)
    if allow:
        ok = ok + (1 - m.view(B, 1, T)) * (1 - m.view(B, T, 1))
    else:
        ok = ok.clone()
        ok[:, range(T), range(T)] = 1.0
    return ok != 0


def attn_weights(qkv, Rk, Rq, m, allow, B, T, HW, C, heads, dtype=torch.float64, pairs=allowed_pairs):
    """(a, v): the softmax weights a [B][HW][heads][T][T] of unet.py:486-525 (RPE terms :357-366, :502-509; mask rule :511-524 as
    `pairs` states it) and the values v [B][HW][heads][T][F], evaluated in `dtype`."""
    Fd = C // heads
    scale = Fd ** -0.5
    x = qkv.to(dtype).permute(0, 2, 1, 3).reshape(B, HW, T, 3, heads, Fd).permute(3, 0, 1, 4, 2, 5)     # t B D H T F
    q, k, v = x[0] * scale, x[1], x[2]
    w = q @ k.transpose(-1, -2)
    if Rk is not None:
        rk, rq = (r.to(dtype).view(B, T, T, heads, Fd) for r in (Rk, Rq))
        w = w + torch.einsum("bdhtf,btshf->bdhts", q, rk)
        w = w + torch.einsum("bdhtf,btshf->bdhts", k * scale, rq).transpose(-1, -2)
    if m is not None:
        w = w.masked_fill(~pairs(m, allow, B, T).view(B, 1, 1, T, T), float("-inf"))
    return torch.softmax(w, -1), v


def attn_ref(qkv, Rk, Rq, Rv, m, allow, B, T, HW, C, heads, dtype=torch.float64):
    """unet.py:486-536 + the RPE einsums :357-378 + the mask rule :511-524, evaluated in `dtype`."""
    a, v = attn_weights(qkv, Rk, Rq, m, allow, B, T, HW, C, heads, dtype)
    o = a @ v
    if Rk is not None:
        o = o + torch.einsum("bdhts,btshf->bdhtf", a, Rv.to(dtype).view(B, T, T, heads, C // heads))
    return o.permute(0, 3, 1, 2, 4).reshape(B, T, HW, C)


def row_scale(qkv, Rv, m, allow, B, T, HW, C, heads):
    """S [B][T][HW][heads] in float64: max over the allowed s and the head's features of |v_s + Rv[t,s]|."""
    Fd = C // heads
    v = qkv.double()[..., 2 * C:].reshape(B, T, HW, heads, Fd)                      # b s p h f
    ok = allowed_pairs(m, allow, B, T)
    S = torch.empty(B, T, HW, heads, dtype=torch.float64)
    for t in range(T):
        u = v
        if Rv is not None:
            u = v + Rv.double()[:, t].reshape(B, T, 1, heads, Fd)                   # v_s + Rv[t,s]
        mag = u.abs().amax(-1)                                                      # b s p h
        mag = mag.masked_fill(~ok[:, t].view(B, T, 1, 1), 0.0)
        S[:, t] = mag.amax(1)
    return S


def scaled_error(got, ref, S, rows=None):
    """max over elements of |got - ref| / S_row; rows: bool [B][T] to keep only some (b, t) rows."""
    B, T, HW, heads = S.shape
    e = (got.double() - ref.double()).abs().reshape(B, T, HW, heads, -1) / S.unsqueeze(-1)
    if rows is not None:
        e = e[rows]
    return float(e.max())
