"""Restatement of the spatial attention operator (csrc/attn_spatial.hip; vd_op_attn_spatial), torch-CPU only, in float64 by default.

    q' = q * scale,  scale = F^-1/2                                              unet.py:487
    w[i,j] = q'_i . k_j                                                          unet.py:489
    a = softmax_j(w);  o_i = sum_j a[i,j] v_j                                    unet.py:525-534 (no RPE, no mask: the call at :260-266)

per (frame, head).  Layouts are the operator's: qkv [N][L][3C] (q | k | v thirds, head h at h*F inside each), out [N][L][C].

row_scale() is the unit the per-element tests measure an error in: an output row (frame, query, head) is a convex combination of the
head's v_j, so no feature of it exceeds S = max over the keys and the head's features of |v_j|.  S does not depend on the query.
"""
import torch


def attn_weights(qkv, N, L, C, heads, dtype=torch.float64):
    """(a, v): softmax(q F^-0.5 k^T) [N][heads][L][L] and the values [N][heads][L][F], evaluated in `dtype`."""
    Fd = C // heads
    x = qkv.to(dtype).reshape(N, L, 3, heads, Fd).permute(2, 0, 3, 1, 4)              # t N H L F
    q, k, v = x[0] * Fd ** -0.5, x[1], x[2]
    return torch.softmax(q @ k.transpose(-1, -2), -1), v


def attn_ref(qkv, N, L, C, heads, dtype=torch.float64):
    """softmax(q F^-0.5 k^T) v per (frame, head), evaluated in `dtype`: out [N][L][C]."""
    a, v = attn_weights(qkv, N, L, C, heads, dtype)
    return (a @ v).permute(0, 2, 1, 3).reshape(N, L, C)


def row_scale(qkv, N, L, C, heads):
    """S [N][heads] in float64: max over the keys and the head's features of |v|."""
    Fd = C // heads
    return qkv.double()[..., 2 * C:].reshape(N, L, heads, Fd).abs().amax(dim=(1, 3))


def scaled_errors(got, ref, S):
    """|got - ref| / S per element, [N][L][heads][F] in float64 (NaN where got is)."""
    N, heads = S.shape
    L = got.shape[1]
    return (got.double() - ref.double()).abs().reshape(N, L, heads, -1) / S.view(N, 1, heads, 1)


def scaled_error(got, ref, S):
    """max over elements of |got - ref| / S."""
    return float(scaled_errors(got, ref, S).max())
