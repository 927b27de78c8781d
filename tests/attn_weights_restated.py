"""Restatement of the return_attn_weights maps (csrc/backward.hip: attn_temporal_weights_kernel, attn_temporal_weights_long_kernel,
attn_spatial_weights_kernel; vd_op_attn_temporal_weights, vd_op_attn_spatial_weights), torch-CPU only, in float64 by default.

    temporal  map[b * HW + p][t][s] = | mean over heads of softmax_s(q'_t . (k_s + Rk[t,s]) + (k_s * scale) . Rq[s,t], masked) |
    spatial   map[n][i][j]          = | mean over heads of softmax_j(q'_i . k_j) |                     unet.py:457-466 (return_attn_weights:
                                                                                    attn.view(B * D, -1, T, T).mean(dim=1).abs())

The softmax weights are those of attn_temporal_restated.attn_weights / attn_spatial_restated.attn_weights (logits, RPE terms and the
mask rule of unet.py:511-524 are stated there, once); this file adds the head mean, the layouts of the two operators' outputs, the
bound and the GPU tests' case lists.
"""
import torch

import attn_spatial_restated as RS
import attn_temporal_restated as RT

# the project's bar for softmax weights in [0, 1] (tests/test_gpu_long_window.py): no floor of this file's may exceed it
ATOL, RTOL = 2e-5, 1e-4
# three times the largest error measured on an MI355X over the cases below, relative to max ref, per kernel family
# (tests/test_gpu_attn_weights.py lists the maxima)
FLOOR_TEMPORAL = 4.6e-6
FLOOR_SPATIAL = 2.4e-6


def temporal_maps(qkv, Rk, Rq, m, allow, B, T, HW, C, heads, dtype=torch.float64, pairs=RT.allowed_pairs):
    """[B * HW][T][T]; qkv [B][T][HW][3C], Rk / Rq [B][T][T][C] or None, m [B][T] (1 = real frame) or None."""
    a, _ = RT.attn_weights(qkv, Rk, Rq, m, allow, B, T, HW, C, heads, dtype, pairs)             # B HW heads T T
    return a.mean(2).abs().reshape(B * HW, T, T)


def spatial_maps(qkv, N, L, C, heads, dtype=torch.float64):
    """[N][L][L]; qkv [N][L][3C]."""
    a, _ = RS.attn_weights(qkv, N, L, C, heads, dtype)                                          # N heads L L
    return a.mean(1).abs()


def maps_bound(ref, ref32, floor):
    """(bound per element, e32, scale): scale = max ref, e32 = max |float32 run - float64 run| / scale (the yardstick's own rounding
    at these inputs: with one key's logits x40 it carries the float32 rounding of logits of several hundred into the exponent),
    bound = max(4 e32 scale, min(floor scale, ATOL + RTOL ref)) with `floor` measured on the GPU, relative to scale."""
    scale = float(ref.max())
    e32 = float((ref32.double() - ref).abs().max()) / scale
    return torch.clamp(ATOL + RTOL * ref, max=floor * scale).clamp(min=4.0 * e32 * scale), e32, scale


# ---------------------------------------------------------------------------------------------------- cases of the GPU tests
# (B, T, HW, C, heads, rpe, mask, allow, hot).  T <= 32: attn_temporal_weights_kernel, above: the long kernel in query chunks of 32
# (T = 33, 65, 97: a last chunk of ONE row -- once with a mask and relative positions, once with a hot key, once with both).  Head dims
# 6, 16, 24, 64, 128 (T 128 at F 128: 117 KB of LDS); heads 1, 2, 4, 8; 1, 5, 16 pixels.  Masks: "half" (every other frame of item 0 and
# the middle frame of both are padding) and "pad16" (the last 20 frames) as in tests/test_gpu_long_window.py, "allpad" (item 0 ALL
# padding: the identity at allow 0, a full softmax at allow 1; item 1 "half").  hot: one key frame x40.
TEMPORAL_CASES = [
    (2, 1, 5, 32, 2, True, None, 1, False),
    (2, 2, 16, 12, 2, True, "half", 0, False),
    (2, 7, 5, 96, 4, True, "half", 1, False),
    (2, 7, 1, 64, 1, False, "allpad", 0, True),
    (2, 31, 16, 128, 8, True, "pad16", 0, False),
    (2, 31, 5, 48, 8, False, "half", 1, True),
    (2, 32, 16, 128, 1, True, "pad16", 1, False),
    (2, 32, 5, 256, 4, True, "allpad", 1, True),
    (2, 33, 16, 64, 4, True, "half", 0, False),
    (2, 33, 5, 24, 1, False, "allpad", 0, True),
    (2, 64, 16, 128, 2, True, None, 1, False),
    (2, 65, 1, 48, 8, True, "pad16", 0, False),
    (2, 65, 5, 128, 1, False, "half", 1, True),
    (2, 97, 16, 96, 4, True, "pad16", 1, True),
    (2, 97, 5, 64, 4, False, "allpad", 1, False),
    (2, 128, 16, 128, 1, True, "half", 0, False),
    (1, 128, 5, 256, 4, False, "pad16", 0, True),
    (2, 128, 1, 12, 2, True, "allpad", 0, False),
]

# (nfr, L, C, heads, hot).  Query tiles of 16: L = 15, 17, 100 end in a clamped tile (each once with a hot key), 1 is a tile of one row.
# Head dims 4, 24, 64, 128; heads 1, 2, 4; hot: one key late in the sequence x40.  L = 1024 needs 131 KB of LDS for its 32 rows.
SPATIAL_CASES = [
    (1, 1, 8, 2, False),
    (3, 15, 48, 2, True),
    (3, 15, 4, 1, False),
    (1, 16, 64, 1, False),
    (3, 17, 128, 1, True),
    (1, 17, 16, 4, False),
    (3, 64, 96, 4, False),
    (1, 64, 256, 4, True),
    (3, 100, 128, 2, True),
    (1, 100, 24, 1, False),
    (1, 256, 256, 2, False),
    (3, 256, 16, 4, True),
    (1, 1024, 128, 1, False),
    (1, 1024, 96, 4, True),
]


def label(c):
    return "_".join(str(int(v)) if isinstance(v, bool) else str(v) for v in c)


def make_mask(kind, B, T):
    if kind is None:
        return None
    m = torch.ones(B, T)
    if kind == "pad16":
        m[:, T - 20:] = 0
        return m
    m[:, T // 2] = 0
    if kind == "half":
        m[0, ::2] = 0
    elif kind == "allpad":
        m[0, :] = 0
    return m


def temporal_inputs(c):
    """(qkv, Rk, Rq, m): qkv ~ N(0, 1.5), R ~ N(0, 1); hot: key frame T // 3 x40 (logits of several hundred)."""
    B, T, HW, C, heads, rpe, mask, allow, hot = c
    g = torch.Generator().manual_seed(7 * T + HW + C)
    qkv = torch.randn(B, T, HW, 3 * C, generator=g) * 1.5
    if hot:
        qkv[:, T // 3, :, C:2 * C] *= 40.0
    Rk = Rq = None
    if rpe:
        Rk, Rq = torch.randn(B, T, T, C, generator=g), torch.randn(B, T, T, C, generator=g)
    return qkv, Rk, Rq, make_mask(mask, B, T)


def spatial_inputs(c):
    """qkv ~ N(0, 1.5); hot: the key at L - 1 - L // 8 x40."""
    N, L, C, heads, hot = c
    g = torch.Generator().manual_seed(11 * L + C + N)
    qkv = torch.randn(N, L, 3 * C, generator=g) * 1.5
    if hot:
        qkv[:, L - 1 - L // 8, C:2 * C] *= 40.0
    return qkv
