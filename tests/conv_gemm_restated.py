"""Plain torch-CPU statements of the convolution and linear kernels (csrc/igemm.hip, gemm_frag.hip, gemm_split.hip, conv_wino.hip,
conv_wino_r64.hip, conv_wino_z128.hip) for the per-element tests: float64 unless a dtype is asked for.  Activations are NHWC
([N][H][W][C], the layout the kernels read and write), weights OIHW; a linear layer of M rows is the 1x1 convolution of M frames of one
pixel.  Checked against explicit loops and F.conv2d in tests/test_conv_gemm_cpu.py.  Not a test file.

    conv_ref          the direct convolution: stride 1 | 2, nearest x2 upsample, virtual concat, affine + SiLU on the operand, bias,
                      per-frame bias, residual; absolute=True gives the unit S = |bias| + |fbias| + |res| + sum |a| |w| of every output
    wino_ref          F(2x2,3x3) as the kernels compute it: U = G g G^T, V = B^T d B, M = sum_c U . V, out = A^T M A, in float64 or float32
                      (the "plain fp32 evaluation of the same algorithm"); absolute=True gives S_w = ... + |A^T| (sum_c |U| . |V|) |A|;
                      subpixel=True is the four-phase form of Upsample + conv over the low-resolution map
    gn_block_sums     per (frame, block, channel) [sum, sum of squares] of a stored output in the block geometry of each kernel
"""
import torch

F64 = torch.float64
G = torch.tensor([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=F64)
BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=F64)
AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=F64)
# Upsample (nearest x2) + conv3x3 = four 3x3 phase kernels over the source map: output row 2y + p reads source rows (y - 1, y, y) for p = 0
# and (y, y, y + 1) for p = 1, so phase p's kernel rows are R[p] @ (rows of w); the same along x
R = torch.tensor([[[1, 0, 0], [0, 1, 1], [0, 0, 0]], [[0, 0, 0], [1, 1, 0], [0, 0, 1]]], dtype=F64)


def silu(x):
    return x / (1.0 + torch.exp(-x))


def operand(x0, x1=None, affA=None, affB=None, act=0, dtype=F64):
    """The operand a kernel multiplies: concat, x * A[frame] + B[frame], SiLU -- [N][H][W][Cin] in dtype."""
    x = (x0 if x1 is None else torch.cat([x0, x1], -1)).to(dtype)
    if affA is not None:
        x = x * affA.to(dtype)[:, None, None, :] + affB.to(dtype)[:, None, None, :]
    return silu(x) if act else x


def upsample2(x):
    return x.repeat_interleave(2, 1).repeat_interleave(2, 2)


def _epilogue(out, bias, fbias, res, absolute):
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    if bias is not None:
        out = out + f(bias.to(out.dtype))
    if fbias is not None:
        out = out + f(fbias.to(out.dtype))[:, None, None, :]
    if res is not None:
        out = out + f(res.to(out.dtype))
    return out


def conv_ref(a, w, bias=None, *, stride=1, ups=0, fbias=None, res=None, absolute=False, dtype=F64, sequential=False, first=False):
    """a: the operand (operand()), [N][H][W][Cin]; w: OIHW, 3x3 (zero padding 1) or 1x1.  out[n][y][x][o] = bias[o] + fbias[n][o] +
    res[n][y][x][o] + sum over taps and channels of a[n][y s + dy - pad][x s + dx - pad][c] w[o][c][dy][dx], one matrix product per tap.
    sequential: the sum as a plain loop instead -- one product and one addition per (tap, channel), taps outermost, every one rounded
    to dtype -- so that the float32 evaluation has ONE defined order (a BLAS product blocks the sum by the CPU's vector width and
    thread count: its rounding, and with it a bound taken from it, would differ from machine to machine).  first: the sum starts AT
    bias + fbias + res, as the accumulators of gemm_frag.hip and gemm_split.hip do, instead of receiving them last (igemm.hip)."""
    a, w = a.to(dtype), w.to(dtype)
    if absolute:
        a, w = a.abs(), w.abs()
    if ups:
        a = upsample2(a)
    N, H, W, C = a.shape
    O, _, k, _ = w.shape
    pad = (k - 1) // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    ap = torch.zeros(N, H + 2 * pad, W + 2 * pad, C, dtype=dtype)
    ap[:, pad:pad + H, pad:pad + W] = a
    out = torch.zeros(N, Ho, Wo, O, dtype=dtype)
    if first:
        out = _epilogue(out, bias, fbias, res, absolute)
    for dy in range(k):
        for dx in range(k):
            patch = ap[:, dy:dy + stride * (Ho - 1) + 1:stride, dx:dx + stride * (Wo - 1) + 1:stride]
            if sequential:
                for ch in range(C):
                    out += patch[..., ch:ch + 1] * w[:, ch, dy, dx]
            else:
                out += (patch.reshape(-1, C) @ w[:, :, dy, dx].t()).reshape(N, Ho, Wo, O)
    return out if first else _epilogue(out, bias, fbias, res, absolute)


def linear_ref(a, w, bias=None, res=None, absolute=False, dtype=F64):
    """a [M][K], w [N][K]: a w^T + bias + res."""
    a, w = a.to(dtype), w.to(dtype)
    if absolute:
        a, w = a.abs(), w.abs()
    out = a @ w.t()
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    if bias is not None:
        out = out + f(bias.to(dtype))
    if res is not None:
        out = out + f(res.to(dtype))
    return out


def phase_kernels(w):
    """OIHW -> [2][2][O][I][3][3] float64: g[py][px] = R[py] w R[px]^T."""
    return torch.einsum("pik,ockl,qjl->pqocij", R, w.to(F64), R)


def _wino_same(a, w, dtype, absolute):
    """F(2x2,3x3) of a [N][H][W][C] (H, W even) with w OIHW in float64, zero padding 1: [N][H][W][O] in dtype, without the epilogue.
    U is formed in float64 and rounded once to dtype (as the weight packers do); everything after it runs in dtype."""
    N, H, W, C = a.shape
    O = w.shape[0]
    U = torch.einsum("ik,ockl,jl->ijoc", G, w.to(F64), G).to(dtype)                   # [4][4][O][C]
    ap = torch.zeros(N, H + 2, W + 2, C, dtype=dtype)
    ap[:, 1:H + 1, 1:W + 1] = a.to(dtype)
    d = ap.unfold(1, 4, 2).unfold(2, 4, 2)                                            # [N][H/2][W/2][C][4][4]
    Bt, At = BT.to(dtype), AT.to(dtype)
    V = torch.einsum("ik,nyxckl,jl->ijnyxc", Bt, d, Bt)                               # [4][4][N][th][tw][C]
    if absolute:
        U, V, At = U.abs(), V.abs(), At.abs()
    T = N * (H // 2) * (W // 2)
    M = torch.bmm(V.reshape(16, T, C), U.reshape(16, O, C).transpose(1, 2)).reshape(4, 4, N, H // 2, W // 2, O)
    Y = torch.einsum("pi,ijnyxo,qj->nypxqo", At, M, At)                               # [N][th][2][tw][2][O]
    return Y.reshape(N, H, W, O)


def wino_ref(a, w, bias=None, *, ups=0, subpixel=False, fbias=None, res=None, absolute=False, dtype=F64):
    """The stride-1 3x3 convolution as the Winograd kernels compute it.  ups: the source is read through a nearest x2 upsample (the
    transform then runs on the upsampled map); subpixel: Upsample + conv as four phase convolutions over the source map, interleaved."""
    if subpixel:
        N, H, W, _ = a.shape
        g = phase_kernels(w)
        out = torch.zeros(N, 2 * H, 2 * W, w.shape[0], dtype=dtype)
        for py in range(2):
            for px in range(2):
                out[:, py::2, px::2] = _wino_same(a, g[py, px], dtype, absolute)
    else:
        out = _wino_same(upsample2(a) if ups else a, w, dtype, absolute)
    return _epilogue(out, bias, fbias, res, absolute)


# ---- GroupNorm partial tables: [N][split][C][2] float64 of a stored output [N][Ho][Wo][C]
def gn_block_sums(out, geometry, rows=0):
    """geometry: "wino" -- one entry per 16 x 16 tile group (row-major; a map of 8 x 8: one entry), the Winograd kernels and, with one
    entry per frame, the split-K reduce kernel (maps <= 16 x 16);
    "ups" -- the sub-pixel form: per 16 x 16 group of SOURCE pixels (32 x 32 of the output) four entries, 2 py + px, each over the output
    pixels (2y + py, 2x + px); "rows" -- the GEMM epilogue: blocks of `rows` consecutive rows of a frame (vd_linear_stats_split)."""
    o = out.to(F64)
    N, Ho, Wo, C = o.shape
    if geometry == "rows":
        b = o.reshape(N, Ho * Wo // rows, rows, C)
        return torch.stack([b.sum(2), (b * b).sum(2)], -1)
    if geometry == "wino":
        t = 16 if Ho >= 16 else Ho
        b = o.reshape(N, Ho // t, t, Wo // t, t, C).permute(0, 1, 3, 2, 4, 5).reshape(N, (Ho // t) * (Wo // t), t * t, C)
        return torch.stack([b.sum(2), (b * b).sum(2)], -1)
    assert geometry == "ups"
    t = 32 if Ho >= 32 else Ho
    gy, gx = Ho // t, Wo // t
    b = o.reshape(N, gy, t // 2, 2, gx, t // 2, 2, C).permute(0, 1, 4, 3, 6, 2, 5, 7).reshape(N, gy * gx * 4, (t // 2) ** 2, C)
    return torch.stack([b.sum(2), (b * b).sum(2)], -1)
