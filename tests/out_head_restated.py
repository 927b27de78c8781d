"""Restatement of the output head as the forward runs it (csrc/engine.hip: out_head(); csrc/misc.hip: head_gemm_kernel, out_gather_kernel;
the generic kernel of csrc/igemm.hip; vd_op_out_head), torch-CPU only, in float64 by default.

    a = SiLU(h * A[frame] + B[frame])                       GroupNorm32 folded to an affine per (frame, channel) + SiLU   unet.py:744-746
    out[n][co][y][x] = b[co] + sum over c, dy, dx of a[n][y + dy - 1][x + dx - 1][c] * w[co][c][dy][dx]                   unet.py:747-749,838
    with a = 0 outside the image (conv_nd(.., 3, padding=1): zero padding AFTER the activation)

Layouts are the operator's: h [N][H][W][C] (channels last), A / B [N][C], w [Cout][C][3][3] (the checkpoint's), b [Cout], out
[N][Cout][H][W].  The nine taps are written out one by one, so that the test of this file against torch.nn.functional.conv2d checks
the tap order and the padding, and so that the float32 run of the same lines is the yardstick's own rounding (head_bound()).

CASES is the GPU test's list, (nfr, H, W, C, Cout) by the path vd_out_head_variant must name for them; the CPU test asks the library
for these names without a GPU.
"""
import torch
import torch.nn.functional as F

# the project's per-operator bar: no bound of this file's may exceed it
ATOL, RTOL = 1e-4, 1e-4
# three times the largest error measured on an MI355X over CASES, relative to max |ref| (tests/test_gpu_out_head.py lists the maxima)
FLOOR = 1.3e-6

CASES = {
    "head_gemm/tpw2": [(1, 32, 32, 128, 3), (3, 32, 32, 32, 3), (2, 64, 16, 64, 3), (2, 16, 64, 96, 3), (1, 32, 32, 8, 3),
                       (1, 32, 32, 120, 3), (2, 64, 64, 128, 3)],
    # the smallest pixel count that takes the 8-tiles-per-wave form: nfr * H * W = 512 * 1024
    "head_gemm/tpw8": [(128, 64, 64, 32, 3)],
    "igemm/32": [(2, 16, 16, 128, 3), (1, 20, 20, 64, 3), (3, 24, 40, 32, 3), (1, 4, 4, 32, 3), (1, 48, 48, 128, 3), (1, 32, 32, 256, 3)],
    "igemm/64": [(2, 32, 32, 128, 6), (1, 20, 20, 64, 6), (1, 64, 64, 32, 6)],
}
ALL_CASES = [(path, c) for path, cs in CASES.items() for c in cs]


def label(c):
    return "n%d_%dx%d_c%d_o%d" % c


def make_inputs(c, seed=0):
    """h ~ N(0, 1.5) with the border pixels three times as large and a pixel in every corner region at +-30 in all channels (SiLU
    saturated on both sides; the largest values sit where a padding or a frame-leak error would pick them up), (A, B) different
    per frame and channel, w ~ N(0, 0.1), b ~ N(0, 0.5)."""
    nfr, H, W, C, Cout = c
    g = torch.Generator().manual_seed(1000 + seed)
    h = torch.randn(nfr, H, W, C, generator=g) * 1.5
    h[:, 0] *= 3.0
    h[:, -1] *= 3.0
    h[:, 1:-1, 0] *= 3.0
    h[:, 1:-1, -1] *= 3.0
    for n in range(nfr):
        s = 1.0 if n % 2 == 0 else -1.0
        h[n, 0, 0] = 30.0 * s
        h[n, 0, W - 1] = -30.0 * s
        h[n, H - 1, 0] = -30.0 * s
        h[n, H - 1, W - 1] = 30.0 * s
        h[n, H // 2, W // 2] = 30.0 * s
    step = (torch.arange(nfr) % 5).view(nfr, 1)                             # neighbouring frames differ by a whole step as well
    A = 1.0 + 0.3 * torch.randn(nfr, C, generator=g) + 0.1 * step
    B = 0.5 * torch.randn(nfr, C, generator=g) - 0.2 * step
    w = 0.1 * torch.randn(Cout, C, 3, 3, generator=g)
    b = 0.5 * torch.randn(Cout, generator=g)
    return h, A, B, w, b


def head_ref(h, A, B, w, b, dtype=torch.float64, pad_mode="constant"):
    """conv2d(silu(h * A[n, :] + B[n, :]), w, b, padding=1), NHWC in, NCHW out, evaluated in `dtype`.  pad_mode is torch.nn.functional.pad's:
    "constant" (zeros) is the operator; the CPU test shows that "replicate" (a clamped read) does not pass for it."""
    N, H, W, C = h.shape
    a = F.silu(h.to(dtype) * A.to(dtype).view(N, 1, 1, C) + B.to(dtype).view(N, 1, 1, C)).permute(0, 3, 1, 2)       # n c y x
    a = F.pad(a, (1, 1, 1, 1), mode=pad_mode)
    wd = w.to(dtype)
    out = b.to(dtype).view(1, -1, 1, 1).expand(N, -1, H, W).clone()
    for dy in range(3):
        for dx in range(3):
            out += torch.einsum("ncyx,oc->noyx", a[:, :, dy:dy + H, dx:dx + W], wd[:, :, dy, dx])
    return out


def head_bound(ref, ref32, floor):
    """(bound per element, e32): e32 = max |float32 run - float64 run| / max |ref|, the yardstick's own rounding at these inputs;
    bound = max(4 e32, floor) max |ref| with `floor` measured on the GPU (relative to max |ref|), cut per element at the project's bar
    ATOL + RTOL |ref|."""
    scale = float(ref.abs().max())
    e32 = float((ref32.double() - ref).abs().max()) / scale
    return torch.clamp(ATOL + RTOL * ref.abs(), max=max(4.0 * e32, floor) * scale), e32


def scaled_error(got, ref):
    """max |got - ref| / max |ref| (NaN where got is)."""
    return float((got.double() - ref).abs().max() / ref.abs().max())
