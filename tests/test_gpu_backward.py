"""GPU: the backward-data kernels of `use_gradient_method` (csrc/backward.hip), one at a time, against fp64 torch autograd of
a plain restatement of each forward; then guided steps on the engine against autograd through the CPU oracle at the windows
the step accepts (padding, up to 32 frames, every conditioning mode, no clipping, the full-size model)."""
import json

import pytest
import torch
import torch.nn.functional as F

import video_diffusion_amd as vda
from helpers import ATOL, RTOL, close, synth_sd
from oracle.sampler_ref import SamplerRef
from oracle.schedule_ref import ScheduleRef
from oracle.unet_ref import UNetRef
from test_gpu_long_window import attn_ref
from video_diffusion_amd import _lib

pytestmark = pytest.mark.gpu
KEYS = vda.video_model_and_diffusion_defaults().keys()
STEM_KPAD = 64                              # engine.hip: im2col width of the stem
_cache = {}


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def dev(t):
    return None if t is None else t.float().to("cuda").contiguous()


def op(name, *args):
    """Call a vd_op_* entry: tensors and None become pointers, the current stream is appended."""
    conv = [_lib.ptr(a) if a is None or torch.is_tensor(a) else a for a in args]
    _lib.check(getattr(_lib.lib(), name)(*conv, _lib.current_stream()))
    torch.cuda.synchronize()


def rel_err(got, ref):
    return float((got.double() - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


def report(what, err):
    """The measured error, printed for the docstrings (pytest -s)."""
    print(f"\nERR {what} {err:.3e}")


def part_scale(part, whole):
    """max|ref| of one of dq / dk / dv; a part that is exactly zero (a softmax over one key) is held to the whole's scale."""
    return float(part.abs().max()) or float(whole.abs().max())


# ---------------------------------------------------------------------------------------------------- GroupNorm backward
def gn_case(N, HW, C, C0, act, film, mean, gmag, seed):
    """x0 | x1, dy, the folded affine (A, B) and (mean, rstd) as the forward leaves them on the tape: fp64 from x, rounded to
    fp32.  gamma' = gamma * (1 + scale), beta' = beta * (1 + scale) + shift per frame (unet.py:185-198)."""
    x = rnd(N, HW, C, seed=seed) + mean
    x[..., ::3] *= 0.5                                                # channels of unequal spread inside a group
    dy = rnd(N, HW, C, seed=seed + 1)
    gamma, beta = rnd(C, seed=seed + 2) * gmag + 1, rnd(C, seed=seed + 3)
    if film:
        scale, shift = rnd(N, C, seed=seed + 4) * 0.5, rnd(N, C, seed=seed + 5)
    else:
        scale, shift = torch.zeros(N, C), torch.zeros(N, C)
    gp = gamma.double() * (1 + scale.double())                       # [N][C]
    bp = beta.double() * (1 + scale.double()) + shift.double()
    xg = x.double().view(N, HW, 32, C // 32)
    mu = xg.mean(dim=(1, 3))                                         # [N][32]
    rstd = 1.0 / torch.sqrt(((xg - mu[:, None, :, None]) ** 2).mean(dim=(1, 3)) + 1e-5)
    mr = torch.stack([mu, rstd], -1).float()                         # [N][32][2]
    rs_c = rstd.repeat_interleave(C // 32, dim=1)
    mu_c = mu.repeat_interleave(C // 32, dim=1)
    A = (rs_c * gp).float()
    B = (bp - mu_c * rs_c * gp).float()
    return x, dy, gp, bp, mr, A, B


def gn_ref(x, dy, gp, bp, C0, act):
    """fp64 autograd of act(GroupNorm32(cat(x0, x1)) * gamma' + beta') w.r.t. x0 and x1 (mean and rstd are functions of x)."""
    x0 = x[..., :C0].double().requires_grad_(True)
    x1 = x[..., C0:].double().requires_grad_(True)
    h = torch.cat([x0, x1], -1).permute(0, 2, 1)                     # [N][C][HW]
    y = F.group_norm(h, 32, eps=1e-5) * gp[:, :, None] + bp[:, :, None]
    if act:
        y = F.silu(y)
    leaves = [x0, x1] if C0 < x.shape[-1] else [x0]
    g = torch.autograd.grad(y, leaves, dy.double().permute(0, 2, 1))
    return g[0], (g[1] if len(g) > 1 else None), y


# (N, HW, C, C0, act, film, acc0, acc1, extra, mean, gmag): C0 = 64 of 160 puts a 5-channel group across the split; C = 1024
# runs one pixel per pass; HW and N move gn_bwd_split and the apply kernel's sp2; gmag 35 drives |y| past 88.7, where SiLU's
# __expf overflows; mean 30 as in test_groupnorm_fold_large_mean.
GN_CASES = [
    (7, 64, 32, 32, 1, True, 0, 0, False, 0.0, 0.3),
    (1, 1024, 96, 96, 0, False, 1, 0, True, 0.0, 0.3),
    (7, 64, 160, 64, 1, True, 1, 0, False, 0.0, 0.3),
    (41, 4, 160, 64, 0, True, 0, 1, True, 0.0, 0.3),
    (1, 4096, 384, 384, 1, True, 0, 0, False, 0.0, 0.3),
    (41, 1, 512, 512, 1, False, 1, 0, True, 0.0, 0.3),
    (7, 64, 896, 512, 1, True, 1, 1, True, 0.0, 0.3),
    (7, 64, 1024, 1024, 1, True, 0, 0, True, 0.0, 0.3),
    (41, 4, 1024, 1024, 0, False, 1, 0, False, 30.0, 0.3),
    (7, 1024, 64, 64, 1, True, 0, 0, False, 30.0, 0.3),
    (7, 256, 128, 128, 1, True, 0, 0, True, 0.0, 35.0),
    (41, 4096, 32, 32, 0, False, 0, 0, False, 0.0, 0.3),
    (1, 1, 1024, 512, 1, True, 0, 1, False, 0.0, 0.3),
    (7, 4096, 96, 32, 1, False, 1, 1, True, 30.0, 0.3),
]


@pytest.mark.parametrize("N,HW,C,C0,act,film,acc0,acc1,extra,mean,gmag", GN_CASES)
def test_gn_bwd(N, HW, C, C0, act, film, acc0, acc1, extra, mean, gmag):
    """gn_bwd_partial / fold / apply against fp64 autograd through F.group_norm over the concat, relative to max|dx|.
    Measured on an MI355X: <= 4.9e-7, bound 1.5e-6; mean 30 under SiLU 1.8e-6, bound 5e-6 (y = x * A + B is recomputed in fp32
    from x ~ 30, as the forward computes it)."""
    tol = 5e-6 if mean and act else 1.5e-6
    x, dy, gp, bp, mr, A, B = gn_case(N, HW, C, C0, act, film, mean, gmag, seed=C + HW + N)
    r0, r1, y = gn_ref(x, dy, gp, bp, C0, act)
    if gmag > 1:
        assert act and float(y.detach().abs().max()) > 89.0                   # SiLU' through __expf overflow
    ex = rnd(N, HW, C, seed=9) if extra else None
    pre0, pre1 = rnd(N, HW, C0, seed=10), rnd(N, HW, C - C0, seed=11)
    dx0, dx1 = dev(pre0), dev(pre1) if C0 < C else None
    op("vd_op_gn_bwd", dev(x[..., :C0]), dev(x[..., C0:]) if C0 < C else None, C0, C, dev(A), dev(B), dev(mr), dev(dy), act, N,
       HW, dev(ex), dx0, acc0, dx1, acc1)
    scale = max(float(r0.abs().max()), float(r1.abs().max()) if r1 is not None else 0.0)
    pairs = [(dx0.cpu(), r0 + (ex[..., :C0].double() if extra else 0) + (pre0.double() if acc0 else 0))]
    if C0 < C:
        pairs.append((dx1.cpu(), r1 + (ex[..., C0:].double() if extra else 0) + (pre1.double() if acc1 else 0)))
    report("gn_bwd", max(float((g.double() - w).abs().max()) for g, w in pairs) / scale)
    for got, want in pairs:
        assert torch.isfinite(got).all()
        close(got, want, atol=tol * scale, rtol=tol)


# ---------------------------------------------------------------------------------------------------- temporal GroupNorm backward
# (B, T, HW, C, acc, mean, tol).  T * C / 32 = 2 (T = 1, C = 64 and T = 2, C = 32): groups of two elements; where the two are
# close, x - mean cancels in the kernel's fp32 and rstd (up to 316) amplifies it, hence the wider bounds of those two cases
# (measured 7.8e-6 and 6.3e-5).
@pytest.mark.parametrize("B,T,HW,C,acc,mean,tol", [(2, 1, 64, 64, 0, 0.0, 2.4e-5), (1, 2, 7, 32, 1, 0.0, 1e-4),
                                                   (2, 5, 256, 96, 0, 0.0, 6e-7), (1, 16, 64, 384, 1, 30.0, 6e-7),
                                                   (2, 31, 7, 512, 0, 0.0, 6e-7), (1, 32, 64, 1024, 1, 0.0, 6e-7),
                                                   (2, 32, 1, 32, 0, 30.0, 6e-7), (1, 16, 256, 64, 0, 0.0, 6e-7),
                                                   (1, 5, 64, 1024, 0, 30.0, 6e-7), (2, 32, 7, 96, 1, 0.0, 6e-7)])
def test_gn_temporal_bwd(B, T, HW, C, acc, mean, tol):
    """GroupNorm32 on the (B*HW, C, T) view (unet.py:472-475) backward: fp64 autograd through F.group_norm, relative to max|dx|.
    HW 7 / 256 leave the last block of pixels ragged.  Measured on an MI355X: <= 2.0e-7 once a group holds 5 or more elements;
    bound 6e-7."""
    x = rnd(B, T, HW, C, seed=T * 7 + C) + mean
    dy = rnd(B, T, HW, C, seed=3)
    gamma = rnd(C, seed=1) + 1
    pre = rnd(B, T, HW, C, seed=4)
    dx = dev(pre)
    op("vd_op_gn_temporal_bwd", dev(x), dev(gamma), dev(dy), B, T, HW, C, acc, dx)
    xd = x.double().requires_grad_(True)
    y = F.group_norm(xd.permute(0, 2, 3, 1).reshape(B * HW, C, T), 32, gamma.double(), None, eps=1e-5)
    g, = torch.autograd.grad(y, xd, dy.double().permute(0, 2, 3, 1).reshape(B * HW, C, T))
    want = g + (pre.double() if acc else 0)
    got = dx.cpu()
    report("gn_temporal_bwd", float((got.double() - want).abs().max()) / float(g.abs().max()))
    close(got, want, atol=tol * float(g.abs().max()), rtol=tol)


def test_gn_temporal_bwd_refuses_33_frames():
    B, T, HW, C = 1, 33, 4, 64
    x = torch.zeros(B, T, HW, C, device="cuda")
    with pytest.raises(_lib.VdError, match=r"T <= 32"):
        op("vd_op_gn_temporal_bwd", x, torch.ones(C, device="cuda"), x, B, T, HW, C, 0, torch.empty_like(x))


# ---------------------------------------------------------------------------------------------------- temporal attention backward
def temporal_mask(kind, B, T):
    if kind is None:
        return None
    m = torch.ones(B, T)
    if kind == "tail":                                                # item 0: the last quarter is padding, item 1: the last frame
        m[0, T - max(1, T // 4):] = 0
        m[1:, T - 1] = 0
    elif kind == "inter":                                             # interleaved padding
        m[0, ::2] = 0
        m[1:, 1::3] = 0
    elif kind == "allpad":                                            # item 0 is padding throughout
        m[0] = 0
        m[1:, T // 2] = 0
    return m


def attn_t_call(qkv, R, m, B, T, HW, C, heads, allow, dout):
    dq = torch.full((B, T, HW, 3 * C), float("nan"), device="cuda")
    op("vd_op_attn_temporal_bwd", dev(qkv), *(dev(r) for r in R), dev(m), B, T, HW, C, heads, allow, dev(dout), dq)
    return dq


# (B, T, HW, C, heads, rpe, mask, allow, hot): head dims 8, 24, 32, 96, 128, 256; F = 256 at T = 32 is the launcher's largest
# LDS (141 568 B); hot: one key frame's logits x40 (a peaked softmax).
AT_CASES = [
    (2, 1, 5, 32, 4, True, None, 0, False),
    (2, 2, 7, 48, 2, True, "tail", 0, False),
    (2, 2, 3, 256, 1, True, None, 1, True),
    (3, 7, 9, 64, 2, True, "inter", 1, False),
    (2, 7, 5, 96, 4, False, "inter", 0, False),
    (2, 16, 4, 192, 2, True, "allpad", 0, True),
    (2, 16, 4, 192, 2, True, "allpad", 1, False),
    (2, 16, 3, 128, 1, False, None, 1, False),
    (2, 20, 6, 256, 2, False, "tail", 1, True),
    (2, 20, 5, 64, 8, True, "tail", 0, False),
    (1, 32, 4, 128, 4, True, None, 0, True),
    (2, 32, 3, 256, 1, True, "inter", 0, False),
    (2, 32, 2, 512, 2, True, "allpad", 1, True),
    (2, 32, 3, 96, 4, False, "allpad", 0, False),
]


@pytest.mark.parametrize("B,T,HW,C,heads,rpe,mask,allow,hot", AT_CASES)
def test_attn_temporal_bwd(B, T, HW, C, heads, rpe, mask, allow, hot):
    """attn_temporal_bwd against fp64 autograd of attn_ref (unet.py:486-536, RPE :357-378, mask rule :511-524), dq, dk and dv
    each relative to its own largest entry.  Measured on an MI355X: <= 1.2e-6, bound 3.5e-6; with a key frame x40 1.5e-5,
    bound 4.5e-5 (the peaked rows' dw = a * (da - sum a * da) cancels).  Item b of a batched call is bit-equal to the call on
    item b alone."""
    tol = 4.5e-5 if hot else 3.5e-6
    qkv = rnd(B, T, HW, 3 * C, seed=T + C) * 1.5
    if hot:
        qkv[:, T // 3, :, C:2 * C] *= 40.0
    R = [rnd(B, T, T, C, seed=s) if rpe else None for s in (1, 2, 3)]
    m = temporal_mask(mask, B, T)
    dout = rnd(B, T, HW, C, seed=5)
    got = attn_t_call(qkv, R, m, B, T, HW, C, heads, allow, dout).cpu()
    assert torch.isfinite(got).all()
    qd = qkv.double().requires_grad_(True)
    o = attn_ref(qd, *R, m, allow, B, T, HW, C, heads)
    want, = torch.autograd.grad(o, qd, dout.double())
    parts = [(got[..., i * C:(i + 1) * C], want[..., i * C:(i + 1) * C]) for i in range(3)]
    report("attn_temporal_bwd", max(float((g.double() - w).abs().max()) / part_scale(w, want) for g, w in parts))
    for g, w in parts:
        close(g, w, atol=tol * part_scale(w, want), rtol=tol)
    for b in range(B if B > 1 else 0):
        one = attn_t_call(qkv[b:b + 1], [r[b:b + 1] if r is not None else None for r in R],
                          m[b:b + 1] if m is not None else None, 1, T, HW, C, heads, allow, dout[b:b + 1])
        assert torch.equal(one[0].cpu(), got[b])


def test_attn_temporal_bwd_limits_are_refused():
    """T = 33 and a head dim whose LDS passes 150 KiB (C = 288, one head, T = 32: 157 952 B) are refused."""
    for T, C, heads, msg in [(33, 64, 2, r"T <= 32"), (32, 288, 1, "head dim too large")]:
        qkv = torch.zeros(1, T, 2, 3 * C, device="cuda")
        with pytest.raises(_lib.VdError, match=msg):
            op("vd_op_attn_temporal_bwd", qkv, None, None, None, None, 1, T, 2, C, heads, 0, torch.zeros(1, T, 2, C, device="cuda"),
               torch.empty_like(qkv))


# ---------------------------------------------------------------------------------------------------- spatial attention backward
def attn_sp_ref(qkv, N, L, C, heads):
    """fp64 softmax(q k^T / sqrt(F)) v per (frame, head) over the L pixels (unet.py:486-536 without RPE)."""
    Fd = C // heads
    x = qkv.view(N, L, 3, heads, Fd).permute(2, 0, 3, 1, 4)
    a = torch.softmax((x[0] * Fd ** -0.5) @ x[1].transpose(-1, -2), -1)
    return (a @ x[2]).permute(0, 2, 1, 3).reshape(N, L, C)


# (N, L, C, heads, qmag, kmag, vmag, peak): L ragged against the 16-query tile (5, 15, 17, 100) and up to the launcher's 1024
# (the dq pass then holds 145 KiB of LDS); head dims 4, 8, 32, 96, 128; magnitudes as test_attention_spatial_accuracy_over_magnitudes;
# peak: one key's logits x30 for every query.
AS_CASES = [
    (3, 1, 32, 1, 1.0, 1.0, 1.0, False),
    (2, 5, 32, 8, 1.0, 1.0, 1.0, False),
    (2, 15, 64, 8, 1.0, 1.0, 1.0, False),
    (2, 16, 96, 1, 1.0, 1.0, 1.0, False),
    (2, 17, 128, 1, 1.0, 1.0, 1.0, True),
    (3, 64, 256, 2, 1.0, 1.0, 1.0, False),
    (2, 100, 192, 2, 1.0, 1.0, 1.0, False),
    (2, 256, 128, 4, 1.0, 1.0, 1.0, False),
    (1, 1024, 128, 1, 1.0, 1.0, 1.0, False),
    (1, 1024, 32, 8, 1.0, 1.0, 1.0, True),
    (2, 64, 384, 4, 1e-3, 1.0, 1e-3, False),
    (2, 64, 384, 4, 30.0, 0.5, 100.0, False),
    (2, 100, 128, 4, 1e-6, 1e-6, 1e3, False),
    (2, 64, 384, 4, 200.0, 0.05, 1e-4, False),
    (2, 256, 64, 2, 1.0, 1.0, 1.0, True),
]


@pytest.mark.parametrize("N,L,C,heads,qm,km,vm,peak", AS_CASES)
def test_attn_spatial_bwd(N, L, C, heads, qm, km, vm, peak):
    """attn_sp_bwd_dq / _dkv against fp64 autograd, dq, dk and dv each relative to its own largest entry.  Measured on an
    MI355X: <= 1.4e-6, bound 4e-6; peaked rows (a key x30, or |q| * |k| >= 10) 1.7e-5, bound 5e-5 (dS = P * (dP - D) cancels)."""
    tol = 5e-5 if peak or qm * km >= 10 else 4e-6
    Fd = C // heads
    g = torch.Generator().manual_seed(L + C)
    q, k, v = (torch.randn(N, L, heads, Fd, generator=g) * mg for mg in (qm, km, vm))
    if peak:
        k[:, L // 2] *= 30.0
    qkv = torch.stack([q, k, v], dim=2).reshape(N, L, 3 * C).contiguous()
    dout = rnd(N, L, C, seed=7)
    dq = torch.full((N, L, 3 * C), float("nan"), device="cuda")
    op("vd_op_attn_spatial_bwd", dev(qkv), N, L, C, heads, dev(dout), dq)
    got = dq.cpu()
    assert torch.isfinite(got).all()
    qd = qkv.double().requires_grad_(True)
    want, = torch.autograd.grad(attn_sp_ref(qd, N, L, C, heads), qd, dout.double())
    parts = [(got.view(N, L, 3, C)[:, :, i], want.view(N, L, 3, C)[:, :, i]) for i in range(3)]
    report("attn_spatial_bwd", max(float((g.double() - w).abs().max()) / part_scale(w, want) for g, w in parts))
    for g, w in parts:
        close(g, w, atol=tol * part_scale(w, want), rtol=tol)


def test_attn_spatial_bwd_limits_are_refused():
    for L, C, heads, msg in [(1025, 64, 2, "L <= 1024"), (16, 132, 1, "head dim <= 128")]:
        qkv = torch.zeros(1, L, 3 * C, device="cuda")
        with pytest.raises(_lib.VdError, match=msg):
            op("vd_op_attn_spatial_bwd", qkv, 1, L, C, heads, torch.zeros(1, L, C, device="cuda"), torch.empty_like(qkv))


# ---------------------------------------------------------------------------------------------------- output head, stem
@pytest.mark.parametrize("N,H,W,C", [(3, 1, 1, 32), (2, 2, 2, 128), (4, 8, 8, 192), (2, 32, 32, 32), (1, 64, 64, 128),
                                     (2, 8, 32, 192), (2, 5, 3, 32)])
def test_out_conv_bwd(N, H, W, C):
    """The output head's 3x3 conv (unet.py:744-749) backward-data: fp64 autograd of F.conv2d(padding=1); NCHW in, NHWC out.
    Measured on an MI355X: <= 2.6e-7 of max|da|; bound 8e-7."""
    Cout = 3
    wt = rnd(Cout, C, 3, 3, seed=C) * 0.1                            # OIHW
    w = wt.permute(2, 3, 0, 1).reshape(9, Cout, C)                   # [tap][Cout][C] as the forward stores it
    deps = rnd(N, Cout, H, W, seed=H * W)
    da = torch.full((N, H, W, C), float("nan"), device="cuda")
    op("vd_op_out_conv_bwd", dev(deps), dev(w), N, H, W, C, Cout, da)
    a = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
    want, = torch.autograd.grad(F.conv2d(a, wt.double(), padding=1), a, deps.double())
    want = want.permute(0, 2, 3, 1)
    got = da.cpu()
    report("out_conv_bwd", rel_err(got, want))
    close(got, want, atol=8e-7 * float(want.abs().max()), rtol=8e-7)


class _StemTap(UNetRef):
    """The oracle's with_grad up to the stem input: its x5 of each conditioning mode, captured in place of the network."""

    def __init__(self, cond):
        self.cond, self.out_ch = cond, 3

    def torso(self, x5, t_frames, fidx, mask, B, T):
        self.x5 = x5
        return torch.zeros(x5.shape[0], 3, x5.shape[2], x5.shape[3], dtype=x5.dtype)


# per frame (obs, lat, km): latent, observed, padding, kinda-marginal, latent + kinda-marginal
STEM_FRAMES = [(0, 1, 0), (1, 0, 0), (0, 0, 0), (0, 0, 1), (0, 1, 1)]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("B,H,W", [(2, 8, 8), (1, 5, 7), (1, 32, 32)])
def test_stem_col2im(mode, B, H, W):
    """stem_col2im: d<cols, dcols>/dx, cols = the stem's im2col of the oracle's network input x5 (UNetRef.with_grad, observed
    frames from x_0, so x0 is held constant), k = tap * Cs + channel, padded to STEM_KPAD; fp64 autograd.  The guided step
    always passes obs = 0 to this kernel: its factor lat + 1 - any is the x-derivative only while the observed frames' source
    is not x.  Columns past 9 * Cs and those of the non-x channels hold noise the kernel must ignore.  The oracle casts x5 to
    fp32, so the reference's gradient at x5 carries one fp32 rounding.  Measured on an MI355X: <= 1.2e-7 of max|dx|; bound
    3.5e-7."""
    cond = ["channel", "duplicate", "t=0"][mode]
    Cs = [5, 6, 3][mode]
    T = len(STEM_FRAMES)
    N = B * T
    obs, lat, km = (torch.tensor([f[i] for f in STEM_FRAMES] * B, dtype=torch.float32).view(B, T, 1, 1, 1) for i in range(3))
    x = rnd(B, T, 3, H, W, seed=H).double().requires_grad_(True)
    x0 = rnd(B, T, 3, H, W, seed=H + 1).double()
    tap = _StemTap(cond)
    tap.with_grad(x, torch.zeros(B), x0=x0, obs_mask=obs.double(), latent_mask=lat.double(), kinda_marg_mask=km.double(),
                  observed_frames="x_0")
    x5 = tap.x5.double()
    assert x5.shape == (N, Cs, H, W)
    cols = F.unfold(x5, 3, padding=1).view(N, Cs, 9, H * W).permute(0, 3, 2, 1).reshape(N, H * W, 9 * Cs)
    cols = F.pad(cols, (0, STEM_KPAD - 9 * Cs))
    dcols = rnd(N, H * W, STEM_KPAD, seed=W)
    want, = torch.autograd.grad((cols * dcols.double()).sum(), x)
    dx = torch.full((N, 3, H, W), float("nan"), device="cuda")
    op("vd_op_stem_col2im", dev(dcols), dev(obs.view(N)), dev(lat.view(N)), dev(km.view(N)), N, H, W, mode, dx)
    got = dx.cpu().view(B, T, 3, H, W)
    report("stem_col2im", rel_err(got, want))
    close(got, want, atol=3.5e-7 * float(want.abs().max()), rtol=3.5e-7)
    if mode != 2:
        assert float(got[:, 1].abs().max()) == 0.0                    # an observed frame's x never reaches the network


# ---------------------------------------------------------------------------------------------------- guided steps on the engine
def engine(cfg):
    key = json.dumps(cfg, sort_keys=True)
    if key not in _cache:
        model, diff = vda.create_video_model_and_diffusion(**{k: cfg[k] for k in KEYS})
        sd = synth_sd(model.param_specs())
        model.load_state_dict(sd)
        model.to("cuda")
        model.eval()
        _cache[key] = (model, diff, sd)
    return _cache[key]


def oracle(cfg):
    model, diff, sd = engine(cfg)
    sched = ScheduleRef(cfg["diffusion_steps"], cfg["noise_schedule"], cfg["timestep_respacing"], cfg["sigma_small"],
                        cfg["rescale_timesteps"])
    return model, diff, SamplerRef(sched, UNetRef(cfg, sd))


def cfg_of(T, **over):
    return {**vda.video_model_and_diffusion_defaults(), **dict(T=T, image_size=32, num_channels=64, num_res_blocks=1, rp_alpha=T,
                                                               rp_beta=T, rp_gamma=T, timestep_respacing="ddim50"), **over}


def window(B, T, S, n_obs, seed, pad=None, km=None):
    """n_obs observed frames first; pad: per item, the frame indices that are padding (in no mask); km: kinda-marginal frames."""
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(B, T, 3, S, S, generator=g) * 2 - 1
    x0[:, n_obs:] = 0
    x = torch.randn(B, T, 3, S, S, generator=g)
    obs = torch.zeros(B, T, 1, 1, 1)
    obs[:, :n_obs] = 1
    lat = 1 - obs
    kmm = torch.zeros(B, T, 1, 1, 1)
    for b, idx in enumerate(pad or []):
        lat[b, idx] = 0
    for b, idx in enumerate(km or []):
        lat[b, idx] = 0
        kmm[b, idx] = 1
    return dict(x=x, x0=x0, obs_mask=obs, latent_mask=lat, kinda_marg_mask=kmm,
                frame_indices=torch.arange(T).view(1, T).repeat(B, 1))


def guided_vs_oracle(cfg, c, t_val, clip=True, seed=5):
    """One guided p_sample on the engine against SamplerRef.guided_p_sample (autograd through the oracle), with the bound of
    test_use_gradient_method_vs_oracle_autograd.  Returns (engine result, oracle result)."""
    model, diff, ora = oracle(cfg)
    B = c["x"].shape[0]
    gen = torch.Generator().manual_seed(seed)
    n1, n2 = torch.randn(c["x"].shape, generator=gen), torch.randn(c["x"].shape, generator=gen)
    xtm1 = c["x0"] + 0.2 * torch.randn(c["x"].shape, generator=gen) * c["obs_mask"]
    t = torch.tensor([t_val] * B)
    kwo = dict(x0=c["x0"], obs_mask=c["obs_mask"], latent_mask=c["latent_mask"], kinda_marg_mask=c["kinda_marg_mask"],
               frame_indices=c["frame_indices"], x_t_minus_1=xtm1)
    want = ora.guided_p_sample(c["x"], t, kwo, n1, n2, clip=clip)
    kw = {k: v.cuda() for k, v in kwo.items()}
    kw["observed_frames"] = "x_0"
    got = diff._guided(model, c["x"].cuda(), t.cuda(), clip, kw, noise2=n2, want_sample=True, _noise=n1)
    scale = float(want["grad"].abs().max())
    assert scale > 0
    close(got["grad"].cpu(), want["grad"], atol=2e-4 * scale, rtol=1e-3)
    close(got["sample"].cpu(), want["sample"], atol=1e-3 * scale, rtol=1e-3)
    return got, want


# item 0: 4 padding frames at the tail; item 1: interleaved padding
PAD12 = [[8, 9, 10, 11], [4, 6, 9]]


@pytest.mark.parametrize("allow", [True, False])
def test_guided_step_with_padding_frames(allow):
    """B = 2, T = 12, 3 observed frames, padding frames in no mask: the -inf masking of attn_temporal_bwd and both
    allow_interactions_between_padding rules inside the whole backward."""
    cfg = cfg_of(12, allow_interactions_between_padding=allow)
    guided_vs_oracle(cfg, window(2, 12, 32, 3, seed=12, pad=PAD12), 30)


@pytest.mark.parametrize("B,T", [(1, 16), (2, 16), (1, 32), (2, 32)])
def test_guided_step_long_windows(B, T):
    """Windows up to the step's limit of 32 frames, with padding: the temporal backward kernels at T = 16 and 32."""
    pad = [[T - 3, T - 2, T - 1], list(range(T // 4 + 1, T, 4))][:B]
    guided_vs_oracle(cfg_of(T, num_channels=32), window(B, T, 32, T // 4, seed=T + B, pad=pad), 20)


@pytest.mark.parametrize("cond", ["duplicate", "t=0"])
def test_guided_step_conditioning_modes(cond):
    """stem_col2im's modes 1 and 2 inside the step (the stem reads 6 and 3 channels)."""
    cfg = cfg_of(8, cond_emb_type=cond)
    guided_vs_oracle(cfg, window(2, 6, 32, 2, seed=66, pad=[[5], []]), 30)


def test_guided_step_without_clipping():
    """clip_denoised=False at a t where the x_0 prediction leaves [-1, 1]: the gradient passes through every pixel.  Item 1 has
    kinda-marginal frames."""
    cfg = cfg_of(8)
    c = window(2, 8, 32, 2, seed=80, pad=[[7], []], km=[[], [5, 6]])
    got, want = guided_vs_oracle(cfg, c, 45, clip=False)
    assert float(want["pred_xstart"].abs().max()) > 1.0
    assert float(got["pred_xstart"].abs().max()) > 1.0


def test_guided_step_full_size_model():
    """The default 64x64 model (128 channels, num_res_blocks=2) on one MineRL-shaped window: B = 1, T = 20, 13 observed
    frames, 2 padding frames."""
    cfg = {**vda.video_model_and_diffusion_defaults(), **dict(T=20, image_size=64, rp_alpha=20, rp_beta=20, rp_gamma=20,
                                                              timestep_respacing="ddim50")}
    assert cfg["num_channels"] == 128 and cfg["num_res_blocks"] == 2
    guided_vs_oracle(cfg, window(1, 20, 64, 13, seed=20, pad=[[18, 19]]), 25)


def test_guided_step_with_no_observed_frame_has_zero_gradient():
    """obs_mask all zero: the loss is 0, so the gradient is exactly zero (grad_rescale's m = 0 branch) and the step equals the
    oracle's."""
    cfg = cfg_of(8)
    c = window(2, 6, 32, 0, seed=60, pad=[[5], []])
    model, diff, ora = oracle(cfg)
    gen = torch.Generator().manual_seed(5)
    n1, n2 = torch.randn(c["x"].shape, generator=gen), torch.randn(c["x"].shape, generator=gen)
    t = torch.tensor([30, 30])
    kwo = dict(x0=c["x0"], obs_mask=c["obs_mask"], latent_mask=c["latent_mask"], kinda_marg_mask=c["kinda_marg_mask"],
               frame_indices=c["frame_indices"], x_t_minus_1=c["x0"])
    want = ora.guided_p_sample(c["x"], t, kwo, n1, n2)
    kw = {k: v.cuda() for k, v in kwo.items()}
    kw["observed_frames"] = "x_0"
    got = diff._guided(model, c["x"].cuda(), t.cuda(), True, kw, noise2=n2, want_sample=True, _noise=n1)
    assert float(got["grad"].abs().max()) == 0.0
    assert torch.isfinite(got["sample"]).all() and torch.isfinite(got["mean"]).all()
    close(got["sample"].cpu(), want["sample"], atol=ATOL, rtol=RTOL)


def test_guided_step_above_256_frames_is_refused():
    """B * T = 288 (B = 9, T = 32) is refused with the limit in the message; a guided step of an ordinary window still
    works afterwards."""
    cfg = cfg_of(32, num_channels=32)
    model, diff, _ = engine(cfg)
    c = window(9, 32, 32, 4, seed=9)
    kw = {k: c[k].cuda() for k in ("x0", "obs_mask", "latent_mask", "kinda_marg_mask", "frame_indices")}
    kw.update(x_t_minus_1=kw["x0"], observed_frames="x_0")
    with pytest.raises(_lib.VdError, match="256"):
        diff._guided(model, c["x"].cuda(), torch.tensor([20] * 9, device="cuda"), True, kw)
    guided_vs_oracle(cfg, window(2, 32, 32, 8, seed=32, pad=[[31], [3, 17]]), 20)
