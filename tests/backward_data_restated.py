"""Plain torch-CPU float64 statements of what lies between the kernels of the backward-data pass (csrc/engine.hip: backward()), each as
the GRADIENT OF THE PLAIN FORWARD: torch.autograd.grad of F.conv2d / x @ w.T / the im2col product with respect to the input.  None of
them takes the rotated or transposed kernel as given; the composed forms the engine runs (zero-stuff + stride-1 conv with the rotated
kernel, conv + 2x2 sums) are stated separately and held to them in tests/test_backward_data_cpu.py.  Activations are NHWC, weights as
the checkpoint stores them (OIHW, [O][I]).  Not a test file.

    conv_bwd / linear_bwd / stem_bwd      autograd gradients with respect to the layer's input (the stem: to its im2col matrix)
    rotated / zero_stuff2 / sumpool2      the pieces of the composed forms; down_bwd_composed / up_bwd_composed put them together
    bwd_weight                            the backward operator's own weight, torch-made: S and the float32 evaluation need it
    guided_grad / guided_final            gaussian_diffusion.py:319-364 as oracle/sampler_ref.py states them, autograd for the gradients
    guided_grad_f32 / guided_final_f32    the same expressions evaluated in float32 torch
    grad_rescale                          the power-of-two scale of launch_grad_rescale in exact arithmetic
"""
import math

import torch
import torch.nn.functional as F

F64 = torch.float64
STEM_KPAD = 64


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def conv_bwd(dy, w, H, stride=1, ups=0):
    """d/dx of F.conv2d(up(x), w, stride, padding=1) against the cotangent dy [N][Ho][Wo][O]; x [N][H][H][I] -> [N][H][H][I] float64.
    ups: x is read through a nearest x2 upsample (the Upsample layer)."""
    N, I = dy.shape[0], w.shape[1]
    x = torch.zeros(N, I, H, H, dtype=F64, requires_grad=True)
    src = F.interpolate(x, scale_factor=2, mode="nearest") if ups else x
    y = F.conv2d(src, w.to(F64), stride=stride, padding=(w.shape[2] - 1) // 2)
    g, = torch.autograd.grad(y, x, _nchw(dy.to(F64)))
    return _nhwc(g)


def linear_bwd(dy, w):
    """d/dx of x @ w.T: dy [M][O], w [O][I] -> [M][I]."""
    x = torch.zeros(dy.shape[0], w.shape[1], dtype=F64, requires_grad=True)
    g, = torch.autograd.grad(x @ w.to(F64).t(), x, dy.to(F64))
    return g


def stem_matrix(w):
    """The stem as its im2col product: lin[o][k = tap * I + i] = w[o][i][tap], padded with zero columns to STEM_KPAD."""
    O, I = w.shape[:2]
    lin = w.to(F64).permute(0, 2, 3, 1).reshape(O, 9 * I)
    return F.pad(lin, (0, STEM_KPAD - 9 * I))


def stem_bwd(dy, w):
    """d/dcols of cols @ lin.T, cols the [M][STEM_KPAD] im2col matrix of the network input: dy [M][O] -> [M][STEM_KPAD]."""
    cols = torch.zeros(dy.shape[0], STEM_KPAD, dtype=F64, requires_grad=True)
    g, = torch.autograd.grad(cols @ stem_matrix(w).t(), cols, dy.to(F64))
    return g


# ---- the composed forms
def rotated(w):
    """w'[i][o][ky][kx] = w[o][i][2 - ky][2 - kx]."""
    return w.flip(2, 3).transpose(0, 1).contiguous()


def zero_stuff2(x):
    """y[n][2 oy][2 ox][c] = x[n][oy][ox][c], zero elsewhere."""
    N, Ho, Wo, C = x.shape
    y = torch.zeros(N, 2 * Ho, 2 * Wo, C, dtype=x.dtype)
    y[:, ::2, ::2] = x
    return y


def sumpool2(x, y=None):
    """((b00 + b01) + b10) + b11 of every 2x2 block, then + y: the kernel's written order, in x's dtype."""
    v = ((x[:, 0::2, 0::2] + x[:, 0::2, 1::2]) + x[:, 1::2, 0::2]) + x[:, 1::2, 1::2]
    return v if y is None else v + y


def conv_s1(x, w):
    """Stride-1 3x3 conv, zero padding 1, NHWC in and out."""
    return _nhwc(F.conv2d(_nchw(x.to(F64)), w.to(F64), padding=1))


def down_bwd_composed(dy, w):
    """Downsample (stride 2) backward as the engine runs it: stride-1 conv of the zero-stuffed gradient with the rotated kernel."""
    return conv_s1(zero_stuff2(dy.to(F64)), rotated(w))


def up_bwd_composed(dy, w):
    """Upsample backward as the engine runs it: the conv's backward at 2H, then the 2x2 sums."""
    return sumpool2(conv_s1(dy, rotated(w)))


def bwd_weight(w, kind):
    """The weight of the backward operator as a forward layer, OIHW: linear W^T [I][O][1][1]; stem [STEM_KPAD][O][1][1]; conv rotated."""
    if kind == "linear":
        return w.reshape(w.shape[0], w.shape[1]).t().contiguous()[:, :, None, None]
    if kind == "stem":
        return stem_matrix(w).t().contiguous().to(w.dtype)[:, :, None, None]
    return rotated(w)


# ---- launch_grad_rescale
def grad_rescale(g):
    """(s, m): m = max |g| over the elements that are not NaN; s = 2^k with m s in [1, 2), k clamped to +-100; 1 for m = 0 or m >= 3e38."""
    a = g.abs()
    a = a[~torch.isnan(a)]
    m = float(a.max()) if a.numel() else 0.0
    if not (0.0 < m < 3.0e38):
        return 1.0, m
    _, ex = math.frexp(m)
    return math.ldexp(1.0, max(-100, min(100, 1 - ex))), m


# ---- the guidance formulas.  tab: name -> float32 row (step_nll_restated.tables + "al" = 1 - beta); t [B] in range; tensors [B][per]
def _rows(tab, t, dtype):
    return {k: torch.as_tensor(tab[k]).to(dtype)[t][:, None] for k in ("sr", "srm1", "c1", "c2", "lv", "al")}


def _guided_fwd(c, x, eps, noise, t, clip):
    x0r = c["sr"] * x - c["srm1"] * eps
    x0 = x0r.clamp(-1, 1) if clip else x0r
    mean = c["c1"] * x0 + c["c2"] * x
    nz = (t != 0).to(x.dtype)[:, None]
    return x0r, x0, mean, mean + nz * torch.exp(0.5 * c["lv"]) * noise


def guided_grad(tab, x, eps, noise, xtm1, obs_e, t, clip):
    """loss = sum(((mean + [t != 0] sigma z - x_t_minus_1) obs)^2); deps = d loss / d eps, dxd = d loss / d x with eps held (the part
    that does not pass through the network), by autograd in float64.  obs_e: the mask per element.  -> dict with x0r for the
    exclusion of the clip boundary."""
    c = _rows(tab, t, F64)
    x = x.to(F64).requires_grad_(True)
    eps = eps.to(F64).requires_grad_(True)
    x0r, x0, mean, smp = _guided_fwd(c, x, eps, noise.to(F64), t, clip)
    loss = (((smp - xtm1.to(F64)) * obs_e.to(F64)) ** 2).sum()
    deps, dxd = torch.autograd.grad(loss, [eps, x])
    return dict(deps=deps, dxd=dxd, mean=mean.detach(), xstart=x0.detach(), x0r=x0r.detach())


def guided_grad_f32(tab, x, eps, noise, xtm1, obs_e, t, clip):
    """The same quantities by the closed expressions in float32 torch: dmean = 2 (smp - xtm1) obs^2, dx0r = c1 dmean [|x0r| <= 1],
    deps = -srm1 dx0r, dxd = c2 dmean + sr dx0r."""
    f = torch.float32
    c = _rows(tab, t, f)
    x, eps = x.to(f), eps.to(f)
    x0r, x0, mean, smp = _guided_fwd(c, x, eps, noise.to(f), t, clip)
    dmean = 2.0 * (smp - xtm1.to(f)) * obs_e.to(f) * obs_e.to(f)
    dx0r = c["c1"] * dmean * (((x0r >= -1) & (x0r <= 1)).to(f) if clip else 1.0)
    return dict(deps=-c["srm1"] * dx0r, dxd=c["c2"] * dmean + c["sr"] * dx0r, mean=mean, xstart=x0)


def guided_grad_units(tab, x, eps, noise, xtm1, obs_e, t):
    """The absolute sum of every output's own terms (float64): what an error of one rounding is measured in."""
    c = _rows(tab, t, F64)
    x, eps = x.to(F64).abs(), eps.to(F64).abs()
    x0 = c["sr"] * x + c["srm1"] * eps
    mean = c["c1"] * x0 + c["c2"] * x
    nz = (t != 0).to(F64)[:, None]
    dmean = 2.0 * (mean + nz * torch.exp(0.5 * c["lv"]) * noise.to(F64).abs() + xtm1.to(F64).abs()) * obs_e.to(F64) ** 2
    dx0r = c["c1"] * dmean
    return dict(deps=c["srm1"] * dx0r, dxd=c["c2"] * dmean + c["sr"] * dx0r, mean=mean, xstart=x0)


def _final(c, dxd, mean, dx_net, inv_s, noise2, t):
    g = dxd + dx_net * inv_s
    m = mean - 10 * c["al"] * g / 2
    nz = (t != 0).to(dxd.dtype)[:, None]
    return g, m, m + nz * torch.exp(0.5 * c["lv"]) * noise2


def guided_final(tab, dxd, mean, dx_net, inv_s, noise2, t, dtype=F64):
    """grad = dxd + dx_net / s; mean' = mean - 10 alpha_t grad / 2; sample = mean' + [t != 0] sigma z2 -- in dtype."""
    g, m, s = _final(_rows(tab, t, dtype), dxd.to(dtype), mean.to(dtype), dx_net.to(dtype), inv_s, noise2.to(dtype), t)
    return dict(grad=g, mean_out=m, sample=s)


def guided_final_units(tab, dxd, mean, dx_net, inv_s, noise2, t):
    """The absolute sum of every output's own terms (float64)."""
    c = _rows(tab, t, F64)
    g = dxd.to(F64).abs() + dx_net.to(F64).abs() * abs(inv_s)
    m = mean.to(F64).abs() + 10 * c["al"] * g / 2
    nz = (t != 0).to(F64)[:, None]
    return dict(grad=g, mean_out=m, sample=m + nz * torch.exp(0.5 * c["lv"]) * noise2.to(F64).abs())
