"""A plain-torch fp64 restatement of the reference's LPIPS frame embedding and farthest-point selection -- the yardstick of the
LPIPS tests.

The reference embeds frames with `LpipsEmbedder` (improved_diffusion/inference_util.py:15-31), a subclass of the pip package
`lpips.LPIPS(net='alex', spatial=False)`: ScalingLayer -> torchvision AlexNet feature slices (conv1 + ReLU | maxpool, conv2 + ReLU |
maxpool, conv3 + ReLU | conv4 + ReLU | conv5 + ReLU) -> per tap `normalize_tensor` (channel L2 norm + 1e-10), `scale_by_proj_weights`
(sqrt of the lin weight) and `not_spatial_average` (flatten, / sqrt(h*w)), concatenated.  Neither `lpips` nor `torchvision` is
installed where these tests run, so parity with the package itself cannot be pinned by a fixture; this file restates those lines
with CPU `F.conv2d` / `F.max_pool2d` in float64 and is what the HIP path is held to.  `select_restated` is the loop of
`select_obs_indices` (:157-185).
"""
import numpy as np
import torch
import torch.nn.functional as F

CONV_SHAPES = ((64, 3, 11, 11), (192, 64, 5, 5), (384, 192, 3, 3), (256, 384, 3, 3), (256, 256, 3, 3))
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)


def synth_weights(seed=0, lin_zero_frac=0.1):
    """Seeded synthetic LPIPS weights in the canonical names: He-scaled convs, small biases, non-negative lin weights (a few
    exact zeros, as trained lin layers have)."""
    g = torch.Generator().manual_seed(seed)
    w = {}
    for k, (o, i, kh, kw) in enumerate(CONV_SHAPES):
        w[f"conv{k + 1}.weight"] = torch.randn(o, i, kh, kw, generator=g) * (2.0 / (i * kh * kw)) ** 0.5
        w[f"conv{k + 1}.bias"] = torch.randn(o, generator=g) * 0.05
        lin = torch.rand(o, generator=g) * 0.2
        lin[torch.rand(o, generator=g) < lin_zero_frac] = 0
        w[f"lin{k + 1}"] = lin
    return w


def taps_restated(frames, w, shift=SHIFT, scale=SCALE):
    """frames (N, 3, H, W) -> the five ReLU feature maps (fp64), as lpips' alexnet.forward returns them."""
    x = frames.to(torch.float64)
    sh = torch.tensor(shift, dtype=torch.float64).view(1, 3, 1, 1)
    sc = torch.tensor(scale, dtype=torch.float64).view(1, 3, 1, 1)
    h = (x - sh) / sc                                                     # ScalingLayer (zero padding of conv1 after it)
    d = {k: v.to(torch.float64) for k, v in w.items()}
    h = F.relu(F.conv2d(h, d["conv1.weight"], d["conv1.bias"], stride=4, padding=2))
    t1 = h
    h = F.relu(F.conv2d(F.max_pool2d(h, 3, 2), d["conv2.weight"], d["conv2.bias"], padding=2))
    t2 = h
    h = F.relu(F.conv2d(F.max_pool2d(h, 3, 2), d["conv3.weight"], d["conv3.bias"], padding=1))
    t3 = h
    h = F.relu(F.conv2d(h, d["conv4.weight"], d["conv4.bias"], padding=1))
    t4 = h
    h = F.relu(F.conv2d(h, d["conv5.weight"], d["conv5.bias"], padding=1))
    return [t1, t2, t3, t4, h]


def embed_parts_restated(frames, w, **kw):
    """The five per-tap embedding pieces (N, C_k*h_k*w_k), fp64."""
    parts = []
    for k, a in enumerate(taps_restated(frames, w, **kw)):
        N, C, H, W = a.shape
        f = a / (torch.sqrt(torch.sum(a ** 2, dim=1, keepdim=True)) + 1e-10)      # lpips.normalize_tensor
        e = (w[f"lin{k + 1}"].to(torch.float64).view(1, C, 1, 1) ** 0.5) * f         # scale_by_proj_weights
        parts.append(e.reshape(N, C * H * W) / (H * W) ** 0.5)                      # not_spatial_average
    return parts


def embed_restated(frames, w, **kw):
    """LpipsEmbedder.forward: (N, 3, H, W) -> (N, D, 1, 1), fp64."""
    e = torch.cat(embed_parts_restated(frames, w, **kw), dim=1)
    return e.reshape(e.shape[0], -1, 1, 1)


def dim_restated(H, W):
    return embed_restated(torch.zeros(1, 3, H, W), synth_weights(0)).shape[1]


def select_restated(embs, n, always_selected=(0,)):
    """select_obs_indices (:157-185) on embs (B, n_cand, ...): candidate indices per item."""
    out = []
    for b in range(embs.shape[0]):
        nearest = [np.inf] * embs.shape[1]
        newest = always_selected[0]
        picked = [newest]
        for i in range(1, n):
            for f in range(len(nearest)):
                d = float(((embs[b, newest] - embs[b, f]) ** 2).sum())
                nearest[f] = min(nearest[f], d)
            newest = always_selected[i] if i < len(always_selected) else int(np.argmax(nearest))
            picked.append(newest)
        out.append(picked)
    return out


def class_embedder(w):
    """A host callable for `inference_util.set_lpips_embedder`: the restatement in fp64 (the host loop then runs in fp64)."""
    def fn(frames):
        return embed_restated(frames.cpu(), w)
    return fn
