"""A plain-torch fp64 restatement of the I3D video embedding and of the reference's Frechet distance -- the yardstick of the FVD tests.

The reference embeds videos with the TF-Hub module deepmind/i3d-kinetics-400/1 through tensorflow
(improved_diffusion/frechet_video_distance.py:38-133); neither tensorflow nor the module's weights exist where these tests run, so
parity with the module itself cannot be pinned by a fixture.  This file restates the published network -- Inception-v1 inflated to
3-D: Unit3D = conv3d without bias -> BatchNorm (inference, eps 1e-3) -> ReLU, TF `SAME` padding, the layer table below -- with CPU
`F.conv3d` / `F.max_pool3d` in float64, explicit pads and the BatchNorm un-folded, the TF1 `resize_bilinear` of `preprocess`, and the
lines of `fid_features_to_metric` (:142-203) with `scipy.linalg.sqrtm`; it is what the HIP path is held to.
"""
import numpy as np
import torch
import torch.nn.functional as F

BN_EPS = 1e-3
MIXED = (("Mixed_3b", 192, (64, 96, 128, 16, 32, 32)), ("Mixed_3c", 256, (128, 128, 192, 32, 96, 64)),
         ("Mixed_4b", 480, (192, 96, 208, 16, 48, 64)), ("Mixed_4c", 512, (160, 112, 224, 24, 64, 64)),
         ("Mixed_4d", 512, (128, 128, 256, 24, 64, 64)), ("Mixed_4e", 512, (112, 144, 288, 32, 64, 64)),
         ("Mixed_4f", 528, (256, 160, 320, 32, 128, 128)), ("Mixed_5b", 832, (256, 160, 320, 32, 128, 128)),
         ("Mixed_5c", 832, (384, 192, 384, 48, 128, 128)))


def unit_shapes():
    """[(unit, (Cout, Cin, k, k, k))] of the 57 Unit3D convolutions."""
    u = [("Conv3d_1a_7x7", (64, 3, 7, 7, 7)), ("Conv3d_2b_1x1", (64, 64, 1, 1, 1)), ("Conv3d_2c_3x3", (192, 64, 3, 3, 3))]
    for name, cin, o in MIXED:
        u += [(f"{name}.b0", (o[0], cin, 1, 1, 1)), (f"{name}.b1a", (o[1], cin, 1, 1, 1)), (f"{name}.b1b", (o[2], o[1], 3, 3, 3)),
              (f"{name}.b2a", (o[3], cin, 1, 1, 1)), (f"{name}.b2b", (o[4], o[3], 3, 3, 3)), (f"{name}.b3b", (o[5], cin, 1, 1, 1))]
    return u


def synth_state_dict(seed=0, bn_weight=True):
    """Seeded synthetic weights in the key layout of the PyTorch port: He-scaled convs, BatchNorm weight and running_var in [0.5, 1.5],
    small bias and running_mean, and a num_batches_tracked per BatchNorm as a real state dict has."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for unit, shape in unit_shapes():
        fan_in = shape[1] * shape[2] * shape[3] * shape[4]
        sd[f"{unit}.conv3d.weight"] = torch.randn(*shape, generator=g) * (2.0 / fan_in) ** 0.5
        if bn_weight:
            sd[f"{unit}.bn.weight"] = torch.rand(shape[0], generator=g) + 0.5
        sd[f"{unit}.bn.bias"] = torch.randn(shape[0], generator=g) * 0.05
        sd[f"{unit}.bn.running_mean"] = torch.randn(shape[0], generator=g) * 0.05
        sd[f"{unit}.bn.running_var"] = torch.rand(shape[0], generator=g) + 0.5
        sd[f"{unit}.bn.num_batches_tracked"] = torch.tensor(0)
    sd["logits.conv3d.weight"] = torch.randn(400, 1024, 1, 1, 1, generator=g) * (2.0 / 1024) ** 0.5
    sd["logits.conv3d.bias"] = torch.randn(400, generator=g) * 0.05
    return sd


def same_pads(size, k, s):
    """(output size, pad before, pad behind) of one axis under TF's SAME rule."""
    if size % s == 0:
        total = max(k - s, 0)
    else:
        total = max(k - size % s, 0)
    return (size + s - 1) // s, total // 2, total - total // 2


def pad_same(x, kernel, stride, value=0.0):
    """x (N, C, T, H, W) padded for a SAME window op with `kernel` / `stride` given as (t, h, w)."""
    pads = []
    for size, k, s in zip(reversed(x.shape[2:]), reversed(kernel), reversed(stride)):     # F.pad counts from the last axis
        _, before, behind = same_pads(size, k, s)
        pads += [before, behind]
    return F.pad(x, pads, value=value)


def conv3d_same(x, w, stride=(1, 1, 1), bias=None):
    return F.conv3d(pad_same(x, tuple(w.shape[2:]), stride), w, bias, stride=stride)


def maxpool3d_same(x, kernel, stride):
    """TF's SAME max pool: the padding never wins (-inf)."""
    return F.max_pool3d(pad_same(x, kernel, stride, value=float("-inf")), kernel, stride)


def resize_bilinear_tf1(frames_u8, size=224):
    """frames (T, 3, H, W) uint8 -> (T, size, size, 3) float64 in [-1, 1]: tf.image.resize_bilinear of TF1 with its defaults
    (align_corners=False, no half-pixel centres), then 2 x / 255 - 1.  `scale` and the source coordinate are taken in float32 as TF
    does, so the source pixels and weights are TF's; the interpolation itself runs in float64."""
    x = torch.as_tensor(frames_u8).to(torch.float64)
    T, C, H, W = x.shape

    def axis(n_in):
        scale = np.float32(n_in) / np.float32(size)
        src = np.arange(size, dtype=np.float32) * scale                      # float32 product
        lo = np.floor(src)
        hi = np.minimum(lo + 1, n_in - 1)
        return torch.from_numpy(lo.astype(np.int64)), torch.from_numpy(hi.astype(np.int64)), torch.from_numpy((src - lo).astype(np.float64))
    y0, y1, yl = axis(H)
    x0, x1, xl = axis(W)
    rows0, rows1 = x[:, :, y0, :], x[:, :, y1, :]
    top = rows0[..., x0] + (rows0[..., x1] - rows0[..., x0]) * xl
    bot = rows1[..., x0] + (rows1[..., x1] - rows1[..., x0]) * xl
    out = top + (bot - top) * yl.view(-1, 1)
    return (2 * out / 255 - 1).permute(0, 2, 3, 1).contiguous()


def _unit(x, sd, name, stride=(1, 1, 1)):
    w = sd[f"{name}.conv3d.weight"].to(x.dtype)
    y = conv3d_same(x, w, stride)
    gamma = sd.get(f"{name}.bn.weight")
    gamma = torch.ones(w.shape[0], dtype=x.dtype) if gamma is None else gamma.to(x.dtype)
    y = F.batch_norm(y, sd[f"{name}.bn.running_mean"].to(x.dtype), sd[f"{name}.bn.running_var"].to(x.dtype),
                     gamma, sd[f"{name}.bn.bias"].to(x.dtype), training=False, eps=BN_EPS)
    return F.relu(y)


def embed_restated(video_u8, sd, dtype=torch.float64):
    """One video (T, 3, H, W) uint8 -> its 400 logits averaged over time, in `dtype` (float64: the yardstick; float32: what a plain
    torch run on the CPU costs, tools/fvd_bench.py)."""
    x = resize_bilinear_tf1(video_u8).permute(3, 0, 1, 2).unsqueeze(0).to(dtype)        # (1, 3, T, 224, 224)
    x = _unit(x, sd, "Conv3d_1a_7x7", (2, 2, 2))
    x = maxpool3d_same(x, (1, 3, 3), (1, 2, 2))
    x = _unit(x, sd, "Conv3d_2b_1x1")
    x = _unit(x, sd, "Conv3d_2c_3x3")
    x = maxpool3d_same(x, (1, 3, 3), (1, 2, 2))
    for name, cin, _ in MIXED:
        if name == "Mixed_4b":
            x = maxpool3d_same(x, (3, 3, 3), (2, 2, 2))
        if name == "Mixed_5b":
            x = maxpool3d_same(x, (2, 2, 2), (2, 2, 2))
        assert x.shape[1] == cin, (name, x.shape)
        x = torch.cat([_unit(x, sd, f"{name}.b0"),
                       _unit(_unit(x, sd, f"{name}.b1a"), sd, f"{name}.b1b"),
                       _unit(_unit(x, sd, f"{name}.b2a"), sd, f"{name}.b2b"),
                       _unit(maxpool3d_same(x, (3, 3, 3), (1, 1, 1)), sd, f"{name}.b3b")], dim=1)
    assert tuple(x.shape[1:]) == (1024, x.shape[2], 7, 7) and x.shape[2] >= 2, x.shape
    x = F.avg_pool3d(x, (2, 7, 7), stride=(1, 1, 1))
    x = F.conv3d(x, sd["logits.conv3d.weight"].to(dtype), sd["logits.conv3d.bias"].to(dtype))
    return x.reshape(400, -1).mean(dim=1)


def frechet_restated(features_1, features_2):
    """fid_features_to_metric (:142-203): mean and np.cov of each set, the matrix square root of the covariances' product by
    scipy.linalg.sqrtm (with the reference's retry on a non-finite result and its real part), and the closed form."""
    import scipy.linalg
    mu1, mu2 = np.mean(features_1, axis=0), np.mean(features_2, axis=0)
    s1, s2 = np.atleast_2d(np.cov(features_1, rowvar=False)), np.atleast_2d(np.cov(features_2, rowvar=False))
    root = scipy.linalg.sqrtm(s1.dot(s2), disp=False)[0]
    if not np.isfinite(root).all():
        eye = np.eye(s1.shape[0]) * 1e-6
        root = scipy.linalg.sqrtm((s1 + eye).dot(s2 + eye))
    if np.iscomplexobj(root):
        assert np.allclose(np.diagonal(root).imag, 0, atol=1e-3)
        root = root.real
    d = mu1 - mu2
    return float(d.dot(d) + np.trace(s1) + np.trace(s2) - 2 * np.trace(root))
