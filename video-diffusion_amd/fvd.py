"""Frechet video distance: the I3D video embedder on the GPU (csrc/i3d.hip) and the Frechet distance of two feature sets on the host.

`I3D` is what `create_id3_embedding(preprocess(videos, (224, 224)))` is to the reference (improved_diffusion/frechet_video_distance.py:38-133):
the TF-Hub module deepmind/i3d-kinetics-400/1 -- Inception-v1 inflated to 3-D, trained on Kinetics-400 RGB -- read at its output
RGB/inception_i3d/Mean:0, the 400 logits averaged over time.  `frechet_distance` is `fid_features_to_metric` (:142-203).

The pretrained weights do not ship and are never fetched.  `from_files` reads them from the user's own file, in the key layout of the
widely used PyTorch port of the network (the `i3d_pretrained_400.pt` that FVD code for PyTorch carries):
  <unit>.conv3d.weight [Cout][Cin][kt][kh][kw], <unit>.bn.{weight,bias,running_mean,running_var} (a missing bn.weight means 1: the TF
  module has no scale), logits.conv3d.{weight,bias}; <unit> = Conv3d_1a_7x7, Conv3d_2b_1x1, Conv3d_2c_3x3,
  Mixed_{3b,3c,4b,4c,4d,4e,4f,5b,5c}.{b0,b1a,b1b,b2a,b2b,b3b}; num_batches_tracked is ignored.
The BatchNorm (inference, eps 1e-3) is folded into weight and bias once at load, in float64, then rounded to float32.
"""
import ctypes

import numpy as np
import torch

from . import _lib

BN_EPS = 1e-3
SIDE = 224
NUM_CLASSES = 400
MIN_FRAMES = 9
MIXED = (("Mixed_3b", 192, (64, 96, 128, 16, 32, 32)), ("Mixed_3c", 256, (128, 128, 192, 32, 96, 64)),
         ("Mixed_4b", 480, (192, 96, 208, 16, 48, 64)), ("Mixed_4c", 512, (160, 112, 224, 24, 64, 64)),
         ("Mixed_4d", 512, (128, 128, 256, 24, 64, 64)), ("Mixed_4e", 512, (112, 144, 288, 32, 64, 64)),
         ("Mixed_4f", 528, (256, 160, 320, 32, 128, 128)), ("Mixed_5b", 832, (256, 160, 320, 32, 128, 128)),
         ("Mixed_5c", 832, (384, 192, 384, 48, 128, 128)))


def _units():
    u = [("Conv3d_1a_7x7", 3, 64, 7), ("Conv3d_2b_1x1", 64, 64, 1), ("Conv3d_2c_3x3", 64, 192, 3)]
    for name, cin, o in MIXED:
        u += [(f"{name}.b0", cin, o[0], 1), (f"{name}.b1a", cin, o[1], 1), (f"{name}.b1b", o[1], o[2], 3),
              (f"{name}.b2a", cin, o[3], 1), (f"{name}.b2b", o[3], o[4], 3), (f"{name}.b3b", cin, o[5], 1)]
    return tuple(u)


UNITS = _units()         # (unit, Cin, Cout, cubic kernel size), in the order the network runs them
KEY_LAYOUT = ("the state dict of the PyTorch port of I3D (i3d_pretrained_400.pt): <unit>.conv3d.weight, "
              "<unit>.bn.{weight,bias,running_mean,running_var} for Conv3d_1a_7x7, Conv3d_2b_1x1, Conv3d_2c_3x3 and "
              "Mixed_{3b..5c}.{b0,b1a,b1b,b2a,b2b,b3b}, and logits.conv3d.{weight,bias}")


def same_pad(size, k, s):
    """TF's SAME padding of one axis: (output size, padding before, padding behind).  The total is max(k - s, 0) when the stride
    divides the size and max(k - size % s, 0) otherwise; the smaller half goes in front."""
    total = max(k - s, 0) if size % s == 0 else max(k - size % s, 0)
    return -(-size // s), total // 2, total - total // 2


def max_frames():
    return int(_lib.lib().vd_i3d_max_frames())


def time_positions(T):
    """Number of positions the time mean of the logits runs over for a T-frame video: ceil(ceil(ceil(T/2)/2)/2) - 1 (the three
    stride-2 stages, then the 2-frame average pool).  ValueError for T < 9, where it would be 0."""
    if T < MIN_FRAMES:
        raise ValueError(f"I3D needs videos of at least {MIN_FRAMES} frames, got {T}: after its three stride-2 stages the 2-frame "
                         "average pool would have nothing to average")
    t = T
    for _ in range(3):
        t = -(-t // 2)
    return t - 1


def frechet_distance(features_1, features_2):
    """|mu1 - mu2|^2 + tr(sigma1) + tr(sigma2) - 2 tr sqrt(sigma1 sigma2) of two feature sets (videos, D), float64.  The last term is the
    sum of the square roots of the eigenvalues of r sigma2 r, r = sigma1^(1/2) from `eigh`: the same eigenvalues as sigma1 sigma2,
    from a symmetric positive semi-definite matrix, so it is finite for singular covariances too (fewer videos than dimensions)."""
    f1, f2 = np.asarray(features_1, dtype=np.float64), np.asarray(features_2, dtype=np.float64)
    if f1.ndim != 2 or f2.ndim != 2 or f1.shape[1] != f2.shape[1]:
        raise ValueError(f"frechet_distance: two (videos, D) feature sets of one D, got {f1.shape} and {f2.shape}")
    if f1.shape[0] < 2 or f2.shape[0] < 2:
        raise ValueError(f"frechet_distance needs at least 2 videos per side for a covariance, got {f1.shape[0]} and {f2.shape[0]}")
    mu1, mu2 = f1.mean(axis=0), f2.mean(axis=0)
    s1, s2 = np.atleast_2d(np.cov(f1, rowvar=False)), np.atleast_2d(np.cov(f2, rowvar=False))
    ev, q = np.linalg.eigh(s1)
    r = (q * np.sqrt(np.clip(ev, 0, None))) @ q.T
    m = r @ s2 @ r
    lam = np.linalg.eigvalsh((m + m.T) / 2)
    diff = mu1 - mu2
    return float(diff @ diff + np.trace(s1) + np.trace(s2) - 2 * np.sqrt(np.clip(lam, 0, None)).sum())


def canonical_weights(sd):
    """A state dict in the layout above -> {"<unit>.weight", "<unit>.bias", "logits.weight", "logits.bias"} as float32 numpy arrays with
    the BatchNorm folded in (float64, rounded once).  ValueError names what is missing, misshapen, non-finite or negative."""
    def get(key, want, optional=False):
        if key not in sd:
            if optional:
                return None
            raise ValueError(f"I3D weights: missing key {key}; expected {KEY_LAYOUT}")
        t = torch.as_tensor(sd[key]).detach()
        if tuple(t.shape) != tuple(want):
            raise ValueError(f"I3D weights: {key} has shape {tuple(t.shape)}, expected {tuple(want)}")
        a = t.to(torch.float64).numpy()
        if not np.isfinite(a).all():
            raise ValueError(f"I3D weights: {key} holds non-finite values")
        return a
    out = {}
    for unit, cin, cout, k in UNITS:
        w = get(f"{unit}.conv3d.weight", (cout, cin, k, k, k))
        gamma = get(f"{unit}.bn.weight", (cout,), optional=True)
        beta, mean = get(f"{unit}.bn.bias", (cout,)), get(f"{unit}.bn.running_mean", (cout,))
        var = get(f"{unit}.bn.running_var", (cout,))
        if (var < 0).any():
            raise ValueError(f"I3D weights: {unit}.bn.running_var has negative entries")
        scale = (1.0 if gamma is None else gamma) / np.sqrt(var + BN_EPS)
        out[f"{unit}.weight"] = np.ascontiguousarray((w * scale[:, None, None, None, None]).astype(np.float32))
        out[f"{unit}.bias"] = np.ascontiguousarray((beta - mean * scale).astype(np.float32))
    out["logits.weight"] = np.ascontiguousarray(get("logits.conv3d.weight", (NUM_CLASSES, 1024, 1, 1, 1)).astype(np.float32))
    out["logits.bias"] = np.ascontiguousarray(get("logits.conv3d.bias", (NUM_CLASSES,)).astype(np.float32))
    return out


def read_weights(path):
    from .lpips import _load_dict
    return canonical_weights(_load_dict(path))


class I3D:
    """The I3D video embedder of the Frechet video distance on one GPU."""

    def __init__(self, weights, device=None):
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise ValueError("I3D runs on a GPU device")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        L = _lib.lib()
        h = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(L.vd_i3d_create(ctypes.byref(h)))
            self._h = h
            for name, a in weights.items():
                a = np.ascontiguousarray(a, dtype=np.float32)
                _lib.check(L.vd_i3d_load_weight(h, name.encode(), a.ctypes.data_as(ctypes.c_void_p), a.nbytes))

    @classmethod
    def from_files(cls, path, device=None):
        return cls(read_weights(path), device)

    @classmethod
    def from_state_dict(cls, sd, device=None):
        return cls(canonical_weights(sd), device)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and _lib._lib is not None:
            _lib.lib().vd_i3d_destroy(h)
            self._h = None

    def embed(self, videos_u8):
        """videos (N, T, 3, H, W) uint8 (any device; numpy accepted) -> (N, 400) float32 on self.device.  9 <= T <= max_frames()."""
        v = torch.as_tensor(videos_u8)
        if v.dtype != torch.uint8 or v.ndim != 5 or v.shape[2] != 3:
            raise ValueError(f"I3D.embed: uint8 videos (N, T, 3, H, W), got {v.dtype} {tuple(v.shape)}")
        v = v.to(self.device).contiguous()
        N, T, _, H, W = v.shape
        out = torch.empty(N, NUM_CLASSES, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().vd_i3d_embed(self._h, N, T, H, W, _lib.ptr(v), _lib.ptr(out), _lib.current_stream()))
        return out


def conv_flops(T):
    """Floating-point operations (2 per multiply-add) of the 57 convolutions and the logits layer for one T-frame video, from the shapes."""
    t, hw, total, i = T, SIDE, 0, 0

    def unit(stride=1):
        nonlocal total, i, t, hw
        _, cin, cout, k = UNITS[i]
        i += 1
        to, ho = same_pad(t, k, stride)[0], same_pad(hw, k, stride)[0]
        total += 2 * to * ho * ho * cout * cin * k ** 3
        return to, ho
    t, hw = unit(2)
    hw = same_pad(hw, 3, 2)[0]
    unit()
    unit()
    hw = same_pad(hw, 3, 2)[0]
    for b in range(9):
        if b == 2:
            t, hw = same_pad(t, 3, 2)[0], same_pad(hw, 3, 2)[0]
        if b == 7:
            t, hw = same_pad(t, 2, 2)[0], same_pad(hw, 2, 2)[0]
        for _ in range(6):
            unit()
    return total + 2 * 1024 * NUM_CLASSES


assert len(UNITS) == 57
