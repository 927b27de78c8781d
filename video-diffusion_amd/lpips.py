"""LPIPS frame embedding and farthest-point frame selection on the GPU (csrc/lpips.hip) for the adaptive-* frame schedulers.

`LpipsAlex` is what `LpipsEmbedder(net='alex', spatial=False)` is to the reference (improved_diffusion/inference_util.py:15-31):
the AlexNet feature stack of the `lpips` package, each of its five taps unit-normalised over channels per pixel, scaled by the
square root of its lin weights and by 1 / sqrt(h*w), flattened and concatenated -> (N, D, 1, 1).  Its `select` is the farthest-point
loop of `select_obs_indices` (:157-185) with the distances, the running minimum and the argmax on the device.

The pretrained weights do not ship.  `from_files` reads them from what a user has:
  * one file with a whole `lpips.LPIPS(net='alex')` state dict (net.slice1.0.*, net.slice2.3.*, net.slice3.6.*, net.slice4.8.*,
    net.slice5.10.*, lin{k}.model.1.weight or lins.{k}.model.1.weight, optional scaling_layer.shift / .scale), or
  * torchvision's AlexNet checkpoint (features.{0,3,6,8,10}.*) plus lpips' weights/v0.1/alex.pth (lin{0..4}.model.1.weight), as
    two files or merged into one dict.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib

CHANNELS = (64, 192, 384, 256, 256)
CONV_SHAPES = ((64, 3, 11, 11), (192, 64, 5, 5), (384, 192, 3, 3), (256, 384, 3, 3), (256, 256, 3, 3))
FEATURE_INDEX = (0, 3, 6, 8, 10)          # torchvision alexnet.features index of conv k
SHIFT = (-0.030, -0.088, -0.188)           # lpips ScalingLayer
SCALE = (0.458, 0.448, 0.450)


def layer_sizes(H, W):
    """[(h_k, w_k)] of the five taps of an H x W frame: conv1 11x11/4 pad 2, maxpool 3/2, conv2 (same size), maxpool 3/2,
    conv3..5 (same size).  ValueError when some layer would be empty (torch would refuse the frame too)."""
    def conv1(s):
        return (s + 4 - 11) // 4 + 1 if s + 4 >= 11 else 0

    def pool(s):
        return (s - 3) // 2 + 1 if s >= 3 else 0
    h1, w1 = conv1(H), conv1(W)
    h2, w2 = pool(h1), pool(w1)
    h3, w3 = pool(h2), pool(w2)
    if min(h1, w1, h2, w2, h3, w3) < 1:
        raise ValueError(f"LPIPS: a {H}x{W} frame is too small for the AlexNet feature stack (a layer would be empty)")
    return [(h1, w1), (h2, w2), (h3, w3), (h3, w3), (h3, w3)]


def embedding_dim(H, W):
    """D of an H x W frame: sum over the taps of channels * h * w (31 872 at 64x64, 148 608 at 128x128)."""
    return sum(c * h * w for c, (h, w) in zip(CHANNELS, layer_sizes(H, W)))


def embed_chunk(H, W):
    """Frames of H x W that one pass of `vd_lpips_embed` takes (its workspace is bounded); a longer batch runs in several passes.
    Host only.  ValueError where the frame is too small for the feature stack."""
    n = int(_lib.lib().vd_lpips_embed_chunk(H, W))
    if n < 0:
        layer_sizes(H, W)
    return n


def _load_dict(path):
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
        sd = sd["state_dict"]
    if not isinstance(sd, dict):
        raise ValueError(f"LPIPS weights: {path} does not hold a state dict")
    return {k[7:] if k.startswith("module.") else k: v for k, v in sd.items()}


def canonical_weights(sd):
    """A state dict in any of the accepted layouts -> {"conv{k}.weight", "conv{k}.bias", "lin{k}", "shift", "scale"} as float32
    numpy arrays (k = 1..5), checked.  ValueError names what is missing, misshapen or negative."""
    def first(*keys):
        for k in keys:
            if k in sd:
                return k
        return None
    out, missing = {}, []
    for k in range(5):
        s, f = f"net.slice{k + 1}.{FEATURE_INDEX[k]}", f"features.{FEATURE_INDEX[k]}"
        for part in ("weight", "bias"):
            key = first(f"{s}.{part}", f"{f}.{part}")
            if key is None:
                missing.append(f"{s}.{part} | {f}.{part}")
            else:
                out[f"conv{k + 1}.{part}"] = (key, sd[key])
        key = first(f"lin{k}.model.1.weight", f"lins.{k}.model.1.weight")
        if key is None:
            missing.append(f"lin{k}.model.1.weight | lins.{k}.model.1.weight")
        else:
            out[f"lin{k + 1}"] = (key, sd[key])
    if missing:
        raise ValueError("LPIPS weights: missing keys (expected an lpips.LPIPS(net='alex') state dict, or torchvision AlexNet "
                         "features.{0,3,6,8,10}.* plus lpips v0.1 lin{0..4}.model.1.weight): " + ", ".join(missing))
    res = {}
    for k in range(5):
        for name, want in ((f"conv{k + 1}.weight", CONV_SHAPES[k]), (f"conv{k + 1}.bias", (CHANNELS[k],)),
                           (f"lin{k + 1}", (1, CHANNELS[k], 1, 1))):
            key, t = out[name]
            t = torch.as_tensor(t)
            if tuple(t.shape) != want and not (name.startswith("lin") and tuple(t.shape) == (CHANNELS[k],)):
                raise ValueError(f"LPIPS weights: {key} has shape {tuple(t.shape)}, expected {want}")
            a = t.detach().to(torch.float32).reshape(-1).numpy() if name.startswith("lin") else t.detach().to(torch.float32).numpy()
            if not np.isfinite(a).all():
                raise ValueError(f"LPIPS weights: {key} holds non-finite values")
            if name.startswith("lin") and (a < 0).any():
                raise ValueError(f"LPIPS weights: {key} has negative entries; the embedding scales by their square root "
                                 "(the reference would produce NaN distances)")
            res[name] = np.ascontiguousarray(a)
    for name, default in (("shift", SHIFT), ("scale", SCALE)):
        t = sd.get(f"scaling_layer.{name}")
        if t is None:
            res[name] = np.asarray(default, dtype=np.float32)
        else:
            t = torch.as_tensor(t)
            if t.numel() != 3:
                raise ValueError(f"LPIPS weights: scaling_layer.{name} has shape {tuple(t.shape)}, expected (1, 3, 1, 1)")
            res[name] = np.ascontiguousarray(t.detach().to(torch.float32).reshape(3).numpy())
    if (res["scale"] == 0).any():
        raise ValueError("LPIPS weights: scaling_layer.scale has a zero entry")
    return res


def read_weights(paths):
    """One path, two paths, or 'a,b': the file(s) merged into one dict, then `canonical_weights`."""
    if isinstance(paths, (str, os.PathLike)):
        paths = [p for p in str(paths).split(",") if p]
    sd = {}
    for p in paths:
        sd.update(_load_dict(p))
    return canonical_weights(sd)


class LpipsAlex:
    """The LPIPS (AlexNet) frame embedder of the adaptive-* schedulers on one GPU.  Build it with `from_files` (or from a
    state dict with `from_state_dict`), then register it: `inference_util.set_lpips_embedder(emb)` or
    `inference_util.load_lpips_weights(paths)`."""

    def __init__(self, weights, device=None):
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise ValueError("LpipsAlex runs on a GPU device")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        L = _lib.lib()
        h = ctypes.c_void_p()
        with torch.cuda.device(device):
            _lib.check(L.vd_lpips_create(ctypes.byref(h)))
            self._h = h
            for name, a in weights.items():
                a = np.ascontiguousarray(a, dtype=np.float32)
                _lib.check(L.vd_lpips_load_weight(h, name.encode(), a.ctypes.data_as(ctypes.c_void_p), a.nbytes))

    @classmethod
    def from_files(cls, paths, device=None):
        return cls(read_weights(paths), device)

    @classmethod
    def from_state_dict(cls, sd, device=None):
        return cls(canonical_weights(sd), device)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and _lib._lib is not None:
            _lib.lib().vd_lpips_destroy(h)
            self._h = None

    @staticmethod
    def dim(H, W):
        return embedding_dim(H, W)

    def _embed_device(self, frames):
        """frames (N, 3, H, W) float32 on self.device -> (N, D) on self.device."""
        N, C, H, W = frames.shape
        if C != 3:
            raise ValueError(f"LPIPS: frames need 3 channels, got {C}")
        D = embedding_dim(H, W)
        frames = frames.contiguous()
        out = torch.empty(N, D, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().vd_lpips_embed(self._h, N, H, W, _lib.ptr(frames), _lib.ptr(out), _lib.current_stream()))
        return out

    def __call__(self, frames):
        """frames (N, 3, H, W) in [-1, 1] (any device) -> (N, D, 1, 1) on self.device: LpipsEmbedder.forward."""
        x = frames.to(device=self.device, dtype=torch.float32)
        return self._embed_device(x).reshape(x.shape[0], -1, 1, 1)

    def distance(self, a, b, chunk=32):
        """LPIPS of frame pairs: a, b (N, 3, H, W) in [-1, 1] (any device) -> (N,) float64 numpy, `lpips.LPIPS(net='alex',
        spatial=False)(a, b)` of the reference's compute_lpips_lazy (scripts/video_eval.py:228-252).  The distance of two frames is the
        squared L2 distance of their embeddings: each tap of the embedding is the channel-normalised feature times sqrt(lin weight) and
        1 / sqrt(h w), so ||e(a) - e(b)||^2 = sum over taps of the spatial mean of sum_c w_c (n_a - n_b)^2.  Both sets are embedded `chunk`
        frames at a time (a 500-frame 128 x 128 video never holds 2 x 500 x 148 608 floats); a frame's embedding does not depend on
        its chunk, so neither does the result."""
        if tuple(a.shape) != tuple(b.shape):
            raise ValueError(f"LPIPS distance: shapes differ, {tuple(a.shape)} and {tuple(b.shape)}")
        if chunk < 1:
            raise ValueError("LPIPS distance: chunk >= 1")
        a = a.to(device=self.device, dtype=torch.float32)
        b = b.to(device=self.device, dtype=torch.float32)
        N = a.shape[0]
        out = torch.empty(N, dtype=torch.float64, device=self.device)
        for k in range(0, N, chunk):
            ea, eb = self._embed_device(a[k:k + chunk]), self._embed_device(b[k:k + chunk])
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().vd_pair_sqdist(ea.shape[0], ea.shape[1], _lib.ptr(ea), _lib.ptr(eb), _lib.ptr(out[k:k + chunk]),
                                                     _lib.current_stream()))
        return out.cpu().numpy()

    def embed(self, videos, indices):
        """videos (B, T, 3, H, W), indices: list of frame indices -> (B, len(indices), D) on self.device; the frames are gathered
        where the videos live and cross to the device in one copy."""
        idx = torch.as_tensor(list(indices), dtype=torch.int64, device=videos.device)
        frames = videos.index_select(1, idx).to(torch.float32)
        B, n = frames.shape[:2]
        x = frames.reshape(B * n, *frames.shape[2:]).to(self.device)
        return self._embed_device(x).reshape(B, n, -1)

    def select(self, embs, n, always_selected=(0,)):
        """Farthest-point selection (inference_util.py:157-185) on embs (B, n_cand, D) on self.device: per item, the candidate
        indices of n picks.  Everything runs on the device; the picks come back in one copy.  FloatingPointError if a distance
        is not finite."""
        embs = embs.to(device=self.device, dtype=torch.float32).contiguous()
        B, n_cand, D = embs.shape
        always = np.ascontiguousarray(np.asarray(list(always_selected), dtype=np.int32))
        if always.size == 0 or (always < 0).any() or (always >= n_cand).any():
            raise IndexError(f"always_selected {list(always_selected)} out of range for {n_cand} candidates")
        work = torch.empty(B * n_cand, dtype=torch.float32, device=self.device)
        out = torch.empty(B * n + 1, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().vd_fps_select(B, n_cand, D, _lib.ptr(embs), n, always.ctypes.data_as(ctypes.c_void_p),
                                                int(always.size), _lib.ptr(work), _lib.ptr(out), _lib.current_stream()))
            res = out.cpu().numpy()
        if res[B * n] & 1:
            raise FloatingPointError("LPIPS frame selection: a distance between frame embeddings is not finite "
                                     "(NaN / inf in the samples or the LPIPS weights)")
        return [[int(v) for v in res[b * n:(b + 1) * n]] for b in range(B)]
