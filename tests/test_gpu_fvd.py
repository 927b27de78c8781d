"""GPU: the I3D video embedder of the video_fvd job (csrc/i3d.hip) against the float64 plain-torch restatement of the network
(tests/i3d_restated.py; tensorflow and the TF-Hub module are not available, so the restatement is the yardstick): the three
operator entries, the whole embedder with synthetic weights, batch independence, the frame limits, and the CLI end to end.

Error bound: the project's per-op bar, |d| <= 1e-4 + 1e-4 |ref|, for every operator output and for every one of the 400
logits of every video.  The operands and the accumulation are fp32 (the fp32 MFMA's documented error is <= 3.5e-7 * sum|a b| at
K = 4096); float32 torch against float64 torch on the same network stays below 2 % of the bar.  Measured on the MI355X: largest
operator error 1.2e-5 (3x3x3, Cin 832, |ref| up to 4.7), resize 5.2e-6, logits 6.5e-6 on logits up to 15.5 (T = 41)."""
import ctypes

import numpy as np
import pytest
import torch

import i3d_restated as ir
from helpers import close
from video_diffusion_amd import _lib, fvd, video_fvd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_cache = {}


def model():
    if "m" not in _cache:
        sd = ir.synth_state_dict(0)
        _cache["m"] = (fvd.I3D.from_state_dict(sd, DEV), sd)
    return _cache["m"]


def _video(T, H, W, seed):
    """uint8 (T, 3, H, W): smooth moving ramps plus noise, so that frames differ and the ReLU maps are neither empty nor full."""
    g = torch.Generator().manual_seed(seed)
    yy = torch.linspace(-1, 1, H).view(1, 1, H, 1)
    xx = torch.linspace(-1, 1, W).view(1, 1, 1, W)
    tt = torch.linspace(0, 1, T).view(T, 1, 1, 1)
    a = torch.rand(1, 3, 1, 1, generator=g) * 2 - 1
    b = torch.rand(1, 3, 1, 1, generator=g) * 2 - 1
    x = 0.5 * torch.sin(3 * (a * yy + b * xx) + 4 * tt) + 0.4 * (torch.rand(T, 3, H, W, generator=g) * 2 - 1)
    return ((x.clamp(-1, 1) + 1) * 127.5).to(torch.uint8)


def _channels_last(x):
    """(1, C, T, H, W) -> [T][H][W][C] on the device."""
    return x[0].permute(1, 2, 3, 0).contiguous().to(device=DEV, dtype=torch.float32)


def _channels_first(y):
    return y.permute(3, 0, 1, 2).unsqueeze(0)


# ---------------------------------------------------------------- operators
CONV_CASES = [
    # kernel, stride, Cin, Cout, (T, H, W), relu + bias, pad channels (before, behind) of a wider output tensor
    ((7, 7, 7), (2, 2, 2), 3, 64, (9, 21, 18), True, (0, 0)),
    ((7, 7, 7), (2, 2, 2), 16, 16, (10, 12, 9), False, (0, 0)),
    ((1, 1, 1), (1, 1, 1), 16, 16, (3, 7, 5), True, (0, 0)),
    ((1, 1, 1), (1, 1, 1), 832, 400, (3, 7, 6), True, (8, 24)),
    ((1, 1, 1), (1, 1, 1), 3, 400, (5, 9, 7), False, (0, 0)),
    ((3, 3, 3), (1, 1, 1), 16, 400, (5, 9, 7), True, (16, 8)),
    ((3, 3, 3), (1, 1, 1), 832, 16, (3, 6, 5), False, (0, 0)),
    ((3, 3, 3), (1, 1, 1), 3, 16, (4, 8, 11), True, (0, 0)),
    ((3, 3, 3), (1, 1, 1), 24, 64, (7, 14, 13), True, (64, 0)),
    # the 2-D use of the same kernel (LPIPS conv2 and conv3..5): kt = 1, the frames on the T axis; SAME at stride 1 = AlexNet's pads 2 and 1
    ((1, 5, 5), (1, 1, 1), 64, 192, (3, 7, 6), True, (0, 0)),
    ((1, 3, 3), (1, 1, 1), 192, 384, (2, 3, 3), True, (0, 0)),
]


@pytest.mark.parametrize("kernel,stride,Cin,Cout,size,act,slack", CONV_CASES)
def test_conv3d_same_vs_float64(kernel, stride, Cin, Cout, size, act, slack):
    g = torch.Generator().manual_seed(Cin * 1000 + Cout + kernel[0])
    T, H, W = size
    x = torch.randn(1, Cin, T, H, W, generator=g)
    w = torch.randn(Cout, Cin, *kernel, generator=g) * (2.0 / (Cin * kernel[0] * kernel[1] * kernel[2])) ** 0.5
    bias = torch.randn(Cout, generator=g) * 0.1 if act else None
    want = ir.conv3d_same(x.double(), w.double(), stride, None if bias is None else bias.double())
    if act:
        want = torch.relu(want)
    To, Ho, Wo = want.shape[2:]
    M = To * Ho * Wo
    width = slack[0] + Cout + slack[1]
    out = torch.full((M, width), -77.0, dtype=torch.float32, device=DEV)
    xd, wd = _channels_last(x), w.to(DEV).contiguous()
    bd = None if bias is None else bias.to(DEV)
    view = out[:, slack[0]:]
    with torch.cuda.device(0):
        _lib.check(_lib.lib().vd_op_conv3d_same(_lib.ptr(xd), _lib.ptr(wd), _lib.ptr(bd), T, H, W, Cin, Cout, *kernel, *stride, int(act),
                                                ctypes.c_void_p(view.data_ptr()), width, _lib.current_stream()))
    torch.cuda.synchronize()
    out = out.cpu()
    got = _channels_first(out[:, slack[0]:slack[0] + Cout].reshape(To, Ho, Wo, Cout)).double()
    err = close(got, want)
    print(f"conv3d k{kernel} s{stride} Cin {Cin} Cout {Cout} M {M}: max|d| {err:.3e}, max|ref| {want.abs().max().item():.3f}")
    assert want.abs().max() > 0.5
    assert bool((out[:, :slack[0]] == -77.0).all()) and bool((out[:, slack[0] + Cout:] == -77.0).all()), "neighbouring channels were written"


@pytest.mark.parametrize("kernel,stride", [((1, 3, 3), (1, 2, 2)), ((3, 3, 3), (2, 2, 2)), ((2, 2, 2), (2, 2, 2)), ((3, 3, 3), (1, 1, 1))])
@pytest.mark.parametrize("size,C", [((6, 14, 12), 64), ((7, 13, 15), 16), ((5, 8, 9), 192)])
def test_maxpool3d_same_is_exact(kernel, stride, size, C):
    g = torch.Generator().manual_seed(C + size[0])
    T, H, W = size
    x = torch.randn(1, C, T, H, W, generator=g)                      # both signs: padding must not win where every tap is negative
    want = ir.maxpool3d_same(x, kernel, stride)
    To, Ho, Wo = want.shape[2:]
    assert (To, Ho, Wo) == tuple(fvd.same_pad(n, k, s)[0] for n, k, s in zip(size, kernel, stride))
    xd = _channels_last(x)
    out = torch.empty(To, Ho, Wo, C, dtype=torch.float32, device=DEV)
    with torch.cuda.device(0):
        _lib.check(_lib.lib().vd_op_maxpool3d_same(_lib.ptr(xd), T, H, W, C, *kernel, *stride, _lib.ptr(out), _lib.current_stream()))
    assert torch.equal(_channels_first(out.cpu()), want)


@pytest.mark.parametrize("H,W", [(64, 64), (128, 128), (100, 60), (224, 224)])
def test_resize_bilinear_tf1(H, W):
    T = 3
    frames = _video(T, H, W, seed=H + W)
    want = ir.resize_bilinear_tf1(frames)
    fd = frames.to(DEV).contiguous()
    out = torch.empty(T, 224, 224, 3, dtype=torch.float32, device=DEV)
    with torch.cuda.device(0):
        _lib.check(_lib.lib().vd_op_resize_bilinear_tf1(_lib.ptr(fd), T, H, W, _lib.ptr(out), _lib.current_stream()))
    got = out.cpu()
    err = close(got.double(), want)
    print(f"resize {H}x{W} -> 224: max|d| {err:.3e}")
    assert want.min() >= -1 and want.max() <= 1 and want.std() > 0.1
    if (H, W) == (224, 224):                                          # identity: every output is its own pixel, no interpolation error
        exact = (2 * frames.to(torch.float32) / torch.full((), 255.0) - 1).permute(0, 2, 3, 1)
        assert torch.equal(got, exact)


# ---------------------------------------------------------------- the embedder
@pytest.mark.parametrize("T,H,W", [(9, 64, 64), (16, 64, 64), (17, 64, 64), (41, 64, 64), (12, 128, 96)])
def test_embedder_vs_float64(T, H, W):
    emb, sd = model()
    v = _video(T, H, W, seed=T * 7 + H)
    got = emb.embed(v[None])
    assert got.shape == (1, 400) and got.dtype == torch.float32 and got.device.type == "cuda"
    want = ir.embed_restated(v, sd)
    err = close(got[0].double(), want)
    print(f"I3D T {T} {H}x{W}: max|d| {err:.3e}, max|logit| {want.abs().max().item():.3f}")
    assert want.abs().max() > 0.5 and want.std() > 0.1


def test_batch_independence_and_determinism():
    emb, _ = model()
    vids = torch.stack([_video(16, 64, 64, seed=s) for s in (1, 2, 3)])
    both = emb.embed(vids)
    again = emb.embed(vids)
    singles = torch.cat([emb.embed(vids[i:i + 1]) for i in range(3)])
    assert torch.equal(both, again) and torch.equal(both, singles)
    assert not torch.equal(both[0], both[1])


def test_frame_limits_are_refused_before_any_work():
    emb, _ = model()
    top = fvd.max_frames()
    assert top == 1024
    with pytest.raises(_lib.VdError, match="at least 9 frames"):
        emb.embed(torch.zeros(1, 8, 3, 16, 16, dtype=torch.uint8))
    with pytest.raises(_lib.VdError, match="1024"):
        emb.embed(torch.zeros(1, top + 1, 3, 8, 8, dtype=torch.uint8))
    v = _video(9, 32, 32, seed=4)
    out = emb.embed(v[None])
    assert bool(torch.isfinite(out).all()) and out.abs().max() > 0


# ---------------------------------------------------------------- the CLI
def test_cli_end_to_end(tmp_path, capsys):
    emb, sd = model()
    n, T, S = 4, 12, 32
    torch.save(sd, tmp_path / "i3d.pt")
    (tmp_path / "samples").mkdir()
    samples = torch.stack([_video(T, S, S, seed=100 + i) for i in range(n)]).numpy()
    for i in range(n):
        np.save(tmp_path / "samples" / f"sample_{i:04d}-0.npy", samples[i])
    gt = torch.stack([_video(T + 3, S, S, seed=200 + i) for i in range(n)]).float() / 255 * 2 - 1
    np.save(tmp_path / "gt.npy", gt.numpy())
    path = video_fvd.main(["--eval_dir", str(tmp_path), "--videos", str(tmp_path / "gt.npy"), "--i3d_weights", str(tmp_path / "i3d.pt"),
                           "--num_videos", str(n), "--T", str(T), "--batch_size", "3"])
    assert path == tmp_path / f"fvd-{n}-0.txt"
    s_bytes = video_fvd.byte_table()[samples]
    g_bytes = ((gt[:, :T].numpy() + 1) * 255 / 2).astype(np.uint8)
    fs = emb.embed(torch.from_numpy(s_bytes)).cpu().double().numpy()
    fg = emb.embed(torch.from_numpy(g_bytes)).cpu().double().numpy()
    want = fvd.frechet_distance(fs, fg)
    got = float(np.loadtxt(path))
    assert got == want and np.isfinite(got) and got > 0
    assert f"FVD: {got}" in capsys.readouterr().out
    for feats, vids in ((fs, s_bytes), (fg, g_bytes)):
        for i in range(n):
            close(feats[i], ir.embed_restated(torch.from_numpy(vids[i]), sd).numpy())
