"""A numpy / scipy restatement of the per-frame metrics of the reference's scripts/video_eval.py -- the yardstick of the metrics tests.

The reference scores one channel plane at a time with `skimage.metrics.structural_similarity(gt, pred)` and
`skimage.metrics.peak_signal_noise_ratio(gt, pred)` of scikit-image 0.19.3 (compute_metrics_lazy, :205-225) and a frame pair with
`lpips.LPIPS(net='alex', spatial=False)` of lpips 0.1.4 (compute_lpips_lazy, :228-252).  Neither package is installed where these
tests run, so parity with the packages themselves could not be confirmed and cannot be pinned by a fixture; this file restates
what their sources do, in the order they do it, and is what the HIP path is held to.

  * `ssim_plane`: structural_similarity with its defaults on float images -- win_size 7, `scipy.ndimage.uniform_filter(size=7)` for the
    five means, sample covariance (cov_norm = 49/48), K1 = 0.01, K2 = 0.03, data_range = the width of the float dtype range (-1, 1) = 2
    when none is passed, the mean (in float64) of S after cropping (win_size - 1) // 2 = 3 pixels per side.  `dtype` is the float type
    the arithmetic runs in: float32 is what 0.19.3 does with float32 images, float64 is the yardstick.
  * `ssim_plane_valid`: the same value from the 7 x 7 windows that lie wholly inside the plane, without any filter (the crop
    removes exactly the outputs whose window touches the border).
  * `psnr_plane`: peak_signal_noise_ratio with data_range = 1 (the float dtype's maximum: a ground truth in [0, 1] has a minimum >= 0),
    10 log10(1 / mse), mse = np.mean((a - b) ** 2, dtype=float64) with the difference in `dtype`.
  * `lpips_pairs`: ((embed_restated(a) - embed_restated(b)) ** 2).sum(1) with tests/lpips_restated.py.
"""
import numpy as np
from scipy.ndimage import uniform_filter

WIN = 7


def u8_to_float(u):
    """What the reference does to a sample file: (u / 255.0).astype(float32)."""
    return (np.asarray(u) / 255.0).astype(np.float32)


def _check(x, y):
    if x.shape != y.shape or x.ndim != 2:
        raise ValueError("two planes of one shape")
    if min(x.shape) < WIN:
        raise ValueError("win_size exceeds image extent.")


def _S(ux, uy, uxx, uyy, uxy, data_range):
    cov_norm = WIN * WIN / (WIN * WIN - 1)
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    R = data_range
    C1 = (0.01 * R) ** 2
    C2 = (0.03 * R) ** 2
    A1, A2, B1, B2 = (2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2)
    D = B1 * B2
    return (A1 * A2) / D


def ssim_plane(x, y, data_range=2.0, dtype=np.float64):
    _check(x, y)
    x = x.astype(dtype, copy=False)
    y = y.astype(dtype, copy=False)
    ux = uniform_filter(x, size=WIN)
    uy = uniform_filter(y, size=WIN)
    uxx = uniform_filter(x * x, size=WIN)
    uyy = uniform_filter(y * y, size=WIN)
    uxy = uniform_filter(x * y, size=WIN)
    S = _S(ux, uy, uxx, uyy, uxy, data_range)
    assert S.dtype == dtype
    pad = (WIN - 1) // 2
    return float(S[pad:S.shape[0] - pad, pad:S.shape[1] - pad].mean(dtype=np.float64))


def ssim_plane_valid(x, y, data_range=2.0):
    _check(x, y)
    x = x.astype(np.float64)
    y = y.astype(np.float64)
    win = lambda a: np.lib.stride_tricks.sliding_window_view(a, (WIN, WIN)).mean(axis=(-1, -2))
    return float(_S(win(x), win(y), win(x * x), win(y * y), win(x * y), data_range).mean())


def psnr_plane(x, y, dtype=np.float32):
    if x.shape != y.shape:
        raise ValueError("two planes of one shape")
    x = x.astype(dtype, copy=False)
    y = y.astype(dtype, copy=False)
    err = np.mean((x - y) ** 2, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return float(10 * np.log10(1.0 / err))


def frame_ssim_psnr(gt, pred, ssim_data_range=2.0, dtype=np.float64):
    """gt (N, C, H, W) in [0, 1], pred float or uint8 -> per frame the channel means (ssim, psnr), float64: the loop of
    compute_metrics_lazy (:218-224).  `dtype`: the arithmetic of SSIM's filters and of PSNR's difference."""
    gt = np.asarray(gt, dtype=np.float32)
    pred = np.asarray(pred)
    pred = u8_to_float(pred) if pred.dtype == np.uint8 else pred.astype(np.float32)
    if gt.ndim != 4 or gt.shape != pred.shape:
        raise ValueError("gt and pred: one (N, C, H, W) shape")
    N, C = gt.shape[:2]
    ssim, psnr = np.zeros(N), np.zeros(N)
    for n in range(N):
        for c in range(C):
            ssim[n] += ssim_plane(gt[n, c], pred[n, c], ssim_data_range, dtype)
            psnr[n] += psnr_plane(gt[n, c], pred[n, c], dtype)
        ssim[n] /= C
        psnr[n] /= C
    return ssim, psnr


def lpips_pairs(a, b, w):
    """a, b (N, 3, H, W) torch tensors in [-1, 1] -> (N,) float64: loss_fn(a, b).flatten() of compute_lpips_lazy (:251)."""
    from lpips_restated import embed_restated
    ea, eb = embed_restated(a, w), embed_restated(b, w)
    return ((ea - eb) ** 2).reshape(ea.shape[0], -1).sum(1).numpy()
