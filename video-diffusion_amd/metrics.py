"""SSIM and PSNR of predicted frames against their ground truth on the GPU (csrc/metrics.hip): what `compute_metrics_lazy` of the
reference's scripts/video_eval.py (:205-225) gets from scikit-image 0.19.3 one channel plane at a time.

`frame_ssim_psnr(gt, pred)` takes N frames at once and returns, per frame, the mean over the channel planes of
`structural_similarity(gt[n, c], pred[n, c])` and of `peak_signal_noise_ratio(gt[n, c], pred[n, c])`, as float64.

The reference passes no `data_range`.  For PSNR scikit-image then takes 1 (the float dtype's maximum, because a ground truth in
[0, 1] has no negative value).  For SSIM its 0.19.3 takes the WIDTH of the float dtype range (-1, 1), i.e. R = 2, so C1 and C2 are
four times what the true range of the images gives.  Every SSIM the reference's authors reported carries that choice, so it is the
default here; `ssim_data_range=1.0` gives the SSIM of images in [0, 1].
"""
import torch

from . import _lib

WIN = 7                      # scikit-image's default window
REFERENCE_SSIM_DATA_RANGE = 2.0


def check_frame_size(H, W):
    """ValueError for frames a 7 x 7 window does not fit (scikit-image: 'win_size exceeds image extent')."""
    if H < WIN or W < WIN:
        raise ValueError(f"win_size exceeds image extent: SSIM's {WIN}x{WIN} window does not fit a {H}x{W} frame")


def launch_plan(H, W):
    """(rows_tile, nstrips, groups) that `vd_frame_metrics` launches with for H x W planes: the input rows of a full LDS strip, the strips
    per plane and the row runs per strip.  Host only; VdError where the size is refused."""
    import ctypes
    r, s, g = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.lib().vd_frame_metrics_plan(H, W, ctypes.byref(r), ctypes.byref(s), ctypes.byref(g)))
    return r.value, s.value, g.value


def _device_tensor(a, device):
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(a)
    if t.dtype != torch.uint8:
        t = t.to(torch.float32)
    return t.to(device).contiguous()


def frame_ssim_psnr_device(gt, pred, ssim_data_range=REFERENCE_SSIM_DATA_RANGE):
    """gt (N, C, H, W) float32 in [0, 1] and pred (same shape, uint8 or float32), both contiguous on one GPU -> (ssim, psnr), two (N,)
    float64 tensors on that GPU.  Enqueued on the current stream."""
    if gt.ndim != 4 or tuple(gt.shape) != tuple(pred.shape):
        raise ValueError(f"frame metrics: gt {tuple(gt.shape)} and pred {tuple(pred.shape)} must be the same (N, C, H, W)")
    N, C, H, W = gt.shape
    check_frame_size(H, W)
    if gt.dtype != torch.float32 or pred.dtype not in (torch.float32, torch.uint8):
        raise TypeError("frame metrics: gt float32, pred float32 or uint8")
    if gt.device.type != "cuda" or pred.device != gt.device or not gt.is_contiguous() or not pred.is_contiguous():
        raise ValueError("frame metrics: contiguous tensors on one GPU")
    ssim = torch.empty(N, dtype=torch.float64, device=gt.device)
    psnr = torch.empty(N, dtype=torch.float64, device=gt.device)
    with torch.cuda.device(gt.device):
        _lib.check(_lib.lib().vd_frame_metrics(N, C, H, W, _lib.ptr(gt), _lib.ptr(pred), int(pred.dtype == torch.uint8),
                                               float(ssim_data_range), _lib.ptr(ssim), _lib.ptr(psnr), _lib.current_stream()))
    return ssim, psnr


def frame_ssim_psnr(gt, pred, ssim_data_range=REFERENCE_SSIM_DATA_RANGE, device=None):
    """gt (N, C, H, W) in [0, 1], pred the same shape in [0, 1] or uint8 (read as u / 255); tensors or arrays on any device ->
    (ssim, psnr) as (N,) float64 numpy arrays.  ValueError for frames below 7 x 7, before anything is launched."""
    shape = tuple(gt.shape)
    if len(shape) != 4 or shape != tuple(pred.shape):
        raise ValueError(f"frame metrics: gt {shape} and pred {tuple(pred.shape)} must be the same (N, C, H, W)")
    check_frame_size(shape[2], shape[3])
    if device is None:
        device = next((t.device for t in (gt, pred) if isinstance(t, torch.Tensor) and t.device.type == "cuda"),
                      torch.device("cuda", torch.cuda.current_device()))
    ssim, psnr = frame_ssim_psnr_device(_device_tensor(gt, device), _device_tensor(pred, device), ssim_data_range)
    return ssim.cpu().numpy(), psnr.cpu().numpy()
