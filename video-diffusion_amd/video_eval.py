"""Score sampled videos against their ground truth: SSIM, PSNR and LPIPS per frame on the GPU -- the job of the reference's
scripts/video_eval.py (LazyDataFetch :26-100, compute_metrics_lazy :205-225, compute_lpips_lazy :228-252, the main block :255-397).

    python -m video_diffusion_amd.video_eval --eval_dir results/.../autoreg_20_10_300_36 --videos test.npy \
        --lpips_weights alexnet.pth,alex.pth

It reads what `video_sample` / `video_sample_full` wrote: `<eval_dir>/samples/sample_%04d-%d.npy`, uint8 (T, 3, H, W), turned into
float32 as u / 255.  The ground truth is the dataset video in [-1, 1] mapped to [0, 1]; no dataset ships, so it comes from
--videos / --synthetic as for the sampling CLIs (--dataset and --dataset_partition are accepted and only reported).  The first
`obs_length` frames of both are dropped.  Per mode the result is a float64 array (num_videos, num_samples, T - obs_length), kept in
`<eval_dir>/metrics_{num_videos}-{num_samples}-{T}.pkl`, a dict mode -> array; modes the pickle already holds are not recomputed,
and the pickle is rewritten under `test_util.Protect`.

  ssim, psnr   metrics.frame_ssim_psnr_device (csrc/metrics.hip): scikit-image 0.19.3's defaults, including the data range 2 that
               it takes for SSIM of float images when none is passed (--ssim_data_range 1.0 for the true range of the images).
  lpips        lpips.LpipsAlex.distance on both videos mapped to [-1, 1]; needs --lpips_weights.
  fvd          not computed here: the reference takes its I3D network from TF-Hub through tensorflow.

One video's ground truth crosses to the device once and serves all its samples and all three metrics; a sample crosses once as
uint8.  A single process: there is no dealing of videos to ranks, and no wandb.
"""
import argparse
import json
import pickle
from collections import defaultdict
from pathlib import Path

import numpy as np
import torch

MODES = ("ssim", "psnr", "lpips")
FVD_REFUSAL = ("fvd is not computed here: the reference embeds videos with the I3D network it downloads from TF-Hub through "
               "tensorflow, and neither ships; ssim, psnr and lpips are available")
drange = [-1, 1]             # range of the dataset's pixel values (video_eval.py:320)


def discover_samples(eval_dir, num_samples=None):
    """video index -> its sample files (video_eval.py:45-63): `samples/sample_*.npy`, the numbers behind the last '_' read as
    (video index, sample index), sorted by VIDEO index only -- a stable sort, so one video's files keep the order in which the
    directory lists them, as there.  Asserts that every video has at least `num_samples` files."""
    samples_dir = Path(eval_dir) / "samples"
    assert samples_dir.exists(), f"Samples dir {samples_dir} does not exist."
    found = [(p, [int(v) for v in p.stem.split("_")[-1].split("-")]) for p in samples_dir.glob("sample_*.npy")]
    found.sort(key=lambda item: item[1][0])
    by_video = defaultdict(list)
    for path, (video_idx, _) in found:
        by_video[video_idx].append(path)
    if num_samples is not None:
        for idx, paths in by_video.items():
            assert len(paths) >= num_samples, \
                f"Expected at least {num_samples} samples for each video, but found {len(paths)} for video #{idx}"
    return dict(by_video)


def _gpu_metrics(gt01, pred_u8, ssim_data_range):
    from .metrics import frame_ssim_psnr_device
    ssim, psnr = frame_ssim_psnr_device(gt01, pred_u8, ssim_data_range)
    return ssim.cpu().numpy(), psnr.cpu().numpy()


def _resolve_modes(modes):
    modes = list(modes)
    if "fvd" in modes:
        raise ValueError(FVD_REFUSAL)
    if "all" in modes:
        print("Modes: all = ssim, psnr, lpips (fvd is not computed here).")
        modes = list(MODES)
    unknown = [m for m in modes if m not in MODES]
    if unknown:
        raise ValueError(f"unknown modes {unknown}; available: {', '.join(MODES)}")
    return [m for m in MODES if m in modes]


def run(args, metrics=None, lpips=None, device=None):
    """The body of the reference's script (:299-397).  `metrics(gt01, pred_u8, ssim_data_range) -> (ssim, psnr)` and
    `lpips(gt, pred) -> distances` (both videos in [-1, 1]) replace the GPU functions, as `infer=` does in video_sample.run: with both
    given nothing here touches a GPU and the tensors stay on the host.  Returns the pickle's path."""
    from . import test_util
    from .video_sample import LPIPS_WEIGHTS_NEEDED, open_videos
    modes = _resolve_modes(args.modes)
    if "lpips" in modes and lpips is None and not getattr(args, "lpips_weights", None):
        raise ValueError(f"--modes lpips {LPIPS_WEIGHTS_NEEDED}")
    eval_dir = Path(args.eval_dir)
    config_path = eval_dir / "model_config.json"
    if getattr(args, "dataset", None) is None and config_path.exists():          # :301-308
        with open(config_path) as f:
            args.dataset = json.load(f).get("dataset")
    files = discover_samples(eval_dir, args.num_samples)
    assert files, f"no sample_*.npy under {eval_dir / 'samples'}"
    keys = list(files)
    if args.num_samples is None:                                                 # :328-329: the first video's count
        args.num_samples = len(files[keys[0]])
        for idx, paths in files.items():
            assert len(paths) >= args.num_samples, \
                f"Expected at least {args.num_samples} video prediction samples. Found {len(paths)} for video #{idx}"
    used = {idx: paths[:args.num_samples] for idx, paths in files.items()}
    first = np.load(used[keys[0]][0], mmap_mode="r")
    if first.ndim != 4:
        raise ValueError(f"{used[keys[0]][0]}: expected a (T, C, H, W) sample, got {first.shape}")
    T_file = int(first.shape[0])
    if args.T is None:                                                           # :330-333
        args.T = T_file
    else:
        assert args.T <= T_file, f"--T {args.T} exceeds the samples' {T_file} frames"
    n_frames = args.T - args.obs_length
    assert n_frames > 0, f"nothing to score: T = {args.T}, obs_length = {args.obs_length}"

    name = f"metrics_{len(keys)}-{args.num_samples}-{args.T}"
    pickle_path = eval_dir / f"{name}.pkl"
    if pickle_path.exists():                                                     # :343-352
        with open(pickle_path, "rb") as f:
            done = pickle.load(f)
        modes = [m for m in modes if m not in done]
    print(f"Modes: {modes}")
    if not modes:
        print("No metrics to compute.")
        return pickle_path

    # the ground truth: the sampling CLIs' stand-in for get_test_dataset; --synthetic videos are a function of (index, T, size) alone
    ns = argparse.Namespace(videos=getattr(args, "videos", None), synthetic=getattr(args, "synthetic", True), T=T_file,
                            image_size=int(first.shape[-1]),
                            num_videos=max(getattr(args, "num_videos", None) or 0, max(keys) + 1))
    dataset = open_videos(ns)
    # every file and every ground-truth video against the first sample, before anything is computed
    want = tuple(first.shape)
    from .metrics import check_frame_size
    check_frame_size(want[2], want[3])
    for idx in keys:
        assert 0 <= idx < len(dataset), f"{used[idx][0]}: video #{idx} is not in the ground truth ({len(dataset)} videos)"
        for path in used[idx]:
            a = np.load(path, mmap_mode="r")
            if tuple(a.shape) != want or a.dtype != np.uint8:
                raise ValueError(f"{path}: {a.dtype} {tuple(a.shape)}, expected uint8 {want} as {used[keys[0]][0]}")
        g = dataset[idx][0]
        if g.shape[0] < args.T or tuple(g.shape[1:]) != want[1:]:
            raise ValueError(f"{used[idx][0]}: samples are {want}, but ground-truth video #{idx} is {tuple(g.shape)} "
                             f"(needs {args.T} frames of {want[1:]})")

    need_sp = "ssim" in modes or "psnr" in modes
    need_lp = "lpips" in modes
    on_gpu = (need_sp and metrics is None) or (need_lp and lpips is None)
    if on_gpu and device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if need_sp and metrics is None:
        metrics = _gpu_metrics
    if need_lp and lpips is None:
        from .lpips import LpipsAlex
        lpips = LpipsAlex.from_files(args.lpips_weights, device).distance
    ssim_range = float(getattr(args, "ssim_data_range", 2.0))
    place = (lambda t: t.to(device)) if on_gpu else (lambda t: t)

    new = {m: np.zeros((len(keys), args.num_samples, n_frames)) for m in modes}
    for i, idx in enumerate(keys):
        gt = dataset[idx][0].to(torch.float32)
        gt01 = ((gt - drange[0]) / (drange[1] - drange[0]))[args.obs_length:args.T]      # :77-83
        gt01 = place(gt01.contiguous())
        gt_pm = gt01 * 2 - 1 if need_lp else None                                         # :245
        for k, path in enumerate(used[idx]):
            pred = place(torch.from_numpy(np.load(path)[args.obs_length:args.T].copy()))  # uint8
            if need_sp:
                ssim, psnr = metrics(gt01, pred, ssim_range)
                if "ssim" in new:
                    new["ssim"][i, k] = np.asarray(ssim, dtype=np.float64)
                if "psnr" in new:
                    new["psnr"][i, k] = np.asarray(psnr, dtype=np.float64)
            if need_lp:
                # u / 255 as an IEEE division (by a tensor: a scalar divisor may be turned into a multiplication), then [-1, 1] (:74,246)
                pred_pm = pred.to(torch.float32) / torch.full((), 255.0, device=pred.device) * 2 - 1
                new["lpips"][i, k] = np.asarray(lpips(gt_pm, pred_pm), dtype=np.float64).reshape(-1)
    for m in modes:
        print("{}\t{:.4f}".format(m, new[m].mean()))

    with test_util.Protect(pickle_path):                                         # :388-396
        if pickle_path.exists():
            with open(pickle_path, "rb") as f:
                saved = pickle.load(f)
        else:
            saved = {}
        for m in modes:
            saved[m] = new[m]
        with open(pickle_path, "wb") as f:
            pickle.dump(saved, f)
    print(f"Saved metrics to {pickle_path}.")
    return pickle_path


def main(argv=None):
    from .script_util import str2bool
    from .video_sample import LPIPS_WEIGHTS_NEEDED, add_lpips_arguments
    ap = argparse.ArgumentParser(description="SSIM, PSNR and LPIPS of the samples under <eval_dir>/samples against their ground truth")
    ap.add_argument("--eval_dir", type=str, required=True)
    ap.add_argument("--dataset", type=str, default=None, help="reported only (default: `dataset` of <eval_dir>/model_config.json); "
                                                              "the ground truth comes from --videos / --synthetic")
    ap.add_argument("--dataset_partition", default="test", choices=["train", "test"], help="reported only")
    ap.add_argument("--modes", nargs="+", type=str, default=["all"], choices=["ssim", "psnr", "lpips", "fvd", "all"],
                    help="all = ssim psnr lpips; fvd is refused (it needs the TF-Hub I3D network)")
    ap.add_argument("--obs_length", type=int, default=36, help="Number of observed frames. Default is 36.")
    ap.add_argument("--T", type=int, default=None, help="Video length. If not given, the samples' length.")
    ap.add_argument("--num_samples", type=int, default=None, help="Number of generated samples per test video.")
    ap.add_argument("--videos", default=None, help=".npy file of the test videos (N, T, 3, H, W): float in [-1, 1] or uint8")
    ap.add_argument("--synthetic", type=str2bool, nargs="?", const=True, default=True,
                    help="without --videos: the synthetic videos the sampling CLIs draw (item i seeded by i)")
    ap.add_argument("--num_videos", type=int, default=None, help="size of the synthetic dataset (default: up to the last sampled video)")
    ap.add_argument("--ssim_data_range", type=float, default=2.0,
                    help="2.0 as the reference's pinned scikit-image computes (the width of the float dtype range); 1.0 is the true range")
    add_lpips_arguments(ap)
    args = ap.parse_args(argv)
    if "fvd" in args.modes:
        ap.error(FVD_REFUSAL)
    if ("lpips" in args.modes or "all" in args.modes) and not args.lpips_weights:
        ap.error(f"--modes lpips {LPIPS_WEIGHTS_NEEDED}")
    return run(args)


if __name__ == "__main__":
    main()
