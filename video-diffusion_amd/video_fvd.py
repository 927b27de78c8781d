"""Frechet video distance of sampled videos against their ground truth, the I3D embedding on the GPU -- the job of the reference's
scripts/video_fvd.py (SampleDataset :22-35, compute_fvd :77-108, the main block :111-162).

    python -m video_diffusion_amd.video_fvd --eval_dir results/.../autoreg_20_10_300_36 --videos test.npy \
        --i3d_weights i3d_pretrained_400.pt --num_videos 256 [--sample_idx 0] [--T 100]

It reads what `video_sample` / `video_sample_full` wrote: `<eval_dir>/samples/sample_{i:04d}-{sample_idx}.npy` for i < num_videos, uint8
(T, 3, H, W).  The ground truth is videos 0 .. num_videos-1 of --videos / --synthetic (no dataset ships), cut to their first T frames.
The result goes to `<eval_dir>/fvd-{num_videos}-{sample_idx}.txt`; when that file exists it is reported and nothing is read.

Bytes.  The reference turns both sides into uint8 before the network, in float32 numpy: a sample goes u -> -1 + 2 u / 255 ->
((x + 1) * 255 / 2) truncated, the ground truth through the second half.  That round trip is lossy (63 byte values come back one
lower); `byte_table()` holds it, built with those numpy expressions, and the samples pass through it on the host.

The I3D weights do not ship: --i3d_weights names the user's file (fvd.py describes the keys).  A single process; --batch_size is
accepted and does not change the result (the network runs in inference mode: a video's feature does not depend on its batch).
"""
import argparse
from pathlib import Path

import numpy as np
import torch

from .fvd import KEY_LAYOUT, MIN_FRAMES, frechet_distance

I3D_WEIGHTS_NEEDED = f"needs --i3d_weights PATH (the pretrained I3D weights do not ship): {KEY_LAYOUT}"
_table = None


def to_uint8(x):
    """video_fvd.py:97-98: float32 [-1, 1] -> uint8, truncated."""
    return ((np.asarray(x, dtype=np.float32) + 1) * 255 / 2).astype(np.uint8)


def byte_table():
    """table[u] = the byte the reference feeds the network for a sample byte u (:33-35 then :97-98), in float32 numpy as there."""
    global _table
    if _table is None:
        npy = np.arange(256, dtype=np.uint8).astype(np.float32)
        _table = to_uint8(-1 + 2 * npy / 255)
    return _table


def result_path(eval_dir, num_videos, sample_idx):
    return Path(eval_dir) / f"fvd-{num_videos}-{sample_idx}.txt"


def run(args, embed=None, device=None):
    """The body of the reference's script.  `embed(uint8 videos (N, T, 3, H, W)) -> (N, 400)` replaces the GPU embedder: with it given
    nothing here touches a GPU.  Returns the result file's path."""
    from .video_sample import open_videos
    n, T = args.num_videos, args.T
    if n is None or n < 2:
        raise ValueError(f"--num_videos {n}: the Frechet distance needs at least 2 videos per side")
    save_path = result_path(args.eval_dir, n, args.sample_idx)
    if save_path.exists():                                                        # :127-132
        print(f"FVD already computed: {np.loadtxt(save_path).squeeze()}")
        return save_path
    if embed is None and not getattr(args, "i3d_weights", None):
        raise ValueError(f"video_fvd {I3D_WEIGHTS_NEEDED}")
    if T < MIN_FRAMES:
        raise ValueError(f"--T {T}: I3D needs videos of at least {MIN_FRAMES} frames")

    # every file and every ground-truth video checked before anything is embedded
    paths = [Path(args.eval_dir) / "samples" / f"sample_{i:04d}-{args.sample_idx}.npy" for i in range(n)]
    for p in paths:
        if not p.exists():
            raise FileNotFoundError(f"{p}: sample file missing ({n} videos, sample index {args.sample_idx})")
    first = np.load(paths[0], mmap_mode="r")
    ns = argparse.Namespace(videos=getattr(args, "videos", None), synthetic=getattr(args, "synthetic", True), T=T,
                            image_size=int(first.shape[-1]), num_videos=n)
    dataset = open_videos(ns)
    if len(dataset) < n:
        raise ValueError(f"the ground truth has {len(dataset)} videos, --num_videos asks for {n}")
    gt_shape = tuple(dataset[0][0].shape)
    if gt_shape[0] < T:
        raise ValueError(f"the ground-truth videos have {gt_shape[0]} frames, --T asks for {T}")
    want = (T,) + gt_shape[1:]
    for p in paths:
        a = np.load(p, mmap_mode="r")
        if a.ndim != 4 or a.dtype != np.uint8 or a.shape[0] != T:
            raise ValueError(f"{p}: {a.dtype} {tuple(a.shape)}, expected uint8 with exactly T = {T} frames")
        if tuple(a.shape) != want:
            raise ValueError(f"{p}: frames of {tuple(a.shape[1:])}, but the ground truth's are {want[1:]}")

    if embed is None:
        from .fvd import I3D
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        embed = I3D.from_files(args.i3d_weights, device).embed
    table = byte_table()

    def features(videos):
        return np.asarray(torch.as_tensor(embed(torch.from_numpy(videos))).detach().cpu(), dtype=np.float64).reshape(1, -1)

    sample_feats, gt_feats = [], []
    for i, p in enumerate(paths):                                                 # one video of each side on the device at a time
        sample_feats.append(features(table[np.load(p)][None]))
        gt_feats.append(features(to_uint8(dataset[i][0][:T].to(torch.float32).numpy())[None]))
    fvd = frechet_distance(np.concatenate(sample_feats), np.concatenate(gt_feats))      # :107: (samples, ground truth)
    np.savetxt(save_path, np.array([fvd]))
    print(f"FVD: {fvd}")
    return save_path


def main(argv=None):
    from .script_util import str2bool
    ap = argparse.ArgumentParser(description="Frechet video distance of <eval_dir>/samples against the ground truth")
    ap.add_argument("--eval_dir", type=str, required=True)
    ap.add_argument("--num_videos", type=int, required=True, help="videos 0 .. num_videos-1 of both sides")
    ap.add_argument("--batch_size", type=int, default=None, help="accepted for compatibility; the result does not depend on it")
    ap.add_argument("--sample_idx", type=int, default=0)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--videos", default=None, help=".npy file of the test videos (N, T, 3, H, W): float in [-1, 1] or uint8")
    ap.add_argument("--synthetic", type=str2bool, nargs="?", const=True, default=True,
                    help="without --videos: the synthetic videos the sampling CLIs draw (item i seeded by i)")
    ap.add_argument("--i3d_weights", default=None, metavar="PATH", help="state dict of the PyTorch port of I3D (fvd.py)")
    args = ap.parse_args(argv)
    if not args.i3d_weights:
        ap.error(f"video_fvd {I3D_WEIGHTS_NEEDED}")
    return run(args)


if __name__ == "__main__":
    main()
