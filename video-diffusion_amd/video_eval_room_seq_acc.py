"""3-class accuracy of sampled GQN-Mazes videos, the green-pixel counts on the GPU -- the job of the reference's
scripts/video_eval_room_seq_acc.py (LazyDataFetch :30-103, the main block :206-294).

    python -m video_diffusion_amd.video_eval_room_seq_acc --eval_dir results/.../autoreg_20_10_300_36 --videos test.npy \
        [--obs_length 36] [--num_samples 5] [--T 300] [--out result.json]

Every video is put into one of three classes by its ground truth: the agent stays in its room, it enters the green hallway and
stays there, or it enters and comes back.  A sample is right when it shows its video's class; the accuracy of sample index k is the
share of videos whose k-th sample is right.  It is the one Mazes metric that asks for long-range coherence rather than per-frame
fidelity.

It reads what `video_sample` / `video_sample_full` wrote: `<eval_dir>/samples/sample_%04d-%d.npy`, uint8 (T, 3, H, W); sample k of a
video is the file whose name ends in -k.  The ground truth is the dataset video in [-1, 1] mapped to [0, 1] in float32 and turned
into bytes as (x * 255) TRUNCATED, as the reference does (for a video that was u / 127.5 - 1 that is not the identity: 63 of the 256
levels come out one lower); no dataset ships, so it comes from --videos / --synthetic as for the other jobs.  The first `obs_length`
frames of both are dropped, and both are cut to --T frames (default: the samples' length).

Per video there are two launches of hallway.hallway_counts (csrc/hallway.hip): the ground truth as float32, all its samples as one
uint8 stack.  Smoothing, the state machine and the accuracy are hallway.py's numpy restatements of the reference, run on (videos, T)
arrays as there.  Thresholds 1000 / 500 and rows 14:45 fit 64 x 64 Mazes frames; --entry_thresh, --out_thresh and --rows exist so
that other sizes can be handled.  A single process.
"""
import argparse
import json
from pathlib import Path

import numpy as np
import torch

from .hallway import (ENTRY_THRESH, OUT_THRESH, ROWS, check_rows, class_members, classify, smooth_counts, three_class_accuracy,
                      three_class_count)
from .video_eval import discover_samples, drange

CLASSES = ("room_stay", "hallway_enter_stay", "hallway_enter_recover")


def _gpu_counts(frames, rows):
    from .hallway import hallway_counts
    return hallway_counts(frames, rows)


def sample_index(path):
    """The k of sample_<video>-<k>.npy (get_sample, :238-241)."""
    return int(Path(path).stem.split("-")[-1])


def run(args, counts=None):
    """The body of the reference's script.  `counts(frames, rows) -> (N,) integers` replaces the GPU function (frames: a (N, 3, H, W)
    tensor, uint8 or float32 in [0, 1]), as `metrics=` does in video_eval.run: with it given nothing here touches a GPU.  Returns
    the result as a dict, prints the reference's lines, and writes the dict as JSON to args.out when that is set."""
    from .video_sample import open_videos
    eval_dir = Path(args.eval_dir)
    num_samples = int(args.num_samples)
    assert num_samples >= 1, f"--num_samples {num_samples}"
    files = discover_samples(eval_dir, num_samples)
    assert files, f"no sample_*.npy under {eval_dir / 'samples'}"
    keys = list(files)
    by_index = {idx: {sample_index(p): p for p in paths} for idx, paths in files.items()}
    for idx in keys:
        missing = [k for k in range(num_samples) if k not in by_index[idx]]
        if missing:
            raise ValueError(f"video #{idx}: no sample with index {missing[0]} under {eval_dir / 'samples'} "
                             f"(sample indices 0..{num_samples - 1} are needed, found {sorted(by_index[idx])})")
    used = {idx: [by_index[idx][k] for k in range(num_samples)] for idx in keys}

    first_path = used[keys[0]][0]
    first = np.load(first_path, mmap_mode="r")
    if first.ndim != 4 or first.shape[1] != 3:
        raise ValueError(f"{first_path}: expected a (T, 3, H, W) sample, got {first.shape}")
    want = tuple(first.shape)
    T_file, H = want[0], want[2]
    T = getattr(args, "T", None)
    if T is None:
        T = T_file
    else:
        assert T <= T_file, f"--T {T} exceeds the samples' {T_file} frames"
    n_frames = T - args.obs_length
    assert n_frames > 0, f"nothing to classify: T = {T}, obs_length = {args.obs_length}"
    rows = getattr(args, "rows", None)
    if rows is None:
        if H < ROWS[1]:
            raise ValueError(f"frames of {H} rows are lower than row {ROWS[1]}: the hallway strip is rows {ROWS[0]}:{ROWS[1]} of a "
                             f"64 x 64 Mazes frame; give --rows FIRST LAST_PLUS_1 (and thresholds) for other sizes")
        rows = ROWS
    rows = check_rows(H, rows)
    entry_thresh = getattr(args, "entry_thresh", None)
    out_thresh = getattr(args, "out_thresh", None)
    entry_thresh = ENTRY_THRESH if entry_thresh is None else entry_thresh
    out_thresh = OUT_THRESH if out_thresh is None else out_thresh

    ns = argparse.Namespace(videos=getattr(args, "videos", None), synthetic=getattr(args, "synthetic", True), T=T_file,
                            image_size=int(want[-1]), num_videos=max(getattr(args, "num_videos", None) or 0, max(keys) + 1))
    dataset = open_videos(ns)
    # every file and every ground-truth video against the first sample, before anything is computed
    for idx in keys:
        assert 0 <= idx < len(dataset), f"{used[idx][0]}: video #{idx} is not in the ground truth ({len(dataset)} videos)"
        for path in used[idx]:
            a = np.load(path, mmap_mode="r")
            if tuple(a.shape) != want or a.dtype != np.uint8:
                raise ValueError(f"{path}: {a.dtype} {tuple(a.shape)}, expected uint8 {want} as {first_path}")
        g = dataset[idx][0]
        if g.shape[0] < T or tuple(g.shape[1:]) != want[1:]:
            raise ValueError(f"{used[idx][0]}: samples are {want}, but ground-truth video #{idx} is {tuple(g.shape)} "
                             f"(needs {T} frames of {want[1:]})")

    if counts is None:
        counts = _gpu_counts
    gt_counts = np.zeros((len(keys), n_frames), dtype=np.int64)
    pred_counts = np.zeros((num_samples, len(keys), n_frames), dtype=np.int64)
    for i, idx in enumerate(keys):
        gt = dataset[idx][0].to(torch.float32)
        gt01 = ((gt - drange[0]) / (drange[1] - drange[0]))[args.obs_length:T].contiguous()          # :81-87
        gt_counts[i] = np.asarray(counts(gt01, rows), dtype=np.int64)
        preds = np.stack([np.load(p)[args.obs_length:T] for p in used[idx]])                         # uint8: (x / 255 * 255) is x
        pred_counts[:, i] = np.asarray(counts(torch.from_numpy(preds.reshape((-1,) + want[1:])), rows),
                                       dtype=np.int64).reshape(num_samples, n_frames)

    _, *gt_ind = classify(smooth_counts(gt_counts), entry_thresh, out_thresh)                        # :252-256
    members = class_members(*gt_ind)
    print("Num examples Class 1:", len(members[0]))
    print("Num examples Class 2:", len(members[1]))
    print("Num examples Class 3:", len(members[2]))
    print("3-class accuracies:")
    gt_acc = three_class_accuracy(members, gt_ind)
    print("{} : acc={}/{} = {}%".format("GT", three_class_count(members, gt_ind), len(keys), gt_acc * 100))
    acc_list, pred_ind = [], []
    for k in range(num_samples):                                                                     # :272-290
        _, *ind = classify(smooth_counts(pred_counts[k]), entry_thresh, out_thresh)
        pred_ind.append(ind)
        acc_list.append(three_class_accuracy(members, ind))
    with np.errstate(all="ignore"):                                                                  # one sample: 0 / 0, as there
        mean, max_ = float(np.mean(acc_list)), float(np.max(acc_list))
        stderr = float(np.std(acc_list) / np.sqrt(num_samples - 1))
    print(f"{mean * 100}% +- {stderr * 100}")
    print(f"{max_ * 100}%")

    as_dict = lambda ind: {c: [int(v) for v in m] for c, m in zip(CLASSES, ind)}  # noqa: E731
    result = dict(num_videos=len(keys), num_samples=num_samples, T=int(T), obs_length=int(args.obs_length), rows=list(rows),
                  entry_thresh=entry_thresh, out_thresh=out_thresh, videos=[int(k) for k in keys],
                  class_sizes={c: int(len(m)) for c, m in zip(CLASSES, members)},
                  gt_accuracy=float(gt_acc), accuracies=[float(a) for a in acc_list], mean=mean, stderr=stderr, max=max_,
                  gt_indicators=as_dict(gt_ind), sample_indicators=[as_dict(ind) for ind in pred_ind])
    if getattr(args, "out", None):
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
        print(f"Saved the result to {args.out}.")
    return result


def main(argv=None):
    from .script_util import str2bool
    ap = argparse.ArgumentParser(description="3-class accuracy (room stay / hallway enter+stay / hallway enter+recover) of the "
                                             "GQN-Mazes samples under <eval_dir>/samples against their ground truth")
    ap.add_argument("--eval_dir", type=str, required=True)
    ap.add_argument("--obs_length", type=int, default=36, help="Number of observed frames. Default is 36.")
    ap.add_argument("--num_samples", type=int, default=5, help="sample indices 0 .. num_samples-1 of every video are scored")
    ap.add_argument("--T", type=int, default=None, help="Video length. If not given, the samples' length.")
    ap.add_argument("--videos", default=None, help=".npy file of the test videos (N, T, 3, H, W): float in [-1, 1] or uint8")
    ap.add_argument("--synthetic", type=str2bool, nargs="?", const=True, default=True,
                    help="without --videos: the synthetic videos the sampling CLIs draw (item i seeded by i)")
    ap.add_argument("--num_videos", type=int, default=None, help="size of the synthetic dataset (default: up to the last sampled video)")
    ap.add_argument("--entry_thresh", type=float, default=None, help=f"smoothed count above which the agent is in the hallway ({ENTRY_THRESH})")
    ap.add_argument("--out_thresh", type=float, default=None, help=f"smoothed count at or below which it has left ({OUT_THRESH})")
    ap.add_argument("--rows", type=int, nargs=2, default=None, metavar=("FIRST", "LAST_PLUS_1"),
                    help=f"rows of a frame that are searched for green (default {ROWS[0]} {ROWS[1]}: 64 x 64 Mazes frames)")
    ap.add_argument("--out", default=None, metavar="PATH", help="write the result as JSON")
    return run(ap.parse_args(argv))


if __name__ == "__main__":
    main()
