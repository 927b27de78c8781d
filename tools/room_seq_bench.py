"""Time the green-hallway pixel count of a Mazes evaluation on the GPU, and the same frames through the numpy restatement
(tests/hallway_restated.py: the adopted OpenCV arithmetic, one frame at a time as the reference walks them) on one CPU core:

  8 videos x 6 sequences (1 ground truth + 5 samples) x 264 frames of 64 x 64, rows 14:45

GPU: the frames resident on the device as uint8, as video_eval_room_seq_acc holds a video's samples; the one launch of
csrc/hallway.hip over all 12672 frames timed with HIP events, median of --reps runs after warm-up; the upload and the read-back of the
counts are timed on the wall clock beside it.  The counts of both sides must be equal.  One JSON line; not a pass/fail gate.

  python tools/room_seq_bench.py [--reps 10] [--out profiles/room_seq_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np      # noqa: E402

VIDEOS, SEQUENCES, FRAMES, SIZE, ROWS = 8, 6, 264, 64, (14, 45)


def make_frames():
    """Noise with a green band whose height wanders per sequence, so that the counts cover 0 .. the whole strip."""
    g = np.random.default_rng(64)
    n = VIDEOS * SEQUENCES * FRAMES
    frames = g.integers(0, 256, size=(n, 3, SIZE, SIZE), dtype=np.uint8)
    heights = np.clip(np.cumsum(g.integers(-2, 3, size=(VIDEOS * SEQUENCES, FRAMES)), axis=1) + 12, 0, 40).reshape(-1)
    for f, h in zip(frames, heights):
        f[0, 10:10 + h], f[1, 10:10 + h], f[2, 10:10 + h] = 20, 230, 40
    return frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import hallway_restated as hr
    frames = make_frames()
    hr.counts(frames[:64], ROWS)                                              # warm: imports, page faults
    t0 = time.perf_counter()
    want = hr.counts(frames, ROWS)
    cpu_ms = (time.perf_counter() - t0) * 1e3

    import torch
    import video_diffusion_amd  # noqa: F401
    from video_diffusion_amd.hallway import hallway_counts_device
    dev = torch.device("cuda", 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    d = torch.from_numpy(frames).to(dev)
    torch.cuda.synchronize()
    h2d_ms = (time.perf_counter() - t0) * 1e3
    hallway_counts_device(d, ROWS)
    hallway_counts_device(d, ROWS)
    ms = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = hallway_counts_device(d, ROWS)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    t0 = time.perf_counter()
    got = out.cpu().numpy()
    d2h_ms = (time.perf_counter() - t0) * 1e3
    gpu_ms = float(np.median(ms))
    strip_bytes = frames.shape[0] * 3 * (ROWS[1] - ROWS[0]) * SIZE
    rec = {"case": "mazes64", "videos": VIDEOS, "sequences_per_video": SEQUENCES, "frames_per_sequence": FRAMES, "H": SIZE, "W": SIZE,
           "rows": list(ROWS), "reps": args.reps, "gpu_counts_ms": round(gpu_ms, 4), "gpu_counts_ms_min": round(float(np.min(ms)), 4),
           "strip_GB_per_s": round(strip_bytes / (gpu_ms * 1e-3) / 1e9, 1), "h2d_frames_ms": round(h2d_ms, 3),
           "d2h_counts_ms": round(d2h_ms, 3), "cpu_numpy_restatement_1core_ms": round(cpu_ms, 1),
           "cpu_over_gpu": round(cpu_ms / gpu_ms, 1), "counts_equal": bool(np.array_equal(got, want)),
           "count_min": int(want.min()), "count_max": int(want.max())}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
