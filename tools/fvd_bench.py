"""Time the I3D embedding of one video on the GPU (fvd.I3D.embed, csrc/i3d.hip), and the float32 plain-torch restatement of the same
network (tests/i3d_restated.py) on this box's CPU threads, in one run:

  t100_64: 100 frames of 64 x 64      t300_64: 300 frames of 64 x 64      t500_128: 500 frames of 128 x 128

GPU: the uint8 video resident on the device; HIP events, median of --reps runs after warm-up.  The line carries the floating-point
operations of the 57 convolutions and the logits layer counted from the shapes (fvd.conv_flops, 2 per multiply-add), the achieved
FLOP/s and its share of the 157 TFLOP/s fp32-MFMA peak for the convolutions as a class (resize, pools and tail are inside the time, not
inside the count).  CPU: `embed_restated` of the same video with float32 weights and activations on --threads threads, once
(--cpu_frames N times its first N frames only, and the line says so).  Synthetic seeded weights and frames.  One JSON line per case; not a pass/fail gate.

  python tools/fvd_bench.py [--cases t100_64,t300_64,t500_128] [--reps 5] [--threads 16] [--out profiles/fvd_bench.jsonl]
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

CASES = {"t100_64": dict(T=100, H=64), "t300_64": dict(T=300, H=64), "t500_128": dict(T=500, H=128)}
PEAK_FP32_MFMA = 157e12


def make_video(name):
    c = CASES[name]
    g = np.random.default_rng(c["T"] + c["H"])
    return g.integers(0, 256, (c["T"], 3, c["H"], c["H"]), dtype=np.uint8)


def cpu_time(video, sd32, threads, max_frames):
    import torch
    import i3d_restated as ir
    torch.set_num_threads(threads)
    v = torch.from_numpy(video[:max_frames] if max_frames else video)
    t0 = time.perf_counter()
    out = ir.embed_restated(v, sd32, dtype=torch.float32)
    dt = time.perf_counter() - t0
    return dt, int(v.shape[0]), out.to(torch.float64)


def gpu_time(video, sd, reps):
    import torch
    from video_diffusion_amd.fvd import I3D
    dev = torch.device("cuda", 0)
    emb = I3D.from_state_dict(sd, dev)
    v = torch.from_numpy(video)[None].to(dev)
    emb.embed(v)
    emb.embed(v)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = emb.embed(v)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), out[0].cpu().to(torch.float64), emb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="t100_64,t300_64,t500_128")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--cpu_frames", type=int, default=0, help="0: the whole video")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import i3d_restated as ir
    import video_diffusion_amd  # noqa: F401
    from video_diffusion_amd.fvd import conv_flops
    sd = ir.synth_state_dict(0)
    lines = []
    for n in [c for c in args.cases.split(",") if c]:
        video = make_video(n)
        T, H = CASES[n]["T"], CASES[n]["H"]
        cpu_s, cpu_T, cpu_out = cpu_time(video, sd, args.threads, args.cpu_frames)
        ms, out, emb = gpu_time(video, sd, args.reps)
        flops = conv_flops(T)
        rec = {"case": n, "frames": T, "H": H, "W": H, "reps": args.reps, "gpu_embed_ms": round(ms, 3), "conv_gflop": round(flops / 1e9, 2),
               "conv_tflops_achieved": round(flops / (ms * 1e-3) / 1e12, 2),
               "share_of_fp32_mfma_peak_157": round(flops / (ms * 1e-3) / PEAK_FP32_MFMA, 4),
               "cpu_threads": args.threads, "cpu_float32_torch_frames": cpu_T, "cpu_float32_torch_s": round(cpu_s, 2),
               "cpu_float32_torch_gflops": round(conv_flops(cpu_T) / cpu_s / 1e9, 1)}
        if cpu_T == T:
            rec["max_abs_logit_gpu_minus_cpu_float32"] = float((out - cpu_out).abs().max())
        del emb
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
