"""Time the three video_eval metrics of one video on the GPU, and the same frames' SSIM / PSNR through the float32 scipy
restatement (tests/metrics_restated.py: what the reference's scikit-image does) on this box's CPU cores, in one run:

  v64:  300 frames of 64 x 64, 3 channels      v128: 500 frames of 128 x 128, 3 channels

GPU: ground truth (float32 in [0, 1]) and sample (uint8) resident on the device, as video_eval holds them; HIP events, median of
--reps runs after warm-up, for csrc/metrics.hip (SSIM + PSNR), for LpipsAlex.distance (mapping to [-1, 1], both embeddings, the paired
distance) and for all three; the upload of both videos and the read-back are timed on the wall clock beside them.  CPU: every frame's
three planes through `frame_ssim_psnr(dtype=float32)` on --workers processes (started before the GPU is opened).  Synthetic seeded
weights and frames.  One JSON line per case; not a pass/fail gate.

  python tools/eval_bench.py [--cases v64,v128] [--reps 10] [--workers 16] [--out profiles/eval_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np      # noqa: E402

CASES = {"v64": dict(H=64, frames=300), "v128": dict(H=128, frames=500)}


def make_video(name):
    c = CASES[name]
    g = np.random.default_rng(c["H"])
    gt = g.random((c["frames"], 3, c["H"], c["H"])).astype(np.float32)
    pred = (np.clip(gt + 0.1 * g.standard_normal(gt.shape), 0, 1) * 255).astype(np.uint8)
    return gt, pred


def _cpu_chunk(job):
    import metrics_restated as mr
    gt, pred = job
    return mr.frame_ssim_psnr(gt, pred, 2.0, np.float32)


def cpu_time(pool, workers, gt, pred):
    jobs = [(gt[k::workers], pred[k::workers]) for k in range(workers)]
    list(pool.map(_cpu_chunk, jobs[:workers]))                               # warm: imports, page faults
    t0 = time.perf_counter()
    res = list(pool.map(_cpu_chunk, jobs))
    dt = time.perf_counter() - t0
    ssim = np.empty(gt.shape[0])
    for k, (s, _) in enumerate(res):
        ssim[k::workers] = s
    return dt, ssim


def gpu_time(name, gt, pred, reps, ssim_cpu):
    import torch
    import video_diffusion_amd  # noqa: F401
    from lpips_restated import synth_weights
    from video_diffusion_amd.lpips import LpipsAlex, canonical_weights
    from video_diffusion_amd.metrics import frame_ssim_psnr_device
    dev = torch.device("cuda", 0)
    w = synth_weights(0)
    feat = (0, 3, 6, 8, 10)
    sd = {f"features.{feat[k]}.{p}": w[f"conv{k + 1}.{p}"] for k in range(5) for p in ("weight", "bias")}
    sd.update({f"lin{k}.model.1.weight": w[f"lin{k + 1}"].view(1, -1, 1, 1) for k in range(5)})
    emb = LpipsAlex(canonical_weights(sd), dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g, p = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
    torch.cuda.synchronize()
    h2d = time.perf_counter() - t0
    c255 = torch.full((), 255.0, device=dev)

    def sp():
        return frame_ssim_psnr_device(g, p, 2.0)

    def lp():
        return emb.distance(g * 2 - 1, p.to(torch.float32) / c255 * 2 - 1)

    def both():
        s, q = sp()
        d = lp()
        return s.cpu(), q.cpu(), d

    def timed(fn):
        fn()
        fn()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms))
    ms_sp, ms_lp, ms_all = timed(sp), timed(lp), timed(both)
    ssim = sp()[0].cpu().numpy()
    return {"gpu_ssim_psnr_ms": round(ms_sp, 4), "gpu_lpips_ms": round(ms_lp, 3), "gpu_all_three_ms": round(ms_all, 3),
            "h2d_both_videos_ms": round(h2d * 1e3, 3), "max_abs_ssim_gpu_minus_cpu_float32": float(np.abs(ssim - ssim_cpu).max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="v64,v128")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    names = [n for n in args.cases.split(",") if n]
    videos = {n: make_video(n) for n in names}
    cpu = {}
    with ProcessPoolExecutor(max_workers=args.workers) as pool:              # before the GPU is opened: the workers are forked clean
        for n in names:
            cpu[n] = cpu_time(pool, args.workers, *videos[n])
    lines = []
    for n in names:
        gt, pred = videos[n]
        rec = {"case": n, "frames": int(gt.shape[0]), "H": int(gt.shape[2]), "W": int(gt.shape[3]), "channels": 3, "reps": args.reps,
               "cpu_workers": args.workers, "cpu_ssim_psnr_float32_ms": round(cpu[n][0] * 1e3, 2)}
        rec.update(gpu_time(n, gt, pred, args.reps, cpu[n][1]))
        rec["cpu_over_gpu_ssim_psnr"] = round(rec["cpu_ssim_psnr_float32_ms"] / rec["gpu_ssim_psnr_ms"], 1)
        rec["cpu_ssim_psnr_over_gpu_all_three"] = round(rec["cpu_ssim_psnr_float32_ms"] / rec["gpu_all_three_ms"], 2)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
