#!/usr/bin/env python3
"""What a dpmpp_2m_sample step costs beside a ddim_sample step, and a whole logsnr40 window beside a whole ddim250 window.
One process, one GPU, the window executor (one captured graph per sampler).

The default 116 M model at 64 x 64, the headline window B = 8 x T = 16 with 4 observed frames ('x_0'):

    step     schedule ddim250; per round each sampler's window is armed at the last index and --steps-per-round steps are replayed
             between two device events; 'ddim' (eta = 0) and 'dpmpp_2m' alternate round by round in the one process; the median of
             --rounds rounds after --warmup, in ms per step.  The 2M pass reads and writes one more tensor of B*T*3*H*W floats
             (the history) than the DDIM pass: the step should cost what a DDIM step costs.
    window   all 40 steps of a logsnr40 window with 'dpmpp_2m' and all 250 steps of a ddim250 window with 'ddim' (eta = 0), begin()
             included, host clock around a device synchronise; the median of --windows windows after one warm-up window each
             (a new schedule drops the captured graphs, so the two are timed one after the other, not interleaved).

No bar is set: one JSON line per case, to stdout and to --out.

    python tools/dpmpp_2m_bench.py [--rounds 10] [--warmup 3] [--steps-per-round 10] [--windows 3] [--out profiles/dpmpp_2m_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, T, N_OBS = 8, 16, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps-per-round", type=int, default=10)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--image-size", type=int, default=64)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()

    import torch
    import video_diffusion_amd as vda
    from video_diffusion_amd.executor import WindowExecutor
    from video_diffusion_amd.script_util import create_gaussian_diffusion
    dev = torch.device("cuda:0")
    S = args.image_size
    cfg = vda.video_model_and_diffusion_defaults()
    cfg.update(T=T, image_size=S, rp_alpha=T, rp_beta=T, rp_gamma=T, timestep_respacing="ddim250")
    model, diff250 = vda.create_video_model_and_diffusion(**cfg)
    model.load_state_dict({k: torch.from_numpy(vda.weights_init.synth_param(k, s)) for k, s in model.param_specs()})
    model.to(dev).eval()
    diff40 = create_gaussian_diffusion(steps=cfg["diffusion_steps"], noise_schedule=cfg["noise_schedule"],
                                       rescale_timesteps=cfg["rescale_timesteps"], timestep_respacing="logsnr40")
    g = torch.Generator().manual_seed(1234)
    x0 = torch.rand(B, T, 3, S, S, generator=g) * 2 - 1
    x0[:, N_OBS:] = 0
    x0 = x0.to(dev)
    x_T = torch.randn(B, T, 3, S, S, generator=g).to(dev)
    obs = torch.zeros(B, T, 1, 1, 1, device=dev)
    obs[:, :N_OBS] = 1
    kw = dict(frame_indices=torch.arange(T, device=dev).view(1, T).repeat(B, 1), x0=x0, obs_mask=obs, latent_mask=1 - obs,
              kinda_marg_mask=torch.zeros_like(obs), x_t_minus_1=x0, observed_frames="x_0")
    common = dict(shape=f"B{B}xT{T}", B=B, T=T, observed=N_OBS, image_size=S)
    lines = []

    # ---- one step, the two samplers interleaved
    ex = WindowExecutor(model, diff250)
    k = args.steps_per_round
    times = {"ddim": [], "dpmpp_2m": []}
    for i in range(args.warmup + args.rounds):
        for sampler in ("ddim", "dpmpp_2m"):
            ex.begin(x_T, kw, sampler=sampler, eta=0.0, seed=0)
            ex.run(1)                                                   # (the 2M window's first step has no history: keep it out of the timing)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            ex.run(k)
            e1.record()
            e1.synchronize()
            if i >= args.warmup:
                times[sampler].append(e0.elapsed_time(e1) / k)
    model.check_device_errors()
    med = {s: sorted(v)[len(v) // 2] for s, v in times.items()}
    line = dict(case="step", **common, schedule="ddim250", rounds=args.rounds, warmup=args.warmup, steps_per_round=k,
                ddim_ms=round(med["ddim"], 4), dpmpp_2m_ms=round(med["dpmpp_2m"], 4),
                dpmpp_2m_over_ddim=round(med["dpmpp_2m"] / med["ddim"], 4),
                min_ms={s: round(min(v), 4) for s, v in times.items()}, max_ms={s: round(max(v), 4) for s, v in times.items()})
    print(json.dumps(line), flush=True)
    lines.append(line)

    # ---- a whole window: 250 DDIM steps against 40 steps of the 2M sampler on logSNR-uniform steps
    whole = {}
    for name, diff, sampler in (("ddim250", diff250, "ddim"), ("logsnr40", diff40, "dpmpp_2m")):
        wex = WindowExecutor(model, diff)
        secs = []
        for i in range(1 + args.windows):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = wex.begin(x_T, kw, sampler=sampler, eta=0.0, seed=0).run()
            torch.cuda.synchronize()
            if i:
                secs.append(time.perf_counter() - t0)
        model.check_device_errors()
        assert torch.isfinite(out).all()
        whole[name] = dict(steps=diff.num_timesteps, sampler=sampler, window_s=round(sorted(secs)[len(secs) // 2], 4),
                           min_s=round(min(secs), 4), max_s=round(max(secs), 4))
    line = dict(case="window", **common, windows=args.windows, **{f"{n}_{k2}": v for n, d in whole.items() for k2, v in d.items()},
                logsnr40_over_ddim250=round(whole["logsnr40"]["window_s"] / whole["ddim250"]["window_s"], 4))
    print(json.dumps(line), flush=True)
    lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
