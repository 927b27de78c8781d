#!/usr/bin/env python3
"""What a cfg_scale = 2 step costs beside the unguided step.  One process, one GPU, the window executor (one captured graph per scale).

The default 116 M model at 64 x 64, the headline window B = 8 x T = 16 with 4 observed frames ('x_0'), schedule ddim250, sampler
'ddim' (eta = 0): per round each window is armed at the last index and --steps-per-round steps are replayed between two device events;
cfg_scale = 1 (one forward: the step as it always was) and cfg_scale = 2 (two forwards, the combine pass) alternate round by round in
the one process; the median of --rounds rounds after --warmup, in ms per step.

The bar: the guided step costs at most 2.02 x the unguided step of the same process -- two forwards, and a combine pass that moves
three tensors of B*T*3*H*W floats, microseconds against a forward; the 2 % is the margin tools/schedule_bench.py uses for
same-process ratios.  One JSON line, to stdout and to --out; the exit status is 1 when the ratio is above the bar.

    python tools/cfg_bench.py [--rounds 10] [--warmup 3] [--steps-per-round 10] [--out profiles/cfg_bench.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, T, N_OBS = 8, 16, 4
BAR = 2.02


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps-per-round", type=int, default=10)
    ap.add_argument("--cfg-scale", type=float, default=2.0)
    ap.add_argument("--image-size", type=int, default=64)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    import video_diffusion_amd as vda
    from video_diffusion_amd.executor import WindowExecutor
    dev = torch.device("cuda:0")
    S = args.image_size
    cfg = vda.video_model_and_diffusion_defaults()
    cfg.update(T=T, image_size=S, rp_alpha=T, rp_beta=T, rp_gamma=T, timestep_respacing="ddim250")
    model, diff = vda.create_video_model_and_diffusion(**cfg)
    model.load_state_dict({k: torch.from_numpy(vda.weights_init.synth_param(k, s)) for k, s in model.param_specs()})
    model.to(dev).eval()
    g = torch.Generator().manual_seed(1234)
    x0 = torch.rand(B, T, 3, S, S, generator=g) * 2 - 1
    x0[:, N_OBS:] = 0
    x0 = x0.to(dev)
    x_T = torch.randn(B, T, 3, S, S, generator=g).to(dev)
    obs = torch.zeros(B, T, 1, 1, 1, device=dev)
    obs[:, :N_OBS] = 1
    kw = dict(frame_indices=torch.arange(T, device=dev).view(1, T).repeat(B, 1), x0=x0, obs_mask=obs, latent_mask=1 - obs,
              kinda_marg_mask=torch.zeros_like(obs), x_t_minus_1=x0, observed_frames="x_0")

    ex = WindowExecutor(model, diff)
    k = args.steps_per_round
    scales = (1.0, args.cfg_scale)
    times = {w: [] for w in scales}
    for i in range(args.warmup + args.rounds):
        for w in scales:
            ex.begin(x_T, kw, sampler="ddim", eta=0.0, seed=0, cfg_scale=w)
            ex.run(1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            ex.run(k)
            e1.record()
            e1.synchronize()
            if i >= args.warmup:
                times[w].append(e0.elapsed_time(e1) / k)
    model.check_device_errors()
    med = {w: sorted(v)[len(v) // 2] for w, v in times.items()}
    ratio = med[args.cfg_scale] / med[1.0]
    line = dict(case="step", shape=f"B{B}xT{T}", B=B, T=T, observed=N_OBS, image_size=S, schedule="ddim250", sampler="ddim",
                rounds=args.rounds, warmup=args.warmup, steps_per_round=k, cfg_scale=args.cfg_scale,
                unguided_ms=round(med[1.0], 4), guided_ms=round(med[args.cfg_scale], 4), guided_over_unguided=round(ratio, 4), bar=BAR,
                within_bar=bool(ratio <= BAR),
                min_ms={str(w): round(min(v), 4) for w, v in times.items()}, max_ms={str(w): round(max(v), 4) for w, v in times.items()},
                spread={str(w): round((max(v) - min(v)) / med[w], 4) for w, v in times.items()})
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    return 0 if ratio <= BAR else 1


if __name__ == "__main__":
    sys.exit(main())
