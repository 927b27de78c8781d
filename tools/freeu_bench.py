#!/usr/bin/env python3
"""What FreeU costs per step beside the plain step.  One process, one GPU, the window executor (one captured graph per setting).

The default 116 M model at 64 x 64, the headline window B = 8 x T = 16 with 4 observed frames ('x_0'), schedule ddim250, sampler
'ddim' (eta = 0): per round each window is armed at the last index and --steps-per-round steps are replayed between two device events;
FreeU off (the step as it always was), on in the plain form and on in the adaptive form -- b = (1.4, 1.2), s = (0.6, 0.8): every pass of
both stages runs -- alternate round by round in the one process; the median of --rounds rounds after --warmup, in ms per step.

Nobody had measured the cost: the figures are reported, there is no bar and the exit status is 0.  What the passes move: per output
block of the two lowest levels one read and one write of h and of the skip tensor, and the GroupNorm statistics pass the block's first
norm now runs over both (their producers' tables do not describe the modified values).  One JSON line, to stdout and to --out.

    python tools/freeu_bench.py [--rounds 10] [--warmup 3] [--steps-per-round 10] [--out profiles/freeu_bench.jsonl]
"""
import argparse
import contextlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, T, N_OBS = 8, 16, 4
CONSTS = (1.4, 1.2, 0.6, 0.8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps-per-round", type=int, default=10)
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
    scopes = {"off": lambda: contextlib.nullcontext(), "plain": lambda: diff.freeu_scope(model, *CONSTS),
              "adaptive": lambda: diff.freeu_scope(model, *CONSTS, adaptive=True)}
    times = {name: [] for name in scopes}
    for i in range(args.warmup + args.rounds):
        for name, scope in scopes.items():
            with scope():
                ex.begin(x_T, kw, sampler="ddim", eta=0.0, seed=0)
            ex.run(1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            ex.run(k)
            e1.record()
            e1.synchronize()
            if i >= args.warmup:
                times[name].append(e0.elapsed_time(e1) / k)
    model.check_device_errors()
    med = {name: sorted(v)[len(v) // 2] for name, v in times.items()}
    line = dict(case="step", shape=f"B{B}xT{T}", B=B, T=T, observed=N_OBS, image_size=S, schedule="ddim250", sampler="ddim",
                rounds=args.rounds, warmup=args.warmup, steps_per_round=k, freeu=list(CONSTS), graphs=ex.graphs,
                off_ms=round(med["off"], 4), plain_ms=round(med["plain"], 4), adaptive_ms=round(med["adaptive"], 4),
                plain_over_off=round(med["plain"] / med["off"], 4), adaptive_over_off=round(med["adaptive"] / med["off"], 4),
                min_ms={n: round(min(v), 4) for n, v in times.items()}, max_ms={n: round(max(v), 4) for n, v in times.items()},
                spread={n: round((max(v) - min(v)) / med[n], 4) for n, v in times.items()})
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
