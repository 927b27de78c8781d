#!/usr/bin/env python3
"""What guidance rescale and dynamic thresholding add to a guided step.  One process, one GPU, the window executor (one captured graph
per configuration).

The default 116 M model at 64 x 64, the headline window B = 8 x T = 16 with 4 observed frames ('x_0'), schedule ddim250, sampler
'ddim' (eta = 0): per round each window is armed at the last index and --steps-per-round steps are replayed between two device events;
the five configurations -- cfg_scale = 2 alone, with the rescale (phi = 0.7), with the threshold (p = 0.995), with both, and
cfg_scale = 1 with the threshold -- alternate round by round in the one process; the median of --rounds rounds after --warmup, in ms
per step, and each configuration's cost over its base (cfg_scale = 2 alone; for the last one the plain step, measured as a sixth).

The added passes move a few times the 6.3 MB network output against one or two UNet forwards: the expectation is well under 1 % of
the step.  The rescale is 2 launches in place of the combine pass' 1, the threshold 11 small launches (zeroing the counters, the x_0
pass, three histogram passes, four one-block-per-item scans, the apply pass).  One JSON line, to stdout and to --out.

    python tools/guidance_bench.py [--rounds 10] [--warmup 3] [--steps-per-round 10] [--out profiles/guidance_bench.jsonl]
"""
import argparse
import contextlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, T, N_OBS = 8, 16, 4
PHI, P = 0.7, 0.995
# name -> (cfg_scale, cfg_rescale, dynamic_threshold)
CONFIGS = {"cfg2": (2.0, 0.0, None), "cfg2_rescale": (2.0, PHI, None), "cfg2_threshold": (2.0, 0.0, P), "cfg2_both": (2.0, PHI, P),
           "cfg1": (1.0, 0.0, None), "cfg1_threshold": (1.0, 0.0, P)}
BASE = {"cfg2_rescale": "cfg2", "cfg2_threshold": "cfg2", "cfg2_both": "cfg2", "cfg1_threshold": "cfg1"}


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
    times = {name: [] for name in CONFIGS}
    for i in range(args.warmup + args.rounds):
        for name, (w, phi, p) in CONFIGS.items():
            scope = diff.guidance_scope(model, cfg_rescale=phi, dynamic_threshold=p) if (phi or p) else contextlib.nullcontext()
            with scope:
                ex.begin(x_T, kw, sampler="ddim", eta=0.0, seed=0, cfg_scale=w)
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
                rounds=args.rounds, warmup=args.warmup, steps_per_round=k, cfg_rescale=PHI, dynamic_threshold=P,
                ms={name: round(m, 4) for name, m in med.items()},
                added_ms={name: round(med[name] - med[base], 4) for name, base in BASE.items()},
                added_fraction={name: round(med[name] / med[base] - 1.0, 5) for name, base in BASE.items()},
                spread={name: round((max(v) - min(v)) / med[name], 4) for name, v in times.items()})
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
