#!/usr/bin/env python3
"""What a dpmpp_2m_sde_sample step costs beside a ddim_sample step and a dpmpp_2m_sample step.  One process, one GPU, the window
executor (one captured graph per sampler).

The default 116 M model at 64 x 64, the headline window B = 8 x T = 16 with 4 observed frames ('x_0'), schedule logsnr80: per round each
sampler's window is armed at the last index, one step is replayed outside the timing (the first step of the two samplers with history
has none) and --steps-per-round steps are replayed between two device events; 'ddim' (eta = 1), 'dpmpp_2m' and 'dpmpp_2m_sde' alternate
round by round in the one process; the median of --rounds rounds after --warmup, in ms per step.  Each step is the same forward plus one
streaming launch (the SDE pass reads the history as 2M does and draws Philox noise as DDIM does): the expectation -- not a gate -- is
that the three are equal within the spread of the rounds.

One JSON line, to stdout and to --out.

    python tools/dpmpp_2m_sde_bench.py [--rounds 10] [--warmup 3] [--steps-per-round 10] [--out profiles/dpmpp_2m_sde_bench.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, T, N_OBS = 8, 16, 4
SAMPLERS = ("ddim", "dpmpp_2m", "dpmpp_2m_sde")


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
    cfg.update(T=T, image_size=S, rp_alpha=T, rp_beta=T, rp_gamma=T, timestep_respacing="logsnr80")
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
    assert 1 + k <= diff.num_timesteps
    times = {s: [] for s in SAMPLERS}
    for i in range(args.warmup + args.rounds):
        for sampler in SAMPLERS:
            ex.begin(x_T, kw, sampler=sampler, eta=1.0, seed=0)
            ex.run(1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            ex.run(k)
            e1.record()
            e1.synchronize()
            if i >= args.warmup:
                times[sampler].append(e0.elapsed_time(e1) / k)
    model.check_device_errors()
    assert torch.isfinite(ex.x).all()
    med = {s: sorted(v)[len(v) // 2] for s, v in times.items()}
    line = dict(case="step", shape=f"B{B}xT{T}", B=B, T=T, observed=N_OBS, image_size=S, schedule="logsnr80", rounds=args.rounds,
                warmup=args.warmup, steps_per_round=k, **{f"{s}_ms": round(med[s], 4) for s in SAMPLERS},
                dpmpp_2m_sde_over_ddim=round(med["dpmpp_2m_sde"] / med["ddim"], 4),
                dpmpp_2m_sde_over_dpmpp_2m=round(med["dpmpp_2m_sde"] / med["dpmpp_2m"], 4),
                min_ms={s: round(min(v), 4) for s, v in times.items()}, max_ms={s: round(max(v), 4) for s, v in times.items()})
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
