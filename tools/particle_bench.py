#!/usr/bin/env python3
"""What particle steering adds to a step.  One process, one GPU, the window executor (one captured graph per configuration).

The default 116 M model at 64 x 64, the headline window B = 8 x T = 16 with 4 observed frames ('x_0') run as ONE group of K = 8
particles, schedule ddim250, sampler 'p_sample', the built-in reward of a 4 x 4 cell-mean measurement ('sr4'): per round each window is
armed at the last index and --steps-per-round steps are replayed between two device events; the plain step and the steered step
alternate round by round in the one process; the median of --rounds rounds after --warmup, in ms per step, and the steering's cost
over the plain step.  ess_threshold = 1, so that every step resamples: the gather moves what it can ever move.

The steered step appends three launches behind the sampler pass: the residual pass (reads the 6.3 MB sample and x_0 prediction), the
weights (one block) and the gather of both tensors (at most four times their bytes).  The expectation is what the known-region merge
and the DPS residual pass cost together: tens of microseconds beside a UNet forward.  No bar is set: what is measured is recorded next
to the plain step of the same process.  One JSON line, to stdout and to --out.

    python tools/particle_bench.py [--rounds 10] [--warmup 3] [--steps-per-round 10] [--out profiles/particle_bench.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, T, N_OBS = 8, 16, 4


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
    truth = x0.clone()
    x0[:, N_OBS:] = 0
    x0 = x0.to(dev)
    x_T = torch.randn(B, T, 3, S, S, generator=g).to(dev)
    obs = torch.zeros(B, T, 1, 1, 1, device=dev)
    obs[:, :N_OBS] = 1
    kw = dict(frame_indices=torch.arange(T, device=dev).view(1, T).repeat(B, 1), x0=x0, obs_mask=obs, latent_mask=1 - obs,
              kinda_marg_mask=torch.zeros_like(obs), x_t_minus_1=x0, observed_frames="x_0")
    from video_diffusion_amd.gaussian_diffusion import measure
    y = measure(truth[:1], 4, False)                        # one video, K = 8 particles: every item carries the same measurement
    y = (y + 0.1 * torch.randn(y.shape, generator=g)).repeat(B, 1, 1, 1, 1).to(dev)

    ex = WindowExecutor(model, diff)
    k = args.steps_per_round
    region = dict(plain={}, steered=dict(particles=B, particle_measurement=y, particle_sr_scale=4, sigma_y=0.5, ess_threshold=1.0))
    times = {name: [] for name in region}
    resamples = 0

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()                                                # (run / jump make the current stream wait for the executor's)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for i in range(args.warmup + args.rounds):
        for name, kn in region.items():
            ex.begin(x_T, kw, sampler="p_sample", seed=0, **kn)
            ex.run(1)
            ms = timed(lambda: ex.run(k)) / k
            if i >= args.warmup:
                times[name].append(ms)
            if kn:
                resamples = int(ex.particle_state()["resamples"][0])
    model.check_device_errors()
    med = {name: sorted(v)[len(v) // 2] for name, v in times.items()}
    line = dict(case="step", shape=f"B{B}xT{T}", B=B, T=T, observed=N_OBS, image_size=S, schedule="ddim250", sampler="p_sample",
                particles=B, groups=1, reward="sr4", ess_threshold=1.0, rounds=args.rounds, warmup=args.warmup, steps_per_round=k,
                resamples_last_round=resamples, of_steps=k + 1,
                ms={name: round(m, 4) for name, m in med.items()}, added_ms=round(med["steered"] - med["plain"], 4),
                added_fraction=round(med["steered"] / med["plain"] - 1.0, 5),
                spread={name: round((max(v) - min(v)) / med[name], 4) for name, v in times.items()})
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
