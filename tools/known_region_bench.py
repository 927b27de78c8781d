#!/usr/bin/env python3
"""What a known region (pixel-mask inpainting) adds to a step.  One process, one GPU, the window executor (one captured graph per
configuration).

The default 116 M model at 64 x 64, the headline window B = 8 x T = 16 with 4 observed frames ('x_0'), schedule ddim250, sampler
'ddim' (eta = 0), half of every latent frame known: per round each window is armed at the last index and --steps-per-round steps are
replayed between two device events; the plain step and the step with the merge pass alternate round by round in the one process; the
median of --rounds rounds after --warmup, in ms per step, and the merge's cost over the plain step.  One vd_window_jump (three plain
launches: the jump kernel between two counter kernels) is timed the same way, one jump per round.

The merge is one more elementwise launch over at most the 6.3 MB sample (read mask, source and sample, write the sample) beside a UNet
forward.  No bar is set: what is measured is recorded next to the unmerged step of the same process.  One JSON line, to stdout and to
--out.

    python tools/known_region_bench.py [--rounds 10] [--warmup 3] [--steps-per-round 10] [--out profiles/known_region_bench.jsonl]
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
    known_src = x0.clone().to(dev)
    x0[:, N_OBS:] = 0
    x0 = x0.to(dev)
    x_T = torch.randn(B, T, 3, S, S, generator=g).to(dev)
    obs = torch.zeros(B, T, 1, 1, 1, device=dev)
    obs[:, :N_OBS] = 1
    kw = dict(frame_indices=torch.arange(T, device=dev).view(1, T).repeat(B, 1), x0=x0, obs_mask=obs, latent_mask=1 - obs,
              kinda_marg_mask=torch.zeros_like(obs), x_t_minus_1=x0, observed_frames="x_0")
    known_mask = torch.zeros(B, T, S, S, device=dev)
    known_mask[:, :, :, : S // 2] = 1                       # the left half of every frame (the merge acts on the latent ones)

    ex = WindowExecutor(model, diff)
    k = args.steps_per_round
    region = dict(plain={}, merged=dict(known_src=known_src, known_mask=known_mask))
    times = {name: [] for name in region}
    jump = []

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
            ex.begin(x_T, kw, sampler="ddim", eta=0.0, seed=0, **kn)
            ex.run(1)
            ms = timed(lambda: ex.run(k)) / k
            if i >= args.warmup:
                times[name].append(ms)
            if kn:
                ms = timed(lambda: ex.jump(1))
                if i >= args.warmup:
                    jump.append(ms)
    model.check_device_errors()
    med = {name: sorted(v)[len(v) // 2] for name, v in times.items()}
    line = dict(case="step", shape=f"B{B}xT{T}", B=B, T=T, observed=N_OBS, image_size=S, schedule="ddim250", sampler="ddim",
                known_fraction=0.5, rounds=args.rounds, warmup=args.warmup, steps_per_round=k,
                ms={name: round(m, 4) for name, m in med.items()}, added_ms=round(med["merged"] - med["plain"], 4),
                added_fraction=round(med["merged"] / med["plain"] - 1.0, 5), window_jump_ms=round(sorted(jump)[len(jump) // 2], 4),
                spread={name: round((max(v) - min(v)) / med[name], 4) for name, v in times.items()})
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
