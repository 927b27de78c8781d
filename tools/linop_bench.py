#!/usr/bin/env python3
"""What the separable linear operator (csrc/linop.hip) costs beside the hand-built cell mean, in the exact projection and in the DPS
step.  One process, one GPU, the eager executor.

The default 116 M model at 64 x 64, the headline window B = 8 x T = 16 with 4 observed frames ('x_0'), schedule ddim250, t = 125.  Five
steps alternate round by round in the one process, each timed between two device events after --warmup rounds; the median of --rounds
rounds, in ms per step, and the spread (max - min) / median of each:
  plain        the p_sample step (one forward, the sampler pass);
  measurement  the measurement_scope step under the x4 cell mean (sr4): one projection pass in front of the sampler pass;
  linear       the linear_measurement_scope step under bicubic x4 (resize_matrix(64, 16)): linop.hip's residual and projection passes;
  dps          the dps_scope step under sr4: taped forward, residual and seed passes, backward-data pass, final pass;
  linear_dps   the linear_dps_scope step under bicubic x4: the same, with linop.hip's two passes.
No bar is set.  One JSON line, to stdout and to --out.

    python tools/linop_bench.py [--rounds 10] [--warmup 3] [--steps-per-round 3] [--out profiles/linop_bench.jsonl]
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
    ap.add_argument("--steps-per-round", type=int, default=3)
    ap.add_argument("--image-size", type=int, default=64)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    import video_diffusion_amd as vda
    from video_diffusion_amd.gaussian_diffusion import measure_separable, resize_matrix
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
    x_t = torch.randn(B, T, 3, S, S, generator=g).to(dev)
    noise = torch.randn(B, T, 3, S, S, generator=g).to(dev)
    obs = torch.zeros(B, T, 1, 1, 1, device=dev)
    obs[:, :N_OBS] = 1
    kw = dict(frame_indices=torch.arange(T, device=dev).view(1, T).repeat(B, 1), x0=x0, obs_mask=obs, latent_mask=1 - obs,
              kinda_marg_mask=torch.zeros_like(obs), x_t_minus_1=x0, observed_frames="x_0")
    A = resize_matrix(S, S // 4)
    jitter = 0.05 * torch.randn(B, T, 3, S // 4, S // 4, generator=g)
    y_sr = (diff.measure(truth, 4, False) + jitter).to(dev)
    y_lin = (measure_separable(truth, A, A) + jitter).to(dev)
    t = torch.tensor([125] * B, device=dev)
    k = args.steps_per_round

    def plain():
        diff._fused_step(0, model, x_t, t, True, kw, noise=noise)

    def moved():                                                # inside a DPS scope: the plain step, then the scope's move
        diff._step(0, model, x_t, t, True, None, kw, 0.0, noise)

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    # every scope is entered afresh around its timed steps: the engine holds one projection at a time, and a scope's entry (two small
    # host-to-device copies for the matrices) is outside the events
    scopes = dict(plain=(lambda: _null(), plain), measurement=(lambda: diff.measurement_scope(model, y_sr, 4), plain),
                  linear=(lambda: diff.linear_measurement_scope(model, y_lin, A, A), plain),
                  dps=(lambda: diff.dps_scope(model, y_sr, 4, zeta=0.5), moved),
                  linear_dps=(lambda: diff.linear_dps_scope(model, y_lin, A, A, zeta=0.5), moved))
    times = {name: [] for name in scopes}
    for i in range(args.warmup + args.rounds):
        for name, (scope, fn) in scopes.items():
            with scope():
                ms = timed(fn, k)
            if i >= args.warmup:
                times[name].append(ms)
    model.check_device_errors()

    med = {name: sorted(v)[len(v) // 2] for name, v in times.items()}
    line = dict(case="linop_step", shape=f"B{B}xT{T}", B=B, T=T, observed=N_OBS, image_size=S, schedule="ddim250", t=125, sampler="p_sample",
                operators=dict(measurement="sr4", dps="sr4", linear=f"bicubic{S}to{S // 4}", linear_dps=f"bicubic{S}to{S // 4}"),
                rounds=args.rounds, warmup=args.warmup, steps_per_round=k, ms={name: round(m, 4) for name, m in med.items()},
                linear_over_measurement=round(med["linear"] / med["measurement"], 5), linear_dps_over_dps=round(med["linear_dps"] / med["dps"], 5),
                linear_minus_plain_ms=round(med["linear"] - med["plain"], 4),
                spread={name: round((max(v) - min(v)) / med[name], 4) for name, v in times.items()})
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    return 0


def _null():
    import contextlib
    return contextlib.nullcontext()


if __name__ == "__main__":
    sys.exit(main())
