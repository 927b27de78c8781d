#!/usr/bin/env python3
"""What a loss-guided step (loss_guidance_scope: a caller's torch loss on the x_0 prediction) costs.  One process, one GPU, the eager executor.

The default 116 M model at 64 x 64, the headline window B = 8 x T = 16 with 4 observed frames ('x_0'), schedule ddim250.  Three ways to
take the same guided step -- down the gradient of rho = ||y - A x_0(x_t)||_2 under a x4 super-resolution measurement -- alternate round by
round in the one process, each timed between two device events after --warmup rounds; the median of --rounds rounds, in ms per step:
  dps        dps_scope: rho's cotangent formed by the engine's own kernels (one taped forward, one backward-data pass);
  loss       loss_guidance_scope with rho written in torch (`measure`, a norm) and differentiated by torch.autograd between vd_guide_begin
             and vd_guide_finish: the same taped forward and backward-data pass, the caller's torch code between them;
  composed   the same guidance built from what existed before: the plain p_sample step (one forward), the torch cotangent on its
             pred_xstart, the seed in torch, eps_vjp (a second, taped forward and the backward-data pass), the move in torch.
`callback` is the caller's torch code alone (rho and its autograd gradient on a fixed x_0), `plain` the p_sample step.  The expectation
to record against: loss ~ dps + callback, and loss below composed by about one forward (plain).  No bar is set; the line says what was
measured.  One JSON line, to stdout and to --out.

    python tools/loss_guidance_bench.py [--rounds 10] [--warmup 3] [--steps-per-round 3] [--out profiles/loss_guidance_bench.jsonl]
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
    lat = 1 - obs
    kw = dict(frame_indices=torch.arange(T, device=dev).view(1, T).repeat(B, 1), x0=x0, obs_mask=obs, latent_mask=lat,
              kinda_marg_mask=torch.zeros_like(obs), x_t_minus_1=x0, observed_frames="x_0")
    y = (diff.measure(truth, 4, False) + 0.05 * torch.randn(B, T, 3, S // 4, S // 4, generator=g)).to(dev)
    tv = 125
    t = torch.tensor([tv] * B, device=dev)
    a, b = float(diff.sqrt_recip_alphas_cumprod[tv]), float(diff.sqrt_recipm1_alphas_cumprod[tv])
    zeta = 0.5
    k = args.steps_per_round

    def rho(x0_, t_):
        return ((y - diff.measure(x0_, 4, False)) * lat).flatten(1).norm(dim=1)

    def cotangent(x0_):
        with torch.enable_grad():
            leaf = x0_.detach().requires_grad_(True)
            return torch.autograd.grad(rho(leaf, t).sum(), leaf)[0]

    def plain():
        return diff._fused_step(0, model, x_t, t, True, kw, noise=noise)

    def dps():
        diff._step(0, model, x_t, t, True, None, kw, 0.0, noise)

    def loss():
        diff._step(0, model, x_t, t, True, None, kw, 0.0, noise)

    def composed():
        sample, xstart = plain()
        c = cotangent(xstart) * lat * (xstart.abs() < 1)          # through the clamp, read off the clamped prediction
        vjp = diff.eps_vjp(model, x_t, t, -b * c, kw)["vjp"]
        return sample - zeta * lat * (a * c + vjp)

    fixed = torch.rand(B, T, 3, S, S, generator=g).to(dev) * 2 - 1

    def callback():
        cotangent(fixed)

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    with diff.dps_scope(model, y, 4, zeta=zeta):
        dps_scope = model._dps
    with diff.loss_guidance_scope(model, rho, scale=zeta):
        loss_scope = model._loss_guidance
    steps = dict(plain=plain, dps=dps, loss=loss, composed=composed, callback=callback)
    times = {name: [] for name in steps}
    for i in range(args.warmup + args.rounds):
        for name, fn in steps.items():
            model._dps = dps_scope if name == "dps" else None       # (what the scopes set: the steps alternate inside one loop)
            model._loss_guidance = loss_scope if name == "loss" else None
            ms = timed(fn, k)
            if i >= args.warmup:
                times[name].append(ms)
    model._dps = model._loss_guidance = None
    model.check_device_errors()

    med = {name: sorted(v)[len(v) // 2] for name, v in times.items()}
    line = dict(case="loss_guidance_step", shape=f"B{B}xT{T}", B=B, T=T, observed=N_OBS, image_size=S, schedule="ddim250", sampler="p_sample",
                loss="rho of dps_scope (sr4) in torch", rounds=args.rounds, warmup=args.warmup, steps_per_round=k,
                ms={name: round(m, 4) for name, m in med.items()},
                loss_over_dps=round(med["loss"] / med["dps"], 5), loss_minus_dps_ms=round(med["loss"] - med["dps"], 4),
                composed_minus_loss_ms=round(med["composed"] - med["loss"], 4), loss_below_composed=bool(med["loss"] < med["composed"]),
                spread={name: round((max(v) - min(v)) / med[name], 4) for name, v in times.items()})
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
