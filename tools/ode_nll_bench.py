#!/usr/bin/env python3
"""What one point of the probability-flow ODE likelihood costs.  One process, one GPU, the eager executor.

The default 116 M model at 64 x 64, the headline window B = 8 x T = 16 with 4 observed frames ('x_0'), schedule ddim250, index 125.  Four
calls alternate round by round in the one process, each timed between two device events after --warmup rounds; the median of --rounds
rounds, in ms per call:
  plain    the p_sample step (one forward, the sampler pass);
  dps      the DPS step under a x4 super-resolution measurement: a taped forward, the backward-data pass and the passes around them;
  eval_k1  vd_ode_nll_eval with one Rademacher probe and the Euler move: the same taped forward and backward, a probe pass and two small
           launches of the masked dot in place of the sampler, residual and seed passes;
  eval_k4  the same with four probes on the one tape: (eval_k4 - eval_k1) / 3 is what a further probe costs (`per_extra_probe`).
The expectation (no bar is set): eval_k1 costs no more than dps, and a further probe the backward share only.  `loop_ddim100_order2_s`:
the wall time of one order-2 ode_nll_loop on the same window under ddim100 (99 steps: 198 taped forwards and backwards), host wait included.
One JSON line, to stdout and to --out.

    python tools/ode_nll_bench.py [--rounds 10] [--warmup 3] [--steps-per-round 3] [--no-loop] [--out FILE]   (default: profiles/ode_nll_bench.jsonl)
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
    ap.add_argument("--steps-per-round", type=int, default=3)
    ap.add_argument("--image-size", type=int, default=64)
    ap.add_argument("--no-loop", action="store_true", help="skip the ddim100 loop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ode_nll_bench.jsonl"), help="also write the JSON line to this file")
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
    kw = dict(frame_indices=torch.arange(T, device=dev).view(1, T).repeat(B, 1), x0=x0, obs_mask=obs, latent_mask=1 - obs,
              kinda_marg_mask=torch.zeros_like(obs), x_t_minus_1=x0, observed_frames="x_0")
    y = (diff.measure(truth, 4, False) + 0.05 * torch.randn(B, T, 3, S // 4, S // 4, generator=g)).to(dev)
    t = torch.tensor([125] * B, device=dev)
    k = args.steps_per_round
    base, xs, tt, pk = diff._vjp_window(model, x_t, t, kw)
    off = torch.tensor([b << 40 for b in range(B)], dtype=torch.int64, device=dev)

    def plain():
        diff._fused_step(0, model, x_t, t, True, kw, noise=noise)

    def dps():
        diff._step(0, model, x_t, t, True, None, kw, 0.0, noise)

    def eval_k1():
        diff._ode_eval(base, xs, tt, pk, 1, 0, off, 0, None, True)

    def eval_k4():
        diff._ode_eval(base, xs, tt, pk, 4, 0, off, 0, None, True)

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    steps = dict(plain=plain, dps=dps, eval_k1=eval_k1, eval_k4=eval_k4)
    times = {name: [] for name in steps}
    with diff.dps_scope(model, y, 4, zeta=0.5):
        scope = model._dps
    for i in range(args.warmup + args.rounds):
        for name, fn in steps.items():
            model._dps = scope if name == "dps" else None       # (what dps_scope sets: the calls alternate inside one loop)
            ms = timed(fn, k)
            if i >= args.warmup:
                times[name].append(ms)
    model._dps = None
    model.check_device_errors()
    med = {name: sorted(v)[len(v) // 2] for name, v in times.items()}
    line = dict(case="ode_nll_eval", shape=f"B{B}xT{T}", B=B, T=T, observed=N_OBS, image_size=S, schedule="ddim250", t=125, rounds=args.rounds,
                warmup=args.warmup, steps_per_round=k, ms={name: round(m, 4) for name, m in med.items()},
                eval_k1_over_dps=round(med["eval_k1"] / med["dps"], 5), per_extra_probe_ms=round((med["eval_k4"] - med["eval_k1"]) / 3.0, 4),
                spread={name: round((max(v) - min(v)) / med[name], 4) for name, v in times.items()})
    if not args.no_loop:
        from video_diffusion_amd.script_util import create_gaussian_diffusion
        diff100 = create_gaussian_diffusion(steps=cfg["diffusion_steps"], noise_schedule=cfg["noise_schedule"], sigma_small=cfg["sigma_small"],
                                            timestep_respacing="ddim100")
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        out = diff100.ode_nll_loop(model, x_t.clamp(-1, 1), model_kwargs=kw, order=2, n_probes=1)
        torch.cuda.synchronize()
        line.update(loop_ddim100_order2_s=round(time.perf_counter() - w0, 3), loop_bpd=[round(float(v), 4) for v in out["total_bpd"]])
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
