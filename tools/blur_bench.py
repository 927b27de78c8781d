#!/usr/bin/env python3
"""What a deblur step (DPS on a convolution measurement) costs beside the DPS step it is modelled on.  One process, one GPU, the eager
executor.

The default 116 M model at 64 x 64, the headline window B = 8 x T = 16 with 4 observed frames ('x_0'), schedule ddim250, t = 125.  Three
steps alternate round by round in the one process, each timed between two device events after --warmup rounds; the median of --rounds
rounds, in ms per step, and the spread (max - min) / median of each:
  plain    the p_sample step (one forward, the sampler pass);
  dps      the dps_scope step under a x4 super-resolution measurement (sr4): taped forward, residual and seed passes, backward-data
           pass, final pass (include/vd_amd.h: vd_dps_step);
  deblur   the deblur_scope step under a k x k Gaussian blur (--blur-size, default 9): the same, with blur.hip's two passes
           (include/vd_amd.h: vd_deblur_step).
`deblur_over_dps` is the ratio the two gradient steps are compared by: they pay the same forward and backward.  The two seed entries
alone (vd_op_dps_seed, vd_op_deblur_seed: two launches each, no network) are timed as --pass-launches back-to-back calls between two device
events; both allocate and free their scratch per call, which is part of the figure.  No bar is set.  One JSON line, to stdout and to --out.

    python tools/blur_bench.py [--rounds 10] [--warmup 3] [--steps-per-round 3] [--blur-size 9] [--out profiles/blur_bench.jsonl]
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
    ap.add_argument("--pass-launches", type=int, default=200)
    ap.add_argument("--image-size", type=int, default=64)
    ap.add_argument("--blur-size", type=int, default=9)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    import video_diffusion_amd as vda
    from video_diffusion_amd import _lib
    dev = torch.device("cuda:0")
    S, K = args.image_size, args.blur_size
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
    w = diff.gaussian_kernel(K, K / 4.0)
    y_sr = (diff.measure(truth, 4, False) + 0.05 * torch.randn(B, T, 3, S // 4, S // 4, generator=g)).to(dev)
    y_blur = (diff.blur(truth, w) + 0.05 * torch.randn(B, T, 3, S, S, generator=g)).to(dev)
    t = torch.tensor([125] * B, device=dev)
    k = args.steps_per_round

    def plain():
        diff._fused_step(0, model, x_t, t, True, kw, noise=noise)

    def moved():                                                # inside dps_scope / deblur_scope: the plain step, then the scope's move
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

    steps = dict(plain=plain, dps=moved, deblur=moved)
    times = {name: [] for name in steps}
    # both scopes stay open; which of the two settings the model carries alternates inside the one loop (what the scopes themselves set)
    with diff.dps_scope(model, y_sr, 4, zeta=0.5), diff.deblur_scope(model, y_blur, w, zeta=0.5):
        held = dict(dps=model._dps, deblur=model._deblur)
        for i in range(args.warmup + args.rounds):
            for name, fn in steps.items():
                model._dps, model._deblur = (held["dps"] if name == "dps" else None), (held["deblur"] if name == "deblur" else None)
                ms = timed(fn, k)
                if i >= args.warmup:
                    times[name].append(ms)
        model._dps, model._deblur = held["dps"], held["deblur"]
    model.check_device_errors()

    # the seed entries alone, as back-to-back calls
    L = _lib.lib()
    n = args.pass_launches
    eps = torch.randn(B, T, 3, S, S, generator=g).to(dev)
    lat = (1 - obs).reshape(-1).contiguous()
    w_d = w.to(dev).contiguous()
    deps, dxd, rho = torch.empty_like(x_t), torch.empty_like(x_t), torch.empty(B, device=dev)
    seeds = dict(
        dps=lambda: _lib.check(L.vd_op_dps_seed(model._handle, B, T, S, S, _lib.ptr(x_t), _lib.ptr(eps), _lib.ptr(t), 1, _lib.ptr(y_sr), _lib.ptr(lat),
                                                4, 0, _lib.ptr(deps), _lib.ptr(dxd), _lib.ptr(rho), None, _lib.current_stream())),
        deblur=lambda: _lib.check(L.vd_op_deblur_seed(model._handle, B, T, S, S, _lib.ptr(x_t), _lib.ptr(eps), _lib.ptr(t), 1, _lib.ptr(y_blur),
                                                      _lib.ptr(lat), _lib.ptr(w_d), K, _lib.ptr(deps), _lib.ptr(dxd), _lib.ptr(rho), None,
                                                      _lib.current_stream())))
    seed_us = {}
    for name, fn in seeds.items():
        timed(fn, n)
        seed_us[name] = round(sorted(timed(fn, n) * 1e3 for _ in range(5))[2], 3)

    med = {name: sorted(v)[len(v) // 2] for name, v in times.items()}
    line = dict(case="deblur_step", shape=f"B{B}xT{T}", B=B, T=T, observed=N_OBS, image_size=S, schedule="ddim250", t=125, sampler="p_sample",
                operators=dict(dps="sr4", deblur=f"gaussian{K}"), rounds=args.rounds, warmup=args.warmup, steps_per_round=k,
                ms={name: round(m, 4) for name, m in med.items()}, deblur_over_dps=round(med["deblur"] / med["dps"], 5),
                deblur_over_plain=round(med["deblur"] / med["plain"], 4),
                spread={name: round((max(v) - min(v)) / med[name], 4) for name, v in times.items()},
                seed_passes_alone_us=seed_us, pass_launches=n)
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
