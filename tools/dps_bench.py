#!/usr/bin/env python3
"""What a DPS step (diffusion posterior sampling for a noisy measurement) costs.  One process, one GPU, the eager executor.

The default 116 M model at 64 x 64, the headline window B = 8 x T = 16 with 4 observed frames ('x_0'), schedule ddim250.  Three steps
alternate round by round in the one process, each timed between two device events after --warmup rounds; the median of --rounds rounds,
in ms per step:
  plain    the p_sample step (one forward, the sampler pass);
  guided   the use_gradient_method step: a taped forward, its loss seed, the backward-data pass, its closing pass;
  dps      the DPS step under a x4 super-resolution measurement (sr4): the same taped forward and backward-data pass, with the sampler
           pass, the residual and seed passes and the final pass around them (include/vd_amd.h: vd_dps_step).
`dps_over_guided` is the ratio the two gradient steps are compared by: they pay the same forward and backward.  The residual and seed
passes alone (vd_op_dps_seed: two launches, no network) are timed as --pass-launches back-to-back calls between two device events; the
entry allocates and frees its scratch per call, which is part of that figure.  `kernel_classes`: the time per kernel class of one profiled
step of each of the two (every launch bracketed by events, so the classes do not add up to the step).  No bar is set.  One JSON line, to
stdout and to --out.

    python tools/dps_bench.py [--rounds 10] [--warmup 3] [--steps-per-round 3] [--out profiles/dps_bench.jsonl]
"""
import argparse
import ctypes
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
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    import video_diffusion_amd as vda
    from video_diffusion_amd import _lib
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
    noise2 = torch.randn(B, T, 3, S, S, generator=g).to(dev)
    obs = torch.zeros(B, T, 1, 1, 1, device=dev)
    obs[:, :N_OBS] = 1
    kw = dict(frame_indices=torch.arange(T, device=dev).view(1, T).repeat(B, 1), x0=x0, obs_mask=obs, latent_mask=1 - obs,
              kinda_marg_mask=torch.zeros_like(obs), x_t_minus_1=x0, observed_frames="x_0")
    y = (diff.measure(truth, 4, False) + 0.05 * torch.randn(B, T, 3, S // 4, S // 4, generator=g)).to(dev)
    t = torch.tensor([125] * B, device=dev)
    k = args.steps_per_round

    def plain():
        diff._fused_step(0, model, x_t, t, True, kw, noise=noise)

    def guided():
        diff._guided(model, x_t, t, True, kw, noise2=noise2, want_sample=True, _noise=noise)

    def dps():
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

    steps = dict(plain=plain, guided=guided, dps=dps)
    times = {name: [] for name in steps}
    with diff.dps_scope(model, y, 4, zeta=0.5):
        scope = model._dps
    for i in range(args.warmup + args.rounds):
        for name, fn in steps.items():
            model._dps = scope if name == "dps" else None       # (what dps_scope sets: the three steps alternate inside one loop)
            ms = timed(fn, k)
            if i >= args.warmup:
                times[name].append(ms)
    model._dps = None
    model.check_device_errors()

    # one profiled step of each gradient step: the time per kernel class (vd_profile_begin / vd_profile_end, as bench.py's kernel_classes)
    L = _lib.lib()
    classes = {}
    for name in ("guided", "dps"):
        nc = L.vd_profile_classes()
        out = (ctypes.c_double * (4 * nc))()
        model._dps = scope if name == "dps" else None
        torch.cuda.synchronize()
        _lib.check(L.vd_profile_begin())
        steps[name]()
        _lib.check(L.vd_profile_end(out, 4 * nc))
        classes[name] = {L.vd_profile_class_name(c).decode(): dict(launches=int(out[4 * c]), ms=round(out[4 * c + 1], 3))
                         for c in range(nc) if out[4 * c]}
    model._dps = None

    # the residual and seed passes alone, as back-to-back calls
    n = args.pass_launches
    eps = torch.randn(B, T, 3, S, S, generator=g).to(dev)
    lat = (1 - obs).reshape(-1).contiguous()
    deps, dxd, rho = torch.empty_like(x_t), torch.empty_like(x_t), torch.empty(B, device=dev)
    seed = lambda: _lib.check(L.vd_op_dps_seed(model._handle, B, T, S, S, _lib.ptr(x_t), _lib.ptr(eps), _lib.ptr(t), 1, _lib.ptr(y), _lib.ptr(lat),  # noqa: E731
                                               4, 0, _lib.ptr(deps), _lib.ptr(dxd), _lib.ptr(rho), None, _lib.current_stream()))
    timed(seed, n)
    seed_us = sorted(timed(seed, n) * 1e3 for _ in range(5))[2]

    med = {name: sorted(v)[len(v) // 2] for name, v in times.items()}
    line = dict(case="dps_step", shape=f"B{B}xT{T}", B=B, T=T, observed=N_OBS, image_size=S, schedule="ddim250", sampler="p_sample",
                operator="sr4", rounds=args.rounds, warmup=args.warmup, steps_per_round=k, ms={name: round(m, 4) for name, m in med.items()},
                dps_over_guided=round(med["dps"] / med["guided"], 5), dps_over_plain=round(med["dps"] / med["plain"], 4),
                spread={name: round((max(v) - min(v)) / med[name], 4) for name, v in times.items()},
                seed_passes_alone_us=round(seed_us, 3), pass_launches=n, kernel_classes=classes)
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
