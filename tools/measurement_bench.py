#!/usr/bin/env python3
"""What a measurement (zero-shot restoration, DDNM) adds to a step.  One process, one GPU, the window executor (one captured graph per
configuration).

The default 116 M model at 64 x 64, the headline window B = 8 x T = 16 with 4 observed frames ('x_0'), schedule ddim250, sampler
'ddim' (eta = 0): per round each window is armed at the last index and --steps-per-round steps are replayed between two device
events; the plain step, the step under a x4 super-resolution measurement (sr4) and the step under a greyscale one (gray) alternate
round by round in the one process; the median of --rounds rounds after --warmup, in ms per step, and each one's cost over the plain
step.

The projection is one more launch in front of the sampler pass: it reads x_t and the network output, writes the projected x_0 (12 bytes
per element of the 6.3 MB window, plus y), and the sampler pass then reads that x_0 instead of the network output.  The pass alone
(vd_measurement_project: in place on an x_0, 8 bytes per element plus y) is timed as --pass-launches back-to-back launches between two
device events, beside a device-to-device copy of the same tensor timed the same way -- the copy roof AT THIS SIZE: a 6.3 MB tensor
lives in the caches, so neither figure is an HBM rate.  No bar is set: what is measured is recorded next to the plain step of the same
process.  One JSON line, to stdout and to --out.

    python tools/measurement_bench.py [--rounds 10] [--warmup 3] [--steps-per-round 10] [--out profiles/measurement_bench.jsonl]
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
    ap.add_argument("--pass-launches", type=int, default=200)
    ap.add_argument("--image-size", type=int, default=64)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    import video_diffusion_amd as vda
    from video_diffusion_amd import _lib
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
    operators = dict(sr4=(4, False), gray=(1, True))
    ys = {name: diff.measure(truth, s, gr).to(dev) for name, (s, gr) in operators.items()}

    ex = WindowExecutor(model, diff)
    k = args.steps_per_round
    configs = dict(plain={}, **{name: dict(measurement=ys[name], sr_scale=s, gray=gr) for name, (s, gr) in operators.items()})
    times = {name: [] for name in configs}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()                                                # (run makes the current stream wait for the executor's)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for i in range(args.warmup + args.rounds):
        for name, opt in configs.items():
            ex.begin(x_T, kw, sampler="ddim", eta=0.0, seed=0, **opt)
            ex.run(1)
            ms = timed(lambda: ex.run(k)) / k
            if i >= args.warmup:
                times[name].append(ms)
    model.check_device_errors()

    # the pass alone, and a copy of the same tensor, as back-to-back launches
    L, n = _lib.lib(), args.pass_launches
    buf, dst = x_T.clone(), torch.empty_like(x_T)
    lat = (1 - obs).reshape(-1).contiguous()
    elems = buf.numel()
    alone = {}

    def launches(fn):
        for _ in range(n):
            fn()

    for name, (s, gr) in operators.items():
        fn = lambda: _lib.check(L.vd_measurement_project(model._handle, B, T, S, S, _lib.ptr(buf), _lib.ptr(ys[name]), _lib.ptr(lat), s,  # noqa: E731
                                                         1 if gr else 0, _lib.current_stream()))
        launches(fn)
        us = sorted(timed(lambda: launches(fn)) / n * 1e3 for _ in range(5))[2]
        # latent frames are read and written, the others read only; y is read once
        nbytes = 4 * (elems + elems * (T - N_OBS) // T + ys[name].numel() * (T - N_OBS) // T)
        alone[name] = dict(us=round(us, 3), bytes=nbytes, gb_per_s=round(nbytes / us * 1e-3, 1))
    launches(lambda: dst.copy_(buf))
    us = sorted(timed(lambda: launches(lambda: dst.copy_(buf))) / n * 1e3 for _ in range(5))[2]
    copy = dict(us=round(us, 3), bytes=8 * elems, gb_per_s=round(8 * elems / us * 1e-3, 1))

    med = {name: sorted(v)[len(v) // 2] for name, v in times.items()}
    line = dict(case="step", shape=f"B{B}xT{T}", B=B, T=T, observed=N_OBS, image_size=S, schedule="ddim250", sampler="ddim",
                rounds=args.rounds, warmup=args.warmup, steps_per_round=k, ms={name: round(m, 4) for name, m in med.items()},
                added_ms={name: round(med[name] - med["plain"], 4) for name in operators},
                added_fraction={name: round(med[name] / med["plain"] - 1.0, 5) for name in operators},
                spread={name: round((max(v) - min(v)) / med[name], 4) for name, v in times.items()},
                pass_alone=alone, copy_same_tensor=copy, pass_launches=n)
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
