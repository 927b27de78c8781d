#!/usr/bin/env python3
"""What a unipc_sample step costs beside a ddim_sample step and a dpmpp_2m_sample step, and what its pass costs alone.  One process, one
GPU, the window executor (one captured graph per sampler).

The default 116 M model at 64 x 64, the headline window B = 8 x T = 16 with 4 observed frames ('x_0'), schedule logsnr40: per round each
sampler's window is armed at the last index, two steps are replayed outside the timing (so that 'dpmpp_2m' has its history and 'unipc'
runs its order-2 corrector and predictor) and --steps-per-round steps are replayed between two device events; 'ddim' (eta = 0),
'dpmpp_2m' and 'unipc' alternate round by round in the one process; the median of --rounds rounds after --warmup, in ms per step.
The pass alone: vd_unipc_from_xstart on the window's tensors with its state in place (count 2), beside a device-to-device copy of the
window, --pass-reps launches each between two events.  The pass moves 9 window tensors where dpmpp_2m's moves 5: the expectation -- not
a gate -- is a step that differs from dpmpp_2m's by less than the round-to-round spread of a step.

One JSON line, to stdout and to --out.

    python tools/unipc_bench.py [--rounds 10] [--warmup 3] [--steps-per-round 10] [--out profiles/unipc_bench.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, T, N_OBS = 8, 16, 4
SAMPLERS = ("ddim", "dpmpp_2m", "unipc")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps-per-round", type=int, default=10)
    ap.add_argument("--pass-reps", type=int, default=20)
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
    cfg.update(T=T, image_size=S, rp_alpha=T, rp_beta=T, rp_gamma=T, timestep_respacing="logsnr40")
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
    assert 2 + k <= diff.num_timesteps

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    # the pass alone, and a copy of the window beside it
    per = T * 3 * S * S
    d_in = (torch.rand(B, per, generator=g) * 2 - 1).to(dev)
    state = tuple(torch.randn(B, per, generator=g).to(dev) for _ in range(3))
    xw, out, dst = x_T.reshape(B, per).clone(), torch.empty(B, per, device=dev), torch.empty(B, per, device=dev)
    tt = torch.full((B,), diff.num_timesteps - 3, device=dev, dtype=torch.int64)
    L, st = _lib.lib(), _lib.current_stream()

    def the_pass():
        for _ in range(args.pass_reps):
            _lib.check(L.vd_unipc_from_xstart(model._handle, B, per, _lib.ptr(xw), _lib.ptr(d_in), *(_lib.ptr(v) for v in state), 2, _lib.ptr(tt), 1,
                                              _lib.ptr(out), None, *(_lib.ptr(v) for v in state), st))

    def the_copy():
        for _ in range(args.pass_reps):
            dst.copy_(xw)

    times = {s: [] for s in SAMPLERS}
    pass_ms, copy_ms = [], []
    for i in range(args.warmup + args.rounds):
        for sampler in SAMPLERS:
            ex.begin(x_T, kw, sampler=sampler, eta=0.0, seed=0)
            ex.run(2)
            ms = timed(lambda: ex.run(k)) / k
            if i >= args.warmup:
                times[sampler].append(ms)
        p, c = timed(the_pass) / args.pass_reps, timed(the_copy) / args.pass_reps
        if i >= args.warmup:
            pass_ms.append(p)
            copy_ms.append(c)
    model.check_device_errors()
    assert torch.isfinite(ex.x).all()
    mid = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    med = {s: mid(v) for s, v in times.items()}
    line = dict(case="step", shape=f"B{B}xT{T}", B=B, T=T, observed=N_OBS, image_size=S, schedule="logsnr40", rounds=args.rounds,
                warmup=args.warmup, steps_per_round=k, **{f"{s}_ms": round(med[s], 4) for s in SAMPLERS},
                unipc_over_ddim=round(med["unipc"] / med["ddim"], 4), unipc_over_dpmpp_2m=round(med["unipc"] / med["dpmpp_2m"], 4),
                min_ms={s: round(min(v), 4) for s, v in times.items()}, max_ms={s: round(max(v), 4) for s, v in times.items()},
                window_mb=round(4e-6 * B * per, 2), pass_reps=args.pass_reps, pass_ms=round(mid(pass_ms), 5), pass_min_ms=round(min(pass_ms), 5),
                copy_ms=round(mid(copy_ms), 5), copy_min_ms=round(min(copy_ms), 5))
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
