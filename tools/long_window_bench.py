#!/usr/bin/env python3
"""Step time of long windows against the headline window, one process, one GPU.

The default 116 M model at 64 x 64, eager `diffusion.p_sample(model, x, t, clip_denoised=True, model_kwargs=kw)`, timed with
device events after warm-up, for three shapes of 128 frames per step:

    B = 8 x T = 16   (the headline shape, bench.py)
    B = 2 x T = 64
    B = 1 x T = 128

Convolutions, GEMMs and spatial attention do the same work in all three; temporal attention, temporal GroupNorm and the
relative-position terms grow with T.  Per shape one JSON line: the median step, the ratio to the B = 8 x T = 16 step of the
same run, and the per-class times of one profiled step (vd_profile_begin / vd_profile_end, as bench.py's kernel_classes).

    python tools/long_window_bench.py [--steps 10] [--warmup 3] [--out profiles/long_window_bench.jsonl]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(8, 16), (2, 64), (1, 128)]


def window(torch, B, T, S, n_obs, device):
    g = torch.Generator().manual_seed(1234)
    x0 = torch.rand(B, T, 3, S, S, generator=g) * 2 - 1
    x0[:, n_obs:] = 0
    obs = torch.zeros(B, T, 1, 1, 1)
    obs[:, :n_obs] = 1
    kw = dict(frame_indices=torch.arange(T).view(1, T).repeat(B, 1), x0=x0, obs_mask=obs, latent_mask=1 - obs,
              kinda_marg_mask=torch.zeros(B, T, 1, 1, 1))
    kw = {k: v.to(device) for k, v in kw.items()}
    kw.update(x_t_minus_1=kw["x0"], observed_frames="x_0")
    return kw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--image-size", type=int, default=64)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()

    import torch
    import video_diffusion_amd as vda
    from video_diffusion_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    S = args.image_size
    lines = []
    base = None
    for B, T in SHAPES:
        cfg = vda.video_model_and_diffusion_defaults()
        cfg.update(T=T, image_size=S, rp_alpha=T, rp_beta=T, rp_gamma=T, timestep_respacing="ddim250")
        model, diff = vda.create_video_model_and_diffusion(**cfg)
        model.load_state_dict({k: torch.from_numpy(vda.weights_init.synth_param(k, s)) for k, s in model.param_specs()})
        model.to(dev).eval()
        kw = window(torch, B, T, S, T // 4, dev)
        x = kw["x0"].clone()
        order = list(range(diff.num_timesteps))[::-1]

        def step(i, x):
            t = torch.tensor([order[i % len(order)]] * B, device=dev)
            return diff.p_sample(model, x, t, clip_denoised=True, model_kwargs=kw)["sample"]

        for i in range(args.warmup):
            x = step(i, x)
        torch.cuda.synchronize()
        times = []
        for i in range(args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            x = step(args.warmup + i, x)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        assert torch.isfinite(x).all()
        model.check_device_errors()
        n = L.vd_profile_classes()
        out = (ctypes.c_double * (4 * n))()
        torch.cuda.synchronize()
        _lib.check(L.vd_profile_begin())
        x = step(0, x)
        _lib.check(L.vd_profile_end(out, 4 * n))
        classes = {}
        for c in range(n):
            cnt, ms, fl, by = out[4 * c:4 * c + 4]
            if cnt:
                classes[L.vd_profile_class_name(c).decode()] = dict(launches=int(cnt), ms=round(ms, 3), gflop=round(fl / 1e9, 2))
        med = sorted(times)[len(times) // 2]
        base = med if base is None else base
        line = dict(shape=f"B{B}xT{T}", B=B, T=T, image_size=S, frames_per_step=B * T, sampler="p_sample", executor="eager",
                    steps=args.steps, warmup=args.warmup, step_ms_median=round(med, 3), step_ms_min=round(min(times), 3),
                    ratio_to_B8xT16=round(med / base, 3), kernel_classes=dict(sorted(classes.items(), key=lambda kv: -kv[1]["ms"])))
        print(json.dumps(line), flush=True)
        lines.append(line)
        del model, diff, kw, x
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
