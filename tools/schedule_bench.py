#!/usr/bin/env python3
"""One scoring call of the observed-frame search (video_optimal_schedule), three ways, one process, one GPU.

The default 116 M model at 64 x 64; per window shape -- B = 8 x T = 20 with 10 observed frames (the window of BASELINE
configs[2]) and B = 8 x T = 16 with 4 observed -- one timestep per item:

    (a) parent     diffusion.calc_bpd_loop_subsampled(..., t_seq of shape (B, 1)): th.randn_like + q_sample + p_mean_variance +
                   vd_vb_terms (+ _prior_bpd), which is what video_nll.run_bpd_evaluation costs per call
    (b) score      diffusion.score_windows(..., suffix_skip=False)
    (c) score+skip diffusion.score_windows(..., suffix_skip=True)

Device events around each call, the three interleaved round by round, the median of --steps rounds after --warmup.  Per shape
one JSON line with the three times, the ratios b/a, c/b, c/a and the two checks (b <= 1.02 a: the same forward and fewer
passes, 2 % same-process noise; c <= b).  Exit status 1 when a check fails.

    python tools/schedule_bench.py [--steps 10] [--warmup 3] [--out profiles/schedule_bench.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(8, 20, 10), (8, 16, 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--image-size", type=int, default=64)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()

    import numpy as np
    import torch
    import video_diffusion_amd as vda
    dev = torch.device("cuda:0")
    S = args.image_size
    lines, ok = [], True
    for B, T, n_obs in SHAPES:
        cfg = vda.video_model_and_diffusion_defaults()
        cfg.update(T=T, image_size=S, rp_alpha=T, rp_beta=T, rp_gamma=T, timestep_respacing="ddim250")
        model, diff = vda.create_video_model_and_diffusion(**cfg)
        model.load_state_dict({k: torch.from_numpy(vda.weights_init.synth_param(k, s)) for k, s in model.param_specs()})
        model.to(dev).eval()
        g = torch.Generator().manual_seed(1234)
        x0 = (torch.rand(B, T, 3, S, S, generator=g) * 2 - 1).to(dev)
        obs = torch.zeros(B, T, 1, 1, 1, device=dev)
        obs[:, :n_obs] = 1
        lat = 1 - obs
        kw = dict(frame_indices=torch.arange(T, device=dev).view(1, T).repeat(B, 1), x0=x0, obs_mask=obs, latent_mask=lat,
                  kinda_marg_mask=torch.zeros_like(obs), x_t_minus_1=x0, observed_frames="x_0")
        grid = diff.num_timesteps - 1 - np.linspace(0, diff.num_timesteps, B, endpoint=False, dtype=int)
        t_seq = grid.reshape(B, 1)
        t = torch.tensor(grid, device=dev)
        per_blocks = T * 3 * S * S // 4
        offs = [b * per_blocks for b in range(B)]
        last = {}

        def parent():
            last["a"] = diff.calc_bpd_loop_subsampled(model, x0, clip_denoised=True, model_kwargs=kw, latent_mask=lat, t_seq=t_seq)["mse"]

        def score():
            last["b"] = diff.score_windows(model, x0, t, kw, lat, 0, offs, suffix_skip=False)

        def score_skip():
            last["c"] = diff.score_windows(model, x0, t, kw, lat, 0, offs, suffix_skip=True)

        paths = [("a", parent), ("b", score), ("c", score_skip)]
        times = {k: [] for k, _ in paths}
        for i in range(args.warmup + args.steps):
            for k, fn in paths:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if i >= args.warmup:
                    times[k].append(e0.elapsed_time(e1))
        model.check_device_errors()
        assert torch.isfinite(last["a"]).all() and torch.isfinite(last["b"]).all()
        assert torch.equal(last["b"], last["c"]), "suffix skip changed the scores"
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        checks = dict(b_le_a=med["b"] <= 1.02 * med["a"], c_le_b=med["c"] <= med["b"])
        ok = ok and all(checks.values())
        line = dict(shape=f"B{B}xT{T}", B=B, T=T, observed=n_obs, image_size=S, steps=args.steps, warmup=args.warmup,
                    parent_ms=round(med["a"], 3), score_ms=round(med["b"], 3), score_suffix_skip_ms=round(med["c"], 3),
                    b_over_a=round(med["b"] / med["a"], 4), c_over_b=round(med["c"] / med["b"], 4), c_over_a=round(med["c"] / med["a"], 4),
                    min_ms={k: round(min(v), 3) for k, v in times.items()}, **checks)
        print(json.dumps(line), flush=True)
        lines.append(line)
        del model, diff, kw, x0
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
