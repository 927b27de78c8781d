"""The DEFAULT full-size models (116 M at 64x64, 119 M at 128x128): eps of the reference for seeded windows."""
import json
import time

import numpy as np
import torch

from . import _reference
from ._common import build, save_json, save_npz

TIMING_KEYS = ("reference_s_per_step", "oracle_s_per_step")     # wall-clock seconds: `check` skips them, `write` keeps old ones


def _default_cfg(size):
    cfg = _reference.load().su.video_model_and_diffusion_defaults()
    cfg.update(T=16, image_size=size, rp_alpha=16, rp_beta=16, rp_gamma=16, timestep_respacing="ddim250")
    return cfg


def full(out):
    """eps of the 64x64 (T = 16) and 128x128 (T = 8 frames through the T = 16 model) models for one clip, plus
    reference-vs-oracle seconds per step and their max |eps| difference (the `cpu_baseline.kind: "port"` equivalence)."""
    from oracle.unet_ref import UNetRef
    timing, paths = {}, []
    for name, size, T, n_obs, seed in [("unet_full64.npz", 64, 16, 4, 9), ("unet_full128.npz", 128, 8, 4, 19)]:
        cfg = _default_cfg(size)
        model, diff = build(cfg)
        n_par = sum(p.numel() for p in model.parameters())
        # the same seeded window the GPU tests build (tests/test_gpu_engine.py::_rand_window)
        g = torch.Generator().manual_seed(seed)
        x0 = torch.rand(1, T, 3, size, size, generator=g) * 2 - 1
        x0[:, n_obs:] = 0
        x = torch.randn(1, T, 3, size, size, generator=g)
        obs = torch.zeros(1, T, 1, 1, 1)
        obs[:, :n_obs] = 1
        fidx = torch.arange(T, dtype=torch.int64).view(1, T)
        kw = dict(frame_indices=fidx, x0=x0, obs_mask=obs, latent_mask=1 - obs, kinda_marg_mask=torch.zeros(1, T, 1, 1, 1),
                  x_t_minus_1=x0, observed_frames="x_0")
        t = torch.tensor([200])
        wrapped = diff._wrap_model(model)
        with torch.no_grad():
            wrapped(x, t, **kw)                                              # warm-up
            t0 = time.time()
            eps, _ = wrapped(x, t, **kw)
            t_ref = time.time() - t0
            sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
            ora = UNetRef(cfg, sd)
            tm = torch.tensor([float(diff.timestep_map[200]) * (1000.0 / diff.original_num_steps)]) if diff.rescale_timesteps \
                else torch.tensor([float(diff.timestep_map[200])])
            ora(x, tm, **kw)
            t0 = time.time()
            eps_o = ora(x, tm, **kw)
            t_ora = time.time() - t0
        d = float((eps - eps_o).abs().max())
        timing[name] = dict(params=n_par, reference_s_per_step=t_ref, oracle_s_per_step=t_ora, max_abs_eps_diff=d, threads=8,
                            shape=[1, T, 3, size, size])
        print(name, timing[name])
        paths.append(save_npz(out, name, eps=eps.numpy(), t=np.array([200]), seed=np.array([seed]), n_obs=np.array([n_obs]),
                              T=np.array([T]), x_checksum=np.array([float(x.double().sum()), float(x0.double().sum())]),
                              cfg_json=json.dumps(cfg), n_params=np.array([n_par])))
    return paths + [save_json(out, "full_size_reference_vs_oracle.json", timing, indent=1)]


def b8(out):
    """The HEADLINE window itself: 116 M model, B = 8 x T = 16 x 64 x 64, 4 observed frames (bench.py's make_window, seed
    1234), eps of the reference at t = 200 for a seeded x_t: every 4th pixel of every frame + per-frame fp64 sums / sums of
    squares of the FULL eps (gaussian_diffusion.py:229-372 -> respace.py:111-119 -> unet.py:949-1026)."""
    cfg = _default_cfg(64)
    model, diff = build(cfg)
    B, T, S, n_obs, seed, t_val = 8, 16, 64, 4, 1234, 200
    g = torch.Generator().manual_seed(seed)                     # bench.py: make_window
    video = torch.rand(B, T, 3, S, S, generator=g) * 2 - 1
    x0 = video.clone()
    x0[:, n_obs:] = 0
    obs = torch.zeros(B, T, 1, 1, 1)
    obs[:, :n_obs] = 1
    x = torch.randn(B, T, 3, S, S, generator=torch.Generator().manual_seed(seed + 1))
    kw = dict(frame_indices=torch.arange(T).view(1, T).repeat(B, 1), x0=x0, obs_mask=obs, latent_mask=1 - obs,
              kinda_marg_mask=torch.zeros(B, T, 1, 1, 1), x_t_minus_1=x0, observed_frames="x_0")
    t = torch.tensor([t_val] * B)
    t0 = time.time()
    with torch.no_grad():
        eps, _ = diff._wrap_model(model)(x, t, **kw)
    print(f"reference B=8 step: {time.time() - t0:.1f} s")
    e64 = eps.double()
    return [save_npz(out, "unet_full64_b8.npz", cfg_json=json.dumps(cfg), B=[B], T=[T], n_obs=[n_obs], seed=[seed], t=[t_val],
                     eps_sub=eps[:, :, :, ::4, ::4].numpy().copy(), frame_sum=e64.sum((2, 3, 4)).numpy(),
                     frame_sumsq=(e64 * e64).sum((2, 3, 4)).numpy(), eps_absmax=[float(eps.abs().max())])]
