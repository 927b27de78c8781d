#!/usr/bin/env python3
"""Mint the long-window golden vectors (windows of more than 32 frames) from the IMPORTED reference, on CPU/fp32, with the
closed-form weights of `video-diffusion_amd/weights_init.py`.  Only the data written to tests/golden/ is committed.

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> \
        python3 <repo>/tools/gen_golden_long_window.py

Output: tests/golden/unet_tiny_long.npz -- the tiny config of unet_tiny.npz at T = 48, B = 2.  One window shared by every
case: 16 observed frames, 24 latent frames and 8 padding frames that are in none of the three masks (attn_mask =
anything_mask, unet.py:953,1024).  Inputs are stored as int8 codes (x = x_q / 32, x0 = x0_q / 127, exact in fp32) and eps
every 4th row and column, to keep the fixture small.  Cases:
  rpe        RPE nets, allow_interactions_between_padding=True (the default)
  nopad      RPE nets, allow_interactions_between_padding=False
  table      use_rpe_net=False: the bucket tables (as unet_tiny_table.npz)
  attn       the rpe case with return_attn_weights=True: the temporal maps (B*HW, T, T), every STRIDE-th map
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")

spec = importlib.util.spec_from_file_location("weights_init", os.path.join(REPO, "video-diffusion_amd", "weights_init.py"))
weights_init = importlib.util.module_from_spec(spec)
spec.loader.exec_module(weights_init)

lp = types.ModuleType("lpips")
lp.LPIPS = type("LPIPS", (torch.nn.Module,), {})
lp.normalize_tensor = lambda x: x
sys.modules["lpips"] = lp

from improved_diffusion import script_util as su  # noqa: E402

torch.set_num_threads(8)
B, T, S, N_OBS, N_PAD, T_VAL, STRIDE = 2, 48, 32, 16, 8, 120, 37


def tiny_cfg(**over):
    d = su.video_model_and_diffusion_defaults()
    d.update(T=T, image_size=S, num_channels=32, num_res_blocks=1, rp_alpha=T, rp_beta=T, rp_gamma=T,
             timestep_respacing="ddim250")
    d.update(over)
    return d


def build(cfg):
    model, diff = su.create_video_model_and_diffusion(**cfg)
    sd = model.state_dict()
    model.load_state_dict({k: torch.from_numpy(weights_init.synth_param(k, tuple(v.shape))) for k, v in sd.items()})
    model.eval()
    return model, diff


def window():
    g = torch.Generator().manual_seed(48)
    x_q = torch.clamp(torch.round(torch.randn(B, T, 3, S, S, generator=g) * 32), -127, 127).to(torch.int8)
    x0_q = torch.round((torch.rand(B, T, 3, S, S, generator=g) * 2 - 1) * 127).to(torch.int8)
    x0_q[:, N_OBS:] = 0
    obs = torch.zeros(B, T, 1, 1, 1)
    obs[:, :N_OBS] = 1
    lat = torch.zeros(B, T, 1, 1, 1)
    lat[:, N_OBS:T - N_PAD] = 1
    fidx = torch.stack([torch.arange(T), torch.arange(T) + 5])
    return dict(x_q=x_q, x0_q=x0_q, obs_mask=obs, latent_mask=lat, kinda_marg_mask=torch.zeros(B, T, 1, 1, 1),
                frame_indices=fidx)


def main():
    w = window()
    x = w["x_q"].float() / 32
    kw = dict(x0=w["x0_q"].float() / 127, obs_mask=w["obs_mask"], latent_mask=w["latent_mask"],
              kinda_marg_mask=w["kinda_marg_mask"], frame_indices=w["frame_indices"], x_t_minus_1=w["x0_q"].float() / 127,
              observed_frames="x_0")
    t = torch.tensor([T_VAL] * B)
    rec = {k: v.numpy() for k, v in w.items()}
    rec.update(t=t.numpy(), stride=np.array(STRIDE))
    for case, over in [("rpe", {}), ("nopad", dict(allow_interactions_between_padding=False)),
                       ("table", dict(use_rpe_net=False))]:
        cfg = tiny_cfg(**over)
        model, diff = build(cfg)
        with torch.no_grad():
            eps, attn = diff._wrap_model(model)(x, t, return_attn_weights=(case == "rpe"), **kw)
        rec[f"{case}_cfg_json"] = np.array(json.dumps(cfg))
        rec[f"{case}_eps"] = eps[..., ::4, ::4].numpy()
        if case == "rpe":
            maps = attn["temporal"]
            rec["attn_n_temporal"] = np.array(len(maps))
            for i, a in enumerate(maps):
                rec[f"attn_temporal_{i}_shape"] = np.array(a.shape)
                rec[f"attn_temporal_{i}"] = a[::STRIDE].numpy()
                print("temporal map", i, tuple(a.shape))
        print(case, "eps", tuple(eps.shape), float(eps.abs().max()))
    path = os.path.join(OUT, "unet_tiny_long.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
