"""Windows of more than 32 frames: the tiny config of unet_tiny.npz at T = 48, B = 2."""
import json

import numpy as np
import torch

from ._common import build, save_npz, tiny_cfg

B, T, S, N_OBS, N_PAD, T_VAL, STRIDE = 2, 48, 32, 16, 8, 120, 37


def window():
    """Inputs as int8 codes (x = x_q / 32, x0 = x0_q / 127, exact in fp32), to keep the fixture small."""
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


def unet_tiny_long(out):
    """One window shared by every case: 16 observed frames, 24 latent frames and 8 padding frames that are in none of the
    three masks (attn_mask = anything_mask, unet.py:953,1024); eps every 4th row and column.  Cases:
      rpe        RPE nets, allow_interactions_between_padding=True (the default)
      nopad      RPE nets, allow_interactions_between_padding=False
      table      use_rpe_net=False: the bucket tables (as unet_tiny_table.npz)
      attn       the rpe case with return_attn_weights=True: the temporal maps (B*HW, T, T), every STRIDE-th map"""
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
        cfg = tiny_cfg("ddim250", T=T, image_size=S, rp_alpha=T, rp_beta=T, rp_gamma=T, **over)
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
    return [save_npz(out, "unet_tiny_long.npz", **rec)]
