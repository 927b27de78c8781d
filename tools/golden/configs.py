"""Model configurations away from the tiny one: widths, head counts, attention layouts, image sizes.  One step each."""
import json

import numpy as np
import torch

from ._common import build, kwargs_of, make_inputs, save_npz, tiny_cfg

B, T, N_OBS, T_VAL = 2, 3, 1, 120
FIDX = [[0, 1, 2], [9, 4, 6]]

# tag -> overrides of tiny_cfg("ddim250")
CONFIGS = {
    "w96_s64": dict(image_size=64, num_channels=96),
    "w96_h2_rb2_s32": dict(image_size=32, num_channels=96, num_heads=2, num_res_blocks=2),
    "w160_s32": dict(image_size=32, num_channels=160),
    "w256_h8_s32": dict(image_size=32, num_channels=256, num_heads=8),
    "w64_h1_s64": dict(image_size=64, num_channels=64, num_heads=1),
    "w64_att32_s64": dict(image_size=64, num_channels=64, attention_resolutions="32,16,8"),
    "w32_att8_rb3_s32": dict(image_size=32, attention_resolutions="8", num_res_blocks=3),
    "w32_s128": dict(image_size=128, num_channels=32),
    "w96_noss_table_s64": dict(image_size=64, num_channels=96, num_heads=2, use_scale_shift_norm=False, use_rpe_net=False,
                               rp_alpha=2, rp_beta=4, rp_gamma=8),
    "w64_h8_s64": dict(image_size=64, num_channels=64, num_heads=8),
    "w96_dup_s32": dict(image_size=32, num_channels=96, cond_emb_type="duplicate"),
}

# int8 codes per image size: x = x_q / X_DIV, x0 = x0_q / X0_DIV, exact in fp32.  32 x 32 uses the codes of unet_tiny_long.npz;
# a window of 4 and 16 times the pixels takes coarser codes (fewer levels deflate better) to keep the fixture under 400 KB.
CODES = {32: (32, 127), 64: (8, 31), 128: (1, 3)}


def eps_stride(size):
    return 8 if size == 128 else 4


def window(size):
    """The window of one image size, drawn as make_inputs draws it (x0 uniform, then x normal, one generator seeded with the
    size) and rounded to int8 codes.  Every configuration of a size shares it: it is stored once per size."""
    x_div, x0_div = CODES[size]
    inp = make_inputs(B, T, size, N_OBS, seed=size, fidx_rows=FIDX, draw=("x0", "x"))
    x_q = torch.clamp(torch.round(inp["x"] * x_div), -127, 127).to(torch.int8)
    x0_q = torch.round(inp["x0"] * x0_div).to(torch.int8)
    inp.update(x=x_q.float() / x_div, x0=x0_q.float() / x0_div)
    return inp, dict(x_q=x_q, x0_q=x0_q, x_div=np.array(x_div), x0_div=np.array(x0_div))


def unet_configs(out):
    """eps of the reference at t = 120 for every entry of CONFIGS, B = 2, T = 3, one observed frame, every 4th row and column
    (every 8th at 128 x 128), with the names and shapes of the reference's state_dict."""
    rec = dict(tags=np.array(json.dumps(list(CONFIGS))), t=np.array([T_VAL] * B))
    windows, specs = {}, {}
    for tag, over in CONFIGS.items():
        cfg = tiny_cfg("ddim250", **over)
        size = cfg["image_size"]
        if size not in windows:
            windows[size], codes = window(size)
            for k, v in codes.items():
                rec[f"s{size}_{k}"] = v
            for k in ("obs_mask", "latent_mask", "kinda_marg_mask", "frame_indices"):
                rec[f"s{size}_{k}"] = windows[size][k].numpy()
        inp = windows[size]
        model, diff = build(cfg)
        with torch.no_grad():
            eps, _ = diff._wrap_model(model)(inp["x"], torch.tensor([T_VAL] * B), **kwargs_of(inp))
        s = eps_stride(size)
        rec[f"{tag}_cfg_json"] = np.array(json.dumps(cfg))
        rec[f"{tag}_eps"] = eps[..., ::s, ::s].numpy()
        specs[tag] = [[k, list(v.shape)] for k, v in model.state_dict().items()]
        print(tag, "eps", tuple(eps.shape), float(eps.abs().max()))
    rec["specs_json"] = np.array(json.dumps(specs, separators=(",", ":")))      # one string: the names repeat across configurations
    return [save_npz(out, "unet_configs.npz", **rec)]
