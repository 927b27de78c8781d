"""use_gradient_method=True: the reference's autograd through its own network."""
import json

import numpy as np
import torch

from ._common import FixedNoise, build, kwargs_of, make_inputs, save_npz, tiny_cfg


def grad(out):
    """The guidance of gaussian_diffusion.py:264-271,350-364: all frames are fed as latent, a sample of x_{t-1} is drawn
    inside p_mean_variance, its squared distance to the observed frames' x_{t-1} is back-propagated to x_t, and the mean
    moves by -10 * alpha_t * grad / 2.  Cases: the tiny config (32 channels: the generic kernels), a 64-channel one (the
    Winograd / split-GEMM kernels take Cout % 64 == 0) and one without scale-shift norm / with the bucket table."""
    rec = {}
    cases = [("c32", tiny_cfg("ddim250"), 2, 4, 2, [[0, 1, 2, 3], [5, 6, 9, 12]]),
             ("c64", tiny_cfg("ddim250", num_channels=64, T=6, rp_alpha=6, rp_beta=6, rp_gamma=6), 1, 6, 3, [[0, 1, 2, 3, 4, 5]]),
             ("c64tab", tiny_cfg("ddim250", num_channels=64, use_rpe_net=False, use_scale_shift_norm=False), 1, 4, 1, [[0, 1, 2, 3]])]
    for name, cfg, B, T, n_obs, fidx in cases:
        model, diff = build(cfg)
        inp = make_inputs(B, T, 32, n_obs, 21 + len(name), fidx, draw=("x0", "x", "noise", "noise2"))
        xtm1 = inp["x0"] + 0.3 * inp["noise2"] * inp["obs_mask"]          # some "x_{t-1} of the observed frames"
        rec[name + "_cfg_json"] = json.dumps(cfg)
        for k, v in inp.items():
            rec[f"{name}_{k}"] = v.numpy()
        rec[name + "_x_t_minus_1"] = xtm1.numpy()
        for t_val in [249, 100, 1, 0]:
            t = torch.tensor([t_val] * B)
            x = inp["x"].clone()
            with FixedNoise(inp["noise"]):
                pm = diff.p_mean_variance(model, x, t, clip_denoised=True, model_kwargs=kwargs_of(inp, xtm1=xtm1),
                                          use_gradient_method=True)
            tag = f"{name}_t{t_val}"
            rec[tag + "_grad"] = x.grad.detach().numpy().copy()
            rec[tag + "_mean"] = pm["mean"].detach().numpy()
            rec[tag + "_pred_xstart"] = pm["pred_xstart"].detach().numpy()
            x = inp["x"].clone()
            with FixedNoise(inp["noise"], inp["noise2"]):                # p_mean_variance draws first, then p_sample
                o = diff.p_sample(model, x, t, clip_denoised=True, model_kwargs=kwargs_of(inp, xtm1=xtm1),
                                  use_gradient_method=True)
            rec[tag + "_psample"] = o["sample"].detach().numpy()
            print(tag, "|grad| max", float(np.abs(rec[tag + "_grad"]).max()), "mean shift max",
                  float((5 * np.abs(rec[tag + "_grad"])).max()))
    return [save_npz(out, "grad_tiny.npz", **rec)]
