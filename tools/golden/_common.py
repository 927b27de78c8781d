"""What the producers share: the tiny config, the closed-form weights, the seeded inputs, the recorded-noise patch.
The draw ORDER of a seeded generator is part of each fixture, so every difference between fixtures is a named argument."""
import functools
import importlib.util
import json
import os

import numpy as np
import torch

from . import _reference

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


@functools.lru_cache(maxsize=None)
def _weights_init():
    spec = importlib.util.spec_from_file_location("weights_init", os.path.join(REPO, "video-diffusion_amd", "weights_init.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def tiny_cfg(respacing, **over):
    """`respacing` has no default: the 250-step fixtures (unet_tiny*, blocks, psample, denoised_fn, grad, attn*, variants,
    xstart, unet_tiny_long, param_specs) and the 5-step ones (window, loops, nll*, full_sampler) must each say which."""
    d = _reference.load().su.video_model_and_diffusion_defaults()
    d.update(T=4, image_size=32, num_channels=32, num_res_blocks=1, rp_alpha=4, rp_beta=4, rp_gamma=4,
             timestep_respacing=respacing)
    d.update(over)
    return d


def build(cfg):
    """The reference's model and diffusion for `cfg`, with the closed-form weights of weights_init.py, in eval mode."""
    model, diff = _reference.load().su.create_video_model_and_diffusion(**cfg)
    synth = _weights_init().synth_param
    model.load_state_dict({k: torch.from_numpy(synth(k, tuple(v.shape))) for k, v in model.state_dict().items()})
    model.eval()
    return model, diff


def make_inputs(B, T, S, n_obs, seed, fidx_rows, draw=("x0", "x", "noise"), zero_latent_x0=True):
    """One seeded window.
    draw: the tensors taken from the generator, IN THIS ORDER ("x0" uniform in [-1, 1], the others normal).  loops and nll
          draw ("x0",) only; grad, denoised_fn, attn and variants draw a fourth tensor, "noise2".
    zero_latent_x0: latent slots of x0 are zeros (video_sample.py:70-71,119-122).  False for loops, nll, nll_xstart and
          attn_denoised (which zeroes them itself afterwards)."""
    g = torch.Generator().manual_seed(seed)
    drawn = {}
    for name in draw:
        if name == "x0":
            drawn[name] = torch.rand(B, T, 3, S, S, generator=g) * 2 - 1
            if zero_latent_x0:
                drawn[name][:, n_obs:] = 0
        else:
            drawn[name] = torch.randn(B, T, 3, S, S, generator=g)
    obs = torch.zeros(B, T, 1, 1, 1)
    obs[:, :n_obs] = 1
    inp = {k: drawn[k] for k in ("x", "x0", "noise", "noise2") if k in drawn}
    inp.update(obs_mask=obs, latent_mask=1 - obs, kinda_marg_mask=torch.zeros(B, T, 1, 1, 1),
               frame_indices=torch.tensor(fidx_rows, dtype=torch.int64))
    return inp


def kwargs_of(inp, observed_frames="x_0", xtm1=None, with_xtm1=True):
    """model_kwargs of one step.
    xtm1: the observed frames' x_{t-1}; x0 when None (grad passes a noised one).
    with_xtm1: False for loops and nll, whose p_sample_loop fills `x_t_minus_1` in by itself."""
    kw = dict(frame_indices=inp["frame_indices"], x0=inp["x0"], obs_mask=inp["obs_mask"], latent_mask=inp["latent_mask"],
              kinda_marg_mask=inp["kinda_marg_mask"], observed_frames=observed_frames)
    if with_xtm1:
        kw["x_t_minus_1"] = inp["x0"] if xtm1 is None else xtm1
    return kw


def npy(d):
    return {k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in d.items()}


def save_json(out, name, obj, **dump_kw):
    path = os.path.join(out, name)
    with open(path, "w") as f:
        json.dump(obj, f, **dump_kw)
    return path


def save_npz(out, name, **rec):
    path = os.path.join(out, name)
    np.savez_compressed(path, **rec)
    return path


class FixedNoise:
    """`th.randn_like` replaced by a queue of recorded tensors: the draw ORDER is part of the fixture."""

    def __init__(self, *tensors):
        self.q = list(tensors)

    def __enter__(self):
        self.real = torch.randn_like
        torch.randn_like = lambda x, **k: self.q.pop(0).clone()
        return self

    def __exit__(self, *exc):
        torch.randn_like = self.real


def denoised_fn(x):
    """An arbitrary but smooth map that leaves [-1, 1] sometimes, so that the clamp behind it matters."""
    return 1.3 * torch.tanh(1.5 * x) + 0.05
