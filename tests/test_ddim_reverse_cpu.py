"""CPU: ddim_reverse_sample's host surface (gaussian_diffusion.py:636-668 of the reference) and its fixture,
tests/golden/ddim_reverse_tiny.npz (tools/golden/loops_nll.py: ddim_reverse).  No GPU compute call is made here."""
import inspect
import json

import numpy as np
import pytest

from ddim_reverse_restated import rounding_bound, sample_fp64, tables
from helpers import load_npz
from video_diffusion_amd import _lib
from video_diffusion_amd.gaussian_diffusion import GaussianDiffusion
from video_diffusion_amd.respace import SpacedDiffusion
from video_diffusion_amd.script_util import create_gaussian_diffusion


def _diffusion(cfg):
    return create_gaussian_diffusion(steps=cfg["diffusion_steps"], learn_sigma=cfg["learn_sigma"], sigma_small=cfg["sigma_small"],
                                     noise_schedule=cfg["noise_schedule"], use_kl=cfg["use_kl"], predict_xstart=cfg["predict_xstart"],
                                     rescale_timesteps=cfg["rescale_timesteps"], rescale_learned_sigmas=cfg["rescale_learned_sigmas"],
                                     timestep_respacing=cfg["timestep_respacing"])


def test_the_step_and_both_loops_exist_with_their_parameter_names():
    names = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert names(GaussianDiffusion.ddim_reverse_sample) == ["self", "model", "x", "t", "clip_denoised", "denoised_fn", "model_kwargs", "eta"]
    loop = ["self", "model", "x_start", "clip_denoised", "denoised_fn", "model_kwargs", "t_start", "t_end", "progress"]
    assert names(GaussianDiffusion.ddim_reverse_sample_loop) == loop
    assert names(GaussianDiffusion.ddim_reverse_sample_loop_progressive) == loop
    d = inspect.signature(GaussianDiffusion.ddim_reverse_sample).parameters
    assert d["clip_denoised"].default is True and d["eta"].default == 0.0 and d["denoised_fn"].default is None
    d = inspect.signature(GaussianDiffusion.ddim_reverse_sample_loop).parameters
    assert d["t_start"].default == 0 and d["t_end"].default is None and d["progress"].default is False
    assert inspect.isgeneratorfunction(GaussianDiffusion.ddim_reverse_sample_loop_progressive)
    assert SpacedDiffusion.ddim_reverse_sample is GaussianDiffusion.ddim_reverse_sample      # reachable through SpacedDiffusion as the other steps are
    for f in (GaussianDiffusion.ddim_reverse_sample_loop, GaussianDiffusion.ddim_reverse_sample_loop_progressive):
        assert "extension" in f.__doc__
    assert "vd_ddim_reverse_sample" in _lib.SIGNATURES


def test_eta_other_than_zero_raises_the_references_assertion_before_any_library_call(monkeypatch):
    def no_library():
        raise RuntimeError("the library was reached")
    monkeypatch.setattr(_lib, "lib", no_library)
    diff = _diffusion(json.loads(str(load_npz("ddim_reverse_tiny.npz")["cfg_json"])))
    with pytest.raises(AssertionError, match="Reverse ODE only for deterministic path"):
        diff.ddim_reverse_sample(None, None, None, eta=0.5)


def test_executor_maps_ddim_reverse_to_its_own_sampler_and_nothing_else():
    from video_diffusion_amd.executor import _sampler_id
    assert _sampler_id("ddim_reverse") == 2
    assert [_sampler_id(s) for s in ("p_sample", "ddim", "ddim_sample", "anything")] == [0, 1, 1, 1]


def test_fixture_loads_and_its_chains_are_consistent():
    """Step k + 1 of the 'x_0' chain was produced from step k: from step k's 'sample' and step k + 1's 'pred_xstart' the
    three lines behind pred_xstart give step k + 1's 'sample', inside the float32 rounding bound -- which the reference's own
    arithmetic (every operation rounded once) must respect as well.  Same for the last step of the clip_denoised=False chain."""
    rec = load_npz("ddim_reverse_tiny.npz")
    cfg = json.loads(str(rec["cfg_json"]))
    assert cfg["timestep_respacing"] == "ddim5" and json.loads(str(rec["xstart_cfg_json"]))["predict_xstart"] is True
    diff = _diffusion(cfg)
    assert diff.num_timesteps == 5 and diff.alphas_cumprod_next[-1] == 0.0
    assert np.array_equal(diff.alphas_cumprod_next[:-1], diff.alphas_cumprod[1:])     # the shifted row: why the engine needs no table of its own
    n = int(rec["thin"])
    thin = lambda v: v[..., ::n, ::n]  # noqa: E731
    assert rec["x0"].shape == (2, 4, 3, 32, 32) and rec["frame_indices"].tolist() == [[0, 1, 2, 3], [4, 5, 8, 11]]
    x = rec["x0"]
    for k in range(5):
        sample, x0p = rec[f"x_0_t{k}_sample"], rec[f"x_0_t{k}_pred_xstart_thin"]
        assert sample.shape == x.shape and sample.dtype == np.float32 and np.isfinite(sample).all()
        assert x0p.shape == thin(x).shape and np.abs(x0p).max() <= 1.0
        a, b, abn = tables(diff, k)
        want, _ = sample_fp64(thin(x), x0p, a, b, abn)
        assert (np.abs(thin(sample) - want) <= rounding_bound(thin(x), x0p, a, b, abn)).all(), k
        x = sample
    assert tables(diff, 4)[2] == 0.0
    a, b, abn = tables(diff, 4)
    want, _ = sample_fp64(thin(rec["noclip_t3_sample"]), rec["noclip_t4_pred_xstart_thin"], a, b, abn)
    assert (np.abs(rec["noclip_t4_sample_thin"] - want)
            <= rounding_bound(thin(rec["noclip_t3_sample"]), rec["noclip_t4_pred_xstart_thin"], a, b, abn)).all()
    assert np.array_equal(thin(rec["noclip_t3_sample"]), rec["noclip_t3_sample_thin"])
    assert np.abs(rec["noclip_t4_pred_xstart_thin"]).max() > 1.0                      # the clamp was really off
    for obsf in ("x_t", "x_t_minus_1"):
        assert not np.array_equal(rec[f"{obsf}_final_thin"], thin(rec["x_0_t4_sample"]))
