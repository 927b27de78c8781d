"""CPU: the oracle (oracle/unet_ref.py) against the long-window golden vectors (tools/golden/long_window.py: unet_tiny_long; the imported
reference at T = 48, B = 2, with padding frames, both padding rules and the bucket tables).  The GPU tests of windows above
32 frames (tests/test_gpu_long_window.py) use this oracle as their checker."""
import json

import pytest
import torch

import video_diffusion_amd as vda
from helpers import close, load_npz, synth_sd
from oracle.sampler_ref import SamplerRef
from oracle.schedule_ref import ScheduleRef
from oracle.unet_ref import UNetRef


def long_window_inputs(rec):
    """x, model kwargs and t of the fixture's shared window (inputs stored as exact int8 codes)."""
    x = torch.from_numpy(rec["x_q"]).float() / 32
    x0 = torch.from_numpy(rec["x0_q"]).float() / 127
    kw = dict(x0=x0, obs_mask=torch.from_numpy(rec["obs_mask"]), latent_mask=torch.from_numpy(rec["latent_mask"]),
              kinda_marg_mask=torch.from_numpy(rec["kinda_marg_mask"]), frame_indices=torch.from_numpy(rec["frame_indices"]))
    return x, kw, torch.from_numpy(rec["t"])


def test_fixture_window_has_padding_frames_in_no_mask():
    rec = load_npz("unet_tiny_long.npz")
    x, kw, _ = long_window_inputs(rec)
    assert tuple(x.shape) == (2, 48, 3, 32, 32)
    anything = (kw["obs_mask"] + kw["latent_mask"] + kw["kinda_marg_mask"]).reshape(2, 48)
    assert int((anything == 0).sum(1)[0]) == 8 and int(kw["obs_mask"].sum()) == 2 * 16


@pytest.mark.parametrize("case", ["rpe", "nopad", "table"])
def test_oracle_eps_matches_long_window_golden(case):
    rec = load_npz("unet_tiny_long.npz")
    cfg = json.loads(str(rec[f"{case}_cfg_json"]))
    x, kw, t = long_window_inputs(rec)
    sched = ScheduleRef(cfg["diffusion_steps"], cfg["noise_schedule"], cfg["timestep_respacing"], cfg["sigma_small"],
                        cfg["rescale_timesteps"])
    ora = SamplerRef(sched, UNetRef(cfg, synth_sd(vda.param_specs(cfg))))
    eps = ora.eps(x, t, kw)
    close(eps[..., ::4, ::4], rec[f"{case}_eps"], atol=1e-4, rtol=1e-4)
