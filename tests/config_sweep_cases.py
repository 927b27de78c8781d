"""The configuration sweep's shared cases: tests/golden/unet_configs.npz (tools/golden/configs.py) read once, and the CPU
oracle's eps per configuration computed once.  Nothing returned here may be written to."""
import functools
import json

import torch

from helpers import load_npz, synth_sd
from oracle.sampler_ref import SamplerRef
from oracle.schedule_ref import ScheduleRef
from oracle.unet_ref import UNetRef

TAGS = ["w96_s64", "w96_h2_rb2_s32", "w160_s32", "w256_h8_s32", "w64_h1_s64", "w64_att32_s64", "w32_att8_rb3_s32", "w32_s128",
        "w96_noss_table_s64", "w64_h8_s64", "w96_dup_s32"]
# The spatial attention serves head dims up to 128: these two are pinned on the oracle and refused by the engine at creation, by name
REFUSED = {"w64_h1_s64": ["num_heads=1", "input_blocks.5.1", "head dim 192", "128"],
           "w96_noss_table_s64": ["num_heads=2", "input_blocks.5.1", "head dim 144", "128"]}
SERVED = [t for t in TAGS if t not in REFUSED]
BACKWARD_TAGS = ["w96_s64", "w96_h2_rb2_s32", "w64_att32_s64", "w160_s32"]
EXECUTOR_TAGS = ["w96_s64", "w64_att32_s64", "w32_att8_rb3_s32"]
MODE_TAGS = ["w96_s64", "w160_s32"]


@functools.lru_cache(maxsize=None)
def fixture():
    rec = load_npz("unet_configs.npz")
    assert json.loads(str(rec["tags"])) == TAGS
    return rec


@functools.lru_cache(maxsize=None)
def case(tag):
    """cfg, the window (CPU tensors), t, the reference's strided eps, its stride, the reference's [(name, shape)]."""
    rec = fixture()
    cfg = json.loads(str(rec[f"{tag}_cfg_json"]))
    s = f"s{cfg['image_size']}_"
    c = {k: torch.from_numpy(rec[s + k]) for k in ("obs_mask", "latent_mask", "kinda_marg_mask", "frame_indices")}
    c["x"] = torch.from_numpy(rec[s + "x_q"]).float() / float(rec[s + "x_div"])
    c["x0"] = torch.from_numpy(rec[s + "x0_q"]).float() / float(rec[s + "x0_div"])
    specs = [(n, tuple(shape)) for n, shape in json.loads(str(rec["specs_json"]))[tag]]
    return dict(cfg=cfg, c=c, t=torch.from_numpy(rec["t"]), eps=torch.from_numpy(rec[f"{tag}_eps"]),
                stride=8 if cfg["image_size"] == 128 else 4, specs=specs)


def oracle_kw(c):
    return dict(x0=c["x0"], obs_mask=c["obs_mask"], latent_mask=c["latent_mask"], kinda_marg_mask=c["kinda_marg_mask"],
                frame_indices=c["frame_indices"], observed_frames="x_0", x_t_minus_1=c["x0"])


def sampler(cfg, net):
    return SamplerRef(ScheduleRef(cfg["diffusion_steps"], cfg["noise_schedule"], cfg["timestep_respacing"], cfg["sigma_small"],
                                  cfg["rescale_timesteps"]), net)


@functools.lru_cache(maxsize=None)
def oracle(tag):
    """The CPU oracle of a configuration on the closed-form weights, whose names and shapes come from the FIXTURE (the
    reference's state_dict), not from the engine under test."""
    k = case(tag)
    return sampler(k["cfg"], UNetRef(k["cfg"], synth_sd(k["specs"])))


@functools.lru_cache(maxsize=None)
def oracle_eps(tag):
    k = case(tag)
    return oracle(tag).eps(k["c"]["x"], k["t"], oracle_kw(k["c"]))


def outside(got, ref, atol=1e-4, rtol=1e-4):
    """(elements outside atol + rtol |ref|, max |d|, max of |d| / bound)."""
    err = (got - ref).abs()
    lim = atol + rtol * ref.abs()
    return int((err > lim).sum()), float(err.max()), float((err / lim).max())
