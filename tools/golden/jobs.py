"""The reference's job scripts: the vertical + horizontal sampler, the result-path naming rules, the names the scripts use."""
import json
import logging
import os
import re
from argparse import Namespace

import numpy as np
import torch

from . import _reference
from ._common import build, save_json, save_npz, tiny_cfg


def full_sampler(out):
    """scripts/video_sample_full.py infer_video (:50-323) on the tiny model, CPU, noise from the seeded global generator."""
    vsf = _reference.video_sample_full()
    cfg = tiny_cfg("ddim5")
    model, diff = build(cfg)
    B, T, obs_len, max_frames, step = 2, 6, 2, 4, 1
    g = torch.Generator().manual_seed(21)
    batch = torch.rand(B, T, 3, 32, 32, generator=g) * 2 - 1
    rec = {}
    for tag, vertical, obs_frames in (("v2_xtm1", 2, "x_t_minus_1"), ("v0_x0", 0, "x_0"), ("v5_x0", 5, "x_0")):
        vsf.args = Namespace(vertical_steps=vertical, observed_frames=obs_frames, save_all_timesteps=False)
        vsf.logger = logging.getLogger("ref_full")
        torch.manual_seed(1234)                        # p_sample draws th.randn_like from the global CPU generator
        samples, _ = vsf.infer_video("autoreg", model, diff, batch, max_frames, obs_len, step, None, use_gradient_method=False)
        rec[f"samples_{tag}"] = samples.astype(np.float32)
    return [save_npz(out, "full_sampler_tiny.npz", batch=batch.numpy(), noise_seed=np.array(1234),
                     cfg_json=np.array(json.dumps(cfg)), B=B, T=T, obs_length=obs_len, max_frames=max_frames, step_size=step,
                     **rec)]


def eval_paths(out):
    """improved_diffusion/test_util.py get_model_results_path / get_eval_run_identifier (:65-132) naming rules."""
    tu = _reference.load().tu
    cases = []
    base = dict(use_ddim=False, timestep_respacing="", eval_dir=None, checkpoint_path="/scratch/vd/saeids-checkpoints/abcdefg/ema_0.9999_550000.pt")
    for over in (dict(), dict(use_ddim=True), dict(timestep_respacing="ddim250"), dict(use_ddim=True, timestep_respacing="250"),
                 dict(checkpoint_path="/data/checkpoints/run7/sub/model_100.pt", timestep_respacing="ddim50"),
                 dict(eval_dir="/tmp/my_eval")):
        a = Namespace(**{**base, **over})
        for postfix in ("", "_x"):
            cases.append(dict(kind="model_results_path", args=vars(a), postfix=postfix,
                              expect=str(tu.get_model_results_path(a, postfix=postfix))))
    ident = dict(inference_mode="autoreg", max_frames=20, step_size=7, T=300, obs_length=36)
    for over in (dict(), dict(optimality="linspace-t"), dict(optimality=None), dict(dataset_partition="train"),
                 dict(dataset_partition="test"), dict(use_gradient_method=True), dict(use_gradient_method=False),
                 dict(override_dataset="carla"), dict(optimality="x", dataset_partition="train", use_gradient_method=True,
                                                       override_dataset="mazes"),
                 dict(inference_mode="hierarchy-2", max_frames=16, step_size=4, T=16, obs_length=4)):
        a = Namespace(**{**ident, **over})
        for postfix in ("", "_p"):
            cases.append(dict(kind="eval_run_identifier", args=vars(a), postfix=postfix,
                              expect=tu.get_eval_run_identifier(a, postfix=postfix)))
    return [save_json(out, "eval_paths.json", cases, indent=1)]


def script_imports(out):
    """Which attributes the reference's sampling scripts take from the modules INTEGRATION.md A swaps (read from the
    scripts' text; the fixture is the list of names, not the scripts)."""
    modules = ["dist_util", "inference_util", "test_util"]
    rec = {}
    for script in ["video_sample.py", "video_sample_full.py", "video_nll.py"]:
        text = open(os.path.join(_reference.directory(), "scripts", script)).read()
        used = {m: sorted(set(re.findall(rf"\b{m}\.([A-Za-z_][A-Za-z0-9_]*)", text))) for m in modules}
        block = re.search(r"from improved_diffusion\.script_util import \(([^)]*)\)", text)
        used["script_util"] = sorted(n.strip() for n in block.group(1).replace("\n", " ").split(",") if n.strip()) if block else []
        rec[script] = {m: v for m, v in used.items() if v}
    return [save_json(out, "script_imports.json", rec, indent=1, sort_keys=True)]
