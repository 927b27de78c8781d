"""The reference's observed-frame search (scripts/video_optimal_schedule.py main, :222-354) with a closed-form metric in place of
the network: which frames it picks, in which order it scores the candidates, and which (video, timestep) pairs every
run_bpd_evaluation call sees."""
import importlib.util
import os
import sys
import tempfile
import types
from argparse import Namespace
from pathlib import Path

import numpy as np
import torch

from . import _reference
from ._common import save_json

# (name, inference_mode, optimality); the shapes are shared
CASES = [("autoreg", "autoreg", "linspace-t"),
         ("hierarchy-2_force-nearby", "hierarchy-2", "linspace-t-force-nearby"),
         ("mixed-autoreg-independent", "mixed-autoreg-independent", "linspace-t")]
SHAPE = dict(T=10, obs_length=3, max_frames=4, step_size=2, subset_size=4, num_timesteps=2, batch_size=3)
N_VIDEOS, DIFFUSION_STEPS = 12, 50


def metric(video, obs, latent, t):
    """Closed form, order-invariant in `obs`: what a network's mean_flat mse would be if it depended on how far the latent frames
    are from the nearest observed one, on the video and on the timestep."""
    gap = sum(min(abs(l - o) for o in obs) for l in latent)
    return (1.0 + 0.05 * video + 0.01 * t) * (gap + 0.125 * sum(obs)) / 64.0 + 0.001 * ((7 * video + 3 * sum(obs)) % 5)


def _script():
    """scripts/video_optimal_schedule.py loaded by path.  It imports `video_nll` (a sibling script that needs wandb): an empty module
    of our own stands in, and `run_bpd_evaluation` is set per case."""
    _reference.load()
    sys.modules["video_nll"] = types.ModuleType("video_nll")
    sys.modules["video_nll"].run_bpd_evaluation = None
    spec = importlib.util.spec_from_file_location("ref_video_optimal_schedule",
                                                  os.path.join(_reference.directory(), "scripts", "video_optimal_schedule.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Videos(torch.utils.data.Dataset):
    """Constant videos that encode their dataset index."""

    def __len__(self):
        return N_VIDEOS

    def __getitem__(self, i):
        return torch.full((SHAPE["T"], 1, 1, 1), float(i)), {}


def _run_case(vos, mode, optimality):
    calls, picks = [], []

    def run_bpd_evaluation(model, diffusion, batch, clip_denoised, obs_indices, lat_indices, t_seq=None):
        videos = [int(v) for v in batch[:, 0, 0, 0, 0]]
        ts = [int(t) for t in t_seq[:, 0]]
        assert clip_denoised is True and t_seq.shape == (len(videos), 1)
        n_slots = len(obs_indices[0]) + len(lat_indices[0])
        mse = np.array([metric(v, o, l, t) for v, o, l, t in zip(videos, obs_indices, lat_indices, ts)], dtype=np.float64)
        calls.append(dict(obs=sorted(int(i) for i in obs_indices[0]), latent=[int(i) for i in lat_indices[0]], videos=videos, t=ts,
                          mse=[float(m) for m in mse]))
        return {"mse": mse * n_slots}                                  # run_bpd_evaluation reports sums over the window's frames

    real_metric = vos.get_mse_linspace

    def get_mse_linspace(latent_frame_indices, obs_frame_indices, **kw):
        res = real_metric(latent_frame_indices=latent_frame_indices, obs_frame_indices=obs_frame_indices, **kw)
        cand, before = int(obs_frame_indices[-1]), sorted(int(i) for i in obs_frame_indices[:-1])
        if not picks or picks[-1]["latent"] != list(latent_frame_indices) or picks[-1]["obs"] != before:
            picks.append(dict(latent=[int(i) for i in latent_frame_indices], obs=before, candidates=[], means=[]))
        picks[-1]["candidates"].append(cand)
        picks[-1]["means"].append(float(np.array(list(res.values())).mean()))
        return res

    vos.run_bpd_evaluation, vos.get_mse_linspace = run_bpd_evaluation, get_mse_linspace
    args = Namespace(inference_mode=mode, optimality=optimality, device="cpu", **SHAPE)
    try:
        with tempfile.TemporaryDirectory() as tmp:
            path = Path(tmp) / "optimal_schedule.pt"
            vos.main(args, None, Namespace(num_timesteps=DIFFUSION_STEPS), _Videos(), schedule_path=path, verbose=False)
            schedule = torch.load(path)
    finally:
        vos.get_mse_linspace = real_metric
    return dict(inference_mode=mode, optimality=optimality, schedule={str(k): [int(i) for i in v] for k, v in schedule.items()},
                picks=picks, calls=calls)


def search(out):
    vos = _script()
    os.environ.pop("SLURM_ARRAY_TASK_ID", None)
    rec = dict(shape=SHAPE, n_videos=N_VIDEOS, diffusion_steps=DIFFUSION_STEPS,
               cases={name: _run_case(vos, mode, opt) for name, mode, opt in CASES})
    return [save_json(out, "optimal_schedule_search.json", rec, indent=1)]
