"""Observed-frame search: writes the `optimal_schedule.pt` that `video_sample --optimality ...` and `video_nll --optimality ...`
read (scripts/video_optimal_schedule.py of the reference: the greedy loop :222-354, force_nearby :119-139, the linspace-t
metric :142-206, the schedule files :209-219, the options :357-500).

    python -m video_diffusion_amd.video_optimal_schedule <ckpt> --videos v.npy --inference_mode autoreg --optimality linspace-t

For every inference step of the strategy the reference greedily picks up to `max_frames - len(latent)` observed frames: each pick
scores every finished frame as a candidate on `subset_size` videos, one timestep per video from a grid of `--num_timesteps`
values, and keeps the candidate with the smallest mean of `mse * window length * diffusion.num_timesteps`.

`search` is that loop as a pure function of an injected scorer; `EngineScorer` is the scorer on the HIP engine
(GaussianDiffusion.score_windows: one call per batch of (video, candidate) windows, the latent frames' mse only, the network
suffix of the observed frames skipped).  Declared deviations from the reference's script:
  * when no candidate is left before the budget is filled (e.g. obs_length 1, max_frames 4, step_size 2) the step ends with
    what it has; the reference raises IndexError on `metrics[0]`;
  * `--step` (parsed and never read there), `--task_id` or SLURM_ARRAY_TASK_ID select one inference step;
  * noise: the reference draws fresh th.randn noise in every run_bpd_evaluation call; here a video's noise is a function of
    (--seed, inference step, pick, dataset index) alone (noise_offset), so all candidates of a pick see the same noise on the
    same video (common random numbers; both estimators are unbiased) and a resumed search repeats an uninterrupted one;
  * the run directory is named like video_sample's, from the options as given, so that `video_sample --optimality <same>`
    finds the file; `--submit` / `--slurm_*` (the SLURM launcher) are not offered; `adaptive-*` modes, on which the reference
    crashes (they need the videos), and `random-t*` (NotImplementedError there too) are refused before any network call.
"""
import os
from pathlib import Path

import numpy as np
import torch

from . import inference_util, test_util

RANDOM_T_MESSAGE = "We decided to not use random-t anymore due to its high variance."


def partial_path_of(schedule_path):
    """.optimal_schedule_partial.pt beside optimal_schedule.pt (:236-237)."""
    schedule_path = Path(schedule_path)
    return schedule_path.parent / ("." + schedule_path.stem + "_partial.pt")


def t_grid(num_diffusion_timesteps, num_timesteps):
    """The linspace-t grid, latest timestep first (:172-173)."""
    return num_diffusion_timesteps - 1 - np.linspace(0, num_diffusion_timesteps, num_timesteps, endpoint=False, dtype=int)


def force_nearby(latent_frame_indices, obs_frame_indices, done_frame_indices):
    """:119-139 -- add the nearest finished frame before and the nearest one after the latent span."""
    done = sorted(done_frame_indices)
    lo, hi = min(latent_frame_indices), max(latent_frame_indices)
    idx = None
    for x in done:
        if x < lo and x not in latent_frame_indices:
            idx = x
        else:
            break
    if idx is not None:
        obs_frame_indices.add(idx)
    idx = None
    for x in done[::-1]:
        if x > hi and x not in latent_frame_indices:
            idx = x
        else:
            break
    if idx is not None:
        obs_frame_indices.add(idx)


def load_schedule(path):
    path = Path(path)
    if not path.exists():
        return {}
    with test_util.Protect(path):
        return torch.load(path)


def update_schedule_on_disk(schedule_path, schedule, force=True):
    """:209-219 -- merge `schedule` into the file under its lock; with `force` a step that is already there is refused."""
    schedule_path = Path(schedule_path)
    with test_util.Protect(schedule_path):
        saved = torch.load(schedule_path) if schedule_path.exists() else {}
        for k, v in schedule.items():
            if force and k in saved:
                raise AssertionError(f"Found {k} in the saved schedule! {schedule_path}")
            saved[k] = v
        torch.save(saved, schedule_path)


def check_options(optimality, inference_mode, subset_size, num_timesteps):
    """The refusals, before anything is loaded or scored."""
    if "random-t" in optimality:
        raise NotImplementedError(RANDOM_T_MESSAGE)                       # :289-292
    if "linspace-t" not in optimality:
        raise ValueError(f"Unrecognized optimality {optimality}.")        # :293-294
    if "adaptive" in inference_mode:
        raise NotImplementedError(f"video_optimal_schedule: inference_mode {inference_mode!r} chooses its observed frames from the "
                                  "videos themselves; there is no per-step schedule to optimise (the reference crashes on it)")
    if subset_size % num_timesteps != 0:
        raise ValueError(f"Subset size should ({subset_size}) be divisible by the number of timesteps ({num_timesteps}).")   # :286-288


def _candidate_mean(values, ts):
    """np.array(list({t: [values of the videos dealt t]}.values())).mean() (:200-206,332-334), in the reference's grouping."""
    by_t = {}
    for t, v in zip(ts, values):
        by_t.setdefault(int(t), []).append(v)
    return np.array(list(by_t.values())).mean()


def search(strategy, n_videos, scorer, *, optimality, subset_size, num_timesteps, num_diffusion_timesteps, schedule_path,
           only_step=None, on_pick=None, log=print):
    """The greedy search of scripts/video_optimal_schedule.py:222-354.

    strategy: a fresh, non-adaptive frame scheduler (no optimal schedule loaded).  scorer(cnt, pick, latent, obs, candidates,
    videos, ts) -> array [len(candidates)][len(videos)]: for candidate c the mse (mean over ALL window elements of the latent
    frames' squared eps error) of video videos[i] at timestep ts[i] when observing sorted(obs + [c]) and predicting `latent`;
    `pick` = len(obs) numbers the pick within its step.  Returns {step: sorted observed frames} of the steps finished by this
    call; they are in `schedule_path` as well, and every pick is in the partial file beside it."""
    check_options(optimality, "", subset_size, num_timesteps)
    schedule_path = Path(schedule_path)
    partial_path = partial_path_of(schedule_path)
    saved, partial = load_schedule(schedule_path), load_schedule(partial_path)
    grid = t_grid(num_diffusion_timesteps, num_timesteps)
    finished = {}
    for cnt, (_, latent) in enumerate(strategy):
        if only_step is not None and cnt != only_step:
            continue
        if cnt in saved:
            log(f"Skipping inference step {cnt}; already done.")
            continue
        n_to_condition_on = strategy._max_frames - len(latent)
        obs = set(partial.get(cnt, ()))
        if "force-nearby" in optimality:
            force_nearby(latent, obs, strategy._done_frames)
        while len(obs) < min(len(strategy._done_frames), n_to_condition_on):
            candidates = sorted(c for c in strategy._done_frames if c not in latent and c not in obs)
            if not candidates:
                break                                   # (the reference: IndexError on metrics[0])
            pick = len(obs)
            videos = np.random.RandomState(cnt * 1000 + pick).choice(n_videos, subset_size, replace=False)
            ts = grid.take(range(len(videos)), mode="wrap")               # dealt by position in the subset (:172-181)
            raw = np.asarray(scorer(cnt, pick, list(latent), sorted(obs), candidates, [int(v) for v in videos], [int(t) for t in ts]),
                             dtype=np.float64)
            assert raw.shape == (len(candidates), len(videos)), raw.shape
            n_slots = len(obs) + 1 + len(latent)
            means = [_candidate_mean(row * n_slots * num_diffusion_timesteps, ts) for row in raw]
            best = int(np.argmin(means))                # the first minimum: ties go to the lowest frame index
            if on_pick is not None:
                on_pick(dict(step=cnt, pick=pick, latent=list(latent), obs=sorted(obs), candidates=candidates,
                             means=[float(m) for m in means], best=candidates[best], scores=raw,
                             videos=[int(v) for v in videos], t=[int(t) for t in ts]))
            obs.add(candidates[best])
            log(f"(Step #{cnt}) Best frame {candidates[best]}, metric = {means[best]}")
            update_schedule_on_disk(partial_path, {cnt: sorted(obs)}, force=False)
        finished[cnt] = sorted(obs)
        log(f"Step #{cnt}:\n\tLatent: {latent}\n\tObserved: {finished[cnt]}")
        update_schedule_on_disk(schedule_path, {cnt: finished[cnt]})
    return finished


def noise_offset(cnt, pick, dataset_index, n_videos, blocks_per_item):
    """Philox block offset of a video's noise in pick `pick` of inference step `cnt`: slot ((cnt * 256 + pick) * n_videos +
    dataset_index) of `blocks_per_item` blocks each (>= the 4-element blocks of the longest window), so no two (step, pick,
    video) triples share a block.  Together with the Philox key (--seed) this is all the noise depends on."""
    assert 0 <= pick < 256 and 0 <= dataset_index < n_videos
    off = ((cnt * 256 + pick) * n_videos + dataset_index) * blocks_per_item
    assert off + blocks_per_item < 2 ** 63, "noise offset beyond the Philox counter"
    return off


class EngineScorer:
    """search's scorer on the HIP engine.  The (candidate, video) pairs of a pick are packed into batches of `batch_size`
    windows -- observed frames ascending, then the latents (video_nll._window_table) -- and each batch is ONE
    diffusion.score_windows call; the scores come back once per pick."""

    def __init__(self, model, diffusion, dataset, T, max_frames, batch_size, seed=0, clip_denoised=True, suffix_skip=True):
        self.model, self.diffusion, self.dataset, self.T = model, diffusion, dataset, T
        self.batch_size, self.seed, self.clip_denoised, self.suffix_skip = batch_size, seed, clip_denoised, suffix_skip
        frame = dataset[0][0].shape[1:]
        self.blocks_per_item = (max_frames * int(np.prod(frame)) + 3) // 4
        self.calls = 0

    @torch.no_grad()
    def __call__(self, cnt, pick, latent, obs, candidates, videos, ts):
        from .video_nll import _window_table
        dev = self.model.device
        clips = torch.stack([self.dataset[v][0][:self.T] for v in videos]).to(dev)            # the pick's videos, once
        offs = [noise_offset(cnt, pick, v, len(self.dataset), self.blocks_per_item) for v in videos]
        pairs = [(ci, vi) for ci in range(len(candidates)) for vi in range(len(videos))]
        out = []
        for k in range(0, len(pairs), self.batch_size):
            chunk = pairs[k:k + self.batch_size]
            table, observed, lat = _window_table([sorted(obs + [candidates[ci]]) for ci, _ in chunk], [latent] * len(chunk), len(chunk))
            assert table.shape[1] * int(np.prod(clips.shape[2:])) <= 4 * self.blocks_per_item, "window longer than --max_frames"
            vid = torch.tensor([vi for _, vi in chunk], device=dev)[:, None]
            x0 = clips[vid, table.to(dev)]
            mask = lambda m: m.to(device=dev, dtype=x0.dtype)[:, :, None, None, None]          # noqa: E731
            kw = dict(frame_indices=table.to(dev), obs_mask=mask(observed), latent_mask=mask(lat),
                      kinda_marg_mask=torch.zeros_like(mask(lat)))
            t = torch.tensor([ts[vi] for _, vi in chunk], device=dev)
            out.append(self.diffusion.score_windows(self.model, x0, t, kw, None, self.seed, [offs[vi] for _, vi in chunk],
                                                    clip_denoised=self.clip_denoised, suffix_skip=self.suffix_skip))
            self.calls += 1
        scores = torch.cat(out).cpu().numpy().reshape(len(candidates), len(videos))
        self.model.check_device_errors()
        return scores


def selected_step(args, environ=None):
    """--step, else --task_id, else SLURM_ARRAY_TASK_ID (:223-224), else None: every step."""
    environ = os.environ if environ is None else environ
    for v in (getattr(args, "step", None), getattr(args, "task_id", None)):
        if v is not None:
            return int(v)
    return int(environ["SLURM_ARRAY_TASK_ID"]) if "SLURM_ARRAY_TASK_ID" in environ else None


def run_directory(args):
    """Where `video_sample --optimality <args.optimality>` with the same options keeps its files (video_sample.run): named
    from the options as given -- call this before --max_frames / --T take their defaults from the model and the dataset."""
    assert getattr(args, "optimality", None) is not None
    run_id = test_util.get_eval_run_identifier(args)
    if args.eval_dir is None:
        alias = getattr(args, "out_dir", None)
        args.eval_dir = alias if alias is not None else (None if args.checkpoint_path else "results/synthetic")
    out_dir = test_util.get_model_results_path(args) / run_id
    if getattr(args, "dataset_partition", None) == "variable_length":
        out_dir = out_dir / "variable_length"
    return out_dir


def run(args, create=None, device=None, on_pick=None, scorer_wrap=None):
    """The body of the reference's script (:467-531) on the engine; returns the path of optimal_schedule.pt."""
    from . import dist as vdist
    from .video_sample import load_model, open_videos
    if args.subset_size is None:
        args.subset_size = args.num_timesteps * 10                                          # :467-468
    check_options(args.optimality, args.inference_mode, args.subset_size, args.num_timesteps)
    rank, local_rank, world = vdist.init(device_index=device.index if device is not None and device.type == "cuda" else None)
    if world != 1:
        raise NotImplementedError("video_optimal_schedule: one process; deal the inference steps with --step / --task_id")
    if device is None:
        device = torch.device("cuda", local_rank)
        torch.cuda.set_device(device)
    out_dir = run_directory(args)
    model, diffusion = load_model(args, device, rank, world, create=create)
    if args.max_frames is None:
        args.max_frames = model.config.get("max_frames") or model.config["T"]
    print(f"max_frames = {args.max_frames}")
    dataset = open_videos(args)
    if args.T is None:
        args.T = int(dataset[0][0].shape[0])
    os.makedirs(out_dir, exist_ok=True)
    schedule_path = out_dir / "optimal_schedule.pt"
    print(f"Saving the optimal inference schedule to {schedule_path}")
    if args.batch_size is None:
        args.batch_size = 16                                                                 # :502-503
    strategy = inference_util.inference_strategies[args.inference_mode](
        video_length=args.T, num_obs=args.obs_length, max_frames=args.max_frames, step_size=args.step_size)
    scorer = EngineScorer(model, diffusion, dataset, args.T, args.max_frames, args.batch_size, seed=getattr(args, "seed", 0))
    if scorer_wrap is not None:
        scorer = scorer_wrap(scorer)
    search(strategy, len(dataset), scorer, optimality=args.optimality, subset_size=args.subset_size,
           num_timesteps=args.num_timesteps, num_diffusion_timesteps=diffusion.num_timesteps, schedule_path=schedule_path,
           only_step=selected_step(args), on_pick=on_pick)
    return schedule_path


def build_parser():
    import argparse
    from .video_sample import add_job_arguments
    ap = add_job_arguments(argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter))
    # the options of the run directory are video_sample's own (the file must land where that job looks); the reference's defaults
    # where they differ: --optimality linspace-t, --batch_size unset -> 16
    ap.set_defaults(optimality="linspace-t", batch_size=None)
    ap.add_argument("--num_timesteps", type=int, default=10, help="size of the timestep grid a pick is scored on")
    ap.add_argument("--step", type=int, default=None,
                    help="only this inference step (as --task_id / SLURM_ARRAY_TASK_ID): one array task per step")
    for a in ap._actions:
        if a.dest == "subset_size":
            a.help = "videos per pick; default 10 * --num_timesteps, and a multiple of it"
        if a.dest == "optimality":
            a.help = "which search writes <eval_dir>/optimal_schedule.pt"
    return ap


def main(argv=None):
    return run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
