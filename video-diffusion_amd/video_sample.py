"""Windowed conditional sampling: the caller of the hot path (scripts/video_sample.py:31-47, 50-190,
266-271 of the reference), driving the HIP engine.

    python -m video_diffusion_amd.video_sample --synthetic --inference_mode autoreg --T 32 \
        --obs_length 4 --max_frames 10 --step_size 2 --timestep_respacing ddim50 --out_dir /tmp/samples

`infer_video` keeps the reference's contract: `batch` (B, T, C, H, W) in [-1, 1]; the first
`obs_length` frames are observed; each window starts from `x0.clone()` (observed frames + whatever
the latent slots currently hold, zeros at first -- SURVEY F5), walks every respaced timestep through
`diffusion.p_sample`, and writes the last `n_latent` frames back.  One H2D transfer of the window's
inputs and one D2H of its result per window; nothing crosses the host inside the step loop.
No datasets or checkpoints ship with the reference: the CLI reads its test videos from a `.npy` file
(`--videos`) or makes synthetic ones (`--synthetic`), and takes either a checkpoint given on the command line or the
closed-form weights.  The job around `infer_video` -- which videos (`--indices`, `--task_id`, `--subset_size`), how many
samples of each (`--num_samples`, `--sample_idx`), what is already on disk and therefore skipped BEFORE any denoise
step runs -- follows scripts/video_sample.py:192-239,570-640; `run()` is that body.
"""
import argparse
import contextlib
import logging
import math
import os

import numpy as np
import torch

from . import _lib, inference_util
from .gaussian_diffusion import (SAMPLERS, _check_guidance, _sampler_step, check_blur_kernel, check_blur_measurement, check_freeu,
                                 check_linear_measurement, check_loss_guidance, check_measurement, check_separable_operator, check_zeta,
                                 gaussian_kernel, resize_matrix, separable_pinv)
from .script_util import (args_to_dict, create_video_model_and_diffusion, str2bool,
                          video_model_and_diffusion_defaults)
from .weights_init import synth_param

logger = logging.getLogger("video_sample")
drange = [-1, 1]


def get_masks(x0, num_obs):
    """video_sample.py:31-47: first `num_obs` frames observed, the rest latent, none kinda-marginal."""
    obs_mask = torch.zeros_like(x0[:, :, :1, :1, :1])
    obs_mask[:, :num_obs] = 1
    latent_mask = 1 - obs_mask
    kinda_marg_mask = torch.zeros_like(x0[:, :, :1, :1, :1])
    return obs_mask, latent_mask, kinda_marg_mask


@torch.no_grad()
def infer_video(mode, model, diffusion, batch, max_frames, obs_length, step_size=1, optimal_schedule_path=None, *,
                use_gradient_method=False, observed_frames="x_0", sampler="p_sample", eta=0.0, executor="eager",
                adaptive_distance="lpips", prefix_cache=False, suffix_skip=False, save_all_timesteps=False, cfg_scale=1.0,
                cfg_rescale=0.0, dynamic_threshold=None, known_mask=None, known_video=None, jump_length=1, n_resample=1,
                measurement=None, sr_scale=1, gray=False, dps_zeta=None, loss_fn=None, cotangent_fn=None, loss_scale=None,
                loss_normalize=False, particles=1, reward_fn=None, reward_scale=1.0, ess_threshold=0.5, particle_measurement=None,
                sigma_y=None, blur_kernel=None, operator=None, operator_rtol=1e-3, freeu=None, freeu_adaptive=False):
    """video_sample.py:50-190.  Returns (samples ndarray (B,T,C,H,W), all_timestep_samples): the second is the
    (B, num_timesteps, T, C, H, W) record of every step's output when `save_all_timesteps` (the reference's
    `args.save_all_timesteps`, :84-91,168-186; eager executor only -- the graph keeps a window on the device), else
    the reference's one-element placeholder.

    'adaptive-*' modes (:74,94-95,104-118,176-183): the strategy sees the current samples before every window and hands
    back one index list per batch item.  `adaptive_distance` is the reference's `distance` ('lpips' is what its script
    passes and needs `inference_util.load_lpips_weights` or `set_lpips_embedder`; 'l2' works on the frames themselves).

    executor='eager' (default): one `diffusion.p_sample` call per step from the host with `th.randn_like` noise, the
    reference's own loop.  executor='graph': each window's step loop runs on the window executor -- one captured hipGraph
    per window shape, step index and noise counter on the device (executor.py).  The device is the bottleneck either way
    (the eager host loop runs ahead of it; measured 7.28 ms eager vs 7.49 ms graph per step at B=1 x T=16 and 28.9 vs 29.1
    at the headline window, profiles/r03a_*), so the graph is an option -- a host too slow to stay ahead, one launch per
    step to trace -- not the default.  `prefix_cache` (graph executor, 'x_0' mode): the observed frames' activations before
    the first attention layer once per window instead of once per step (executor.py; 2.6 % at 4 observed frames of 16, 12 %
    at 10 of 20, profiles/r03x_*).  `suffix_skip` (graph executor, 'x_0' / 'x_t_minus_1'): everything behind the last attention
    layer runs without the purely observed frames, whose step output this function never reads (write_back keeps the latent
    frames only); the latent frames are those of the full step (executor.py, include/vd_amd.h: vd_set_window_suffix_skip).

    sampler: 'p_sample' (default), 'ddim' (ddim_sample with `eta`) or 'dpmpp_2m' (dpmpp_2m_sample, this project's extension: the
    second-order multistep solver; each window starts without history, so its first step is first-order; on both executors; meant for
    timestep_respacing='logsnrN') or 'dpmpp_2m_sde' (dpmpp_2m_sde_sample, this project's extension: the stochastic second-order
    multistep solver; history per window like 'dpmpp_2m'; `eta` is not read; its noise is the engine's Philox stream on BOTH executors,
    from a seed drawn per window from torch's global generator, so the two executors agree to the bit; refused by name with
    use_gradient_method and dps_zeta; meant for timestep_respacing='logsnrN') or 'unipc' (unipc_sample, this project's extension: UniPC,
    dpmpp_2m's predictor plus a corrector that reuses the step's own forward -- third order at no further network call; state per window,
    the first step of each first-order; no noise, both executors agree to the bit; refused by name with use_gradient_method, dps_zeta and
    known_mask; meant for timestep_respacing='logsnrN' with N of 20 or more).

    cfg_scale (this project's extension, both executors, every sampler): the weight w of classifier-free guidance on each window's
    observed frames -- every step runs on out_u + w (out_c - out_u), out_u being the network output with the window's obs_mask
    zeroed (gaussian_diffusion.py: p_sample).  1.0 (default) is the sampling as it always was; any other value costs two forwards
    per step and is refused together with use_gradient_method, prefix_cache (graph) and suffix_skip (graph).

    cfg_rescale, dynamic_threshold (this project's extensions, both executors, every sampler): the whole of this function's work runs
    inside `diffusion.guidance_scope(model, cfg_rescale, dynamic_threshold)` -- guidance rescale (phi in [0, 1], acts with
    cfg_scale != 1) and dynamic thresholding (the percentile p in (0, 1], in place of the clamp of x_0), each with its statistic per
    batch item over the window's latent frames (gaussian_diffusion.py: guidance_scope).  With both at their defaults (0.0, None) no
    scope is entered and the engine is not touched.  Refused together with use_gradient_method, prefix_cache and suffix_skip.

    known_mask, known_video, jump_length, n_resample (this project's extension: pixel-mask inpainting, RePaint; both executors, every
    sampler; composes with cfg_scale, cfg_rescale and dynamic_threshold): known_mask (T, H, W) or (B, T, H, W) over the WHOLE video, nonzero
    = known; known_video (B, T, C, H, W), default `batch`.  Per window both are gathered by the window's frame indices exactly as x0 is
    (per item in the adaptive-* modes) and every step ends in the merge pass on the window's latent frames (gaussian_diffusion.py:
    known_region_scope): the known pixels of every generated frame come out equal to known_video.  n_resample > 1 walks
    respace.repaint_schedule(num_timesteps - 1, jump_length, n_resample) in every window.  The noise of the merge and of the jumps is the
    engine's Philox stream on both executors, from a seed drawn per window from torch's global generator (the sampler's own noise stays
    th.randn_like on the eager executor): with a sampler that draws none, the two executors agree to the bit.  Refused with
    use_gradient_method, prefix_cache and suffix_skip, and n_resample > 1 with save_all_timesteps (the record has one slot per
    timestep).  With known_mask=None no scope is entered and the engine is not touched.

    measurement, sr_scale, gray (this project's extension: zero-shot restoration, DDNM; both executors, every sampler; composes with
    cfg_scale, cfg_rescale and dynamic_threshold): measurement = y over the WHOLE video, (B, T, Cy, H / sr_scale, W / sr_scale) with
    Cy = 1 when gray else 3 -- what diffusion.measure(video, sr_scale, gray) returns.  Per window it is gathered by the window's frame
    indices exactly as x0 is (per item in the adaptive-* modes) and the x_0 prediction of every step is projected onto it on the
    window's latent frames (gaussian_diffusion.py: measurement_scope): measure(generated frames) == y up to rounding.  The observed
    frames still come from `batch`, untouched.  Refused by name with use_gradient_method, prefix_cache, suffix_skip and known_mask.  With
    measurement=None no scope is entered and the engine is not touched.

    dps_zeta (this project's extension: diffusion posterior sampling, DPS, for a measurement that carries NOISE; eager executor,
    samplers 'p_sample' and 'ddim'): with a step size zeta given, the measurement -- gathered per window exactly as above -- drives
    gaussian_diffusion.py: dps_scope in place of the projection: every step is the plain step followed by a move of the window's latent
    frames down the gradient of ||y - A x_0(x_t)||_2, through the whole UNet (windows of at most 32 frames).  Refused by name before the
    engine is touched: no measurement, executor='graph', prefix_cache, suffix_skip, sampler='dpmpp_2m', use_gradient_method, known_mask,
    cfg_scale != 1, cfg_rescale and dynamic_threshold.  None (default): the projection, as before.

    loss_fn, cotangent_fn, loss_scale, loss_normalize (this project's extension: loss-guided sampling; eager executor, samplers
    'p_sample' and 'ddim'): with one of the two functions given, every window's step loop runs inside gaussian_diffusion.py:
    loss_guidance_scope(model, loss_fn, cotangent_fn=cotangent_fn, scale=loss_scale, normalize=loss_normalize) -- every step is the
    plain step followed by a move of the window's latent frames down the gradient of the caller's function of the step's x_0
    prediction, through the whole UNet (windows of at most 32 frames).  The function sees a WINDOW (B, Tw, 3, H, W), observed frames
    first, not the whole video.  Refused by name before the engine is touched: both or a missing loss_scale (ValueError),
    executor='graph', prefix_cache, suffix_skip, the samplers 'dpmpp_2m', 'dpmpp_2m_sde' and 'unipc', use_gradient_method, known_mask,
    a measurement, cfg_scale != 1, cfg_rescale and dynamic_threshold.  Both None (default): no scope is entered.

    particles, reward_fn, reward_scale, ess_threshold, particle_measurement, sigma_y (this project's extension: particle steering,
    gradient-free guidance by resampling; gaussian_diffusion.py: steering_scope): with particles = K > 1 every video of the batch runs
    as K consecutive items, every window's step loop inside steering_scope -- reward_fn(x0, t) on the WINDOW's x_0 prediction
    (B K, Tw, 3, H, W), eager executor only, or the built-in reward of a noisy measurement particle_measurement = y over the WHOLE
    video (the layout of `measurement`, operator sr_scale / gray, noise level sigma_y), gathered per window like x0, on both executors.
    Behind each window the particle 'chosen' at t == 0 becomes that window's result for all K particles of its video, so the next window
    conditions on one history; the return shape is unchanged.  With the built-in reward and sampler='dpmpp_2m_sde' the two executors
    give equal bits.  Every sampler that draws noise, cfg_scale, cfg_rescale and dynamic_threshold are served, and windows of up to 128
    frames.  Refused by name before the engine is touched: use_gradient_method, known_mask, a measurement (the exact projection),
    dps_zeta, loss_fn / cotangent_fn, prefix_cache, suffix_skip, save_all_timesteps, a sampler that draws no noise ('ddim' at eta = 0,
    'dpmpp_2m', 'unipc'), and a reward_fn with executor='graph'.  particles=1 (default): nothing of this runs.

    blur_kernel (this project's extension: deblurring; gaussian_diffusion.py: deblur_scope): the measurement is a blurred, noisy copy of
    the WHOLE video, of the video's own shape -- what diffusion.blur(video, blur_kernel) returns, plus noise -- and blur_kernel one real
    (k, k) kernel, k odd and at most 15 (check_blur_kernel); sr_scale and gray stay at their defaults.  It takes one of the two paths that
    accept a noisy measurement, each with its own rules above: dps_zeta= (deblur_scope in place of dps_scope), or particles=K, sigma_y=
    (the built-in reward on the blur; `measurement` is then read as particle_measurement when that is not given).  With neither it is
    refused by name: the exact projection of measurement_scope has no pseudo-inverse for a blur.

    operator, operator_rtol (this project's extension: separable linear measurements; gaussian_diffusion.py: linear_measurement_scope):
    operator=(A_h, A_w), A_h (Mh, H) and A_w (Mw, W), makes the measurement one under y[b, t, c] = A_h x[b, t, c] A_w^T over the WHOLE
    video, (B, T, 3, Mh, Mw) -- what diffusion.measure_separable(video, A_h, A_w) returns; sr_scale, gray and blur_kernel stay at their
    defaults.  It takes any of the three paths, each with its own rules above: neither option (the exact projection, with the truncated
    pseudo-inverses separable_pinv(A, operator_rtol); both executors, every sampler a measurement is served with), dps_zeta=
    (linear_dps_scope), or particles=K, sigma_y= (the built-in reward on the operator; `measurement` is then read as
    particle_measurement when that is not given; both executors).

    freeu, freeu_adaptive (this project's extension: FreeU; both executors, every sampler): freeu=(b1, b2, s1, s2) runs the whole of this
    function's work inside `diffusion.freeu_scope(model, b1, b2, s1, s2, adaptive=freeu_adaptive)` -- in every forward the backbone half
    of the concat at the two lowest-resolution decoder levels is scaled and the lowest frequencies of the skip half are damped
    (gaussian_diffusion.py: freeu_scope).  Under a sampler that draws no noise the two executors agree to the bit.  Composes with
    cfg_scale, cfg_rescale, dynamic_threshold, known_mask, a measurement and particles; refused by name before the engine is touched
    with use_gradient_method, dps_zeta, loss_fn / cotangent_fn, prefix_cache and suffix_skip.  None (default): no scope is entered and
    the engine is not touched."""
    lin = None
    if operator is not None:
        if not isinstance(operator, (tuple, list)) or len(operator) != 2:     # before anything touches the engine
            raise ValueError("operator is a pair (A_h, A_w)")
        lin = check_separable_operator(*operator)
        if blur_kernel is not None or not (sr_scale == 1 and gray is False):
            raise ValueError("operator together with blur_kernel, sr_scale or gray is not served: leave them at their defaults")
        if measurement is None and particle_measurement is None:
            raise ValueError("operator needs a measurement (measurement=: measure_separable(video, A_h, A_w))")
        separable_pinv(lin[0], operator_rtol)                               # (the check of operator_rtol)
        steered = particles != 1 or sigma_y is not None or particle_measurement is not None
        if steered and dps_zeta is None and particle_measurement is None:
            measurement, particle_measurement = None, measurement
    blur_w = None
    if blur_kernel is not None:
        blur_w = check_blur_kernel(blur_kernel)                             # before anything touches the engine
        if not (sr_scale == 1 and gray is False):
            raise ValueError("blur_kernel together with sr_scale or gray is not served: leave them at their defaults")
        if measurement is None and particle_measurement is None:
            raise ValueError("blur_kernel needs a measurement (measurement=: the blurred copy of the video)")
        steered = particles != 1 or sigma_y is not None or particle_measurement is not None
        if dps_zeta is None and not steered:
            raise _lib.VdError("blur_kernel without dps_zeta or particles is not served: measurement_scope together with a blur is refused, "
                               "the exact projection has no pseudo-inverse for this operator")
        if steered and dps_zeta is None and particle_measurement is None:
            measurement, particle_measurement = None, measurement
    steer = _check_particles(particles, reward_fn, reward_scale, ess_threshold, particle_measurement, sigma_y, batch, sr_scale, gray, sampler, eta,
                             executor, blur_w if lin is None else lin, [("use_gradient_method", use_gradient_method), ("known_mask", known_mask is not None),
                                        ("a measurement", measurement is not None), ("dps_zeta", dps_zeta is not None),
                                        ("loss_fn / cotangent_fn", loss_fn is not None or cotangent_fn is not None), ("prefix_cache", prefix_cache),
                                        ("suffix_skip", suffix_skip), ("save_all_timesteps", save_all_timesteps)])
    loss_guided = loss_fn is not None or cotangent_fn is not None
    # what a step that moves the latent frames behind the plain step (loss_guidance_scope, dps_scope) is not served with, in the order it is
    # refused; the three that dps_zeta leaves to the checks of the measurement below are marked
    moved_step = [("executor='graph'", executor == "graph", False), ("prefix_cache", prefix_cache, False), ("suffix_skip", suffix_skip, False),
                  *((f"sampler='{s}'", sampler == s, False) for s, row in SAMPLERS.items() if row.carry),       # the multistep samplers
                  ("use_gradient_method", use_gradient_method, True), ("known_mask", known_mask is not None, True),
                  ("a measurement", measurement is not None, True), ("cfg_scale != 1", float(cfg_scale) != 1.0, False),
                  ("cfg_rescale", float(cfg_rescale) != 0.0, False), ("dynamic_threshold", dynamic_threshold is not None, False)]
    if loss_guided or loss_scale is not None:
        if loss_scale is None:
            raise ValueError("loss_fn / cotangent_fn need a step size (loss_scale=)")
        loss_scale = check_loss_guidance(loss_fn, cotangent_fn, loss_scale)
        for name, on, _ in moved_step:
            if on:
                raise _lib.VdError(f"{name} together with loss_fn / cotangent_fn (loss_guidance_scope) is not served")
    if dps_zeta is not None:
        dps_zeta = check_zeta(dps_zeta)
        if measurement is None:
            raise ValueError("dps_zeta needs a measurement (measurement=, sr_scale=, gray=)")
        for name, on, left_to_measurement in moved_step:
            if on and not left_to_measurement:
                raise _lib.VdError(f"{name} together with dps_zeta is not served")
    if sampler in ("dpmpp_2m_sde", "unipc") and use_gradient_method:
        raise NotImplementedError(f"sampler='{sampler}' together with use_gradient_method")
    if sampler == "unipc" and known_mask is not None:
        raise NotImplementedError("sampler='unipc' together with known_mask: the corrector rebuilds the state from its own, the merge of a "
                                  "known region behind the pass would be discarded")
    if measurement is not None:
        measurement_v = (check_linear_measurement(torch.as_tensor(measurement), batch.shape, *lin) if lin is not None
                         else check_measurement(torch.as_tensor(measurement), batch.shape, sr_scale, gray) if blur_w is None     # before anything touches the engine
                         else check_blur_measurement(torch.as_tensor(measurement), batch.shape)).cpu()
        if known_mask is not None:
            raise _lib.VdError("a measurement together with a known region (known_mask) is not served")
        if use_gradient_method:
            raise _lib.VdError("use_gradient_method together with a measurement is not served")
    if known_mask is not None:
        for name, on in (("use_gradient_method", use_gradient_method), ("prefix_cache", prefix_cache), ("suffix_skip", suffix_skip)):
            if on:
                raise NotImplementedError(f"{name} together with known_mask")
        if int(n_resample) != 1 and save_all_timesteps:
            raise NotImplementedError("n_resample > 1 together with save_all_timesteps: the record has one slot per timestep")
        from .respace import repaint_schedule
        repaint_schedule(diffusion.num_timesteps - 1, jump_length, n_resample)     # the range checks, before anything touches the engine
        known_mask_v, known_video_v = video_known_region(batch, known_mask, known_video)
    if freeu is not None:
        if not isinstance(freeu, (tuple, list)) or len(freeu) != 4:          # before anything touches the engine
            raise ValueError("freeu is four numbers (b1, b2, s1, s2)")
        consts = check_freeu(*freeu)
        for name, on in (("use_gradient_method", use_gradient_method), ("dps_zeta", dps_zeta is not None), ("loss_fn / cotangent_fn", loss_guided),
                         ("prefix_cache", prefix_cache), ("suffix_skip", suffix_skip)):
            if on:
                raise NotImplementedError(f"{name} together with freeu")
        with diffusion.freeu_scope(model, *consts, adaptive=freeu_adaptive):
            return infer_video(mode, model, diffusion, batch, max_frames, obs_length, step_size, optimal_schedule_path,
                               observed_frames=observed_frames, sampler=sampler, eta=eta, executor=executor, adaptive_distance=adaptive_distance,
                               save_all_timesteps=save_all_timesteps, cfg_scale=cfg_scale, cfg_rescale=cfg_rescale,
                               dynamic_threshold=dynamic_threshold, known_mask=known_mask, known_video=known_video, jump_length=jump_length,
                               n_resample=n_resample, measurement=measurement, sr_scale=sr_scale, gray=gray, particles=particles,
                               reward_fn=reward_fn, reward_scale=reward_scale, ess_threshold=ess_threshold,
                               particle_measurement=particle_measurement, sigma_y=sigma_y, blur_kernel=blur_kernel, operator=operator,
                               operator_rtol=operator_rtol)
    if float(cfg_rescale) != 0.0 or dynamic_threshold is not None:
        _check_guidance(cfg_rescale, dynamic_threshold)                     # before anything touches the engine
        for name, on in (("use_gradient_method", use_gradient_method), ("prefix_cache", prefix_cache), ("suffix_skip", suffix_skip)):
            if on:
                raise NotImplementedError(f"{name} together with cfg_rescale / dynamic_threshold")
        with diffusion.guidance_scope(model, cfg_rescale=cfg_rescale, dynamic_threshold=dynamic_threshold):
            return infer_video(mode, model, diffusion, batch, max_frames, obs_length, step_size, optimal_schedule_path,
                               use_gradient_method=use_gradient_method, observed_frames=observed_frames, sampler=sampler, eta=eta,
                               executor=executor, adaptive_distance=adaptive_distance, prefix_cache=prefix_cache, suffix_skip=suffix_skip,
                               save_all_timesteps=save_all_timesteps, cfg_scale=cfg_scale, known_mask=known_mask, known_video=known_video,
                               jump_length=jump_length, n_resample=n_resample, measurement=measurement, sr_scale=sr_scale, gray=gray,
                               particles=particles, reward_fn=reward_fn, reward_scale=reward_scale, ess_threshold=ess_threshold,
                               particle_measurement=particle_measurement, sigma_y=sigma_y, blur_kernel=blur_kernel,
                               operator=operator, operator_rtol=operator_rtol)
    step_sampler = sampler if sampler in SAMPLERS and not SAMPLERS[sampler].up else "ddim"    # (the eager step: any other name is ddim_sample)
    adaptive = "adaptive" in mode
    if steer is not None:                  # every video as K consecutive items; the return takes one of each group again
        batch = batch.repeat_interleave(steer["K"], dim=0)
    B, T, C, H, W = batch.shape
    device = model.device
    samples = torch.zeros_like(batch).cpu()
    samples[:, :obs_length] = batch[:, :obs_length].cpu()
    if "goal-directed" in mode:
        samples[:, -5] = batch[:, -5].cpu()              # the reference hands over ONE goal frame (index -5) here
    schedule = iter(inference_util.inference_strategies[mode](
        video_length=T, num_obs=obs_length, max_frames=max_frames, step_size=step_size,
        optimal_schedule_path=optimal_schedule_path, **(dict(distance=adaptive_distance) if adaptive else {})))
    timesteps = list(range(diffusion.num_timesteps))[::-1]
    t_tensors = None
    if save_all_timesteps:
        all_timestep_samples = torch.zeros([B, diffusion.num_timesteps, T, C, H, W])
        all_timestep_samples[:, :, :obs_length] = samples[:, :obs_length].unsqueeze(1)
    else:
        all_timestep_samples = torch.zeros([1])
    use_graph = (executor == "graph" and observed_frames in ("x_0", "x_t", "x_t_minus_1") and not use_gradient_method
                 and not save_all_timesteps)
    if use_graph:
        from .executor import WindowExecutor
        wex = getattr(model, "_window_executor", None)
        if wex is None or wex.diffusion is not diffusion or wex.prefix_cache != bool(prefix_cache) or wex.suffix_skip != bool(suffix_skip):
            wex = model._window_executor = WindowExecutor(model, diffusion, prefix_cache=prefix_cache, suffix_skip=suffix_skip)
    while True:
        if adaptive:
            schedule.set_videos(samples)
        try:
            obs_frame_indices, latent_frame_indices = next(schedule)
        except StopIteration:
            break
        logger.info(f"Conditioning on {sorted(obs_frame_indices)} frames, predicting {sorted(latent_frame_indices)}.")
        if adaptive:                   # one (obs, latent) index row per batch item
            frame_indices = torch.cat([torch.tensor(obs_frame_indices, dtype=torch.int64).reshape(B, -1),
                                       torch.tensor(latent_frame_indices, dtype=torch.int64).reshape(B, -1)], dim=1)
            x0 = torch.stack([samples[i, fi] for i, fi in enumerate(frame_indices)], dim=0).clone()
            n_obs_w, n_latent = len(obs_frame_indices[0]), len(latent_frame_indices[0])
        else:
            x0 = torch.cat([samples[:, obs_frame_indices], samples[:, latent_frame_indices]], dim=1).clone()
            frame_indices = torch.cat([torch.tensor(obs_frame_indices, dtype=torch.int64),
                                       torch.tensor(latent_frame_indices, dtype=torch.int64)], dim=0).repeat((B, 1))
            n_obs_w, n_latent = len(obs_frame_indices), len(latent_frame_indices)
        obs_mask, latent_mask, kinda_marg_mask = get_masks(x0, n_obs_w)

        def write_back(local, every_step=None):
            if adaptive:
                for i, li in enumerate(latent_frame_indices):
                    samples[i, li] = local[i, n_obs_w:].cpu()
                    if every_step is not None:
                        all_timestep_samples[i, :, li] = every_step[i, :, n_obs_w:].cpu()
            else:
                samples[:, latent_frame_indices] = local[:, -n_latent:].cpu()
                if every_step is not None:
                    all_timestep_samples[:, :, latent_frame_indices] = every_step[:, :, -n_latent:].cpu()
        x0, obs_mask, latent_mask, kinda_marg_mask, frame_indices = [
            v.to(device) for v in (x0, obs_mask, latent_mask, kinda_marg_mask, frame_indices)]
        model_kwargs = dict(frame_indices=frame_indices, x0=x0, obs_mask=obs_mask, latent_mask=latent_mask,
                            kinda_marg_mask=kinda_marg_mask, x_t_minus_1=x0, observed_frames=observed_frames)
        if t_tensors is None:          # the reference re-creates this tensor every step (video_sample.py:154-155)
            t_tensors = [torch.tensor([ts] * B, device=device) for ts in range(diffusion.num_timesteps)]
        k_src = k_mask = None
        if known_mask is not None:     # the window's share of the region, gathered like x0
            k_src, k_mask = (gather_window(v, frame_indices).to(device) for v in (known_video_v, known_mask_v))
        y_w = None
        if measurement is not None:    # ... and so is the window's share of the measurement
            y_w = gather_window(measurement_v, frame_indices).to(device)
        if steer is not None:
            pm_w = None if steer["y"] is None else gather_window(steer["y"], frame_indices).to(device)
            if use_graph:
                wex.begin(x0, model_kwargs, sampler=sampler, eta=eta, renoise=False, cfg_scale=cfg_scale, particles=steer["K"],
                          reward_scale=steer["scale"], ess_threshold=steer["tau"], particle_measurement=pm_w, particle_sr_scale=sr_scale,
                          particle_gray=gray, sigma_y=sigma_y, blur_kernel=None if pm_w is None else blur_w,
                          operator=None if pm_w is None else lin)
                local_samples = wex.run(diffusion.num_timesteps).clone()
                chosen = wex.particle_state()["chosen"]
            else:
                local_samples, chosen = _eager_particle_window(model, diffusion, x0, model_kwargs, step_sampler, eta, cfg_scale, steer, pm_w,
                                                               sr_scale, gray, sigma_y, t_tensors, timesteps, blur_w, lin)
            write_back(_chosen_for_all(local_samples, chosen, steer["K"]))
            model.check_device_errors()
            continue
        if use_graph:
            # renoise=False: like the eager loop below (and scripts/video_sample.py:149-166), every step reads x_t_minus_1 = x0 as it is
            write_back(wex.sample_window(x0, model_kwargs, sampler=sampler, eta=eta, renoise=False, cfg_scale=cfg_scale, known_src=k_src,
                                         known_mask=k_mask, jump_length=jump_length, n_resample=n_resample, measurement=y_w,
                                         sr_scale=sr_scale, gray=gray, operator=None if y_w is None else lin, operator_rtol=operator_rtol))
            model.check_device_errors()
            continue
        if known_mask is not None:
            local_samples, trace = _eager_known_window(model, diffusion, x0, model_kwargs, k_src, k_mask, step_sampler, eta, cfg_scale, jump_length,
                                                       n_resample, save_all_timesteps)
            write_back(local_samples, None if trace is None else torch.stack(trace, dim=1))
            model.check_device_errors()
            continue
        local_samples = x0.clone()
        trace = [] if save_all_timesteps else None
        carry = None                                        # dpmpp_2m, dpmpp_2m_sde: the history is the window's own; and so is unipc's state
        step_kw = dict(return_attn_weights=False, use_gradient_method=use_gradient_method) if sampler == "p_sample" else {}
        sde_seed = None
        if SAMPLERS[step_sampler].noise == "philox":        # ... and the noise what the window executor would draw (its seed, its ranges)
            sde_seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        if loss_guided:
            scope = diffusion.loss_guidance_scope(model, loss_fn, cotangent_fn=cotangent_fn, scale=loss_scale, normalize=loss_normalize)
        elif y_w is None:
            scope = contextlib.nullcontext()
        elif lin is not None:
            scope = diffusion.linear_dps_scope(model, y_w, *lin, zeta=dps_zeta) if dps_zeta is not None \
                else diffusion.linear_measurement_scope(model, y_w, *lin, rtol=operator_rtol)
        elif dps_zeta is not None and blur_w is not None:
            scope = diffusion.deblur_scope(model, y_w, blur_w, zeta=dps_zeta)
        elif dps_zeta is not None:
            scope = diffusion.dps_scope(model, y_w, sr_scale, gray, zeta=dps_zeta)
        else:
            scope = diffusion.measurement_scope(model, y_w, sr_scale, gray)
        with scope:
            for timestep in timesteps:
                philox = None if sde_seed is None else (sde_seed, (diffusion.num_timesteps - 1 - timestep) * local_samples.numel())
                out, carry = _sampler_step(diffusion, step_sampler, model, local_samples, t_tensors[timestep], carry, cfg_scale, eta, philox,
                                           clip_denoised=True, model_kwargs=model_kwargs, **step_kw)
                local_samples = out["sample"]
                if trace is not None:
                    trace.append(local_samples.clone())
        write_back(local_samples, None if trace is None else torch.stack(trace, dim=1))
        model.check_device_errors()    # once per window (write_back has synchronised): a non-finite network output of any of its steps raises here
    return (samples if steer is None else samples[::steer["K"]]).numpy(), all_timestep_samples.numpy()


def _check_particles(particles, reward_fn, reward_scale, ess_threshold, y, sigma_y, batch, sr_scale, gray, sampler, eta, executor, blur_w, others):
    """infer_video's particle keywords, checked before anything touches the engine -> dict K, scale, tau, reward_fn, y (the whole video's
    measurement repeated per particle, on the host, or None), or None for the plain run (particles=1 or reward_scale=0)."""
    from .gaussian_diffusion import check_steering
    if particles == 1 and reward_fn is None and y is None:
        return None
    K, lam, tau, _ = check_steering(reward_fn, y, particles, reward_scale, ess_threshold, sigma_y)
    y_v = None
    if y is not None:
        y_v = (check_linear_measurement(torch.as_tensor(y), batch.shape, *blur_w) if isinstance(blur_w, tuple)          # (a separable operator)
               else check_measurement(torch.as_tensor(y), batch.shape, sr_scale, gray) if blur_w is None
               else check_blur_measurement(torch.as_tensor(y), batch.shape)).cpu()
    for name, on in others:
        if on:
            raise NotImplementedError(f"{name} together with particles is not served")
    row = SAMPLERS[sampler if sampler in SAMPLERS else "ddim"]
    if row.noise is None or (row.eta and float(eta) == 0.0):
        raise NotImplementedError(f"sampler='{sampler}'{' at eta = 0' if row.noise is not None else ''} together with particles is not served: the "
                                  "step draws no noise, duplicated particles would never separate")
    if reward_fn is not None and executor == "graph":
        raise NotImplementedError("executor='graph' together with a reward_fn is not served: a Python callback between two steps cannot be "
                                  "captured in a graph (the built-in reward can: particle_measurement=, sigma_y=)")
    if K == 1 or lam == 0.0:
        return None
    return dict(K=K, scale=lam, tau=tau, reward_fn=reward_fn, y=None if y_v is None else y_v.repeat_interleave(K, dim=0))


def _chosen_for_all(local, chosen, K):
    """A window's result for all K particles of every video: the particle chosen at t == 0, repeated."""
    G = local.shape[0] // K
    picked = local.view(G, K, *local.shape[1:])[torch.arange(G, device=local.device), chosen.to(device=local.device, dtype=torch.int64)]
    return picked.repeat_interleave(K, dim=0)


def _eager_particle_window(model, diffusion, x0, model_kwargs, sampler, eta, cfg_scale, steer, y_w, sr_scale, gray, sigma_y, t_tensors, timesteps,
                           blur_w=None, lin=None):
    """One window of infer_video's eager executor inside steering_scope -> (the window's K samples per video, chosen (G,)).  A sampler
    whose noise is the engine's Philox stream draws it, and the uniforms of the built-in reward, where the window executor would."""
    local, carry, out = x0.clone(), None, None
    seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if SAMPLERS[sampler].noise == "philox" else None
    with diffusion.steering_scope(model, steer["reward_fn"], particles=steer["K"], scale=steer["scale"], ess_threshold=steer["tau"],
                                  measurement=y_w, sr_scale=sr_scale if y_w is not None else 1, gray=gray if y_w is not None else False,
                                  sigma_y=sigma_y, blur_kernel=None if y_w is None else blur_w,
                                  operator=None if y_w is None else lin):
        for timestep in timesteps:
            philox = None if seed is None else (seed, (diffusion.num_timesteps - 1 - timestep) * local.numel())
            out, carry = _sampler_step(diffusion, sampler, model, local, t_tensors[timestep], carry, cfg_scale, eta, philox,
                                       clip_denoised=True, model_kwargs=model_kwargs)
            local = out["sample"]
    return local, out["chosen"]


def video_known_region(batch, known_mask, known_video=None):
    """infer_video's known region over the whole video, on the host: known_mask (T, H, W) or (B, T, H, W), nonzero = known, ->
    (B, T, H, W) float32 of 0 / 1; known_video (B, T, C, H, W), default `batch`, -> float32.  ValueError on any other shape."""
    B, T, C, H, W = batch.shape
    m = torch.as_tensor(known_mask)
    if tuple(m.shape) == (T, H, W):
        m = m.unsqueeze(0).expand(B, T, H, W)
    if tuple(m.shape) != (B, T, H, W):
        raise ValueError(f"known_mask must be {(T, H, W)} or {(B, T, H, W)} for a batch of {tuple(batch.shape)}, got {tuple(m.shape)}")
    src = batch if known_video is None else torch.as_tensor(known_video)
    if tuple(src.shape) != tuple(batch.shape):
        raise ValueError(f"known_video must be {tuple(batch.shape)}, got {tuple(src.shape)}")
    return (m != 0).to(torch.float32).cpu().contiguous(), src.to(torch.float32).cpu().contiguous()


def gather_window(video, frame_indices):
    """video (B, T, ...) -> (B, Tw, ...): item i's frames frame_indices[i] ((B, Tw) int64), the way infer_video forms x0."""
    fi = torch.as_tensor(frame_indices).cpu()
    return torch.stack([video[i, fi[i]] for i in range(video.shape[0])], dim=0).clone()


def _eager_known_window(model, diffusion, x0, model_kwargs, k_src, k_mask, sampler, eta, cfg_scale, jump_length, n_resample, want_trace):
    """One window of infer_video's eager executor with a known region: the walk of repaint_schedule through the step entry points inside
    known_region_scope.  The merge's and the jumps' noise is what the window executor would draw: vd_randn at (seed, k B per + B per / 4)
    for op k's merge and (seed, k B per) for a jump, the seed drawn as WindowExecutor.begin draws it."""
    from .respace import repaint_schedule
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    B = x0.shape[0]
    n = x0.numel()
    local, prev, trace = x0.clone(), None, ([] if want_trace else None)
    z = torch.empty_like(local)
    for k, (op, ts) in enumerate(repaint_schedule(diffusion.num_timesteps - 1, jump_length, n_resample)):
        t = torch.tensor([ts] * B, device=x0.device)
        _lib.check(_lib.lib().vd_randn(_lib.ptr(z), n, seed, k * n + (n // 4 if op == "step" else 0), _lib.current_stream()))
        if op == "jump":
            local, prev = diffusion.q_jump(local, t, latent_mask=model_kwargs["latent_mask"], noise=z, model=model), None
            continue
        with diffusion.known_region_scope(model, k_src, k_mask, known_noise=z):
            philox = (seed, k * n) if SAMPLERS[sampler].noise == "philox" else None       # the head of op k's range
            out, prev = _sampler_step(diffusion, sampler, model, local, t, prev, cfg_scale, eta, philox, clip_denoised=True,
                                      model_kwargs=model_kwargs)
        local = out["sample"]
        if trace is not None:
            trace.append(local.clone())
    return local, trace


def to_uint8(recon):
    """video_sample.py:266-268: ((x+1)/2*255) truncated to uint8."""
    return ((recon - drange[0]) / (drange[1] - drange[0]) * 255).astype(np.uint8)


class SyntheticVideos:
    """Stand-in for `get_test_dataset` (image_datasets.py; no dataset ships offline): item i is a U[-1, 1] video drawn
    from a generator seeded by i alone, so a video does not depend on how the job was cut into batches or ranks."""

    def __init__(self, n, T, size, channels=3):
        self.n, self.shape = int(n), (int(T), channels, int(size), int(size))

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if not 0 <= i < self.n:
            raise IndexError(i)
        g = torch.Generator().manual_seed(1234 + int(i))
        return torch.rand(*self.shape, generator=g) * 2 - 1, {}


class ArrayVideos:
    """`--videos file.npy`: (N, T, 3, H, W); float arrays are taken as already in [-1, 1] (what the reference's datasets
    hand over), uint8 arrays -- the format this tool writes -- are mapped back by x / 255 * 2 - 1."""

    def __init__(self, path):
        a = np.load(path, mmap_mode="r")
        if a.ndim != 5:
            raise ValueError(f"{path}: expected (N, T, C, H, W), got {a.shape}")
        self.a = a

    def __len__(self):
        return self.a.shape[0]

    def __getitem__(self, i):
        v = np.array(self.a[i])
        if v.dtype == np.uint8:
            return torch.from_numpy(v).float() / 255 * (drange[1] - drange[0]) + drange[0], {}
        return torch.from_numpy(v).float(), {}


def open_videos(args):
    path = getattr(args, "videos", None)
    if path:
        return ArrayVideos(path)
    if not getattr(args, "synthetic", True):
        raise ValueError("no dataset ships with this tool: give --videos <file.npy> or --synthetic")
    return SyntheticVideos(args.num_videos, args.T if args.T is not None else 16, args.image_size)


def resolve_indices(args, dataset_len):
    """Which dataset items the job covers (video_sample.py:570-590): --indices as given; else --task_id -> one batch worth
    of consecutive items (NOT clipped to the dataset: `Subset` then fails on the first missing item, as there); else the
    first --subset_size items; else everything.  --task_id refuses --subset_size as the reference asserts."""
    indices, task_id = getattr(args, "indices", None), getattr(args, "task_id", None)
    subset_size = getattr(args, "subset_size", None)
    if indices is None and task_id is not None:
        assert subset_size is None
        logger.info(f"Only generating predictions for the batch #{task_id}.")
        return list(range(task_id * args.batch_size, (task_id + 1) * args.batch_size))
    if subset_size is not None:
        logger.info(f"Only generating predictions for the first {subset_size} videos of the dataset.")
        return list(range(subset_size))
    if indices is None:
        logger.info("Generating predictions for the whole dataset.")
        return list(range(dataset_len))
    return [int(i) for i in indices]


def sample_names(out_dir, dataset_ids, sample_idx, prefix="sample"):
    """samples/<prefix>_%04d-%d.npy for each dataset item of a batch (video_sample.py:209-230)."""
    return [out_dir / "samples" / f"{prefix}_{i:04d}-{sample_idx}.npy" for i in dataset_ids]


def q_sample_every_timestep(diffusion, model, batch):
    """video_sample.py:245-254: the clean videos noised to every timestep, (B, num_timesteps, T, C, H, W)."""
    out = [diffusion.q_sample(batch, t=torch.full((batch.shape[0],), ts, dtype=torch.long), model=model).cpu()
           for ts in range(diffusion.num_timesteps)]
    return torch.stack(out, dim=1).numpy()


def load_model(args, device, rank=0, world=1, create=None):
    """video_sample.py:547-567: checkpoint dict {'state_dict','config','step'} -> (model, diffusion).

    One process per GPU: ONLY rank 0 opens the checkpoint.  Its `config` (a small dict) goes to the other ranks with
    `broadcast_object_list`, every rank builds the same engine from it, rank 0 packs the state_dict into the engine's
    kernel-ready image and that ONE buffer travels by a single broadcast (RCCL over xGMI; `dist.share_weights`) -- in
    place of the reference's N checkpoint reads or its per-tensor `sync_params` (dist_util.py:139-143)."""
    from . import dist as vdist
    create = create or create_video_model_and_diffusion
    defaults = video_model_and_diffusion_defaults()
    holder = {}
    if rank == 0:
        if args.checkpoint_path:
            data = torch.load(args.checkpoint_path, map_location="cpu")
            cfg = dict(data["config"])
            cfg.setdefault("enforce_position_invariance", False)      # back-compat fills, video_sample.py:25-28,557-559
            cfg.setdefault("cond_emb_type", "channel")
            holder["sd"] = data["state_dict"]
        else:
            mf = args.max_frames if args.max_frames is not None else 10   # video_train.py:164's default
            cfg = dict(defaults, T=mf, max_frames=mf, image_size=args.image_size, num_channels=args.num_channels,
                       num_res_blocks=args.num_res_blocks, rp_alpha=mf, rp_beta=mf, rp_gamma=mf)
        cfg.update(use_ddim=bool(getattr(args, "use_ddim", False)), timestep_respacing=args.timestep_respacing)   # video_sample.py:551-554
        if getattr(args, "override_dataset", None) is not None:
            cfg["dataset"] = args.override_dataset                                                                # :555-556
    else:
        cfg = None
    cfg = vdist.broadcast_object(cfg, src=0)
    ns = argparse.Namespace(**cfg)
    model, diffusion = create(**args_to_dict(ns, defaults.keys()))
    model.config = {k: v for k, v in cfg.items() if isinstance(v, (int, float, str, bool, type(None), list, tuple, dict))}
    model.to(device)
    model.eval()

    def state_dict_fn():                                              # called on rank 0 only
        if "sd" not in holder:
            holder["sd"] = {k: torch.from_numpy(synth_param(k, s)) for k, s in model.param_specs()}
        return holder["sd"]

    if rank == 0 and (getattr(args, "dps_zeta", None) is not None or getattr(args, "loss_guidance", None)):
        model.enable_guidance()      # --dps_zeta / --loss_guidance run the backward-data pass: rank 0 packs the second image, share_weights broadcasts it
    vdist.share_weights(model, state_dict_fn, rank)
    return model, diffusion




def add_job_arguments(ap):
    """The options the two sampling CLIs share; names, defaults and meaning of scripts/video_sample.py:405-528 where the
    reference has the option (its dataset options are replaced by --videos / --synthetic)."""
    ap.add_argument("checkpoint_path", nargs="?", default="")
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--eval_dir", default=None,
                    help="results directory; default: derived from the checkpoint path and the sampling options "
                         "(test_util.get_model_results_path), 'results/synthetic' without a checkpoint")
    ap.add_argument("--out_dir", default=None, help="alias of --eval_dir (earlier rounds' flag)")
    ap.add_argument("--videos", default=None, help=".npy file of test videos (N, T, 3, H, W): float in [-1, 1] or uint8")
    ap.add_argument("--synthetic", type=str2bool, nargs="?", const=True, default=True,
                    help="without --videos: --num_videos synthetic U[-1, 1] videos, item i seeded by i")
    ap.add_argument("--num_videos", type=int, default=2, help="size of the synthetic dataset")
    ap.add_argument("--dataset_partition", default="test", choices=["train", "test", "variable_length"],
                    help="names the run directory as the reference does ('trainset_' prefix, 'variable_length/' subdirectory); the videos themselves "
                         "come from --videos / --synthetic")
    ap.add_argument("--override_dataset", default=None, help="'<name>_' prefix of the run directory and `dataset` of model_config.json (video_sample.py:555-556)")
    ap.add_argument("--use_gradient_method", action="store_true")
    ap.add_argument("--inference_mode", default="autoreg", choices=sorted(inference_util.inference_strategies))
    ap.add_argument("--max_frames", type=int, default=None,
                    help="frames (observed or latent) per window; defaults to what the model was trained with")
    ap.add_argument("--obs_length", type=int, default=36)
    ap.add_argument("--step_size", type=int, default=1)
    ap.add_argument("--indices", type=int, nargs="*", default=None, help="only these dataset items")
    ap.add_argument("--use_ddim", type=str2bool, nargs="?", const=True, default=False)
    ap.add_argument("--timestep_respacing", default="")
    ap.add_argument("--T", type=int, default=None, help="video length; default: the dataset's (16 for --synthetic)")
    ap.add_argument("--subset_size", type=int, default=None, help="only the first N dataset items")
    ap.add_argument("--num_samples", type=int, default=1, help="samples per test video")
    ap.add_argument("--sample_idx", type=int, default=None,
                    help="write exactly this sample index (--num_samples is then ignored)")
    ap.add_argument("--task_id", type=int, default=None,
                    help="only the batch-sized block of dataset items #task_id (composes with the rank shard)")
    ap.add_argument("--optimality", default=None,
                    choices=["linspace-t", "random-t", "linspace-t-force-nearby", "random-t-force-nearby"],
                    help="read <eval_dir>/optimal_schedule.pt (made by video_optimal_schedule with the same options)")
    ap.add_argument("--observed_frames", default="x_0", choices=["x_0", "x_t", "x_t_minus_1"])
    ap.add_argument("--save_all_timesteps", action="store_true")
    ap.add_argument("--image_size", type=int, default=64, help="without a checkpoint: the closed-form model's size")
    ap.add_argument("--num_channels", type=int, default=128)
    ap.add_argument("--num_res_blocks", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    return ap


def add_lpips_arguments(ap):
    """--lpips_weights of the three CLIs (next to their --adaptive_distance)."""
    ap.add_argument("--lpips_weights", default=None, metavar="PATH[,PATH]",
                    help="with --adaptive_distance lpips: an lpips.LPIPS(net='alex') state dict, or torchvision's AlexNet "
                         "checkpoint and lpips' weights/v0.1/alex.pth, comma-separated (lpips.py)")
    return ap


LPIPS_WEIGHTS_NEEDED = "needs --lpips_weights PATH[,PATH] (the LPIPS AlexNet weights do not ship)"


def parse_with_lpips(ap, argv):
    """parse_args + the refusal of --adaptive_distance lpips without weights (unless an embedder is registered already)."""
    args = ap.parse_args(argv)
    if (getattr(args, "adaptive_distance", "l2") == "lpips" and not getattr(args, "lpips_weights", None)
            and inference_util._lpips_embedder is None):
        ap.error(f"--adaptive_distance lpips {LPIPS_WEIGHTS_NEEDED}")
    return args


_lpips_loaded = {}


def load_lpips_for(args, device):
    """Adaptive mode with --adaptive_distance lpips and --lpips_weights: build the GPU embedder on this rank's device and
    register it -- once per process and (weights, device)."""
    paths = getattr(args, "lpips_weights", None)
    if not paths or getattr(args, "adaptive_distance", "l2") != "lpips" or "adaptive" not in args.inference_mode:
        return None
    key = (str(paths), str(device))
    if key not in _lpips_loaded:
        _lpips_loaded[key] = inference_util.load_lpips_weights(paths, device)
    else:
        inference_util.set_lpips_embedder(_lpips_loaded[key])
    return _lpips_loaded[key]


def build_parser():
    ap = add_job_arguments(argparse.ArgumentParser())
    ap.add_argument("--sampler", default="p_sample", choices=[s for s, row in SAMPLERS.items() if not row.up],
                    help="the step: p_sample (default), ddim (ddim_sample with --eta), dpmpp_2m (the second-order multistep solver), dpmpp_2m_sde "
                         "(its stochastic form) or unipc (dpmpp_2m's predictor plus a corrector on the same forward: third order; all three "
                         "meant for --timestep_respacing logsnrN, unipc for N of 20 or more); a non-default sampler is named in the run directory")
    ap.add_argument("--eta", type=float, default=0.0, help="with --sampler ddim: ddim_sample's eta")
    ap.add_argument("--cfg_scale", type=float, default=1.0,
                    help="classifier-free guidance weight on the observed frames: every step runs on out_u + w (out_c - out_u), out_u being the "
                         "network output with nothing observed; 1.0 (default) is plain sampling, any other value costs two forwards per step and "
                         "is named in the run directory")
    ap.add_argument("--cfg_rescale", type=float, default=0.0,
                    help="guidance rescale (with --cfg_scale other than 1): blend PHI in [0, 1] that brings the guided output's standard "
                         "deviation over each item's latent frames back towards the conditional output's; 0 (default) is off; named in the "
                         "run directory when set")
    ap.add_argument("--dynamic_threshold", type=float, default=None,
                    help="dynamic thresholding: the percentile P in (0, 1] of |x_0| over each item's latent frames that replaces the 1 of the "
                         "clamp of x_0 (never below 1); off by default; named in the run directory when set")
    ap.add_argument("--freeu", type=float, nargs=4, default=None, metavar=("B1", "B2", "S1", "S2"),
                    help="FreeU: in every forward the backbone half of the decoder's concat at the two lowest-resolution levels is scaled by "
                         "B1 / B2 and the lowest frequencies of the skip half by S1 / S2 (e.g. 1.4 1.2 0.6 0.8); all four finite and > 0; off "
                         "by default; named in the run directory when set")
    ap.add_argument("--freeu_adaptive", action="store_true",
                    help="with --freeu: the structure-aware backbone factor (b - 1) g + 1, g the frame's min-max normalised channel mean")
    ap.add_argument("--known_mask", default=None, metavar="MASK.npy",
                    help="pixel-mask inpainting: a (T, H, W) or (H, W) array, nonzero = known, one mask for all videos; the known pixels of every "
                         "generated frame are kept from the source (--known_videos, default: the test videos themselves)")
    ap.add_argument("--known_videos", default=None, metavar="K.npy",
                    help="with --known_mask: the source of the known pixels, (N, T, 3, H, W) indexed like --videos; float in [-1, 1] or uint8")
    ap.add_argument("--jump_length", type=int, default=1, help="with --known_mask and --n_resample > 1: steps per resampling jump")
    ap.add_argument("--n_resample", type=int, default=1, help="with --known_mask: times each level is walked (RePaint resampling); 1 = off")
    ap.add_argument("--measurement", default=None, metavar="Y.npy",
                    help="zero-shot restoration (DDNM): a degraded copy of the test videos, (N, T, Cy, H / S, W / S) float32 indexed like "
                         "--videos, Cy = 1 with --gray else 3 -- the mean over every S x S cell per channel (--gray: over the three "
                         "channels too); every generated frame reproduces it (needs --sr_scale and / or --gray)")
    ap.add_argument("--sr_scale", type=int, default=1, choices=[1, 2, 4, 8],
                    help="with --measurement: the cell size S of the measurement (super-resolution factor); 1 needs --gray")
    ap.add_argument("--gray", type=str2bool, nargs="?", const=True, default=False,
                    help="with --measurement: the measurement is greyscale, channel weights 1/3 each (colourisation)")
    ap.add_argument("--dps_zeta", type=float, default=None, metavar="Z",
                    help="with --measurement: diffusion posterior sampling (DPS) for a measurement that carries noise -- every step moves the "
                         "generated frames down the gradient of ||y - A x_0||_2 through the network with step size Z, in place of the exact "
                         "projection; eager executor, samplers p_sample and ddim; named in the run directory when set")
    ap.add_argument("--sr_kernel", default="box", choices=["box", "bicubic", "bilinear"],
                    help="with --measurement and --sr_scale S: how the measurement was down-sampled -- 'box' (default): the S x S cell mean; "
                         "'bicubic' / 'bilinear': torch's antialiased resampler, (N, T, 3, H / S, W / S), through the separable linear "
                         "operator (named in the run directory: '_lin<Mh>x<Mw>')")
    ap.add_argument("--operator_h", default=None, metavar="AH.npy",
                    help="with --measurement and --operator_w: the measurement is A_h x A_w^T of every channel plane, (N, T, 3, Mh, Mw); AH.npy "
                         "is the (Mh, H) matrix, Mh <= H <= 128; alone: the exact projection, or with --dps_zeta, or with --particles and "
                         "--measurement_sigma")
    ap.add_argument("--operator_w", default=None, metavar="AW.npy", help="with --operator_h: the (Mw, W) matrix")
    ap.add_argument("--operator_rtol", type=float, default=1e-3, metavar="R",
                    help="with --operator_h / --sr_kernel: the exact projection drops singular values at or below R times the largest")
    ap.add_argument("--blur_kernel", default=None, metavar="K.npy",
                    help="with --measurement: deblurring -- the measurement is a blurred, noisy copy of the test videos, (N, T, 3, H, W), and "
                         "K.npy the (k, k) kernel it was blurred with (k odd, at most 15; applied as torch's conv2d, zeros outside the frame); "
                         "needs --dps_zeta, or --particles with --measurement_sigma; named in the run directory ('_blur<k>')")
    ap.add_argument("--blur_sigma", type=float, default=None, metavar="S",
                    help="in place of --blur_kernel: a normalised Gaussian kernel of standard deviation S pixels")
    ap.add_argument("--blur_size", type=int, default=None, metavar="N",
                    help="with --blur_sigma: the kernel is N x N (odd, at most 15; default: the odd size that covers 3 S, at most 15)")
    ap.add_argument("--loss_guidance", default=None, metavar="MODULE:FUNCTION",
                    help="loss-guided sampling: FUNCTION(x0, t) of the importable MODULE (the current directory is searched too) is a loss on "
                         "each window's x_0 prediction (B, Tw, 3, H, W), differentiated by torch; every step moves the generated frames down "
                         "its gradient through the network; needs --loss_guidance_scale; eager executor, samplers p_sample and ddim; "
                         "named in the run directory when set")
    ap.add_argument("--loss_guidance_scale", type=float, default=None, metavar="S", help="with --loss_guidance: the step size, finite and not negative")
    ap.add_argument("--loss_guidance_normalize", action="store_true",
                    help="with --loss_guidance: the step is S / ||grad||_2 per video, the norm over the window's generated frames")
    ap.add_argument("--loss_guidance_cotangent", action="store_true",
                    help="with --loss_guidance: FUNCTION returns d loss / d x_0 itself (float32, x_0's shape, on the device), no autograd")
    ap.add_argument("--particles", type=int, default=1, metavar="K",
                    help="particle steering (gradient-free guidance by resampling): every video runs as K particles that are reweighted by a "
                         "reward on each step's x_0 prediction and resampled when their weights degenerate; needs --reward, or --measurement "
                         "with --measurement_sigma; every sampler that draws noise; named in the run directory ('_smc<K>') when above 1")
    ap.add_argument("--reward", default=None, metavar="MODULE:FUNCTION",
                    help="with --particles: FUNCTION(x0, t) of the importable MODULE (the current directory is searched too) returns one reward "
                         "per item of each window's x_0 prediction (B, Tw, 3, H, W); eager executor")
    ap.add_argument("--reward_scale", type=float, default=1.0, metavar="L", help="with --particles: the weight of the reward, finite and not negative")
    ap.add_argument("--measurement_sigma", type=float, default=None, metavar="SIGMA",
                    help="with --particles and --measurement: the measurement carries Gaussian noise of this standard deviation and is the "
                         "built-in reward -||y - A x_0||^2 / (2 SIGMA^2) of the particles, in place of the exact projection; both executors")
    ap.add_argument("--ess_threshold", type=float, default=0.5, metavar="TAU",
                    help="with --particles: resample when the effective sample size falls below TAU * K; in [0, 1]")
    ap.add_argument("--adaptive_distance", default="l2", choices=["l2", "lpips"],
                    help="adaptive-* modes: frame embedding for the farthest-point selection (lpips needs --lpips_weights)")
    add_lpips_arguments(ap)
    ap.add_argument("--executor", default="eager", choices=["graph", "eager"],
                    help="eager: one p_sample call per step (default); graph: one captured hipGraph per window shape (executor.py)")
    ap.add_argument("--suffix_skip", type=str2bool, nargs="?", const=True, default=False,
                    help="with --executor graph and observed_frames x_0 / x_t_minus_1: run the network behind its last attention layer "
                         "on the non-observed frames only")
    ap.add_argument("--prefix_cache", type=str2bool, nargs="?", const=True, default=False,
                    help="with --executor graph and observed_frames x_0: compute the observed frames' encoder prefix once per window")
    return ap


def check_particle_arguments(ap, args):
    """The rules between --particles and its companions, as argparse errors naming the options."""
    K, sigma = getattr(args, "particles", 1), getattr(args, "measurement_sigma", None)
    uses = [name for name, on in (("--dps_zeta", getattr(args, "dps_zeta", None) is not None), ("--measurement_sigma", sigma is not None)) if on]
    if len(uses) > 1:
        ap.error(f"{' and '.join(uses)} are two uses of --measurement (the gradient step of DPS, the reward of --particles; without either, the "
                 "exact projection): give one")
    if K < 1:
        ap.error("--particles K: at least 1")
    kern, bsig, bsize = (getattr(args, n, None) for n in ("blur_kernel", "blur_sigma", "blur_size"))
    if kern and bsig is not None:
        ap.error("--blur_kernel and --blur_sigma are two kernels: give one")
    if bsize is not None and bsig is None:
        ap.error("--blur_size needs --blur_sigma S")
    if bsig is not None and not bsig > 0.0:
        ap.error("--blur_sigma S: positive")
    if bsize is not None and not (1 <= bsize <= 15 and bsize % 2 == 1):
        ap.error("--blur_size N: odd, from 1 to 15")
    if kern or bsig is not None:
        if not getattr(args, "measurement", None):
            ap.error("--blur_kernel / --blur_sigma need --measurement Y.npy")
        if not uses:
            ap.error("--blur_kernel / --blur_sigma need --dps_zeta Z, or --particles K with --measurement_sigma SIGMA: the exact projection has "
                     "no pseudo-inverse for a blur")
        if int(getattr(args, "sr_scale", 1)) != 1 or getattr(args, "gray", False):
            ap.error("--blur_kernel / --blur_sigma together with --sr_scale or --gray are not served")
    oh, ow, srk = getattr(args, "operator_h", None), getattr(args, "operator_w", None), getattr(args, "sr_kernel", "box")
    if bool(oh) != bool(ow):
        ap.error("--operator_h and --operator_w come together")
    if oh or srk != "box":
        if not getattr(args, "measurement", None):
            ap.error("--operator_h / --operator_w / --sr_kernel need --measurement Y.npy")
        if kern or bsig is not None or getattr(args, "gray", False):
            ap.error("--operator_h / --operator_w / --sr_kernel together with --blur_kernel, --blur_sigma or --gray are not served")
        if oh and (srk != "box" or int(getattr(args, "sr_scale", 1)) != 1):
            ap.error("--operator_h / --operator_w and --sr_scale / --sr_kernel are two operators: give one")
        if srk != "box" and int(getattr(args, "sr_scale", 1)) == 1:
            ap.error("--sr_kernel bicubic / bilinear needs --sr_scale S with S above 1")
    if sigma is not None and not getattr(args, "measurement", None):
        ap.error("--measurement_sigma needs --measurement Y.npy")
    if sigma is not None and getattr(args, "reward", None):
        ap.error("--reward and --measurement_sigma are two rewards for --particles: give one")
    if K > 1 and sigma is None and not getattr(args, "reward", None):
        ap.error("--particles needs a reward: --reward MODULE:FUNCTION, or --measurement Y.npy with --measurement_sigma SIGMA")
    if K == 1 and (sigma is not None or getattr(args, "reward", None)):
        ap.error("--reward and --measurement_sigma need --particles K with K above 1")
    return args


def main(argv=None):
    ap = build_parser()
    return run(check_particle_arguments(ap, parse_with_lpips(ap, argv)))


def _known_options(args, batch):
    """--known_mask / --known_videos of the job -> infer_video's keywords for this batch ({} without a mask).  The batch's dataset
    items are args._batch_ids (run() sets it)."""
    path = getattr(args, "known_mask", None)
    if not path:
        return {}
    m = np.load(path)
    T = batch.shape[1]
    if m.ndim == 2:
        m = np.broadcast_to(m[None], (T, *m.shape))
    if m.ndim != 3:
        raise ValueError(f"{path}: --known_mask is (T, H, W) or (H, W), got {m.shape}")
    kw = dict(known_mask=torch.from_numpy(np.ascontiguousarray(m[:T] != 0)), jump_length=getattr(args, "jump_length", 1),
              n_resample=getattr(args, "n_resample", 1))
    if getattr(args, "known_videos", None):
        src = ArrayVideos(args.known_videos)
        kw["known_video"] = torch.stack([src[i][0] for i in args._batch_ids])[:, :T]
    return kw


def blur_kernel_of(args):
    """--blur_kernel K.npy / --blur_sigma S [--blur_size N] -> the (k, k) float32 taps, checked, or None without either."""
    path, sigma = getattr(args, "blur_kernel", None), getattr(args, "blur_sigma", None)
    if path:
        return check_blur_kernel(np.load(path))
    if sigma is None:
        return None
    size = getattr(args, "blur_size", None)
    if size is None:
        size = min(15, 2 * int(math.ceil(3.0 * float(sigma))) + 1)
    return gaussian_kernel(int(size), float(sigma))


def operator_of(args):
    """--operator_h AH.npy --operator_w AW.npy, or --sr_scale S --sr_kernel bicubic|bilinear on frames of --image_size -> (A_h, A_w),
    checked float32 host tensors, or None without either (the default --sr_kernel box is the cell-mean path)."""
    oh, ow, srk = getattr(args, "operator_h", None), getattr(args, "operator_w", None), getattr(args, "sr_kernel", "box")
    if oh and ow:
        return check_separable_operator(np.load(oh), np.load(ow))
    if srk in ("bicubic", "bilinear"):
        n, S = int(args.image_size), int(getattr(args, "sr_scale", 1))
        if S < 2 or n % S:
            raise ValueError(f"--sr_kernel {srk}: --sr_scale S above 1 that divides --image_size {n}")
        A = resize_matrix(n, n // S, srk)
        return check_separable_operator(A, A)
    return None


def _measurement_options(args, batch):
    """--measurement / --sr_scale / --gray of the job -> infer_video's keywords for this batch ({} without a measurement).  The
    batch's dataset items are args._batch_ids (run() sets it)."""
    path = getattr(args, "measurement", None)
    zeta = getattr(args, "dps_zeta", None)
    if not path:
        if zeta is not None:
            raise ValueError("--dps_zeta needs --measurement")
        return {}
    y = np.load(path, mmap_mode="r")
    if y.ndim != 5:
        raise ValueError(f"{path}: --measurement is (N, T, Cy, H / S, W / S), got {y.shape}")
    T = batch.shape[1]
    rows = np.stack([np.asarray(y[i][:T], dtype=np.float32) for i in args._batch_ids])
    lin = operator_of(args)
    if lin is not None:                                               # a separable operator: any of the three paths
        kw = dict(operator=lin, operator_rtol=float(getattr(args, "operator_rtol", 1e-3)))
        if getattr(args, "measurement_sigma", None) is not None:
            return dict(particle_measurement=torch.from_numpy(rows), sigma_y=float(args.measurement_sigma), **kw)
        return dict(measurement=torch.from_numpy(rows), **kw, **({} if zeta is None else dict(dps_zeta=float(zeta))))
    blur_w = blur_kernel_of(args)
    if blur_w is not None:                                            # a blurred copy: the video's shape, and one of the two noisy paths
        if getattr(args, "measurement_sigma", None) is not None:
            return dict(particle_measurement=torch.from_numpy(rows), sigma_y=float(args.measurement_sigma), blur_kernel=blur_w)
        return dict(measurement=torch.from_numpy(rows), blur_kernel=blur_w, **({} if zeta is None else dict(dps_zeta=float(zeta))))
    if getattr(args, "measurement_sigma", None) is not None:          # the reward of --particles, not the projection
        return dict(particle_measurement=torch.from_numpy(rows), sr_scale=int(getattr(args, "sr_scale", 1)), gray=bool(getattr(args, "gray", False)),
                    sigma_y=float(args.measurement_sigma))
    return dict(measurement=torch.from_numpy(rows), sr_scale=int(getattr(args, "sr_scale", 1)), gray=bool(getattr(args, "gray", False)),
                **({} if zeta is None else dict(dps_zeta=float(zeta))))


def _particle_options(args):
    """--particles and its companions -> infer_video's keywords ({} at the default K = 1); the measurement's share comes from
    _measurement_options."""
    K = int(getattr(args, "particles", 1))
    if K == 1:
        return {}
    spec = getattr(args, "reward", None)
    return dict(particles=K, reward_fn=import_function(spec, "--reward") if spec else None, reward_scale=float(getattr(args, "reward_scale", 1.0)),
                ess_threshold=float(getattr(args, "ess_threshold", 0.5)))


def import_function(spec, option="--loss_guidance"):
    """'MODULE:FUNCTION' -> the callable FUNCTION of the module importlib finds under the name MODULE; the current directory is searched
    like the rest of sys.path (a script run as `python -m` does not have it there).  ValueError for a spec of another form, a module that
    cannot be imported, or a name that is missing or not callable."""
    import importlib
    import sys
    mod, sep, fn = str(spec).partition(":")
    if not (sep and mod and fn):
        raise ValueError(f"{option} {spec!r}: expected MODULE:FUNCTION")
    if os.getcwd() not in sys.path and "" not in sys.path:
        sys.path.append(os.getcwd())
    try:
        module = importlib.import_module(mod)
    except ImportError as e:
        raise ValueError(f"{option} {spec!r}: cannot import module {mod!r}: {e}") from e
    f = getattr(module, fn, None)
    if not callable(f):
        raise ValueError(f"{option} {spec!r}: module {mod!r} has no callable {fn!r}")
    return f


def _loss_guidance_options(args):
    """--loss_guidance MODULE:FUNCTION and its companions -> infer_video's keywords ({} without the option)."""
    spec = getattr(args, "loss_guidance", None)
    scale = getattr(args, "loss_guidance_scale", None)
    if not spec:
        for name in ("loss_guidance_scale", "loss_guidance_normalize", "loss_guidance_cotangent"):
            if getattr(args, name, None):
                raise ValueError(f"--{name} needs --loss_guidance MODULE:FUNCTION")
        return {}
    if scale is None:
        raise ValueError("--loss_guidance needs --loss_guidance_scale S")
    f = import_function(spec)
    cot = bool(getattr(args, "loss_guidance_cotangent", False))
    return dict(loss_fn=None if cot else f, cotangent_fn=f if cot else None, loss_scale=float(scale),
                loss_normalize=bool(getattr(args, "loss_guidance_normalize", False)))


def _freeu_options(args):
    """--freeu B1 B2 S1 S2 [--freeu_adaptive] -> infer_video's keywords ({} without the option)."""
    fu = getattr(args, "freeu", None)
    if fu is None:
        if getattr(args, "freeu_adaptive", False):
            raise ValueError("--freeu_adaptive needs --freeu B1 B2 S1 S2")
        return {}
    return dict(freeu=check_freeu(*fu), freeu_adaptive=bool(getattr(args, "freeu_adaptive", False)))


def _default_infer(args, model, diffusion, batch, optimal_schedule_path):
    return infer_video(args.inference_mode, model, diffusion, batch, args.max_frames, args.obs_length, args.step_size,
                       optimal_schedule_path, use_gradient_method=getattr(args, "use_gradient_method", False),
                       observed_frames=args.observed_frames, sampler=getattr(args, "sampler", "p_sample"), eta=getattr(args, "eta", 0.0),
                       executor=getattr(args, "executor", "eager"),
                       adaptive_distance=getattr(args, "adaptive_distance", "l2"),
                       prefix_cache=getattr(args, "prefix_cache", False), suffix_skip=getattr(args, "suffix_skip", False),
                       save_all_timesteps=getattr(args, "save_all_timesteps", False), cfg_scale=getattr(args, "cfg_scale", 1.0),
                       cfg_rescale=getattr(args, "cfg_rescale", 0.0), dynamic_threshold=getattr(args, "dynamic_threshold", None),
                       **_known_options(args, batch), **_measurement_options(args, batch), **_loss_guidance_options(args),
                       **_particle_options(args), **_freeu_options(args))


def run_postfix(args):
    """What the options add to the run directory's name: a sampler other than the default, then a cfg_scale other than 1
    ('_cfg2', '_cfg1.5', '_cfg-0.5'), a cfg_rescale other than 0 ('_resc0.7'), a dynamic_threshold ('_dt0.995'), a --known_mask and a
    --measurement ('_sr4', '_gray', '_sr4gray', with --dps_zeta '_sr4_dps0.5'; under --blur_kernel / --blur_sigma '_blur9' in their place, under --operator_h / --sr_kernel bicubic '_lin8x8'), a --loss_guidance ('_lg0.5': its scale) and --particles
    above 1 ('_smc8') and a --freeu ('_freeu1.4-1.2-0.6-0.8', with --freeu_adaptive '_freeu1.4-1.2-0.6-0.8a') -- samples of different samplers or guidance settings never share a directory, and a run
    without the options keeps its name."""
    sampler = getattr(args, "sampler", "p_sample")
    w = float(getattr(args, "cfg_scale", 1.0))
    phi = float(getattr(args, "cfg_rescale", 0.0) or 0.0)
    p = getattr(args, "dynamic_threshold", None)
    known = ""
    if getattr(args, "known_mask", None):         # '_known', '_known_j2r3' with resampling
        r = int(getattr(args, "n_resample", 1))
        known = "_known" + ("" if r == 1 else f"_j{int(getattr(args, 'jump_length', 1))}r{r}")
    meas = ""
    if getattr(args, "measurement", None):        # '_sr4', '_gray', '_sr4gray'; under a blur '_blur9'
        S = int(getattr(args, "sr_scale", 1))
        blur_w, lin = blur_kernel_of(args), operator_of(args)
        meas = f"_lin{int(lin[0].shape[0])}x{int(lin[1].shape[0])}" if lin is not None else f"_blur{int(blur_w.shape[0])}" if blur_w is not None else "_" + ("" if S == 1 else f"sr{S}") + ("gray" if getattr(args, "gray", False) else "")
        if getattr(args, "dps_zeta", None) is not None:
            meas += f"_dps{float(args.dps_zeta):g}"
    lg = ""
    if getattr(args, "loss_guidance", None):      # '_lg0.5' (the function is not named: a run directory is one function's)
        lg = "_lg" + ("None" if getattr(args, "loss_guidance_scale", None) is None else f"{float(args.loss_guidance_scale):g}")
    smc = f"_smc{int(args.particles)}" if int(getattr(args, "particles", 1) or 1) > 1 else ""      # '_smc8': the particles of a video
    fu = getattr(args, "freeu", None)
    freeu = "" if fu is None else "_freeu" + "-".join(f"{float(v):g}" for v in fu) + ("a" if getattr(args, "freeu_adaptive", False) else "")
    return ("" if sampler == "p_sample" else f"_{sampler}") + ("" if w == 1.0 else f"_cfg{w:g}") + \
        ("" if phi == 0.0 else f"_resc{phi:g}") + ("" if p is None else f"_dt{float(p):g}") + known + meas + lg + smc + freeu


def run(args, create=None, device=None, infer=None):
    """The body of the reference's script (video_sample.py:192-298, 530-640): join the job, load + share the weights,
    decide which dataset items this job covers, and for every batch this rank owns and every sample index: form the
    output names, look at the disk, and run `infer_video` only if a file is missing (`todo`, :231-239) -- a resumed
    job repeats no denoise step.  Files: samples/sample_%04d-%d.npy (+ all_timestep_sample_ / q_sample_ / error_ with
    --save_all_timesteps) under results/<...>/<run id>/ (test_util.py:65-132).  `create` / `device` let the CPU tests
    drive the sharding + broadcast path with a stand-in engine; `infer(args, model, diffusion, batch, schedule_path)`
    is the sampler (video_sample_full passes its own)."""
    import json
    from pathlib import Path
    from . import test_util
    logging.basicConfig(level=logging.INFO)
    from . import dist as vdist
    # the process group is bound to the device this job computes on (an explicit `device` wins over LOCAL_RANK)
    rank, local_rank, world = vdist.init(device_index=device.index if device is not None and device.type == "cuda" else None)
    if device is None:
        device = torch.device("cuda", local_rank)
        torch.cuda.set_device(device)
    torch.manual_seed(args.seed + rank)
    load_lpips_for(args, device)
    infer = infer or _default_infer
    # the run identifier is formed from the options AS GIVEN, before --max_frames / --T take their defaults from the model and
    # the dataset (video_sample.py:530-533 precedes :568-570,612-615: an unset one reads 'None' in the directory name)
    # (a sampler other than the default and a cfg_scale other than 1 are part of the name: run_postfix)
    run_id = test_util.get_eval_run_identifier(args, postfix=run_postfix(args))
    model, diffusion = load_model(args, device, rank, world, create=create)
    if args.max_frames is None:                                            # video_sample.py:568-570
        args.max_frames = model.config.get("max_frames") or model.config["T"]
    dataset = open_videos(args)
    if args.T is None:                                                     # :612-615
        args.T = int(dataset[0][0].shape[0])
    # results/<checkpoint subpath>/<stem>[_<step>][_ddim][_respace<X>]/<mode>_<max_frames>_<step_size>_<T>_<obs_length>/
    # (test_util.py:65-132 of the reference, video_sample.py:530-533,600-611): what video_eval.py reads
    # -- derived on rank 0 (a '*latest' checkpoint is opened once more there for its step) and sent to the others
    out_dir = None
    if rank == 0:
        if args.eval_dir is None:
            alias = getattr(args, "out_dir", None)
            args.eval_dir = alias if alias is not None else (None if args.checkpoint_path else "results/synthetic")
        out_dir = test_util.get_model_results_path(args) / run_id
        if getattr(args, "dataset_partition", None) == "variable_length":                                       # video_sample.py:603-604
            out_dir = out_dir / "variable_length"
        os.makedirs(out_dir / "samples", exist_ok=True)
        json_path = out_dir / "model_config.json"                         # video_sample.py:620-626
        if not json_path.exists():
            with test_util.Protect(json_path):
                with open(json_path, "w") as f:
                    json.dump(model.config, f, indent=4)
    out_dir = Path(vdist.broadcast_object(out_dir, src=0))
    optimal_schedule_path = None if getattr(args, "optimality", None) is None else out_dir / "optimal_schedule.pt"   # :199-200
    args.indices = resolve_indices(args, len(dataset))
    batches = [args.indices[k:k + args.batch_size] for k in range(0, len(args.indices), args.batch_size)]   # DataLoader(Subset(..)), no shuffle
    one_idx = getattr(args, "sample_idx", None)
    sample_ids = range(getattr(args, "num_samples", 1)) if one_idx is None else [one_idx]
    every = getattr(args, "save_all_timesteps", False)
    for task in vdist.task_ids(len(batches), rank, world):                  # one process per GPU: rank r owns batches r, r+R, ...
        ids = batches[task]
        batch = None
        for sample_idx in sample_ids:
            names = sample_names(out_dir, ids, sample_idx)
            todo = [not p.exists() for p in names]
            if not any(todo):
                logger.info(f"Nothing to do for the videos {ids[0]} - {ids[-1]}, sample #{sample_idx}.")
                continue
            if batch is None:
                batch = torch.stack([dataset[i][0] for i in ids])[:, :args.T].to(device)
            q_all = q_sample_every_timestep(diffusion, model, batch) if every else None
            args._batch_ids = ids
            recon, recon_all = infer(args, model, diffusion, batch, optimal_schedule_path)
            outputs = [(names, to_uint8(recon))]
            if every:
                outputs += [(sample_names(out_dir, ids, sample_idx, "q_sample"), q_all),
                            (sample_names(out_dir, ids, sample_idx, "error"), q_all - recon_all),
                            (sample_names(out_dir, ids, sample_idx, "all_timestep_sample"), to_uint8(recon_all))]
            for paths, arrays in outputs:
                for i, path in enumerate(paths):
                    if todo[i]:
                        np.save(path, arrays[i])
                        logger.info(f"*** Saved {path} ***")
                    else:
                        logger.info(f"Skipped {path}")
    vdist.barrier()
    return out_dir


if __name__ == "__main__":
    main()
