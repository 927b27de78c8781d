"""Window executor: the step loop of scripts/video_sample.py:149-168 as graph replays.

    for timestep in reversed(range(diffusion.num_timesteps)):
        local = diffusion.p_sample(model, local, t, clip_denoised=True, model_kwargs=kw)['sample']

The reference (and the eager path here) drives that loop from the host: ~330 kernel launches per step.  The executor
keeps the loop state on the device (respaced index, Philox counter), holds ONE captured hipGraph per window signature
and replays it `num_timesteps` times (C ABI: vd_window_begin / vd_window_run, include/vd_amd.h; BASELINE configs[4]).
The window's tensors live in buffers owned by this object, one set per (B, T), so every window of that shape reuses the
same graph: CARLA's 47 windows need two graphs (Tw = 20 and Tw = 14).

Noise: the engine's counter-based generator (Philox4x32-10 + Box-Muller inside the posterior kernel) with a seed drawn
from torch's global generator, so `torch.manual_seed` still makes a run reproducible; the draws are N(0, 1) like the
reference's `th.randn_like`, not the same stream.  `observed_frames` in {'x_0', 'x_t', 'x_t_minus_1'}.  'x_t_minus_1' has two
callers in the reference and they differ: `p_sample_loop` re-noises the clean observed frames to t - 1 before each step
(gaussian_diffusion.py:565-568) -- `renoise=True`, the default here: q_sample inside the graph from the same Philox stream --
while scripts/video_sample.py:149-166 calls `p_sample` directly with `x_t_minus_1 = x0`, a clean placeholder that is read as it
is at every step -- `renoise=False`, what `infer_video` passes, so that its graph and eager executors sample the same
conditional distribution.

Pixel-mask inpainting (this project's extension, RePaint): `begin(..., known_src=, known_mask=)` captures a step that ends in the merge pass
on the window tensor, `jump(n)` walks the armed window n forward diffusion steps back up (plain launches), and `run_repaint(j, r)` is the
walk of `respace.repaint_schedule` over both; all noise stays on the window's Philox stream (include/vd_amd.h: vd_set_known_region).
Zero-shot restoration (DDNM, this project's extension too): `begin(..., measurement=, sr_scale=, gray=)` captures a step whose x_0
prediction is projected onto the measurement in front of the sampler pass (include/vd_amd.h: vd_set_measurement).
Separable linear measurements (this project's extension): `begin(..., measurement=, operator=(A_h, A_w))` captures the two projection passes
of csrc/linop.hip in the same place, `begin(..., particle_measurement=, operator=, sigma_y=)` the built-in reward on that operator; the
matrices live in the engine at fixed addresses (include/vd_amd.h: vd_set_linear_operator).
Particle steering (this project's extension): `begin(..., particles=K, particle_measurement=, sigma_y=)` captures a step that ends in the
residual pass, the weights and the gather of the built-in reward; the weights live in the engine, the uniforms on the window's Philox
stream, and `particle_state()` reads them (include/vd_amd.h: vd_set_particles).
"""
import math

import torch as th

from . import _lib
from .gaussian_diffusion import (SAMPLERS, _check_operator, _engine_linear, _engine_measurement, _engine_particles, _engine_region, _refuse,
                                 _scope, check_blur_kernel, check_blur_measurement, check_known_region, check_linear_measurement,
                                 check_measurement, check_separable_operator, check_steering, measurement_shape, separable_pinv)

_OBS_MODES = {"x_0": 0, "x_t": 1, "x_t_minus_1": 2}


def _sampler_id(sampler):
    """vd_window_begin's sampler: 'ddim_reverse' is 2, 'dpmpp_2m' 3, 'dpmpp_2m_sde' 4, 'unipc' 5, 'p_sample' 0 and every other string ddim_sample, 1."""
    return SAMPLERS.get(sampler, SAMPLERS["ddim"]).id


class WindowExecutor:
    def __init__(self, model, diffusion, prefix_cache=False, suffix_skip=False):
        """prefix_cache: compute the observed frames' activations before the first attention layer once per window instead
        of once per step ('x_0' mode, cond_emb_type='channel'; include/vd_amd.h: vd_set_window_prefix_cache).
        suffix_skip: run everything behind the last attention layer without the purely observed frames ('x_0' and
        'x_t_minus_1'; vd_set_window_suffix_skip): the other frames' samples are those of the full step, the observed frames'
        entries of the returned window are meaningless (infer_video keeps only the latent frames, video_sample.py:170-186)."""
        self.model = diffusion._bind(model)
        self.diffusion = diffusion
        self.prefix_cache = bool(prefix_cache)
        self.suffix_skip = bool(suffix_skip)
        self.stream = th.cuda.Stream(device=self.model.device)        # a capture needs a non-default stream
        self._bufs = {}
        self.x = None

    def _buffers(self, B, T):
        key = (B, T)
        if key not in self._bufs:
            dev, S = self.model.device, self.model.image_size
            f = lambda *s: th.zeros(*s, dtype=th.float32, device=dev)  # noqa: E731
            self._bufs[key] = dict(x=f(B, T, 3, S, S), obs_src=f(B, T, 3, S, S), obs_mask=f(B * T), latent_mask=f(B * T),
                                   kinda_marg_mask=f(B * T), frame_indices=th.zeros(B, T, dtype=th.int64, device=dev))
        return self._bufs[key]

    def _known_buffers(self, B, T):
        """The window's known region, one pair per (B, T) like the window tensors: stable addresses, so one graph per shape."""
        bufs = self._buffers(B, T)
        if "known_src" not in bufs:
            S = self.model.image_size
            bufs["known_src"] = th.zeros(B, T, 3, S, S, dtype=th.float32, device=self.model.device)
            bufs["known_mask"] = th.zeros(B, T, S, S, dtype=th.float32, device=self.model.device)
        return bufs["known_src"], bufs["known_mask"]

    def _measurement_buffer(self, B, T, scale, gray, blur=False):
        """The window's measurement, one buffer per (B, T, scale, gray) and one for a blurred one (the video's shape): a stable address, so
        one graph per shape and operator."""
        bufs, key = self._buffers(B, T), "measurement_blur" if blur else f"measurement_s{scale}_g{int(gray)}"
        if key not in bufs:
            S = self.model.image_size
            shape = (B, T, 3, S, S) if blur else measurement_shape((B, T, 3, S, S), scale, gray)
            bufs[key] = th.zeros(*shape, dtype=th.float32, device=self.model.device)
        return bufs[key]

    def _linear_buffer(self, B, T, Mh, Mw, use):
        """The window's measurement under a separable operator, one buffer per (B, T, Mh, Mw) and use: a stable address."""
        bufs, key = self._buffers(B, T), f"linear_{use}_{Mh}x{Mw}"
        if key not in bufs:
            bufs[key] = th.zeros(B, T, 3, Mh, Mw, dtype=th.float32, device=self.model.device)
        return bufs[key]

    def begin(self, x_init, model_kwargs, t_start=None, seed=None, sampler="p_sample", eta=0.0, clip_denoised=True, renoise=True,
              known_src=None, known_mask=None, measurement=None, sr_scale=1, gray=False, particles=1, reward_fn=None, reward_scale=1.0,
              ess_threshold=0.5, particle_measurement=None, particle_sr_scale=1, particle_gray=False, sigma_y=None, blur_kernel=None,
              operator=None, operator_rtol=1e-3, cfg_scale=1.0):
        """Arm a window: copy its tensors into the executor's buffers, set the device counters, capture if new.
        renoise ('x_t_minus_1' only): True = p_sample_loop's form, the clean model_kwargs['x0'] frames re-noised to t - 1 inside
        every step; False = model_kwargs['x_t_minus_1'] read as it is at every step (a direct p_sample caller).
        sampler: 'p_sample', 'ddim' or 'ddim_reverse' (ddim_reverse_sample, gaussian_diffusion.py:636-668: the window walks from
        t_start, default 0, UP to the last index, draws no noise -- seed and eta are not read -- and takes 'x_t_minus_1' with
        renoise=False only) or 'dpmpp_2m' (dpmpp_2m_sample, this project's extension: walks down like 'ddim', the previous step's
        x_0 prediction lives in an engine-owned buffer, the window's first step is first-order whatever t_start is, no noise --
        seed and eta are not read -- and 'x_t_minus_1' with renoise=False only) or 'dpmpp_2m_sde' (dpmpp_2m_sde_sample, this project's
        extension: the history of 'dpmpp_2m' and the Philox noise of 'ddim' both live in the graph; eta is not read; every
        observed_frames mode 'ddim' takes, renoise=True included) or 'unipc' (unipc_sample, this project's extension: walks down like
        'dpmpp_2m', its three state tensors live in engine-owned buffers, the window's first step runs no corrector and a first-order
        predictor whatever t_start is, no noise -- seed and eta are not read -- 'x_t_minus_1' with renoise=False only, and a known
        region is refused by name).
        cfg_scale (this project's extension; gaussian_diffusion.py: p_sample): the captured step holds both forwards, the combine pass
        and the sampler pass; the weight is part of the graph's signature, so windows under different weights replay different graphs.
        The noise of a window does not depend on it.  Not served together with prefix_cache or suffix_skip: in the unconditional
        forward the observed frames are padding frames whose content is whatever the window tensor holds.
        Guidance rescale and dynamic thresholding are not parameters: a begin() inside `diffusion.guidance_scope(...)` captures (or finds)
        the graph of the scope's values -- they are part of the signature like the weight -- and run() may be called outside the scope.
        The engine refuses either of them together with prefix_cache or suffix_skip.
        FreeU is not a parameter either: a begin() inside `diffusion.freeu_scope(...)` captures (or finds) the graph whose forwards hold
        the scope's passes -- the four constants and the form are part of the signature, and going back to off finds the plain graph
        again.  Refused together with prefix_cache or suffix_skip.
        known_src, known_mask (this project's extension; gaussian_diffusion.py: known_region_scope): pixel-mask inpainting -- both are
        copied into buffers of this object, the captured step ends in the merge pass, and the merge's noise comes from the window's own
        Philox stream (the step's range at + B*per/4; every sampler's step then advances the counter by B*per).  Without them, a begin()
        inside `diffusion.known_region_scope(...)` takes the scope's region.  Not served with 'ddim_reverse', prefix_cache or suffix_skip.
        measurement, sr_scale, gray (this project's extension; gaussian_diffusion.py: measurement_scope): zero-shot restoration -- y =
        measure(window, sr_scale, gray) is checked (check_measurement) and copied into a buffer of this object, one per (B, T, sr_scale,
        gray); the captured step projects its x_0 prediction onto it, and y's address, the scale and the flag are part of the graph's
        signature.  Without it, a begin() inside `diffusion.measurement_scope(...)` takes the scope's measurement.  The engine refuses it
        by name with 'ddim_reverse', prefix_cache, suffix_skip and a known region.
        particles, reward_scale, ess_threshold, particle_measurement, particle_sr_scale, particle_gray, sigma_y (this project's extension;
        gaussian_diffusion.py: steering_scope): particle steering with the BUILT-IN reward of a noisy measurement -- the batch is groups
        of `particles` consecutive items, y = particle_measurement is checked and copied into a buffer of this object, and the captured
        step ends in the residual pass, the weights and the gather of the window tensor and the x_0 prediction; K, the scale, the
        threshold, y's address, the operator and sigma_y are part of the graph's signature.  The weights are reset by every begin();
        the uniforms come from the window's Philox stream.  particle_state() reads the state behind any run().  Without them, a begin()
        inside `diffusion.steering_scope(..., measurement=)` takes the scope's setting.  A reward_fn -- the keyword, or the scope's -- is
        refused by name: a Python callback cannot be captured.  Refused by name too: a sampler that draws no noise ('ddim' at eta = 0,
        'dpmpp_2m', 'unipc', 'ddim_reverse'), a known region, a measurement, prefix_cache, suffix_skip, B no multiple of particles.
        blur_kernel (this project's extension; gaussian_diffusion.py: deblur_scope): with particle_measurement, the built-in reward's
        operator is this (k, k) blur in place of the cell mean -- particle_measurement then has the window's own shape, and
        particle_sr_scale and particle_gray stay at their defaults.  The taps are copied into the engine's own buffer, whose address never
        changes: the graph's signature carries k alone, and a begin() with other taps of the same size replays the same graph on the new
        taps.  They stay there until the next kernel is installed (another begin() with a blur, a deblur_scope, a steering_scope with a
        blur), so run() the window before that.
        operator, operator_rtol (this project's extension; gaussian_diffusion.py: linear_measurement_scope): operator=(A_h, A_w) makes the
        measurement -- `measurement` or `particle_measurement`, one of them -- one under that separable operator, (B, T, 3, Mh, Mw), and
        sr_scale, gray and blur_kernel stay at their defaults.  With `measurement` the captured step holds the two projection passes, with
        the truncated pseudo-inverses separable_pinv(A, operator_rtol) as the back-projection; with `particle_measurement` the built-in
        reward runs on the operator.  The matrices are copied into the engine's own buffers, whose addresses never change: the graph's
        signature carries y's address and (Mh, Mw), and a begin() with other matrices of the same shape replays the same graph on them.
        Without the keyword, a begin() inside `diffusion.linear_measurement_scope(...)` takes the scope's measurement, matrices and
        back-projection.  A begin() inside `diffusion.linear_dps_scope(...)` is refused by name.
        A begin() inside `diffusion.dps_scope(...)` is refused by name: a DPS step runs a backward pass and is eager only; so is one
        inside `diffusion.loss_guidance_scope(...)`, whose step runs the caller's Python between two launches."""
        cfg_scale = float(cfg_scale)
        if not math.isfinite(cfg_scale):
            raise ValueError(f"cfg_scale={cfg_scale!r}: the guidance weight must be finite")
        if cfg_scale != 1.0 and self.prefix_cache:
            raise NotImplementedError("prefix_cache together with cfg_scale != 1")
        if cfg_scale != 1.0 and self.suffix_skip:
            raise NotImplementedError("suffix_skip together with cfg_scale != 1")
        if (known_src is None) != (known_mask is None):
            raise ValueError("known_src and known_mask are given together")
        _refuse(self.model, "dps", "WindowExecutor.begin")               # before anything touches the engine
        _refuse(self.model, "deblur", "WindowExecutor.begin")
        _refuse(self.model, "linear_dps", "WindowExecutor.begin")
        lin, lm_scope = None, _scope(self.model, "linear_measurement")
        if operator is not None:
            if (measurement is None) == (particle_measurement is None):
                raise ValueError("WindowExecutor.begin: operator is the operator of measurement= or of particle_measurement=: give one of them")
            if blur_kernel is not None or not (sr_scale == 1 and gray is False and particle_sr_scale == 1 and particle_gray is False):
                raise ValueError("WindowExecutor.begin: operator together with blur_kernel, sr_scale or gray is not served: leave them at their defaults")
            if not isinstance(operator, (tuple, list)) or len(operator) != 2:
                raise ValueError("WindowExecutor.begin: operator is a pair (A_h, A_w)")
            a_h, a_w = check_separable_operator(*operator)
            if measurement is not None:
                lin = dict(y=check_linear_measurement(measurement, x_init.shape, a_h, a_w), A_h=a_h, A_w=a_w,
                           P_h=separable_pinv(a_h, operator_rtol)[0], P_w=separable_pinv(a_w, operator_rtol)[0])
                measurement = None
            else:
                operator = (a_h, a_w)
        elif lm_scope is not None:
            lin = dict(lm_scope, y=check_linear_measurement(lm_scope["y"], x_init.shape, lm_scope["A_h"], lm_scope["A_w"]))
        if lin is not None and (measurement is not None or _scope(self.model, "measurement") is not None):
            raise _lib.VdError("a linear measurement together with a measurement is not served")
        _refuse(self.model, "loss_guidance", "WindowExecutor.begin")     # (a Python callback between two launches cannot be captured)
        steer = self._steering(x_init, sampler, eta, particles, reward_fn, reward_scale, ess_threshold, particle_measurement, particle_sr_scale,
                               particle_gray, sigma_y, blur_kernel, known_src is not None or _scope(self.model, "known_region") is not None,
                               measurement is not None or _scope(self.model, "measurement") is not None or lin is not None,
                               operator if lin is None else None)
        scope = _scope(self.model, "known_region")
        if known_src is not None:
            known_src, known_mask = check_known_region(known_src, known_mask)
        elif scope is not None:
            known_src, known_mask = scope["src"], scope["mask"]
        if known_src is not None:
            if tuple(known_src.shape) != tuple(x_init.shape):
                raise ValueError(f"known_src {tuple(known_src.shape)} against a window of {tuple(x_init.shape)}")
            for name, on in (("prefix_cache", self.prefix_cache), ("suffix_skip", self.suffix_skip), ("sampler='ddim_reverse'", sampler == "ddim_reverse"),
                             ("sampler='unipc'", sampler == "unipc")):
                if on:
                    raise NotImplementedError(f"{name} together with a known region")
        m_scope = _scope(self.model, "measurement")
        if measurement is not None:
            meas = dict(y=check_measurement(measurement, x_init.shape, sr_scale, gray), scale=int(sr_scale), gray=bool(gray))
        elif m_scope is not None:
            meas = dict(m_scope, y=check_measurement(m_scope["y"], x_init.shape, m_scope["scale"], m_scope["gray"]))
        else:
            meas = None
        if self.prefix_cache or self.suffix_skip:                 # the guidance options of an enclosing guidance_scope (engine state)
            L, h = _lib.lib(), self.model._handle
            which = "prefix_cache" if self.prefix_cache else "suffix_skip"
            if float(L.vd_guidance_rescale(h)) != 0.0 and (cfg_scale != 1.0 or float(L.vd_cfg_scale(h)) != 1.0):
                raise NotImplementedError(f"{which} together with cfg_rescale != 0")
            if float(L.vd_dynamic_threshold(h)) != 0.0 and clip_denoised:
                raise NotImplementedError(f"{which} together with dynamic_threshold")
            if L.vd_freeu(h, None, None):                             # an enclosing freeu_scope
                raise NotImplementedError(f"{which} together with FreeU (freeu_scope)")
        mode = model_kwargs.get("observed_frames", "x_0")
        if mode not in _OBS_MODES:
            raise NotImplementedError(f"observed_frames={mode!r}: the window executor handles 'x_0', 'x_t' and 'x_t_minus_1'")
        self.diffusion._refuse_learned(x_init)                        # a learned variance cannot sample (gaussian_diffusion.py:283)
        B, T = x_init.shape[:2]
        bufs = self._buffers(B, T)
        # the engine holds ONE schedule: another diffusion may have been bound to this model since the last window
        # (vd_set_schedule drops the captured graphs, so a stale replay is impossible)
        self.diffusion._bind(self.model)
        cur = th.cuda.current_stream(self.model.device)
        self.stream.wait_stream(cur)
        with th.cuda.stream(self.stream):
            kw = self.model._pack_kwargs(x_init, model_kwargs)
            # the copies below read the caller's tensors on self.stream: keep the caching allocator from handing their
            # memory out again on the caller's stream before these reads have run
            for v in [x_init] + [v for v in kw.values() if isinstance(v, th.Tensor)]:
                if v.is_cuda:
                    v.record_stream(self.stream)
            bufs["x"].copy_(x_init)
            region = None
            if known_src is not None:
                ks, km = self._known_buffers(B, T)
                for v in (known_src, known_mask):
                    if v.is_cuda:
                        v.record_stream(self.stream)
                ks.copy_(known_src)
                km.copy_(known_mask)
                region = dict(src=ks, mask=km)
            if meas is not None:
                yb = self._measurement_buffer(B, T, meas["scale"], meas["gray"])
                if meas["y"].is_cuda:
                    meas["y"].record_stream(self.stream)
                yb.copy_(meas["y"])
                meas = dict(meas, y=yb)
            if lin is not None:
                yb = self._linear_buffer(B, T, lin["A_h"].shape[0], lin["A_w"].shape[0], "projection")
                if lin["y"].is_cuda:
                    lin["y"].record_stream(self.stream)
                yb.copy_(lin["y"])
                lin = dict(lin, y=yb)
            if steer is not None:
                pm = steer["measurement"]
                yb = self._linear_buffer(B, T, pm["A_h"].shape[0], pm["A_w"].shape[0], "reward") if pm.get("A_h") is not None \
                    else self._measurement_buffer(B, T, pm["scale"], pm["gray"], pm.get("kernel") is not None)
                if pm["y"].is_cuda:
                    pm["y"].record_stream(self.stream)
                yb.copy_(pm["y"])
                steer = dict(steer, measurement=dict(pm, y=yb))
            for k in ("obs_mask", "latent_mask", "kinda_marg_mask", "frame_indices"):
                bufs[k].copy_(kw[k].view(bufs[k].shape))
            if mode == "x_0":
                bufs["obs_src"].copy_(kw["obs_src"])
            elif mode == "x_t_minus_1" and renoise:                    # the CLEAN frames: the graph draws q_sample(x0, t - 1) from them
                bufs["obs_src"].copy_(model_kwargs["x0"].to(device=bufs["obs_src"].device, dtype=th.float32))
            elif mode == "x_t_minus_1":                                # the caller's tensor, read as it is by every step
                bufs["obs_src"].copy_(kw["obs_src"])
            if seed is None:
                seed = int(th.randint(0, 2 ** 62, (1,)).item())        # torch.manual_seed governs the run
            sid, up = _sampler_id(sampler), SAMPLERS.get(sampler, SAMPLERS["ddim"]).up
            if t_start is None:
                t_start = 0 if up else self.diffusion.num_timesteps - 1
            obs_src = bufs["x"] if mode == "x_t" else bufs["obs_src"]
            _lib.check(_lib.lib().vd_set_window_prefix_cache(self.model._handle, 1 if self.prefix_cache else 0))
            _lib.check(_lib.lib().vd_set_window_suffix_skip(self.model._handle, 1 if self.suffix_skip else 0))
            # the scale is engine state for the length of this call only: the captured graph keeps the weight, run() needs none
            if cfg_scale != 1.0:
                _lib.check(_lib.lib().vd_set_cfg_scale(self.model._handle, cfg_scale))
            # ... and so is the region: the graph's signature keeps the two buffer addresses
            if region is not None or scope is not None:
                _engine_region(self.model, region)
            # ... and the measurement: the signature keeps the buffer's address, the scale and the gray flag
            if meas is not None:
                _engine_measurement(self.model, meas)
            # ... and the linear measurement: the signature keeps the buffer's address and (Mh, Mw); the matrices' addresses are the engine's
            if lin is not None:
                _engine_linear(self.model, op=lin)
            # ... and the particles: the signature keeps K, the scale, the threshold, y's address, the operator and sigma_y
            s_scope = _scope(self.model, "steering")
            if steer is not None:
                _engine_particles(self.model, steer)
            try:
                rc = _lib.lib().vd_window_begin(
                    self.model._handle, B, T, _lib.ptr(bufs["x"]), _lib.ptr(obs_src), _lib.ptr(bufs["obs_mask"]),
                    _lib.ptr(bufs["latent_mask"]), _lib.ptr(bufs["kinda_marg_mask"]), _lib.ptr(bufs["frame_indices"]),
                    3 if (mode == "x_t_minus_1" and not renoise) else _OBS_MODES[mode], sid, 1 if clip_denoised else 0, float(eta), seed, 0,
                    int(t_start), self.stream.cuda_stream)
            finally:
                if steer is not None:
                    _engine_particles(self.model, s_scope)
                if lin is not None:
                    _engine_linear(self.model)
                if meas is not None:
                    _engine_measurement(self.model, m_scope)
                if region is not None or scope is not None:
                    _engine_region(self.model, scope)
                if cfg_scale != 1.0:
                    _lib.check(_lib.lib().vd_set_cfg_scale(self.model._handle, 1.0))
            _lib.check(rc)
        self.x = bufs["x"]
        self._particles = None if steer is None else (B, steer["K"])
        self.seed = seed
        self._left = self.diffusion.num_timesteps - int(t_start) if up else int(t_start) + 1
        self._gen = int(_lib.lib().vd_window_generation(self.model._handle))
        return self

    def _steering(self, x_init, sampler, eta, particles, reward_fn, reward_scale, ess_threshold, y, sr_scale, gray, sigma_y, blur_kernel, region,
                  meas, operator=None):
        """begin()'s particle keywords, or the enclosing steering_scope's setting, checked before anything touches the engine -> a steering
        dict (gaussian_diffusion.py: _engine_particles) or None (the plain window)."""
        scope = _scope(self.model, "steering")
        if reward_fn is not None or (scope is not None and scope["measurement"] is None and particles == 1):
            raise NotImplementedError("WindowExecutor.begin with a reward_fn is not served: a Python callback between two steps cannot be "
                                      "captured in a graph (the built-in reward can: particle_measurement=, sigma_y=)")
        if blur_kernel is not None and y is None:
            raise ValueError("WindowExecutor.begin: blur_kernel is the operator of the built-in reward: it needs particle_measurement= and sigma_y=")
        if particles == 1 and y is None:
            if scope is None:
                return None
            d = dict(scope)
        else:
            if y is None:
                raise ValueError("WindowExecutor.begin: particles > 1 needs particle_measurement= and sigma_y= (the built-in reward)")
            K, lam, tau, sig = check_steering(None, y, particles, reward_scale, ess_threshold, sigma_y)
            lin_op = {}
            if operator is not None:
                sc, gr, w, lin_op = 1, False, None, dict(A_h=operator[0], A_w=operator[1])
            elif blur_kernel is not None:
                if not (sr_scale == 1 and gray is False):
                    raise ValueError("WindowExecutor.begin: blur_kernel together with particle_sr_scale or particle_gray is not served: "
                                     "leave them at their defaults")
                sc, gr, w = 1, False, check_blur_kernel(blur_kernel)
            else:
                (sc, gr), w = _check_operator(sr_scale, gray), None
            if K == 1 or lam == 0.0:
                return None
            d = dict(K=K, scale=lam, tau=tau, measurement=dict(y=y, scale=sc, gray=gr, sigma_y=sig, kernel=w, **lin_op))
        m = d["measurement"]
        if m.get("A_h") is not None:
            m = dict(m, y=check_linear_measurement(m["y"], x_init.shape, m["A_h"], m["A_w"]))
        elif m.get("kernel") is not None:
            m = dict(m, y=check_blur_measurement(m["y"], x_init.shape))
        else:
            m = dict(m, y=check_measurement(m["y"], x_init.shape, m["scale"], m["gray"]))
        row = SAMPLERS.get(sampler, SAMPLERS["ddim"])
        if row.noise is None or (row.eta and float(eta) == 0.0):
            raise NotImplementedError(f"sampler={sampler!r}{' at eta = 0' if row.noise is not None else ''} together with particles is not served: "
                                      "the step draws no noise, duplicated particles would never separate")
        for name, on in (("prefix_cache", self.prefix_cache), ("suffix_skip", self.suffix_skip), ("a known region", region), ("a measurement", meas)):
            if on:
                raise NotImplementedError(f"{name} together with particles is not served")
        if x_init.shape[0] % d["K"]:
            raise ValueError(f"WindowExecutor.begin: the batch of {x_init.shape[0]} items is no multiple of particles={d['K']}")
        return dict(d, measurement=m)

    def particle_state(self):
        """The particle state of the armed window behind the steps run so far (waits for the device) -> dict log_weights (B,), rprev (B,)
        float64, ancestors (B,) int32 (of the last step), chosen (G,) int32 (-1 before the step at t == 0), ess (G,) float64, resamples
        (G,) and degenerate (G,) int64, as host tensors."""
        if getattr(self, "_particles", None) is None:
            raise RuntimeError("WindowExecutor.particle_state: the armed window has no particles (begin(..., particles=K, ...))")
        self._check_gen("particle_state")
        B, K = self._particles
        G = B // K
        out = dict(log_weights=th.empty(B, dtype=th.float64), rprev=th.empty(B, dtype=th.float64), ancestors=th.empty(B, dtype=th.int32),
                   chosen=th.empty(G, dtype=th.int32), ess=th.empty(G, dtype=th.float64))
        counters = th.empty(G, 2, dtype=th.int64)
        _lib.check(_lib.lib().vd_particle_state(self.model._handle, B, *(_lib.ptr(out[k]) for k in ("log_weights", "rprev", "ancestors", "chosen", "ess")),
                                                _lib.ptr(counters)))
        out["resamples"], out["degenerate"] = counters[:, 0].clone(), counters[:, 1].clone()
        return out

    def run(self, n_steps=None):
        """Replay the step graph n_steps times (default: down to t = 0; 'ddim_reverse': up to the last index).  Returns the
        window tensor (updated in place)."""
        if n_steps is None:
            n_steps = self._left
        self._check_gen("run")
        self._after_caller()
        _lib.check(_lib.lib().vd_window_run(self.model._handle, int(n_steps), self.stream.cuda_stream))
        self._left -= int(n_steps)
        th.cuda.current_stream(self.model.device).wait_stream(self.stream)
        return self.x

    def _after_caller(self):
        """The executor's stream waits for what the caller's stream holds: a read of the window tensor enqueued there (`run(3).clone()`)
        must finish before the next replay or jump writes the tensor."""
        self.stream.wait_stream(th.cuda.current_stream(self.model.device))

    def _check_gen(self, what):
        # the step counters are one set per engine: refuse to continue a window another executor has re-armed since
        if getattr(self, "_gen", None) != int(_lib.lib().vd_window_generation(self.model._handle)):
            raise RuntimeError(f"WindowExecutor.{what}: another window was begun on this model since this executor's begin(); "
                               "begin() again")

    def jump(self, n=1):
        """n forward diffusion steps of the armed window (a window with a known region only): t += 1 and q_jump at the new t, n times,
        noise from the window's Philox stream (a range of B*per each); a 'dpmpp_2m' or 'dpmpp_2m_sde' window's next step is first-order again.  Returns
        the window tensor (updated in place)."""
        self._check_gen("jump")
        self._after_caller()
        _lib.check(_lib.lib().vd_window_jump(self.model._handle, int(n), self.stream.cuda_stream))
        self._left += int(n)
        th.cuda.current_stream(self.model.device).wait_stream(self.stream)
        return self.x

    def run_repaint(self, jump_length=1, n_resample=1):
        """The walk of respace.repaint_schedule from the armed window's current index down to 0: runs of steps as graph replays, runs of
        jumps through jump().  Returns the window tensor."""
        from .respace import repaint_schedule
        if self._left < 1:
            raise RuntimeError("WindowExecutor.run_repaint: the window has no step left")
        ops = repaint_schedule(self._left - 1, jump_length, n_resample)
        k = 0
        while k < len(ops):
            n = 1
            while k + n < len(ops) and ops[k + n][0] == ops[k][0]:
                n += 1
            (self.run if ops[k][0] == "step" else self.jump)(n)
            k += n
        return self.x

    def sample_window(self, x_init, model_kwargs, sampler="p_sample", eta=0.0, seed=None, renoise=True, known_src=None, known_mask=None,
                      jump_length=1, n_resample=1, measurement=None, sr_scale=1, gray=False, particles=1, reward_fn=None, reward_scale=1.0,
                      ess_threshold=0.5, particle_measurement=None, particle_sr_scale=1, particle_gray=False, sigma_y=None, blur_kernel=None,
                      operator=None, operator_rtol=1e-3, cfg_scale=1.0):
        """All num_timesteps steps of one window (with a known region and n_resample > 1: the walk of run_repaint); returns a fresh tensor."""
        self.begin(x_init, model_kwargs, seed=seed, sampler=sampler, eta=eta, renoise=renoise, cfg_scale=cfg_scale, known_src=known_src,
                   known_mask=known_mask, measurement=measurement, sr_scale=sr_scale, gray=gray, particles=particles, reward_fn=reward_fn,
                   reward_scale=reward_scale, ess_threshold=ess_threshold, particle_measurement=particle_measurement,
                   particle_sr_scale=particle_sr_scale, particle_gray=particle_gray, sigma_y=sigma_y, blur_kernel=blur_kernel,
                   operator=operator, operator_rtol=operator_rtol)
        if int(n_resample) != 1:
            return self.run_repaint(jump_length, n_resample).clone()
        return self.run(self.diffusion.num_timesteps).clone()

    @property
    def cached_frames(self):
        """Frames of the armed window whose prefix activations come from the cache (0: cache off or nothing observed)."""
        return int(_lib.lib().vd_window_prefix_frames(self.model._handle))

    @property
    def suffix_frames(self):
        """Frames the armed window's suffix (everything behind the last attention layer) runs on (0: all of them)."""
        return int(_lib.lib().vd_window_suffix_frames(self.model._handle))

    @property
    def graphs(self):
        return int(_lib.lib().vd_window_graphs(self.model._handle))
