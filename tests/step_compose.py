"""A denoise step composed from entries that have per-element tests of their own, in the order csrc/engine.hip's step_launches runs its
passes -- shared by the GPU files that compare a fused step, or a window graph, with such a composition to the bit.

The first half are the helpers test_gpu_guidance.py (_combine, _rescale, _threshold, _kw, _compose), test_gpu_measurement.py (_project,
_from_xstart) and test_gpu_known_region.py (_randn, _eager_chain) owned and still import; the second half is the composition of the whole
option matrix of tests/step_matrix_cases.py, and the eager chain a window of that matrix is compared with.  Imported on a GPU machine only."""
import contextlib

import torch

import step_matrix_cases as sm
from video_diffusion_amd import _lib
from video_diffusion_amd.gaussian_diffusion import (SAMPLERS, blur, check_separable_operator, freeu_state, gaussian_kernel, measure,
                                                    measure_separable, resize_matrix, separable_pinv)

MODES = {"p_sample": 0, "ddim": 1, "dpmpp_2m": 3}


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def _tb(B, v):
    return torch.tensor([v] * B, device="cuda")


# ------------------------------------------------------------------------------------------------ moved from test_gpu_guidance.py
def _combine(c, u, w):
    out = torch.empty_like(c)
    _lib.check(_lib.lib().vd_op_cfg_combine(_lib.ptr(c), _lib.ptr(u), float(w), c.numel(), _lib.ptr(out), _lib.current_stream()))
    return out


def _rescale(c, u, w, lat, phi, out=None):
    b, t, fe = c.shape
    out = torch.empty_like(c) if out is None else out
    f = torch.empty(b, device="cuda")
    _lib.check(_lib.lib().vd_op_cfg_rescale(_lib.ptr(c), _lib.ptr(u), float(w), _lib.ptr(lat), b, t, fe, float(phi), _lib.ptr(out), _lib.ptr(f),
                                            _lib.current_stream()))
    return out, f


def _threshold(x, lat, p, out=None):
    b, t, fe = x.shape
    out = torch.empty_like(x) if out is None else out
    s = torch.empty(b, device="cuda")
    _lib.check(_lib.lib().vd_op_dynamic_threshold(_lib.ptr(x), _lib.ptr(lat), b, t, fe, float(p), _lib.ptr(out), _lib.ptr(s), _lib.current_stream()))
    return out, s


def _kw(c, zero_obs=False):
    d = {k: c[k] for k in ["x0", "obs_mask", "latent_mask", "kinda_marg_mask", "frame_indices"]}
    if zero_obs:
        d["obs_mask"] = torch.zeros_like(d["obs_mask"])
    return dict(d, x_t_minus_1=c["xtm1"], observed_frames="x_0")


def _compose(model, diff, c, tv, w, phi, p, mode, eta, nz, start_x, prev=None):
    """The step from existing entries: p_mean_variance(clip off, cfg_scale) for the network outputs, the two op entries on them, then the
    *_from_xstart pass with its clamp off behind the threshold (on, as in the plain step, without it).  Called outside any scope.
    -> (sample, pred_xstart, per-item thresholds or None)."""
    L = _lib.lib()
    x, per = c["x"], c["x"][0].numel()
    B, T = x.shape[:2]
    FE = per // T
    kw, t = _kw(c), _tb(B, tv)
    lat = c["latent_mask"].reshape(B, T).contiguous()
    out = diff.p_mean_variance(model, x, t, clip_denoised=False, model_kwargs=kw, cfg_scale=w)["eps"]
    if phi != 0.0 and w != 1.0:
        out_c = diff.p_mean_variance(model, x, t, clip_denoised=False, model_kwargs=kw)["eps"]
        out_u = diff.p_mean_variance(model, x, t, clip_denoised=False, model_kwargs=_kw(c, zero_obs=True))["eps"]
        assert torch.equal(bits(_combine(out_c, out_u, w)), bits(out))
        out = _rescale(out_c.view(B, T, FE), out_u.view(B, T, FE), w, lat, phi)[0].view_as(x)
    if start_x:
        x0 = out
    else:                                                                        # x_0 as the posterior pass forms it from eps
        x0, dummy = torch.empty_like(x), torch.empty_like(x)
        _lib.check(L.vd_posterior_update(model._handle, 0, B, per, _lib.ptr(x), _lib.ptr(out), _lib.ptr(t), 0, 0.0, _lib.ptr(nz), 0, 0,
                                         _lib.ptr(dummy), _lib.ptr(x0), _lib.current_stream()))
    s, clip = None, 1
    if p:
        x0, s = _threshold(x0.view(B, T, FE), lat, p)
        x0, clip = x0.view_as(x), 0
    sample, xstart = torch.empty_like(x), torch.empty_like(x)
    if mode == 2:
        _lib.check(L.vd_ddim_reverse_from_xstart(model._handle, B, per, _lib.ptr(x), _lib.ptr(x0), _lib.ptr(t), clip, _lib.ptr(sample),
                                                 _lib.ptr(xstart), _lib.current_stream()))
    elif mode == 3:
        _lib.check(L.vd_dpmpp_2m_from_xstart(model._handle, B, per, _lib.ptr(x), _lib.ptr(x0), _lib.ptr(prev), _lib.ptr(t), clip,
                                             _lib.ptr(sample), _lib.ptr(xstart), _lib.current_stream()))
    else:
        _lib.check(L.vd_posterior_from_xstart(model._handle, mode, B, per, _lib.ptr(x), _lib.ptr(x0), _lib.ptr(t), clip, eta, _lib.ptr(nz), 0, 0,
                                              _lib.ptr(sample), _lib.ptr(xstart), None, _lib.current_stream()))
    return sample, xstart, s


# ------------------------------------------------------------------------------------------------ moved from test_gpu_measurement.py
def _project(model, x0, y, lat, s, gray, misalign=False):
    """vd_measurement_project on device copies -> the projected x_0 (a device tensor).  misalign: x_0 at an address 4 bytes off."""
    B, T, _, H, W = x0.shape
    if misalign:
        buf = torch.empty(x0.numel() + 1, device="cuda")
        out = buf[1:].view(x0.shape)
        out.copy_(x0)
        assert out.data_ptr() % 16 == 4
    else:
        out = x0.cuda().clone()
    yd, ld = y.cuda().float().contiguous(), lat.cuda().float().reshape(-1).contiguous()
    _lib.check(_lib.lib().vd_measurement_project(model._handle, B, T, H, W, _lib.ptr(out), _lib.ptr(yd), _lib.ptr(ld), s, 1 if gray else 0,
                                                 _lib.current_stream()))
    return out


def _from_xstart(model, mode, x, x0, t, eta, noise, prev, want_mean=False):
    """The sampler pass alone on an x_0 handed in, clip off -> (sample, pred_xstart) or the posterior mean."""
    L = _lib.lib()
    B, per = x.shape[0], x[0].numel()
    sample, xs, mean = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    if mode == 3:
        _lib.check(L.vd_dpmpp_2m_from_xstart(model._handle, B, per, _lib.ptr(x), _lib.ptr(x0), _lib.ptr(prev), _lib.ptr(t), 0, _lib.ptr(sample),
                                             _lib.ptr(xs), _lib.current_stream()))
    else:
        _lib.check(L.vd_posterior_from_xstart(model._handle, mode, B, per, _lib.ptr(x), _lib.ptr(x0), _lib.ptr(t), 0, float(eta), _lib.ptr(noise),
                                              0, 0, None if want_mean else _lib.ptr(sample), _lib.ptr(xs), _lib.ptr(mean) if want_mean else None,
                                              _lib.current_stream()))
    return mean if want_mean else (sample, xs)


# ------------------------------------------------------------------------------------------------ moved from test_gpu_known_region.py
def _randn(shape, seed, offset):
    out = torch.empty(shape, device="cuda")
    _lib.check(_lib.lib().vd_randn(_lib.ptr(out), out.numel(), seed, offset, _lib.current_stream()))
    return out


def _eager_chain(model, diff, sampler, eta, x_init, kw, src, mask, seed, ops, keep=()):
    """The window's documented arithmetic from the eager entries: op k owns the Philox range [k n, (k + 1) n), n = B per; a step draws
    its sampler noise at k n and its merge noise at k n + n // 4 (vd_known_merge on the plain step's sample); a jump draws at k n and
    drops dpmpp_2m's history."""
    L = _lib.lib()
    B, T, _, S, _ = x_init.shape
    n = x_init.numel()
    lat = kw["latent_mask"].reshape(-1).float().contiguous()
    x, prev, kept = x_init.clone(), None, {}
    for k, (op, tv) in enumerate(ops):
        tt = _tb(B, tv)
        if op == "jump":
            out = torch.empty_like(x)
            _lib.check(L.vd_q_jump(model._handle, B, T, S * S, _lib.ptr(x), _lib.ptr(lat), _lib.ptr(tt), _lib.ptr(_randn(x.shape, seed, k * n)), 0, 0,
                                   _lib.ptr(out), _lib.current_stream()))
            x, prev = out, None
        else:
            noise = _randn(x.shape, seed, k * n) if sampler != "dpmpp_2m" else None
            x, prev = diff._fused_step(MODES[sampler], model, x, tt, True, kw, eta=eta, noise=noise, prev_xstart=prev)
            if src is not None:
                z = _randn(x.shape, seed, k * n + n // 4)
                _lib.check(L.vd_known_merge(model._handle, B, T, S * S, _lib.ptr(x), _lib.ptr(src), _lib.ptr(mask), _lib.ptr(lat), _lib.ptr(tt),
                                            _lib.ptr(z), 0, 0, _lib.current_stream()))
        if k + 1 in keep:
            kept[k + 1] = x.clone()
    return x, kept


# ================================================================================================ the option matrix
T_, S_ = 6, 32
SIGMA_Y = 1.5                                                                    # the built-in reward's noise level: weights that differ, none of them 0


def matrix_window(B, seed):
    """The window of test_gpu_guidance._window as two groups of B / 2 consecutive items that share everything but x (the particles of
    one video; B = 2: the window itself).  Group 0: frames 0-1 observed, frame 2 kinda-marginalised, frames 3-4 latent, frame 5 padding;
    group 1: nothing observed, frames 0-4 latent, frame 5 padding."""
    g = torch.Generator().manual_seed(seed)
    K = B // 2
    x0 = torch.rand(2, T_, 3, S_, S_, generator=g) * 2 - 1
    obs, lat, km = torch.zeros(2, T_, 1, 1, 1), torch.zeros(2, T_, 1, 1, 1), torch.zeros(2, T_, 1, 1, 1)
    obs[0, :2] = 1
    km[0, 2] = 1
    lat[0, 3:5] = 1
    lat[1, :5] = 1
    x0 = x0 * obs
    xtm1 = 0.5 * x0 + 0.1 * torch.randn(2, T_, 3, S_, S_, generator=g) * obs
    rep = lambda v: v.repeat_interleave(K, dim=0).cuda()                         # noqa: E731
    return dict(x=(1.5 * torch.randn(B, T_, 3, S_, S_, generator=g)).cuda(), x0=rep(x0), obs_mask=rep(obs), latent_mask=rep(lat), kinda_marg_mask=rep(km),
                frame_indices=torch.arange(T_).view(1, T_).repeat(B, 1).cuda(), xtm1=rep(xtm1),
                truth=torch.rand(2, T_, 3, S_, S_, generator=g) * 2 - 1)


def restoration_of(kind, c, seed):
    """What the row's restoration option is made of, for the window `c`: the tensors the scope is handed and the composition reads."""
    B = c["x"].shape[0]
    K = B // 2
    g = torch.Generator().manual_seed(seed)
    video = torch.rand(B, T_, 3, S_, S_, generator=g) * 2 - 1
    noisy = lambda y: (y + 0.1 * torch.randn(y.shape, generator=g)).repeat_interleave(K, dim=0).cuda()   # noqa: E731
    if kind.startswith("meas"):
        s, gray = (2, False) if kind == "meas_s2_colour" else (1, True)
        return dict(kind=kind, y=measure(video, s, gray).cuda(), scale=s, gray=gray)
    if kind == "linear":
        A = resize_matrix(S_, S_ // 2)
        a_h, a_w = check_separable_operator(A, A)
        return dict(kind=kind, y=measure_separable(video, A, A).cuda(), A=(A, A), a=(a_h, a_w), P=(separable_pinv(a_h, 1e-3)[0], separable_pinv(a_w, 1e-3)[0]))
    if kind == "known":
        return dict(kind=kind, src=video.cuda(), mask=(torch.rand(B, T_, S_, S_, generator=g) < 0.5).float().cuda())
    if kind == "part_cell4":
        return dict(kind=kind, y=noisy(measure(c["truth"], 4, False)), steer=dict(sr_scale=4))
    if kind == "part_blur5":
        w = gaussian_kernel(5, 1.2)
        return dict(kind=kind, y=noisy(blur(c["truth"], w)), steer=dict(blur_kernel=w))
    if kind == "part_linear":
        A = resize_matrix(S_, S_ // 2)
        return dict(kind=kind, y=noisy(measure_separable(c["truth"], A, A)), steer=dict(operator=(A, A)))
    assert kind == "none"
    return dict(kind=kind)


@contextlib.contextmanager
def model_scopes(diff, model, case):
    """FreeU and guidance_scope of the row (cfg_scale is each entry's own keyword or scope)."""
    _, phi, p = sm.GUIDANCE[case.guidance]
    fu = sm.FREEU[case.freeu]
    with contextlib.ExitStack() as st:
        if fu is not None:
            st.enter_context(diff.freeu_scope(model, **fu))
        if phi != 0.0 or p is not None:
            st.enter_context(diff.guidance_scope(model, cfg_rescale=phi, dynamic_threshold=p))
        yield


def restoration_scope(diff, model, R, known_noise=None, uniforms=None):
    """The row's restoration scope.  known_noise: the merge's noise; uniforms: steering_scope's (a callable, or None: the step's Philox pair)."""
    k = R["kind"]
    if k.startswith("meas"):
        return diff.measurement_scope(model, R["y"], R["scale"], R["gray"])
    if k == "linear":
        return diff.linear_measurement_scope(model, R["y"], *R["A"])
    if k == "known":
        return diff.known_region_scope(model, R["src"], R["mask"], known_noise=known_noise)
    if k.startswith("part"):
        return diff.steering_scope(model, particles=sm.PARTICLES, scale=1.0, ess_threshold=1.0, measurement=R["y"], sigma_y=SIGMA_Y, uniforms=uniforms,
                                   **R["steer"])
    return contextlib.nullcontext()


def fused_step(diff, model, case, x, t, kw, noise=None, carry=None, philox=None):
    """The row's sampler through the entry a caller reaches it by, under the row's cfg_scale -> dict sample, pred_xstart[, state][, ancestors, ...].
    carry: prev_xstart (dpmpp_2m, dpmpp_2m_sde) or the state (unipc) of the step before, or None."""
    name, eta = sm.SAMPLER[case.sampler]
    w = sm.GUIDANCE[case.guidance][0]
    row = SAMPLERS[name]
    if row.cfg_keyword:
        sample, xstart = diff._step(row.id, model, x, t, True, None, kw, eta, noise, cfg_scale=w)
        return dict(sample=sample, pred_xstart=xstart, **(diff._last_steer or {}))
    with (diff.cfg_scale_scope(model, w) if w != 1.0 else contextlib.nullcontext()):
        return diff._scope_step(name, model, x, t, True, None, kw, noise=noise, philox=philox, **({row.carry: carry} if row.carry else {}))


def from_xstart(model, name, x, x0, t, clip, eta=0.0, noise=None, prev=None, state=None):
    """The network-free entry of sampler `name` on an x_0 handed in -> (sample, pred_xstart, state or None, posterior mean or None).  Every
    argument list is written out here as include/vd_amd.h declares it."""
    L, h, st = _lib.lib(), model._handle, _lib.current_stream()
    B, per, clip = x.shape[0], x[0].numel(), 1 if clip else 0
    P = _lib.ptr
    sample, xs, mean, new = torch.empty_like(x), torch.empty_like(x), None, None
    if name in ("p_sample", "ddim"):
        mean = torch.empty_like(x)
        _lib.check(L.vd_posterior_from_xstart(h, MODES[name], B, per, P(x), P(x0), P(t), clip, float(eta), P(noise), 0, 0, P(sample), P(xs), P(mean), st))
    elif name == "ddim_reverse":
        _lib.check(L.vd_ddim_reverse_from_xstart(h, B, per, P(x), P(x0), P(t), clip, P(sample), P(xs), st))
    elif name == "dpmpp_2m":
        _lib.check(L.vd_dpmpp_2m_from_xstart(h, B, per, P(x), P(x0), P(prev), P(t), clip, P(sample), P(xs), st))
    elif name == "dpmpp_2m_sde":
        _lib.check(L.vd_dpmpp_2m_sde_from_xstart(h, B, per, P(x), P(x0), P(prev), P(t), clip, P(noise), 0, 0, P(sample), P(xs), st))
    else:
        assert name == "unipc"
        base, d1, d2, count = (None, None, None, 0) if state is None else state
        outs = tuple(torch.empty_like(x) for _ in range(3))
        _lib.check(L.vd_unipc_from_xstart(h, B, per, P(x), P(x0), P(base), P(d1), P(d2), int(count), P(t), clip, P(sample), P(xs), P(outs[0]), P(outs[1]),
                                          P(outs[2]), st))
        new = (*outs, int(count) + 1)
    return sample, xs, new, mean


def compose_step(model, diff, case, c, R, tv, noise, carry=None, known_noise=None):
    """The row's step at index tv from tested entries, in step_launches' order -> dict sample, pred_xstart, state (unipc), and x0 / mean:
    the finished x_0 in front of anything behind the sampler pass, and p_mean_variance's posterior mean of it.
    1 the conditional and the unconditional network output (p_mean_variance, clip off, inside the row's freeu_scope and nothing else);
    2 vd_op_cfg_combine, or vd_op_cfg_rescale in its place;  3 the x_0 head, vd_op_dynamic_threshold behind it;  4 the projection
    (vd_measurement_project / vd_op_linear_project) on the clamped or thresholded x_0;  5 the sampler's *_from_xstart entry, clamp off
    behind 3's threshold or 4, on otherwise;  6 vd_known_merge.  Particles: the tensors in front of the gather -- `restated_particles` says
    from them which item each item takes."""
    L = _lib.lib()
    name, eta = sm.SAMPLER[case.sampler]
    w, phi, p = sm.GUIDANCE[case.guidance]
    fu = sm.FREEU[case.freeu]
    x, per = c["x"], c["x"][0].numel()
    B, T = x.shape[:2]
    FE = per // T
    kw, t = _kw(c), _tb(B, tv)
    lat = c["latent_mask"].reshape(B, T).contiguous()
    nz = noise if noise is not None else torch.zeros_like(x)
    with (diff.freeu_scope(model, **fu) if fu is not None else contextlib.nullcontext()):
        out = diff.p_mean_variance(model, x, t, clip_denoised=False, model_kwargs=kw)["eps"]
        if w != 1.0:
            out_u = diff.p_mean_variance(model, x, t, clip_denoised=False, model_kwargs=_kw(c, zero_obs=True))["eps"]
            out = _rescale(out.view(B, T, FE), out_u.view(B, T, FE), w, lat, phi)[0].view_as(x) if phi != 0.0 else _combine(out, out_u, w)
    if case.model == "xstart":
        x0 = out
    else:
        x0, dummy = torch.empty_like(x), torch.empty_like(x)
        _lib.check(L.vd_posterior_update(model._handle, 0, B, per, _lib.ptr(x), _lib.ptr(out), _lib.ptr(t), 0, 0.0, _lib.ptr(nz), 0, 0,
                                         _lib.ptr(dummy), _lib.ptr(x0), _lib.current_stream()))
    clip = True
    if p is not None:
        x0, clip = _threshold(x0.view(B, T, FE), lat, p)[0].view_as(x), False
    kind = R["kind"]
    if kind.startswith("meas") or kind == "linear":
        if clip:                                                                 # the clamp of clip_denoised, as the posterior entry applies it
            x0, clip = from_xstart(model, "p_sample", x, x0, t, True, noise=nz)[1], False
        if kind == "linear":
            mats = [m.cuda() for m in (*R["a"], *R["P"])]
            x0 = x0.clone()
            _lib.check(L.vd_op_linear_project(model._handle, B, T, S_, S_, _lib.ptr(x0), _lib.ptr(R["y"]), _lib.ptr(lat.reshape(-1)), _lib.ptr(mats[0]),
                                              mats[0].shape[0], _lib.ptr(mats[1]), mats[1].shape[0], _lib.ptr(mats[2]), _lib.ptr(mats[3]), 0,
                                              _lib.current_stream()))
        else:
            x0 = _project(model, x0, R["y"], lat, R["scale"], R["gray"])
    row = SAMPLERS[name]
    sample, xs, state, _ = from_xstart(model, name, x, x0, t, clip, eta, noise if row.noise is not None else None,
                                       carry if row.carry == "prev_xstart" else None, carry if row.carry == "state" else None)
    mean = from_xstart(model, "p_sample", x, x0, t, clip, noise=nz)[3]
    res = dict(x0=xs, mean=mean, state=state)
    if kind == "known":
        sample = sample.clone()
        _lib.check(L.vd_known_merge(model._handle, B, T, S_ * S_, _lib.ptr(sample), _lib.ptr(R["src"]), _lib.ptr(R["mask"]), _lib.ptr(lat.reshape(-1)),
                                    _lib.ptr(t), _lib.ptr(known_noise), 0, 0, _lib.current_stream()))
    return dict(res, sample=sample, pred_xstart=xs, lat=lat)


def particle_reward(R, v, lat):
    """The built-in reward of the row's operator in float64 from the tensor `v` the engine's residual pass reads (pred_xstart; the sample
    at t == 0), as test_gpu_particles.py restates it -> (r (B,), bar (B,)).  The restated seed_bound of each operator (dps_restated,
    blur_restated, linop_restated: the float32 products and residuals, the fp64 sum) gives rho and a bound d on the engine's rho; the reward is
    r = -rho^2 / (2 sigma_y^2), so |r_engine - r| <= ((rho + d)^2 - rho^2) / (2 sigma_y^2) = bar."""
    import numpy as np
    vn, yn = v.detach().cpu().numpy().astype(np.float64), R["y"].detach().cpu().numpy().astype(np.float64)
    latn = lat.detach().cpu().numpy().reshape(vn.shape[0], -1)
    h = np.zeros_like(vn)
    if R["kind"] == "part_cell4":
        from dps_restated import seed_bound
        rho, d = seed_bound(vn, h, yn, latn, 4, False)["rho"]
    elif R["kind"] == "part_blur5":
        from blur_restated import seed_bound
        rho, d = seed_bound(vn, h, yn, latn, R["steer"]["blur_kernel"].numpy())["rho"]
    else:
        from linop_restated import seed_bound
        a_h, a_w = (a.numpy() for a in check_separable_operator(*R["steer"]["operator"]))
        rho, d = seed_bound(vn, h, yn, latn, a_h, a_w)["rho"]
    return -rho ** 2 / (2 * SIGMA_Y ** 2), (2 * rho * d + d * d) / (2 * SIGMA_Y ** 2)


def restated_particles(R, pre, final, seed):
    """What particle steering does behind the composition's tensors `pre`, from a chain's first step (weights 0), by tests/particle_restated.py:
    the reward on pre's pred_xstart (its sample where `final`: t == 0), the weights at scale 1 and ess_threshold 1, the ancestors.  The
    uniforms are the first draw of default_rng(seed) whose thresholds keep 4 x the reward's bar away from every running sum c_k -- the
    margin of test_gpu_particles.py, under which the engine's float32 residuals cannot move an ancestor -> (u (G, 2) for the step to be
    handed, the restatement's dict, the state behind it, r, bar)."""
    import numpy as np
    import particle_restated as pr
    from test_gpu_particles import _margin
    B = pre["sample"].shape[0]
    G, K = B // sm.PARTICLES, sm.PARTICLES
    r, bar = particle_reward(R, pre["sample"] if final else pre["pred_xstart"], pre["lat"])
    rng = np.random.default_rng(seed)
    fin = np.full(G, final)
    for _ in range(100):
        u = rng.random((G, 2))
        st = pr.new_state(G, K)
        want = pr.particle_weights(st, r.reshape(G, K), 1.0, 1.0, u, fin)
        if _margin(want, u, fin) > 4 * bar.max():
            return u, want, st, r, bar
    raise AssertionError(("no uniforms with the margin", float(bar.max())))


def engine_state(model):
    """The engine's option state: cfg_scale, guidance rescale, dynamic threshold, FreeU, and whether a measurement, a known region, a linear
    measurement, particles and the two particle operators are set."""
    L, h = _lib.lib(), model._handle
    return (float(L.vd_cfg_scale(h)), float(L.vd_guidance_rescale(h)), float(L.vd_dynamic_threshold(h)), freeu_state(model),
            L.vd_measurement(h, None, None), L.vd_known_region(h), L.vd_linear_measurement(h), L.vd_particles(h), L.vd_particle_blur(h),
            L.vd_particle_linear(h))


ENGINE_OFF = (1.0, 0.0, 0.0, ((1.0, 1.0, 1.0, 1.0), False), 0, 0, 0, 0, 0, 0)


def window_history(ex, name, B):
    """What the armed window of `ex` (sampler `name`) carries: (hist, ubase, ud2) as fresh tensors, None where the sampler carries none."""
    row = SAMPLERS[name]
    if row.carry is None:
        return None
    x = ex.x
    hist = torch.empty_like(x)
    ubase, ud2 = (torch.empty_like(x), torch.empty_like(x)) if row.carry == "state" else (None, None)
    _lib.check(_lib.lib().vd_window_history(ex.model._handle, B, x.shape[1], _lib.ptr(hist), _lib.ptr(ubase), _lib.ptr(ud2), ex.stream.cuda_stream))
    torch.cuda.current_stream().wait_stream(ex.stream)
    return hist, ubase, ud2


def eager_window(model, diff, case, c, R, seed, steps, t_start):
    """The window's steps as fused eager steps inside the row's scopes, at the window's Philox offsets: step k owns [k n, (k + 1) n),
    n = B per -- the sampler's noise at k n (a vd_randn tensor; dpmpp_2m_sde: the pass draws there itself), the merge's at k n + n // 4,
    the particles' uniforms from the same range through a (seed, offset) pair -> per step (sample, what the next step is handed)."""
    name, _ = sm.SAMPLER[case.sampler]
    row = SAMPLERS[name]
    kw, x = _kw(c), c["x"]
    B, n = x.shape[0], x.numel()
    k_now = [0]
    steer = R["kind"].startswith("part")
    uniforms = None if (not steer or name == "dpmpp_2m_sde") else (lambda tt: (seed, k_now[0] * n))
    trace, carry = [], None
    with model_scopes(diff, model, case), (restoration_scope(diff, model, R, uniforms=uniforms) if steer else contextlib.nullcontext()):
        for k in range(steps):
            k_now[0] = k
            t = _tb(B, t_start + k if row.up else t_start - k)
            noise = _randn(x.shape, seed, k * n) if row.noise == "tensor" else None
            philox = (seed, k * n) if row.noise == "philox" else None
            z = _randn(x.shape, seed, k * n + n // 4) if R["kind"] == "known" else None
            with (contextlib.nullcontext() if steer else restoration_scope(diff, model, R, known_noise=z)):
                out = fused_step(diff, model, case, x, t, kw, noise=noise, carry=carry, philox=philox)
            x = out["sample"]
            carry = out["pred_xstart"] if row.carry == "prev_xstart" else out.get("state")
            trace.append((x, carry))
    return trace
