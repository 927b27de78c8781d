"""GPU: no engine entry's bits depend on what its scratch memory held when the call began -- one test per row of
tests/scratch_cases.py and history, the windows, the held pass, the long-window and configuration shapes, and the evaluator handles.

The engine's workspace is one buffer every entry shares (stack discipline, a tail recomputed per shape), about twenty more buffers are
grown lazily with their contents not kept, and many kernels read padding on purpose.  A pad column times a zero weight, or a partial
that is accumulated into, is right on the zero pages of a fresh process and on finite leftovers, which is all the rest of the suite
ever offers.  Here the memory is SET (vd_scratch_fill: every byte of the workspace and of each scratch buffer) to zeros, to 0x7F bytes
(float32 3.39e38, float64 1.4e306: 0 x it is 0, it + it overflows) and to 0xFF bytes (NaN in both widths), in that order, or left as
other calls left it.

The yardstick is the same call on a freshly created engine, to the bit: both sides run the same deterministic kernels on the same
inputs, so nothing is measured and nothing has a tolerance.  Compared: every tensor the entry writes, the state it leaves (particle
state, window history) and the flags of vd_device_errors.

The step rows are the served rows of tests/step_matrix_cases.py on the windows of tests/step_compose.py (B = 2 or 4, T = 6, as those
files define them); every other row runs at B = 2, T = 3 with one observed frame in item 0 and none in item 1."""
import ctypes
import functools

import pytest
import torch

import scratch_cases as sk
import step_compose as sc
import step_matrix_cases as sm
import video_diffusion_amd as vda
from video_diffusion_amd import _lib
from video_diffusion_amd.executor import WindowExecutor
from video_diffusion_amd.gaussian_diffusion import SAMPLERS, blur, gaussian_kernel, measure, measure_separable, resize_matrix
from video_diffusion_amd.weights_init import synth_param

pytestmark = pytest.mark.gpu
KEYS = vda.video_model_and_diffusion_defaults().keys()
TINY = dict(T=6, image_size=32, num_channels=32, num_res_blocks=1, rp_alpha=6, rp_beta=6, rp_gamma=6, timestep_respacing="ddim10")
S = 32
P = _lib.ptr
_sds, _keep = {}, []


# ------------------------------------------------------------------------------------------------ engines and inputs
def _fresh(xstart=False, **over):
    """A model of its own: no buffer of its engine has grown yet."""
    cfg = {**vda.video_model_and_diffusion_defaults(), **TINY, "predict_xstart": xstart, **over}
    model, diff = vda.create_video_model_and_diffusion(**{k: cfg[k] for k in KEYS})
    if "tiny" not in _sds:
        _sds["tiny"] = {n: torch.from_numpy(synth_param(n, s)) for n, s in model.param_specs()}
    model.load_state_dict(_sds["tiny"])
    model.to("cuda")
    model.eval()
    diff._bind(model)
    return model, diff


@functools.lru_cache(maxsize=None)
def _engine(role, xstart):
    """The engine of a history ('filled', 'grown', 'leftovers', 'window'), shared by the rows: the more went before, the better."""
    return _fresh(xstart)


@functools.lru_cache(maxsize=None)
def _win(B, T, seed=77):
    """Item 0 observes its first frame, every other frame of the batch is latent (tests/step_compose.py's keys)."""
    g = torch.Generator().manual_seed(seed + 100 * B + T)
    obs = torch.zeros(B, T, 1, 1, 1)
    obs[0, 0] = 1
    x0 = (torch.rand(B, T, 3, S, S, generator=g) * 2 - 1)
    x = 1.5 * torch.randn(B, T, 3, S, S, generator=g)
    return dict(x=x.cuda(), x0=(x0 * obs).cuda(), obs_mask=obs.cuda(), latent_mask=(1 - obs).cuda(), kinda_marg_mask=torch.zeros(B, T, 1, 1, 1).cuda(),
                frame_indices=torch.arange(T).view(1, T).repeat(B, 1).cuda(), xtm1=(x0 * obs).cuda(), full=x0.cuda(),
                noise=torch.randn(B, T, 3, S, S, generator=g).cuda(), noise2=torch.randn(B, T, 3, S, S, generator=g).cuda(),
                cot=torch.randn(B, T, 3, S, S, generator=g).cuda())


@functools.lru_cache(maxsize=None)
def _mwin(B):
    return sc.matrix_window(B, 700 + B)


@functools.lru_cache(maxsize=None)
def _mrest(kind, B):
    return sc.restoration_of(kind, _mwin(B), 800 + B)


def _flags(model):
    """The sticky flags, read and cleared (vd_device_errors without the host mirror's exceptions)."""
    f = ctypes.c_int(0)
    _lib.check(_lib.lib().vd_device_errors(model._handle, ctypes.byref(f)))
    return f.value


def _pstate(model, B, G):
    out = dict(p_logw=torch.empty(B, dtype=torch.float64), p_rprev=torch.empty(B, dtype=torch.float64), p_anc=torch.empty(B, dtype=torch.int32),
               p_chosen=torch.empty(G, dtype=torch.int32), p_ess=torch.empty(G, dtype=torch.float64), p_counters=torch.empty(G, 2, dtype=torch.int64))
    _lib.check(_lib.lib().vd_particle_state(model._handle, B, *(P(out[k]) for k in ("p_logw", "p_rprev", "p_anc", "p_chosen", "p_ess", "p_counters"))))
    return out


def _ws_bytes(model, B, T):
    n = ctypes.c_longlong(0)
    _lib.check(_lib.lib().vd_workspace_bytes(model._handle, B, T, ctypes.byref(n)))
    return n.value


def _raw(t):
    return t.detach().contiguous().cpu().view(torch.uint8)


def _check(got, want, what):
    """Every value of the yardstick's dict, to the bit (NaN payloads included)."""
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k, w in want.items():
        g = got[k]
        if torch.is_tensor(w):
            assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
            if not torch.equal(_raw(g), _raw(w)):
                d = (g.double() - w.double()).abs()
                raise AssertionError((what, k, "elements that differ", int((_raw(g) != _raw(w)).sum()), "max |d|", float(d[torch.isfinite(d)].max()) if torch.isfinite(d).any() else "nan",
                                      "not finite", int((~torch.isfinite(g.double())).sum())))
        else:
            assert g == w, (what, k, g, w)


# ------------------------------------------------------------------------------------------------ the runners: (model, diff) -> dict
def _tb(B, v):
    return torch.tensor([v] * B, device="cuda")


def _hkw(c):
    return dict(x0=c["x0"], obs_mask=c["obs_mask"], latent_mask=c["latent_mask"], kinda_marg_mask=c["kinda_marg_mask"], frame_indices=c["frame_indices"],
                x_t_minus_1=c["xtm1"], observed_frames="x_0")


def run_forward(model, diff, B=2, T=3):
    c = _win(B, T)
    return dict(eps=model(c["x"], torch.tensor([250.0] * B), **_hkw(c))[0])


def run_p_mean_variance(model, diff, B=2, T=3):
    c = _win(B, T)
    out = diff.p_mean_variance(model, c["x"], _tb(B, 5), model_kwargs=_hkw(c))
    return {k: out[k] for k in ("mean", "pred_xstart", "eps")}


def run_psample(model, diff, B=2, T=3):
    """vd_p_sample on the plain window (the long-window and configuration shapes; the grower and the neighbour of the histories)."""
    c = _win(B, T)
    s, x = diff._step(0, model, c["x"], _tb(B, 5), True, None, _hkw(c), 0.0, c["noise"])
    return dict(sample=s, pred_xstart=x)


def run_ddim(model, diff, B=2, T=3):
    c = _win(B, T)
    s, x = diff._step(1, model, c["x"], _tb(B, 4), True, None, _hkw(c), 0.5, c["noise"])
    return dict(sample=s, pred_xstart=x)


def run_step(case, model, diff):
    """The row's sampler inside the row's scopes, at the middle of the schedule, with the carry of a chain in flight."""
    name, _ = sm.SAMPLER[case.sampler]
    row = SAMPLERS[name]
    B = sm.batch(case)
    c, R = _mwin(B), _mrest(case.restoration, B)
    x = c["x"]
    g = torch.Generator().manual_seed(31)
    noise, z = torch.randn(x.shape, generator=g).cuda(), torch.randn(x.shape, generator=g).cuda()
    u = torch.tensor([[0.37, 0.61], [0.83, 0.12]], dtype=torch.float64)
    carry = None
    if row.carry == "prev_xstart":
        carry = (0.3 * x).clamp(-1, 1)
    elif row.carry == "state":
        carry = ((0.9 * x).contiguous(), (0.3 * x).clamp(-1, 1), (-0.2 * x).clamp(-1, 1), 2)
    with sc.model_scopes(diff, model, case), sc.restoration_scope(diff, model, R, known_noise=z, uniforms=lambda tt: u):
        out = sc.fused_step(diff, model, case, x, _tb(B, diff.num_timesteps // 2), sc._kw(c), noise=noise, carry=carry)
    res = {k: v for k, v in out.items() if torch.is_tensor(v)}
    if out.get("state") is not None:
        res.update(base=out["state"][0], d1=out["state"][1], d2=out["state"][2], count=out["state"][3])
    if sm.particles(case):
        res.update(_pstate(model, B, B // sm.PARTICLES))
    return res


def run_from_xstart(name, model, diff):
    c = _win(2, 3)
    x = c["x"]
    state = ((0.9 * x).contiguous(), (0.3 * x).clamp(-1, 1), (-0.2 * x).clamp(-1, 1), 2) if name == "unipc" else None
    prev = (0.3 * x).clamp(-1, 1) if name in ("dpmpp_2m", "dpmpp_2m_sde") else None
    s, xs, new, mean = sc.from_xstart(model, name, x, c["full"].contiguous(), _tb(2, 4), True, 0.5 if name == "ddim" else 0.0, c["noise"], prev, state)
    res = dict(sample=s, pred_xstart=xs)
    if mean is not None:
        res["mean"] = mean
    if new is not None:
        res.update(base=new[0], d1=new[1], d2=new[2])
    return res


def run_posterior_update(model, diff):
    c = _win(2, 3)
    x, per = c["x"], c["x"][0].numel()
    s, xs = torch.empty_like(x), torch.empty_like(x)
    _lib.check(_lib.lib().vd_posterior_update(model._handle, 0, 2, per, P(x), P(c["cot"]), P(_tb(2, 4)), 1, 0.0, P(c["noise"]), 0, 0, P(s), P(xs), _lib.current_stream()))
    return dict(sample=s, pred_xstart=xs)


def run_q_sample(model, diff):
    c = _win(2, 3)
    return dict(x_t=diff.q_sample(c["full"], _tb(2, 6), c["noise"], model))


def run_q_jump(model, diff):
    c = _win(2, 3)
    return dict(x_t=diff.q_jump(c["x"], _tb(2, 6), c["latent_mask"], c["noise"], model))


def run_known_merge(model, diff):
    c = _win(2, 3)
    sample = c["x"].clone()
    mask = (c["noise2"][:, :, 0] > 0).float().contiguous()
    _lib.check(_lib.lib().vd_known_merge(model._handle, 2, 3, S * S, P(sample), P(c["full"]), P(mask), P(c["latent_mask"].reshape(-1).contiguous()), P(_tb(2, 4)),
                                         P(c["noise"]), 0, 0, _lib.current_stream()))
    return dict(sample=sample)


def run_measurement_project(model, diff):
    c = _win(2, 3)
    return dict(x0=sc._project(model, c["x"].clamp(-1, 1), measure(c["full"].cpu(), 2, False), c["latent_mask"].reshape(2, 3), 2, False))


@functools.lru_cache(maxsize=None)
def _linear():
    from video_diffusion_amd.gaussian_diffusion import check_separable_operator, separable_pinv
    A = resize_matrix(S, S // 2)
    a_h, a_w = check_separable_operator(A, A)
    return A, [m.cuda().contiguous() for m in (a_h, a_w, separable_pinv(a_h, 1e-3)[0], separable_pinv(a_w, 1e-3)[0])]


def run_linear_project(model, diff):
    c = _win(2, 3)
    A, mats = _linear()
    y = measure_separable(c["full"].cpu(), A, A).cuda().contiguous()
    x0 = c["x"].clamp(-1, 1).contiguous()
    _lib.check(_lib.lib().vd_op_linear_project(model._handle, 2, 3, S, S, P(x0), P(y), P(c["latent_mask"].reshape(-1).contiguous()), P(mats[0]), mats[0].shape[0],
                                               P(mats[1]), mats[1].shape[0], P(mats[2]), P(mats[3]), 0, _lib.current_stream()))
    return dict(x0=x0)


def run_vb_terms(model, diff):
    c = _win(2, 3)
    out = diff._vb_terms_bpd(model, c["full"], c["x"], torch.tensor([0, 5], device="cuda"), model_kwargs=_hkw(c), latent_mask=c["latent_mask"], _noise=c["noise"])
    return dict(vb=out["output"], xstart_mse=out["xstart_mse"], mse=out["mse"], pred_xstart=out["pred_xstart"])


def run_prior_bpd(model, diff):
    c = _win(2, 3)
    return dict(bpd=diff._prior_bpd(c["full"], c["latent_mask"], model))


def run_score_windows(model, diff):
    c = _win(2, 3)
    kw = {k: v for k, v in _hkw(c).items() if k not in ("x0", "x_t_minus_1", "observed_frames")}
    a = diff.score_windows(model, c["full"], _tb(2, 5), kw, None, 99, [0, 1 << 20], suffix_skip=False)
    b = diff.score_windows(model, c["full"], _tb(2, 5), kw, None, 99, [0, 1 << 20], suffix_skip=True)
    return dict(mse=a, mse_skip=b)


def run_eps_mse(model, diff):
    c = _win(2, 3)
    out = torch.empty(2, dtype=torch.float64, device="cuda")
    off = torch.tensor([0, 1 << 20], dtype=torch.int64, device="cuda")
    _lib.check(_lib.lib().vd_op_eps_mse(model._handle, 2, 3, P(c["full"]), P(c["cot"]), P(_tb(2, 5)), 1, P(c["latent_mask"].reshape(-1).contiguous()), 99, P(off),
                                        None, P(out), _lib.current_stream()))
    return dict(mse=out)


def run_guided_step(model, diff):
    c = _win(2, 3)
    out = diff._guided(model, c["x"], _tb(2, 5), True, _hkw(c), noise2=c["noise2"], want_sample=True, _noise=c["noise"])
    return {k: out[k] for k in ("mean", "pred_xstart", "grad", "sample")}


def run_guided_grad(model, diff):
    c = _win(2, 3)
    per = c["x"][0].numel()
    f = lambda k: c[k].reshape(2, per).contiguous()                              # noqa: E731
    obs = c["obs_mask"].reshape(2, 3).contiguous()
    out = {k: torch.empty(2, per, device="cuda") for k in ("deps", "dxd", "mean", "xstart")}
    _lib.check(_lib.lib().vd_op_guided_grad(model._handle, 2, 3, per, P(f("x")), P(f("cot")), P(f("noise")), P(f("full")), P(obs), P(_tb(2, 5)), 1, P(out["deps"]),
                                            P(out["dxd"]), P(out["mean"]), P(out["xstart"]), _lib.current_stream()))
    return out


def run_guided_final(model, diff):
    c = _win(2, 3)
    per = c["x"][0].numel()
    f = lambda k: c[k].reshape(2, per).contiguous()                              # noqa: E731
    gs = torch.tensor([0.5, 2.0, 0.0, 0.0], device="cuda")
    out = {k: torch.empty(2, per, device="cuda") for k in ("grad", "mean_out", "sample")}
    _lib.check(_lib.lib().vd_op_guided_final(model._handle, 2, 3, per, P(_tb(2, 5)), P(f("x")), P(f("full")), P(f("cot")), P(gs), P(f("noise")), P(out["grad"]),
                                             P(out["mean_out"]), P(out["sample"]), _lib.current_stream()))
    return out


def _moved(model, diff, scope):
    """A p_sample step inside one of the scopes that move the latent frames down a gradient."""
    c = _win(2, 3)
    with scope:
        s, x = diff._step(0, model, c["x"], _tb(2, 5), True, None, _hkw(c), 0.0, c["noise"])
        extra = diff._dps_extras()
    return dict(sample=s, pred_xstart=x, **{k: v for k, v in extra.items() if torch.is_tensor(v)})


def run_dps_step(model, diff):
    return _moved(model, diff, diff.dps_scope(model, measure(_win(2, 3)["full"].cpu(), 2, False), 2, False, zeta=0.5))


def run_deblur_step(model, diff):
    w = gaussian_kernel(5, 1.2)
    return _moved(model, diff, diff.deblur_scope(model, blur(_win(2, 3)["full"].cpu(), w), w, zeta=0.5))


def run_linear_dps_step(model, diff):
    A = _linear()[0]
    return _moved(model, diff, diff.linear_dps_scope(model, measure_separable(_win(2, 3)["full"].cpu(), A, A), A, A, zeta=0.5))


def run_loss_guidance(model, diff):
    cot = _win(2, 3)["cot"]
    return _moved(model, diff, diff.loss_guidance_scope(model, cotangent_fn=lambda x0, t: (x0 - 0.1 * cot).contiguous(), scale=0.3, normalize=True))


def _seed_out(c):
    return [torch.empty_like(c["x"]) for _ in range(3)], torch.empty(2, device="cuda")


def run_dps_seed(model, diff):
    c = _win(2, 3)
    y = measure(c["full"].cpu(), 2, False).cuda().contiguous()
    o, rho = _seed_out(c)
    _lib.check(_lib.lib().vd_op_dps_seed(model._handle, 2, 3, S, S, P(c["x"]), P(c["cot"]), P(_tb(2, 5)), 1, P(y), P(c["latent_mask"].reshape(-1).contiguous()), 2, 0,
                                         P(o[0]), P(o[1]), P(rho), P(o[2]), _lib.current_stream()))
    return dict(deps=o[0], dxd=o[1], rho=rho, xstart=o[2])


def run_deblur_seed(model, diff):
    c = _win(2, 3)
    w = gaussian_kernel(5, 1.2)
    y, wd = blur(c["full"].cpu(), w).cuda().contiguous(), w.float().cuda().contiguous()
    o, rho = _seed_out(c)
    _lib.check(_lib.lib().vd_op_deblur_seed(model._handle, 2, 3, S, S, P(c["x"]), P(c["cot"]), P(_tb(2, 5)), 1, P(y), P(c["latent_mask"].reshape(-1).contiguous()), P(wd), 5,
                                            P(o[0]), P(o[1]), P(rho), P(o[2]), _lib.current_stream()))
    return dict(deps=o[0], dxd=o[1], rho=rho, xstart=o[2])


def run_linear_dps_seed(model, diff):
    c = _win(2, 3)
    A, mats = _linear()
    y = measure_separable(c["full"].cpu(), A, A).cuda().contiguous()
    o, rho = _seed_out(c)
    _lib.check(_lib.lib().vd_op_linear_dps_seed(model._handle, 2, 3, S, S, P(c["x"]), P(c["cot"]), P(_tb(2, 5)), 1, P(y), P(c["latent_mask"].reshape(-1).contiguous()),
                                                P(mats[0]), mats[0].shape[0], P(mats[1]), mats[1].shape[0], P(o[0]), P(o[1]), P(rho), P(o[2]), _lib.current_stream()))
    return dict(deps=o[0], dxd=o[1], rho=rho, xstart=o[2])


def run_guide_seed(model, diff):
    c = _win(2, 3)
    o = [torch.empty_like(c["x"]) for _ in range(2)]
    _lib.check(_lib.lib().vd_op_guide_seed(model._handle, 2, 3, S, S, P(c["x"]), P(c["cot"]), P(_tb(2, 5)), 1, P(c["noise"]), P(c["latent_mask"].reshape(-1).contiguous()),
                                           P(o[0]), P(o[1]), _lib.current_stream()))
    return dict(deps=o[0], dxd=o[1])


def run_eps_vjp(model, diff, B=2, T=3):
    c = _win(B, T)
    return diff.eps_vjp(model, c["x"], _tb(B, 5), c["cot"], _hkw(c))


def run_ode_nll_eval(model, diff):
    c = _win(2, 3)
    base, xs, tt, kw = diff._vjp_window(model, c["x"], _tb(2, 5), _hkw(c), what="ode_nll_loop")
    off = torch.tensor([0, 1 << 20], dtype=torch.int64, device="cuda")
    eps, tr, nxt = diff._ode_eval(base, xs, tt, kw, 2, 99, off, 0, None, True)
    return dict(eps=eps, trace=tr, x_next=nxt)


def run_ode_heun(model, diff):
    c = _win(2, 3)
    out = torch.empty_like(c["x"])
    _lib.check(_lib.lib().vd_op_ode_heun(model._handle, 2, 3, 3 * S * S, P(c["x"]), P(c["cot"]), P(c["noise"]), P(_tb(2, 5)), P(c["latent_mask"].reshape(-1).contiguous()),
                                         P(out), _lib.current_stream()))
    return dict(x_next=out)


def run_particle_apply(model, diff):
    """A p_sample step of two groups of two particles under a caller's reward: vd_particle_apply weights, resamples and gathers."""
    c = _mwin(4)
    u = torch.tensor([[0.37, 0.61], [0.83, 0.12]], dtype=torch.float64)
    noise = torch.randn(c["x"].shape, generator=torch.Generator().manual_seed(32)).cuda()
    reward = lambda x0, t: -(x0.double() ** 2).flatten(1).mean(1) * 40.0         # noqa: E731
    with diff.steering_scope(model, reward, particles=2, scale=1.0, ess_threshold=1.0, uniforms=lambda tt: u):
        s, x = diff._step(0, model, c["x"], _tb(4, 5), True, None, sc._kw(c), 0.0, noise)
        extra = diff._last_steer
    return dict(sample=s, pred_xstart=x, ancestors=extra["ancestors"], log_weights=extra["log_weights"], ess=extra["ess"], **_pstate(model, 4, 2))


RUNNERS = dict(forward=run_forward, p_mean_variance=run_p_mean_variance, posterior_update=run_posterior_update, q_sample=run_q_sample, q_jump=run_q_jump,
               known_merge=run_known_merge, measurement_project=run_measurement_project, linear_project=run_linear_project, vb_terms=run_vb_terms,
               prior_bpd=run_prior_bpd, score_windows=run_score_windows, eps_mse=run_eps_mse, guided_step=run_guided_step, guided_grad=run_guided_grad,
               guided_final=run_guided_final, dps_step=run_dps_step, dps_seed=run_dps_seed, deblur_step=run_deblur_step, deblur_seed=run_deblur_seed,
               linear_dps_step=run_linear_dps_step, linear_dps_seed=run_linear_dps_seed, loss_guidance=run_loss_guidance, guide_seed=run_guide_seed,
               eps_vjp=run_eps_vjp, ode_nll_eval=run_ode_nll_eval, ode_heun=run_ode_heun, particle_apply=run_particle_apply)
FROM_XSTART = {"vd_posterior_from_xstart": "p_sample", "vd_ddim_reverse_from_xstart": "ddim_reverse", "vd_dpmpp_2m_from_xstart": "dpmpp_2m",
               "vd_dpmpp_2m_sde_from_xstart": "dpmpp_2m_sde", "vd_unipc_from_xstart": "unipc"}
Job = __import__("collections").namedtuple("Job", "id entry fn xstart shape")


def _jobs():
    jobs = []
    for entry, row in sk.ENTRIES.items():
        if row.run in ("window", "window_jump"):
            continue                                                             # the window tests below
        if row.run == "step":
            for case in sk.STEP_ROWS:
                if sk.entry_of(case) == entry:
                    jobs.append(Job(f"{entry}:{sm.case_id(case)}", entry, functools.partial(run_step, case), case.model == "xstart", (sm.batch(case), sc.T_)))
        elif row.run == "from_xstart":
            jobs.append(Job(entry, entry, functools.partial(run_from_xstart, FROM_XSTART[entry]), False, sk.SHAPE))
        elif entry == "vd_guide_finish":
            continue                                                             # vd_guide_begin's job is the whole loss-guided step: both entries
        else:
            name = "vd_guide_begin+vd_guide_finish" if entry == "vd_guide_begin" else entry
            jobs.append(Job(name, entry, RUNNERS[row.run], False, (4, sc.T_) if row.run == "particle_apply" else sk.SHAPE))
    return jobs


JOBS = _jobs()
_yard = {}


def _yardstick(job):
    """The row on a freshly created engine (once per row; the engine is dropped)."""
    if job.id not in _yard:
        model, diff = _fresh(job.xstart)
        out = job.fn(model, diff)
        out["flags"] = _flags(model)
        row = sk.ENTRIES[job.entry]
        assert set(row.outputs) <= set(out), (job.id, "the row names an output the runner does not return", row.outputs, sorted(out))
        assert out["flags"] == 0, (job.id, out["flags"])
        for k in row.outputs:
            assert torch.isfinite(out[k].double()).all(), (job.id, k, "the yardstick itself is not finite")
        _yard[job.id] = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items()}
    return _yard[job.id]


def _run(job, model, diff, what):
    out = job.fn(model, diff)
    out["flags"] = _flags(model)
    _check(out, _yardstick(job), (job.id, what))


def _neighbour(job, model, diff):
    """A call of a different entry at the row's shape."""
    B, T = job.shape
    (run_p_mean_variance if job.entry == "vd_ddim_sample" else run_ddim)(model, diff, B, T)


def _grown_shape(job):
    """B = 3, T = 7; one item more than the row's where the row has four (the steered rows)."""
    return sk.GROWN_SHAPE if job.shape[0] < sk.GROWN_SHAPE[0] else (job.shape[0] + 1, sk.GROWN_SHAPE[1])


def _grow(job, model, diff):
    """A larger call of another entry: one that lays DiffWs over the workspace when the row does not, and the reverse."""
    B, T = _grown_shape(job)
    if sk.ENTRIES[job.entry].diffws or job.xstart:                               # (the differentiated passes serve epsilon models only)
        run_psample(model, diff, B, T)
    else:
        run_eps_vjp(model, diff, B, T)


def _refused(model):
    """A call refused in front of any launch: a window beyond vd_max_window_frames."""
    c = _win(2, 3)
    L = _lib.lib()
    k = model._pack_kwargs(c["x"], _hkw(c))
    rc = L.vd_p_sample(model._handle, 2, L.vd_max_window_frames() + 1, *model._window_ptrs(c["x"], k), P(_tb(2, 5)), 0, 1, P(c["noise"]), 0, 0, P(torch.empty_like(c["x"])),
                       None, None, _lib.current_stream())
    assert rc != 0 and str(L.vd_max_window_frames()).encode() in L.vd_last_error(), L.vd_last_error()


def _poisoned(model, diff, B, T):
    """A step whose item 0 carries a t outside the table: poisoned alone, the sticky flag read and cleared."""
    c = _win(B, T)
    t = torch.tensor([diff.num_timesteps + 5] + [1] * (B - 1), device="cuda")
    s, _ = diff._step(0, model, c["x"], t, True, None, _hkw(c), 0.0, c["noise"])
    assert torch.isnan(s[0]).all() and torch.isfinite(s[1:]).all()
    assert _flags(model) & 1
    assert _flags(model) == 0


# ------------------------------------------------------------------------------------------------ histories 1 to 3, one test per row
@pytest.mark.parametrize("history,job", [(h, j) for h in sk.HISTORIES for j in JOBS], ids=[f"{h}-{j.id}" for h in sk.HISTORIES for j in JOBS])
def test_row(history, job):
    """Every row in place behind the fills (zeros first, for every row, before anything harsher runs), then behind a larger call, then
    behind natural leftovers."""
    want = _yardstick(job)
    model, diff = _engine(history, job.xstart)
    B, T = job.shape
    if history == "filled":
        _run(job, model, diff, "the engine as the rows before left it")          # every buffer the row needs exists
        for byte in sk.FILLS:
            n = model.scratch_fill(byte)
            assert n > 0 and n >= _ws_bytes(model, B, T), (job.id, byte, n, _ws_bytes(model, B, T))
            _run(job, model, diff, f"filled with 0x{byte:02X}")
    elif history == "grown":
        _grow(job, model, diff)
        assert _flags(model) == 0
        n = model.scratch_fill(0xFF)
        assert n >= _ws_bytes(model, *_grown_shape(job)) > _ws_bytes(model, B, T), (job.id, n)
        _run(job, model, diff, "behind a larger call of another entry, filled with 0xFF")
    else:
        _refused(model)
        _run(job, model, diff, "behind a refused call")
        _poisoned(model, diff, B, T)
        _run(job, model, diff, "behind a poisoned item")
        _neighbour(job, model, diff)
        assert _flags(model) == 0
        _run(job, model, diff, "behind another entry at the same shape")
    assert want["flags"] == 0


def test_the_fill_reports_what_it_wrote_and_leaves_addresses_and_state_alone():
    """On an engine that has not run: 0 bytes.  Behind a step: at least the workspace of the shape; a second fill writes the same bytes
    (nothing grew); the flags, the schedule and the weights are as they were (the next step's bits are the yardstick's -- test_row)."""
    model, diff = _fresh()
    assert model.scratch_fill(0xFF) == 0
    run_psample(model, diff)
    n = model.scratch_fill(0xFF)
    assert n >= _ws_bytes(model, 2, 3) > 0 and model.scratch_fill(0x00) == n
    with pytest.raises(_lib.VdError, match="byte 0..255"):
        model.scratch_fill(256)
    assert _flags(model) == 0


# ------------------------------------------------------------------------------------------------ shapes TINY at (2, 3) does not reach
LONG = dict(forward=run_forward, p_sample=run_psample)


@pytest.mark.parametrize("what", sorted(LONG))
def test_the_first_long_window(what):
    """B = 1, T = 33: the first window on the long-form temporal attention and GroupNorm kernels, which have scratch of their own."""
    B, T = sk.LONG_SHAPE
    fn = LONG[what]
    ym, yd = _fresh()
    want = fn(ym, yd, B, T)
    assert _flags(ym) == 0 and all(torch.isfinite(v).all() for v in want.values())
    model, diff = _engine("long", False)
    _check(fn(model, diff, B, T), want, (what, "first"))
    for byte in sk.FILLS:
        assert model.scratch_fill(byte) >= _ws_bytes(model, B, T)
        _check(fn(model, diff, B, T), want, (what, f"filled with 0x{byte:02X}"))
    run_eps_vjp(model, diff, 2, 8)                                                # DiffWs's tail over the long window's arena
    model.scratch_fill(0xFF)
    _check(fn(model, diff, B, T), want, (what, "behind a differentiated pass, filled with 0xFF"))
    assert _flags(model) == 0


def _config_models(tag):
    """A freshly created engine of the configuration, and the one tests/test_gpu_config_sweep.py keeps (whatever that file ran on it)."""
    import config_sweep_cases as cs
    from helpers import synth_sd
    from test_gpu_config_sweep import engine
    used = engine(tag)
    cfg = dict(cs.case(tag)["cfg"])
    model, diff = vda.create_video_model_and_diffusion(**{k: cfg[k] for k in KEYS})
    model.load_state_dict(synth_sd(model.param_specs()))
    model.to("cuda")
    model.eval()
    for m, d in ((model, diff), used):
        d._bind(m)
    return ((model, diff), used), cs.case(tag)


def _config_runs(k, model, diff):
    """Forward, p_sample and eps_vjp on the configuration's stored inputs."""
    c, t = {a: v.cuda() for a, v in k["c"].items()}, k["t"]
    B = c["x"].shape[0]
    kw = dict(frame_indices=c["frame_indices"], x0=c["x0"], obs_mask=c["obs_mask"], latent_mask=c["latent_mask"], kinda_marg_mask=c["kinda_marg_mask"],
              x_t_minus_1=c["x0"], observed_frames="x_0")
    g = torch.Generator().manual_seed(5)
    noise, cot = torch.randn(c["x"].shape, generator=g).cuda(), torch.randn(c["x"].shape, generator=g).cuda()
    tt = torch.full((B,), diff.num_timesteps // 2, device="cuda")
    out = dict(eps=diff._wrap_model(model)(c["x"], t.cuda(), **kw)[0])
    s, x = diff._step(0, model, c["x"], tt, True, None, kw, 0.0, noise)
    out.update(sample=s, pred_xstart=x)
    try:
        v = diff.eps_vjp(model, c["x"], t.cuda(), cot, kw)
        out.update(vjp=v["vjp"], vjp_eps=v["eps"])
    except _lib.VdError as exc:                                                  # refused by name: the same refusal every time (test_configuration says which configurations must serve it)
        out["vjp_refused"] = str(exc)
    out["flags"] = _flags(model)
    return out


def _served_tags():
    import config_sweep_cases as cs
    return cs.SERVED


@pytest.mark.parametrize("tag", _served_tags())
def test_configuration(tag):
    """The nine served configurations of the sweep, whose kernel selection TINY does not reach: generic and Winograd convs alternating at
    96 and 160 channels, the r64, z128 and Upsample Winograd kernels at 64 x 64 and 128 x 128, the three forms of the temporal
    GroupNorm, 1024-token spatial attention, the 1024-channel concat."""
    ((ym, yd), (model, diff)), k = _config_models(tag)
    want = _config_runs(k, ym, yd)
    assert want["flags"] == 0 and all(torch.isfinite(v).all() for v in want.values() if torch.is_tensor(v))
    print(f"SCRATCH_CONFIG | {tag} | eps_vjp {'refused: ' + want['vjp_refused'] if 'vjp_refused' in want else 'served'}")
    if _lib.lib().vd_math_mode() != 2:                                           # every served configuration serves the backward-data pass ...
        assert "vjp" in want and "vjp_refused" not in want, (tag, want.get("vjp_refused"))
    else:                                                                        # ... but VD_MATH=fp32 serves no differentiated pass, and says so
        assert "split arithmetic only" in want.get("vjp_refused", ""), (tag, sorted(want))
    del ym, yd
    _check(_config_runs(k, model, diff), want, (tag, "first"))
    B, T = k["c"]["x"].shape[:2]
    for byte in sk.FILLS:
        assert model.scratch_fill(byte) >= _ws_bytes(model, B, T) > 0
        _check(_config_runs(k, model, diff), want, (tag, f"filled with 0x{byte:02X}"))


# ------------------------------------------------------------------------------------------------ history 4: windows
STEPS = 3


def _begin(ex, diff, model, case, seed):
    name, eta = sm.SAMPLER[case.sampler]
    B = sm.batch(case)
    c, R = _mwin(B), _mrest(case.restoration, B)
    with sc.model_scopes(diff, model, case), sc.restoration_scope(diff, model, R):
        ex.begin(c["x"], sc._kw(c), t_start=0 if SAMPLERS[name].up else STEPS - 1, seed=seed, sampler=name, eta=eta, renoise=False,
                 cfg_scale=sm.GUIDANCE[case.guidance][0])


def _window_trace(model, diff, case, fill):
    """begin, then STEPS runs of one step; `fill`: the byte set between begin and the first run and between every two runs, or None
    -> per step (x, history, particle state), and the graph count and generation at the end."""
    name, _ = sm.SAMPLER[case.sampler]
    B = sm.batch(case)
    ex = WindowExecutor(model, diff, prefix_cache=case.switch == "prefix_cache", suffix_skip=case.switch == "suffix_skip")
    _keep.append(ex)
    _begin(ex, diff, model, case, 4321)
    graphs, gen = ex.graphs, int(_lib.lib().vd_window_generation(model._handle))
    trace = []
    for k in range(STEPS):
        if fill is not None:
            assert model.scratch_fill(fill) >= _ws_bytes(model, B, sc.T_)
            assert (ex.graphs, int(_lib.lib().vd_window_generation(model._handle))) == (graphs, gen), "the fill dropped a graph or moved the generation"
        x = ex.run(1).clone()
        hist = sc.window_history(ex, name, B)
        d = dict(x=x)
        if hist is not None:
            d.update({f"hist{j}": h for j, h in enumerate(hist) if h is not None})
        if sm.particles(case):
            d.update({f"p_{a}": v for a, v in ex.particle_state().items()})
        trace.append(d)
    assert (ex.graphs, int(_lib.lib().vd_window_generation(model._handle))) == (graphs, gen)
    return trace, _flags(model)


@pytest.mark.parametrize("case", sk.WINDOW_ROWS, ids=[sm.case_id(c) for c in sk.WINDOW_ROWS])
def test_window(case):
    """The fill between vd_window_begin and the first vd_window_run, and between two vd_window_runs of one window: the replay of the
    captured graph on filled scratch equals the same window on a fresh engine, step by step -- the window tensor, the carried history
    (vd_window_history), the particle state -- and neither the graph count nor the generation moves.  Under the suffix skip the purely
    observed frames' entries are meaningless and not compared."""
    B = sm.batch(case)
    c = _mwin(B)
    read = torch.ones(B, sc.T_, dtype=torch.bool, device="cuda")
    if case.switch == "suffix_skip":
        read = ~((c["obs_mask"].reshape(B, -1) == 1) & (c["latent_mask"].reshape(B, -1) == 0))
    pick = lambda tr: [{k: (v[read] if torch.is_tensor(v) and v.shape[:2] == read.shape and v.is_cuda else v) for k, v in d.items()} for d in tr]   # noqa: E731
    want, wflags = _window_trace(*_fresh(case.model == "xstart"), case, None)
    assert wflags == 0 and all(torch.isfinite(d["x"]).all() for d in pick(want))
    model, diff = _engine("window", case.model == "xstart")
    for byte in sk.FILLS:
        got, flags = _window_trace(model, diff, case, byte)
        assert flags == 0
        for k, (g, w) in enumerate(zip(pick(got), pick(want))):
            _check(g, w, (sm.case_id(case), f"filled with 0x{byte:02X}", "step", k))


def test_window_jump_on_filled_scratch():
    """vd_window_jump between two runs of a window with a known region, the fill in front of the jump and behind it."""
    case = sm.Case("p_sample", "eps", "off", "off", "known", "none")

    def walk(model, diff, fill):
        ex = WindowExecutor(model, diff)
        _keep.append(ex)
        _begin(ex, diff, model, case, 99)
        out = []
        for op in ("run", "jump", "run", "run"):
            if fill is not None:
                model.scratch_fill(fill)
            out.append((ex.run(1) if op == "run" else ex.jump(1)).clone())
        return out, _flags(model)
    want, wf = walk(*_fresh(), None)
    model, diff = _engine("window", False)
    for byte in sk.FILLS:
        got, f = walk(model, diff, byte)
        assert f == wf == 0
        for k, (g, w) in enumerate(zip(got, want)):
            _check(dict(x=g), dict(x=w), ("jump", byte, k))


# ------------------------------------------------------------------------------------------------ history 5: the held pass
def test_a_fill_ends_the_held_pass_by_name():
    """vd_guide_begin, the fill, vd_guide_finish: the tape and the eps of the held pass lay in the workspace, so the finish is refused
    by the stale-ticket message, with the fill's own reason; the engine is good for the next step."""
    model, diff = _engine("filled", False)
    c = _win(2, 3)

    def overwritten(x0, t):
        assert model.scratch_fill(0xFF) > 0
        return torch.zeros_like(x0)
    with pytest.raises(_lib.VdError, match=r"no taped pass is held for this ticket \(dropped by vd_scratch_fill"):
        with diff.loss_guidance_scope(model, cotangent_fn=overwritten, scale=0.3):
            diff._step(0, model, c["x"], _tb(2, 5), True, None, _hkw(c), 0.0, c["noise"])
    job = next(j for j in JOBS if j.entry == "vd_guide_begin")
    _run(job, model, diff, "behind a held pass the fill ended")


# ------------------------------------------------------------------------------------------------ the evaluator handles
def _eval_fill(name, handle=None):
    n = ctypes.c_longlong(0)
    args = ([handle] if handle is not None else []) + [0, ctypes.byref(n)]

    def fill(byte):
        args[-2] = byte
        _lib.check(getattr(_lib.lib(), name)(*args))
        return n.value
    return fill


def _evaluator(make, run, small, large, fill_name):
    """`run(handle, inputs)` behind each fill and behind a larger call of the same handle, against a fresh handle."""
    want = run(make(), small)
    assert torch.isfinite(want.double()).all()
    h = make()
    fill = _eval_fill(fill_name, getattr(h, "_h", None))
    assert fill(0xFF) == 0 or fill_name == "vd_frame_metrics_scratch_fill"      # a handle that has not run owns no workspace
    _check(dict(out=run(h, small)), dict(out=want), (fill_name, "first"))
    for byte in sk.FILLS:
        assert fill(byte) > 0
        _check(dict(out=run(h, small)), dict(out=want), (fill_name, f"filled with 0x{byte:02X}"))
    run(h, large)
    n = fill(0xFF)
    _check(dict(out=run(h, small)), dict(out=want), (fill_name, "behind a larger call, filled with 0xFF"))
    assert fill(0x00) == n


def test_lpips_embed_on_filled_scratch():
    """Two 64 x 192 frames; the larger call: five 96 x 224 frames."""
    from lpips_restated import synth_weights
    from test_gpu_lpips import _state_dict
    from video_diffusion_amd.lpips import LpipsAlex
    g = torch.Generator().manual_seed(3)
    small, large = (torch.rand(2, 3, 64, 192, generator=g) * 2 - 1).cuda(), (torch.rand(5, 3, 96, 224, generator=g) * 2 - 1).cuda()
    _evaluator(lambda: LpipsAlex.from_state_dict(_state_dict(synth_weights(0)), "cuda:0"), lambda h, v: h._embed_device(v), small, large, "vd_lpips_scratch_fill")


def test_i3d_embed_on_filled_scratch():
    """One 9-frame 32 x 32 video; the larger call: one of 17 frames."""
    import i3d_restated as ir
    from video_diffusion_amd import fvd
    sd = ir.synth_state_dict(0)
    g = torch.Generator().manual_seed(4)
    small, large = torch.randint(0, 256, (1, 9, 3, 32, 32), generator=g, dtype=torch.uint8).cuda(), torch.randint(0, 256, (1, 17, 3, 32, 32), generator=g, dtype=torch.uint8).cuda()
    _evaluator(lambda: fvd.I3D.from_state_dict(sd, "cuda:0"), lambda h, v: torch.as_tensor(h.embed(v)), small, large, "vd_i3d_scratch_fill")


@pytest.mark.parametrize("H,W", [(40, 48), (60, 263)])
def test_frame_metrics_on_filled_scratch(H, W):
    """One narrow shape and W = 263 of tests/eval_regime_cases.py (threads that walk two columns, a short last strip); the table is the
    library's, one per device: the yardstick is the call behind a fill with zeros, which is what a first call finds."""
    import eval_regime_cases as er
    from video_diffusion_amd.metrics import frame_ssim_psnr_device
    assert (H, W) in er.WIDE_CASES or W < 240
    g = torch.Generator().manual_seed(H + W)
    gt, pred = torch.rand(3, 2, H, W, generator=g).cuda(), torch.rand(3, 2, H, W, generator=g).cuda()
    big = torch.rand(9, 3, H + 16, W, generator=g).cuda()
    run = lambda: torch.stack(frame_ssim_psnr_device(gt, pred))                  # noqa: E731
    fill = _eval_fill("vd_frame_metrics_scratch_fill")
    first = run()
    assert fill(0x00) > 0
    want = run()
    _check(dict(out=first), dict(out=want), ("metrics", "as it was found"))
    assert torch.isfinite(want).all()
    for byte in sk.FILLS:
        assert fill(byte) > 0
        _check(dict(out=run()), dict(out=want), ("metrics", f"filled with 0x{byte:02X}"))
    frame_ssim_psnr_device(big, big.clone())
    n = fill(0xFF)
    _check(dict(out=run()), dict(out=want), ("metrics", "behind a larger call, filled with 0xFF"))
    assert fill(0x7F) == n
