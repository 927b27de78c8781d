"""GPU: dpmpp_2m_sample (this project's extension: DPM-Solver++(2M), the second-order multistep sampler) -- the fused pass, the step
on the network, its loops, its window graph and infer_video -- against the float64 restatement of the pass and the analytic model
(tests/dpmpp_2m_restated.py; the reference has no such sampler, so there is no fixture) and against itself (mixed t, executor vs
eager calls)."""
import json

import numpy as np
import pytest
import torch

import video_diffusion_amd as vda
from dpmpp_2m_restated import denoiser_coef, order_conditions, rel_err, rounding_bound, start, step_fp64, tables
from helpers import ATOL, RTOL, close, load_npz, synth_sd
from video_diffusion_amd import _lib
from video_diffusion_amd.executor import WindowExecutor
from video_diffusion_amd.script_util import create_gaussian_diffusion

pytestmark = pytest.mark.gpu
KEYS = vda.video_model_and_diffusion_defaults().keys()
_cache = {}
TINY = dict(T=6, image_size=32, num_channels=64, num_res_blocks=1, rp_alpha=6, rp_beta=6, rp_gamma=6, timestep_respacing="logsnr10")
PER = 1152                                          # the pass alone: B = 2 items of 1152 floats, 576 groups of four in 3 blocks


def engine(cfg):
    key = json.dumps(cfg, sort_keys=True)
    if key not in _cache:
        model, diff = vda.create_video_model_and_diffusion(**{k: cfg[k] for k in KEYS})
        model.load_state_dict(synth_sd(model.param_specs()))
        model.to("cuda")
        model.eval()
        _cache[key] = (model, diff)
    return _cache[key]


def tiny(**over):
    return engine({**vda.video_model_and_diffusion_defaults(), **TINY, **over})


def _denoised_fn(x):
    return 1.3 * torch.tanh(1.5 * x) + 0.05


def _rand_window(B, T, S, n_obs, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(B, T, 3, S, S, generator=g) * 2 - 1
    x0[:, n_obs:] = 0
    x = torch.randn(B, T, 3, S, S, generator=g)
    obs = torch.zeros(B, T, 1, 1, 1)
    obs[:, :n_obs] = 1
    return dict(x=x, x0=x0, obs_mask=obs, latent_mask=1 - obs, kinda_marg_mask=torch.zeros(B, T, 1, 1, 1),
                frame_indices=torch.arange(T).view(1, T).repeat(B, 1))


def _window_kw(c, observed_frames="x_0"):
    d = {k: c[k].cuda() for k in ["x0", "obs_mask", "latent_mask", "kinda_marg_mask", "frame_indices"]}
    return dict(d, x_t_minus_1=d["x0"], observed_frames=observed_frames)


def _t(B, v):
    return torch.tensor([v] * B, device="cuda")


def _pass(model, x, d_in, prev, t, clip, xstart=None):
    """vd_dpmpp_2m_from_xstart on (B, per) tensors -> (sample, D_t)."""
    sample = torch.empty_like(x)
    xstart = torch.empty_like(x) if xstart is None else xstart
    _lib.check(_lib.lib().vd_dpmpp_2m_from_xstart(model._handle, x.shape[0], x[0].numel(), _lib.ptr(x), _lib.ptr(d_in), _lib.ptr(prev),
                                                  _lib.ptr(t), clip, _lib.ptr(sample), _lib.ptr(xstart), _lib.current_stream()))
    return sample, xstart


def _check_sample(diff, tv, x, d_t, d_prev, sample, tag):
    """sample against the float64 restatement fed the step's own float32 x, D_t and D_prev, per element inside the derived bound."""
    a, b, abp, w = tables(diff, tv)
    xn, dn, sn = (v.detach().cpu().numpy() for v in (x, d_t, sample))
    pn = None if d_prev is None else d_prev.detach().cpu().numpy()
    want, _, _ = step_fp64(xn, dn, pn, a, b, abp, w)
    lim = rounding_bound(xn, dn, pn, a, b, abp, w)
    err = np.abs(sn - want)
    ratio = float((err / np.maximum(lim, 1e-300)).max())
    print(f"{tag}: max |d| / bound = {ratio:.3f}, max |d| = {err.max():.3e}")
    assert (err <= lim).all(), (tag, ratio)
    return lim


# ---------------------------------------------------------------------------------------------------------------- 5
def test_the_pass_per_element_against_float64():
    """The pass alone (no network), B = 2, per = 1152: t in {0, 1, N-2, N-1}, with and without history, with and without the clamp."""
    model, diff = tiny()
    diff._bind(model)
    N = diff.num_timesteps
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, PER, generator=g).cuda()
    d_in = (0.8 * torch.randn(2, PER, generator=g)).cuda()                     # about a fifth beyond +-1: the clamp matters
    prev = (torch.rand(2, PER, generator=g) * 2 - 1).cuda()
    uniform = {}
    for tv in (0, 1, N - 2, N - 1):
        for hist in (None, prev):
            for clip in (1, 0):
                sample, d_t = _pass(model, x, d_in, hist, _t(2, tv), clip)
                assert torch.equal(d_t, d_in.clamp(-1, 1) if clip else d_in)     # D_t: the x_0 handed in, clamped
                lim = _check_sample(diff, tv, x, d_t, hist, sample, f"t={tv} hist={hist is not None} clip={clip}")
                if tv == 0:                                                      # abp = 1, w = 0: the sample is D_t whatever the history
                    assert tables(diff, 0)[2:] == (1.0, 0.0)
                    assert (np.abs((sample - d_t).cpu().numpy()) <= lim).all()
                uniform[tv, hist is not None, clip] = (sample, d_t)
                only = torch.empty_like(x)                                       # pred_xstart may be NULL: same sample
                _lib.check(_lib.lib().vd_dpmpp_2m_from_xstart(model._handle, 2, PER, _lib.ptr(x), _lib.ptr(d_in), _lib.ptr(hist), _lib.ptr(_t(2, tv)),
                                                              clip, _lib.ptr(only), None, _lib.current_stream()))
                assert torch.equal(only, sample)
    # the weight multiplies the DIFFERENCE: at an interior t (w != 0) no history and a history equal to D_t itself give the same bits
    for tv in (1, 4, N - 2):
        assert tables(diff, tv)[3] != 0.0
        none_s, none_d = uniform.get((tv, False, 1)) or _pass(model, x, d_in, None, _t(2, tv), 1)
        same_s, same_d = _pass(model, x, d_in, none_d, _t(2, tv), 1)
        assert torch.equal(same_s, none_s) and torch.equal(same_d, none_d), tv
        other_s, _ = _pass(model, x, d_in, prev, _t(2, tv), 1)
        assert not torch.equal(other_s, none_s)                                  # and a different history moves the sample
        # history kept in place (what the window executor does): prev_xstart and pred_xstart are one tensor
        buf = prev.clone()
        inplace_s, inplace_d = _pass(model, x, d_in, buf, _t(2, tv), 1, xstart=buf)
        assert torch.equal(inplace_s, other_s) and torch.equal(buf, none_d) and inplace_d is buf
    # mixed t per item: bit-equal to the uniform calls
    ts = [1, N - 2]
    for hist in (None, prev):
        ms, md = _pass(model, x, d_in, hist, torch.tensor(ts, device="cuda"), 1)
        for b, tv in enumerate(ts):
            us, ud = uniform[tv, hist is not None, 1]
            assert torch.equal(ms[b], us[b]) and torch.equal(md[b], ud[b]), (b, tv)
    assert not torch.equal(ms[0], ms[1])
    model.check_device_errors()
    # an out-of-range t poisons its item; a non-finite x_0 stays NaN and sets the sticky bit
    for bad in (N, -1):
        s, d = _pass(model, x, d_in, prev, torch.tensor([2, bad], device="cuda"), 1)
        assert torch.isfinite(s[0]).all() and torch.isnan(s[1]).all() and torch.isnan(d[1]).all()
    nan_in = d_in.clone()
    nan_in[1, 7] = float("nan")
    s, d = _pass(model, x, nan_in, prev, _t(2, 3), 1)
    assert torch.isnan(s[1, 7]) and torch.isnan(d[1, 7]) and torch.isfinite(s).sum() == s.numel() - 1
    with pytest.raises(FloatingPointError):
        model.check_device_errors()
    model.check_device_errors()
    # per must be a multiple of 4
    rc = _lib.lib().vd_dpmpp_2m_from_xstart(model._handle, 2, PER - 2, _lib.ptr(x), _lib.ptr(d_in), None, _lib.ptr(_t(2, 3)), 1,
                                            _lib.ptr(torch.empty_like(x)), None, _lib.current_stream())
    assert rc != 0 and b"multiple of 4" in _lib.lib().vd_last_error()


def test_weight_row_belongs_to_the_schedule():
    """vd_set_multistep_weights takes the bound schedule's length only; vd_set_schedule drops the row, and the sampler then fails
    with a message that says so -- on the eager entry and on vd_window_begin."""
    model, diff = tiny(timestep_respacing="logsnr5")
    diff._bind(model)
    L = _lib.lib()
    w = np.zeros(6, np.float32)
    assert L.vd_set_multistep_weights(model._handle, 6, _lib.ptr(w)) != 0 and b"bound schedule" in L.vd_last_error()
    x = torch.randn(2, PER).cuda()
    _pass(model, x, x, None, _t(2, 2), 1)
    tab = diff._device_tables()
    tm = np.ascontiguousarray(np.array(diff.timestep_map, dtype=np.int32))
    try:
        _lib.check(L.vd_set_schedule(model._handle, diff.num_timesteps, _lib.ptr(tab), _lib.ptr(tm), 1.0))
        with pytest.raises(_lib.VdError, match="vd_set_multistep_weights"):
            _pass(model, x, x, None, _t(2, 2), 1)
        c = _rand_window(2, 6, 32, 2, seed=3)
        with pytest.raises(_lib.VdError, match="vd_set_multistep_weights"):
            diff.dpmpp_2m_sample(model, c["x"].cuda(), _t(2, 2), model_kwargs=_window_kw(c))
        ex = WindowExecutor(model, diff)
        model._bound_schedule = diff                                             # keep begin() from re-binding: the row stays dropped
        with pytest.raises(_lib.VdError, match="vd_set_multistep_weights"):
            ex.begin(c["x"].cuda(), _window_kw(c), sampler="dpmpp_2m")
        ex.begin(c["x"].cuda(), _window_kw(c), sampler="ddim").run(1)            # the other samplers do not need it
    finally:
        model._bound_schedule = None
    diff._bind(model)
    _pass(model, x, x, None, _t(2, 2), 1)
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 6
def _device_chain(model, diff, s, x0, second_order):
    L = _lib.lib()
    coef = [float(np.float32(denoiser_coef(s, a))) for a in diff.alphas_cumprod]
    x, prev, B = x0.clone(), None, x0.shape[0]
    for tv in range(diff.num_timesteps - 1, -1, -1):
        d = x * coef[tv]
        if second_order:
            x, prev = _pass(model, x, d, prev, _t(B, tv), 0)
        else:
            nxt = torch.empty_like(x)
            _lib.check(L.vd_posterior_from_xstart(model._handle, 1, B, PER, _lib.ptr(x), _lib.ptr(d), _lib.ptr(_t(B, tv)), 0, 0.0, None, 0, 0,
                                                  _lib.ptr(nxt), None, None, _lib.current_stream()))
            x = nxt
    return x


@pytest.mark.parametrize("s", [0.5, 1.0])
def test_order_of_convergence_on_the_device(s):
    """The analytic model's chain through vd_dpmpp_2m_from_xstart (and eta = 0 DDIM through vd_posterior_from_xstart), D computed in
    torch on the device: the four conditions of the CPU restatement hold for the device results."""
    model, _ = tiny()
    err = {}
    try:
        for rs in ("logsnr20", "logsnr40", "ddim250"):
            diff = create_gaussian_diffusion(timestep_respacing=rs)
            diff._bind(model)
            x, exact = start(s, diff.alphas_cumprod[-1], 2 * PER, seed=7)
            x = torch.from_numpy(x).view(2, PER).cuda()
            err[rs] = tuple(rel_err(_device_chain(model, diff, s, x, so).cpu().numpy().reshape(-1), exact) for so in (True, False))
            print(f"s={s} {rs}: E2M = {err[rs][0]:.3e}, E_DDIM = {err[rs][1]:.3e}")
    finally:
        model._bound_schedule = None                                             # the next test binds its own schedule again
    for name, value, holds in order_conditions(err["logsnr20"][0], err["logsnr40"][0], err["logsnr20"][1], err["logsnr40"][1], err["ddim250"][1]):
        print(f"s={s}: {name}: {value:.3f}")
        assert holds, (s, name, value)
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("case", ["x_0", "x_t", "x_t_minus_1", "denoised_fn", "predict_xstart"])
def test_the_step_on_the_network_along_a_chain(case):
    """Five steps from the last index, each fed its own predecessor's sample and x_0 prediction: pred_xstart equals ddim_sample's for the same
    input at the step tolerance, the sample stays inside the derived bound of the float64 restatement fed the step's own x, D_t, D_prev."""
    model, diff = tiny(predict_xstart=True) if case == "predict_xstart" else tiny()
    assert diff.model_mean_type.name == ("START_X" if case == "predict_xstart" else "EPSILON")
    c = _rand_window(2, 6, 32, 2, seed=70)
    kw = _window_kw(c, case if case.startswith("x_") else "x_0")
    fn = _denoised_fn if case == "denoised_fn" else None
    N = diff.num_timesteps
    x, prev = c["x"].cuda(), None
    for tv in range(N - 1, N - 6, -1):
        before = x.clone()
        out = diff.dpmpp_2m_sample(model, x, _t(2, tv), prev_xstart=prev, denoised_fn=fn, model_kwargs=kw)
        assert set(out) == {"sample", "pred_xstart"} and torch.equal(x, before) and out["sample"].data_ptr() != x.data_ptr()
        assert float(out["pred_xstart"].abs().max()) <= 1.0
        ref = diff.ddim_sample(model, x, _t(2, tv), denoised_fn=fn, model_kwargs=kw, eta=0.0)
        close(out["pred_xstart"], ref["pred_xstart"], atol=ATOL, rtol=RTOL)
        _check_sample(diff, tv, x, out["pred_xstart"], prev, out["sample"], f"{case} t={tv}")
        if prev is None:                                                         # without history the step IS eta = 0 DDIM
            close(out["sample"], ref["sample"], atol=ATOL, rtol=RTOL)
        elif tv < N - 1:
            assert not torch.equal(out["sample"], ref["sample"])
        x, prev = out["sample"], out["pred_xstart"]
    assert torch.isfinite(x).all()
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 8
def test_loops_chain_the_step_and_differ_from_ddim():
    model, diff = tiny()
    c = _rand_window(2, 6, 32, 2, seed=80)
    kw = _window_kw(c)
    x_T = c["x"].cuda()
    N = diff.num_timesteps
    outs = list(diff.dpmpp_2m_sample_loop_progressive(model, tuple(x_T.shape), noise=x_T, model_kwargs=kw))
    assert len(outs) == N and all(set(o) == {"sample", "pred_xstart"} for o in outs)
    x, prev = x_T, None
    for k, tv in enumerate(range(N - 1, -1, -1)):
        o = diff.dpmpp_2m_sample(model, x, _t(2, tv), prev_xstart=prev, model_kwargs=kw)
        assert torch.equal(o["sample"], outs[k]["sample"]) and torch.equal(o["pred_xstart"], outs[k]["pred_xstart"]), tv
        x, prev = o["sample"], o["pred_xstart"]
    final = diff.dpmpp_2m_sample_loop(model, tuple(x_T.shape), noise=x_T, model_kwargs=kw)
    assert torch.is_tensor(final) and torch.equal(final, x) and torch.isfinite(final).all()
    assert torch.equal(diff.dpmpp_2m_sample_loop(diff._wrap_model(model), tuple(x_T.shape), noise=x_T, model_kwargs=kw), final)
    ddim = diff.ddim_sample_loop(model, tuple(x_T.shape), noise=x_T, model_kwargs=kw)
    assert not torch.equal(ddim, final)
    # a history-free chain of the step is the DDIM chain: the two loops differ by the extrapolation alone
    x = x_T
    for tv in range(N - 1, -1, -1):
        x = diff.dpmpp_2m_sample(model, x, _t(2, tv), model_kwargs=kw)["sample"]
    close(x, ddim, atol=1e-3, rtol=1e-3)            # (the two closing passes round differently, about 1e-7 a step, through ten network steps)
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 9
def _eager(model, diff, x_init, kw, n_steps, t_start, keep=()):
    """dpmpp_2m_sample step by step from t_start, the first one without history; returns the last sample and those kept."""
    x, prev, kept = x_init.clone(), None, {}
    for step in range(n_steps):
        o = diff.dpmpp_2m_sample(model, x, _t(x.shape[0], t_start - step), prev_xstart=prev, model_kwargs=kw)
        x, prev = o["sample"], o["pred_xstart"]
        if step + 1 in keep:
            kept[step + 1] = x
    return x, kept


def test_window_executor_runs_the_step_as_a_graph():
    """sampler='dpmpp_2m': the captured step is map_t -> forward -> deterministic_kernel<SAMPLER_DPMPP_2M> in place (history in place too) -> t -= 1, steps += 1.
    The window is bit-equal to the eager chain: two windows of one shape on ONE graph (the second one's first step first-order again),
    a later t_start, run(k) then run(), 'x_0' / 'x_t' / 'x_t_minus_1' as handed."""
    model, diff = tiny()
    diff._bind(model)
    N = diff.num_timesteps
    ex = WindowExecutor(model, diff)
    g0 = None
    for wi, (B, T, n_obs, obsf) in enumerate([(2, 6, 2, "x_0"), (2, 6, 2, "x_0"), (2, 6, 2, "x_t"), (2, 6, 3, "x_t_minus_1")]):
        c = _rand_window(B, T, 32, n_obs, seed=900 + wi)
        kw = _window_kw(c, obsf)
        if obsf == "x_t_minus_1":
            kw["x_t_minus_1"] = (c["x0"] * 0.5).cuda()
        x_init = c["x"].cuda()
        ex.begin(x_init, kw, sampler="dpmpp_2m", seed=wi, renoise=False)
        assert ex._left == N
        if wi == 0:
            g0 = ex.graphs
        if wi == 1:
            assert ex.graphs == g0                                               # same signature: the first window's graph
        got_mid = ex.run(3).clone()
        got = ex.run().clone()
        with pytest.raises(_lib.VdError, match="t would pass 0"):
            ex.run(1)
        want, kept = _eager(model, diff, x_init, kw, N, N - 1, keep=(3,))
        assert torch.equal(kept[3], got_mid), (wi, obsf, float((kept[3] - got_mid).abs().max()))
        assert torch.equal(want, got) and torch.isfinite(got).all(), (wi, obsf, float((want - got).abs().max()))
        if wi == 1:                                                              # a later start on the same graph: first-order at t = 6
            ex.begin(x_init, kw, sampler="dpmpp_2m", t_start=6)
            assert ex.graphs == g0 and ex._left == 7
            assert torch.equal(ex.run().clone(), _eager(model, diff, x_init, kw, 7, 6)[0])
    model.check_device_errors()
    # `sampler` is part of the graph key: 'p_sample' on the same tensors is a second graph, and coming back captures nothing
    c = _rand_window(2, 6, 32, 2, seed=950)
    kw, x_init = _window_kw(c), c["x"].cuda()
    ex.begin(x_init, kw, sampler="dpmpp_2m")
    g = ex.graphs
    ex.begin(x_init, kw, sampler="p_sample", seed=77)
    assert ex.graphs == g + 1
    assert torch.isfinite(ex.run().clone()).all()
    ex.begin(x_init, kw, sampler="dpmpp_2m")
    assert ex.graphs == g + 1
    assert torch.equal(ex.run().clone(), _eager(model, diff, x_init, kw, N, N - 1)[0])
    # the re-noising 'x_t_minus_1' form draws noise inside the graph: refused, by name and reason
    with pytest.raises(_lib.VdError, match="dpmpp_2m_sample.*draws no noise"):
        ex.begin(x_init, _window_kw(c, "x_t_minus_1"), sampler="dpmpp_2m", renoise=True)
    model.check_device_errors()
    # a learned variance cannot sample
    var = load_npz("variants_tiny.npz")
    model_ls, diff_ls = engine(json.loads(str(var["ls_cfg_json"])))
    cl = {k: torch.from_numpy(var[f"ls_{k}"]).cuda() for k in ["x", "x0", "obs_mask", "latent_mask", "kinda_marg_mask", "frame_indices"]}
    kwl = dict({k: v for k, v in cl.items() if k != "x"}, x_t_minus_1=cl["x0"], observed_frames="x_0")
    with pytest.raises(AssertionError, match="gaussian_diffusion.py:283"):
        WindowExecutor(model_ls, diff_ls).begin(cl["x"], kwl, sampler="dpmpp_2m")
    with pytest.raises(AssertionError, match="gaussian_diffusion.py:283"):
        diff_ls.dpmpp_2m_sample(model_ls, cl["x"], _t(2, 3), model_kwargs=kwl)
    with pytest.raises(AssertionError, match="gaussian_diffusion.py:283"):
        diff_ls.dpmpp_2m_sample_loop(model_ls, tuple(cl["x"].shape), noise=cl["x"], model_kwargs=kwl)


def test_window_with_suffix_skip_leaves_every_read_frame_bit_identical():
    """The step shares the forward's launches with the other samplers, so the suffix skip applies unchanged: every frame that is not a
    pure observation -- every frame the caller reads -- equals the plain executor's to the bit."""
    model, diff = tiny()
    plain, skip = WindowExecutor(model, diff), WindowExecutor(model, diff, suffix_skip=True)
    for wi, (B, T, n_obs, obsf) in enumerate([(2, 6, 2, "x_0"), (3, 5, 4, "x_t_minus_1")]):
        c = _rand_window(B, T, 32, n_obs, seed=960 + wi)
        read = ~((c["obs_mask"].reshape(B, T) == 1) & (c["latent_mask"].reshape(B, T) == 0))
        kw = _window_kw(c, obsf)
        x_init = c["x"].cuda()
        want = plain.begin(x_init, kw, sampler="dpmpp_2m", renoise=False).run().clone().cpu()
        skip.begin(x_init, kw, sampler="dpmpp_2m", renoise=False)
        assert skip.suffix_frames == int(read.sum())
        got = skip.run().clone().cpu()
        assert torch.isfinite(got[read]).all() and torch.equal(got[read], want[read]), (wi, float((got[read] - want[read]).abs().max()))
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 10
def test_infer_video_graph_and_eager_agree_to_the_bit():
    from video_diffusion_amd.video_sample import infer_video
    model, diff = tiny()
    g = torch.Generator().manual_seed(10)
    batch = (torch.rand(2, 12, 3, 32, 32, generator=g) * 2 - 1).cuda()
    eager, _ = infer_video("autoreg", model, diff, batch, 6, 2, 4, sampler="dpmpp_2m", executor="eager")
    graph, _ = infer_video("autoreg", model, diff, batch, 6, 2, 4, sampler="dpmpp_2m", executor="graph")
    assert eager.shape == (2, 12, 3, 32, 32) and np.isfinite(eager).all()
    assert np.array_equal(eager, graph)
    assert np.array_equal(eager[:, :2], batch[:, :2].cpu().numpy()) and np.abs(eager[:, 2:]).max() > 0
    ddim, _ = infer_video("autoreg", model, diff, batch, 6, 2, 4, sampler="ddim", executor="eager")
    assert not np.array_equal(ddim, eager)
    every, trace = infer_video("autoreg", model, diff, batch, 6, 2, 4, sampler="dpmpp_2m", save_all_timesteps=True)
    assert np.array_equal(every, eager) and trace.shape == (2, diff.num_timesteps, 12, 3, 32, 32)
    assert np.array_equal(trace[:, -1], eager)
    model.check_device_errors()
