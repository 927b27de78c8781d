"""GPU: cfg_scale -- classifier-free guidance on the observed frames (this project's extension): the combine pass per element against its
float64 restatement (tests/cfg_restated.py), the step at w = 1 / w = 0 / on an item without observed frames, the step against its
restated chain (two model() calls -> vd_op_cfg_combine -> the sampler pass) to the bit, linearity in w, the window graph and
infer_video.  B = 2 windows of T = 6 at 32 x 32: item 0 has 2 observed + 4 latent frames, item 1 has no observed frame."""
import ctypes
import json

import numpy as np
import pytest
import torch

import video_diffusion_amd as vda
from cfg_restated import combine_fp64, rounding_bound
from helpers import ATOL, RTOL, close, synth_sd
from video_diffusion_amd import _lib
from video_diffusion_amd.executor import WindowExecutor
from video_diffusion_amd.script_util import create_gaussian_diffusion

pytestmark = pytest.mark.gpu
KEYS = vda.video_model_and_diffusion_defaults().keys()
_cache = {}
TINY = dict(T=6, image_size=32, num_channels=64, num_res_blocks=1, rp_alpha=6, rp_beta=6, rp_gamma=6, timestep_respacing="ddim10")
B, T, S = 2, 6, 32


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


def _logsnr10():
    if "logsnr10" not in _cache:
        _cache["logsnr10"] = create_gaussian_diffusion(timestep_respacing="logsnr10")
    return _cache["logsnr10"]


def _window(seed, n_obs=2):
    """Item 0: n_obs observed frames and T - n_obs latent ones; item 1: nothing observed, every frame latent."""
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(B, T, 3, S, S, generator=g) * 2 - 1
    obs = torch.zeros(B, T, 1, 1, 1)
    obs[0, :n_obs] = 1
    x0 = x0 * obs
    x = torch.randn(B, T, 3, S, S, generator=g)
    return dict(x=x.cuda(), x0=x0.cuda(), obs_mask=obs.cuda(), latent_mask=(1 - obs).cuda(),
                kinda_marg_mask=torch.zeros(B, T, 1, 1, 1).cuda(), frame_indices=torch.arange(T).view(1, T).repeat(B, 1).cuda(),
                xtm1=(0.5 * x0 + 0.1 * torch.randn(B, T, 3, S, S, generator=g) * obs).cuda())


def _kw(c, observed_frames="x_0", zero_obs=False):
    d = {k: c[k] for k in ["x0", "obs_mask", "latent_mask", "kinda_marg_mask", "frame_indices"]}
    if zero_obs:
        d["obs_mask"] = torch.zeros_like(d["obs_mask"])
    return dict(d, x_t_minus_1=c["xtm1"], observed_frames=observed_frames)


def _t(v):
    return torch.tensor([v] * B, device="cuda")


def _noise(seed):
    return torch.randn(B, T, 3, S, S, generator=torch.Generator().manual_seed(seed)).cuda()


def _scale(model):
    return float(_lib.lib().vd_cfg_scale(model._handle))


def _combine(c, u, w):
    out = torch.empty_like(c)
    _lib.check(_lib.lib().vd_op_cfg_combine(_lib.ptr(c), _lib.ptr(u), float(w), c.numel(), _lib.ptr(out), _lib.current_stream()))
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------- 1
def _operands():
    """Pairs (out_c, out_u): the special ones first, random normal ones behind them."""
    sub = 1e-40                                                                  # subnormal in float32
    special = [(0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0), (0.0, 0.0), (sub, -sub), (3 * sub, sub), (1.0, sub), (1e30, -1e30), (-2e30, 1e30),
               (1e30, 1.0), (0.75, -1.25), (float("inf"), 1.0)]
    g = np.random.default_rng(11)
    c = np.concatenate([np.array([p[0] for p in special], np.float32), g.standard_normal(4200).astype(np.float32)])
    u = np.concatenate([np.array([p[1] for p in special], np.float32), g.standard_normal(4200).astype(np.float32)])
    return c, u, len(special)


@pytest.mark.parametrize("n", [1, 3, 255, 4099])
def test_the_pass_per_element_against_float64(n):
    """vd_op_cfg_combine for w in {0, 1, 1.5, 7.5, -1} on normal values, +-0, subnormals, 1e30-sized values and one inf, on 16-byte
    aligned tensors (float4 groups + scalar tail) and on tensors that start one float later (element by element), out of place and in
    place: |out - (out_u + w d)| <= 2^-23 (|out_u| + |w d|) + 2^-126 with d the float32 difference (cfg_restated.py: derived from one
    rounding of the fma), NaN where d is not finite, and at w = 0 out_u to the bit."""
    pc, pu, k = _operands()
    offsets = range(0, k, n) if n < k else [0]
    worst = 0.0
    seen_nan = False
    for off in offsets:
        cn, un = pc[off:off + n], pu[off:off + n]
        for shift in (0, 1):                                                     # 1: the three tensors are 4-byte aligned only
            base_c, base_u = torch.zeros(n + 4, device="cuda"), torch.zeros(n + 4, device="cuda")
            c, u = base_c[shift:shift + n], base_u[shift:shift + n]
            c.copy_(torch.from_numpy(cn))
            u.copy_(torch.from_numpy(un))
            assert c.data_ptr() % 16 == 4 * shift
            for w in (0.0, 1.0, 1.5, 7.5, -1.0):
                base_o = torch.full((n + 4,), 7.0, device="cuda")
                out = base_o[shift:shift + n]
                _lib.check(_lib.lib().vd_op_cfg_combine(_lib.ptr(c), _lib.ptr(u), w, n, _lib.ptr(out), _lib.current_stream()))
                assert (base_o[:shift] == 7.0).all() and (base_o[shift + n:] == 7.0).all()      # nothing written outside [0, n)
                got = out.cpu().numpy()
                want, d, ok = combine_fp64(cn, un, w)
                assert np.isnan(got[~ok]).all() and np.isfinite(got[ok]).all()
                seen_nan |= bool((~ok).any())
                lim = rounding_bound(un, w, d)
                err = np.abs(got[ok].astype(np.float64) - want[ok])
                assert (err <= lim[ok]).all(), (n, off, shift, w, float((err / lim[ok]).max()))
                if ok.any():
                    worst = max(worst, float((err / lim[ok]).max()))
                if w == 0.0:
                    assert np.array_equal(got[ok].view(np.int32), un[ok].view(np.int32))
                inplace = c.clone()
                _lib.check(_lib.lib().vd_op_cfg_combine(_lib.ptr(inplace), _lib.ptr(u), w, n, _lib.ptr(inplace), _lib.current_stream()))
                assert torch.equal(_bits(inplace), _bits(out))
    print(f"n={n}: largest |d| / bound = {worst:.3f}")
    assert seen_nan                                                              # (the inf pair, index 11, is inside some slice for every n)
    L = _lib.lib()
    x = torch.zeros(4, device="cuda")
    assert L.vd_op_cfg_combine(_lib.ptr(x), _lib.ptr(x), float("nan"), 4, _lib.ptr(x), _lib.current_stream()) != 0 and b"finite" in L.vd_last_error()
    assert L.vd_op_cfg_combine(_lib.ptr(x), _lib.ptr(x), 2.0, 0, _lib.ptr(x), _lib.current_stream()) != 0


def test_setter_refuses_a_scale_that_is_not_finite():
    model, diff = tiny()
    L = _lib.lib()
    assert _scale(model) == 1.0
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert L.vd_set_cfg_scale(model._handle, bad) != 0 and b"finite" in L.vd_last_error()
    assert _scale(model) == 1.0
    _lib.check(L.vd_set_cfg_scale(model._handle, -0.5))
    assert _scale(model) == -0.5
    _lib.check(L.vd_set_cfg_scale(model._handle, 1.0))
    with pytest.raises(ValueError, match="finite"):
        diff.p_sample(model, torch.zeros(B, T, 3, S, S), _t(3), model_kwargs={}, cfg_scale=float("nan"))


# ---------------------------------------------------------------------------------------------------------------- 2
def _launches(model, fn):
    L = _lib.lib()
    n = L.vd_profile_classes()
    out = (ctypes.c_double * (4 * n))()
    torch.cuda.synchronize()
    _lib.check(L.vd_profile_begin())
    try:
        res = fn()
    finally:
        _lib.check(L.vd_profile_end(out, 4 * n))
    return res, {L.vd_profile_class_name(i).decode(): int(out[4 * i]) for i in range(n) if out[4 * i]}


def test_scale_one_is_the_step_as_it_was_with_one_forward():
    model, diff = tiny()
    c = _window(20)
    kw, nz = _kw(c), _noise(21)
    plain, n_plain = _launches(model, lambda: diff._step(0, model, c["x"], _t(7), True, None, kw, 0.0, nz))
    one, n_one = _launches(model, lambda: diff._step(0, model, c["x"], _t(7), True, None, kw, 0.0, nz, cfg_scale=1.0))
    two, n_two = _launches(model, lambda: diff._step(0, model, c["x"], _t(7), True, None, kw, 0.0, nz, cfg_scale=2.0))
    assert torch.equal(_bits(plain[0]), _bits(one[0])) and torch.equal(_bits(plain[1]), _bits(one[1]))
    torch.manual_seed(5)
    a = diff.p_sample(model, c["x"], _t(7), model_kwargs=kw)
    torch.manual_seed(5)
    b = diff.p_sample(model, c["x"], _t(7), model_kwargs=kw, cfg_scale=1.0)
    assert torch.equal(_bits(a["sample"]), _bits(b["sample"])) and torch.equal(_bits(a["pred_xstart"]), _bits(b["pred_xstart"]))
    # the launch counts of the profiled classes: w = 1 is one forward and one posterior pass, w = 2 two forwards, one combine pass
    # (counted with the elementwise class) and still one posterior pass
    assert n_one == n_plain and n_plain["posterior_kernel"] == 1
    fwd = {k: v for k, v in n_plain.items() if k != "posterior_kernel"}
    want = {k: 2 * v for k, v in fwd.items()}
    want["affine_act_kernel"] = want.get("affine_act_kernel", 0) + 1
    want["posterior_kernel"] = 1
    assert n_two == want, (n_plain, n_two)
    assert not torch.equal(two[0][0], plain[0][0])
    assert _scale(model) == 1.0
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 3, 4
@pytest.mark.parametrize("observed_frames", ["x_0", "x_t", "x_t_minus_1"])
def test_scale_zero_is_the_unconditional_step_and_an_item_without_observations_is_untouched(observed_frames):
    model, diff = tiny()
    c = _window(30)
    kw, nz = _kw(c, observed_frames), _noise(31)
    step = lambda k, **o: diff._step(0, model, c["x"], _t(6), True, None, k, 0.0, nz, **o)  # noqa: E731
    plain = step(kw)
    uncond = step(_kw(c, observed_frames, zero_obs=True))
    zero = step(kw, cfg_scale=0.0)
    assert torch.equal(_bits(zero[0]), _bits(uncond[0])) and torch.equal(_bits(zero[1]), _bits(uncond[1]))
    assert not torch.equal(plain[0][0], uncond[0][0])                            # the observed frames do steer item 0
    three = step(kw, cfg_scale=3.0)
    assert torch.equal(_bits(three[0][1]), _bits(plain[0][1])) and torch.equal(_bits(three[1][1]), _bits(plain[1][1]))
    assert torch.equal(_bits(uncond[0][1]), _bits(plain[0][1]))                  # (item 1: both passes are the same kernels on the same inputs)
    assert not torch.equal(three[0][0], plain[0][0])
    assert _scale(model) == 1.0
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 5
def _chain(model, diff, c, kw, kw_u, tv, w, mode, eta, nz, start_x):
    """model(...) twice -> vd_op_cfg_combine -> the posterior pass alone: (sample, pred_xstart, out_g)."""
    L = _lib.lib()
    wrapped = diff._wrap_model(model)
    out_c, _ = wrapped(c["x"], _t(tv), **kw)
    out_u, _ = wrapped(c["x"], _t(tv), **kw_u)
    out_g = _combine(out_c, out_u, w)
    sample, xstart = torch.empty_like(c["x"]), torch.empty_like(c["x"])
    per = c["x"][0].numel()
    if start_x:
        _lib.check(L.vd_posterior_from_xstart(model._handle, mode, B, per, _lib.ptr(c["x"]), _lib.ptr(out_g), _lib.ptr(_t(tv)), 1, eta,
                                              _lib.ptr(nz), 0, 0, _lib.ptr(sample), _lib.ptr(xstart), None, _lib.current_stream()))
    else:
        _lib.check(L.vd_posterior_update(model._handle, mode, B, per, _lib.ptr(c["x"]), _lib.ptr(out_g), _lib.ptr(_t(tv)), 1, eta,
                                         _lib.ptr(nz), 0, 0, _lib.ptr(sample), _lib.ptr(xstart), _lib.current_stream()))
    return sample, xstart, out_g


@pytest.mark.parametrize("case", ["x_0", "x_t", "x_t_minus_1", "predict_xstart"])
@pytest.mark.parametrize("w", [2.0, -0.5])
def test_the_step_equals_its_restated_chain_to_the_bit(case, w):
    start_x = case == "predict_xstart"
    model, diff = tiny(predict_xstart=True) if start_x else tiny()
    obsf = case if case.startswith("x_") else "x_0"
    c = _window(50)
    kw, kw_u, nz = _kw(c, obsf), _kw(c, obsf, zero_obs=True), _noise(51)
    diff._bind(model)
    for mode, eta in ((0, 0.0), (1, 0.0), (1, 0.5)):
        want_s, want_x, out_g = _chain(model, diff, c, kw, kw_u, 5, w, mode, eta, nz, start_x)
        got_s, got_x = diff._step(mode, model, c["x"], _t(5), True, None, kw, eta, nz, cfg_scale=w)
        assert torch.equal(_bits(got_s), _bits(want_s)) and torch.equal(_bits(got_x), _bits(want_x)), (mode, eta, float((got_s - want_s).abs().max()))
    # the public names, on torch's generator
    torch.manual_seed(9)
    pub = diff.ddim_sample(model, c["x"], _t(5), model_kwargs=kw, eta=0.0, cfg_scale=w)
    assert torch.equal(_bits(pub["sample"]), _bits(_chain(model, diff, c, kw, kw_u, 5, w, 1, 0.0, nz, start_x)[0]))
    # p_mean_variance: 'eps' is the guided output, and denoised_fn sees the guided x_0 prediction
    pmv = diff.p_mean_variance(model, c["x"], _t(5), model_kwargs=kw, cfg_scale=w)
    assert torch.equal(_bits(pmv["eps"]), _bits(out_g))
    seen = []
    diff.p_sample(model, c["x"], _t(5), clip_denoised=False, denoised_fn=lambda v: seen.append(v) or v, model_kwargs=kw, cfg_scale=w)
    assert torch.equal(_bits(seen[0]), _bits(diff.p_mean_variance(model, c["x"], _t(5), clip_denoised=False, model_kwargs=kw, cfg_scale=w)["pred_xstart"]))
    model.check_device_errors()


def _ulps(a, b):
    """(elements whose bits differ, largest difference in units of the last place) of two float32 tensors of one sign pattern."""
    d = (_bits(a).long() - _bits(b).long()).abs()
    return int((d != 0).sum()), int(d.max())


@pytest.mark.parametrize("case", ["x_0", "x_t", "x_t_minus_1", "predict_xstart"])
@pytest.mark.parametrize("w", [2.0, -0.5])
def test_fused_dpmpp_2m_and_ddim_reverse_steps_equal_their_denoised_fn_form_to_the_bit(case, w):
    """dpmpp_2m_sample and ddim_reverse_sample take their scale from cfg_scale_scope: the fused step equals the same step through
    denoised_fn = identity, which goes through the guided p_mean_variance (vd_p_mean_variance, clip off) and the *_from_xstart pass.
    The figures are printed before they are asserted, for the scale under test and for w = 1 (no second forward, no combine pass).

    Both forms must take the x_0 prediction of an epsilon-model with one rounding sequence: posterior_kernel (the denoised_fn form) forms
    sr x - srm1 eps as two rounded products and a subtraction, and so does deterministic_kernel, through the same head (pass_x0: xstart_from_eps)."""
    start_x = case == "predict_xstart"
    model, diff = tiny(predict_xstart=True) if start_x else tiny()
    obsf = case if case.startswith("x_") else "x_0"
    c = _window(50)
    kw = _kw(c, obsf)
    d10 = _logsnr10() if not start_x else diff
    prev = (0.3 * c["x"]).clamp(-1, 1)
    ident_fn = lambda v: v  # noqa: E731
    res = {}
    try:
        for scale in (1.0, w):
            with d10.cfg_scale_scope(model, scale):
                assert _scale(model) == scale
                res[scale, "2m"] = (d10.dpmpp_2m_sample(model, c["x"], _t(5), model_kwargs=kw),
                                    d10.dpmpp_2m_sample(model, c["x"], _t(5), denoised_fn=ident_fn, model_kwargs=kw))
                res[scale, "2m+hist"] = (d10.dpmpp_2m_sample(model, c["x"], _t(5), prev_xstart=prev, model_kwargs=kw),
                                         d10.dpmpp_2m_sample(model, c["x"], _t(5), prev_xstart=prev, denoised_fn=ident_fn, model_kwargs=kw))
                res[scale, "reverse"] = (d10.ddim_reverse_sample(model, c["x"], _t(5), model_kwargs=kw),
                                         d10.ddim_reverse_sample(model, c["x"], _t(5), denoised_fn=ident_fn, model_kwargs=kw))
            assert _scale(model) == 1.0
    finally:
        model._bound_schedule = None                                             # the next test binds its own schedule again
    for (scale, name), (fused, ident) in res.items():
        for key in ("pred_xstart", "sample"):
            n_diff, ulp = _ulps(fused[key], ident[key])
            print(f"{case} w={scale} {name} {key}: {n_diff} of {fused[key].numel()} elements differ, at most {ulp} ulp")
    # the scale does guide these two steps as well, and leaves the item without observed frames alone
    for name in ("2m", "2m+hist", "reverse"):
        plain, guided = res[1.0, name][0]["sample"], res[w, name][0]["sample"]
        assert not torch.equal(plain[0], guided[0]) and torch.equal(_bits(plain[1]), _bits(guided[1])), name
    for (scale, name), (fused, ident) in res.items():
        assert torch.equal(_bits(fused["pred_xstart"]), _bits(ident["pred_xstart"])), (scale, name, "pred_xstart")     # (at w = 1 as well)
        assert torch.equal(_bits(fused["sample"]), _bits(ident["sample"])), (scale, name, "sample")
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 6
def test_it_guides_and_is_linear_in_the_scale():
    model, diff = tiny()
    c = _window(60)
    kw, nz = _kw(c), _noise(61)
    pred = {w: diff._step(0, model, c["x"], _t(4), False, None, kw, 0.0, nz, cfg_scale=w)[1] for w in (0.0, 1.0, 2.0)}
    assert not torch.equal(pred[2.0][0], pred[1.0][0])
    up, down = (pred[2.0] - pred[1.0]).cpu().numpy(), (pred[1.0] - pred[0.0]).cpu().numpy()
    assert float(np.abs(down[0]).max()) > 10 * ATOL, float(np.abs(down[0]).max())         # a difference the tolerance below can tell from none
    print(f"max |pred(1) - pred(0)| = {np.abs(down).max():.3e}, max |(pred(2) - pred(1)) - (pred(1) - pred(0))| = {np.abs(up - down).max():.3e}")
    close(up, down, atol=ATOL, rtol=RTOL)
    loops = {w: diff.ddim_sample_loop(model, tuple(c["x"].shape), noise=c["x"], model_kwargs=kw, cfg_scale=w) for w in (1.0, 2.0)}
    assert torch.equal(_bits(loops[1.0]), _bits(diff.ddim_sample_loop(model, tuple(c["x"].shape), noise=c["x"], model_kwargs=kw)))
    assert not torch.equal(loops[2.0][0], loops[1.0][0]) and torch.isfinite(loops[2.0]).all()
    assert _scale(model) == 1.0
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 7
def _eager_window(model, diff, c, kw, sampler, w, seed, renoise):
    """The window's steps one by one through the C entries under the engine's scale w, with the window's own Philox offsets."""
    L = _lib.lib()
    N = diff.num_timesteps
    cur = c["x"].clone()
    per = cur[0].numel()
    k = model._pack_kwargs(cur, kw)
    prev = None
    _lib.check(L.vd_set_cfg_scale(model._handle, w))
    try:
        for step, ti in enumerate(range(N)[::-1]):
            t = _t(ti)
            nxt = torch.empty_like(cur)
            obs_src = cur if kw["observed_frames"] == "x_t" else k["obs_src"]
            if renoise:                                                          # p_sample_loop's form: q_sample(x0, t - 1) once per step
                nz = torch.empty_like(cur)
                _lib.check(L.vd_randn(_lib.ptr(nz), nz.numel(), seed, step * B * per + B * per // 2, _lib.current_stream()))
                obs_src = torch.empty_like(cur)
                _lib.check(L.vd_q_sample(model._handle, B, per, _lib.ptr(c["x0"]), _lib.ptr(t - 1), _lib.ptr(nz), _lib.ptr(obs_src), _lib.current_stream()))
            args = (model._handle, B, T, _lib.ptr(cur), _lib.ptr(obs_src), _lib.ptr(k["obs_mask"]), _lib.ptr(k["latent_mask"]),
                    _lib.ptr(k["kinda_marg_mask"]), _lib.ptr(k["frame_indices"]), _lib.ptr(t))
            if sampler == "p_sample":
                _lib.check(L.vd_p_sample(*args, k["obs_mode"], 1, None, seed, step * B * per, _lib.ptr(nxt), None, None, _lib.current_stream()))
            elif sampler == "ddim":
                _lib.check(L.vd_ddim_sample(*args, k["obs_mode"], 1, 0.5, None, seed, step * B * per, _lib.ptr(nxt), None, None, _lib.current_stream()))
            else:
                xs = torch.empty_like(cur)
                _lib.check(L.vd_dpmpp_2m_sample(*args, _lib.ptr(prev), k["obs_mode"], 1, _lib.ptr(nxt), _lib.ptr(xs), None, _lib.current_stream()))
                prev = xs
            cur = nxt
    finally:
        _lib.check(L.vd_set_cfg_scale(model._handle, 1.0))
    return cur


@pytest.mark.parametrize("sampler", ["p_sample", "ddim", "dpmpp_2m"])
def test_window_graph_holds_both_forwards(sampler):
    model, diff = tiny()
    diff._bind(model)
    N = diff.num_timesteps
    ex = WindowExecutor(model, diff)
    c = _window(70)
    for obsf, renoise in (("x_0", False), ("x_t_minus_1", sampler == "p_sample")):
        kw = _kw(c, obsf)
        seed = 4321
        if renoise:
            kw["x_t_minus_1"] = c["x0"]
        got2 = ex.begin(c["x"], kw, seed=seed, sampler=sampler, eta=0.5, renoise=renoise, cfg_scale=2.0).run().clone()
        assert _scale(model) == 1.0 and ex._left == 0
        g2 = ex.graphs
        want2 = _eager_window(model, diff, c, kw, sampler, 2.0, seed, renoise)
        assert torch.equal(_bits(got2), _bits(want2)) and torch.isfinite(got2).all(), (obsf, float((got2 - want2).abs().max()))
        # the same shapes at 1.0: the unguided window, no stale scale and no stale graph
        got1 = ex.begin(c["x"], kw, seed=seed, sampler=sampler, eta=0.5, renoise=renoise, cfg_scale=1.0).run().clone()
        assert ex.graphs == g2 + 1
        assert torch.equal(_bits(got1), _bits(_eager_window(model, diff, c, kw, sampler, 1.0, seed, renoise)))
        assert torch.equal(_bits(got1), _bits(ex.begin(c["x"], kw, seed=seed, sampler=sampler, eta=0.5, renoise=renoise).run().clone()))
        assert ex.graphs == g2 + 1
        assert not torch.equal(got1[0], got2[0]) and torch.equal(_bits(got1[1]), _bits(got2[1]))     # item 1 has nothing to be guided by
        got3 = ex.begin(c["x"], kw, seed=seed, sampler=sampler, eta=0.5, renoise=renoise, cfg_scale=3.0).run().clone()
        assert ex.graphs == g2 + 2 and not torch.equal(got3[0], got2[0])
        # back at 2.0: the graph captured first, found by its key
        again = ex.begin(c["x"], kw, seed=seed, sampler=sampler, eta=0.5, renoise=renoise, cfg_scale=2.0).run(N).clone()
        assert ex.graphs == g2 + 2 and torch.equal(_bits(again), _bits(got2))
    model.check_device_errors()


def test_window_refuses_the_prefix_cache_and_the_suffix_skip():
    model, diff = tiny()
    c = _window(75)
    kw = _kw(c)
    for opt, setter in (("prefix_cache", "vd_set_window_prefix_cache"), ("suffix_skip", "vd_set_window_suffix_skip")):
        ex = WindowExecutor(model, diff, **{opt: True})
        with pytest.raises(NotImplementedError, match=f"{opt} together with cfg_scale"):
            ex.begin(c["x"], kw, sampler="ddim", cfg_scale=2.0)
        # the C entry itself, the host check bypassed
        plain = WindowExecutor(model, diff)
        plain.begin(c["x"], kw, sampler="ddim")                                  # (its buffers; this call switches both options off)
        L = _lib.lib()
        bufs = plain._bufs[B, T]
        _lib.check(getattr(L, setter)(model._handle, 1))
        _lib.check(L.vd_set_cfg_scale(model._handle, 2.0))
        try:
            rc = L.vd_window_begin(model._handle, B, T, _lib.ptr(bufs["x"]), _lib.ptr(bufs["obs_src"]), _lib.ptr(bufs["obs_mask"]),
                                   _lib.ptr(bufs["latent_mask"]), _lib.ptr(bufs["kinda_marg_mask"]), _lib.ptr(bufs["frame_indices"]), 0, 1, 1,
                                   0.0, 0, 0, diff.num_timesteps - 1, plain.stream.cuda_stream)
            with pytest.raises(_lib.VdError, match="cfg_scale != 1 together with the window " + opt.replace("_", " ")):
                _lib.check(rc)
        finally:
            _lib.check(L.vd_set_cfg_scale(model._handle, 1.0))
            _lib.check(getattr(L, setter)(model._handle, 0))
        # and with the scale back at 1 the option works as before
        assert torch.isfinite(ex.begin(c["x"], kw, sampler="ddim").run()[:, 2:]).all()
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 8
def test_infer_video_graph_and_eager_agree_to_the_bit():
    from video_diffusion_amd.video_sample import infer_video
    model, diff = tiny()
    g = torch.Generator().manual_seed(80)
    batch = (torch.rand(2, 10, 3, 32, 32, generator=g) * 2 - 1).cuda()
    run = lambda **o: infer_video("autoreg", model, diff, batch, 6, 2, 4, **o)[0]  # noqa: E731
    eager = run(sampler="ddim", executor="eager", cfg_scale=2.0)
    graph = run(sampler="ddim", executor="graph", cfg_scale=2.0)
    assert eager.shape == (2, 10, 3, 32, 32) and np.isfinite(eager).all() and np.array_equal(eager, graph)
    today = run(sampler="ddim", executor="eager")
    assert np.array_equal(run(sampler="ddim", executor="eager", cfg_scale=1.0), today)
    assert np.array_equal(run(sampler="ddim", executor="graph", cfg_scale=1.0), today)
    assert not np.array_equal(eager, today) and np.array_equal(eager[:, :2], batch[:, :2].cpu().numpy())
    assert np.array_equal(run(sampler="dpmpp_2m", executor="eager", cfg_scale=2.0), run(sampler="dpmpp_2m", executor="graph", cfg_scale=2.0))
    with pytest.raises(NotImplementedError, match="suffix_skip together with cfg_scale"):
        run(sampler="ddim", executor="graph", suffix_skip=True, cfg_scale=2.0)
    with pytest.raises(NotImplementedError, match="use_gradient_method together with cfg_scale"):
        run(use_gradient_method=True, cfg_scale=2.0)
    assert _scale(model) == 1.0
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 9
def test_the_scale_is_back_at_one_after_every_path_also_one_that_raised():
    model, diff = tiny()
    c = _window(90)
    kw = _kw(c)
    too_long = torch.zeros(1, _lib.lib().vd_max_window_frames() + 1, 3, S, S, device="cuda")
    m = torch.zeros(1, too_long.shape[1], 1, 1, 1, device="cuda")
    kw_long = dict(x0=too_long, obs_mask=m, latent_mask=1 - m, kinda_marg_mask=m, x_t_minus_1=too_long, observed_frames="x_0")
    t1 = torch.tensor([3], device="cuda")
    for call in (lambda: diff.p_sample(model, too_long, t1, model_kwargs=kw_long, cfg_scale=2.0),
                 lambda: diff.ddim_sample(model, too_long, t1, model_kwargs=kw_long, cfg_scale=2.0),
                 lambda: diff.p_mean_variance(model, too_long, t1, model_kwargs=kw_long, cfg_scale=2.0)):
        with pytest.raises(_lib.VdError, match="vd_max_window_frames"):
            call()
        assert _scale(model) == 1.0
    with pytest.raises(_lib.VdError, match="vd_max_window_frames"):
        with diff.cfg_scale_scope(model, 2.0):
            assert _scale(model) == 2.0
            diff.ddim_reverse_sample(model, too_long, t1, model_kwargs=kw_long)
    assert _scale(model) == 1.0
    with pytest.raises(_lib.VdError, match="vd_max_window_frames"):
        WindowExecutor(model, diff).begin(too_long, kw_long, sampler="ddim", cfg_scale=2.0)
    assert _scale(model) == 1.0
    with pytest.raises(NotImplementedError, match="return_attn_weights together with cfg_scale"):
        diff.p_sample(model, c["x"], _t(3), model_kwargs=kw, return_attn_weights=True, cfg_scale=2.0)
    # the engine's own refusal, the host check bypassed: an armed attention capture and a second forward
    with pytest.raises(_lib.VdError, match="return_attn_weights"):
        with diff.cfg_scale_scope(model, 2.0):
            diff.p_sample(model, c["x"], _t(3), model_kwargs=kw, return_attn_weights=True)
    assert _scale(model) == 1.0
    # an inf in the conditional output alone: NaN out of the combine pass even at w = 0, and the sampler pass says so
    bad = dict(kw, x0=c["x0"].clone())
    bad["x0"][0, 0, 0, 0, 0] = float("inf")
    out = diff.p_sample(model, c["x"], _t(3), model_kwargs=bad, cfg_scale=0.0)
    assert torch.isnan(out["sample"][0]).any() and torch.isfinite(out["sample"][1]).all()
    with pytest.raises(FloatingPointError):
        model.check_device_errors()
    assert torch.isfinite(diff.p_sample(model, c["x"], _t(3), model_kwargs=kw)["sample"]).all() and _scale(model) == 1.0
    model.check_device_errors()
