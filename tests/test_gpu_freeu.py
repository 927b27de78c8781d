"""GPU: FreeU (this project's extension; Si, Huang, Jiang, Liu, CVPR 2024) -- the two passes per element against their float64
restatements (tests/freeu_restated.py), the whole model under freeu_scope against the oracle that runs them (FreeUNetRef; the constants
are licensed by tests/test_freeu_cpu.py), the steps, the window graph, infer_video, the refusals and the command line.

A one-level model (no stage 2: b2 and s2 accepted and unused) cannot be created -- the level count follows the image size, four to
six levels -- so beside the tiny model and a 64-channel one with three blocks per stage the third model is a configuration of the sweep
fixture with four blocks per stage, and vd_freeu_stages() == 2 is asserted for every model here."""
import ctypes

import numpy as np
import pytest
import torch

import video_diffusion_amd as vda
from freeu_restated import (B_CONST, EPS_ATOL, EPS_RTOL, S_CONST, backbone, filter_closed, model_cfg, oracle, oracle_eps, rounding_bound, window)
from helpers import ATOL, RTOL, Guarded, close, synth_sd
from video_diffusion_amd import _lib
from video_diffusion_amd.executor import WindowExecutor
from video_diffusion_amd.gaussian_diffusion import freeu_state, measure

pytestmark = pytest.mark.gpu
KEYS = vda.video_model_and_diffusion_defaults().keys()
_models = {}
SHAPES = [(1, 2, 32), (3, 4, 64), (2, 5, 32), (1, 7, 40), (2, 8, 96), (2, 16, 160), (1, 32, 64), (1, 4, 1024)]
FU = dict(b1=B_CONST[0], b2=B_CONST[1], s1=S_CONST[0], s2=S_CONST[1])
OFF = ((1.0, 1.0, 1.0, 1.0), False)


def engine(name):
    if name not in _models:
        cfg = model_cfg(name)
        model, diff = vda.create_video_model_and_diffusion(**{k: cfg[k] for k in KEYS})
        model.load_state_dict(synth_sd(model.param_specs()))
        model.to("cuda")
        model.eval()
        _models[name] = (model, diff)
    return _models[name]


def _dev(kw):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _planes(N, S, C, seed, hostile=False):
    """Channels-last [N][S][S][C] on the CPU; hostile: 1e4 + unit noise, where the filter's update cancels against x."""
    x = torch.randn(N, S, S, C, generator=torch.Generator().manual_seed(seed))
    return x + 1e4 if hostile else x


def _cl(f, x, *a):
    """A restated operator of freeu_restated.py (planes last) on a channels-last tensor, float64."""
    return f(x.permute(0, 3, 1, 2).double(), *a).permute(0, 2, 3, 1).contiguous()


def _filter(xd, s):
    N, S, _, C = xd.shape
    out = Guarded(N, S, S, C)
    _lib.check(_lib.lib().vd_op_freeu_filter(_lib.ptr(xd), N, S, C, float(s), _lib.ptr(out.t), _lib.current_stream()))
    return out.read()


def _backbone(hd, b, adaptive):
    N, S, _, C = hd.shape
    out = Guarded(N, S, S, C)
    _lib.check(_lib.lib().vd_op_freeu_backbone(_lib.ptr(hd), N, S, C, float(b), 1 if adaptive else 0, _lib.ptr(out.t), _lib.current_stream()))
    return out.read()


def _inside(got, ref64, x, tag):
    lim = rounding_bound(ref64, x)
    err = (got.double() - ref64).abs()
    ratio = float((err / lim).max())
    print(f"{tag}: max |d| / bound = {ratio:.3f}, max |d| = {float(err.max()):.3e}")
    assert bool((err <= lim).all()), (tag, ratio)


# ---------------------------------------------------------------------------------------------------------------- the two passes
@pytest.mark.parametrize("N,S,C", SHAPES)
def test_filter_per_element_against_float64(N, S, C):
    """|got - ref64| <= 2^-23 |ref64| + 2^-40 max|x|: one float32 rounding of a float64-exact value; the absolute term covers float64's
    own error where the update cancels against x (the hostile set).  s = 1 returns the input bits, two runs are equal to the bit, and
    the pads around the output stay intact (Guarded)."""
    for hostile in (False, True) if (N, S, C) == (2, 8, 96) else (False,):
        x = _planes(N, S, C, 1000 + S + C, hostile)
        xd = x.cuda()
        for s in (0.2, 0.9, 1.7):
            got = _filter(xd, s)
            _inside(got, _cl(filter_closed, x, s), x, f"filter {N}x{S}x{S}x{C} s={s} hostile={hostile}")
            assert torch.equal(_bits(got), _bits(_filter(xd, s)))
            assert not torch.equal(got, x)
        assert torch.equal(_bits(_filter(xd, 1.0)), _bits(x))
        assert torch.equal(xd.cpu(), x)                                          # the input is not written


def test_filter_refuses_bad_arguments():
    L = _lib.lib()
    x, y = torch.zeros(1, 4, 4, 8, device="cuda"), torch.zeros(1, 4, 4, 8, device="cuda")
    st = _lib.current_stream()
    assert L.vd_op_freeu_filter(_lib.ptr(x), 1, 4, 8, 0.5, _lib.ptr(x), st) != 0 and b"in place" in L.vd_last_error()
    assert L.vd_op_freeu_filter(_lib.ptr(x), 1, 4, 6, 0.5, _lib.ptr(y), st) != 0 and b"multiple of 4" in L.vd_last_error()
    assert L.vd_op_freeu_filter(_lib.ptr(x), 1, 4, 8, float("nan"), _lib.ptr(y), st) != 0 and b"finite" in L.vd_last_error()
    assert L.vd_op_freeu_backbone(_lib.ptr(x), 1, 4, 8, 1.5, 0, _lib.ptr(x), st) != 0 and b"in place" in L.vd_last_error()
    # one pixel: the four bins coincide and the published box is empty -- refused, not filtered four times
    assert L.vd_op_freeu_filter(_lib.ptr(x), 1, 1, 8, 0.5, _lib.ptr(y), st) != 0 and b"S >= 2" in L.vd_last_error()


# ... and two whose half C / 2 is no multiple of 4: a channel quad straddles the half (the kernel's per-element guard)
BACKBONE_SHAPES = SHAPES + [(2, 3, 36), (2, 4, 4)]


@pytest.mark.parametrize("N,S,C", BACKBONE_SHAPES)
def test_backbone_plain_is_torchs_float32_multiply_to_the_bit(N, S, C):
    h = _planes(N, S, C, 2000 + S + C)
    hd = h.cuda()
    for b in (1.4, 0.7, 1.0):
        got = _backbone(hd, b, False)
        want = torch.cat([hd[..., :C // 2] * b, hd[..., C // 2:]], dim=-1).cpu()
        assert torch.equal(_bits(got), _bits(want)), (N, S, C, b)
    assert torch.equal(hd.cpu(), h)


@pytest.mark.parametrize("N,S,C", BACKBONE_SHAPES)
def test_backbone_adaptive_per_element_against_float64(N, S, C):
    """The filter's bound on the filter's shapes, plus a frame whose channel mean is the same at every pixel: g = 0 there and the output
    equals the input to the bit (the published code would divide 0 by 0)."""
    h = _planes(N + 1, S, C, 3000 + S + C)                                       # the shape's N frames, and the constant one behind them
    h[N] = torch.randn(C, generator=torch.Generator().manual_seed(5)).view(1, 1, C).expand(S, S, C)
    hd = h.cuda()
    for b in (1.4, 0.7):
        got = _backbone(hd, b, True)
        _inside(got, _cl(backbone, h, b, True), h, f"backbone {N}x{S}x{S}x{C} b={b}")
        assert torch.equal(_bits(got[N]), _bits(h[N]))
        assert torch.equal(_bits(got[..., C // 2:]), _bits(h[..., C // 2:]))
        assert torch.equal(_bits(got), _bits(_backbone(hd, b, True)))
        assert not torch.equal(got[0, ..., :C // 2], h[0, ..., :C // 2])
    assert torch.equal(_bits(_backbone(hd, 1.0, True)), _bits(h))


# ---------------------------------------------------------------------------------------------------------------- the whole model
@pytest.mark.parametrize("name,adaptive,w", [("tiny", False, 1.0), ("tiny", True, 1.0), ("w64_rb2", False, 1.0), ("w64_rb2", True, 1.0),
                                             ("sweep", False, 1.0), ("sweep", True, 1.0), ("tiny", False, 2.0)])
def test_eps_under_the_scope_against_the_oracle(name, adaptive, w):
    """eps of the engine under freeu_scope against FreeUNetRef at test_gpu_engine.py's tolerance on eps.  w = 2: the guided output
    out_u + w (out_c - out_u) of p_mean_variance, both forwards under FreeU, at the same tolerance."""
    model, diff = engine(name)
    assert _lib.lib().vd_freeu_stages(model._handle) == 2
    x, t, kw = window(name)
    with diff.freeu_scope(model, **FU, adaptive=adaptive):
        assert freeu_state(model) == ((*B_CONST, *S_CONST), adaptive)
        if w == 1.0:
            got, _ = diff._wrap_model(model)(x.cuda(), t.cuda(), **_dev(kw))
            want, k = oracle_eps(name, adaptive), 1.0
        else:
            got = diff.p_mean_variance(model, x.cuda(), t.cuda(), clip_denoised=False, model_kwargs=_dev(kw), cfg_scale=w)["eps"]
            c, u = oracle_eps(name, adaptive), oracle_eps(name, adaptive, True)
            want, k = u + w * (c - u), 1.0
    assert freeu_state(model) == OFF
    model.check_device_errors()
    err = close(got.cpu(), want, atol=k * EPS_ATOL, rtol=EPS_RTOL)
    print(f"{name} adaptive={adaptive} w={w}: max |eps - oracle| = {err:.3e}; max |oracle - plain oracle| = {float((want - oracle_eps(name)).abs().max()):.3e}")
    plain, _ = diff._wrap_model(model)(x.cuda(), t.cuda(), **_dev(kw))           # behind the scope: the plain forward again
    close(plain.cpu(), oracle_eps(name), atol=EPS_ATOL, rtol=EPS_RTOL)


@pytest.mark.parametrize("adaptive", [False, True])
def test_eps_where_the_skip_convolution_writes_the_activation_image(adaptive):
    """Stage 2 at 16 x 16 over 128 frames (freeu_restated.wide_window): its blocks' 1x1 skip convolutions run on the 128 x 128 tile, the
    ResBlock form that folds the first GroupNorm ahead of the block instead of inside its transient.  The statistics of h' and skip' must
    not come out of the step arena there -- the dry run that sizes it sees the unmodified halves with their producers' tables -- so the
    forward has to be served (no workspace overflow) for every FreeU setting, and eps of two items equals the oracle's."""
    from freeu_restated import WIDE_ITEMS, wide_oracle_eps, wide_window
    model, diff = engine("w64_s64")
    L = _lib.lib()
    x, t, kw = wide_window()
    name = ctypes.create_string_buffer(256)                                      # the stage-2 skip convolution: 448 -> 192 at 16 x 16, 128 frames
    assert L.vd_igemm_variant(1, 1, 0, 448, 256, 192, 128, 0, 16, 3, 0, 0, 0, 0, 1, 1, 0, name, 256) == 1, name.value
    assert b"gemm_split_kernel<128,128," in name.value, name.value
    pick = list(WIDE_ITEMS)
    with diff.freeu_scope(model, **FU, adaptive=adaptive):
        got, _ = diff._wrap_model(model)(x.cuda(), t.cuda(), **_dev(kw))
    model.check_device_errors()
    want = wide_oracle_eps(adaptive)
    err = close(got[pick].cpu(), want, atol=EPS_ATOL, rtol=EPS_RTOL)
    moved = float((want - wide_oracle_eps()).abs().max())
    print(f"wide adaptive={adaptive}: max |eps - oracle| = {err:.3e}; max |oracle - plain oracle| = {moved:.3e}")
    assert moved >= 100 * EPS_ATOL
    plain, _ = diff._wrap_model(model)(x.cuda(), t.cuda(), **_dev(kw))
    close(plain[pick].cpu(), wide_oracle_eps(), atol=EPS_ATOL, rtol=EPS_RTOL)


# ---------------------------------------------------------------------------------------------------------------- steps
def _tt(B, v):
    return torch.tensor([v] * B, device="cuda")


def test_p_sample_and_ddim_sample_under_the_scope_against_the_oracle():
    """test_gpu_engine.py's tolerances for these two steps: pred_xstart at 2e-5 (1 + sqrt_recipm1) / 1e-4, p_sample at 1e-4, ddim at 2e-4."""
    model, diff = engine("tiny")
    x, t, kw = window("tiny")
    noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(3))
    for adaptive in (False, True):
        ora = oracle("tiny", adaptive)
        with diff.freeu_scope(model, **FU, adaptive=adaptive):
            sample, xstart = diff._step(0, model, x.cuda(), t.cuda(), True, None, _dev(kw), 0.0, noise)
            s2, xs2 = diff._step(1, model, x.cuda(), t.cuda(), True, None, _dev(kw), 0.5, noise)
        gain = 1.0 + float(diff.sqrt_recipm1_alphas_cumprod[int(t[0])])
        want = ora.p_sample(x, t, kw, noise)
        close(xstart.cpu(), want["pred_xstart"], atol=2e-5 * gain, rtol=1e-4)
        close(sample.cpu(), want["sample"], atol=1e-4, rtol=1e-4)
        close(s2.cpu(), ora.ddim_sample(x, t, kw, noise, eta=0.5)["sample"], atol=2e-4, rtol=2e-4)
        assert torch.equal(_bits(xs2), _bits(xstart))
        assert float((want["sample"] - oracle("tiny").p_sample(x, t, kw, noise)["sample"]).abs().max()) > 100 * 1e-4
    model.check_device_errors()


def test_dpmpp_2m_and_unipc_under_the_scope_against_the_restated_samplers():
    """Two steps of each from the last index, as the samplers' own files check them: pred_xstart against the oracle's for the same input
    at the step tolerance, the first sample (no history) against the oracle's eta = 0 DDIM at ATOL / RTOL, the second inside the derived
    bound of the float64 restatement fed the step's own x, D_t and history."""
    from test_gpu_dpmpp_2m import _check_sample
    from test_gpu_unipc import _check
    model, diff = engine("tiny")
    x, _, kw = window("tiny")
    ora = oracle("tiny", False)
    B, N = x.shape[0], diff.num_timesteps
    gain = lambda tv: 1.0 + float(diff.sqrt_recipm1_alphas_cumprod[tv])          # noqa: E731
    with diff.freeu_scope(model, **FU):
        for name in ("dpmpp_2m", "unipc"):
            cur, carry = x.cuda(), None
            for k, tv in enumerate((N - 1, N - 2)):
                if name == "dpmpp_2m":
                    out = diff.dpmpp_2m_sample(model, cur, _tt(B, tv), prev_xstart=carry, model_kwargs=_dev(kw))
                else:
                    out = diff.unipc_sample(model, cur, _tt(B, tv), state=carry, model_kwargs=_dev(kw))
                tc = torch.tensor([tv] * B)
                ref = ora.ddim_sample(cur.cpu(), tc, kw, torch.zeros_like(x), eta=0.0)      # (both evaluate the network at the x handed in)
                close(out["pred_xstart"].cpu(), ref["pred_xstart"], atol=2e-5 * gain(tv), rtol=1e-4)
                if k == 0:
                    close(out["sample"].cpu(), ref["sample"], atol=ATOL, rtol=RTOL)
                if name == "dpmpp_2m":
                    _check_sample(diff, tv, cur, out["pred_xstart"], carry, out["sample"], f"dpmpp_2m t={tv}")
                    cur, carry = out["sample"], out["pred_xstart"]
                else:
                    _check(diff, [tv] * B, k, cur, out["pred_xstart"], carry, out["state"][0], out["sample"], f"unipc t={tv}")
                    cur, carry = out["sample"], out["state"]
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- graphs
def _eager(model, diff, x, kw, sampler, n, seed):
    """n steps one by one through the C entries under the engine's state, with a window's own Philox offsets."""
    L = _lib.lib()
    B, T = x.shape[:2]
    cur = x.cuda().clone()
    per = cur[0].numel()
    k = model._pack_kwargs(cur, _dev(kw))
    for step, ti in enumerate(range(diff.num_timesteps)[::-1][:n]):
        nxt = torch.empty_like(cur)
        args = (model._handle, B, T, _lib.ptr(cur), _lib.ptr(k["obs_src"]), _lib.ptr(k["obs_mask"]), _lib.ptr(k["latent_mask"]),
                _lib.ptr(k["kinda_marg_mask"]), _lib.ptr(k["frame_indices"]), _lib.ptr(_tt(B, ti)))
        if sampler == "p_sample":
            _lib.check(L.vd_p_sample(*args, k["obs_mode"], 1, None, seed, step * B * per, _lib.ptr(nxt), None, None, _lib.current_stream()))
        else:
            _lib.check(L.vd_ddim_sample(*args, k["obs_mode"], 1, 0.5, None, seed, step * B * per, _lib.ptr(nxt), None, None, _lib.current_stream()))
        cur = nxt
    return cur


@pytest.mark.parametrize("sampler", ["p_sample", "ddim"])
def test_window_graph_equals_the_eager_steps_and_is_keyed_by_the_constants(sampler):
    model, diff = engine("tiny")
    diff._bind(model)
    x, _, kw = window("tiny")
    ex = WindowExecutor(model, diff)
    run = lambda: ex.begin(x.cuda(), _dev(kw), seed=99, sampler=sampler, eta=0.5, renoise=False).run(3).clone()  # noqa: E731
    off = run()
    g0 = ex.graphs
    assert torch.equal(_bits(off), _bits(_eager(model, diff, x, kw, sampler, 3, 99)))
    with diff.freeu_scope(model, **FU):
        a = run()
        assert ex.graphs == g0 + 1
        assert torch.equal(_bits(a), _bits(_eager(model, diff, x, kw, sampler, 3, 99))) and not torch.equal(a, off)
    with diff.freeu_scope(model, **FU, adaptive=True):
        b = run()
        assert ex.graphs == g0 + 2
        assert torch.equal(_bits(b), _bits(_eager(model, diff, x, kw, sampler, 3, 99))) and not torch.equal(a, b)
    assert torch.equal(_bits(run()), _bits(off)) and ex.graphs == g0 + 2         # back to off: the plain graph, found by its key
    with diff.freeu_scope(model, **FU):
        assert torch.equal(_bits(run()), _bits(a)) and ex.graphs == g0 + 2
    with diff.freeu_scope(model, 1.0, 1.0, 1.0, 1.0, adaptive=True):            # all constants 1: off, whatever the form
        assert torch.equal(_bits(run()), _bits(off)) and ex.graphs == g0 + 2
    with diff.freeu_scope(model, **FU):                                          # a window armed inside the scope runs outside it
        ex.begin(x.cuda(), _dev(kw), seed=99, sampler=sampler, eta=0.5, renoise=False)
    assert freeu_state(model) == OFF and torch.equal(_bits(ex.run(3).clone()), _bits(a))
    model.check_device_errors()


def _launches(fn):
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


def test_unit_constants_are_the_plain_step_with_no_added_launch():
    model, diff = engine("tiny")
    x, t, kw = window("tiny")
    noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(4))
    step = lambda: diff._step(0, model, x.cuda(), t.cuda(), True, None, _dev(kw), 0.0, noise)  # noqa: E731
    plain, n_plain = _launches(step)
    with diff.freeu_scope(model, 1.0, 1.0, 1.0, 1.0):
        one, n_one = _launches(step)
    assert torch.equal(_bits(plain[0]), _bits(one[0])) and torch.equal(_bits(plain[1]), _bits(one[1])) and n_one == n_plain
    # on: per block of the two stages (2 x 2 here) one backbone and one filter record in the elementwise class; with b2 = s1 = 1 half of them
    with diff.freeu_scope(model, **FU):
        on, n_on = _launches(step)
    with diff.freeu_scope(model, b1=1.4, s2=0.8, adaptive=True):
        half, n_half = _launches(step)
    assert n_on["affine_act_kernel"] == n_plain.get("affine_act_kernel", 0) + 8, (n_plain, n_on)
    assert n_half["affine_act_kernel"] == n_plain.get("affine_act_kernel", 0) + 4, (n_plain, n_half)
    assert not torch.equal(on[0], plain[0]) and not torch.equal(half[0], on[0])
    model.check_device_errors()


def test_infer_video_graph_and_eager_agree_to_the_bit():
    from video_diffusion_amd.video_sample import infer_video
    model, diff = engine("tiny")
    batch = (torch.rand(2, 7, 3, 32, 32, generator=torch.Generator().manual_seed(80)) * 2 - 1).cuda()
    run = lambda **o: infer_video("autoreg", model, diff, batch, 4, 2, 2, sampler="ddim", **o)[0]  # noqa: E731
    fu = (*B_CONST, *S_CONST)
    eager, graph = run(executor="eager", freeu=fu), run(executor="graph", freeu=fu)
    assert eager.shape == (2, 7, 3, 32, 32) and np.isfinite(eager).all() and np.array_equal(eager, graph)
    today = run(executor="eager")
    assert np.array_equal(run(executor="graph", freeu=(1.0, 1.0, 1.0, 1.0)), today) and not np.array_equal(eager, today)
    ad = run(executor="eager", freeu=fu, freeu_adaptive=True)
    assert np.array_equal(ad, run(executor="graph", freeu=fu, freeu_adaptive=True)) and not np.array_equal(ad, eager)
    assert np.array_equal(run(executor="eager", freeu=fu, cfg_scale=2.0), run(executor="graph", freeu=fu, cfg_scale=2.0))
    for opts, what in ((dict(executor="graph", suffix_skip=True), "suffix_skip"), (dict(executor="graph", prefix_cache=True), "prefix_cache"),
                       (dict(use_gradient_method=True), "use_gradient_method")):
        with pytest.raises(NotImplementedError, match=f"{what} together with freeu"):
            run(freeu=fu, **opts)
    with pytest.raises(ValueError, match="finite and > 0"):
        run(freeu=(1.4, 1.2, -0.6, 0.8))
    assert freeu_state(model) == OFF
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_every_refusal_by_name():
    model, diff = engine("tiny")
    diff._bind(model)
    L = _lib.lib()
    x, t, kw = window("tiny")
    xd, td, kd = x.cuda(), t.cuda(), _dev(kw)
    B, T = x.shape[:2]
    y = measure(torch.rand(tuple(x.shape), generator=torch.Generator().manual_seed(6)) * 2 - 1, 4, False)
    cot = torch.randn(x.shape, generator=torch.Generator().manual_seed(7)).cuda()

    def dps():
        with diff.dps_scope(model, y, 4, zeta=0.5):
            diff.p_sample(model, xd, td, model_kwargs=kd)

    def loss():
        with diff.loss_guidance_scope(model, lambda x0, t_: (x0 ** 2).sum(), scale=0.5):
            diff.p_sample(model, xd, td, model_kwargs=kd)

    with diff.freeu_scope(model, **FU):
        for call, what in ((dps, "dps"), (loss, "loss_guidance"),
                           (lambda: diff.eps_vjp(model, xd, td, cot, kd), "eps_vjp"),
                           (lambda: diff.ode_nll_loop(model, kd["x0"], model_kwargs=kd), "ode_nll"),
                           (lambda: diff.p_sample(model, xd, td, model_kwargs=kd, use_gradient_method=True), "use_gradient_method"),
                           (lambda: diff.score_windows(model, kd["x0"], td, kd, None, 1, [0] * B), "score_windows")):
            with pytest.raises(_lib.VdError, match=f"{what} together with FreeU"):
                call()
        with pytest.raises(_lib.VdError, match="NLL loop .calc_bpd_loop. together with FreeU"):
            diff.calc_bpd_loop(model, kd["x0"], model_kwargs=kd)
        # the NLL's own engine entry, the host check bypassed
        v = torch.zeros(B, device="cuda")
        assert L.vd_vb_terms(model._handle, B, T, _lib.ptr(xd), _lib.ptr(xd), _lib.ptr(xd), None, _lib.ptr(td), 1, None, _lib.ptr(v), _lib.ptr(v),
                             None, None, _lib.current_stream()) != 0 and b"NLL path) together with FreeU" in L.vd_last_error()
        for opt, setter in (("prefix_cache", "vd_set_window_prefix_cache"), ("suffix_skip", "vd_set_window_suffix_skip")):
            with pytest.raises(NotImplementedError, match=f"{opt} together with FreeU"):
                WindowExecutor(model, diff, **{opt: True}).begin(xd, kd, sampler="ddim")
            plain = WindowExecutor(model, diff)                                  # the C entry itself, the host check bypassed
            plain.begin(xd, kd, sampler="ddim")
            bufs = plain._bufs[B, T]
            _lib.check(getattr(L, setter)(model._handle, 1))
            try:
                rc = L.vd_window_begin(model._handle, B, T, _lib.ptr(bufs["x"]), _lib.ptr(bufs["obs_src"]), _lib.ptr(bufs["obs_mask"]),
                                       _lib.ptr(bufs["latent_mask"]), _lib.ptr(bufs["kinda_marg_mask"]), _lib.ptr(bufs["frame_indices"]), 0, 1, 1,
                                       0.0, 0, 0, diff.num_timesteps - 1, plain.stream.cuda_stream)
                with pytest.raises(_lib.VdError, match="FreeU .vd_set_freeu. together with the window " + opt.replace("_", " ")):
                    _lib.check(rc)
            finally:
                _lib.check(getattr(L, setter)(model._handle, 0))
    assert freeu_state(model) == OFF
    # outside the scope the same calls are served
    assert torch.isfinite(diff.eps_vjp(model, xd, td, cot, kd)["vjp"]).all()
    assert torch.isfinite(diff.score_windows(model, kd["x0"], td, kd, None, 1, [0] * B)).all()
    # constants: finite and > 0, on the Python side and in the engine
    for bad in (0.0, -1.2, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite and > 0"):
            diff.freeu_scope(model, b1=1.4, b2=bad)
        assert L.vd_set_freeu(model._handle, 1.4, 1.2, bad, 0.8, 0) != 0 and b"finite and > 0" in L.vd_last_error()
        assert freeu_state(model) == OFF
    # the setting is back after a block that raised, and scopes nest
    with pytest.raises(RuntimeError, match="inside"):
        with diff.freeu_scope(model, **FU):
            with diff.freeu_scope(model, b1=2.0, adaptive=True):
                assert freeu_state(model) == ((2.0, 1.0, 1.0, 1.0), True)
            assert freeu_state(model) == ((*B_CONST, *S_CONST), False)
            raise RuntimeError("inside")
    assert freeu_state(model) == OFF
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- command line
def test_video_sample_writes_what_infer_video_returns(tmp_path, monkeypatch):
    """`video_sample.run()` -- the body of the command line -- with --freeu on a tiny checkpoint file: the .npy files of the suffixed run
    directory are infer_video's return for the same arguments (ddim at eta = 0 draws no noise), as uint8."""
    from argparse import Namespace
    from video_diffusion_amd import video_sample as vs
    model, diff = engine("tiny")
    cfg = model_cfg("tiny")
    ck = tmp_path / "my-checkpoints" / "exp7" / "ema_0.9999_latest.pt"
    ck.parent.mkdir(parents=True)
    saved_cfg = {k: v for k, v in cfg.items() if k != "timestep_respacing"}
    saved_cfg.update(timestep_respacing="", max_frames=4)
    torch.save({"state_dict": synth_sd(model.param_specs()), "config": saved_cfg, "step": 1234}, ck)
    vids = torch.rand(2, 6, 3, 32, 32, generator=torch.Generator().manual_seed(90)) * 2 - 1
    np.save(tmp_path / "videos.npy", vids.numpy())
    monkeypatch.chdir(tmp_path)
    fu = [1.4, 1.2, 0.6, 0.8]
    args = Namespace(checkpoint_path=str(ck), videos=str(tmp_path / "videos.npy"), synthetic=False, inference_mode="autoreg",
                     T=None, max_frames=None, obs_length=2, step_size=2, batch_size=2, num_videos=0, timestep_respacing="ddim10",
                     observed_frames="x_0", image_size=32, num_channels=32, num_res_blocks=1, seed=0, adaptive_distance="l2",
                     executor="eager", eval_dir=None, out_dir=None, use_ddim=False, sample_idx=None, num_samples=1, indices=None,
                     task_id=None, subset_size=None, optimality=None, use_gradient_method=False, save_all_timesteps=False,
                     sampler="ddim", eta=0.0, freeu=fu, freeu_adaptive=True)
    out = vs.run(args, device=torch.device("cuda", 0))
    assert str(out).endswith("_ddim_freeu1.4-1.2-0.6-0.8a"), out
    want = vs.to_uint8(vs.infer_video("autoreg", model, diff, vids.cuda(), 4, 2, 2, sampler="ddim", freeu=tuple(fu), freeu_adaptive=True)[0])
    plain = vs.to_uint8(vs.infer_video("autoreg", model, diff, vids.cuda(), 4, 2, 2, sampler="ddim")[0])
    assert not np.array_equal(want, plain)
    for i in range(2):
        got = np.load(tmp_path / out / "samples" / f"sample_{i:04d}-0.npy")
        assert got.dtype == np.uint8 and np.array_equal(got, want[i])
    assert freeu_state(model) == OFF
