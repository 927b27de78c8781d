"""GPU: zero-shot restoration (this project's extension, DDNM) -- the projection pass per element against the float64 restatement
(tests/measurement_restated.py) inside its derived bound, the step on the network against the plain step + vd_measurement_project +
the sampler pass on the projected x_0, the window graph against the eager chain, infer_video and the video_sample job, and every
refusal by message.  Bit equality or a derived bound throughout; nothing here is tuned on the code under test."""
import numpy as np
import pytest
import torch

from measurement_restated import cell_mean_of, measure_fp64, project_bound, project_f32, second_application_bound
from step_compose import MODES, _eager_chain, _from_xstart, _project
from step_nll_restated import U, ratio
from test_gpu_dpmpp_2m import _rand_window, _t, _window_kw, tiny
from test_gpu_known_region import _bits, _np, _same_bits
from video_diffusion_amd import _lib
from video_diffusion_amd.executor import WindowExecutor
from video_diffusion_amd.gaussian_diffusion import measure

pytestmark = pytest.mark.gpu
STEP_OPERATORS = [(4, False), (1, True)]                                         # "at s = 4 and at gray"


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("H,s,gray", [(8, 2, False), (8, 4, False), (8, 8, False), (12, 4, False), (6, 2, False), (7, 1, True), (8, 2, True)])
def test_projection_per_element(H, s, gray):
    """B = 2, T = 3, frame 1 not latent.  8 x 8 and 12 x 12 take the 16-byte form, 6 x 6 and 7 x 7 the scalar one; at s = 8 a cell is
    the whole 8 x 8 plane."""
    model, diff = tiny()
    B, T = 2, 3
    g = torch.Generator().manual_seed(100 + 10 * s + H)
    x0 = torch.randn(B, T, 3, H, H, generator=g) * 0.8
    y = torch.rand(B, T, 1 if gray else 3, H // s, H // s, generator=g) * 2 - 1
    lat = torch.ones(B, T)
    lat[:, 1] = 0
    xn, yn, ln = _np(x0), _np(y), _np(lat)
    got_d = _project(model, x0, y, lat, s, gray)
    got = _np(got_d)
    want, lim = project_bound(xn, yn, ln, s, gray)
    r = ratio(got, want, lim)
    print(f"H={H} s={s} gray={gray}: max |d| / bound = {r.max():.3f}; f32 restatement equal: {_same_bits(got, project_f32(xn, yn, ln, s, gray))}")
    assert (r <= 1.0).all(), float(r.max())
    assert _same_bits(got[:, 1], xn[:, 1]) and not np.array_equal(got[:, 0], xn[:, 0])       # non-latent frames keep their input bits
    # A(out) = y within the bound (its cell mean: A(out) - y is the cell mean of out - exact)
    a_err = np.abs(measure_fp64(got, s, gray) - yn)
    a_lim = measure_fp64(lim, s, gray)
    print(f"  A(out) - y: max {a_err[:, [0, 2]].max():.3e}, max / bound {(a_err[:, [0, 2]] / a_lim[:, [0, 2]]).max():.3f}")
    assert (a_err[:, [0, 2]] <= a_lim[:, [0, 2]]).all()
    # a second application moves nothing beyond the bound
    again = _np(_project(model, got_d, y, lat, s, gray))
    w2, l2 = second_application_bound(got, yn, ln, s, gray, lim)
    assert (ratio(again, w2, l2) <= 1.0).all() and _same_bits(again[:, 1], xn[:, 1])
    # a rerun, an x_0 4 bytes off alignment (the scalar form) and item b alone: the same bits
    assert _same_bits(_project(model, x0, y, lat, s, gray), got)
    assert _same_bits(_project(model, x0, y, lat, s, gray, misalign=True), got)
    for b in range(B):
        assert _same_bits(_project(model, x0[b:b + 1], y[b:b + 1], lat[b:b + 1], s, gray), got[b:b + 1]), b
    # one cell with an Inf comes out not finite; no other cell is touched
    for bad_v in (float("inf"), float("nan")):
        xi = x0.clone()
        xi[1, 2, 1, H - 1, H - 1] = bad_v
        gi = _np(_project(model, xi, y, lat, s, gray))
        bad = cell_mean_of(np.where(np.isfinite(_np(xi)), 0.0, 1.0), s, gray) > 0
        assert bad.sum() == s * s * (3 if gray else 1) and not np.isfinite(gi[bad]).any()
        assert np.array_equal(_bits(gi)[~bad], _bits(got)[~bad])
    model.check_device_errors()                                                  # the projection sets no error bit of its own


def test_projection_entry_refusals():
    model, diff = tiny()
    L = _lib.lib()
    x = torch.zeros(1, 1, 3, 8, 8, device="cuda")
    y, lat = torch.zeros(1, 1, 3, 8, 8, device="cuda"), torch.ones(1, device="cuda")
    call = lambda H, W, s, gr: L.vd_measurement_project(model._handle, 1, 1, H, W, _lib.ptr(x), _lib.ptr(y), _lib.ptr(lat), s, gr,  # noqa: E731
                                                        _lib.current_stream())
    for s, gr in ((1, 0), (3, 0), (16, 1), (0, 1), (-2, 0)):
        assert call(8, 8, s, gr) != 0 and b"scale is 2, 4 or 8, or 1 together with gray" in L.vd_last_error()
    assert call(6, 8, 4, 0) != 0 and b"divisible by scale" in L.vd_last_error()
    assert call(8, 6, 4, 1) != 0 and b"divisible by scale" in L.vd_last_error()
    assert L.vd_set_measurement(model._handle, _lib.ptr(y), 1, 0) != 0 and b"scale is 2, 4 or 8" in L.vd_last_error()
    assert L.vd_measurement(model._handle, None, None) == 0


# ---------------------------------------------------------------------------------------------------------------- 2
def _window_measurement(c, s, gray, seed):
    """A measurement for the window `c`: A of a random video, so every frame's cells get a target of their own."""
    g = torch.Generator().manual_seed(seed)
    return measure(torch.rand(tuple(c["x"].shape), generator=g) * 2 - 1, s, gray).cuda()


@pytest.mark.parametrize("start_x", [False, True])
@pytest.mark.parametrize("s,gray", STEP_OPERATORS)
@pytest.mark.parametrize("sampler,eta", [("p_sample", 0.0), ("ddim", 0.5), ("dpmpp_2m", 0.0)])
def test_the_step_on_the_network(sampler, eta, s, gray, start_x):
    """B = 2, 2 observed of 6 frames, EPSILON and START_X: the step inside the scope is the plain step's x_0, projected, and the sampler
    pass on it with clip off."""
    model, diff = tiny(predict_xstart=True) if start_x else tiny()
    N = diff.num_timesteps
    c = _rand_window(2, 6, 32, 2, seed=70)
    kw, x = _window_kw(c), c["x"].cuda()
    lat = kw["latent_mask"].reshape(2, 6)
    y = _window_measurement(c, s, gray, seed=71)
    noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(72)).cuda()
    prev = (torch.rand(x.shape, generator=torch.Generator().manual_seed(73)) * 2 - 1).cuda() if sampler == "dpmpp_2m" else None
    mode = MODES[sampler]
    L = _lib.lib()
    for tv in (N - 1, 3, 0):
        tt = _t(2, tv)
        plain, plain_x0 = diff._fused_step(mode, model, x, tt, True, kw, eta=eta, noise=noise, prev_xstart=prev)
        with diff.measurement_scope(model, y, s, gray):
            assert L.vd_measurement(model._handle, None, None) == 1
            got, got_x0 = diff._fused_step(mode, model, x, tt, True, kw, eta=eta, noise=noise, prev_xstart=prev)
            pmv = diff.p_mean_variance(model, x, tt, clip_denoised=True, model_kwargs=kw)
            free, free_x0 = diff._fused_step(mode, model, x, tt, False, kw, eta=eta, noise=noise, prev_xstart=prev)
        assert L.vd_measurement(model._handle, None, None) == 0
        want_x0 = _project(model, plain_x0, y, lat, s, gray)
        assert torch.equal(got_x0, want_x0) and not torch.equal(got_x0, plain_x0)                  # pred_xstart: the projected x_0
        assert torch.equal(got_x0[:, :2], plain_x0[:, :2])                                          # observed frames: unprojected
        want, want_xs = _from_xstart(model, mode, x, want_x0, tt, eta, noise, prev)
        assert torch.equal(got, want) and torch.equal(want_xs, want_x0), float((got - want).abs().max())
        assert torch.equal(pmv["pred_xstart"], want_x0)                                             # p_mean_variance agrees
        assert torch.equal(pmv["mean"], _from_xstart(model, 0, x, want_x0, tt, 0.0, None, None, want_mean=True))
        if tv == 0:                                                              # the last step returns x_0 itself: A(sample) = y
            assert torch.equal(got, got_x0)
        # clip_denoised=False: the same step with denoised_fn = the projection
        fn = lambda v: _project(model, v, y, lat, s, gray)                       # noqa: E731
        if mode == 3:
            o = diff.dpmpp_2m_sample(model, x, tt, prev_xstart=prev, clip_denoised=False, denoised_fn=fn, model_kwargs=kw)
            via, via_x0 = o["sample"], o["pred_xstart"]
        else:
            via, via_x0 = diff._step(mode, model, x, tt, False, fn, kw, eta, noise)
        assert torch.equal(free, via) and torch.equal(free_x0, via_x0), float((free - via).abs().max())
        again, again_x0 = diff._fused_step(mode, model, x, tt, True, kw, eta=eta, noise=noise, prev_xstart=prev)
        assert torch.equal(again, plain) and torch.equal(again_x0, plain_x0)     # behind the scope: the plain step's bits
    model.check_device_errors()


@pytest.mark.parametrize("s,gray", STEP_OPERATORS)
def test_the_step_under_guidance(s, gray):
    """cfg_scale = 2 with dynamic thresholding: network (two forwards, combine), threshold, projection, sampler pass -- in that order."""
    model, diff = tiny()
    N = diff.num_timesteps
    c = _rand_window(2, 6, 32, 2, seed=74)
    kw, x = _window_kw(c), c["x"].cuda()
    lat = kw["latent_mask"].reshape(2, 6)
    y = _window_measurement(c, s, gray, seed=75)
    noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(76)).cuda()
    for mode, tv in ((0, N - 2), (1, 2), (3, 0)):
        tt = _t(2, tv)
        with diff.guidance_scope(model, dynamic_threshold=0.9):
            _, thr_x0 = diff._fused_step(mode, model, x, tt, True, kw, noise=noise, cfg_scale=2.0)
            with diff.measurement_scope(model, y, s, gray):
                got, got_x0 = diff._fused_step(mode, model, x, tt, True, kw, noise=noise, cfg_scale=2.0)
        _, unguided_x0 = diff._fused_step(mode, model, x, tt, True, kw, noise=noise)
        assert not torch.equal(thr_x0, unguided_x0)
        want_x0 = _project(model, thr_x0, y, lat, s, gray)
        want, _ = _from_xstart(model, mode, x, want_x0, tt, 0.0, noise, None)
        assert torch.equal(got_x0, want_x0) and torch.equal(got, want), (mode, float((got - want).abs().max()))
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("sampler,eta", [("p_sample", 0.0), ("ddim", 0.5), ("dpmpp_2m", 0.0)])
def test_window_graph(sampler, eta):
    """begin(measurement=...), run(): to the bit the eager chain of steps inside the scope; one graph per (signature, scale, gray);
    a window without a measurement on the same executor is the plain window."""
    model, diff = tiny()
    diff._bind(model)
    N = diff.num_timesteps
    ex = WindowExecutor(model, diff)
    ops = [("step", tv) for tv in range(N - 1, -1, -1)]
    counts = []
    for wi, (s, gray) in enumerate(STEP_OPERATORS + STEP_OPERATORS[:1]):
        c = _rand_window(2, 6, 32, 2, seed=500 + wi)
        kw, x_init = _window_kw(c), c["x"].cuda()
        y = _window_measurement(c, s, gray, seed=510 + wi)
        ex.begin(x_init, kw, sampler=sampler, eta=eta, seed=80 + wi, measurement=y, sr_scale=s, gray=gray)
        assert _lib.lib().vd_measurement(model._handle, None, None) == 0          # engine state for the length of begin() only
        counts.append(ex.graphs)
        got = ex.run().clone()
        with diff.measurement_scope(model, y, s, gray):
            want, _ = _eager_chain(model, diff, sampler, eta, x_init, kw, None, None, 80 + wi, ops)
        assert torch.equal(want, got) and torch.isfinite(got).all(), (wi, float((want - got).abs().max()))
        a_err = np.abs(measure_fp64(_np(got), s, gray) - _np(y))[:, 2:]
        assert (a_err <= _final_bound(_np(got), _np(y), s, gray)[:, 2:]).all()   # the window ends on the measurement
    assert counts[1] == counts[0] + 1 and counts[2] == counts[1]                 # the third window found the first one's graph
    # a begin() inside the scope takes the scope's measurement
    c = _rand_window(2, 6, 32, 2, seed=520)
    kw, x_init = _window_kw(c), c["x"].cuda()
    s, gray = STEP_OPERATORS[0]
    y = _window_measurement(c, s, gray, seed=521)
    with diff.measurement_scope(model, y, s, gray):
        ex.begin(x_init, kw, sampler=sampler, eta=eta, seed=90)
        assert _lib.lib().vd_measurement(model._handle, None, None) == 1
    scoped = ex.run().clone()
    assert ex.graphs == counts[2]
    with diff.measurement_scope(model, y, s, gray):
        want, _ = _eager_chain(model, diff, sampler, eta, x_init, kw, None, None, 90, ops)
    assert torch.equal(scoped, want)
    # without a measurement, on the same executor and buffers: the window as it always was
    ex.begin(x_init, kw, sampler=sampler, eta=eta, seed=90)
    got = ex.run().clone()
    want, _ = _eager_chain(model, diff, sampler, eta, x_init, kw, None, None, 90, ops)
    assert torch.equal(want, got) and not torch.equal(got, scoped)
    model.check_device_errors()


def _final_bound(out, y, s, gray):
    """|A(sample) - y| per cell behind the LAST step, from what is known of its inputs without reading them: the sample is the projected
    x_0 itself (p_sample: coefficients 1 and 0; ddim and dpmpp_2m: alpha_bar_prev = 1), the x_0 it was projected from went through the
    clamp of clip_denoised, so mean_cell|x_0| <= 1 and |y - m| <= |y| + 1; the cell mean of measurement_restated's bound with those."""
    n = s * s * (3 if gray else 1)
    gamma = n * U / (1.0 - n * U)
    return gamma + U * (np.abs(y) + 1.0) + U * measure_fp64(np.abs(out), s, gray)


# ---------------------------------------------------------------------------------------------------------------- 4
def test_infer_video_and_the_job(tmp_path, monkeypatch):
    from video_diffusion_amd import video_sample as vs
    model, diff = tiny()
    g = torch.Generator().manual_seed(60)
    batch = (torch.rand(2, 10, 3, 32, 32, generator=g) * 2 - 1).cuda()
    truth = (torch.rand(2, 10, 3, 32, 32, generator=g) * 2 - 1)
    run = lambda **k: vs.infer_video("autoreg", model, diff, batch, 6, 2, 4, **k)[0]      # noqa: E731
    src = batch.cpu().numpy()
    for (s, gray), sampler, executor in (((4, False), "p_sample", "eager"), ((1, True), "ddim", "graph"), ((4, True), "dpmpp_2m", "eager"),
                                         ((4, False), "dpmpp_2m", "graph"), ((2, False), "ddim", "eager"), ((1, True), "p_sample", "graph")):
        y = measure(truth, s, gray)
        torch.manual_seed(61)
        out = run(sampler=sampler, executor=executor, measurement=y, sr_scale=s, gray=gray, cfg_scale=1.5 if sampler == "ddim" else 1.0)
        assert np.isfinite(out).all() and np.array_equal(out[:, :2], src[:, :2])                 # observed frames: untouched
        a_err = np.abs(measure_fp64(out, s, gray) - y.numpy())[:, 2:]
        lim = _final_bound(out, y.numpy(), s, gray)[:, 2:]
        print(f"s={s} gray={gray} {sampler} {executor}: max |A(out) - y| = {a_err.max():.3e}, max / bound = {(a_err / lim).max():.3f}")
        assert (a_err <= lim).all()
        if (s, gray, sampler) == (4, True, "dpmpp_2m"):                          # without the measurement: other frames, far from y
            plain = run(sampler=sampler, executor=executor)
            assert (np.abs(measure_fp64(plain, s, gray) - y.numpy())[:, 2:] > lim).any()
    # a deterministic sampler: the two executors agree to the bit
    y = measure(truth, 4, True)
    outs = [run(sampler="dpmpp_2m", executor=e, measurement=y, sr_scale=4, gray=True) for e in ("eager", "graph")]
    assert np.array_equal(outs[0], outs[1])
    with pytest.raises(ValueError, match="y must be"):
        run(measurement=y, sr_scale=4, gray=False)
    model.check_device_errors()
    # the job: --measurement, --sr_scale, --gray; the suffixed run directory
    vids = (torch.rand(2, 8, 3, 32, 32, generator=g) * 2 - 1)
    yj = measure(torch.rand(2, 8, 3, 32, 32, generator=g) * 2 - 1, 4, True).numpy()
    np.save(tmp_path / "videos.npy", vids.numpy())
    np.save(tmp_path / "y.npy", yj)
    monkeypatch.chdir(tmp_path)
    args = vs.build_parser().parse_args(
        ["--videos", str(tmp_path / "videos.npy"), "--inference_mode", "autoreg", "--max_frames", "6", "--obs_length", "2", "--step_size", "4",
         "--batch_size", "2", "--timestep_respacing", "logsnr5", "--image_size", "32", "--num_channels", "32", "--num_res_blocks", "1",
         "--sampler", "ddim", "--eval_dir", str(tmp_path / "out"), "--measurement", str(tmp_path / "y.npy"), "--sr_scale", "4", "--gray"])
    out_dir = vs.run(args, device=torch.device("cuda", 0))
    assert str(out_dir).endswith("_ddim_sr4gray")
    for i in range(2):
        f = np.load(out_dir / "samples" / f"sample_{i:04d}-0.npy")
        assert f.dtype == np.uint8 and f.shape == (8, 3, 32, 32) and np.array_equal(f[:2], vs.to_uint8(vids.numpy()[i])[:2])


# ---------------------------------------------------------------------------------------------------------------- 5
def test_every_refusal_by_message():
    model, diff = tiny()
    diff._bind(model)
    N = diff.num_timesteps
    L = _lib.lib()
    c = _rand_window(2, 6, 32, 2, seed=95)
    kw, x = _window_kw(c), c["x"].cuda()
    y = _window_measurement(c, 4, False, seed=96)
    src = torch.zeros_like(x)
    mask = torch.ones(2, 6, 32, 32, device="cuda")
    fn = lambda v: v                                                             # noqa: E731
    with diff.measurement_scope(model, y, 4):
        for call, what in ((lambda: diff.ddim_reverse_sample(model, x, _t(2, 3), model_kwargs=kw), "ddim_reverse_sample inside measurement_scope"),
                           (lambda: diff.p_sample(model, x, _t(2, 3), denoised_fn=fn, model_kwargs=kw), "denoised_fn inside measurement_scope"),
                           (lambda: diff.ddim_sample(model, x, _t(2, 3), denoised_fn=fn, model_kwargs=kw), "denoised_fn inside measurement_scope"),
                           (lambda: diff.dpmpp_2m_sample(model, x, _t(2, 3), denoised_fn=fn, model_kwargs=kw), "denoised_fn inside measurement_scope"),
                           (lambda: diff.p_sample(model, x, _t(2, 3), model_kwargs=kw, use_gradient_method=True),
                            "use_gradient_method inside measurement_scope")):
            with pytest.raises(_lib.VdError, match=what):
                call()
        # the engine refuses the reverse step by name as well
        tt, out = _t(2, 3), torch.empty_like(x)
        pk = model._pack_kwargs(x, kw)
        rc = L.vd_ddim_reverse_sample(model._handle, 2, 6, *model._window_ptrs(x, pk), _lib.ptr(tt), pk["obs_mode"], 1, _lib.ptr(out), None, None,
                                      _lib.current_stream())
        assert rc != 0 and b"ddim_reverse_sample together with a measurement" in L.vd_last_error()
        # a measurement together with a known region, either way round
        with diff.known_region_scope(model, src, mask):
            with pytest.raises(_lib.VdError, match="a measurement .vd_set_measurement. together with a known region"):
                diff.ddim_sample(model, x, _t(2, 3), model_kwargs=kw)
        with pytest.raises(ValueError, match="measurement_scope: y"):
            diff.ddim_sample(model, x[:, :4], _t(2, 3), model_kwargs={k: (v[:, :4] if torch.is_tensor(v) else v) for k, v in kw.items()})
    assert L.vd_measurement(model._handle, None, None) == 0
    # the window: sampler 2, the two switches and a known region
    ex = WindowExecutor(model, diff)
    x_init = c["x"].cuda()
    with pytest.raises(_lib.VdError, match="ddim_reverse_sample together with a measurement"):
        ex.begin(x_init, dict(kw, observed_frames="x_t_minus_1"), sampler="ddim_reverse", renoise=False, measurement=y, sr_scale=4)
    for opt, name in (("prefix_cache", "window prefix cache"), ("suffix_skip", "window suffix skip")):
        with pytest.raises(_lib.VdError, match=f"a measurement .vd_set_measurement. together with the {name}"):
            WindowExecutor(model, diff, **{opt: True}).begin(x_init, kw, measurement=y, sr_scale=4)
        _lib.check(getattr(L, f"vd_set_window_{opt}")(model._handle, 0))
    with pytest.raises(_lib.VdError, match="a measurement .vd_set_measurement. together with a known region"):
        ex.begin(x_init, kw, sampler="ddim", measurement=y, sr_scale=4, known_src=src, known_mask=mask)
    assert L.vd_measurement(model._handle, None, None) == 0 and L.vd_known_region(model._handle) == 0
    with pytest.raises(ValueError, match="y must be"):
        ex.begin(x_init, kw, measurement=y, sr_scale=2)
    # the engine is as it was: a plain window runs
    ex.begin(x_init, kw, sampler="ddim", seed=3)
    assert torch.isfinite(ex.run()).all()
    torch.cuda.synchronize()
    model.check_device_errors()
