"""GPU: guidance rescale and dynamic thresholding (this project's extensions; csrc/guidance.hip) -- the two op entries per element against
their float64 restatements (tests/guidance_restated.py), the steps inside `guidance_scope` against a composition of existing entries to
the bit, the window graph, the scope's state and the refusals.  Every bound is derived in guidance_restated.py, none is measured."""
import ctypes
import json

import numpy as np
import pytest
import torch

import video_diffusion_amd as vda
from guidance_restated import rescale_factor_fp64, threshold_fp64
from helpers import synth_sd
from step_compose import _combine, _compose, _kw, _rescale, _threshold
from video_diffusion_amd import _lib
from video_diffusion_amd.executor import WindowExecutor

pytestmark = pytest.mark.gpu
KEYS = vda.video_model_and_diffusion_defaults().keys()
_cache = {}
TINY = dict(T=6, image_size=32, num_channels=32, num_res_blocks=1, rp_alpha=6, rp_beta=6, rp_gamma=6, timestep_respacing="ddim10")
B, T, S = 2, 6, 32
FE = 3 * S * S
SHAPES = [(3, 5, 192), (2, 4, 105), (2, 16, 12288)]      # small; a frame that is no multiple of 4 (element by element); many blocks per item


def _bits(t):
    return t.contiguous().view(torch.int32)


def _masks(shape, kind):
    """'edge': item 0 has no latent frame, item 1 a single one (its second frame), any further item is mixed;  'mixed': every item has
    latent frames between other ones."""
    b, t, _ = shape
    lat = np.zeros((b, t), np.float32)
    for i in range(b):
        if kind == "edge" and i == 0:
            continue
        if kind == "edge" and i == 1:
            lat[i, 1] = 1
        else:
            lat[i, 1 + (i % 2)::2] = 1
    return lat


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------- the rescale op
def _rescale_inputs(shape, data):
    g = np.random.default_rng(sum(shape))
    if data == "normal":
        return g.standard_normal(shape).astype(np.float32), (0.6 * g.standard_normal(shape) + 0.1).astype(np.float32)
    if data == "offset":                                  # the mean is 30 times the spread
        return (3.0 + 0.1 * g.standard_normal(shape)).astype(np.float32), (3.0 + 0.1 * g.standard_normal(shape)).astype(np.float32)
    flat = np.full(shape, 0.3, np.float32)                # sigma_g = 0: out_c = out_u = a constant, whatever w is
    return flat, flat.copy()


@pytest.mark.parametrize("data", ["normal", "offset", "flat"])
@pytest.mark.parametrize("kind", ["edge", "mixed"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rescale_op_against_float64(shape, kind, data):
    """vd_op_cfg_rescale against the float64 rescale of the float32 bits vd_op_cfg_combine returns for the same inputs: the factor within
    2^-24 relative of the float64 one (its one rounding to float32), every latent output within 1.01 2^-23 |ref| (that rounding and the
    product's), every other output the combine's bits, and two runs the same bits."""
    c_np, u_np = _rescale_inputs(shape, data)
    lat_np = _masks(shape, kind)
    c, u, lat = _dev(c_np), _dev(u_np), _dev(lat_np)
    m = np.broadcast_to((lat_np == 1)[:, :, None], shape)
    worst_f = worst_o = 0.0
    for w in (0.0, 2.0, -0.5, 7.5):
        g = _combine(c, u, w)
        g_np = g.cpu().numpy()
        for phi in (0.3, 0.7, 1.0):
            out, f = _rescale(c, u, w, lat, phi)
            f64 = rescale_factor_fp64(c_np, g_np, lat_np, np.float32(phi))
            f_np, out_np = f.cpu().numpy().astype(np.float64), out.cpu().numpy().astype(np.float64)
            err_f = np.abs(f_np - f64) / np.abs(f64)
            worst_f = max(worst_f, float(err_f.max()))
            assert (err_f <= 2.0 ** -24).all(), (w, phi, f_np, f64)
            if kind == "edge":
                assert f_np[0] == 1.0                                             # no latent frame
            if data == "flat":
                assert (f_np == 1.0).all()                                        # sigma_g = 0
            ref = g_np.astype(np.float64) * f64[:, None, None]
            err = np.abs(out_np - ref)[m]
            lim = (1.01 * 2.0 ** -23 * np.abs(ref))[m]
            if err.size:
                worst_o = max(worst_o, float((err / np.maximum(np.abs(ref[m]), 1e-300)).max()))
            assert (err <= lim).all(), (w, phi, float((err - lim).max()))
            assert torch.equal(_bits(out)[torch.from_numpy(~m).cuda()], _bits(g)[torch.from_numpy(~m).cuda()])
            again, f2 = _rescale(c, u, w, lat, phi)
            assert torch.equal(_bits(again), _bits(out)) and torch.equal(_bits(f2), _bits(f))
        # in place over out_c, as the step runs it
        cc = c.clone()
        inplace, _ = _rescale(cc, u, w, lat, 0.7, out=cc)
        assert torch.equal(_bits(inplace), _bits(_rescale(c, u, w, lat, 0.7)[0]))
    print(f"{shape} {kind} {data}: worst factor error {worst_f / 2.0 ** -24:.3f} x 2^-24, worst output error {worst_o / 2.0 ** -23:.3f} x 2^-23")


# ---------------------------------------------------------------------------------------------------------------- the threshold op
def _threshold_input(shape, lat, data):
    g = np.random.default_rng(sum(shape) + 1)
    if data in ("gauss3", "nan_latent", "nan_observed"):
        x = (3.0 * g.standard_normal(shape)).astype(np.float32)
        b = shape[0] - 1                                                          # the last item: 'edge' gives it one latent frame (B = 2) or a mixed set
        frames = np.flatnonzero(lat[b] == (1 if data == "nan_latent" else 0))
        if data != "gauss3":
            x[b, frames[-1], shape[2] // 2] = np.nan
        return x
    if data == "half_to_one":                                                     # every high radix digit the same; s = 1
        return (g.uniform(0.5, 1.0, shape) * g.choice([-1.0, 1.0], shape)).astype(np.float32).clip(-0.99999994, 0.99999994)
    if data == "quantised":                                                       # 16 levels: heavy ties around every rank
        return (g.integers(-8, 8, shape) / 4.0).astype(np.float32)
    x = np.zeros(shape, np.float32)                                               # zeros of both signs and denormals; s = 1
    flat = x.reshape(-1)
    flat[::3] = -0.0
    flat[1::5] = g.integers(1, 2 ** 23, flat[1::5].size).astype(np.uint32).view(np.float32)
    flat[2::7] *= -1
    return x


@pytest.mark.parametrize("data", ["gauss3", "half_to_one", "quantised", "zeros_denormals", "nan_latent", "nan_observed"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_threshold_op_against_float64(shape, data):
    """vd_op_dynamic_threshold for p in {0.5, 0.995, 1}: s_out is np.float32 of the restated float64 s EXACTLY (the order statistics are
    exact and the interpolation is the same three float64 operations, rounded once to float32; no allowance proved necessary), every
    latent output within 2^-24 relative of clamp(x, -s, s) / s in float64 (one division), every other output clamp(x, -1, 1) to the bit,
    and where s = 1 the whole output is that clamp to the bit.  A NaN on a latent frame poisons that item's latent frames and nothing
    else; a NaN on another frame poisons nothing."""
    for kind in ("edge", "mixed"):
        lat_np = _masks(shape, kind)
        x_np = _threshold_input(shape, lat_np, data)
        x, lat = _dev(x_np), _dev(lat_np)
        m = np.broadcast_to((lat_np == 1)[:, :, None], shape)
        clamp = torch.clamp(x, -1.0, 1.0)
        for p in (0.5, 0.995, 1.0):
            out, s = _threshold(x, lat, p)
            ref, s32 = threshold_fp64(x_np, lat_np, np.float32(p))
            s_np, out_np = s.cpu().numpy(), out.cpu().numpy()
            assert np.array_equal(s_np, s32, equal_nan=True), (p, s_np, s32)
            if kind == "edge":
                assert s_np[0] == 1.0                                             # no latent frame
            poisoned = np.isnan(s32)
            assert poisoned.any() == (data == "nan_latent")
            if data in ("half_to_one", "zeros_denormals"):
                assert (s_np == 1.0).all()
            if data == "gauss3" and p > 0.5:
                assert (s_np[lat_np.any(axis=1)] > 1.0).all()                     # (the threshold does act)
            # latent frames
            o64 = out_np.astype(np.float64)
            assert np.array_equal(np.isnan(o64[m]), np.isnan(ref[m]))
            ok = m & ~np.isnan(ref)
            assert (np.abs(o64 - ref)[ok] <= 2.0 ** -24 * np.abs(ref)[ok]).all(), (p, float(np.abs(o64 - ref)[ok].max()))
            for b in np.flatnonzero(poisoned):
                assert np.isnan(out_np[b][m[b]]).all()
            # the other frames: the static clamp to the bit, a NaN left as it is
            rest = torch.from_numpy(~m).cuda() & ~torch.isnan(x)
            assert torch.equal(_bits(out)[rest], _bits(clamp)[rest])
            assert torch.isnan(out[torch.from_numpy(~m).cuda() & torch.isnan(x)]).all()
            # s = 1: the clamped tensor to the bit, latent frames included
            one = torch.from_numpy(np.broadcast_to((s32 == 1.0)[:, None, None], shape).copy()).cuda() & ~torch.isnan(x)
            assert torch.equal(_bits(out)[one], _bits(clamp)[one])
            again, s2 = _threshold(x, lat, p)
            assert torch.equal(_bits(again), _bits(out)) and torch.equal(_bits(s2), _bits(s))
        xx = x.clone()
        inplace, _ = _threshold(xx, lat, 0.995, out=xx)
        assert torch.equal(_bits(inplace), _bits(_threshold(x, lat, 0.995)[0]))


# ---------------------------------------------------------------------------------------------------------------- the steps
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


def _window(seed):
    """Item 0: frames 0-1 observed, frame 2 kinda-marginalised, frames 3-4 latent, frame 5 padding; item 1: nothing observed, frames 0-4
    latent, frame 5 padding."""
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(B, T, 3, S, S, generator=g) * 2 - 1
    obs, lat, km = torch.zeros(B, T, 1, 1, 1), torch.zeros(B, T, 1, 1, 1), torch.zeros(B, T, 1, 1, 1)
    obs[0, :2] = 1
    km[0, 2] = 1
    lat[0, 3:5] = 1
    lat[1, :5] = 1
    x0 = x0 * obs
    x = 1.5 * torch.randn(B, T, 3, S, S, generator=g)
    return dict(x=x.cuda(), x0=x0.cuda(), obs_mask=obs.cuda(), latent_mask=lat.cuda(), kinda_marg_mask=km.cuda(),
                frame_indices=torch.arange(T).view(1, T).repeat(B, 1).cuda(),
                xtm1=(0.5 * x0 + 0.1 * torch.randn(B, T, 3, S, S, generator=g) * obs).cuda())


def _t(v):
    return torch.tensor([v] * B, device="cuda")


def _noise(seed):
    return torch.randn(B, T, 3, S, S, generator=torch.Generator().manual_seed(seed)).cuda()


def _state(model):
    L = _lib.lib()
    return float(L.vd_cfg_scale(model._handle)), float(L.vd_guidance_rescale(model._handle)), float(L.vd_dynamic_threshold(model._handle))


@pytest.mark.parametrize("start_x", [False, True], ids=["eps", "predict_xstart"])
@pytest.mark.parametrize("w,phi,p", [(2.0, 0.7, None), (2.0, 0.0, 0.995), (2.0, 0.7, 0.995), (1.0, 0.7, 0.9), (-0.5, 1.0, 1.0)])
def test_steps_in_the_scope_equal_the_composition_to_the_bit(start_x, w, phi, p):
    model, diff = tiny(predict_xstart=True) if start_x else tiny()
    diff._bind(model)
    c = _window(50)
    kw, nz = _kw(c), _noise(51)
    prev = (0.3 * c["x"]).clamp(-1, 1)
    want = {("p", 0.0): _compose(model, diff, c, 5, w, phi, p, 0, 0.0, nz, start_x),
            ("ddim", 0.5): _compose(model, diff, c, 5, w, phi, p, 1, 0.5, nz, start_x),
            ("reverse", 0.0): _compose(model, diff, c, 5, w, phi, p, 2, 0.0, nz, start_x),
            ("2m", 0.0): _compose(model, diff, c, 5, w, phi, p, 3, 0.0, nz, start_x, prev)}
    assert _state(model) == (1.0, 0.0, 0.0)
    with diff.guidance_scope(model, cfg_rescale=phi, dynamic_threshold=p):
        assert _state(model)[1:] == (float(np.float32(phi)), float(np.float32(p or 0.0)))
        got = {("p", 0.0): diff._step(0, model, c["x"], _t(5), True, None, kw, 0.0, nz, cfg_scale=w),
               ("ddim", 0.5): diff._step(1, model, c["x"], _t(5), True, None, kw, 0.5, nz, cfg_scale=w)}
        with diff.cfg_scale_scope(model, w):
            o = diff.ddim_reverse_sample(model, c["x"], _t(5), model_kwargs=kw)
            got["reverse", 0.0] = (o["sample"], o["pred_xstart"])
            o = diff.dpmpp_2m_sample(model, c["x"], _t(5), prev_xstart=prev, model_kwargs=kw)
            got["2m", 0.0] = (o["sample"], o["pred_xstart"])
        # the public names draw from torch's generator
        torch.manual_seed(9)
        pub = diff.p_sample(model, c["x"], _t(5), model_kwargs=kw, cfg_scale=w)
        pmv = diff.p_mean_variance(model, c["x"], _t(5), model_kwargs=kw, cfg_scale=w)
    assert _state(model) == (1.0, 0.0, 0.0)
    for key, (sample, xstart) in got.items():
        ws, wx, s = want[key]
        assert torch.equal(_bits(xstart), _bits(wx)), (key, float((xstart - wx).abs().max()))
        assert torch.equal(_bits(sample), _bits(ws)), (key, float((sample - ws).abs().max()))
    assert torch.equal(_bits(pub["pred_xstart"]), _bits(want["p", 0.0][1])) and torch.equal(_bits(pmv["pred_xstart"]), _bits(want["p", 0.0][1]))
    # the options do act: against the plain step at the same scale, the latent frames differ and every other frame keeps its bits
    plain = diff._step(0, model, c["x"], _t(5), True, None, kw, 0.0, nz, cfg_scale=w)[1]
    fused = got["p", 0.0][1]
    lat = c["latent_mask"].reshape(B, T).bool()
    s = want["p", 0.0][2]
    print(f"w={w} phi={phi} p={p}: thresholds {None if s is None else s.tolist()}, max |x_0 - plain x_0| on latent frames "
          f"{float((fused - plain)[lat].abs().max()):.3e}")
    assert torch.equal(_bits(fused[~lat]), _bits(plain[~lat]))
    acts = (phi != 0.0 and w != 1.0) or (p is not None and bool((s > 1.0).any()))
    assert acts and not torch.equal(fused[lat], plain[lat])
    if p is not None:
        assert float(fused[lat].abs().max()) <= 1.0
    model.check_device_errors()


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


def test_options_off_is_the_step_as_it_was():
    """Inside a scope with both options off, with a rescale but cfg_scale = 1, and with a threshold but clip_denoised off, a step is the
    step outside any scope: the same bits and the same launches."""
    model, diff = tiny()
    c = _window(20)
    kw, nz = _kw(c), _noise(21)
    step = lambda clip=True, w=1.0: diff._step(0, model, c["x"], _t(7), clip, None, kw, 0.0, nz, cfg_scale=w)  # noqa: E731
    plain, n_plain = _launches(model, step)
    plain2, n_plain2 = _launches(model, lambda: step(w=2.0))
    unclipped = step(clip=False)
    with diff.guidance_scope(model):
        off, n_off = _launches(model, step)
        off2, n_off2 = _launches(model, lambda: step(w=2.0))
    with diff.guidance_scope(model, cfg_rescale=0.7):
        resc1, n_resc1 = _launches(model, step)                                  # accepted, a no-op at cfg_scale = 1
    with diff.guidance_scope(model, dynamic_threshold=0.9):
        thr_unclipped = step(clip=False)
    for a, b in ((off, plain), (off2, plain2), (resc1, plain), (thr_unclipped, unclipped)):
        assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
    assert n_off == n_plain and n_off2 == n_plain2 and n_resc1 == n_plain
    assert _state(model) == (1.0, 0.0, 0.0)
    model.check_device_errors()


def test_a_latent_value_that_is_not_finite_poisons_the_item_and_sets_the_flag():
    model, diff = tiny()
    c = _window(25)
    kw, nz = _kw(c), _noise(26)
    x = c["x"].clone()
    x[0, 3, 1, 4, 4] = float("inf")                                              # a latent frame of item 0: its x_0 is not finite there
    with diff.guidance_scope(model, dynamic_threshold=0.995):
        _, xstart = diff._step(0, model, x, _t(5), True, None, kw, 0.0, nz)
    lat = c["latent_mask"].reshape(B, T).bool()
    assert torch.isnan(xstart[0][lat[0]]).all() and torch.isfinite(xstart[1]).all()                # every latent element of item 0, nothing of item 1
    with pytest.raises(FloatingPointError, match="not finite"):
        model.check_device_errors()
    model.check_device_errors()                                                  # (reading the flags cleared them)


# ---------------------------------------------------------------------------------------------------------------- the window graph
def _eager_window(model, diff, c, kw, sampler, seed):
    """The window's steps one by one through the C entries under the engine's current state, with the window's own Philox offsets."""
    L = _lib.lib()
    cur = c["x"].clone()
    per = cur[0].numel()
    k = model._pack_kwargs(cur, kw)
    prev = None
    for step, ti in enumerate(range(diff.num_timesteps)[::-1]):
        t = _t(ti)
        nxt = torch.empty_like(cur)
        args = (model._handle, B, T, _lib.ptr(cur), _lib.ptr(k["obs_src"]), _lib.ptr(k["obs_mask"]), _lib.ptr(k["latent_mask"]),
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
    return cur


@pytest.mark.parametrize("sampler", ["p_sample", "ddim", "dpmpp_2m"])
def test_window_graph_equals_the_eager_loop_and_is_keyed_by_both_options(sampler):
    model, diff = tiny()
    diff._bind(model)
    ex = WindowExecutor(model, diff)
    c = _window(70)
    kw, seed = _kw(c), 4321
    L = _lib.lib()
    run = lambda w: ex.begin(c["x"], kw, seed=seed, sampler=sampler, eta=0.5, renoise=False, cfg_scale=w).run().clone()  # noqa: E731
    plain = run(2.0)
    g0 = ex.graphs
    with diff.guidance_scope(model, cfg_rescale=0.7, dynamic_threshold=0.995):
        ex.begin(c["x"], kw, seed=seed, sampler=sampler, eta=0.5, renoise=False, cfg_scale=2.0)
    got = ex.run().clone()                                                       # the graph keeps the values: run() needs no scope
    assert ex.graphs == g0 + 1 and _state(model) == (1.0, 0.0, 0.0)
    with diff.guidance_scope(model, cfg_rescale=0.7, dynamic_threshold=0.995), diff.cfg_scale_scope(model, 2.0):
        want = _eager_window(model, diff, c, kw, sampler, seed)
    assert torch.equal(_bits(got), _bits(want)) and torch.isfinite(got).all(), float((got - want).abs().max())
    lat = c["latent_mask"].reshape(B, T).bool()
    assert not torch.equal(got[lat], plain[lat])
    with diff.guidance_scope(model, cfg_rescale=0.7, dynamic_threshold=0.995):
        assert torch.equal(_bits(run(2.0)), _bits(got)) and ex.graphs == g0 + 1  # the same phi and p: the captured graph again
    with diff.guidance_scope(model, cfg_rescale=0.3, dynamic_threshold=0.995):
        other_phi = run(2.0)
    assert ex.graphs == g0 + 2 and not torch.equal(other_phi[lat], got[lat])
    with diff.guidance_scope(model, cfg_rescale=0.7, dynamic_threshold=0.5):
        other_p = run(2.0)
    assert ex.graphs == g0 + 3 and not torch.equal(other_p[lat], got[lat])
    assert torch.equal(_bits(run(2.0)), _bits(plain)) and ex.graphs == g0 + 3    # outside: the plain guided window, its first graph
    assert _state(model) == (1.0, 0.0, 0.0)
    model.check_device_errors()


def test_infer_video_graph_and_eager_agree_to_the_bit():
    from video_diffusion_amd.video_sample import infer_video
    model, diff = tiny()
    g = torch.Generator().manual_seed(80)
    batch = (torch.rand(2, 10, 3, 32, 32, generator=g) * 2 - 1).cuda()
    run = lambda **o: infer_video("autoreg", model, diff, batch, 6, 2, 4, sampler="ddim", **o)[0]  # noqa: E731
    opts = dict(cfg_scale=2.0, cfg_rescale=0.7, dynamic_threshold=0.995)
    eager = run(executor="eager", **opts)
    graph = run(executor="graph", **opts)
    assert eager.shape == (2, 10, 3, 32, 32) and np.isfinite(eager).all() and np.array_equal(eager, graph)
    guided = run(executor="eager", cfg_scale=2.0)
    assert np.array_equal(run(executor="graph", cfg_scale=2.0, cfg_rescale=0.0, dynamic_threshold=None), guided)      # the defaults: the run as it was
    assert not np.array_equal(eager, guided) and np.array_equal(eager[:, :2], batch[:, :2].cpu().numpy())
    assert np.array_equal(run(executor="eager", dynamic_threshold=0.9), run(executor="graph", dynamic_threshold=0.9))  # at cfg_scale = 1 too
    assert _state(model) == (1.0, 0.0, 0.0)
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- state and refusals
def test_state_is_restored_also_when_the_body_raises():
    model, diff = tiny()
    with pytest.raises(RuntimeError, match="boom"):
        with diff.guidance_scope(model, cfg_rescale=0.5, dynamic_threshold=0.9):
            assert _state(model) == (1.0, 0.5, float(np.float32(0.9)))
            with diff.guidance_scope(model, cfg_rescale=1.0):
                assert _state(model) == (1.0, 1.0, 0.0)
            assert _state(model) == (1.0, 0.5, float(np.float32(0.9)))
            raise RuntimeError("boom")
    assert _state(model) == (1.0, 0.0, 0.0)
    with pytest.raises(IndexError):
        with diff.guidance_scope(model, dynamic_threshold=1.0):
            diff.p_sample(model, torch.zeros(B, T, 3, S, S), torch.tensor([99] * B), model_kwargs=_kw(_window(1)))
    assert _state(model) == (1.0, 0.0, 0.0)


def test_the_three_refusals_name_both_parties():
    model, diff = tiny()
    c = _window(75)
    kw = _kw(c)
    L = _lib.lib()
    for opt, setter in (("prefix_cache", "vd_set_window_prefix_cache"), ("suffix_skip", "vd_set_window_suffix_skip")):
        ex = WindowExecutor(model, diff, **{opt: True})
        with diff.guidance_scope(model, cfg_rescale=0.7):
            # the rescale acts only beside cfg_scale != 1, which these two switches refuse first: the same refusal, by the scale's name
            with pytest.raises(NotImplementedError, match=f"{opt} together with cfg_scale"):
                ex.begin(c["x"], kw, sampler="ddim", cfg_scale=2.0)
            assert torch.isfinite(ex.begin(c["x"], kw, sampler="ddim").run()[:, 3:5]).all()       # cfg_scale = 1: the rescale does not act
        with diff.guidance_scope(model, dynamic_threshold=0.995):
            with pytest.raises(NotImplementedError, match=f"{opt} together with dynamic_threshold"):
                ex.begin(c["x"], kw, sampler="ddim")
        # the C entry itself, the host check bypassed
        plain = WindowExecutor(model, diff)
        plain.begin(c["x"], kw, sampler="ddim")                                  # (its buffers; this call switches both switches off)
        bufs = plain._bufs[B, T]
        begin = lambda: L.vd_window_begin(model._handle, B, T, _lib.ptr(bufs["x"]), _lib.ptr(bufs["obs_src"]), _lib.ptr(bufs["obs_mask"]),  # noqa: E731
                                          _lib.ptr(bufs["latent_mask"]), _lib.ptr(bufs["kinda_marg_mask"]), _lib.ptr(bufs["frame_indices"]), 0, 1, 1,
                                          0.0, 0, 0, diff.num_timesteps - 1, plain.stream.cuda_stream)
        _lib.check(getattr(L, setter)(model._handle, 1))
        try:
            with diff.guidance_scope(model, dynamic_threshold=0.995):
                with pytest.raises(_lib.VdError, match=r"dynamic_threshold .* together with the window " + opt.replace("_", " ")):
                    _lib.check(begin())
            with diff.guidance_scope(model, cfg_rescale=0.7), diff.cfg_scale_scope(model, 1.0 + 2.0 ** -10):
                with pytest.raises(_lib.VdError):
                    _lib.check(begin())
        finally:
            _lib.check(getattr(L, setter)(model._handle, 0))
        assert torch.isfinite(ex.begin(c["x"], kw, sampler="ddim").run()[:, 3:5]).all()           # outside the scopes the switch works as before
    with diff.guidance_scope(model, dynamic_threshold=0.995):
        for f in (diff.p_sample, diff.ddim_sample, diff.ddim_reverse_sample, diff.dpmpp_2m_sample, diff.p_mean_variance):
            with pytest.raises(NotImplementedError, match="denoised_fn together with dynamic_threshold"):
                f(model, c["x"], _t(5), denoised_fn=lambda v: v, model_kwargs=kw)
        diff.p_sample(model, c["x"], _t(5), clip_denoised=False, denoised_fn=lambda v: v, model_kwargs=kw)      # no clamp, nothing to replace
    with diff.guidance_scope(model, cfg_rescale=0.7):                            # the rescale sits in front of the callback: served
        diff.p_sample(model, c["x"], _t(5), denoised_fn=lambda v: v, model_kwargs=kw, cfg_scale=2.0)
    assert _state(model) == (1.0, 0.0, 0.0)
    model.check_device_errors()
