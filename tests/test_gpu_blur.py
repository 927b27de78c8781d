"""GPU: deblurring (this project's extension) -- the residual and seed passes and the operator itself per element against the float64
restatement (tests/blur_restated.py) inside its derived bound, a one-hot tap as a pure shift to the bit, the step's gradient against
autograd through the CPU oracle with conv2d at the bars of test_use_gradient_method_vs_oracle_autograd, the step's identities bit for bit
against the plain step, the loop, infer_video and the video_sample job, every refusal by message, and particle steering on the blur:
against a reward_fn that computes the same in torch, graph against eager, 40 frames, and taps changed between two windows.  Nothing here
is tuned on the code under test."""
import numpy as np
import pytest
import torch

import particle_restated as pr
from blur_restated import (SHAPES, apply_bound, assert_unambiguous, blur_f32, deblur_bound, deblur_f32, gaussian_taps, one_hot_taps,
                           random_taps, seed_bound, seed_inputs, shifted)
from helpers import close
from step_nll_restated import ratio, tables
from test_gpu_dpmpp_2m import _rand_window, _t, _window_kw, tiny
from test_gpu_dps import ORACLE_CFG, _dev, _fma32, _plain_xstart
from test_gpu_engine import _oracle
from test_gpu_known_region import _np, _same_bits
from test_gpu_long_window import engine as long_engine, kwargs_of, rand_window, tiny_cfg
from test_gpu_particles import _cfg, _group_window, _margin, _noise, _randn, _tt, G_, K_, T_
import video_diffusion_amd as vda
from video_diffusion_amd import _lib, inference_util
from video_diffusion_amd.executor import WindowExecutor
from video_diffusion_amd.gaussian_diffusion import blur, gaussian_kernel

pytestmark = pytest.mark.gpu


def _seed(model, xt, eps, t, clip, y, lat, w, misalign=False):
    """vd_op_deblur_seed -> (d_eps, d_x, rho, pred_xstart) as numpy arrays."""
    B, T, _, H, W = xt.shape
    x_d, e_d = _dev(xt, misalign), _dev(eps, misalign)
    t_d = torch.as_tensor(t).long().cuda()
    y_d, l_d, w_d = _dev(y, misalign), _dev(lat).reshape(-1).contiguous(), _dev(w)
    outs = [_dev(np.full(xt.shape, 7.0, np.float32), misalign) for _ in range(3)]
    rho = torch.full((B,), 7.0, device="cuda")
    _lib.check(_lib.lib().vd_op_deblur_seed(model._handle, B, T, H, W, _lib.ptr(x_d), _lib.ptr(e_d), _lib.ptr(t_d), 1 if clip else 0,
                                            _lib.ptr(y_d), _lib.ptr(l_d), _lib.ptr(w_d), int(w.shape[0]), _lib.ptr(outs[0]), _lib.ptr(outs[1]),
                                            _lib.ptr(rho), _lib.ptr(outs[2]), _lib.current_stream()))
    return _np(outs[0]), _np(outs[1]), _np(rho), _np(outs[2])


def _apply(x, w, adjoint, misalign=False):
    """vd_op_blur -> numpy."""
    B, T, _, H, W = x.shape
    x_d, w_d = _dev(x, misalign), _dev(w)
    out = _dev(np.full(x.shape, 7.0, np.float32), misalign)
    _lib.check(_lib.lib().vd_op_blur(B, T, H, W, _lib.ptr(x_d), _lib.ptr(w_d), int(w.shape[0]), 1 if adjoint else 0, _lib.ptr(out),
                                     _lib.current_stream()))
    return _np(out)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("H,W,k", SHAPES)
def test_seed_and_operator_per_element(H, W, k, clip):
    """B = 2, T = 3, frame 1 not latent; signed asymmetric random taps and a Gaussian.  Every element of d eps, d_x, rho, A x and A^T x
    inside the derived bound; W = 10 and 7 take the scalar form, every other shape the 16-byte one; (8, 8, 15): the kernel is wider than
    the plane; (72, 68, 5): three tiles of 32 in both directions."""
    model, diff = tiny()
    diff._bind(model)
    tab = tables(diff)
    B, T = 2, 3
    for kind, w in (("random", random_taps(k, seed=500 + k)), ("gaussian", gaussian_taps(k))):
        xt, eps, t, y, lat = seed_inputs(tab, B, T, H, W, w, clip, seed=2000 + 10 * H + W + k)
        assert_unambiguous(tab, xt, eps, t, y, lat, w, clip)
        de, dx, rho, xs = _seed(model, xt, eps, t, clip, y, lat, w)
        lim = deblur_bound(tab, xt, eps, t, y, lat, w, clip)
        f32 = deblur_f32(tab, xt, eps, t, y, lat, w, clip)
        for name, got in (("deps", de), ("dxd", dx), ("rho", rho)):
            want, bound = lim[name]
            r = ratio(got, want, bound)
            print(f"H={H} W={W} k={k} {kind} clip={clip} {name}: max |d| / bound = {r.max():.3f}; f32 restatement equal: {_same_bits(got, f32[name])}")
            assert got.shape == want.shape and (r <= 1.0).all(), (kind, name, float(r.max()))
        assert not de[:, 1].any() and not dx[:, 1].any() and de[:, 0].any() and dx[:, 2].any()       # the frame that is not latent: exactly 0
        assert _same_bits(xs, _plain_xstart(model, xt, eps, t, clip))                                 # pred_xstart: the sampler pass's bits
        if clip:
            beyond = np.abs(f32["x0"]) == 1.0
            assert 0.15 < beyond.mean() < 0.35 and not dx[beyond].any()
        for adj in (False, True):                                                                     # the operator alone, on x_t
            got = _apply(xt, w, adj)
            want, bound = apply_bound(xt, w, adj)
            r = ratio(got, want, bound)
            print(f"H={H} W={W} k={k} {kind} adjoint={adj}: max |d| / bound = {r.max():.3f}; f32 restatement equal: {_same_bits(got, blur_f32(xt, w, adj))}")
            assert (r <= 1.0).all(), (kind, adj, float(r.max()))
            assert _same_bits(got, _apply(xt, w, adj, misalign=True))
        # <A u, v> = <u, A^T v> on the device's own outputs: the two differ by what the per-element bounds allow, summed
        (_, bA), (_, bAt) = apply_bound(xt, w, False), apply_bound(eps, w, True)
        gA, gAt = _apply(xt, w, False).astype(np.float64), _apply(eps, w, True).astype(np.float64)
        u64, v64 = xt.astype(np.float64), eps.astype(np.float64)
        gap, room = abs(float((gA * v64).sum() - (u64 * gAt).sum())), float((bA * np.abs(v64)).sum() + (np.abs(u64) * bAt).sum())
        print(f"H={H} W={W} k={k} {kind}: |<A u, v> - <u, A^T v>| / bound = {gap / room:.3f}")
        assert gap <= room * (1 + 1e-9)
        if kind == "gaussian":
            continue
        # a rerun, inputs 4 bytes off alignment (the scalar form) and item b alone: the same bits
        for again in (_seed(model, xt, eps, t, clip, y, lat, w), _seed(model, xt, eps, t, clip, y, lat, w, misalign=True)):
            assert all(_same_bits(a, b) for a, b in zip(again, (de, dx, rho, xs)))
        for b in range(B):
            alone = _seed(model, xt[b:b + 1], eps[b:b + 1], t[b:b + 1], clip, y[b:b + 1], lat[b:b + 1], w)
            assert all(_same_bits(a, v[b:b + 1]) for a, v in zip(alone, (de, dx, rho, xs))), b
        # an item with no latent frame: rho = 0, no gradient, no NaN; the other item keeps its bits
        lat0 = lat.copy()
        lat0[0] = 0
        de0, dx0, rho0, xs0 = _seed(model, xt, eps, t, clip, y, lat0, w)
        assert rho0[0] == 0 and not de0[0].any() and not dx0[0].any() and np.isfinite(de0).all() and np.isfinite(dx0).all()
        assert _same_bits(de0[1], de[1]) and _same_bits(rho0[1:], rho[1:]) and _same_bits(xs0, xs)
        model.check_device_errors()
        # an index outside the schedule poisons its item as the sampler pass does, and sets the error bit
        tb = t.copy()
        tb[0] = tab["NT"]
        deb, dxb, rhob, xsb = _seed(model, xt, eps, tb, clip, y, lat, w)
        assert np.isnan(deb[0]).all() and np.isnan(dxb[0]).all() and np.isnan(rhob[0]) and np.isnan(xsb[0]).all()
        assert _same_bits(deb[1], de[1]) and _same_bits(dxb[1], dx[1]) and _same_bits(rhob[1:], rho[1:]) and _same_bits(xsb[1], xs[1])
        with pytest.raises(IndexError):
            model.check_device_errors()
        model.check_device_errors()


@pytest.mark.parametrize("H,W,k", SHAPES)
def test_one_hot_tap_is_a_pure_shift_to_the_bit(H, W, k):
    """w = 1 at (c + di, c + dj) off centre: (A x)[i, j] = x[i + di, j + dj] and (A^T x)[i, j] = x[i - di, j - dj], zeros entering at the two
    edges the shift leaves -- orientation and padding, with no bound in sight.  The seed passes then hold the float32 restatement's bits,
    whose r = y - shift(x_0) and A^T r = shift back."""
    model, diff = tiny()
    diff._bind(model)
    tab = tables(diff)
    c = k // 2
    di, dj = -min(c, 3), min(c, 2)
    w = one_hot_taps(k, c + di, c + dj)
    x = np.random.default_rng(k + H).standard_normal((2, 3, 3, H, W)).astype(np.float32)
    fwd, adj = _apply(x, w, False), _apply(x, w, True)
    assert _same_bits(fwd, shifted(x, di, dj)) and _same_bits(adj, shifted(x, -di, -dj))
    if c:
        a, b = min(-di, H), min(dj, W)
        assert not fwd[..., :a, :].any() and not fwd[..., :, W - b:].any()           # rows from above the plane, columns from its right
        assert not adj[..., H - a:, :].any() and not adj[..., :, :b].any()
        if H > a and W > b:
            assert _same_bits(fwd[..., a:, :W - b], x[..., :H - a, b:]) and _same_bits(adj[..., :H - a, b:], x[..., a:, :W - b])
    for clip in (True, False):
        xt, eps, t, y, lat = seed_inputs(tab, 2, 3, H, W, w, clip, seed=3000 + H + W + k)
        assert_unambiguous(tab, xt, eps, t, y, lat, w, clip)
        de, dx, rho, xs = _seed(model, xt, eps, t, clip, y, lat, w)
        f32 = deblur_f32(tab, xt, eps, t, y, lat, w, clip)
        sel = np.broadcast_to(lat.reshape(2, 3, 1, 1, 1) == 1, xt.shape)
        r = np.where(sel, y - shifted(xs, di, dj), np.float32(0))                     # on the kernel's own x_0, one subtraction
        assert _same_bits(xs, f32["x0"]) and _same_bits(r, f32["r"])
        assert _same_bits(rho, f32["rho"]) and _same_bits(de, f32["deps"]) and _same_bits(dx, f32["dxd"])
        g = shifted(r, -di, -dj)                                                      # ... and d_x is a (-(g / rho)) where the clamp passes
        a_ = tab["sr"][t].astype(np.float32).reshape(-1, 1, 1, 1, 1)
        live = sel & (dx != 0)
        assert live.any() and _same_bits(dx[live], (a_ * (-(g / rho.reshape(-1, 1, 1, 1, 1))).astype(np.float32)).astype(np.float32)[live])
    model.check_device_errors()


def test_entry_refusals():
    model, diff = tiny()
    diff._bind(model)
    L = _lib.lib()
    x = torch.zeros(1, 1, 3, 8, 8, device="cuda")
    lat, t = torch.ones(1, device="cuda"), torch.zeros(1, dtype=torch.long, device="cuda")
    w, out = torch.ones(15, 15, device="cuda"), torch.empty_like(x)
    seed = lambda k: L.vd_op_deblur_seed(model._handle, 1, 1, 8, 8, _lib.ptr(x), _lib.ptr(x), _lib.ptr(t), 1, _lib.ptr(x), _lib.ptr(lat),  # noqa: E731
                                         _lib.ptr(w), k, _lib.ptr(out), _lib.ptr(out), None, None, _lib.current_stream())
    op = lambda k, o: L.vd_op_blur(1, 1, 8, 8, _lib.ptr(x), _lib.ptr(w), k, 0, _lib.ptr(o), _lib.current_stream())                       # noqa: E731
    for k in (0, 2, 17, -1):
        assert seed(k) != 0 and b"k odd and 1 <= k <= 15" in L.vd_last_error()
        assert op(k, out) != 0 and b"k odd and 1 <= k <= 15" in L.vd_last_error()
    assert op(3, x) != 0 and b"out == x" in L.vd_last_error()
    assert seed(15) == 0 and op(1, out) == 0
    # the engine's kernel: k == 0 clears; the rules; what is installed
    h = model._handle
    kk = _lib._I(0)
    assert L.vd_blur_kernel(h, kk) == 0 and kk.value == 0
    taps = np.ones((3, 3), np.float32)
    for bad, k, what in ((taps, 2, b"k odd"), (taps, 17, b"k odd"), (None, 3, b"null taps"), (np.zeros((3, 3), np.float32), 3, b"not all be zero"),
                         (np.full((3, 3), np.nan, np.float32), 3, b"must be finite")):
        assert L.vd_set_blur_kernel(h, _lib.ptr(bad), k) != 0 and what in L.vd_last_error()
    assert L.vd_set_particle_blur(h, 1) != 0 and b"no kernel is installed" in L.vd_last_error()
    _lib.check(L.vd_set_blur_kernel(h, _lib.ptr(taps), 3))
    assert L.vd_blur_kernel(h, kk) == 1 and kk.value == 3
    _lib.check(L.vd_set_particle_blur(h, 1))
    assert L.vd_particle_blur(h) == 1 and L.vd_set_blur_kernel(h, None, 0) != 0 and b"switch that off first" in L.vd_last_error()
    _lib.check(L.vd_set_particle_blur(h, 0))
    _lib.check(L.vd_set_blur_kernel(h, None, 0))
    assert L.vd_blur_kernel(h, kk) == 0 and L.vd_particle_blur(h) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 2
def _oracle_grad(ora, c, t, y, w):
    """Steps 2-4 composed in torch on the oracle's network with conv2d -> (grad of sum_b rho_b w.r.t. x_t, rho)."""
    sch = ora.s
    kwo = dict(x0=c["x0"], obs_mask=c["obs_mask"], latent_mask=c["latent_mask"], kinda_marg_mask=c["kinda_marg_mask"],
               frame_indices=c["frame_indices"], x_t_minus_1=c["x0"])
    x = c["x"].detach().clone().requires_grad_(True)
    tm = torch.tensor(sch.timestep_map, dtype=t.dtype)[t]
    coef = lambda tabl: torch.from_numpy(np.asarray(tabl))[t].float().view(-1, 1, 1, 1, 1)      # noqa: E731
    k = w.shape[0]
    with torch.enable_grad():
        eps = ora.net.with_grad(x, tm, **kwo)
        x0 = (coef(sch.sqrt_recip_alphas_cumprod) * x - coef(sch.sqrt_recipm1_alphas_cumprod) * eps).clamp(-1, 1)
        Ax = torch.nn.functional.conv2d(x0.reshape(-1, 1, *x0.shape[-2:]), w.reshape(1, 1, k, k), padding=k // 2).reshape(x0.shape)
        r = (y - Ax) * c["latent_mask"]
        rho = r.reshape(r.shape[0], -1).pow(2).sum(dim=1).sqrt()
        g, = torch.autograd.grad(rho.sum(), x)
    return g, rho.detach()


def _deblur_call(diff, model, mode, x, tt, kw, eta, noise, y, w, zeta):
    with diff.deblur_scope(model, y, w, zeta=zeta):
        diff._step(mode, model, x, tt, True, None, kw, eta, noise)
    return diff._last_dps


@pytest.mark.parametrize("case", [("random7", 0, 0.0, "plain"), ("gauss9", 1, 0.5, "plain"), ("random7", 0, 0.0, "marg_and_padding")],
                         ids=lambda c: f"{c[0]}-mode{c[1]}-{c[3]}")
def test_step_gradient_vs_oracle_autograd(case):
    """The bars are test_use_gradient_method_vs_oracle_autograd's own, as test_gpu_dps.py takes them: the same backward pass against the
    same oracle."""
    kind, mode, eta, masks = case
    cfg = {**vda.video_model_and_diffusion_defaults(), **ORACLE_CFG}
    model, diff, ora = _oracle(cfg)
    c = _rand_window(2, 5, 32, 2, seed=725)
    if masks == "marg_and_padding":
        c["latent_mask"][:, 2] = 0
        c["kinda_marg_mask"][:, 2] = 1
        c["latent_mask"][:, 4] = 0
    w = torch.tensor(random_taps(7, seed=9)) if kind == "random7" else gaussian_kernel(9, 2.0)
    g = torch.Generator().manual_seed(31)
    y = blur(torch.rand(c["x"].shape, generator=g) * 2 - 1, w) + 0.1 * torch.randn(c["x"].shape, generator=g)
    noise = torch.randn(c["x"].shape, generator=g)
    t = torch.tensor([30, 30])
    want, want_rho = _oracle_grad(ora, c, t, y, w)
    kw = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in c.items() if k != "x"}
    kw.update(x_t_minus_1=kw["x0"], observed_frames="x_0")
    out = _deblur_call(diff, model, mode, c["x"].cuda(), t.cuda(), kw, eta, noise, y, w, 0.5)
    scale = float(want.abs().max())
    err = (out["grad"].cpu() - want).abs()
    print(f"{case}: max |grad - ref| = {float(err.max()):.3e} = {float(err.max()) / scale:.3e} max |ref|; rho {out['residual_norm'].tolist()} ref {want_rho.tolist()}")
    assert scale > 0 and not out["grad"][:, :2].any()                           # observed frames: exactly 0
    if masks == "marg_and_padding":
        assert want[:, 4].abs().max() > 0
    close(out["grad"].cpu(), want, atol=2e-4 * scale, rtol=1e-3)
    # residual_norm against the float64 norm of the engine's own pred_xstart, inside the restatement's bound for rho
    lat = _np(c["latent_mask"]).reshape(2, 5)
    x0 = _np(out["pred_xstart"]).astype(np.float64)
    rho, lim = seed_bound(x0, np.zeros_like(x0), _np(y.float()), lat, _np(w))["rho"]
    r = ratio(_np(out["residual_norm"]), rho, lim)
    print(f"  residual_norm: max |d| / bound = {r.max():.3f}")
    assert (r <= 1.0).all() and (rho > 1e-3).all()
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("mode,eta", [(0, 0.0), (1, 0.5)])
def test_step_identities_bit_for_bit(mode, eta):
    model, diff = tiny()
    N = diff.num_timesteps
    c = _rand_window(2, 6, 32, 2, seed=170)
    kw, x = _window_kw(c), c["x"].cuda()
    lat = _np(kw["latent_mask"]).reshape(2, 6) == 1
    g = torch.Generator().manual_seed(171)
    w = torch.tensor(random_taps(5, seed=3))
    y = blur(torch.rand(tuple(x.shape), generator=g) * 2 - 1, w) + 0.1 * torch.randn(tuple(x.shape), generator=g)
    noise = torch.randn(x.shape, generator=g).cuda()
    zeta = 0.75
    for tv in (N - 1, 3, 0):
        tt = _t(2, tv)
        plain, plain_x0 = diff._fused_step(mode, model, x, tt, True, kw, eta=eta, noise=noise)
        out = _deblur_call(diff, model, mode, x, tt, kw, eta, noise, y, w, zeta)
        got, grad = _np(out["sample"]), _np(out["grad"])
        assert torch.equal(out["pred_xstart"], plain_x0)                        # pred_xstart: the plain step's
        assert _same_bits(got[~lat], _np(plain)[~lat])                           # every other frame: sample_plain's bits
        assert _same_bits(got[lat], _fma32(np.float32(-zeta), grad[lat], _np(plain)[lat]))
        assert not grad[:, :2].any() and np.abs(grad[lat]).max() > 0 and not np.array_equal(got[lat], _np(plain)[lat])
        zero = _deblur_call(diff, model, mode, x, tt, kw, eta, noise, y, w, 0.0)
        assert torch.equal(zero["sample"], plain) and torch.equal(zero["pred_xstart"], plain_x0)     # zeta = 0: the plain step entirely
        assert torch.equal(zero["grad"], out["grad"]) and torch.equal(zero["residual_norm"], out["residual_norm"])
        again, again_x0 = diff._fused_step(mode, model, x, tt, True, kw, eta=eta, noise=noise)
        assert torch.equal(again, plain) and torch.equal(again_x0, plain_x0)     # a plain step behind a deblur step: its usual bits
    # the public entries: the dict gains 'residual_norm' and 'grad'; the sampler noise is drawn once, where the plain step draws it
    L, kk = _lib.lib(), _lib._I(0)
    with diff.deblur_scope(model, y, w, zeta=zeta):
        assert L.vd_blur_kernel(model._handle, kk) == 1 and kk.value == 5
        with diff.deblur_scope(model, y, gaussian_kernel(3, 1.0), zeta=0.1):      # scopes nest and restore
            assert L.vd_blur_kernel(model._handle, kk) == 1 and kk.value == 3
        assert L.vd_blur_kernel(model._handle, kk) == 1 and kk.value == 5
        torch.manual_seed(9)
        o = (diff.p_sample(model, x, _t(2, 3), model_kwargs=kw) if mode == 0 else diff.ddim_sample(model, x, _t(2, 3), model_kwargs=kw, eta=eta))
        after = torch.randn(3, device="cuda")
    assert L.vd_blur_kernel(model._handle, kk) == 0
    torch.manual_seed(9)
    n1 = torch.randn_like(x)
    assert torch.equal(after, torch.randn(3, device="cuda"))
    want = _deblur_call(diff, model, mode, x, _t(2, 3), kw, eta, n1, y, w, zeta)
    assert torch.equal(o["sample"], want["sample"]) and torch.equal(o["grad"], want["grad"]) and o["residual_norm"].shape == (2,)
    assert "grad" not in diff.p_sample(model, x, _t(2, 3), model_kwargs=kw)
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 4
def test_loop_is_the_chain_of_steps():
    model, diff = tiny(timestep_respacing="logsnr3")
    c = _rand_window(2, 6, 32, 2, seed=180)
    kw, x = _window_kw(c), c["x"].cuda()
    w = gaussian_kernel(7, 1.5)
    y = blur(torch.rand(tuple(x.shape), generator=torch.Generator().manual_seed(181)) * 2 - 1, w)
    with diff.deblur_scope(model, y, w, zeta=0.4):
        torch.manual_seed(11)
        got, _ = diff.p_sample_loop(model, tuple(x.shape), noise=x, model_kwargs=dict(kw))
        torch.manual_seed(11)
        noises = [torch.randn_like(x) for _ in range(3)]
        img = x
        for k, tv in enumerate((2, 1, 0)):
            img, _ = diff._step(0, model, img, _t(2, tv), True, None, kw, 0.0, noises[k])
    assert torch.equal(got, img) and torch.isfinite(got).all()
    with diff.deblur_scope(model, y, w, zeta=0.4):
        torch.manual_seed(11)
        d = diff.ddim_sample_loop(model, tuple(x.shape), noise=x, model_kwargs=dict(kw), eta=0.5)
        img = x
        for k, tv in enumerate((2, 1, 0)):
            img, _ = diff._step(1, model, img, _t(2, tv), True, None, kw, 0.5, noises[k])
    assert torch.equal(d, img)
    model.check_device_errors()


def test_infer_video_and_the_job(tmp_path, monkeypatch):
    from video_diffusion_amd import video_sample as vs
    model, diff = tiny(timestep_respacing="logsnr3")
    g = torch.Generator().manual_seed(60)
    batch = (torch.rand(2, 10, 3, 32, 32, generator=g) * 2 - 1).cuda()
    w = torch.tensor(random_taps(5, seed=61))
    y = blur(torch.rand(2, 10, 3, 32, 32, generator=g) * 2 - 1, w) + 0.05 * torch.randn(2, 10, 3, 32, 32, generator=g)
    torch.manual_seed(61)
    out, _ = vs.infer_video("autoreg", model, diff, batch, 6, 2, 4, measurement=y, blur_kernel=w, dps_zeta=0.3)
    # the per-window eager chain: every window's tensors gathered by its frame indices, p_sample inside deblur_scope
    torch.manual_seed(61)
    samples = torch.zeros_like(batch).cpu()
    samples[:, :2] = batch[:, :2].cpu()
    windows = 0
    for obs_i, lat_i in inference_util.inference_strategies["autoreg"](video_length=10, num_obs=2, max_frames=6, step_size=4, optimal_schedule_path=None):
        fi = torch.tensor(list(obs_i) + list(lat_i))
        x0 = samples[:, fi].clone().cuda()
        obs_mask, latent_mask, km = vs.get_masks(x0, len(obs_i))
        kw = dict(frame_indices=fi.repeat(2, 1).cuda(), x0=x0, obs_mask=obs_mask.cuda(), latent_mask=latent_mask.cuda(), kinda_marg_mask=km.cuda(),
                  x_t_minus_1=x0, observed_frames="x_0")
        local = x0.clone()
        with diff.deblur_scope(model, y[:, fi], w, zeta=0.3):
            for tv in (2, 1, 0):
                local = diff.p_sample(model, local, _t(2, tv), model_kwargs=kw)["sample"]
        samples[:, list(lat_i)] = local[:, -len(lat_i):].cpu()
        windows += 1
    assert windows == 2 and np.array_equal(out, samples.numpy()) and np.isfinite(out).all()
    assert np.array_equal(out[:, :2], batch[:, :2].cpu().numpy())
    torch.manual_seed(61)
    plain, _ = vs.infer_video("autoreg", model, diff, batch, 6, 2, 4)
    assert not np.array_equal(plain, out)
    with pytest.raises(_lib.VdError, match="blur_kernel without dps_zeta or particles is not served: measurement_scope together with a blur"):
        vs.infer_video("autoreg", model, diff, batch, 6, 2, 4, measurement=y, blur_kernel=w)
    # ... and through the particles, on both executors
    for ex in ("eager", "graph"):
        torch.manual_seed(62)
        smc, _ = vs.infer_video("autoreg", model, diff, batch, 6, 2, 4, measurement=y, blur_kernel=w, particles=2, sigma_y=0.5, executor=ex)
        assert smc.shape == out.shape and np.isfinite(smc).all() and np.array_equal(smc[:, :2], batch[:, :2].cpu().numpy())
    model.check_device_errors()
    # the job: --blur_sigma with --dps_zeta; the suffixed run directory
    vids = (torch.rand(2, 8, 3, 32, 32, generator=g) * 2 - 1)
    np.save(tmp_path / "videos.npy", vids.numpy())
    np.save(tmp_path / "y.npy", blur(vids, gaussian_kernel(5, 1.0)).numpy())
    monkeypatch.chdir(tmp_path)
    ap = vs.build_parser()
    args = vs.check_particle_arguments(ap, ap.parse_args(
        ["--videos", str(tmp_path / "videos.npy"), "--inference_mode", "autoreg", "--max_frames", "6", "--obs_length", "2", "--step_size", "4",
         "--batch_size", "2", "--timestep_respacing", "logsnr3", "--image_size", "32", "--num_channels", "32", "--num_res_blocks", "1",
         "--sampler", "ddim", "--eval_dir", str(tmp_path / "out"), "--measurement", str(tmp_path / "y.npy"), "--blur_sigma", "1", "--blur_size", "5",
         "--dps_zeta", "0.5"]))
    out_dir = vs.run(args, device=torch.device("cuda", 0))
    assert str(out_dir).endswith("_ddim_blur5_dps0.5")
    for i in range(2):
        f = np.load(out_dir / "samples" / f"sample_{i:04d}-0.npy")
        assert f.dtype == np.uint8 and f.shape == (8, 3, 32, 32) and np.array_equal(f[:2], vs.to_uint8(vids.numpy()[i])[:2])


def test_window_of_32_frames_runs_and_33_is_refused():
    model, diff = long_engine(tiny_cfg(40, num_channels=64, timestep_respacing="ddim50"))
    w = gaussian_kernel(9, 2.0)
    for T, n_obs in ((32, 8), (33, 8)):
        c = rand_window(1, T, 32, n_obs, seed=41)
        kw = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in c.items() if k != "x"}
        kw.update(x_t_minus_1=kw["x0"], observed_frames="x_0")
        x = c["x"].cuda()
        y = blur(torch.rand(tuple(x.shape), generator=torch.Generator().manual_seed(42)) * 2 - 1, w)
        with diff.deblur_scope(model, y, w, zeta=0.5):
            if T == 33:
                with pytest.raises(_lib.VdError, match=r"deblur: windows of at most 32 frames.*got 33"):
                    diff.p_sample(model, x, _t(1, 30), model_kwargs=kw)
                continue
            torch.manual_seed(1)
            o = diff.p_sample(model, x, _t(1, 30), model_kwargs=kw)
        assert torch.isfinite(o["sample"]).all() and torch.isfinite(o["grad"]).all() and float(o["residual_norm"][0]) > 0
        assert not o["grad"][:, :n_obs].any() and o["grad"][:, n_obs:].abs().max() > 0
    model.check_device_errors()


def test_every_refusal_by_message():
    model, diff = tiny()
    diff._bind(model)
    L = _lib.lib()
    c = _rand_window(2, 6, 32, 2, seed=195)
    kw, x = _window_kw(c), c["x"].cuda()
    w = gaussian_kernel(5, 1.0)
    y = blur(torch.rand(tuple(x.shape), generator=torch.Generator().manual_seed(196)) * 2 - 1, w)
    fn = lambda v: v                                                             # noqa: E731
    tt = _t(2, 3)
    with diff.deblur_scope(model, y, w, zeta=0.5):
        for call, what in ((lambda: diff.dpmpp_2m_sample(model, x, tt, model_kwargs=kw), "dpmpp_2m_sample"),
                           (lambda: diff.dpmpp_2m_sde_sample(model, x, tt, model_kwargs=kw), "dpmpp_2m_sde_sample"),
                           (lambda: diff.unipc_sample(model, x, tt, model_kwargs=kw), "unipc_sample"),
                           (lambda: diff.ddim_reverse_sample(model, x, tt, model_kwargs=kw), "ddim_reverse_sample"),
                           (lambda: diff.p_sample(model, x, tt, denoised_fn=fn, model_kwargs=kw), "denoised_fn"),
                           (lambda: diff.p_sample(model, x, tt, model_kwargs=kw, use_gradient_method=True), "use_gradient_method"),
                           (lambda: diff.p_sample(model, x, tt, model_kwargs=kw, return_attn_weights=True), "return_attn_weights"),
                           (lambda: diff.ddim_sample(model, x, tt, model_kwargs=kw, cfg_scale=2.0), "cfg_scale != 1"),
                           (lambda: WindowExecutor(model, diff).begin(x, kw), "WindowExecutor.begin")):      # a window graph
            with pytest.raises(_lib.VdError, match=f"{what} inside deblur_scope is not served"):
                call()
        with diff.cfg_scale_scope(model, 2.0):
            with pytest.raises(_lib.VdError, match="cfg_scale != 1 .cfg_scale_scope. inside deblur_scope"):
                diff.p_sample(model, x, tt, model_kwargs=kw)
        for opts in (dict(cfg_rescale=0.5), dict(dynamic_threshold=0.9)):
            with diff.guidance_scope(model, **opts):
                with pytest.raises(_lib.VdError, match="guidance_scope with cfg_rescale or dynamic_threshold set inside deblur_scope"):
                    diff.p_sample(model, x, tt, model_kwargs=kw)
        with diff.known_region_scope(model, torch.zeros_like(x), torch.ones(2, 6, 32, 32, device="cuda")):
            with pytest.raises(_lib.VdError, match="known_region_scope inside deblur_scope"):
                diff.p_sample(model, x, tt, model_kwargs=kw)
        with diff.measurement_scope(model, diff.measure(y, 4), 4):                   # measurement_scope with a blur
            with pytest.raises(_lib.VdError, match="measurement_scope inside deblur_scope"):
                diff.ddim_sample(model, x, tt, model_kwargs=kw)
        with diff.dps_scope(model, diff.measure(y, 4), 4, zeta=0.1):
            with pytest.raises(_lib.VdError, match="dps_scope inside deblur_scope"):
                diff.ddim_sample(model, x, tt, model_kwargs=kw)
        with pytest.raises(ValueError, match="deblur_scope: y"):
            diff.ddim_sample(model, x[:, :4], tt, model_kwargs={k: (v[:, :4] if torch.is_tensor(v) else v) for k, v in kw.items()})
        with pytest.raises(NotImplementedError, match="deblur_scope together with steering_scope is not served"):
            with diff.steering_scope(model, lambda x0, t: x0.flatten(1).sum(1), particles=2):
                diff.p_sample(model, x, tt, model_kwargs=kw)
    for bad, what in ((dict(zeta=-1.0), "zeta"), (dict(zeta=float("nan")), "zeta"), (dict(kernel=torch.ones(4, 4)), "must be odd"),
                      (dict(kernel=torch.ones(17, 17)), "at most 15"), (dict(kernel=torch.zeros(3, 3)), "all zero"),
                      (dict(y=y[0]), "y must be a .B, T, 3, H, W. tensor"), (dict(y=y[:, :, :1]), "a video is"),
                      (dict(y=torch.full_like(y, float("inf"))), "y must be finite")):
        args = dict(y=y, kernel=w, zeta=0.5)
        args.update(bad)
        with pytest.raises(ValueError, match=what):
            diff.deblur_scope(model, args["y"], args["kernel"], zeta=args["zeta"])
    with pytest.raises(TypeError):
        diff.deblur_scope(model, y, w)                                                # zeta is required
    for kwargs, what in ((dict(blur_kernel=w), "needs measurement= and sigma_y="), (dict(blur_kernel=w, measurement=y, sigma_y=1.0, sr_scale=2), "leave them at their defaults"),
                         (dict(blur_kernel=w, measurement=y, sigma_y=1.0, gray=True), "leave them at their defaults"),
                         (dict(blur_kernel=w, measurement=y[0], sigma_y=1.0), r"\(B, T, 3, H, W\) tensor under a blur"),
                         (dict(blur_kernel=torch.ones(2, 2), measurement=y, sigma_y=1.0), "must be odd"), (dict(blur_kernel=w, measurement=y), "sigma_y")):
        with pytest.raises(ValueError, match=what):
            diff.steering_scope(model, (lambda x0, t: x0.flatten(1).sum(1)) if "measurement" not in kwargs else None, particles=2, **kwargs)
    # the engine's own refusals, by message
    model._require_guidance()
    pk = model._pack_kwargs(x, kw)
    sample, xs = torch.empty_like(x), torch.empty_like(x)
    noise, yd = torch.zeros_like(x), y.cuda().float().contiguous()

    def step(m=model, sampler=0, zeta=0.5):
        return L.vd_deblur_step(m._handle, 2, 6, *m._window_ptrs(x, pk), _lib.ptr(tt), pk["obs_mode"], 1, sampler, 0.0, _lib.ptr(noise),
                                _lib.ptr(yd), zeta, _lib.ptr(sample), _lib.ptr(xs), None, None, _lib.current_stream())
    assert step() != 0 and b"deblur: no kernel is installed" in L.vd_last_error()
    taps = w.contiguous()
    _lib.check(L.vd_set_blur_kernel(model._handle, _lib.ptr(taps), 5))
    for kwargs, what in ((dict(sampler=2), b"deblur: p_sample (0) or ddim_sample (1)"), (dict(sampler=3), b"deblur: p_sample (0) or ddim_sample (1)"),
                         (dict(zeta=-1.0), b"deblur: zeta must be finite and not negative"), (dict(zeta=float("nan")), b"zeta must be finite and not negative"),
                         (dict(zeta=float("inf")), b"zeta must be finite and not negative")):
        assert step(**kwargs) != 0 and what in L.vd_last_error(), kwargs
    for setter, value, off, what in ((L.vd_set_cfg_scale, 2.0, 1.0, b"deblur together with cfg_scale != 1"),
                                     (L.vd_set_guidance_rescale, 0.5, 0.0, b"deblur together with guidance_rescale"),
                                     (L.vd_set_dynamic_threshold, 0.9, 0.0, b"deblur together with dynamic_threshold")):
        _lib.check(setter(model._handle, value))
        assert step() != 0 and what in L.vd_last_error()
        _lib.check(setter(model._handle, off))
    with diff.measurement_scope(model, diff.measure(y, 4), 4):
        assert step() != 0 and b"deblur together with a measurement" in L.vd_last_error()
    with diff.known_region_scope(model, torch.zeros_like(x), torch.ones(2, 6, 32, 32, device="cuda")):
        assert step() != 0 and b"deblur together with a known region" in L.vd_last_error()
    assert step() == 0                                                           # the engine is as it was: the step runs
    _lib.check(L.vd_set_blur_kernel(model._handle, None, 0))
    mx, dx_ = tiny(predict_xstart=True)
    with dx_.deblur_scope(mx, y, w, zeta=0.5):
        with pytest.raises(NotImplementedError, match="deblur_scope with predict_xstart=True: epsilon-prediction models only"):
            dx_.p_sample(mx, x, tt, model_kwargs=kw)
        mx._require_guidance()
        assert step(mx) != 0 and b"deblur: epsilon-prediction models only" in L.vd_last_error()
    fresh, dfresh = tiny(rp_alpha=7)                                             # a model whose backward image was never asked for
    dfresh._bind(fresh)
    _lib.check(L.vd_set_blur_kernel(fresh._handle, _lib.ptr(taps), 5))
    assert step(fresh) != 0 and b"deblur: the backward-data weight image is not on the device" in L.vd_last_error()
    _lib.check(L.vd_set_blur_kernel(fresh._handle, None, 0))
    torch.cuda.synchronize()
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 5: steering
def _blur_measurement(truth, K, w, sigma, seed):
    y = blur(truth, w)
    y = y + sigma * torch.randn(y.shape, generator=torch.Generator().manual_seed(seed))
    return y.repeat_interleave(K, dim=0).cuda()


def _torch_reward(y, w, lat, sigma):
    """reward_fn: r = -||y - blur(x0)||^2 / (2 sigma^2) over the latent frames, in float64 through blur() in torch."""
    def fn(x0, tt):                                                  # (on the host: conv2d in float64)
        r = (y.double().cpu() - blur(x0.double().cpu(), w)) * lat.double().cpu().view(x0.shape[0], -1, 1, 1, 1)
        return (-(r * r).flatten(1).sum(1) / (2.0 * sigma * sigma)).to(x0.device)
    return fn


def test_builtin_blur_reward_against_reward_fn():
    """B = 6 as G = 2 x K = 3, T = 5.  Under ess_threshold 0 nothing moves and the log-weights are lam r: the built-in reward against the
    reward_fn that computes the same with blur() in float64, inside the bar test_gpu_particles.py derives from the residual norm's bound
    (here blur_restated.seed_bound on the step's own x_0: |r_dev - r| <= (2 rho d + d^2) / (2 sigma^2)).  Under ess_threshold 1 both
    resample, with the same ancestors -- the thresholds keep 4 x the bar away from every c_k -- and the same gathered tensors."""
    model, diff = long_engine(_cfg())
    c, truth = _group_window(G_, K_, T_, 43)
    B, sigma, lam = G_ * K_, 1.5, 1.0
    # signed asymmetric taps with sum |w| = 1: the residual, and with it the bar (which grows with rho k k u sum |w| |x_0|), stays on the
    # scale of test_gpu_particles.py's, well below the margin the uniforms leave
    w = torch.tensor(random_taps(5, seed=44))
    w = w / w.abs().sum()
    y = _blur_measurement(truth, K_, w, 0.1, 7)
    kw, x = kwargs_of(c), c["x"].cuda()
    fn = _torch_reward(y, w, kw["latent_mask"], sigma)
    for t in (6, 0):
        noise = _noise(x.shape, 50 + t)
        plain = diff._step(0, model, x, _tt(B, t), True, None, kw, 0.0, noise)
        u = torch.tensor([[0.37, 0.61], [0.83, 0.12]], dtype=torch.float64)
        got = {}
        for tau in (0.0, 1.0):
            with diff.steering_scope(model, particles=K_, scale=lam, ess_threshold=tau, measurement=y, blur_kernel=w, sigma_y=sigma, uniforms=lambda _t: u):
                sb, xb = diff._step(0, model, x, _tt(B, t), True, None, kw, 0.0, noise)
                a = diff._last_steer
            with diff.steering_scope(model, fn, particles=K_, scale=lam, ess_threshold=tau, uniforms=lambda _t: u):
                sf, xf = diff._step(0, model, x, _tt(B, t), True, None, kw, 0.0, noise)
                f = diff._last_steer
            got[tau] = (a, f)
            assert torch.equal(a["ancestors"], f["ancestors"]) and torch.equal(sb, sf) and torch.equal(xb, xf), (t, tau)
            anc = a["ancestors"].long()
            assert torch.equal(sb, plain[0][anc]) and torch.equal(xb, plain[1][anc])
        a, f = got[0.0]
        x0n = _np(plain[0] if t == 0 else plain[1]).astype(np.float64)
        latn = _np(kw["latent_mask"]).reshape(B, -1)
        rho, d = seed_bound(x0n, np.zeros_like(x0n), _np(y).astype(np.float64), latn, _np(w))["rho"]
        bar = lam * (2 * rho * d + d * d) / (2 * sigma ** 2)
        lb, lf = a["log_weights"].cpu().numpy(), f["log_weights"].cpu().numpy()
        assert np.allclose(lf, -lam * rho ** 2 / (2 * sigma ** 2), rtol=1e-12)
        print(f"t={t}: log-weights {lb}, max |d| / bar = {(np.abs(lb - lf) / bar).max():.3f}, bar {bar.max():.3e}")
        assert (np.abs(lb - lf) <= bar).all() and np.ptp(lb[:K_]) > 0.05
        assert torch.equal(a["ancestors"].cpu(), torch.arange(B, dtype=torch.int32))
        st = pr.new_state(G_, K_)
        want = pr.particle_weights(st, (lf / lam).reshape(G_, K_), lam, 1.0, u.numpy(), np.full(G_, t == 0))
        assert _margin(want, u.numpy(), np.full(G_, t == 0)) > 4 * bar.max()
        assert np.array_equal(got[1.0][0]["ancestors"].cpu().numpy(), want["ancestors"])
        if t != 0:
            assert want["resampled"].all() and not got[1.0][0]["log_weights"].any()
    assert _lib.lib().vd_particles(model._handle) == 0 and _lib.lib().vd_particle_blur(model._handle) == 0
    kk = _lib._I(0)
    assert _lib.lib().vd_blur_kernel(model._handle, kk) == 0
    model.check_device_errors()


def _graph_window(wex, c, y, w, sampler, eta, seed, sigma, tau, steps):
    wex.begin(c["x"].cuda(), kwargs_of(c), seed=seed, sampler=sampler, eta=eta, particles=K_, particle_measurement=y, blur_kernel=w,
              sigma_y=sigma, ess_threshold=tau)
    trace = []
    for _ in range(steps):
        x = wex.run(1).clone()
        trace.append((x, wex.particle_state()["ancestors"].clone()))
    return trace, wex.particle_state()


def _eager_window(model, diff, c, y, w, sampler, eta, seed, sigma, tau, steps):
    """test_gpu_particles._eager_window with the blur: eager steps that repeat the graph's draws."""
    kw, x = kwargs_of(c), c["x"].cuda()
    B, n = x.shape[0], x.numel()
    trace, prev, out = [], None, None
    NT = diff.num_timesteps
    with diff.steering_scope(model, particles=K_, ess_threshold=tau, measurement=y, blur_kernel=w, sigma_y=sigma,
                             uniforms=None if sampler == "dpmpp_2m_sde" else (lambda tt: (seed, (NT - 1 - int(tt[0])) * n))):
        for k in range(steps):
            t = _tt(B, NT - 1 - k)
            if sampler == "dpmpp_2m_sde":
                out = diff._dpmpp_2m_sde(model, x, t, prev, True, None, kw, philox=(seed, k * n))
                prev = out["pred_xstart"]
            else:
                sample, _ = diff._step(0 if sampler == "p_sample" else 1, model, x, t, True, None, kw, eta, _randn(n, seed, k * n).view(x.shape))
                out = dict(diff._last_steer, sample=sample)
            x = out["sample"]
            trace.append((x, out["ancestors"].cpu()))
    return trace, out


def _same_windows(eager, last, graph, state):
    for k, ((xe, ae), (xg, ag)) in enumerate(zip(eager, graph)):
        assert torch.equal(xe, xg) and torch.equal(ae, ag), k
    assert torch.equal(last["chosen"].cpu(), state["chosen"]) and torch.equal(last["log_weights"].cpu(), state["log_weights"])


def test_graph_against_eager_and_taps_changed_between_windows():
    """dpmpp_2m_sde: one whole window of five steps on both executors, the same bits at every step.  Then a second window of the same
    executor with other taps of the same size: no new graph, another result, and the eager chain's bits under the new taps."""
    model, diff = long_engine(_cfg(respacing="ddim5"))
    c, truth = _group_window(G_, K_, T_, 81)
    w1, w2 = torch.tensor(random_taps(5, seed=82)), gaussian_kernel(5, 1.0)
    y = _blur_measurement(truth, K_, w1, 0.1, 8)
    L = _lib.lib()
    wex = WindowExecutor(model, diff)
    steps = diff.num_timesteps
    graph1, state1 = _graph_window(wex, c, y, w1, "dpmpp_2m_sde", 0.0, 1234567, 1.5, 0.9, steps)
    n_graphs = L.vd_window_graphs(model._handle)
    eager1, last1 = _eager_window(model, diff, c, y, w1, "dpmpp_2m_sde", 0.0, 1234567, 1.5, 0.9, steps)
    _same_windows(eager1, last1, graph1, state1)
    assert int(state1["resamples"].sum()) > 0 and int(state1["degenerate"].sum()) == 0
    graph2, state2 = _graph_window(wex, c, y, w2, "dpmpp_2m_sde", 0.0, 1234567, 1.5, 0.9, steps)
    assert L.vd_window_graphs(model._handle) == n_graphs                       # equal k: the same graph, replayed on the new taps
    assert not torch.equal(graph2[-1][0], graph1[-1][0]) or not torch.equal(state2["log_weights"], state1["log_weights"])
    eager2, last2 = _eager_window(model, diff, c, y, w2, "dpmpp_2m_sde", 0.0, 1234567, 1.5, 0.9, steps)
    _same_windows(eager2, last2, graph2, state2)
    assert not torch.equal(state2["log_weights"], state1["log_weights"])
    graph3, _ = _graph_window(wex, c, y, gaussian_kernel(7, 1.0), "dpmpp_2m_sde", 0.0, 1234567, 1.5, 0.9, 1)
    assert L.vd_window_graphs(model._handle) == n_graphs + 1                   # another k: another graph
    assert L.vd_particles(model._handle) == 0 and L.vd_particle_blur(model._handle) == 0
    model.check_device_errors()


def test_window_of_40_frames_runs():
    """Beyond the gradient scopes' 32 frames: deblur_scope refuses by name, the steered step and the steered window graph run and resample."""
    model, diff = long_engine(_cfg(40, respacing="ddim5"))
    c, truth = _group_window(1, K_, 40, 91, n_obs=3)
    w = gaussian_kernel(9, 2.0)
    y = _blur_measurement(truth, K_, w, 0.1, 9)
    kw, x, B = kwargs_of(c), c["x"].cuda(), K_
    with pytest.raises(_lib.VdError, match="deblur: windows of at most 32 frames"):
        with diff.deblur_scope(model, y, w, zeta=0.5):
            diff.p_sample(model, x, _tt(B, 4), model_kwargs=kw)
    plain = diff._step(0, model, x, _tt(B, 4), True, None, kw, 0.0, _noise(x.shape, 92))
    with diff.steering_scope(model, particles=K_, ess_threshold=1.0, measurement=y, blur_kernel=w, sigma_y=1.0):
        sample, xstart = diff._step(0, model, x, _tt(B, 4), True, None, kw, 0.0, _noise(x.shape, 92))
        a = diff._last_steer
    anc = a["ancestors"].long()
    assert torch.isfinite(sample).all() and torch.equal(sample, plain[0][anc]) and torch.equal(xstart, plain[1][anc])
    assert float(a["ess"][0]) < K_ and not a["log_weights"].any()
    trace, state = _graph_window(WindowExecutor(model, diff), c, y, w, "p_sample", 0.0, 77, 1.0, 1.0, diff.num_timesteps)
    # the first step resamples (K distinct x_t under ess_threshold 1).  Where a resampling leaves K copies of ONE particle the next step's
    # x_0 predictions -- functions of x_t alone -- and with them the rewards are bit-equal and nothing moves, and the step behind it
    # resamples again: of the four steps above t == 0 at least two do
    assert torch.isfinite(trace[-1][0]).all() and int(state["resamples"][0]) >= 2 and 0 <= int(state["chosen"][0]) < K_
    model.check_device_errors()
