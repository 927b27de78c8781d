"""GPU: loss-guided sampling (this project's extension) -- the seed pass per element against the float32 restatement
(tests/loss_guidance_restated.py) bit for bit, the step's gradient of a caller's torch loss against autograd through the CPU oracle at
the bars of test_gpu_dps.test_step_gradient_vs_oracle_autograd, the step's identities bit for bit against the plain step and against
eps_vjp (one forward, the same bits), DPS written as a torch loss against dps_scope, the held pass and its stale-ticket refusals, the
loops, infer_video and the video_sample job, and every refusal by message.  Nothing here is tuned on the code under test."""
import ctypes
import json

import numpy as np
import pytest
import torch

import video_diffusion_amd as vda
from helpers import close, synth_sd
from loss_guidance_restated import F, final_f32, fma32, multiplier_f32, norm_fp64, rows, seed_f32, xstart_r
from oracle.sampler_ref import SamplerRef
from oracle.schedule_ref import ScheduleRef
from oracle.unet_ref import UNetRef
from video_diffusion_amd import _lib, inference_util
from video_diffusion_amd.executor import WindowExecutor
from video_diffusion_amd.gaussian_diffusion import measure

pytestmark = pytest.mark.gpu
KEYS = vda.video_model_and_diffusion_defaults().keys()
_cache = {}
TINY = dict(T=6, image_size=32, num_channels=64, num_res_blocks=1, rp_alpha=6, rp_beta=6, rp_gamma=6, timestep_respacing="logsnr10")
ORACLE_CFG = dict(T=8, image_size=32, num_channels=64, num_res_blocks=1, rp_alpha=8, rp_beta=8, rp_gamma=8, timestep_respacing="ddim50")
STALE = "loss_guidance: no taped pass is held for this ticket"


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


def _rand_window(B, T, S, n_obs, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(B, T, 3, S, S, generator=g) * 2 - 1
    x0[:, n_obs:] = 0
    x = torch.randn(B, T, 3, S, S, generator=g)
    obs = torch.zeros(B, T, 1, 1, 1)
    obs[:, :n_obs] = 1
    return dict(x=x, x0=x0, obs_mask=obs, latent_mask=1 - obs, kinda_marg_mask=torch.zeros(B, T, 1, 1, 1),
                frame_indices=torch.arange(T).view(1, T).repeat(B, 1))


def _window_kw(c):
    d = {k: c[k].cuda() for k in ["x0", "obs_mask", "latent_mask", "kinda_marg_mask", "frame_indices"]}
    return dict(d, x_t_minus_1=d["x0"], observed_frames="x_0")


def _t(B, v):
    return torch.tensor([v] * B, device="cuda")


def _np(v):
    return v.detach().cpu().numpy()


def _same_bits(a, b):
    bits = lambda v: np.ascontiguousarray(_np(v) if torch.is_tensor(v) else v).view(np.uint32)      # noqa: E731
    return np.array_equal(bits(a), bits(b))


def _dev(v, misalign=False):
    """A float32 device copy of a numpy array / tensor; misalign: at an address 4 bytes off 16."""
    v = torch.as_tensor(v).float()
    if not misalign:
        return v.cuda().contiguous()
    buf = torch.empty(v.numel() + 1, device="cuda")
    out = buf[1:].view(v.shape)
    out.copy_(v)
    assert out.data_ptr() % 16 == 4
    return out


def _seed(model, xt, eps, t, clip, cot, lat, misalign=False):
    """vd_op_guide_seed -> (d_eps, d_x) as numpy arrays."""
    B, T, _, H, W = xt.shape
    x_d, e_d, c_d = (_dev(v, misalign) for v in (xt, eps, cot))
    t_d = torch.as_tensor(t).long().cuda()
    l_d = _dev(lat).reshape(-1).contiguous()
    outs = [_dev(np.full(xt.shape, 7.0, np.float32), misalign) for _ in range(2)]
    _lib.check(_lib.lib().vd_op_guide_seed(model._handle, B, T, H, W, _lib.ptr(x_d), _lib.ptr(e_d), _lib.ptr(t_d), 1 if clip else 0, _lib.ptr(c_d),
                                           _lib.ptr(l_d), _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.current_stream()))
    return _np(outs[0]), _np(outs[1])


# ---------------------------------------------------------------------------------------------------------------- 1
def _seed_inputs(diff, t, H, seed):
    """x_t, eps, cot (2, 3, 3, H, H) float32 and lat (2, 3) with frame 1 not latent.  x_0r is spread over about [-2.5, 2.5]; in every
    frame the first elements of the first row are planted: x_0r exactly +1, exactly -1 (eps = 0 and the x_t whose rounded product with a
    is 1, found among the neighbours of 1 / a), just above +1 and just below -1 -- one group of four holds both sides of the clamp."""
    rng = np.random.default_rng(seed)
    a, b = rows(diff, t)
    shape = (2, 3, 3, H, H)
    x0 = rng.uniform(-2.5, 2.5, shape)
    eps = rng.standard_normal(shape).astype(F)
    xt = ((x0 + b.astype(np.float64) * eps) / a.astype(np.float64)).astype(F)
    cot = rng.standard_normal(shape).astype(F)
    for bi in range(2):
        one = None
        cand = F(1.0) / a[bi, 0, 0, 0, 0]
        for k in range(-16, 17):
            v = cand
            for _ in range(abs(k)):
                v = np.nextafter(v, F(np.inf if k > 0 else -np.inf))
            if F(a[bi, 0, 0, 0, 0] * v) == F(1.0):
                one = v
                break
        assert one is not None, "no float32 x with fl(a x) == 1 near 1 / a"
        eps[bi, :, 0, 0, :4] = 0
        xt[bi, :, 0, 0, 0], xt[bi, :, 0, 0, 1] = one, -one
        xt[bi, :, 0, 0, 2], xt[bi, :, 0, 0, 3] = np.nextafter(one, F(np.inf)) * F(1.001), -np.nextafter(one, F(np.inf)) * F(1.001)
    lat = np.array([[1, 0, 1], [1, 0, 1]], np.float32)
    return xt, eps, cot, lat, a, b


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("H,misalign", [(8, False), (6, False), (7, False), (8, True)])
def test_seed_per_element_bit_for_bit(H, misalign, clip):
    """B = 2, T = 3, frame 1 not latent.  8 takes the 16-byte form, 6 and 7 (W % 4 != 0, odd) and the pointers 4 bytes off 16 the scalar
    one; t at both ends of the schedule and inside it, differing between the items."""
    model, diff = tiny()
    diff._bind(model)
    N = diff.num_timesteps
    for k, t in enumerate(([0, N // 2], [N // 2, N - 1], [N - 1, 0])):
        t = np.array(t)
        xt, eps, cot, lat, a, b = _seed_inputs(diff, t, H, seed=300 + 10 * H + k)
        de, dx = _seed(model, xt, eps, t, clip, cot, lat, misalign)
        wde, wdx, x0r = seed_f32(a, b, xt, eps, cot, lat, clip)
        sel = np.broadcast_to(lat.reshape(2, 3, 1, 1, 1) == 1, xt.shape)
        assert (x0r[sel] == 1).any() and (x0r[sel] == -1).any() and (x0r[sel] > 1).any() and (x0r[sel] < -1).any() and (np.abs(x0r[sel]) < 1).any()
        assert _same_bits(de, wde) and _same_bits(dx, wdx), (H, misalign, clip, t.tolist())
        assert not de[:, 1].any() and not dx[:, 1].any() and de[:, 0].any() and dx[:, 2].any()       # the frame that is not latent: exactly 0
        at_one = sel & (np.abs(x0r) == 1)
        assert _same_bits(dx[at_one], (a * cot).astype(F)[at_one])                                    # exactly +-1 lies inside the clamp
        if clip:
            assert not dx[sel & (np.abs(x0r) > 1)].any() and not de[sel & (np.abs(x0r) > 1)].any()
        else:
            assert _same_bits(dx[sel], np.broadcast_to((a * cot).astype(F), xt.shape)[sel])
    model.check_device_errors()
    # a cotangent that is not finite propagates and raises no error bit
    cot_bad = cot.copy()
    cot_bad[0, 0, 1, 2, 1], cot_bad[1, 2, 0, 1, 0] = np.inf, np.nan
    de, dx = _seed(model, xt, eps, t, False, cot_bad, lat, misalign)
    wde, wdx, _ = seed_f32(a, b, xt, eps, cot_bad, lat, False)
    assert np.isinf(dx[0, 0, 1, 2, 1]) and np.isnan(dx[1, 2, 0, 1, 0]) and np.array_equal(np.isfinite(dx), np.isfinite(wdx))
    assert np.array_equal(np.isfinite(de), np.isfinite(wde))
    model.check_device_errors()
    # an index outside the schedule poisons its item and sets the error bit
    tb = t.copy()
    tb[0] = N
    deb, dxb = _seed(model, xt, eps, tb, clip, cot, lat, misalign)
    wde, wdx, _ = seed_f32(*rows(diff, t), xt, eps, cot, lat, clip)
    assert np.isnan(deb[0]).all() and np.isnan(dxb[0]).all() and _same_bits(deb[1], wde[1]) and _same_bits(dxb[1], wdx[1])
    with pytest.raises(IndexError):
        model.check_device_errors()
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 2
def _oracle(cfg):
    model, diff = engine(cfg)
    net = UNetRef(cfg, synth_sd(model.param_specs()))
    sched = ScheduleRef(cfg["diffusion_steps"], cfg["noise_schedule"], cfg["timestep_respacing"], cfg["sigma_small"], cfg["rescale_timesteps"])
    return model, diff, SamplerRef(sched, net)


def _oracle_grad(ora, c, t, loss):
    """x_0 = clamp(a x_t - b eps) on the oracle's network with the window's real masks; the gradient of loss(x_0) restricted to the latent
    frames with respect to x_t."""
    sch = ora.s
    kwo = dict(x0=c["x0"], obs_mask=c["obs_mask"], latent_mask=c["latent_mask"], kinda_marg_mask=c["kinda_marg_mask"],
               frame_indices=c["frame_indices"], x_t_minus_1=c["x0"])
    x = c["x"].detach().clone().requires_grad_(True)
    tm = torch.tensor(sch.timestep_map, dtype=t.dtype)[t]
    coef = lambda tabl: torch.from_numpy(np.asarray(tabl))[t].float().view(-1, 1, 1, 1, 1)      # noqa: E731
    with torch.enable_grad():
        eps = ora.net.with_grad(x, tm, **kwo)
        x0 = (coef(sch.sqrt_recip_alphas_cumprod) * x - coef(sch.sqrt_recipm1_alphas_cumprod) * eps).clamp(-1, 1)
        x0l = x0 * c["latent_mask"] + x0.detach() * (1 - c["latent_mask"])       # what the loss says about the other frames is ignored
        g, = torch.autograd.grad(loss(x0l).sum(), x)
    return g


def _step(diff, model, mode, x, tt, kw, eta, noise, **scope):
    with diff.loss_guidance_scope(model, **scope):
        diff._step(mode, model, x, tt, True, None, kw, eta, noise)
    return diff._last_dps


@pytest.mark.parametrize("mode,eta", [(0, 0.0), (1, 0.5)])
def test_step_gradient_vs_oracle_autograd(mode, eta):
    """The smallest case and the bars of test_gpu_dps.test_step_gradient_vs_oracle_autograd: the same backward pass, the same oracle."""
    cfg = {**vda.video_model_and_diffusion_defaults(), **ORACLE_CFG}
    model, diff, ora = _oracle(cfg)
    c = _rand_window(2, 5, 32, 2, seed=725)
    g = torch.Generator().manual_seed(33)
    w = torch.randn(c["x"].shape, generator=g)
    noise = torch.randn(c["x"].shape, generator=g)
    t = torch.tensor([30, 30])
    want = _oracle_grad(ora, c, t, lambda x0: (w * x0).tanh().pow(2))
    kw = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in c.items() if k != "x"}
    kw.update(x_t_minus_1=kw["x0"], observed_frames="x_0")
    wd = w.cuda()
    out = _step(diff, model, mode, c["x"].cuda(), t.cuda(), kw, eta, noise, loss_fn=lambda x0, tt: (wd * x0).tanh().pow(2).sum(), scale=0.5)
    scale = float(want.abs().max())
    err = (out["grad"].cpu() - want).abs()
    print(f"mode {mode}: max |grad - ref| = {float(err.max()):.3e} = {float(err.max()) / scale:.3e} max |ref|")
    assert scale > 0 and not out["grad"][:, :2].any()                           # observed frames: exactly 0
    close(out["grad"].cpu(), want, atol=2e-4 * scale, rtol=1e-3)
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("mode,eta", [(0, 0.0), (1, 0.5)])
def test_one_forward_same_bits(mode, eta):
    model, diff = tiny()
    N = diff.num_timesteps
    c = _rand_window(2, 6, 32, 2, seed=170)
    kw, x = _window_kw(c), c["x"].cuda()
    latf = _np(kw["latent_mask"]).reshape(2, 6)
    lat = np.broadcast_to(latf.reshape(2, 6, 1, 1, 1) == 1, tuple(x.shape))
    g = torch.Generator().manual_seed(171)
    cot = torch.randn(x.shape, generator=g).cuda()
    noise = torch.randn(x.shape, generator=g).cuda()
    cot_fn = lambda x0, tt: cot                                                  # noqa: E731
    scale = 0.75
    for tv in (N - 1, 3, 0):
        tt = _t(2, tv)
        plain, plain_x0 = diff._fused_step(mode, model, x, tt, True, kw, eta=eta, noise=noise)
        out = _step(diff, model, mode, x, tt, kw, eta, noise, cotangent_fn=cot_fn, scale=scale)
        got, grad = _np(out["sample"]), _np(out["grad"])
        # the gradient is the seed pass on eps_vjp's eps and eps_vjp on its d eps: the composition costs a second forward, the bits agree
        eps = diff.eps_vjp(model, x, tt, cot, kw)["eps"]
        de, dx = _seed(model, _np(x), _np(eps), _np(tt), True, _np(cot), latf)
        vjp = diff.eps_vjp(model, x, tt, torch.from_numpy(de).cuda(), kw)["vjp"]
        assert _same_bits(grad, (dx + _np(vjp)).astype(F)), tv
        assert torch.equal(out["pred_xstart"], plain_x0)                        # pred_xstart: the plain step's
        assert _same_bits(got[~lat], _np(plain)[~lat])                           # every other frame: sample_plain's bits
        assert _same_bits(got[lat], fma32(F(-scale), grad[lat], _np(plain)[lat]))
        assert not grad[:, :2].any() and np.abs(grad[lat]).max() > 0 and not np.array_equal(got[lat], _np(plain)[lat])
        assert "grad_norm" not in out
        zero = _step(diff, model, mode, x, tt, kw, eta, noise, cotangent_fn=cot_fn, scale=0.0)
        assert torch.equal(zero["sample"], plain) and torch.equal(zero["pred_xstart"], plain_x0)     # scale 0: the plain step entirely
        assert torch.equal(zero["grad"], out["grad"])
        again, again_x0 = diff._fused_step(mode, model, x, tt, True, kw, eta=eta, noise=noise)
        assert torch.equal(again, plain) and torch.equal(again_x0, plain_x0)     # a plain step behind a guided one: its usual bits
        # normalised: the norm inside the restatement's bound of the float64 norm of the returned grad; one float32 division per item
        nrm = _step(diff, model, mode, x, tt, kw, eta, noise, cotangent_fn=cot_fn, scale=lambda t_: torch.tensor([scale, 2.0]), normalize=True)
        assert torch.equal(nrm["grad"], out["grad"]) and torch.equal(nrm["pred_xstart"], plain_x0)
        n_got = _np(nrm["grad_norm"])
        n64, lim = norm_fp64(grad, latf)
        r = np.abs(n_got.astype(np.float64) - n64) / lim
        print(f"mode {mode} t {tv}: grad_norm {n_got.tolist()}, |d| / bound = {r.tolist()}")
        assert (r <= 1.0).all() and (n64 > 0).all()
        m = multiplier_f32([scale, 2.0], n_got)
        assert _same_bits(_np(nrm["sample"]), final_f32(m, grad, _np(plain), latf))
        rerun = _step(diff, model, mode, x, tt, kw, eta, noise, cotangent_fn=cot_fn, scale=lambda t_: torch.tensor([scale, 2.0]), normalize=True)
        assert torch.equal(rerun["grad"], nrm["grad"]) and torch.equal(rerun["grad_norm"], nrm["grad_norm"]) and torch.equal(rerun["sample"], nrm["sample"])
        # an item whose cotangent is all zero keeps the plain step exactly, normalised (n_b == 0) or not; the other item keeps its bits
        cz = cot.clone()
        cz[1] = 0
        for normalize in (True, False):
            z = _step(diff, model, mode, x, tt, kw, eta, noise, cotangent_fn=lambda x0, t_: cz, scale=scale, normalize=normalize)
            assert torch.equal(z["sample"][1], plain[1]) and not z["grad"][1].any() and torch.isfinite(z["sample"]).all()
            assert not torch.equal(z["sample"][0], plain[0])
            if normalize:
                assert float(z["grad_norm"][1]) == 0.0 and float(z["grad_norm"][0]) > 0
    # the public entries: the dict gains 'grad'; the sampler noise is drawn once, where the plain step draws it
    with diff.loss_guidance_scope(model, cotangent_fn=cot_fn, scale=scale):
        torch.manual_seed(9)
        o = (diff.p_sample(model, x, _t(2, 3), model_kwargs=kw) if mode == 0 else diff.ddim_sample(model, x, _t(2, 3), model_kwargs=kw, eta=eta))
        after = torch.randn(3, device="cuda")
    torch.manual_seed(9)
    n1 = torch.randn_like(x)
    assert torch.equal(after, torch.randn(3, device="cuda"))
    want = _step(diff, model, mode, x, _t(2, 3), kw, eta, n1, cotangent_fn=cot_fn, scale=scale)
    assert torch.equal(o["sample"], want["sample"]) and torch.equal(o["grad"], want["grad"]) and "grad_norm" not in o
    assert "grad" not in diff.p_sample(model, x, _t(2, 3), model_kwargs=kw)
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("mode,eta", [(0, 0.0), (1, 0.5)])
def test_dps_is_an_instance(mode, eta):
    """rho of dps_scope written in torch with `measure`: the same gradient to the bars of the oracle comparison, against the larger of the
    two maxima (torch forms the cotangent in another order: no bit equality)."""
    model, diff = tiny()
    c = _rand_window(2, 6, 32, 2, seed=190)
    kw, x = _window_kw(c), c["x"].cuda()
    g = torch.Generator().manual_seed(191)
    y = (measure(torch.rand(tuple(x.shape), generator=g) * 2 - 1, 4, True) + 0.1 * torch.randn(2, 6, 1, 8, 8, generator=g)).cuda()
    noise = torch.randn(x.shape, generator=g).cuda()
    latm = kw["latent_mask"]

    def rho(x0, tt):
        return ((y - measure(x0, 4, True)) * latm).flatten(1).norm(dim=1)

    tt = _t(2, 4)
    with diff.dps_scope(model, y, 4, True, zeta=0.5):
        diff._step(mode, model, x, tt, True, None, kw, eta, noise)
    dps = diff._last_dps
    out = _step(diff, model, mode, x, tt, kw, eta, noise, loss_fn=rho, scale=0.5)
    top = max(float(out["grad"].abs().max()), float(dps["grad"].abs().max()))
    err = (out["grad"] - dps["grad"]).abs()
    print(f"mode {mode}: max |grad - dps grad| = {float(err.max()):.3e} = {float(err.max()) / top:.3e} of the larger maximum")
    assert top > 0 and torch.equal(out["pred_xstart"], dps["pred_xstart"])
    close(out["grad"], dps["grad"], atol=2e-4 * top, rtol=1e-3)
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 5
def test_the_held_pass_is_never_read_stale():
    """Every case is a host-side refusal before any launch."""
    model, diff = tiny()
    diff._bind(model)
    model._require_guidance()
    L = _lib.lib()
    c = _rand_window(2, 6, 32, 2, seed=200)
    kw, x = _window_kw(c), c["x"].cuda()
    pk = model._pack_kwargs(x, kw)
    tt = _t(2, 3)
    g = torch.Generator().manual_seed(201)
    noise, cot = (torch.randn(x.shape, generator=g).cuda() for _ in range(2))
    scale = torch.tensor([0.5, 0.5], device="cuda")
    sample, xs, grad = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)

    def begin():
        ticket = ctypes.c_ulonglong(0)
        _lib.check(L.vd_guide_begin(model._handle, 2, 6, *model._window_ptrs(x, pk), _lib.ptr(tt), pk["obs_mode"], 1, 0, 0.0, _lib.ptr(noise),
                                    _lib.ptr(sample), _lib.ptr(xs), ctypes.byref(ticket), _lib.current_stream()))
        assert ticket.value != 0
        return ticket.value

    def finish(ticket):
        return L.vd_guide_finish(model._handle, ticket, _lib.ptr(cot), _lib.ptr(scale), 0, _lib.ptr(sample), _lib.ptr(grad), None, _lib.current_stream())

    def stale(ticket, why):
        before = sample.clone()
        assert finish(ticket) != 0
        msg = L.vd_last_error().decode()
        assert STALE in msg and why in msg, msg
        torch.cuda.synchronize()
        assert torch.equal(sample, before)                                       # nothing was launched: sample is untouched

    plain, _ = diff._fused_step(0, model, x, tt, True, kw, noise=noise)
    stale(1 << 40, "never begun")
    stale(0, "never begun")
    t1 = begin()
    assert torch.equal(sample, plain)                                            # the first half leaves the plain step's sample
    assert finish(t1) == 0
    want = sample.clone()
    assert not torch.equal(want, plain)
    stale(t1, "already finished")                                                # finish twice
    t2 = begin()
    assert t2 != t1
    model(x, torch.zeros(2, device="cuda"), **kw)                                # an engine call on the same model in between
    stale(t2, "dropped by an engine call in between")
    t3 = begin()
    t4 = begin()                                                                 # begin twice: the first ticket is dead, the second works
    assert t4 != t3
    stale(t3, "dropped by an engine call in between")
    assert finish(t4) == 0
    assert torch.equal(sample, want)
    t5 = begin()
    _lib.check(L.vd_guide_abort(model._handle))
    stale(t5, "aborted")
    _lib.check(L.vd_guide_abort(model._handle))                                  # nothing held: no effect
    # the Python step: a function that calls the engine on the same model fails with the stale-ticket error ...
    with diff.loss_guidance_scope(model, cotangent_fn=lambda x0, t_: model(x0, torch.zeros(2, device="cuda"), **kw)[0], scale=0.5):
        with pytest.raises(_lib.VdError, match=STALE):
            diff.p_sample(model, x, tt, model_kwargs=kw)

    # ... and one that raises leaves nothing held: its ticket (the next in line) is reported aborted, the next plain step has its usual bits
    def boom(x0, t_):
        raise KeyError("the caller's own")

    t6 = begin()
    _lib.check(L.vd_guide_abort(model._handle))
    with diff.loss_guidance_scope(model, boom, scale=0.5):
        with pytest.raises(KeyError, match="the caller's own"):
            diff.p_sample(model, x, tt, model_kwargs=kw)
    stale(t6 + 1, "aborted")
    again, _ = diff._fused_step(0, model, x, tt, True, kw, noise=noise)
    assert torch.equal(again, plain)
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 6
def _bright(x0, t):
    return (x0 - 0.25).pow(2).mean(dim=(1, 2, 3, 4))


def test_loop_is_the_chain_of_steps():
    model, diff = tiny(timestep_respacing="logsnr3")
    c = _rand_window(2, 6, 32, 2, seed=180)
    kw, x = _window_kw(c), c["x"].cuda()
    seen = []

    def scale(t):
        seen.append(int(t[0]))
        return 40.0 * (1 + int(t[0]))

    with diff.loss_guidance_scope(model, _bright, scale=scale, normalize=True):
        torch.manual_seed(11)
        got, _ = diff.p_sample_loop(model, tuple(x.shape), noise=x, model_kwargs=dict(kw))
        torch.manual_seed(11)
        noises = [torch.randn_like(x) for _ in range(3)]
        img = x
        for k, tv in enumerate((2, 1, 0)):
            img, _ = diff._step(0, model, img, _t(2, tv), True, None, kw, 0.0, noises[k])
    assert torch.equal(got, img) and torch.isfinite(got).all() and seen == [2, 1, 0, 2, 1, 0]
    torch.manual_seed(11)
    unguided, _ = diff.p_sample_loop(model, tuple(x.shape), noise=x, model_kwargs=dict(kw))
    assert not torch.equal(unguided, got)
    with diff.loss_guidance_scope(model, _bright, scale=scale):
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
    torch.manual_seed(61)
    out, _ = vs.infer_video("autoreg", model, diff, batch, 6, 2, 4, loss_fn=_bright, loss_scale=30.0)
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
        with diff.loss_guidance_scope(model, _bright, scale=30.0):
            for tv in (2, 1, 0):
                local = diff.p_sample(model, local, _t(2, tv), model_kwargs=kw)["sample"]
        samples[:, list(lat_i)] = local[:, -len(lat_i):].cpu()
        windows += 1
    assert windows == 2 and np.array_equal(out, samples.numpy()) and np.isfinite(out).all()
    assert np.array_equal(out[:, :2], batch[:, :2].cpu().numpy())
    torch.manual_seed(61)
    plain, _ = vs.infer_video("autoreg", model, diff, batch, 6, 2, 4)
    assert not np.array_equal(plain, out)
    with pytest.raises(_lib.VdError, match="executor='graph' together with loss_fn"):
        vs.infer_video("autoreg", model, diff, batch, 6, 2, 4, loss_fn=_bright, loss_scale=30.0, executor="graph")
    model.check_device_errors()
    # the job: --loss_guidance MODULE:FUNCTION on the synthetic videos; the suffixed run directory; the files are infer_video's
    (tmp_path / "job_losses.py").write_text("def bright(x0, t):\n    return (x0 - 0.25).pow(2).mean(dim=(1, 2, 3, 4))\n")
    monkeypatch.syspath_prepend(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    args = vs.build_parser().parse_args(
        ["--num_videos", "2", "--T", "10", "--inference_mode", "autoreg", "--max_frames", "6", "--obs_length", "2", "--step_size", "4",
         "--batch_size", "2", "--timestep_respacing", "logsnr3", "--image_size", "32", "--num_channels", "32", "--num_res_blocks", "1",
         "--sampler", "ddim", "--eval_dir", str(tmp_path / "out"), "--loss_guidance", "job_losses:bright", "--loss_guidance_scale", "30"])
    seen = {}

    def infer(a, m, d, b, path):
        seen.update(model=m, diff=d, batch=b.clone(), cpu=torch.get_rng_state(), cuda=torch.cuda.get_rng_state())
        return vs._default_infer(a, m, d, b, path)

    out_dir = vs.run(args, device=torch.device("cuda", 0), infer=infer)
    assert str(out_dir).endswith("_ddim_lg30")
    torch.set_rng_state(seen["cpu"])
    torch.cuda.set_rng_state(seen["cuda"])
    import job_losses
    want, _ = vs.infer_video("autoreg", seen["model"], seen["diff"], seen["batch"], 6, 2, 4, sampler="ddim", loss_fn=job_losses.bright, loss_scale=30.0)
    for i in range(2):
        f = np.load(out_dir / "samples" / f"sample_{i:04d}-0.npy")
        assert f.dtype == np.uint8 and f.shape == (10, 3, 32, 32) and np.array_equal(f, vs.to_uint8(want)[i])


# ---------------------------------------------------------------------------------------------------------------- 7
def test_every_refusal_by_message():
    model, diff = tiny()
    diff._bind(model)
    L = _lib.lib()
    c = _rand_window(2, 6, 32, 2, seed=195)
    kw, x = _window_kw(c), c["x"].cuda()
    y = measure(torch.rand(tuple(x.shape), generator=torch.Generator().manual_seed(196)) * 2 - 1, 4, False)
    fn = lambda v: v                                                             # noqa: E731
    cot_fn = lambda x0, t_: x0                                                   # noqa: E731
    tt = _t(2, 3)
    with diff.loss_guidance_scope(model, cotangent_fn=cot_fn, scale=0.5):
        for call, what in ((lambda: diff.dpmpp_2m_sample(model, x, tt, model_kwargs=kw), "dpmpp_2m_sample"),
                           (lambda: diff.dpmpp_2m_sde_sample(model, x, tt, model_kwargs=kw), "dpmpp_2m_sde_sample"),
                           (lambda: diff.unipc_sample(model, x, tt, model_kwargs=kw), "unipc_sample"),
                           (lambda: diff.ddim_reverse_sample(model, x, tt, model_kwargs=kw), "ddim_reverse_sample"),
                           (lambda: diff.p_sample(model, x, tt, denoised_fn=fn, model_kwargs=kw), "denoised_fn"),
                           (lambda: diff.p_sample(model, x, tt, model_kwargs=kw, use_gradient_method=True), "use_gradient_method"),
                           (lambda: diff.p_sample(model, x, tt, model_kwargs=kw, return_attn_weights=True), "return_attn_weights"),
                           (lambda: diff.ddim_sample(model, x, tt, model_kwargs=kw, cfg_scale=2.0), "cfg_scale != 1"),
                           (lambda: WindowExecutor(model, diff).begin(x, kw), "WindowExecutor.begin")):
            with pytest.raises(_lib.VdError, match=f"{what} inside loss_guidance_scope is not served"):
                call()
        with diff.cfg_scale_scope(model, 2.0):
            with pytest.raises(_lib.VdError, match="cfg_scale != 1 .cfg_scale_scope. inside loss_guidance_scope"):
                diff.p_sample(model, x, tt, model_kwargs=kw)
        for opts in (dict(cfg_rescale=0.5), dict(dynamic_threshold=0.9)):
            with diff.guidance_scope(model, **opts):
                with pytest.raises(_lib.VdError, match="guidance_scope with cfg_rescale or dynamic_threshold set inside loss_guidance_scope"):
                    diff.p_sample(model, x, tt, model_kwargs=kw)
        with diff.known_region_scope(model, torch.zeros_like(x), torch.ones(2, 6, 32, 32, device="cuda")):
            with pytest.raises(_lib.VdError, match="known_region_scope inside loss_guidance_scope"):
                diff.p_sample(model, x, tt, model_kwargs=kw)
        with diff.measurement_scope(model, y, 4):
            with pytest.raises(_lib.VdError, match="measurement_scope inside loss_guidance_scope"):
                diff.ddim_sample(model, x, tt, model_kwargs=kw)
        with diff.dps_scope(model, y, 4, zeta=0.5):
            with pytest.raises(_lib.VdError, match="dps_scope inside loss_guidance_scope"):
                diff.ddim_sample(model, x, tt, model_kwargs=kw)
        for bad in (-1.0, float("nan")):
            with diff.loss_guidance_scope(model, cotangent_fn=cot_fn, scale=lambda t_, bad=bad: bad):
                with pytest.raises(ValueError, match="finite and not negative"):
                    diff.p_sample(model, x, tt, model_kwargs=kw)
        # not honoured by model(...), p_mean_variance and the vjp / NLL path: they run as outside the scope
        assert torch.equal(model(x, torch.zeros(2, device="cuda"), **kw)[0], model(x, torch.zeros(2, device="cuda"), **kw)[0])
        assert "grad" not in diff.p_mean_variance(model, x, tt, model_kwargs=kw)
        assert diff.eps_vjp(model, x, tt, x, kw)["vjp"].shape == x.shape
    for kwargs in (dict(), dict(loss_fn=fn, cotangent_fn=fn)):
        with pytest.raises(ValueError, match="exactly one of loss_fn and cotangent_fn"):
            with diff.loss_guidance_scope(model, scale=1.0, **kwargs):
                pass
    # the engine's own refusals, by message
    model._require_guidance()
    pk = model._pack_kwargs(x, kw)
    sample, xs = torch.empty_like(x), torch.empty_like(x)
    noise = torch.zeros_like(x)
    ticket = ctypes.c_ulonglong(0)

    def begin(m=model, sampler=0):
        return L.vd_guide_begin(m._handle, 2, 6, *m._window_ptrs(x, pk), _lib.ptr(tt), pk["obs_mode"], 1, sampler, 0.0, _lib.ptr(noise),
                                _lib.ptr(sample), _lib.ptr(xs), ctypes.byref(ticket), _lib.current_stream())
    for sampler in (2, 3, 5):
        assert begin(sampler=sampler) != 0 and b"loss_guidance: p_sample (0) or ddim_sample (1)" in L.vd_last_error(), sampler
    for setter, value, off, what in ((L.vd_set_cfg_scale, 2.0, 1.0, b"loss_guidance together with cfg_scale != 1"),
                                     (L.vd_set_guidance_rescale, 0.5, 0.0, b"loss_guidance together with guidance_rescale"),
                                     (L.vd_set_dynamic_threshold, 0.9, 0.0, b"loss_guidance together with dynamic_threshold")):
        _lib.check(setter(model._handle, value))
        assert begin() != 0 and what in L.vd_last_error()
        _lib.check(setter(model._handle, off))
    with diff.measurement_scope(model, y, 4):
        assert begin() != 0 and b"loss_guidance together with a measurement" in L.vd_last_error()
    with diff.known_region_scope(model, torch.zeros_like(x), torch.ones(2, 6, 32, 32, device="cuda")):
        assert begin() != 0 and b"loss_guidance together with a known region" in L.vd_last_error()
    assert ticket.value == 0
    assert begin() == 0 and ticket.value != 0                                    # the engine is as it was: the first half runs
    _lib.check(L.vd_guide_abort(model._handle))
    mx, dx_ = tiny(predict_xstart=True)
    with dx_.loss_guidance_scope(mx, cotangent_fn=cot_fn, scale=0.5):
        with pytest.raises(NotImplementedError, match="loss_guidance_scope with predict_xstart=True: epsilon-prediction models only"):
            dx_.p_sample(mx, x, tt, model_kwargs=kw)
    dx_._bind(mx)
    mx._require_guidance()
    assert begin(mx) != 0 and b"loss_guidance: epsilon-prediction models only" in L.vd_last_error()
    fresh, dfresh = tiny(rp_alpha=7)                                             # a model whose backward image was never asked for
    dfresh._bind(fresh)
    assert begin(fresh) != 0 and b"loss_guidance: the backward-data weight image is not on the device" in L.vd_last_error()
    torch.cuda.synchronize()
    model.check_device_errors()
