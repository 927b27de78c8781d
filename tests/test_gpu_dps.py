"""GPU: diffusion posterior sampling (this project's extension, DPS) -- the residual and seed passes per element against the float64
restatement (tests/dps_restated.py) inside its derived bound, the step's gradient against autograd through the CPU oracle with the
window's real masks at the bars of test_use_gradient_method_vs_oracle_autograd, the step's identities bit for bit against the plain
step, the loop, infer_video and the video_sample job, and every refusal by message.  Nothing here is tuned on the code under test."""
import numpy as np
import pytest
import torch

import video_diffusion_amd as vda
from dps_restated import assert_unambiguous, dps_bound, dps_f32, seed_bound, seed_inputs
from helpers import close
from step_nll_restated import ratio, tables
from test_gpu_dpmpp_2m import _rand_window, _t, _window_kw, tiny
from test_gpu_engine import _oracle
from test_gpu_known_region import _bits, _np, _same_bits
from test_gpu_long_window import engine as long_engine, rand_window, tiny_cfg
from video_diffusion_amd import _lib, inference_util
from video_diffusion_amd.executor import WindowExecutor
from video_diffusion_amd.gaussian_diffusion import measure

pytestmark = pytest.mark.gpu
STEP_OPERATORS = [(4, False), (1, True)]


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


def _seed(model, xt, eps, t, clip, y, lat, s, gray, misalign=False):
    """vd_op_dps_seed -> (d_eps, d_x, rho, pred_xstart) as numpy arrays."""
    B, T, _, H, W = xt.shape
    x_d, e_d = _dev(xt, misalign), _dev(eps, misalign)
    t_d = torch.as_tensor(t).long().cuda()
    y_d, l_d = _dev(y), _dev(lat).reshape(-1).contiguous()
    outs = [_dev(np.full(xt.shape, 7.0, np.float32), misalign) for _ in range(3)]
    rho = torch.full((B,), 7.0, device="cuda")
    _lib.check(_lib.lib().vd_op_dps_seed(model._handle, B, T, H, W, _lib.ptr(x_d), _lib.ptr(e_d), _lib.ptr(t_d), 1 if clip else 0, _lib.ptr(y_d),
                                         _lib.ptr(l_d), s, 1 if gray else 0, _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(rho), _lib.ptr(outs[2]),
                                         _lib.current_stream()))
    return _np(outs[0]), _np(outs[1]), _np(rho), _np(outs[2])


def _plain_xstart(model, xt, eps, t, clip):
    """pred_xstart of the sampler pass alone (vd_posterior_update) on the same (x_t, eps)."""
    B = xt.shape[0]
    x_d, e_d = _dev(xt).reshape(B, -1), _dev(eps).reshape(B, -1)
    t_d = torch.as_tensor(t).long().cuda()
    z, smp, xs = torch.zeros_like(x_d), torch.empty_like(x_d), torch.empty_like(x_d)
    _lib.check(_lib.lib().vd_posterior_update(model._handle, 0, B, x_d.shape[1], _lib.ptr(x_d), _lib.ptr(e_d), _lib.ptr(t_d), 1 if clip else 0, 0.0,
                                              _lib.ptr(z), 0, 0, _lib.ptr(smp), _lib.ptr(xs), _lib.current_stream()))
    return _np(xs).reshape(xt.shape)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("H,s,gray", [(8, 2, False), (8, 4, False), (8, 8, False), (12, 4, False), (6, 2, False), (7, 1, True), (8, 2, True),
                                      (8, 4, True), (16, 8, True)])
def test_seed_per_element(H, s, gray, clip):
    """B = 2, T = 3, frame 1 not latent.  8, 12 and 16 take the 16-byte form, 6 and 7 the scalar one; every cell size.  With the clamp a
    quarter of the elements sits beyond +-1."""
    model, diff = tiny()
    diff._bind(model)
    tab = tables(diff)
    B, T = 2, 3
    xt, eps, t, y, lat = seed_inputs(tab, B, T, H, s, gray, clip, seed=1000 + 10 * H + s + (5 if gray else 0))
    assert_unambiguous(tab, xt, eps, t, y, lat, s, gray, clip)
    de, dx, rho, xs = _seed(model, xt, eps, t, clip, y, lat, s, gray)
    lim = dps_bound(tab, xt, eps, t, y, lat, s, gray, clip)
    f32 = dps_f32(tab, xt, eps, t, y, lat, s, gray, clip)
    for name, got in (("deps", de), ("dxd", dx), ("rho", rho)):
        want, bound = lim[name]
        r = ratio(got, want, bound)
        print(f"H={H} s={s} gray={gray} clip={clip} {name}: max |d| / bound = {r.max():.3f}; f32 restatement equal: {_same_bits(got, f32[name])}")
        assert (r <= 1.0).all(), (name, float(r.max()))
    assert not de[:, 1].any() and not dx[:, 1].any() and de[:, 0].any() and dx[:, 2].any()       # the frame that is not latent: exactly 0
    assert _same_bits(xs, _plain_xstart(model, xt, eps, t, clip))                                 # pred_xstart: the sampler pass's bits
    if clip:
        beyond = np.abs(f32["x0"]) == 1.0
        assert 0.15 < beyond.mean() < 0.35 and not dx[beyond].any()
    # a rerun, inputs 4 bytes off alignment (the scalar form) and item b alone: the same bits
    for again in (_seed(model, xt, eps, t, clip, y, lat, s, gray), _seed(model, xt, eps, t, clip, y, lat, s, gray, misalign=True)):
        assert all(_same_bits(a, b) for a, b in zip(again, (de, dx, rho, xs)))
    for b in range(B):
        alone = _seed(model, xt[b:b + 1], eps[b:b + 1], t[b:b + 1], clip, y[b:b + 1], lat[b:b + 1], s, gray)
        assert all(_same_bits(a, w[b:b + 1]) for a, w in zip(alone, (de, dx, rho, xs))), b
    # an item with no latent frame: rho = 0, no gradient, no NaN; the other item keeps its bits
    lat0 = lat.copy()
    lat0[0] = 0
    de0, dx0, rho0, xs0 = _seed(model, xt, eps, t, clip, y, lat0, s, gray)
    assert rho0[0] == 0 and not de0[0].any() and not dx0[0].any() and np.isfinite(de0).all() and np.isfinite(dx0).all()
    assert _same_bits(de0[1], de[1]) and _same_bits(rho0[1:], rho[1:]) and _same_bits(xs0, xs)
    model.check_device_errors()
    # an index outside the schedule poisons its item as the sampler pass does, and sets the error bit
    tb = t.copy()
    tb[0] = tab["NT"]
    deb, dxb, rhob, xsb = _seed(model, xt, eps, tb, clip, y, lat, s, gray)
    assert np.isnan(deb[0]).all() and np.isnan(dxb[0]).all() and np.isnan(rhob[0]) and np.isnan(xsb[0]).all()
    assert _same_bits(deb[1], de[1]) and _same_bits(dxb[1], dx[1]) and _same_bits(rhob[1:], rho[1:])
    with pytest.raises(IndexError):
        model.check_device_errors()
    model.check_device_errors()


def test_seed_entry_refusals():
    model, diff = tiny()
    diff._bind(model)
    L = _lib.lib()
    x = torch.zeros(1, 1, 3, 8, 8, device="cuda")
    y, lat, t = torch.zeros(1, 1, 3, 8, 8, device="cuda"), torch.ones(1, device="cuda"), torch.zeros(1, dtype=torch.long, device="cuda")
    out = torch.empty_like(x)
    call = lambda H, W, s, gr: L.vd_op_dps_seed(model._handle, 1, 1, H, W, _lib.ptr(x), _lib.ptr(x), _lib.ptr(t), 1, _lib.ptr(y), _lib.ptr(lat),  # noqa: E731
                                                s, gr, _lib.ptr(out), _lib.ptr(out), None, None, _lib.current_stream())
    for s, gr in ((1, 0), (3, 0), (16, 1), (0, 1)):
        assert call(8, 8, s, gr) != 0 and b"scale is 2, 4 or 8, or 1 together with gray" in L.vd_last_error()
    assert call(6, 8, 4, 0) != 0 and b"divisible by scale" in L.vd_last_error()
    assert call(8, 8, 4, 0) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 2
ORACLE_CFG = dict(T=8, image_size=32, num_channels=64, num_res_blocks=1, rp_alpha=8, rp_beta=8, rp_gamma=8, timestep_respacing="ddim50")


def _oracle_case(masks):
    """The smallest window of test_use_gradient_method_vs_oracle_autograd: B = 2, T = 5, 2 observed, 64 channels, 32 x 32, ddim50."""
    cfg = {**vda.video_model_and_diffusion_defaults(), **ORACLE_CFG}
    model, diff, ora = _oracle(cfg)
    c = _rand_window(2, 5, 32, 2, seed=725)
    if masks == "marg_and_padding":                 # frame 2 kinda-marginalised, frame 4 in none of the masks
        c["latent_mask"][:, 2] = 0
        c["kinda_marg_mask"][:, 2] = 1
        c["latent_mask"][:, 4] = 0
    return model, diff, ora, c


def _oracle_grad(ora, c, t, y, s, gray):
    """Steps 2-4 composed in torch on the oracle's network with the window's real masks -> (grad of sum_b rho_b w.r.t. x_t, rho)."""
    sch = ora.s
    kwo = dict(x0=c["x0"], obs_mask=c["obs_mask"], latent_mask=c["latent_mask"], kinda_marg_mask=c["kinda_marg_mask"],
               frame_indices=c["frame_indices"], x_t_minus_1=c["x0"])
    x = c["x"].detach().clone().requires_grad_(True)
    tm = torch.tensor(sch.timestep_map, dtype=t.dtype)[t]
    coef = lambda tabl: torch.from_numpy(np.asarray(tabl))[t].float().view(-1, 1, 1, 1, 1)      # noqa: E731
    with torch.enable_grad():
        eps = ora.net.with_grad(x, tm, **kwo)
        x0 = (coef(sch.sqrt_recip_alphas_cumprod) * x - coef(sch.sqrt_recipm1_alphas_cumprod) * eps).clamp(-1, 1)
        r = (y - measure(x0, s, gray)) * c["latent_mask"]
        rho = r.reshape(r.shape[0], -1).pow(2).sum(dim=1).sqrt()
        g, = torch.autograd.grad(rho.sum(), x)
    return g, rho.detach()


def _dps_call(diff, model, mode, x, tt, kw, eta, noise, y, s, gray, zeta):
    with diff.dps_scope(model, y, s, gray, zeta=zeta):
        diff._step(mode, model, x, tt, True, None, kw, eta, noise)
    return diff._last_dps


@pytest.mark.parametrize("case", [(4, False, 0, 0.0, "plain"), (4, False, 1, 0.5, "plain"), (1, True, 0, 0.0, "plain"), (1, True, 1, 0.5, "plain"),
                                  (4, False, 0, 0.0, "marg_and_padding")], ids=lambda c: f"s{c[0]}-gray{int(c[1])}-mode{c[2]}-{c[4]}")
def test_step_gradient_vs_oracle_autograd(case):
    """The bars are test_use_gradient_method_vs_oracle_autograd's own: the same backward pass against the same oracle."""
    s, gray, mode, eta, masks = case
    model, diff, ora, c = _oracle_case(masks)
    g = torch.Generator().manual_seed(31)
    y = measure(torch.rand(c["x"].shape, generator=g) * 2 - 1, s, gray) + 0.1 * torch.randn(measure(c["x"], s, gray).shape, generator=g)
    noise = torch.randn(c["x"].shape, generator=g)
    t = torch.tensor([30, 30])
    want, want_rho = _oracle_grad(ora, c, t, y, s, gray)
    kw = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in c.items() if k != "x"}
    kw.update(x_t_minus_1=kw["x0"], observed_frames="x_0")
    out = _dps_call(diff, model, mode, c["x"].cuda(), t.cuda(), kw, eta, noise, y, s, gray, 0.5)
    scale = float(want.abs().max())
    err = (out["grad"].cpu() - want).abs()
    print(f"{case}: max |grad - ref| = {float(err.max()):.3e} = {float(err.max()) / scale:.3e} max |ref|; rho {out['residual_norm'].tolist()} ref {want_rho.tolist()}")
    assert scale > 0 and not out["grad"][:, :2].any()                           # observed frames: exactly 0
    if masks == "marg_and_padding":
        assert want[:, 4].abs().max() > 0                                       # the padding frame enters the network: its gradient is the network's own
    close(out["grad"].cpu(), want, atol=2e-4 * scale, rtol=1e-3)
    # residual_norm against the float64 norm of the engine's own pred_xstart, inside the restatement's bound for rho
    lat = _np(c["latent_mask"]).reshape(2, 5)
    x0 = _np(out["pred_xstart"]).astype(np.float64)
    rho, lim = seed_bound(x0, np.zeros_like(x0), _np(y.float()), lat, s, gray)["rho"]
    r = ratio(_np(out["residual_norm"]), rho, lim)
    print(f"  residual_norm: max |d| / bound = {r.max():.3f}")
    assert (r <= 1.0).all() and (rho > 1e-3).all()
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 3
def _fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays, exactly: the product is exact in float64, the sum's rounding error comes from TwoSum, and where the
    float64 sum lies on a float32 tie the error's sign decides."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    r = s.astype(np.float32)
    lo, hi = np.nextafter(r, np.float32(-np.inf)).astype(np.float64), np.nextafter(r, np.float32(np.inf)).astype(np.float64)
    r64 = r.astype(np.float64)
    up = (s - r64 == (hi - r64) / 2) & (e > 0)                                   # rounded down to even on a tie the true sum lies above
    down = (r64 - s == (r64 - lo) / 2) & (e < 0)
    return np.where(up, hi, np.where(down, lo, r64)).astype(np.float32)


@pytest.mark.parametrize("s,gray", STEP_OPERATORS)
@pytest.mark.parametrize("mode,eta", [(0, 0.0), (1, 0.5)])
def test_step_identities_bit_for_bit(mode, eta, s, gray):
    model, diff = tiny()
    N = diff.num_timesteps
    c = _rand_window(2, 6, 32, 2, seed=170)
    kw, x = _window_kw(c), c["x"].cuda()
    lat = _np(kw["latent_mask"]).reshape(2, 6) == 1
    g = torch.Generator().manual_seed(171)
    y = measure(torch.rand(tuple(x.shape), generator=g) * 2 - 1, s, gray) + 0.1 * torch.randn(measure(c["x"], s, gray).shape, generator=g)
    noise = torch.randn(x.shape, generator=g).cuda()
    zeta = 0.75
    for tv in (N - 1, 3, 0):
        tt = _t(2, tv)
        plain, plain_x0 = diff._fused_step(mode, model, x, tt, True, kw, eta=eta, noise=noise)
        out = _dps_call(diff, model, mode, x, tt, kw, eta, noise, y, s, gray, zeta)
        got, grad = _np(out["sample"]), _np(out["grad"])
        assert torch.equal(out["pred_xstart"], plain_x0)                        # pred_xstart: the plain step's
        assert _same_bits(got[~lat], _np(plain)[~lat])                           # every other frame: sample_plain's bits
        assert _same_bits(got[lat], _fma32(np.float32(-zeta), grad[lat], _np(plain)[lat]))
        assert not grad[:, :2].any() and np.abs(grad[lat]).max() > 0 and not np.array_equal(got[lat], _np(plain)[lat])
        zero = _dps_call(diff, model, mode, x, tt, kw, eta, noise, y, s, gray, 0.0)
        assert torch.equal(zero["sample"], plain) and torch.equal(zero["pred_xstart"], plain_x0)     # zeta = 0: the plain step entirely
        assert torch.equal(zero["grad"], out["grad"]) and torch.equal(zero["residual_norm"], out["residual_norm"])
        again, again_x0 = diff._fused_step(mode, model, x, tt, True, kw, eta=eta, noise=noise)
        assert torch.equal(again, plain) and torch.equal(again_x0, plain_x0)     # a plain step behind a DPS step: its usual bits
        rerun = _dps_call(diff, model, mode, x, tt, kw, eta, noise, y, s, gray, zeta)
        assert torch.equal(rerun["residual_norm"], out["residual_norm"])         # rho: the same bits on a rerun
    # the public entries: the dict gains 'residual_norm' and 'grad'; the sampler noise is drawn once, where the plain step draws it
    with diff.dps_scope(model, y, s, gray, zeta=zeta):
        torch.manual_seed(9)
        o = (diff.p_sample(model, x, _t(2, 3), model_kwargs=kw) if mode == 0 else diff.ddim_sample(model, x, _t(2, 3), model_kwargs=kw, eta=eta))
        after = torch.randn(3, device="cuda")
    torch.manual_seed(9)
    n1 = torch.randn_like(x)
    assert torch.equal(after, torch.randn(3, device="cuda"))
    want = _dps_call(diff, model, mode, x, _t(2, 3), kw, eta, n1, y, s, gray, zeta)
    assert torch.equal(o["sample"], want["sample"]) and torch.equal(o["grad"], want["grad"]) and o["residual_norm"].shape == (2,)
    assert "grad" not in diff.p_sample(model, x, _t(2, 3), model_kwargs=kw)
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 4
def test_loop_is_the_chain_of_steps():
    model, diff = tiny(timestep_respacing="logsnr3")
    c = _rand_window(2, 6, 32, 2, seed=180)
    kw, x = _window_kw(c), c["x"].cuda()
    y = measure(torch.rand(tuple(x.shape), generator=torch.Generator().manual_seed(181)) * 2 - 1, 4, False)
    with diff.dps_scope(model, y, 4, zeta=0.4):
        torch.manual_seed(11)
        got, _ = diff.p_sample_loop(model, tuple(x.shape), noise=x, model_kwargs=dict(kw))
        torch.manual_seed(11)
        noises = [torch.randn_like(x) for _ in range(3)]
        img = x
        for k, tv in enumerate((2, 1, 0)):
            img, _ = diff._step(0, model, img, _t(2, tv), True, None, kw, 0.0, noises[k])
    assert torch.equal(got, img) and torch.isfinite(got).all()
    with diff.dps_scope(model, y, 4, zeta=0.4):
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
    y = measure(torch.rand(2, 10, 3, 32, 32, generator=g) * 2 - 1, 4, False) + 0.05 * torch.randn(2, 10, 3, 8, 8, generator=g)
    torch.manual_seed(61)
    out, _ = vs.infer_video("autoreg", model, diff, batch, 6, 2, 4, measurement=y, sr_scale=4, dps_zeta=0.3)
    # the per-window eager chain: every window's tensors gathered by its frame indices, p_sample inside dps_scope
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
        with diff.dps_scope(model, y[:, fi], 4, zeta=0.3):
            for tv in (2, 1, 0):
                local = diff.p_sample(model, local, _t(2, tv), model_kwargs=kw)["sample"]
        samples[:, list(lat_i)] = local[:, -len(lat_i):].cpu()
        windows += 1
    assert windows == 2 and np.array_equal(out, samples.numpy()) and np.isfinite(out).all()
    assert np.array_equal(out[:, :2], batch[:, :2].cpu().numpy())
    torch.manual_seed(61)
    proj, _ = vs.infer_video("autoreg", model, diff, batch, 6, 2, 4, measurement=y, sr_scale=4)
    assert not np.array_equal(proj, out)                                         # without dps_zeta: the projection, as before
    model.check_device_errors()
    # the job: --dps_zeta; the suffixed run directory
    vids = (torch.rand(2, 8, 3, 32, 32, generator=g) * 2 - 1)
    np.save(tmp_path / "videos.npy", vids.numpy())
    np.save(tmp_path / "y.npy", measure(torch.rand(2, 8, 3, 32, 32, generator=g) * 2 - 1, 4, True).numpy())
    monkeypatch.chdir(tmp_path)
    args = vs.build_parser().parse_args(
        ["--videos", str(tmp_path / "videos.npy"), "--inference_mode", "autoreg", "--max_frames", "6", "--obs_length", "2", "--step_size", "4",
         "--batch_size", "2", "--timestep_respacing", "logsnr3", "--image_size", "32", "--num_channels", "32", "--num_res_blocks", "1",
         "--sampler", "ddim", "--eval_dir", str(tmp_path / "out"), "--measurement", str(tmp_path / "y.npy"), "--sr_scale", "4", "--gray",
         "--dps_zeta", "0.5"])
    out_dir = vs.run(args, device=torch.device("cuda", 0))
    assert str(out_dir).endswith("_ddim_sr4gray_dps0.5")
    for i in range(2):
        f = np.load(out_dir / "samples" / f"sample_{i:04d}-0.npy")
        assert f.dtype == np.uint8 and f.shape == (8, 3, 32, 32) and np.array_equal(f[:2], vs.to_uint8(vids.numpy()[i])[:2])


def test_window_of_32_frames_runs_and_33_is_refused():
    model, diff = long_engine(tiny_cfg(40, num_channels=64, timestep_respacing="ddim50"))
    for T, n_obs in ((32, 8), (33, 8)):
        c = rand_window(1, T, 32, n_obs, seed=41)
        kw = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in c.items() if k != "x"}
        kw.update(x_t_minus_1=kw["x0"], observed_frames="x_0")
        x = c["x"].cuda()
        y = measure(torch.rand(tuple(x.shape), generator=torch.Generator().manual_seed(42)) * 2 - 1, 4, False)
        with diff.dps_scope(model, y, 4, zeta=0.5):
            if T == 33:
                with pytest.raises(_lib.VdError, match=r"dps: windows of at most 32 frames.*got 33"):
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
    y = measure(torch.rand(tuple(x.shape), generator=torch.Generator().manual_seed(196)) * 2 - 1, 4, False)
    fn = lambda v: v                                                             # noqa: E731
    tt = _t(2, 3)
    with diff.dps_scope(model, y, 4, zeta=0.5):
        for call, what in ((lambda: diff.dpmpp_2m_sample(model, x, tt, model_kwargs=kw), "dpmpp_2m_sample"),
                           (lambda: diff.ddim_reverse_sample(model, x, tt, model_kwargs=kw), "ddim_reverse_sample"),
                           (lambda: diff.p_sample(model, x, tt, denoised_fn=fn, model_kwargs=kw), "denoised_fn"),
                           (lambda: diff.p_sample(model, x, tt, model_kwargs=kw, use_gradient_method=True), "use_gradient_method"),
                           (lambda: diff.p_sample(model, x, tt, model_kwargs=kw, return_attn_weights=True), "return_attn_weights"),
                           (lambda: diff.ddim_sample(model, x, tt, model_kwargs=kw, cfg_scale=2.0), "cfg_scale != 1"),
                           (lambda: WindowExecutor(model, diff).begin(x, kw), "WindowExecutor.begin")):
            with pytest.raises(_lib.VdError, match=f"{what} inside dps_scope is not served"):
                call()
        with diff.cfg_scale_scope(model, 2.0):
            with pytest.raises(_lib.VdError, match="cfg_scale != 1 .cfg_scale_scope. inside dps_scope"):
                diff.p_sample(model, x, tt, model_kwargs=kw)
        for opts in (dict(cfg_rescale=0.5), dict(dynamic_threshold=0.9)):
            with diff.guidance_scope(model, **opts):
                with pytest.raises(_lib.VdError, match="guidance_scope with cfg_rescale or dynamic_threshold set inside dps_scope"):
                    diff.p_sample(model, x, tt, model_kwargs=kw)
        with diff.known_region_scope(model, torch.zeros_like(x), torch.ones(2, 6, 32, 32, device="cuda")):
            with pytest.raises(_lib.VdError, match="known_region_scope inside dps_scope"):
                diff.p_sample(model, x, tt, model_kwargs=kw)
        with diff.measurement_scope(model, y, 4):
            with pytest.raises(_lib.VdError, match="measurement_scope inside dps_scope"):
                diff.ddim_sample(model, x, tt, model_kwargs=kw)
        with pytest.raises(ValueError, match="dps_scope: y"):
            diff.ddim_sample(model, x[:, :4], tt, model_kwargs={k: (v[:, :4] if torch.is_tensor(v) else v) for k, v in kw.items()})
    # the engine's own refusals, by message
    model._require_guidance()
    pk = model._pack_kwargs(x, kw)
    sample, xs = torch.empty_like(x), torch.empty_like(x)
    noise, yd = torch.zeros_like(x), y.cuda().float().contiguous()

    def step(sampler=0, zeta=0.5, scale=4, gray=0):
        return L.vd_dps_step(model._handle, 2, 6, *model._window_ptrs(x, pk), _lib.ptr(tt), pk["obs_mode"], 1, sampler, 0.0, _lib.ptr(noise),
                             _lib.ptr(yd), scale, gray, zeta, _lib.ptr(sample), _lib.ptr(xs), None, None, _lib.current_stream())
    for kwargs, what in ((dict(sampler=2), b"dps: p_sample (0) or ddim_sample (1)"), (dict(sampler=3), b"dps: p_sample (0) or ddim_sample (1)"),
                         (dict(zeta=-1.0), b"zeta must be finite and not negative"), (dict(zeta=float("nan")), b"zeta must be finite and not negative"),
                         (dict(zeta=float("inf")), b"zeta must be finite and not negative"), (dict(scale=3), b"scale is 2, 4 or 8"),
                         (dict(scale=1, gray=0), b"scale is 2, 4 or 8"), (dict(scale=64), b"scale is 2, 4 or 8")):
        assert step(**kwargs) != 0 and what in L.vd_last_error(), kwargs
    for setter, value, off, what in ((L.vd_set_cfg_scale, 2.0, 1.0, b"dps together with cfg_scale != 1"),
                                     (L.vd_set_guidance_rescale, 0.5, 0.0, b"dps together with guidance_rescale"),
                                     (L.vd_set_dynamic_threshold, 0.9, 0.0, b"dps together with dynamic_threshold")):
        _lib.check(setter(model._handle, value))
        assert step() != 0 and what in L.vd_last_error()
        _lib.check(setter(model._handle, off))
    with diff.measurement_scope(model, y, 4):
        assert step() != 0 and b"dps together with a measurement" in L.vd_last_error()
    with diff.known_region_scope(model, torch.zeros_like(x), torch.ones(2, 6, 32, 32, device="cuda")):
        assert step() != 0 and b"dps together with a known region" in L.vd_last_error()
    assert step() == 0                                                           # the engine is as it was: the step runs
    mx, dx_ = tiny(predict_xstart=True)
    with dx_.dps_scope(mx, y, 4, zeta=0.5):
        with pytest.raises(NotImplementedError, match="epsilon-prediction models only"):
            dx_.p_sample(mx, x, tt, model_kwargs=kw)
    dx_._bind(mx)
    mx._require_guidance()
    rc = L.vd_dps_step(mx._handle, 2, 6, *mx._window_ptrs(x, pk), _lib.ptr(tt), pk["obs_mode"], 1, 0, 0.0, _lib.ptr(noise), _lib.ptr(yd), 4, 0, 0.5,
                       _lib.ptr(sample), _lib.ptr(xs), None, None, _lib.current_stream())
    assert rc != 0 and b"dps: epsilon-prediction models only" in L.vd_last_error()
    fresh, dfresh = tiny(rp_alpha=7)                                             # a model whose backward image was never asked for
    dfresh._bind(fresh)
    rc = L.vd_dps_step(fresh._handle, 2, 6, *fresh._window_ptrs(x, pk), _lib.ptr(tt), pk["obs_mode"], 1, 0, 0.0, _lib.ptr(noise), _lib.ptr(yd), 4, 0, 0.5,
                       _lib.ptr(sample), _lib.ptr(xs), None, None, _lib.current_stream())
    assert rc != 0 and b"dps: the backward-data weight image is not on the device" in L.vd_last_error()
    torch.cuda.synchronize()
    model.check_device_errors()
