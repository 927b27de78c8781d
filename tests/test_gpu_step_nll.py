"""GPU: posterior_kernel, vb_terms_kernel / vb_final_kernel, prior_bpd_kernel, q_sample_kernel / q_sample_prev_kernel and randn_kernel
through their C entries, per element against the float64 restatements and derived bounds of tests/step_nll_restated.py, on the
inputs tests/test_step_nll_cpu.py proves those bounds on (a float32 restatement inside, thirteen seeded mistakes outside).  No entry
here runs the network except the one window-executor test.  Every test prints its largest |error| / bound."""
import json

import numpy as np
import pytest
import torch

import step_nll_restated as R
import video_diffusion_amd as vda
from helpers import load_npz, synth_sd
from video_diffusion_amd import _lib
from video_diffusion_amd.executor import WindowExecutor
from video_diffusion_amd.script_util import create_gaussian_diffusion

pytestmark = pytest.mark.gpu
F = np.float32
SCHED = dict(R.SCHEDULES)
NAMES = list(SCHED)
_state = {}


def bound(name):
    """The tiny engine the other tests build, with schedule `name` bound -> (model, diffusion, float32 tables)."""
    if "model" not in _state:
        cfg = json.loads(str(load_npz("unet_tiny.npz")["cfg_json"]))
        assert (cfg["image_size"], cfg["num_channels"], cfg["num_res_blocks"]) == (32, 32, 1)
        model, _ = vda.create_video_model_and_diffusion(**{k: cfg[k] for k in vda.video_model_and_diffusion_defaults()})
        model.load_state_dict(synth_sd(model.param_specs()))
        model.to("cuda")
        model.eval()
        _state["model"] = model
        _state["diff"] = {n: create_gaussian_diffusion(**SCHED[n]) for n in NAMES}
    model, diff = _state["model"], _state["diff"][name]
    diff._bind(model)
    _lib.check(_lib.lib().vd_set_model_mean_type(model._handle, 0))
    return model, diff, R.tables(diff)


def dev(v):
    return None if v is None else torch.from_numpy(np.ascontiguousarray(v)).cuda()


def host(v):
    return None if v is None else v.cpu().numpy()


def posterior(model, x, src, t, mode, eta, clip, noise, given, seed=0, offset=0, xstart=True, mean=True):
    """vd_posterior_update / vd_posterior_from_xstart on numpy inputs -> dict of numpy outputs (mean: the given form only)."""
    dx, ds, dt, dn = dev(x), dev(src), dev(np.asarray(t, np.int64)), dev(noise)
    B, per = x.shape
    out = {"sample": torch.empty_like(dx), "pred_xstart": torch.empty_like(dx) if xstart else None,
           "mean": torch.empty_like(dx) if (mean and given) else None}
    L = _lib.lib()
    if given:
        _lib.check(L.vd_posterior_from_xstart(model._handle, mode, B, per, _lib.ptr(dx), _lib.ptr(ds), _lib.ptr(dt), clip, eta, _lib.ptr(dn), seed, offset,
                                              _lib.ptr(out["sample"]), _lib.ptr(out["pred_xstart"]), _lib.ptr(out["mean"]), _lib.current_stream()))
    else:
        _lib.check(L.vd_posterior_update(model._handle, mode, B, per, _lib.ptr(dx), _lib.ptr(ds), _lib.ptr(dt), clip, eta, _lib.ptr(dn), seed, offset,
                                         _lib.ptr(out["sample"]), _lib.ptr(out["pred_xstart"]), _lib.current_stream()))
    return {k: host(v) for k, v in out.items() if v is not None}


def _fold(worst, r):
    for k, v in r.items():
        worst[k] = max(worst.get(k, 0.0), v)


# ------------------------------------------------------------------------------------------------------------ posterior
@pytest.mark.parametrize("name", NAMES)
def test_posterior_pass_per_element_against_float64(name):
    """sample, pred_xstart and (given x_0) mean inside posterior_bound: B = 3 x 1001 (items unaligned to 256 and to 4) for p_sample and
    DDIM at eta 0, 0.5, 1, clip on and off, from eps and from a given x_0, two mixed t vectors with 0, 1, NT - 2, NT - 1; B = 5 x 250 003
    (past 4096 blocks of 256) once per form.  Items at t == 0 equal the noise-free value, the others do not; without pred_xstart
    the sample is the same bits."""
    model, diff, tab = bound(name)
    worst = {}
    for large in (False, True):
        for (x, src, t, mode, eta, clip, noise, given) in R.posterior_cases(tab, large):
            got = posterior(model, x, src, t, mode, eta, clip, noise, given)
            r = R.posterior_ratios(tab, x, src, t, mode, eta, clip, noise, given, got)
            _fold(worst, r)
            assert max(r.values()) <= 1.0, (name, large, mode, eta, clip, given, t.tolist(), r)
            if clip:
                assert np.abs(got["pred_xstart"]).max() <= 1.0
            if large or (clip and eta in (0.0, 0.5)):
                quiet = posterior(model, x, src, t, mode, eta, clip, np.zeros_like(noise), given, mean=False)["sample"]
                same = np.array([np.array_equal(quiet[b], got["sample"][b]) for b in range(len(t))])
                want_same = (t == 0) | (mode == 1 and eta == 0.0)
                assert np.array_equal(same, want_same), (name, mode, eta, t.tolist(), same.tolist())
                only = posterior(model, x, src, t, mode, eta, clip, noise, given, xstart=False, mean=False)["sample"]
                assert np.array_equal(only, got["sample"])
    print(f"posterior_kernel {name}: max |d| / bound  " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    model.check_device_errors()


def test_in_kernel_philox_is_the_vd_randn_stream_past_2_to_the_32():
    """noise = NULL at (seed, offset) equals the same call on vd_randn(seed, offset), bit for bit, for an offset above 2^32 whose
    block counter also carries within the call; both forms of the pass."""
    model, diff, tab = bound("linear_ddim250")
    B, per = R.SMALL
    seed, offset = 2 ** 63 + 11, 2 ** 32 - 100                              # block offset + i // 4 passes 2^32 at element 400
    t = R.posterior_t(tab["NT"], B, 1)
    x, target, eps, _ = R.posterior_inputs(tab, t, per, seed=41)
    z = torch.empty(B * per, device="cuda")
    _lib.check(_lib.lib().vd_randn(_lib.ptr(z), z.numel(), seed, offset, _lib.current_stream()))
    z = host(z).reshape(B, per)
    for off2 in (offset, 2 ** 32 + 12345):
        if off2 != offset:
            z = torch.empty(B * per, device="cuda")
            _lib.check(_lib.lib().vd_randn(_lib.ptr(z), z.numel(), seed, off2, _lib.current_stream()))
            z = host(z).reshape(B, per)
        for mode, eta, given in ((0, 0.0, False), (1, 1.0, True)):
            src = target if given else eps
            a = posterior(model, x, src, t, mode, eta, 1, None, given, seed=seed, offset=off2)
            b = posterior(model, x, src, t, mode, eta, 1, z, given)
            assert np.array_equal(a["sample"], b["sample"]) and np.isfinite(a["sample"]).all(), (off2, mode)
            assert not np.array_equal(a["sample"], posterior(model, x, src, t, mode, eta, 1, None, given, seed=seed, offset=off2 + 1)["sample"])
    model.check_device_errors()


@pytest.mark.parametrize("name", NAMES)
def test_posterior_items_with_t_outside_the_table_are_poisoned_alone(name):
    """t = NT and t = -1 among good items (one row past the table at most): those items are NaN in every output, the good ones are the
    bits of a batch without them.  These network-free entries poison only: bit 0 stays clear (include/vd_amd.h)."""
    model, diff, tab = bound(name)
    NT = tab["NT"]
    per = R.SMALL[1]
    t = np.array([5, NT, 0, -1, NT - 1], np.int64)
    good = np.array([0, 2, 4])
    x, target, eps, noise = R.posterior_inputs(tab, np.where((t < 0) | (t >= NT), 0, t), per, seed=51)
    for mode, eta, given in ((0, 0.0, False), (1, 0.5, False), (0, 0.0, True), (1, 1.0, True)):
        src = target if given else eps
        got = posterior(model, x, src, t, mode, eta, 1, noise, given)
        ref = posterior(model, x[good], src[good], t[good], mode, eta, 1, noise[good], given)
        assert set(got) == ({"sample", "pred_xstart", "mean"} if given else {"sample", "pred_xstart"})
        for k in got:
            assert np.isnan(got[k][[1, 3]]).all(), (mode, given, k)
            assert np.array_equal(got[k][good], ref[k]) and np.isfinite(ref[k]).all(), (mode, given, k)
    model.check_device_errors()


def _nonfinite(name, kind):
    model, diff, tab = bound(name)
    model.check_device_errors()
    x, eps, t, noise = R.nonfinite_case(tab, (kind,))
    at = R.NONFINITE_AT[kind]
    clean = R.nonfinite_case(tab, ())[1]
    for mode, eta in ((0, 0.0), (1, 0.5)):
        got = posterior(model, x, eps, t, mode, eta, 1, noise, False)
        with pytest.raises(FloatingPointError):
            model.check_device_errors()
        model.check_device_errors()                                          # cleared by the read
        ref = posterior(model, x, clean, t, mode, eta, 1, noise, False)
        model.check_device_errors()
        for k in ("sample", "pred_xstart"):
            print(f"{name} {kind} eps, mode {mode}: {k} = {got[k][at]}")
            hit = np.zeros(x.shape, bool)
            hit[at] = True
            assert np.array_equal(got[k][~hit], ref[k][~hit]), (mode, k)
        yield mode, got, at


@pytest.mark.parametrize("name", NAMES)
def test_a_nan_eps_element_stays_nan_through_the_clamp_and_raises_bit_1(name):
    for mode, got, at in _nonfinite(name, "nan"):
        for k in ("sample", "pred_xstart"):
            assert np.isnan(got[k][at]) and np.isnan(got[k]).sum() == 1, (mode, k, got[k][at])


@pytest.mark.parametrize("name", NAMES)
def test_an_infinite_eps_element_is_nan_not_plus_minus_one(name):
    """With clip on, exactly the element whose eps is infinite is NaN in pred_xstart and sample, both modes, not +-1 and not an
    infinity (eps = +inf makes x_0 = sr x - srm1 inf = -inf, which p_sample's mean would carry on as -inf); bit 1 is raised."""
    seen = {}
    for mode, got, at in _nonfinite(name, "inf"):
        for k in ("sample", "pred_xstart"):
            assert not np.isin(got[k][at], (1.0, -1.0))
            seen[(mode, k)] = (float(got[k][at]), int(np.isnan(got[k]).sum()))
    assert all(np.isnan(v) and n == 1 for v, n in seen.values()), seen


# ------------------------------------------------------------------------------------------------------------ NLL terms
def vb_terms(model, T, xs, xt, src, noise, t, clip, mask, want_mse=True):
    """vd_vb_terms on (B, per) numpy inputs -> dict of numpy outputs."""
    B = xs.shape[0]
    d = [dev(v) for v in (xs, xt, src, noise, np.asarray(t, np.int64), mask)]
    out = dict(vb=torch.empty(B, device="cuda"), xstart_mse=torch.empty(B, device="cuda"),
               mse=torch.empty(B, device="cuda") if (want_mse and noise is not None) else None, pred_xstart=torch.empty_like(d[0]))
    _lib.check(_lib.lib().vd_vb_terms(model._handle, B, T, _lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]), _lib.ptr(d[3]), _lib.ptr(d[4]), clip,
                                      _lib.ptr(d[5]), _lib.ptr(out["vb"]), _lib.ptr(out["xstart_mse"]), _lib.ptr(out["mse"]), _lib.ptr(out["pred_xstart"]),
                                      _lib.current_stream()))
    return {k: host(v) for k, v in out.items() if v is not None}


@pytest.mark.parametrize("name", NAMES)
def test_nll_terms_per_element_through_constant_items(name):
    """T = 1 (per = 3072, one block): every item holds one scalar scenario in all its elements, so vb[b], xstart_mse[b] and mse[b] are
    that scenario's term.  The decoder grid at t = 0 -- x_start at and next to -0.999f / 0.999f, +-1, prediction errors from 0 to 40
    sigma_0, i.e. through the ill-conditioned points, the 1e-12 clamp and a saturated tanhf -- and the KL grid at t in {1, 2, NT / 2, NT - 1};
    clip on and off, EPSILON and START_X engine, with and without noise.  vb inside vb_term_interval / ln 2, the squared errors and
    pred_xstart inside their rounding bounds."""
    model, diff, tab = bound(name)
    per, worst = 3072, {}
    try:
        for clip, start_x, with_noise in R.VB_CALLS:
            _lib.check(_lib.lib().vd_set_model_mean_type(model._handle, 1 if start_x else 0))
            xs, xt, src, noise, t = R.vb_grid(tab, start_x)
            wide = lambda v: np.ascontiguousarray(np.broadcast_to(v[:, None], (len(v), per)))  # noqa: E731
            nz = wide(noise) if with_noise else None
            got = vb_terms(model, 1, wide(xs), wide(xt), wide(src), nz, t, clip, None)
            assert (got["pred_xstart"] == got["pred_xstart"][:, :1]).all() and ("mse" in got) == with_noise
            got["pred_xstart"] = got["pred_xstart"][:, :1]
            col = lambda v: v[:, None]  # noqa: E731
            r = R.vb_ratios(tab, col(xs), col(xt), col(src), t, clip, start_x, col(noise) if with_noise else None, np.ones((len(xs), 1)), got)
            _fold(worst, r)
            assert max(r.values()) <= 1.0, (name, clip, start_x, with_noise, r)
    finally:
        _lib.check(_lib.lib().vd_set_model_mean_type(model._handle, 0))
    print(f"vb_terms_kernel {name} (per element): max ratio  " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    model.check_device_errors()


@pytest.mark.parametrize("T,B", [(5, 3), (128, 2)])
@pytest.mark.parametrize("name", NAMES)
def test_masked_sums_against_the_float64_mean(name, T, B):
    """Per-frame masks of 0, 1 and 0.5 (index j / fsz) and latent_mask = NULL as all ones, on well-conditioned data: every output inside
    the mean over ALL elements of the per-element intervals plus one float32 cast.  T = 128: per = 393 216, vb_terms_blocks at its cap
    of 64 blocks, 24 strides per thread; vd_prior_bpd on the same data."""
    model, diff, tab = bound(name)
    per, worst = T * 3072, {}
    xs, xt, eps, noise, t, mask = R.masked_inputs(tab, B, T, per, seed=20 + T)
    for mk in (mask, None):
        m = R.elem_mask(mk, B, T, per)
        got = vb_terms(model, T, xs, xt, eps, noise, t, 1, mk)
        r = R.vb_ratios(tab, xs, xt, eps, t, 1, False, noise, m, got)
        out, d = torch.empty(B, device="cuda"), [dev(xs), dev(mk)]
        _lib.check(_lib.lib().vd_prior_bpd(model._handle, B, T, _lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(out), _lib.current_stream()))
        r["prior"] = float(R.ratio_in(host(out), *R.prior_bpd_interval(tab, xs, m)).max())
        lo, hi = R.prior_bpd_interval(tab, xs, m)
        want = R.prior_bpd_fp64(tab, xs, m)
        assert ((want >= lo) & (want <= hi)).all()
        _fold(worst, r)
        assert max(r.values()) <= 1.0, (name, T, mk is None, r)
    print(f"vb_terms_kernel / prior_bpd_kernel {name} T={T}: max ratio  " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    if T == 5:                                                                # mse needs the noise x_t was drawn with: refused by name
        d = [dev(v) for v in (xs, xt, eps, np.asarray(t, np.int64))]
        o = torch.empty(B, device="cuda")
        rc = _lib.lib().vd_vb_terms(model._handle, B, T, _lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]), None, _lib.ptr(d[3]), 1, None, _lib.ptr(o), None,
                                    _lib.ptr(o), None, _lib.current_stream())
        assert rc != 0 and b"mse needs the noise" in _lib.lib().vd_last_error()
    model.check_device_errors()


@pytest.mark.parametrize("name", NAMES)
def test_nll_item_with_t_outside_the_table_is_nan_and_raises_index_error(name):
    model, diff, tab = bound(name)
    NT, T, B = tab["NT"], 5, 3
    xs, xt, eps, noise, t, mask = R.masked_inputs(tab, B, T, T * 3072, seed=77)
    model.check_device_errors()
    ref = vb_terms(model, T, xs[[0, 2]], xt[[0, 2]], eps[[0, 2]], noise[[0, 2]], t[[0, 2]], 1, mask[[0, 2]])
    model.check_device_errors()
    for bad in (NT, -1):
        tb = t.copy()
        tb[1] = bad
        got = vb_terms(model, T, xs, xt, eps, noise, tb, 1, mask)
        for k in ("vb", "xstart_mse", "mse", "pred_xstart"):
            assert np.isnan(got[k][1]).all(), (bad, k)
            assert np.array_equal(got[k][[0, 2]], ref[k]) and np.isfinite(ref[k]).all(), (bad, k)
        with pytest.raises(IndexError):
            model.check_device_errors()
        model.check_device_errors()                                          # cleared by the read


# ------------------------------------------------------------------------------------------------------------ q_sample
def q_sample(model, x0, t, noise):
    out = torch.empty(x0.shape, device="cuda")
    B, per = x0.shape
    d = [dev(x0), dev(np.asarray(t, np.int64)), dev(noise)]               # held until the result is back
    _lib.check(_lib.lib().vd_q_sample(model._handle, B, per, _lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]), _lib.ptr(out), _lib.current_stream()))
    return host(out)


@pytest.mark.parametrize("name", NAMES)
def test_q_sample_per_element_with_the_wrap_of_index_minus_1(name):
    model, diff, tab = bound(name)
    NT, worst = tab["NT"], 0.0
    for B, per in ((4, 1001), (3, 400_003)):
        x0, t, noise = R.q_sample_inputs(NT, B, per, seed=31)
        assert {0, NT - 1, -1} <= set(t.tolist())
        got = q_sample(model, x0, t, noise)
        r = float(R.ratio(got, *R.q_sample_bound(tab, x0, t, noise)).max())
        worst = max(worst, r)
        assert r <= 1.0, (name, B, per, r)
        assert np.array_equal(got, q_sample(model, x0, np.where(t == -1, NT - 1, t), noise))     # -1 is the last row, bit for bit
        for bad in (NT, -NT - 1):
            tb = t.copy()
            tb[1] = bad
            out = q_sample(model, x0, tb, noise)
            keep = np.arange(B) != 1
            assert np.isnan(out[1]).all() and np.array_equal(out[keep], got[keep])
    print(f"q_sample_kernel {name}: max |d| / bound {worst:.3f}")
    model.check_device_errors()


def _window(B, T, n_obs, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(B, T, 3, 32, 32, generator=g) * 2 - 1
    x = torch.randn(B, T, 3, 32, 32, generator=g)
    obs = torch.zeros(B, T, 1, 1, 1)
    obs[:, :n_obs] = 1
    kw = dict(x0=x0.cuda(), obs_mask=obs.cuda(), latent_mask=(1 - obs).cuda(), kinda_marg_mask=torch.zeros(B, T, 1, 1, 1).cuda(),
              frame_indices=torch.arange(T).view(1, T).repeat(B, 1).cuda())
    return x.cuda(), dict(kw, x_t_minus_1=kw["x0"], observed_frames="x_t_minus_1")


def test_q_sample_prev_in_the_window_executor_at_the_last_and_the_first_index():
    """The executor keeps the re-noised observed frames in an engine-owned buffer it does not expose, so q_sample_prev_kernel is
    compared through the replay test_window_executor_equals_eager_steps_bit_for_bit does: one captured step with
    observed_frames = 'x_t_minus_1', renoise on, equals vd_p_sample on obs_src = vd_q_sample(x0, t - 1, vd_randn(seed, B per / 2)) to the
    bit -- at the last index, and at the first, where t - 1 = -1 wraps to the last row -- and that obs_src is inside the bound of
    q_sample_fp64(x0, t - 1, normal_fp64(seed, B per / 2, i)), the noise's own tolerance carried through sqrt(1 - acp)."""
    model, diff, tab = bound("linear_ddim250")
    NT, L = tab["NT"], _lib.lib()
    ex = WindowExecutor(model, diff)
    B, T = 2, 4
    x_init, kw = _window(B, T, 2, seed=61)
    per = x_init[0].numel()
    worst = 0.0
    for wi, t_start in enumerate((NT - 1, 0)):
        seed = 900 + wi
        ex.begin(x_init, kw, t_start=t_start, seed=seed, sampler="p_sample", renoise=True)
        got = ex.run(1).clone()
        t = torch.full((B,), t_start, dtype=torch.int64, device="cuda")
        nz, obs_src, nxt = torch.empty_like(x_init), torch.empty_like(x_init), torch.empty_like(x_init)
        _lib.check(L.vd_randn(_lib.ptr(nz), nz.numel(), seed, B * per // 2, _lib.current_stream()))
        x0d = kw["x0"].float().contiguous()
        _lib.check(L.vd_q_sample(model._handle, B, per, _lib.ptr(x0d), _lib.ptr(t - 1), _lib.ptr(nz), _lib.ptr(obs_src), _lib.current_stream()))
        k = model._pack_kwargs(x_init, kw)
        _lib.check(L.vd_p_sample(model._handle, B, T, _lib.ptr(x_init), _lib.ptr(obs_src), _lib.ptr(k["obs_mask"]), _lib.ptr(k["latent_mask"]),
                                 _lib.ptr(k["kinda_marg_mask"]), _lib.ptr(k["frame_indices"]), _lib.ptr(t), k["obs_mode"], 1, None, seed, 0,
                                 _lib.ptr(nxt), None, None, _lib.current_stream()))
        assert torch.equal(nxt, got) and torch.isfinite(got).all(), (t_start, float((nxt - got).abs().max()))
        z, rad = R.normal_fp64(seed, B * per // 2, np.arange(B * per))
        tm1 = np.full(B, t_start - 1)
        x0n = host(x0d).reshape(B, per)
        want, lim = R.q_sample_bound(tab, x0n, tm1, z.reshape(B, per).astype(F))
        want = R.q_sample_fp64(tab, x0n, tm1, z.reshape(B, per))
        lim = lim + float(tab["s1"][(t_start - 1) % NT]) * (R.normal_bound(rad).reshape(B, per) + R.U * np.abs(z.reshape(B, per)))
        r = float(R.ratio(host(obs_src).reshape(B, per), want, lim).max())
        worst = max(worst, r)
        assert r <= 1.0, (t_start, r)
    print(f"q_sample_prev_kernel (through the replay): max |d| / bound {worst:.3f}")
    model.check_device_errors()


# ------------------------------------------------------------------------------------------------------------ randn
def randn(n, seed, offset):
    out = torch.empty(n, device="cuda")
    _lib.check(_lib.lib().vd_randn(_lib.ptr(out), n, seed, offset, _lib.current_stream()))
    return host(out)


@pytest.mark.parametrize("seed,offset", R.RANDN_CASES + [R.RANDN_SMALL_U1[:2]])
def test_randn_is_philox4x32_10_with_box_muller_element_by_element(seed, offset):
    """n = 4099 elements within 16 2^-24 max(1, rad) of normal_fp64 (the width is generous: one wrong bit in Philox, in the counter
    layout or in the (0, 1] mapping moves a value by order 1); the stream at offset + 1 is this one from element 4 on, bit for bit.
    The last plain case carries offset + i / 4 into the counter's high word; the fourth holds a Philox word of 526 in a u1 slot."""
    n = R.RANDN_N
    got = randn(n, seed, offset)
    want, rad = R.normal_fp64(seed, offset, np.arange(n))
    r = R.ratio(got, want, R.normal_bound(rad))
    print(f"randn_kernel seed={seed} offset={offset}: max |d| / bound {r.max():.3f}, max |d| {np.abs(got - want).max():.3e}")
    assert r.max() <= 1.0, (seed, offset, float(r.max()), int(r.argmax()))
    nxt = randn(n, seed, offset + 1)
    assert np.array_equal(nxt[:n - 4], got[4:])
    assert np.abs(nxt[n - 4:] - R.normal_fp64(seed, offset, np.arange(n, n + 4))[0]).max() < 1e-4


# ------------------------------------------------------------------------------------------------------------ one x_0 head
@pytest.mark.parametrize("clip", [True, False], ids=["clip", "noclip"])
@pytest.mark.parametrize("start_x", [False, True], ids=["eps", "predict_xstart"])
def test_pred_xstart_is_one_bit_pattern_in_all_five_step_entries(start_x, clip):
    """What the shared x_0 head of the sampler passes is for: on the same window, the same x and per-item t = {0, last index},
    vd_p_mean_variance, vd_p_sample, vd_ddim_sample, vd_ddim_reverse_sample and vd_dpmpp_2m_sample (no history) return the same
    pred_xstart, compared as int32 bit patterns -- for an epsilon model (x_0 = two rounded products and one subtraction in every pass)
    and a predict_xstart model (the network output itself), with and without the clamp.  The forward is deterministic, so the five
    passes read the same network output.  (The separate kernels this head replaced passed the same four cases: the test pins
    behaviour the library had, it does not depend on the compiler's contraction default any more.)"""
    key = ("x0_head", start_x)
    if key not in _state:
        cfg = dict(vda.video_model_and_diffusion_defaults(), T=6, image_size=32, num_channels=64, num_res_blocks=1, rp_alpha=6, rp_beta=6,
                   rp_gamma=6, timestep_respacing="logsnr10", predict_xstart=start_x)
        model, diff = vda.create_video_model_and_diffusion(**cfg)
        model.load_state_dict(synth_sd(model.param_specs()))
        model.to("cuda")
        model.eval()
        _state[key] = (model, diff)
    model, diff = _state[key]
    assert diff.model_mean_type.name == ("START_X" if start_x else "EPSILON") and diff.num_timesteps == 10
    B, T = 2, 6
    x, kw = _window(B, T, 2, seed=71)
    kw = dict(kw, observed_frames="x_0")
    t = torch.tensor([0, diff.num_timesteps - 1], device="cuda")
    steps = {"p_mean_variance": diff.p_mean_variance, "p_sample": diff.p_sample, "ddim_sample": diff.ddim_sample,
             "ddim_reverse_sample": diff.ddim_reverse_sample, "dpmpp_2m_sample": diff.dpmpp_2m_sample}
    got = {name: f(model, x, t, clip_denoised=clip, model_kwargs=kw)["pred_xstart"] for name, f in steps.items()}
    model.check_device_errors()
    want = got["p_mean_variance"]
    assert torch.isfinite(want).all() and (not clip or float(want.abs().max()) <= 1.0)
    assert not torch.equal(want[0], want[1])
    for name, v in got.items():
        diffs = int((v.view(torch.int32) != want.view(torch.int32)).sum())
        print(f"pred_xstart {name} vs p_mean_variance ({'START_X' if start_x else 'EPSILON'}, clip={clip}): {diffs} differing bit patterns")
        assert diffs == 0, (name, diffs)
