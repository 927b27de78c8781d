"""CPU: tests/step_nll_restated.py is anchored to what the imported reference recorded (tests/golden/psample_tiny.npz, nll_tiny.npz)
and to the oracle, its Philox to known answers; a numpy-float32 restatement in the reference's operation order stays inside every
bound on the inputs tests/test_gpu_step_nll.py runs the kernels on, fused or not; and each of thirteen seeded mistakes leaves a
bound on those same inputs.  No GPU, no library call."""
import functools
import json

import numpy as np
import pytest
import torch

import step_nll_restated as R
from helpers import load_npz
from oracle import losses_ref
from oracle.sampler_ref import SamplerRef
from oracle.schedule_ref import ScheduleRef
from video_diffusion_amd.script_util import create_gaussian_diffusion

F = np.float32
SCHED = dict(R.SCHEDULES)


@functools.lru_cache(maxsize=None)
def tab_of(name):
    return R.tables(create_gaussian_diffusion(**SCHED[name]))


def _flat(v):
    return np.ascontiguousarray(v).reshape(v.shape[0], -1)


# ------------------------------------------------------------------------------------------------------------ anchors
def test_tables_are_the_rows_the_engine_is_handed():
    for name in SCHED:
        diff = create_gaussian_diffusion(**SCHED[name])
        up, tab = diff._device_tables(), R.tables(diff)
        for row, key in enumerate(["sr", "srm1", "c1", "c2", "lv", "ab", "abp", "sa", "s1", "tlv", "l1m"]):
            assert np.array_equal(up[row], tab[key]), (name, key)
        kw = {k: v for k, v in SCHED[name].items()}
        assert np.array_equal(R.tables(ScheduleRef(rescale_timesteps=False, **kw))["lv"], tab["lv"])      # the oracle's tables too
    assert tab_of("linear_ddim250")["NT"] == 250 and tab_of("cosine_1000_small")["NT"] == 1000
    assert abs(float(tab_of("linear_ddim250")["srm1"][0]) - 0.0100) < 1e-4 and abs(float(tab_of("cosine_1000_small")["srm1"][0]) - 0.0064) < 1e-4
    assert np.array_equal(tab_of("cosine_1000_small")["lv"], tab_of("cosine_1000_small")["tlv"])           # sigma_small
    assert not np.array_equal(tab_of("linear_1000")["lv"], tab_of("linear_1000")["tlv"])


def test_philox_known_answers():
    assert [f"{v:08x}" for v in R.philox4x32_10([0, 0, 0, 0], [0, 0])] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    got = R.philox4x32_10([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0])
    assert [f"{v:08x}" for v in got] == ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]
    # the array form is the integer form; the counter's low word carries into the high one; the key is the seed's two halves
    seed, off = 2 ** 63 + 11, 2 ** 32 - 2
    w = R.philox_words(seed, off, np.arange(16))
    for i in (0, 7, 8, 15):
        ctr = off + i // 4
        want = R.philox4x32_10([ctr & R.M32, ctr >> 32, 0x5EED5EED, 0], [seed & R.M32, seed >> 32])
        assert [int(v) for v in w[:, i]] == list(want), i
    assert (off + 8 // 4) >> 32 == 1
    seed, off, i, word = R.RANDN_SMALL_U1
    assert int(R.philox_words(seed, off, np.array([i]))[0, 0]) == word and i < R.RANDN_N
    # elements 4q .. 4q+3 share block q; the stream at offset + 1 is the stream at offset from element 4 on
    a, _ = R.normal_fp64(5, 7, np.arange(4, 44))
    b, _ = R.normal_fp64(5, 8, np.arange(0, 40))
    assert np.array_equal(a, b)
    z, rad = R.normal_fp64(0, 0, np.arange(200000))
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1.0) < 0.01 and np.isfinite(z).all() and (rad >= 0).all()


def test_posterior_and_q_sample_reproduce_the_recorded_reference_steps():
    """x, noise and the recorded pred_xstart handed over as a given x_0: the reference's own float32 results lie inside the bounds
    of its float64 restatement, at t = 249, 248, 1, 0 of linear ddim250; so does the oracle's torch-float32 arithmetic from eps."""
    rec = load_npz("psample_tiny.npz")
    tab = tab_of("linear_ddim250")
    x, noise = _flat(rec["x"]), _flat(rec["noise"])
    B = x.shape[0]
    ora = SamplerRef(ScheduleRef(timestep_respacing="ddim250"), None)
    for tv in (249, 248, 1, 0):
        t = np.full(B, tv)
        x0p = _flat(rec[f"t{tv}_pred_xstart"])
        for key, mode, eta in ((f"t{tv}_psample", 0, 0.0), (f"t{tv}_ddim_eta0", 1, 0.0), (f"t{tv}_ddim_eta1", 1, 1.0)):
            r = R.posterior_ratios(tab, x, x0p, t, mode, eta, True, noise, True,
                                   dict(sample=_flat(rec[key]), mean=_flat(rec[f"t{tv}_mean"]), pred_xstart=x0p))
            assert max(r.values()) <= 1.0, (key, r)
        assert np.array_equal(_flat(rec[f"t{tv}_sample"]), _flat(rec[f"t{tv}_psample"]))
        # the oracle from an eps that reproduces the recorded x_0 to within rounding
        c = R._rows32(tab, t)
        eps = ((c["sr"] * x - x0p) / c["srm1"]).astype(F)
        tt, shape = torch.tensor(t), rec["x"].shape
        for clip in (True, False):
            o = ora.p_sample(torch.from_numpy(x).view(shape), tt, None, torch.from_numpy(noise).view(shape), clip=clip, eps=torch.from_numpy(eps).view(shape))
            r = R.posterior_ratios(tab, x, eps, t, 0, 0.0, clip, noise, False, {k: _flat(o[k].numpy()) for k in ("sample", "mean", "pred_xstart")})
            assert max(r.values()) <= 1.0, (tv, clip, r)
            for eta in (0.0, 0.5, 1.0):
                o = ora.ddim_sample(torch.from_numpy(x).view(shape), tt, None, torch.from_numpy(noise).view(shape), eta=eta, clip=clip,
                                    eps=torch.from_numpy(eps).view(shape))
                r = R.posterior_ratios(tab, x, eps, t, 1, eta, clip, noise, False, dict(sample=_flat(o["sample"].numpy())))
                assert r["sample"] <= 1.0, (tv, clip, eta, r)
    x0 = _flat(rec["x0"])
    want, lim = R.q_sample_bound(tab, x0, np.full(B, 3), noise)
    assert R.ratio(_flat(rec["q_sample_t3"]), want, lim).max() <= 1.0
    q = ora.q_sample(torch.from_numpy(x0), torch.tensor([0, 249]), torch.from_numpy(noise)).numpy()
    assert R.ratio(q, *R.q_sample_bound(tab, x0, np.array([-250, -1]), noise)).max() <= 1.0          # negative indices count from the end
    assert np.isnan(R.q_sample_fp64(tab, x0, np.array([250, -251]), noise)).all()


# torch's float32 mean over n elements (a cascade of partial sums): at most (log2 n + 4) roundings of 2^-24 on the mean of |values|
def _sum32(v, m, bits):
    n = v.shape[1]
    return (np.log2(n) + 4.0) * R.U * (np.abs(v) * m).mean(axis=1) / (np.log(2.0) if bits else 1.0)


def test_nll_terms_hold_the_recorded_reference_values():
    """From the recorded pred_xstart, x_t, x0 and the mask: t*_vb_clip1, t*_vb_nomask, prior_bpd and prior_bpd_nomask lie inside the
    mean of the per-element intervals (widened by what the reference's float32 mean adds, which the engine's float64 sums do not
    have); the oracle's per-element losses lie inside the per-element intervals."""
    rec = load_npz("nll_tiny.npz")
    cfg = json.loads(str(rec["cfg_json"]))
    diff = create_gaussian_diffusion(steps=cfg["diffusion_steps"], sigma_small=cfg["sigma_small"], noise_schedule=cfg["noise_schedule"],
                                     timestep_respacing=cfg["timestep_respacing"])
    tab = R.tables(diff)
    xs = _flat(rec["x0"])
    B, per = xs.shape
    T = rec["x0"].shape[1]
    masks = {"clip1": R.elem_mask(rec["latent_mask"], B, T, per), "nomask": R.elem_mask(None, B, T, per)}
    for tv in (4, 2, 0):
        t = np.full(B, tv)
        xt, x0p = _flat(rec[f"t{tv}_x_t"]), _flat(rec[f"t{tv}_pred_xstart"])
        lo, hi = R.vb_term_interval(tab, xs, xt, x0p, t)
        assert (lo <= hi).all()
        for key, m in masks.items():
            ilo, ihi = R.item_mean(lo, hi, m, bits=True)
            slack = _sum32(np.maximum(np.abs(lo), np.abs(hi)), m, True)
            got = rec[f"t{tv}_vb_{key}"].astype(np.float64)
            assert ((got >= ilo - slack) & (got <= ihi + slack)).all(), (tv, key, got, ilo, ihi)
            assert ((ihi - ilo) <= 2e-4 * np.abs(got)).all(), (tv, key)      # and the interval says something: well-conditioned data
        # the oracle's losses, per element
        c = R._rows32(tab, t)
        mean = torch.from_numpy((c["c1"] * x0p + c["c2"] * xt).astype(F))
        lv = torch.from_numpy(np.broadcast_to(c["lv"], xs.shape).copy())
        if tv == 0:
            term = -losses_ref.discretized_gaussian_log_likelihood(torch.from_numpy(xs), means=mean, log_scales=0.5 * lv)
        else:
            tmean = torch.from_numpy((c["c1"] * xs + c["c2"] * xt).astype(F))
            term = losses_ref.normal_kl(tmean, torch.from_numpy(np.broadcast_to(c["tlv"], xs.shape).copy()), mean, lv)
        assert R.ratio_in(term.numpy(), lo, hi).max() <= 1.0, tv
    for key, m in (("prior_bpd", masks["clip1"]), ("prior_bpd_nomask", masks["nomask"])):
        ilo, ihi = R.prior_bpd_interval(tab, xs, m)
        want = R.prior_bpd_fp64(tab, xs, m)
        slack = _sum32(np.abs(R._prior(R.Ex, tab, xs).lo), m, True)
        got = rec[key].astype(np.float64)
        assert ((want >= ilo) & (want <= ihi)).all() and ((got >= ilo - slack) & (got <= ihi + slack)).all(), (key, got, ilo, ihi)
    ora = SamplerRef(ScheduleRef(timestep_respacing=cfg["timestep_respacing"]), None)
    got = ora.prior_bpd(torch.from_numpy(rec["x0"]), torch.from_numpy(rec["latent_mask"])).numpy().astype(np.float64)
    ilo, ihi = R.prior_bpd_interval(tab, xs, masks["clip1"])
    slack = _sum32(np.abs(R._prior(R.Ex, tab, xs).lo), masks["clip1"], True)
    assert ((got >= ilo - slack) & (got <= ihi + slack)).all()


def test_the_decoder_interval_follows_the_conditioning():
    """The figures the comparison is built around (linear ddim250, t = 0, sigma_0 = 0.00926): float32 and float64 agree to 2e-6 up to
    3 sigma, differ by 4e-4 at 4 sigma and by 6.4 at 6 sigma, where float32 has reached the clamp -- and the interval holds both."""
    tab = tab_of("linear_ddim250")
    sig0 = float(np.exp(0.5 * np.float64(tab["lv"][0])))
    assert abs(sig0 - 0.00926) < 1e-5
    ks = np.array([0.0, 1.0, 3.0, 4.0, 6.0])
    xs = np.zeros((5, 1), F)
    x0 = (-ks * sig0).astype(F)[:, None]
    t = np.zeros(5, np.int64)
    lo, hi = R.vb_term_interval(tab, xs, xs, x0, t)
    f32 = R.vb_terms_f32(tab, xs, xs, x0, t, False, 1, start_x=True)["term"].astype(np.float64)
    cx = xs.astype(np.float64) - x0.astype(np.float64)
    inv, q = np.exp(-0.5 * np.float64(tab["lv"][0])), float(F(1 / 255.0))
    f64 = -np.log(np.maximum(R._cdf(inv * (cx + q)) - R._cdf(inv * (cx - q)), 1e-12))
    d = np.abs(f32 - f64)[:, 0]
    assert (d[:3] < 2e-6).all() and 1e-4 < d[3] < 1e-3 and abs(f64[3, 0] - 8.98545) < 1e-4 and d[4] > 6.0 and abs(f32[4, 0] - 27.631) < 1e-3
    assert ((f32 >= lo) & (f32 <= hi) & (f64 >= lo) & (f64 <= hi)).all()
    assert (hi - lo)[:2].max() < 2e-5 and (hi - lo)[2, 0] < 1e-3 and (hi - lo)[4, 0] > 6.0     # narrow where the term is well-conditioned


# ------------------------------------------------------------------------------------------------------------ the inputs, once
def _posterior_worst(name, fused=False, mistake=None, large=False):
    tab, worst = tab_of(name), 0.0
    for (x, src, t, mode, eta, clip, noise, given) in R.posterior_cases(tab, large):
        got = R.posterior_f32(tab, x, src, t, mode, eta, clip, noise, given, fused=fused, mistake=mistake)
        worst = max(worst, *R.posterior_ratios(tab, x, src, t, mode, eta, clip, noise, given, got).values())
    x, eps, t, noise = R.nonfinite_case(tab)
    for mode in (0, 1):
        got = R.posterior_f32(tab, x, eps, t, mode, 0.5, 1, noise, False, fused=fused, mistake=mistake)
        worst = max(worst, *R.posterior_ratios(tab, x, eps, t, mode, 0.5, 1, noise, False, got).values())
    return worst


def _vb_worst(name, fused=False, mistake=None, big=False):
    tab, worst = tab_of(name), {}

    def fold(r):
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    for clip, start_x, with_noise in R.VB_CALLS:
        xs, xt, src, noise, t = (v[:, None] if v.dtype != np.int64 else v for v in R.vb_grid(tab, start_x))
        nz = noise if with_noise else None
        got = R.vb_terms_f32(tab, xs, xt, src, t, clip, 1, start_x=start_x, noise=nz, fused=fused, mistake=mistake)
        fold(R.vb_ratios(tab, xs, xt, src, t, clip, start_x, nz, np.ones_like(xs, np.float64), got))
    for (B, T) in ([(3, 5), (2, 128)] if big else [(3, 5)]):
        per = T * 3072
        xs, xt, eps, noise, t, mask = R.masked_inputs(tab, B, T, per, seed=20 + T)
        for use_mask in (True, False):
            mk = mask if use_mask else None
            got = R.vb_terms_f32(tab, xs, xt, eps, t, 1, T, mask=mk, noise=noise, fused=fused, mistake=mistake)
            fold(R.vb_ratios(tab, xs, xt, eps, t, 1, False, noise, R.elem_mask(mk, B, T, per), got))
            if mistake is None:
                m = R.elem_mask(mk, B, T, per)
                fold({"prior": float(R.ratio_in(R.prior_bpd_f32(tab, xs, m, fused), *R.prior_bpd_interval(tab, xs, m)).max())})
    return worst


def _q_worst(name, fused=False, mistake=None, large=False):
    tab, worst = tab_of(name), 0.0
    for B, per in ([(4, 1001), (3, 400_003)] if large else [(4, 1001)]):
        x0, t, noise = R.q_sample_inputs(tab["NT"], B, per, seed=31)
        worst = max(worst, float(R.ratio(R.q_sample_f32(tab, x0, t, noise, fused, mistake), *R.q_sample_bound(tab, x0, t, noise)).max()))
    return worst


def _randn_worst(mistake=None):
    worst = 0.0
    for seed, off in R.RANDN_CASES + [R.RANDN_SMALL_U1[:2]]:
        i = np.arange(R.RANDN_N)
        want, rad = R.normal_fp64(seed, off, i)
        worst = max(worst, float(R.ratio(R.normal_f32(seed, off, i, mistake), want, R.normal_bound(rad)).max()))
    return worst


# ------------------------------------------------------------------------------------------------------------ the bounds are honest
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", list(SCHED))
def test_float32_restatement_is_inside_every_bound(name, fused):
    """All elements, the ill-conditioned decoder points at 4, 5, 6, 7 sigma and beyond saturation included; the large shapes once."""
    big = name == "linear_ddim250"
    p = _posterior_worst(name, fused)
    if big:
        p = max(p, _posterior_worst(name, fused, large=True))
    v = _vb_worst(name, fused, big=big)
    q = _q_worst(name, fused, large=big)
    print(f"{name} fused={fused}: posterior {p:.3f}  q_sample {q:.3f}  " + "  ".join(f"{k} {x:.3f}" for k, x in v.items()))
    assert p <= 1.0 and q <= 1.0 and max(v.values()) <= 1.0, (p, q, v)


def test_float32_box_muller_is_inside_the_bound():
    r = _randn_worst()
    print(f"randn: {r:.3f}")
    assert r <= 1.0


def test_the_grid_reaches_every_branch_and_the_clamp():
    tab = tab_of("linear_ddim250")
    xs, xt, src, noise, t = R.vb_grid(tab, True)
    assert len(xs) == len(R.XS_GRID) * len(R.ERR_SIGMAS) + 4 * 3 * len(R.KL_ERRS) and 150 <= len(xs) <= 260
    z = t == 0
    assert (xs[z] < F(-0.999)).sum() == 2 * 19 and (xs[z] > F(0.999)).sum() == 2 * 19 and (xs[z] == F(0.999)).any() and (xs[z] == F(-0.999)).any()
    term = R.vb_terms_f32(tab, xs[:, None], xt[:, None], src[:, None], t, 0, 1, start_x=True)["term"][:, 0]
    assert (term[z] == -np.log(F(1e-12))).any() and (term[z] < 1.0).any()                     # the clamp, and a saturated tanhf next to ordinary points
    assert set(t[~z]) == {1, 2, 125, 249}


# ------------------------------------------------------------------------------------------------------------ the bounds bite
MISTAKES = {
    "coef1_coef2_swapped": ("posterior", "vb"),
    "t0_switch_from_item0": ("posterior",),
    "abp_read_at_t_minus_1": ("posterior",),
    "eta_dropped_from_sigma": ("posterior",),
    "clamp_before_nonfinite_test": ("posterior",),
    "cdf_min_in_low_branch": ("vb",),
    "threshold_0.99": ("vb",),
    "mask_index_fsz_plus_1": ("vb",),
    "logvar_and_post_logvar_exchanged": ("vb",),
    "mean_over_masked_count": ("vb",),
    "index_minus_1_unwrapped": ("q",),
    "pairs_02_13": ("randn",),
    "u1_plus_one_dropped": ("randn",),
}


@pytest.mark.parametrize("mistake", list(MISTAKES))
def test_a_seeded_mistake_leaves_the_bound(mistake):
    """Applied to the float32 restatement, on the inputs the restatement itself passes on.  LOGVAR and POST_LOGVAR are one row under
    sigma_small: that exchange is caught on the two linear schedules, every other mistake on all three."""
    for name in SCHED:
        if mistake == "logvar_and_post_logvar_exchanged" and SCHED[name]["sigma_small"]:
            continue
        for kind in MISTAKES[mistake]:
            if kind == "posterior":
                worst = _posterior_worst(name, mistake=mistake)
            elif kind == "vb":
                worst = max(_vb_worst(name, mistake=mistake).values())
            elif kind == "q":
                worst = _q_worst(name, mistake=mistake)
            else:
                worst = _randn_worst(mistake)
            assert worst > 1.0, (mistake, name, kind, worst)
