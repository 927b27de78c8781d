"""No GPU: particle steering -- the float64 restatement (tests/particle_restated.py) on hand-worked cases, the Gaussian check of the
restated chain against the exact posterior, and the host logic on the recording stand-in library of test_step_dispatch_cpu.py: the
call sequence of a steered step and of infer_video with particles, every refusal raised before any engine call, the scope restored
behind an exception, the job's options and its run directory."""
import numpy as np
import pytest
import torch

import particle_restated as pr
from test_step_dispatch_cpu import B, T, _FakeLib, _recording
from video_diffusion_amd import _lib, executor, video_sample
from video_diffusion_amd.gaussian_diffusion import measure

NINF = -np.inf


def _one(r, tau, u, final=False, lam=1.0, state=None):
    r = np.asarray(r, np.float64).reshape(1, -1)
    st = state or pr.new_state(1, r.shape[1])
    return pr.particle_weights(st, r, lam, tau, np.asarray(u, np.float64).reshape(1, 2), final), st


# ---------------------------------------------------------------------------------------------------------------- hand-worked cases
def test_restatement_k1():
    out, st = _one([3.5], 1.0, [0.3, 0.9], lam=2.0)
    assert out["ancestors"].tolist() == [0] and out["ess"][0] == 1.0 and st["logw"][0, 0] == 7.0 and st["rprev"][0, 0] == 3.5
    assert out["chosen"].tolist() == [-1] and st["resamples"][0] == 0
    out, _ = _one([1.0], 1.0, [0.3, 0.9], final=True, lam=2.0, state=st)
    assert out["chosen"].tolist() == [0] and st["logw"][0, 0] == 7.0 + 2.0 * (1.0 - 3.5)


def test_restatement_k2_weights_one_and_zero():
    """p = (1, 0): ESS = 1.  Under ess_threshold 0.5 (1 < 1 is false) nothing moves; under 1 both slots take particle 0 for any u."""
    out, st = _one([0.0, NINF], 0.5, [0.7, 0.0])
    assert out["p"][0].tolist() == [1.0, 0.0] and out["ess"][0] == 1.0 and out["ancestors"].tolist() == [0, 1] and st["resamples"][0] == 0
    assert st["logw"][0].tolist() == [0.0, NINF]
    for u in (0.0, 0.5, 1.0 - 2.0 ** -53):
        out, st = _one([0.0, NINF], 1.0, [u, 0.0])
        assert out["ancestors"].tolist() == [0, 0] and st["logw"][0].tolist() == [0.0, 0.0] and st["rprev"][0].tolist() == [0.0, 0.0]
        assert st["resamples"][0] == 1 and st["degenerate"][0] == 0


def test_restatement_k5_u_at_both_ends():
    """p = (.1, .2, .4, .2, .1), c = (.1, .3, .7, .9, 1).  u = 0: thresholds 0, .2, .4, .6, .8 -> (0, 1, 2, 2, 3).  u = 1 - 2^-53: u + i
    rounds to i + 1 for i >= 1 and (u + 4) / 5 to 1, which no c_k exceeds: the last particle -> (1, 2, 2, 3, 4)."""
    r = np.log([0.1, 0.2, 0.4, 0.2, 0.1])
    out, st = _one(r, 1.0, [0.0, 0.0])
    assert np.allclose(out["c"][0], [0.1, 0.3, 0.7, 0.9, 1.0], atol=1e-15) and out["c"][0, -1] == 1.0
    assert abs(out["ess"][0] - 1 / 0.26) < 1e-12 and out["ancestors"].tolist() == [0, 1, 2, 2, 3]
    assert np.allclose(st["rprev"][0], r[[0, 1, 2, 2, 3]], rtol=0, atol=0) and not st["logw"].any()
    out, _ = _one(r, 1.0, [1.0 - 2.0 ** -53, 0.0])
    assert out["ancestors"].tolist() == [1, 2, 2, 3, 4]
    out, st = _one(r, 0.5, [0.0, 0.0])                              # ESS 3.85 >= 2.5: nothing moves, the weights stay
    assert out["ancestors"].tolist() == [0, 1, 2, 3, 4] and np.array_equal(st["logw"][0], r) and st["resamples"][0] == 0


def test_restatement_bit_equal_weights_all_inf_and_some_inf():
    out, st = _one([2.5, 2.5, 2.5], 1.0, [0.9, 0.9])               # ESS = 3 is not below 3 either; the rule is the bit-equality
    assert out["ancestors"].tolist() == [0, 1, 2] and st["resamples"][0] == 0 and st["logw"][0].tolist() == [2.5, 2.5, 2.5]
    st = pr.new_state(1, 3)
    st["logw"][0] = [1.0, 1.0, 1.0]
    st["rprev"][0] = [0.5, 0.25, 0.125]
    out, _ = _one([1.5, 1.25, 1.125], 1.0, [0.9, 0.9], state=st)    # one increment of 1 on equal weights: still bit-equal
    assert out["ancestors"].tolist() == [0, 1, 2] and st["resamples"][0] == 0
    out, st = _one([NINF, NINF, NINF], 1.0, [0.2, 0.2])
    assert out["ancestors"].tolist() == [0, 1, 2] and st["degenerate"][0] == 1 and st["resamples"][0] == 0 and out["ess"][0] == 0
    assert np.isneginf(st["logw"]).all()
    out, _ = _one([0.0, 0.0, 0.0], 1.0, [0.2, 0.2], state=st)       # a dead group stays dead: -inf absorbs
    assert st["degenerate"][0] == 2 and np.isneginf(st["logw"]).all()
    out, st = _one([NINF, 0.0, NINF, 0.0], 1.0, [0.5, 0.0])         # p = (0, .5, 0, .5), thresholds .125, .375, .625, .875
    assert out["c"][0].tolist() == [0.0, 0.5, 0.5, 1.0] and out["ess"][0] == 2.0 and out["ancestors"].tolist() == [1, 1, 3, 3]
    assert not st["logw"].any() and not st["rprev"].any()


def test_restatement_final_pick_skips_a_particle_of_weight_zero():
    """t == 0 with p_0 = 0 and u2 = 0: c_0 = 0 is not above 0, particle 1 is picked; nothing is gathered, the weights stay."""
    out, st = _one([NINF, 0.0, 0.0], 1.0, [0.0, 0.0], final=True)
    assert out["chosen"].tolist() == [1] and out["ancestors"].tolist() == [0, 1, 2] and st["resamples"][0] == 0
    assert st["logw"][0].tolist() == [NINF, 0.0, 0.0]
    assert _one([NINF, 0.0, 0.0], 1.0, [0.0, 0.5], final=True)[0]["chosen"].tolist() == [2]
    assert _one([0.0, 0.0, NINF], 1.0, [0.0, 1.0 - 2.0 ** -53], final=True)[0]["chosen"].tolist() == [1]     # ... nor a trailing one
    two, st = pr.particle_weights(pr.new_state(2, 2), np.array([[0.0, 5.0], [5.0, 0.0]]), 1.0, 1.0, np.array([[0.5, 0.5], [0.5, 0.5]]),
                                  np.array([True, False])), None
    assert two["chosen"].tolist() == [1, -1] and two["ancestors"].tolist() == [0, 1, 2, 2]      # groups at different t; batch indices


def test_restatement_helpers():
    part = np.array([[1.0, 2.0, 3.0], [0.5, 0.0, 0.25]])
    assert pr.reward_from_partials(part, 0.5).tolist() == [-12.0, -1.5]
    x = np.arange(12.0).reshape(6, 2)
    assert np.array_equal(pr.gather(x, [1, 0, 2, 4, 5, 3]), x[[1, 0, 2, 4, 5, 3]])
    v = torch.rand(2, 3, 3, 4, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    for s, gray in ((2, False), (1, True), (4, True)):
        assert np.allclose(pr.measure(v.numpy(), s, gray), measure(v, s, gray).numpy(), rtol=0, atol=1e-15)
    y = pr.measure(v.numpy(), 2, False)
    lat = np.array([[1, 0, 1], [0, 0, 0]])
    r = pr.measurement_reward(np.zeros_like(v.numpy()), y, 2, False, lat, 2.0)
    assert np.isclose(r[0], -(y[0, 0] ** 2).sum() / 8 - (y[0, 2] ** 2).sum() / 8) and r[1] == 0
    u = pr.philox_uniforms(3, 1000, 4)
    assert u.shape == (4, 2) and ((u >= 0) & (u < 1)).all() and len(np.unique(u)) == 8
    assert np.array_equal(pr.philox_uniforms(3, 1001, 3), u[1:])                               # group g reads block offset + g


# ---------------------------------------------------------------------------------------------------------------- the Gaussian check
def _fit(x, y):
    """Slope of x on y, its residual variance, and one standard error of each."""
    n = len(y)
    slope = np.cov(x, y)[0, 1] / np.var(y, ddof=1)
    res = (x - x.mean()) - slope * (y - y.mean())
    rv = res.var(ddof=2)
    return slope, rv, np.sqrt(rv / (n * np.var(y))), rv * np.sqrt(2.0 / n)


def test_gaussian_chain_samples_the_posterior():
    """One-dimensional data x ~ N(0, 0.5^2) with its exact denoiser, y = x + 0.5 n, p_sample on 50 of 1000 linear steps, lam = 1,
    ess_threshold 0.5, N = 20000 measurements, on the restated chain alone.  The chain has a prior variance of its own (the K = 1 run:
    v = 0.266 here, a discretisation effect of p_sample with the fixed large variance), so the reference is the posterior under THAT
    prior: slope v / (v + sw^2) and residual variance v sw^2 / (v + sw^2) of the chosen sample on the measurement.  K = 64 is held to it
    within four Monte-Carlo standard errors -- of the fit and of v, computed here -- plus a K-bias allowance: the gap between K = 64 and
    K = 256 runs of this restatement at N = 20000, recorded once: slopes 0.5151, 0.5094, 0.5141 (K = 64) against 0.5135, 0.5215
    (K = 256), residual variances 0.1295, 0.1314, 0.1286 against 0.1293, 0.1284: 0.005 and 0.001 between the means.  Control: K = 4 is
    further from the reference than K = 64 (0.42 against 0.515 for a reference of 0.515)."""
    N, sw2 = 20000, 0.25
    rng = np.random.default_rng(0)
    y = 0.5 * rng.standard_normal(N) + 0.5 * rng.standard_normal(N)
    x1, _ = pr.gaussian_chain(y, 1, rng)
    v = x1.var(ddof=1)
    se_v = v * np.sqrt(2.0 / N)
    slope1 = _fit(x1, y)[0]
    assert abs(slope1) < 4 * np.sqrt(v / (N * np.var(y)))           # the plain chain does not see y
    ref_slope, ref_var = v / (v + sw2), v * sw2 / (v + sw2)
    d_slope, d_var = sw2 / (v + sw2) ** 2 * se_v, (sw2 / (v + sw2)) ** 2 * se_v          # the reference's own standard errors, through v
    got = {}
    for K in (4, 64):
        x, st = pr.gaussian_chain(y, K, np.random.default_rng(K))
        got[K] = _fit(x, y)
        assert st["resamples"].sum() > N // 10 and st["degenerate"].sum() == 0
    slope, rv, se_s, se_r = got[64]
    print(f"v = {v:.4f}; reference slope {ref_slope:.4f}, residual variance {ref_var:.4f}; K = 64: {slope:.4f} +- {se_s:.4f}, {rv:.4f} +- {se_r:.4f}; "
          f"K = 4: {got[4][0]:.4f}, {got[4][1]:.4f}")
    assert abs(slope - ref_slope) <= 4 * np.hypot(se_s, d_slope) + 0.005
    assert abs(rv - ref_var) <= 4 * np.hypot(se_r, d_var) + 0.001
    assert abs(got[4][0] - ref_slope) > abs(slope - ref_slope) + 4 * se_s and abs(got[4][1] - ref_var) > abs(rv - ref_var)


# ---------------------------------------------------------------------------------------------------------------- host logic
class _Lib(_FakeLib):
    """The recording stand-in, whose vd_particle_state also fills its outputs (chosen = 0: infer_video indexes with it)."""

    def __getattr__(self, name):
        call = super().__getattr__(name)
        if name != "vd_particle_state":
            return call

        def state(*args):
            for a in args:
                if torch.is_tensor(a):
                    a.zero_()
            return call(*args)
        return state


def _standin(monkeypatch, rec, full=False):
    """Inside _recording: its stand-in library becomes a _Lib (nothing of this test outlives the recording's own patches)."""
    fake = _lib.lib()
    assert isinstance(fake, _FakeLib) and fake.rec is rec and fake.full == full
    fake.__class__ = _Lib
    return fake


def _reward(x0, t):
    return torch.zeros(x0.shape[0])                                  # (the stand-in's step leaves its outputs uninitialised: nothing to read)


def test_call_sequence_of_a_steered_step(monkeypatch):
    """reward_fn: the scope sets the engine's state, the first step resets the weights and draws its uniforms (one torch.rand) in front
    of the plain step -- whose own noise draw and entry are the plain step's -- then vd_particle_apply and vd_particle_state; the second
    step does not reset; a step at t == 0 returns 'chosen' and the next one resets again; the scope's exit clears the state."""
    with _recording(monkeypatch, full=False) as (rec, model, diff, (x, t, noise, prev, state)):
        _standin(monkeypatch, rec)
        with diff.steering_scope(model, _reward, particles=2):
            out = diff.p_sample(model, x, t, model_kwargs={})
            assert {"sample", "pred_xstart", "ancestors", "ess", "log_weights"} <= set(out) and "chosen" not in out
            assert out["ancestors"].shape == (B,) and out["ess"].shape == (B // 2,) and out["log_weights"].dtype == torch.float64
            diff.ddim_sample(model, x, t, model_kwargs={}, eta=1.0)
            assert "chosen" in diff.dpmpp_2m_sde_sample(model, x, t * 0, model_kwargs={})
            diff.p_sample(model, x, t, model_kwargs={})
        assert rec.events == [
            "vd_set_particles",
            "vd_particle_reset", "rand", "randn_like", "vd_p_sample@1", "vd_particle_apply@1", "vd_particle_state",
            "rand", "randn_like", "vd_ddim_sample@1", "vd_particle_apply@1", "vd_particle_state",
            "rand", "randn_like", "vd_dpmpp_2m_sde_sample@0", "vd_particle_apply@0", "vd_particle_state",
            "vd_particle_reset", "rand", "randn_like", "vd_p_sample@1", "vd_particle_apply@1", "vd_particle_state",
            "vd_set_particles"]
    # the built-in reward: no callback and no apply -- the step's own launches do it; the uniforms go to the engine in front of the step,
    # as a tensor, or as the step's Philox pair where the sampler draws from the engine's stream
    with _recording(monkeypatch, full=False) as (rec, model, diff, (x, t, noise, prev, state)):
        _standin(monkeypatch, rec)
        y = torch.zeros(B, T, 3, 1, 1)
        with diff.steering_scope(model, particles=2, measurement=y, sr_scale=2, sigma_y=0.5):
            diff.p_sample(model, x, t, model_kwargs={})
            diff._dpmpp_2m_sde(model, x, t, None, True, None, {}, philox=(7, 11))
        assert rec.events == ["vd_set_particles", "vd_particle_reset", "rand", "vd_particle_draws", "randn_like", "vd_p_sample@1", "vd_particle_state",
                              "vd_particle_draws+11", "vd_dpmpp_2m_sde_sample@1+11", "vd_particle_state", "vd_set_particles"]
    # particles=1 and scale=0 are the plain step: the scope clears the engine's state and the step adds no call
    for kwargs in (dict(particles=1), dict(particles=2, scale=0.0)):
        with _recording(monkeypatch, full=False) as (rec, model, diff, (x, t, noise, prev, state)):
            _standin(monkeypatch, rec)
            with diff.steering_scope(model, _reward, **kwargs):
                assert "ancestors" not in diff.p_sample(model, x, t, model_kwargs={})
            assert rec.events == ["vd_set_particles", "randn_like", "vd_p_sample@1", "vd_set_particles"]


def test_scope_arguments_and_nesting(monkeypatch):
    with _recording(monkeypatch, full=True) as (rec, model, diff, (x, t, noise, prev, state)):
        _standin(monkeypatch, rec, full=True)
        y = torch.zeros(B, T, 1, 1, 1)
        with diff.steering_scope(model, _reward, particles=2, scale=3.0, ess_threshold=0.25):
            with diff.steering_scope(model, particles=4, measurement=y, sr_scale=2, gray=True, sigma_y=0.5):
                pass
            with pytest.raises(RuntimeError, match="boom"):
                with diff.steering_scope(model, _reward, particles=1):
                    raise RuntimeError("boom")
            assert getattr(model, "_steering")["K"] == 2
        assert getattr(model, "_steering") is None
        assert rec.events == ["vd_set_particles(17 2 3.0 0.25 N 1 0 0.0)", "vd_set_particles(17 4 1.0 0.5 p 2 1 0.5)",
                              "vd_set_particles(17 2 3.0 0.25 N 1 0 0.0)", "vd_set_particles(17 0 0.0 0.0 N 1 0 0.0)",
                              "vd_set_particles(17 2 3.0 0.25 N 1 0 0.0)", "vd_set_particles(17 0 0.0 0.0 N 1 0 0.0)"]


def test_every_refusal_is_raised_before_any_engine_call(monkeypatch):
    with _recording(monkeypatch, full=False) as (rec, model, diff, (x, t, noise, prev, state)):
        _standin(monkeypatch, rec)
        y3, y1 = torch.zeros(B, T, 3, 1, 1), torch.zeros(B, T, 1, 1, 1)
        src, mask = torch.zeros(B, T, 3, 2, 2), torch.ones(B, T, 2, 2)
        scope = lambda **k: diff.steering_scope(model, **({"reward_fn": _reward, "particles": 2} | k))      # noqa: E731
        steps = ((lambda: diff.ddim_sample(model, x, t, model_kwargs={}), NotImplementedError, "ddim_sample at eta = 0 inside steering_scope"),
                 (lambda: diff.dpmpp_2m_sample(model, x, t, model_kwargs={}), NotImplementedError, "dpmpp_2m_sample inside steering_scope"),
                 (lambda: diff.unipc_sample(model, x, t, model_kwargs={}), NotImplementedError, "unipc_sample inside steering_scope"),
                 (lambda: diff.ddim_reverse_sample(model, x, t, model_kwargs={}), NotImplementedError, "ddim_reverse_sample inside steering_scope"),
                 (lambda: diff.p_sample(model, x, t, model_kwargs={}, use_gradient_method=True), NotImplementedError, "use_gradient_method inside"),
                 (lambda: diff.p_sample(model, x, t, model_kwargs={}, return_attn_weights=True), NotImplementedError, "return_attn_weights inside"),
                 (lambda: diff.p_sample(model, x[:3], t[:3], model_kwargs={}), ValueError, "no multiple of particles=2"))
        for call, exc, name in steps:
            with scope():
                del rec.events[:]
                with pytest.raises(exc, match=name):
                    call()
                assert rec.events == [], name
        with scope(reward_fn=None, measurement=y3, sr_scale=2, sigma_y=1.0):
            del rec.events[:]
            with pytest.raises(NotImplementedError, match="denoised_fn together with the built-in reward"):
                diff.p_sample(model, x, t, model_kwargs={}, denoised_fn=lambda v: v)
            with pytest.raises(ValueError, match="measurement .* against a step"):
                diff.p_sample(model, torch.zeros(B, T, 3, 4, 4), t, model_kwargs={})
            assert rec.events == []
        others = (("known_region", lambda: diff.known_region_scope(model, src, mask)), ("measurement", lambda: diff.measurement_scope(model, y3, scale=2)),
                  ("dps", lambda: diff.dps_scope(model, y1, 2, True, zeta=0.1)),
                  ("loss_guidance", lambda: diff.loss_guidance_scope(model, lambda x0, tt: x0.sum(), scale=1.0)))
        for name, other in others:
            for outer, inner in ((other, scope), (scope, other)):
                with outer():
                    with inner():
                        del rec.events[:]
                        with pytest.raises(NotImplementedError, match=f"{name}_scope together with steering_scope"):
                            diff.p_sample(model, x, t, model_kwargs={})
                        assert rec.events == [], name
        del rec.events[:]
        for kwargs, name in ((dict(reward_fn=None, measurement=y3, sr_scale=2, sigma_y=0.0), "sigma_y"), (dict(reward_fn=None, measurement=y3, sr_scale=2), "sigma_y"),
                             (dict(ess_threshold=1.01), "ess_threshold"), (dict(ess_threshold=float("nan")), "ess_threshold"), (dict(measurement=y3, sigma_y=1.0), "exactly one"),
                             (dict(reward_fn=None), "exactly one"), (dict(scale=-1.0), "scale"), (dict(particles=0), "particles"), (dict(particles=257), "particles"),
                             (dict(particles=2.0), "particles"), (dict(reward_fn=3), "callable"), (dict(uniforms=0.5), "uniforms"),
                             (dict(reward_fn=None, measurement=y3, sr_scale=3, sigma_y=1.0), "scale")):
            with pytest.raises(ValueError, match=name):
                scope(**kwargs)
        # a learned variance: the step's own refusal
        from video_diffusion_amd.gaussian_diffusion import ModelVarType
        diff.model_var_type = ModelVarType.LEARNED
        with scope():
            del rec.events[:]
            with pytest.raises(AssertionError, match="learned variance"):
                diff.p_sample(model, x, t, model_kwargs={})
            assert rec.events == []
        # the caller's reward: NaN and +inf are refused behind the step, -inf is served
        diff.model_var_type = ModelVarType.FIXED_LARGE
        for bad in (float("nan"), float("inf")):
            with pytest.raises(ValueError, match="NaN or \\+inf"):
                with scope(reward_fn=lambda x0, tt: torch.full((B,), bad)):
                    diff.p_sample(model, x, t, model_kwargs={})
        with scope(reward_fn=lambda x0, tt: torch.tensor([0.0, -np.inf] * (B // 2))):
            diff.p_sample(model, x, t, model_kwargs={})
        with pytest.raises(ValueError, match=r"must return a \(4,\) tensor"):
            with scope(reward_fn=lambda x0, tt: torch.zeros(B, 2)):
                diff.p_sample(model, x, t, model_kwargs={})
        assert getattr(model, "_steering") is None


class _Wex(executor.WindowExecutor):
    def __init__(self, model, diffusion, prefix_cache=False, suffix_skip=False):      # (no stream: the refusals come before it is used)
        self.model, self.diffusion, self.prefix_cache, self.suffix_skip = model, diffusion, prefix_cache, suffix_skip


def test_window_executor_refusals(monkeypatch):
    with _recording(monkeypatch, full=False) as (rec, model, diff, (x, t, noise, prev, state)):
        _standin(monkeypatch, rec)
        y = torch.zeros(B, T, 3, 1, 1)
        pk = dict(particles=2, particle_measurement=y, particle_sr_scale=2, sigma_y=1.0)
        cases = ((_Wex(model, diff), dict(particles=2, reward_fn=_reward), NotImplementedError, "reward_fn is not served: a Python callback"),
                 (_Wex(model, diff, prefix_cache=True), pk, NotImplementedError, "prefix_cache together with particles"),
                 (_Wex(model, diff, suffix_skip=True), pk, NotImplementedError, "suffix_skip together with particles"),
                 (_Wex(model, diff), dict(pk, known_src=x, known_mask=torch.ones(B, T, 2, 2)), NotImplementedError, "a known region together with particles"),
                 (_Wex(model, diff), dict(pk, measurement=y, sr_scale=2), NotImplementedError, "a measurement together with particles"),
                 (_Wex(model, diff), dict(pk, sampler="ddim"), NotImplementedError, "sampler='ddim' at eta = 0"),
                 (_Wex(model, diff), dict(pk, sampler="dpmpp_2m"), NotImplementedError, "sampler='dpmpp_2m' together with particles"),
                 (_Wex(model, diff), dict(pk, sampler="unipc"), NotImplementedError, "sampler='unipc'"),
                 (_Wex(model, diff), dict(pk, sampler="ddim_reverse"), NotImplementedError, "sampler='ddim_reverse'"),
                 (_Wex(model, diff), dict(pk, particles=3), ValueError, "no multiple of particles=3"),
                 (_Wex(model, diff), dict(pk, sigma_y=0.0), ValueError, "sigma_y"), (_Wex(model, diff), dict(pk, sigma_y=None), ValueError, "sigma_y"),
                 (_Wex(model, diff), dict(pk, ess_threshold=2.0), ValueError, "ess_threshold"),
                 (_Wex(model, diff), dict(particles=2), ValueError, "needs particle_measurement"),
                 (_Wex(model, diff), dict(pk, particle_measurement=torch.zeros(B, T, 3, 2, 2)), ValueError, "y must be"))
        for wex, kwargs, exc, name in cases:
            with pytest.raises(exc, match=name):
                wex.begin(x, {}, **kwargs)
        with pytest.raises(NotImplementedError, match="reward_fn is not served"):
            with diff.steering_scope(model, _reward, particles=2):
                del rec.events[:]
                _Wex(model, diff).begin(x, {})
        assert rec.events == ["vd_set_particles"]                    # (the scope's exit; no refusal touched the engine)
        with pytest.raises(RuntimeError, match="has no particles"):
            _Wex(model, diff).particle_state()


def test_infer_video_call_sequence_and_refusals(monkeypatch):
    """2 videos, K = 2, 'autoreg' with two windows on a 2-step schedule: every window runs inside its own scope (set, reset, the steps with
    apply and state behind each, clear), the batch the engine sees is B K items, and the return has the batch's shape."""
    with _recording(monkeypatch, respacing="ddim2", full=False) as (rec, model, diff, _):
        _standin(monkeypatch, rec)
        batch = torch.empty(2, 5, 3, 2, 2).uniform_(-1, 1, generator=torch.Generator().manual_seed(3))      # (not one of the recorded draws)
        seen = []

        def reward(x0, t):
            seen.append(tuple(x0.shape))
            return torch.zeros(x0.shape[0])                          # (the stand-in's tensors are uninitialised)

        out, _ = video_sample.infer_video("autoreg", model, diff, batch, 3, 1, 2, particles=2, reward_fn=reward, sampler="ddim", eta=1.0)
        assert out.shape == tuple(batch.shape) and np.array_equal(out[:, :1], batch[:, :1].numpy())
        step = lambda tv: ["rand", "randn_like", f"vd_ddim_sample@{tv}", f"vd_particle_apply@{tv}", "vd_particle_state"]      # noqa: E731
        window = ["vd_set_particles", "vd_particle_reset", *step(1), *step(0), "vd_set_particles", "check_device_errors"]
        assert rec.events == window + window and seen == [(4, 3, 3, 2, 2)] * 4
        # the built-in reward under dpmpp_2m_sde: the window's seed (one randint), the uniforms on the step's own Philox range
        del rec.events[:]
        y = measure(batch, 2, False)
        out, _ = video_sample.infer_video("autoreg", model, diff, batch, 3, 1, 2, particles=2, particle_measurement=y, sr_scale=2, sigma_y=0.5,
                                          sampler="dpmpp_2m_sde")
        n = 4 * 3 * 3 * 2 * 2
        window = ["randint", "vd_set_particles", "vd_particle_reset", "vd_particle_draws", "vd_dpmpp_2m_sde_sample@1", "vd_particle_state",
                  f"vd_particle_draws+{n}", f"vd_dpmpp_2m_sde_sample@0+{n}", "vd_particle_state", "vd_set_particles", "check_device_errors"]
        assert rec.events == window + window and out.shape == tuple(batch.shape)
        # particles=1: the plain loop, no particle entry
        del rec.events[:]
        video_sample.infer_video("autoreg", model, diff, batch, 3, 1, 2, particles=1)
        assert not [e for e in rec.events if "particle" in e]
        del rec.events[:]
        pk = dict(particles=2, particle_measurement=y, sr_scale=2, sigma_y=0.5)
        for kwargs, exc, name in ((dict(pk, use_gradient_method=True), NotImplementedError, "use_gradient_method together with particles"),
                                  (dict(pk, known_mask=torch.ones(5, 2, 2)), NotImplementedError, "known_mask together with particles"),
                                  (dict(pk, measurement=y), NotImplementedError, "a measurement together with particles"),
                                  (dict(pk, executor="graph", prefix_cache=True), NotImplementedError, "prefix_cache together with particles"),
                                  (dict(pk, executor="graph", suffix_skip=True), NotImplementedError, "suffix_skip together with particles"),
                                  (dict(pk, save_all_timesteps=True), NotImplementedError, "save_all_timesteps together with particles"),
                                  (dict(pk, sampler="ddim"), NotImplementedError, "sampler='ddim' at eta = 0"),
                                  (dict(pk, sampler="dpmpp_2m"), NotImplementedError, "sampler='dpmpp_2m' together with particles"),
                                  (dict(pk, sampler="unipc"), NotImplementedError, "sampler='unipc'"),
                                  (dict(particles=2, reward_fn=reward, executor="graph"), NotImplementedError, "executor='graph' together with a reward_fn"),
                                  (dict(particles=2, reward_fn=reward, loss_fn=reward, loss_scale=1.0), NotImplementedError, "loss_fn / cotangent_fn together with particles"),
                                  (dict(particles=2), ValueError, "exactly one"), (dict(pk, reward_fn=reward), ValueError, "exactly one"),
                                  (dict(pk, sigma_y=None), ValueError, "sigma_y"), (dict(pk, sigma_y=-1.0), ValueError, "sigma_y"),
                                  (dict(pk, ess_threshold=-0.5), ValueError, "ess_threshold"), (dict(pk, particles=300), ValueError, "particles"),
                                  (dict(pk, particle_measurement=y[:, :, :1]), ValueError, "y must be")):
            with pytest.raises(exc, match=name):
                video_sample.infer_video("autoreg", model, diff, batch, 3, 1, 2, **kwargs)
        assert rec.events == []


# ---------------------------------------------------------------------------------------------------------------- the job's options
def _args(*argv):
    ap = video_sample.build_parser()
    return ap, ap.parse_args(list(argv))


def test_cli_options_and_run_directory(capsys, tmp_path, monkeypatch):
    ap, a = _args()
    assert (a.particles, a.reward, a.reward_scale, a.measurement_sigma, a.ess_threshold) == (1, None, 1.0, None, 0.5)
    assert video_sample.check_particle_arguments(ap, a) is a and video_sample.run_postfix(a) == "" and video_sample._particle_options(a) == {}
    ap, a = _args("--particles", "8", "--measurement", "y.npy", "--sr_scale", "4", "--measurement_sigma", "0.1", "--ess_threshold", "0.3")
    assert video_sample.check_particle_arguments(ap, a) is a and video_sample.run_postfix(a) == "_sr4_smc8"
    assert video_sample._particle_options(a) == dict(particles=8, reward_fn=None, reward_scale=1.0, ess_threshold=0.3)
    np.save(tmp_path / "y.npy", np.zeros((3, 4, 1, 2, 2), np.float32))
    a.measurement, a.gray, a._batch_ids = str(tmp_path / "y.npy"), True, [2, 0]
    kw = video_sample._measurement_options(a, torch.zeros(2, 4, 3, 8, 8))
    assert set(kw) == {"particle_measurement", "sr_scale", "gray", "sigma_y"} and kw["sigma_y"] == 0.1 and kw["particle_measurement"].shape == (2, 4, 1, 2, 2)
    a.measurement_sigma = None                                       # without the sigma: the exact projection, as before
    assert set(video_sample._measurement_options(a, torch.zeros(2, 4, 3, 8, 8))) == {"measurement", "sr_scale", "gray"}
    (tmp_path / "my_rewards.py").write_text("def bright(x0, t):\n    return x0.mean(dim=(1, 2, 3, 4))\n")
    monkeypatch.syspath_prepend(str(tmp_path))
    ap, a = _args("--particles", "4", "--reward", "my_rewards:bright", "--reward_scale", "2.5", "--sampler", "ddim")
    opts = video_sample._particle_options(video_sample.check_particle_arguments(ap, a))
    assert opts["particles"] == 4 and opts["reward_scale"] == 2.5 and opts["reward_fn"](torch.ones(2, 1, 3, 2, 2), None).tolist() == [1.0, 1.0]
    assert video_sample.run_postfix(a) == "_ddim_smc4"
    with pytest.raises(ValueError, match="--reward 'nothing:here'"):
        video_sample.import_function("nothing:here", "--reward")
    for argv, name in ((("--particles", "4", "--measurement", "y.npy", "--measurement_sigma", "0.1", "--dps_zeta", "0.5"), "--dps_zeta and --measurement_sigma"),
                       (("--particles", "4"), "--particles needs a reward"), (("--reward", "m:f"), "need --particles"),
                       (("--measurement", "y.npy", "--measurement_sigma", "0.1"), "need --particles"),
                       (("--particles", "4", "--measurement_sigma", "0.1"), "--measurement_sigma needs --measurement"),
                       (("--particles", "4", "--reward", "m:f", "--measurement", "y.npy", "--measurement_sigma", "0.1"), "two rewards"),
                       (("--particles", "0", "--reward", "m:f"), "at least 1")):
        ap, a = _args(*argv)
        with pytest.raises(SystemExit):
            video_sample.check_particle_arguments(ap, a)
        assert name in capsys.readouterr().err, argv
