"""GPU: particle steering (this project's extension, Feynman-Kac steering) -- the weights and gather kernels against the float64
restatement (tests/particle_restated.py), the built-in measurement reward against the restatement fed with the engine's own x_0
prediction, the identities with the plain step bit for bit, eager steps against the window graph, the configurations the gradient
scopes refuse (40 frames, predict_xstart), infer_video, and every refusal by name.  Nothing here is tuned on the code under test but
ESS_BAR, which is 4 x what the first run showed for the device's fp64 exp (see there)."""
import ctypes

import numpy as np
import pytest
import torch

import particle_restated as pr
from dps_restated import seed_bound
from test_gpu_long_window import engine, kwargs_of, rand_window, tiny_cfg
from video_diffusion_amd import _lib
from video_diffusion_amd.executor import WindowExecutor
from video_diffusion_amd.gaussian_diffusion import measure

pytestmark = pytest.mark.gpu

# The device's fp64 exp against numpy's is the only operation of the weights kernel that is not a single IEEE rounding (the kernel is
# compiled without contraction): log-weights, rprev, ancestors, chosen and the counters are compared exactly, the effective sample size
# relatively.  Seen on the first run over every case below: 4.5e-16 (two ulp); the bar is 4 x that.
ESS_BAR = 4 * 4.5e-16
MARGIN = 1e-9


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda().contiguous()


def _weights_op(G, K, lam, tau, t, logw, rprev, r=None, u=None, part=None, sigma=0.0, seed=0, offset=0):
    """vd_op_particle_weights on copies of the state -> dict of numpy arrays."""
    B = G * K
    d = dict(logw=_dev(logw.reshape(-1), torch.float64), rprev=_dev(rprev.reshape(-1), torch.float64),
             ancestors=torch.full((B,), -7, dtype=torch.int32, device="cuda"), chosen=torch.full((G,), -7, dtype=torch.int32, device="cuda"),
             ess=torch.full((G,), -7.0, dtype=torch.float64, device="cuda"), counters=torch.zeros(G, 2, dtype=torch.int64, device="cuda"))
    r_d = None if r is None else _dev(r.reshape(-1), torch.float64)
    p_d = None if part is None else _dev(part.reshape(B, -1), torch.float64)
    u_d = None if u is None else _dev(u, torch.float64)
    t_d = _dev(np.repeat(np.asarray(t, np.int64), K), torch.int64)
    _lib.check(_lib.lib().vd_op_particle_weights(G, K, float(lam), float(tau), _lib.ptr(r_d), _lib.ptr(p_d), 0 if part is None else part.shape[-1],
                                                 float(sigma), _lib.ptr(t_d), _lib.ptr(u_d), seed, offset, *(_lib.ptr(d[k]) for k in
                                                 ("logw", "rprev", "ancestors", "chosen", "ess", "counters")), _lib.current_stream()))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in d.items()}


def _margin(out, u, final):
    """The least distance between a threshold that is used ((u + i) / K of a group that resamples, u2 of a group at t == 0) and any c_k."""
    c, K = out["c"], out["c"].shape[1]
    worst = np.inf
    for g in range(c.shape[0]):
        thr = (u[g, 0] + np.arange(K)) / K if out["resampled"][g] else (u[g, 1:2] if final[g] and out["ess"][g] > 0 else np.zeros(0))
        if thr.size:
            worst = min(worst, float(np.abs(c[g][None, :] - thr[:, None]).min()))
    return worst


def _scenarios(G, K, rng):
    """(name, r, logw0, rprev0, final, tau): rewards spread over 1e-3, 1 and 1e4, -inf on some particles, on a whole group, a group of
    bit-equal log-weights; steps in the middle of a chain (a state that is not 0) and at t == 0."""
    out = []
    for spread in (1e-3, 1.0, 1e4):
        for tau, final in ((0.5, False), (1.0, False), (1.0, True)):
            out.append((f"spread{spread:g}-tau{tau}-final{int(final)}", spread * rng.standard_normal((G, K)), 0.1 * rng.standard_normal((G, K)),
                        0.5 * spread * rng.standard_normal((G, K)), np.full(G, final), tau))
    r = rng.standard_normal((G, K))
    r[:, ::3] = -np.inf                                             # (K <= 3: particle 0 alone; K = 1: the whole group)
    out.append(("neg-inf-some", r, np.zeros((G, K)), np.zeros((G, K)), np.zeros(G, bool), 1.0))
    out.append(("neg-inf-some-final", r.copy(), np.zeros((G, K)), np.zeros((G, K)), np.ones(G, bool), 1.0))
    r = rng.standard_normal((G, K))
    r[G - 1] = -np.inf
    out.append(("neg-inf-group", r, np.zeros((G, K)), np.zeros((G, K)), np.zeros(G, bool), 1.0))
    r, lw, rp = rng.standard_normal((G, K)), 0.3 * rng.standard_normal((G, K)), rng.standard_normal((G, K))
    r[0], lw[0], rp[0] = 2.5, -0.75, 1.25                           # group 0: one increment on equal log-weights
    out.append(("equal-group", r, lw, rp, np.zeros(G, bool), 1.0))
    final = np.zeros(G, bool)
    final[0] = True                                                 # groups at different t in one launch
    out.append(("mixed-final", 3.0 * rng.standard_normal((G, K)), np.zeros((G, K)), np.zeros((G, K)), final, 1.0))
    return out


@pytest.mark.parametrize("K", [1, 2, 5, 8, 256])
@pytest.mark.parametrize("G", [1, 3])
def test_weights_kernel_against_restatement(G, K):
    rng = np.random.default_rng(100 * G + K)
    lam, seen = 0.7, 0.0
    for name, r, lw0, rp0, final, tau in _scenarios(G, K, rng):
        for _ in range(100):                                        # inputs whose thresholds keep clear of every c_k: a 1-ulp exp cannot move an ancestor
            u = rng.random((G, 2))
            st = dict(pr.new_state(G, K), logw=lw0.copy(), rprev=rp0.copy())
            want = pr.particle_weights(st, r, lam, tau, u, final)
            if _margin(want, u, final) >= MARGIN:
                break
        assert _margin(want, u, final) >= MARGIN, name
        got = _weights_op(G, K, lam, tau, np.where(final, 0, 7), lw0, rp0, r=r, u=u)
        assert np.array_equal(got["ancestors"], want["ancestors"]), name
        assert np.array_equal(got["chosen"], want["chosen"]), name
        assert np.array_equal(got["logw"].reshape(G, K), st["logw"]) and np.array_equal(got["rprev"].reshape(G, K), st["rprev"]), name
        assert np.array_equal(got["counters"][:, 0], st["resamples"]) and np.array_equal(got["counters"][:, 1], st["degenerate"]), name
        rel = np.abs(got["ess"] - want["ess"]) / np.maximum(want["ess"], 1e-300)
        seen = max(seen, float(rel.max()))
        assert (rel <= ESS_BAR).all(), (name, rel)
        if name.startswith("equal"):
            assert not want["resampled"][0] and np.array_equal(got["ancestors"][:K], np.arange(K))
        if name == "neg-inf-group":
            assert st["degenerate"][G - 1] == 1 and got["ess"][G - 1] == 0
        if name == "spread10000-tau1.0-final0" and K > 1:
            assert want["resampled"].all()
    print(f"G={G} K={K}: max relative ESS difference seen {seen:.3e}")


def test_weights_kernel_partials_and_philox():
    """The reward folded from the residual pass's partials (index order, r = -(sum / (2 sigma^2))), and the uniforms drawn from the
    engine's Philox stream: both against the restatement, exactly."""
    G, K, nblk, sigma = 3, 5, 7, 0.8
    rng = np.random.default_rng(5)
    part = rng.random((G, K, nblk)) * 3.0
    r = pr.reward_from_partials(part.reshape(G * K, nblk), sigma).reshape(G, K)
    zeros = np.zeros((G, K))
    for final in (False, True):
        for seed in range(40):
            u = pr.philox_uniforms(seed, 12345, G)
            st = pr.new_state(G, K)
            want = pr.particle_weights(st, r, 1.0, 1.0, u, np.full(G, final))
            if _margin(want, u, np.full(G, final)) >= MARGIN:
                break
        assert _margin(want, u, np.full(G, final)) >= MARGIN and ((u >= 0) & (u < 1)).all()
        got = _weights_op(G, K, 1.0, 1.0, np.full(G, 0 if final else 3), zeros, zeros, part=part, sigma=sigma, seed=seed, offset=12345)
        assert np.array_equal(got["ancestors"], want["ancestors"]) and np.array_equal(got["chosen"], want["chosen"])
        assert np.array_equal(got["rprev"].reshape(G, K), st["rprev"]) and np.array_equal(got["logw"].reshape(G, K), st["logw"])
        assert want["resampled"].all() != final


# ------------------------------------------------------------------------------------------------------------ the gather
def _gather_op(tensors, anc):
    B, per = tensors[0].shape
    arr = (ctypes.c_void_p * len(tensors))(*[v.data_ptr() for v in tensors])
    _lib.check(_lib.lib().vd_op_particle_gather(B, per, _lib.ptr(anc), arr, len(tensors), _lib.current_stream()))
    torch.cuda.synchronize()


def _bit_tensor(B, per, seed, misalign):
    """Random bit patterns (NaNs and infinities among them) as a (B, per) float32 view, 16-byte aligned or 4 bytes off."""
    g = torch.Generator().manual_seed(seed)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (B * per,), generator=g, dtype=torch.int64).to(torch.int32)
    buf = torch.empty(B * per + 4, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    out = buf[1:1 + B * per] if misalign else buf[:B * per]
    out.copy_(bits)
    return out.view(B, per)


MAPS = {"identity": [0, 1, 2, 3, 4, 5], "one-parent": [4, 4, 4, 4, 4, 4], "two-cycle": [1, 0, 2, 3, 4, 5], "three-cycle": [0, 1, 2, 4, 5, 3],
        "chain": [0, 0, 1, 2, 3, 3], "batched": [1, 0, 2, 5, 5, 5]}


@pytest.mark.parametrize("per", [1, 3, 4, 1021, 3 * 32 * 32 * 5])
def test_gather_is_bit_exact(per):
    """Item i takes item ancestors[i], out of place: the identity, one parent for all, cycles of two and three, a chain in which a source
    is itself overwritten, on 1 to 4 tensors, 16-byte aligned (the float4 form where per % 4 == 0) and 4 bytes off (the scalar form)."""
    B = 6
    for name, m in MAPS.items():
        anc = torch.tensor(m, dtype=torch.int32, device="cuda")
        for n in (1, 2, 3, 4):
            for misalign in (False, True):
                xs = [_bit_tensor(B, per, 10 * n + k, misalign and k % 2 == 0 or misalign and n == 1) for k in range(n)]
                want = [v.clone()[anc.long()] for v in xs]
                _gather_op([v.view(torch.float32) for v in xs], anc)
                for k in range(n):
                    assert torch.equal(xs[k], want[k]), (name, n, misalign, k)
    # a batched call gives the bits of each group alone (groups of 3: a two-cycle in the first, one parent in the second)
    x = _bit_tensor(B, per, 99, False)
    whole = x.clone()
    _gather_op([whole.view(torch.float32)], torch.tensor(MAPS["batched"], dtype=torch.int32, device="cuda"))
    for g, local in enumerate(([1, 0, 2], [2, 2, 2])):
        alone = x[3 * g:3 * g + 3].clone()
        _gather_op([alone.view(torch.float32)], torch.tensor(local, dtype=torch.int32, device="cuda"))
        assert torch.equal(alone, whole[3 * g:3 * g + 3])


# ------------------------------------------------------------------------------------------------------------ steps
G_, K_, T_, S_ = 2, 3, 5, 32


def _cfg(T=T_, respacing="ddim10", **over):
    return tiny_cfg(T, timestep_respacing=respacing, **over)


def _group_window(G, K, T, seed, n_obs=2):
    """A window of G videos as K consecutive particles each: a group's items share the masks, the indices and the observed content and
    differ in x_t -> (the window dict on the host, the truth video (G, T, 3, S, S))."""
    c = rand_window(G, T, S_, n_obs, seed)
    rep = {k: v.repeat_interleave(K, dim=0) for k, v in c.items()}
    rep["x"] = torch.randn(G * K, T, 3, S_, S_, generator=torch.Generator().manual_seed(seed + 1))
    truth = torch.rand(G, T, 3, S_, S_, generator=torch.Generator().manual_seed(seed + 2)) * 2 - 1
    return rep, truth


def _measurement(truth, K, s, gray, sigma, seed):
    y = measure(truth, s, gray)
    y = y + sigma * torch.randn(y.shape, generator=torch.Generator().manual_seed(seed))
    return y.repeat_interleave(K, dim=0).cuda()


def _tt(B, v):
    return torch.tensor([v] * B, device="cuda")


def _noise(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).cuda()


def _reward_and_bar(x0, y, lat, s, gray, sigma, lam):
    """r in float64 from the engine's own x_0 (through measure) and the bar on lam * r.  test_gpu_dps.py bounds the engine's residual norm
    rho against the float64 norm of its own pred_xstart by dps_restated.seed_bound(x0, 0, y, lat, s, gray)['rho'] = (rho, d): the float32
    cell means and residuals, and the fp64 sum.  (d also holds the rounding of rho to float32, which the reward does not make: the bar is
    the looser for it.)  The reward is r = -rho^2 / (2 sigma^2), so |r_dev - r| <= ((rho + d)^2 - rho^2) / (2 sigma^2) = (2 rho d + d^2) /
    (2 sigma^2), and from a state of 0 the log-weight is lam r."""
    x0n, yn, latn = x0.detach().cpu().numpy().astype(np.float64), y.detach().cpu().numpy().astype(np.float64), lat.detach().cpu().numpy().reshape(x0.shape[0], -1)
    rho, d = seed_bound(x0n, np.zeros_like(x0n), yn, latn, s, gray)["rho"]
    r = pr.measurement_reward(x0n, yn, s, gray, latn, sigma)
    assert np.allclose(r, -rho ** 2 / (2 * sigma ** 2), rtol=1e-12)
    return r, lam * (2 * rho * d + d * d) / (2 * sigma ** 2)


@pytest.mark.parametrize("s,gray", [(2, False), (1, True)], ids=["sr2", "gray"])
def test_builtin_reward_against_restatement(s, gray):
    """B = 6 as G = 2 x K = 3, T = 5.  A step that cannot resample (ess_threshold 0) hands out the plain step's tensors and the log-weights
    lam r: compared with the restatement fed with that pred_xstart inside the bar of _reward_and_bar.  The same step with ess_threshold 1
    resamples: its ancestors are the restatement's -- the thresholds keep 4 x the bar away from every c_k: p_k moves by at most a factor
    exp(2 bar) -- and its tensors are the plain ones gathered, to the bit.  The same at t == 0, where the reward is taken on the sample."""
    model, diff = engine(_cfg())
    c, truth = _group_window(G_, K_, T_, 40 + s)
    B, sigma, lam = G_ * K_, 1.5, 1.0
    y = _measurement(truth, K_, s, gray, 0.1, 7)
    kw = kwargs_of(c)
    x = c["x"].cuda()
    for t in (6, 0):
        noise = _noise(x.shape, 50 + t)
        plain = diff._step(0, model, x, _tt(B, t), True, None, kw, 0.0, noise)
        u = torch.tensor([[0.37, 0.61], [0.83, 0.12]], dtype=torch.float64)
        with diff.steering_scope(model, particles=K_, scale=lam, ess_threshold=0.0, measurement=y, sr_scale=s, gray=gray, sigma_y=sigma,
                                 uniforms=lambda _t: u):
            sample, xstart = diff._step(0, model, x, _tt(B, t), True, None, kw, 0.0, noise)
            a = diff._last_steer
        assert torch.equal(sample, plain[0]) and torch.equal(xstart, plain[1])
        assert torch.equal(a["ancestors"].cpu(), torch.arange(B, dtype=torch.int32))
        r, bar = _reward_and_bar(sample if t == 0 else xstart, y, kw["latent_mask"], s, gray, sigma, lam)
        got = a["log_weights"].cpu().numpy()
        print(f"s={s} gray={gray} t={t}: log-weights {got}, max |d| / bar = {(np.abs(got - lam * r) / bar).max():.3f}, bar {bar.max():.3e}")
        assert (np.abs(got - lam * r) <= bar).all() and np.ptp(got[:K_]) > 0.05
        st = pr.new_state(G_, K_)
        want = pr.particle_weights(st, r.reshape(G_, K_), lam, 1.0, u.numpy(), np.full(G_, t == 0))
        assert _margin(want, u.numpy(), np.full(G_, t == 0)) > 4 * bar.max()
        with diff.steering_scope(model, particles=K_, scale=lam, ess_threshold=1.0, measurement=y, sr_scale=s, gray=gray, sigma_y=sigma,
                                 uniforms=lambda _t: u):
            sample2, xstart2 = diff._step(0, model, x, _tt(B, t), True, None, kw, 0.0, noise)
            b = diff._last_steer
        anc = torch.from_numpy(want["ancestors"]).long().cuda()
        assert np.array_equal(b["ancestors"].cpu().numpy(), want["ancestors"])
        assert torch.equal(sample2, sample[anc]) and torch.equal(xstart2, xstart[anc])
        if t == 0:
            assert np.array_equal(b["chosen"].cpu().numpy(), want["chosen"]) and np.array_equal(want["ancestors"], np.arange(B))
        else:
            assert want["resampled"].all() and "chosen" not in b and not b["log_weights"].any()
    model.check_device_errors()


def test_plain_step_to_the_bit():
    """particles=1, scale=0 and a reward that is constant over each group leave the plain step's bits, and so does a plain step behind a
    scope that resampled."""
    model, diff = engine(_cfg())
    c, _ = _group_window(G_, K_, T_, 61)
    B = G_ * K_
    kw, x, t = kwargs_of(c), c["x"].cuda(), _tt(B, 4)
    noise = _noise(x.shape, 62)
    plain = diff._step(0, model, x, t, True, None, kw, 0.0, noise)
    const = lambda x0, tt: torch.tensor([1.5, 1.5, 1.5, -2.0, -2.0, -2.0], device=x0.device)      # noqa: E731
    moving = lambda x0, tt: 40.0 * x0[:, 2:].mean(dim=(1, 2, 3, 4))                                 # noqa: E731
    for kwargs in (dict(particles=1), dict(particles=K_, scale=0.0), dict(particles=K_, reward_fn=const, ess_threshold=1.0)):
        with diff.steering_scope(model, kwargs.pop("reward_fn", moving), **kwargs):
            got = diff._step(0, model, x, t, True, None, kw, 0.0, noise)
            extras = diff._last_steer
        assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1]), kwargs
    lw = extras["log_weights"].cpu().view(G_, K_)                   # the constant reward: equal weights inside each group, nothing moved
    assert torch.equal(extras["ancestors"].cpu(), torch.arange(B, dtype=torch.int32)) and torch.equal(lw, lw[:, :1].expand(G_, K_))
    # rewards and uniforms under which both groups certainly move: p = (.007, .993, 0) and (.95, .002, .047) at thresholds 1/6, 1/2, 5/6
    uneven = lambda x0, tt: torch.tensor([0.0, 5.0, -5.0, 3.0, -3.0, 0.0], device=x0.device)        # noqa: E731
    with diff.steering_scope(model, uneven, particles=K_, ess_threshold=1.0, uniforms=lambda tt: torch.full((G_, 2), 0.5, dtype=torch.float64)):
        moved = diff._step(0, model, x, t, True, None, kw, 0.0, noise)
        assert diff._last_steer["ancestors"].tolist() == [1, 1, 1, 3, 3, 3]
    assert not torch.equal(moved[0], plain[0])
    again = diff._step(0, model, x, t, True, None, kw, 0.0, noise)
    assert diff._last_steer is None and torch.equal(again[0], plain[0]) and torch.equal(again[1], plain[1])
    assert _lib.lib().vd_particles(model._handle) == 0


def test_callback_path_against_restatement():
    """Two steps of a chain with the caller's reward: the weights, the ancestors and the gathered tensors are the restatement's on the
    rewards the callback returned; the public entries return the dict's new keys."""
    model, diff = engine(_cfg())
    c, _ = _group_window(G_, K_, T_, 71)
    B, lam = G_ * K_, 2.0
    kw, x = kwargs_of(c), c["x"].cuda()
    seen = []

    def reward(x0, tt):
        seen.append((30.0 * x0[:, 2:].mean(dim=(1, 2, 3, 4))).double())
        return seen[-1]

    us = {3: torch.tensor([[0.21, 0.5], [0.77, 0.5]], dtype=torch.float64), 2: torch.tensor([[0.55, 0.5], [0.05, 0.5]], dtype=torch.float64),
          0: torch.tensor([[0.5, 0.3], [0.5, 0.9]], dtype=torch.float64)}
    st = pr.new_state(G_, K_)
    with diff.steering_scope(model, reward, particles=K_, scale=lam, ess_threshold=1.0, uniforms=lambda tt: us[int(tt[0])]):
        for t in (3, 2):
            noise = _noise(x.shape, 72 + t)
            plain = diff._plain_step(0, model, x, _tt(B, t), True, None, kw, 0.0, noise)
            sample, xstart = diff._step(0, model, x, _tt(B, t), True, None, kw, 0.0, noise)
            a = diff._last_steer
            want = pr.particle_weights(st, seen[-1].cpu().numpy().reshape(G_, K_), lam, 1.0, us[t].numpy(), False)
            assert _margin(want, us[t].numpy(), np.zeros(G_, bool)) >= MARGIN and want["resampled"].all()
            anc = torch.from_numpy(want["ancestors"]).long().cuda()
            assert np.array_equal(a["ancestors"].cpu().numpy(), want["ancestors"])
            assert torch.equal(sample, plain[0][anc]) and torch.equal(xstart, plain[1][anc])
            assert np.array_equal(a["log_weights"].cpu().numpy(), st["logw"].reshape(-1))
            assert np.abs(a["ess"].cpu().numpy() - want["ess"]).max() <= ESS_BAR * K_
            x = sample
        out = diff.ddim_sample(model, x, _tt(B, 0), model_kwargs=kw, eta=1.0)
        assert {"ancestors", "ess", "log_weights", "chosen"} <= set(out) and out["chosen"].shape == (G_,)
        assert ((out["chosen"] >= 0) & (out["chosen"] < K_)).all()
        with pytest.raises(ValueError, match="NaN or \\+inf"):
            with diff.steering_scope(model, lambda x0, tt: torch.full((B,), float("nan")), particles=K_):
                diff.p_sample(model, x, _tt(B, 3), model_kwargs=kw)
        assert _lib.lib().vd_particles(model._handle) == K_          # the inner scope restored the outer setting
    assert _lib.lib().vd_particles(model._handle) == 0
    model.check_device_errors()


def _randn(n, seed, offset):
    out = torch.empty(n, device="cuda")
    _lib.check(_lib.lib().vd_randn(_lib.ptr(out), n, seed, offset, _lib.current_stream()))
    return out


def _graph_window(model, diff, c, y, sampler, eta, seed, s, sigma, tau, steps):
    """The window on the graph executor, one replay at a time -> per step (the window tensor, ancestors), and the final state."""
    wex = WindowExecutor(model, diff)
    wex.begin(c["x"].cuda(), kwargs_of(c), seed=seed, sampler=sampler, eta=eta, particles=K_, particle_measurement=y, particle_sr_scale=s,
              sigma_y=sigma, ess_threshold=tau)
    trace = []
    for _ in range(steps):
        x = wex.run(1).clone()
        trace.append((x, wex.particle_state()["ancestors"].clone()))
    return trace, wex.particle_state()


def _eager_window(model, diff, c, y, sampler, eta, seed, s, sigma, tau, steps):
    """The same window as eager steps that repeat the graph's draws: the sampler's noise from vd_randn at the head of step k's Philox
    range (dpmpp_2m_sde: the pass itself draws there), the uniforms from the same range through a (seed, offset) pair."""
    kw, x = kwargs_of(c), c["x"].cuda()
    B, n = x.shape[0], x.numel()
    trace, prev, out = [], None, None
    NT = diff.num_timesteps
    with diff.steering_scope(model, particles=K_, ess_threshold=tau, measurement=y, sr_scale=s, sigma_y=sigma,
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


@pytest.mark.parametrize("sampler,eta", [("p_sample", 0.0), ("ddim", 1.0), ("dpmpp_2m_sde", 0.0)])
def test_eager_against_graph(sampler, eta):
    """One whole window of five steps with the built-in reward: the samples of every step, the ancestors of every step and the particle
    chosen at t == 0 are the same bits on both executors, and the window resampled."""
    model, diff = engine(_cfg(respacing="ddim5"))
    c, truth = _group_window(G_, K_, T_, 81)
    y = _measurement(truth, K_, 2, False, 0.1, 8)
    args = (model, diff, c, y, sampler, eta, 1234567, 2, 1.5, 0.9, diff.num_timesteps)
    eager, last = _eager_window(*args)
    graph, state = _graph_window(*args)
    for k, ((xe, ae), (xg, ag)) in enumerate(zip(eager, graph)):
        assert torch.equal(xe, xg), (sampler, k)
        assert torch.equal(ae, ag), (sampler, k)
    assert torch.equal(last["chosen"].cpu(), state["chosen"]) and ((state["chosen"] >= 0) & (state["chosen"] < K_)).all()
    assert torch.equal(last["log_weights"].cpu(), state["log_weights"])
    assert int(state["resamples"].sum()) > 0 and int(state["degenerate"].sum()) == 0
    model.check_device_errors()


@pytest.mark.parametrize("case", ["T40", "xstart"])
def test_reach_beyond_the_gradient_scopes(case):
    """A window of 40 frames (the long-window kernels) and a predict_xstart model: dps_scope and loss_guidance_scope refuse both by name,
    a steered step and a steered window graph serve them and resample.  This test cannot pass without particle steering."""
    T = 40 if case == "T40" else T_
    model, diff = engine(_cfg(T, respacing="ddim5", **({} if case == "T40" else {"predict_xstart": True})))
    c, truth = _group_window(1, K_, T, 91, n_obs=3)
    y = _measurement(truth, K_, 4, False, 0.1, 9)
    kw, x, B = kwargs_of(c), c["x"].cuda(), K_
    name = "at most 32 frames" if case == "T40" else "predict_xstart|epsilon-prediction"
    with pytest.raises((NotImplementedError, _lib.VdError), match=name):
        with diff.dps_scope(model, y, 4, zeta=0.5):
            diff.p_sample(model, x, _tt(B, 4), model_kwargs=kw)
    with pytest.raises((NotImplementedError, _lib.VdError), match=name):
        with diff.loss_guidance_scope(model, lambda x0, t: x0.sum(), scale=1.0):
            diff.p_sample(model, x, _tt(B, 4), model_kwargs=kw)
    plain = diff._step(0, model, x, _tt(B, 4), True, None, kw, 0.0, _noise(x.shape, 92))
    with diff.steering_scope(model, particles=K_, ess_threshold=1.0, measurement=y, sr_scale=4, sigma_y=1.0):
        sample, xstart = diff._step(0, model, x, _tt(B, 4), True, None, kw, 0.0, _noise(x.shape, 92))
        a = diff._last_steer
    anc = a["ancestors"].long()
    assert torch.isfinite(sample).all() and torch.equal(sample, plain[0][anc]) and torch.equal(xstart, plain[1][anc])
    assert float(a["ess"][0]) < K_ and not a["log_weights"].any()            # unequal weights under ess_threshold 1: the group resampled
    trace, state = _graph_window(model, diff, c, y, "p_sample", 0.0, 77, 4, 1.0, 1.0, diff.num_timesteps)
    assert torch.isfinite(trace[-1][0]).all() and int(state["resamples"][0]) >= 3 and 0 <= int(state["chosen"][0]) < K_
    model.check_device_errors()


# ------------------------------------------------------------------------------------------------------------ infer_video
def test_infer_video_with_particles(monkeypatch):
    """2 videos of 10 frames, K = 3, two windows of 'autoreg' (6 frames, 2 observed, 4 new): the return has the batch's shape, the
    observed frames are the batch's, and every window's new frames are, to the bit, those of ONE of that video's three particles -- the
    chosen one.  The caller's reward on the eager executor; the built-in reward on both, which agree to the bit under dpmpp_2m_sde."""
    from video_diffusion_amd import video_sample as vs
    model, diff = engine(_cfg(6, respacing="ddim5"))
    g = torch.Generator().manual_seed(60)
    batch = (torch.rand(2, 10, 3, S_, S_, generator=g) * 2 - 1).cuda()
    y = measure(torch.rand(2, 10, 3, S_, S_, generator=g) * 2 - 1, 4, False) + 0.1 * torch.randn(2, 10, 3, 8, 8, generator=g)
    seen = []
    real = vs._chosen_for_all

    def spy(local, chosen, K):
        seen.append((local.clone().cpu(), chosen.clone().cpu()))
        return real(local, chosen, K)

    monkeypatch.setattr(vs, "_chosen_for_all", spy)
    runs = {}
    for name, kwargs in (("callback", dict(reward_fn=lambda x0, t: 25.0 * x0[:, 2:].mean(dim=(1, 2, 3, 4)), ess_threshold=1.0)),
                         ("eager", dict(particle_measurement=y, sr_scale=4, sigma_y=1.0, ess_threshold=0.9, sampler="dpmpp_2m_sde")),
                         ("graph", dict(particle_measurement=y, sr_scale=4, sigma_y=1.0, ess_threshold=0.9, sampler="dpmpp_2m_sde", executor="graph"))):
        del seen[:]
        torch.manual_seed(61)
        out, _ = vs.infer_video("autoreg", model, diff, batch, 6, 2, 4, particles=K_, **kwargs)
        assert out.shape == tuple(batch.shape) and np.isfinite(out).all() and np.array_equal(out[:, :2], batch[:, :2].cpu().numpy())
        assert len(seen) == 2
        for w, (local, chosen) in enumerate(seen):
            assert local.shape[0] == 2 * K_ and ((chosen >= 0) & (chosen < K_)).all()
            for v in range(2):
                new = out[v, 2 + 4 * w:6 + 4 * w]
                same = [np.array_equal(new, local[v * K_ + k, -4:].numpy()) for k in range(K_)]
                assert same[int(chosen[v])] and sum(same) >= 1, (name, w, v, same)
        runs[name] = out
    assert np.array_equal(runs["eager"], runs["graph"]) and not np.array_equal(runs["eager"], runs["callback"])
    plain, _ = vs.infer_video("autoreg", model, diff, batch, 6, 2, 4, particles=1)
    assert plain.shape == tuple(batch.shape)
    for kwargs, name in ((dict(executor="graph", reward_fn=lambda x0, t: x0.sum(dim=(1, 2, 3, 4))), "reward_fn"), (dict(particle_measurement=y, sr_scale=4, sigma_y=1.0, sampler="unipc"), "unipc"),
                         (dict(particle_measurement=y, sr_scale=4, sigma_y=1.0, measurement=y), "a measurement"),
                         (dict(particle_measurement=y, sr_scale=4, sigma_y=1.0, use_gradient_method=True), "use_gradient_method"),
                         (dict(particle_measurement=y, sr_scale=4, sigma_y=1.0, executor="graph", prefix_cache=True), "prefix_cache")):
        with pytest.raises(NotImplementedError, match=name):
            vs.infer_video("autoreg", model, diff, batch, 6, 2, 4, particles=K_, **kwargs)
    model.check_device_errors()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_by_name():
    model, diff = engine(_cfg())
    c, truth = _group_window(G_, K_, T_, 95)
    B = G_ * K_
    kw, x, t = kwargs_of(c), c["x"].cuda(), _tt(B, 4)
    y = _measurement(truth, K_, 2, False, 0.1, 3)
    reward = lambda x0, tt: x0.mean(dim=(1, 2, 3, 4))                       # noqa: E731
    scope = lambda **k: diff.steering_scope(model, reward, particles=K_, **k)      # noqa: E731
    # the samplers that draw no noise, in Python and -- the engine's state set behind Python's back -- in the engine
    for call, name in ((lambda: diff.ddim_sample(model, x, t, model_kwargs=kw), "ddim_sample at eta = 0"),
                       (lambda: diff.dpmpp_2m_sample(model, x, t, model_kwargs=kw), "dpmpp_2m_sample"),
                       (lambda: diff.unipc_sample(model, x, t, model_kwargs=kw), "unipc_sample"),
                       (lambda: diff.ddim_reverse_sample(model, x, t, model_kwargs=kw), "ddim_reverse_sample")):
        with pytest.raises(NotImplementedError, match=name):
            with scope():
                call()
        L = _lib.lib()
        diff._bind(model)
        _lib.check(L.vd_set_particles(model._handle, K_, 1.0, 0.5, None, 1, 0, 0.0))
        try:
            with pytest.raises(_lib.VdError, match=name.split(" at ")[0] + ".*particle steering"):
                call()
        finally:
            _lib.check(L.vd_set_particles(model._handle, 0, 0.0, 0.0, None, 1, 0, 0.0))
    region = (torch.zeros_like(x), torch.zeros(B, T_, 1, S_, S_, device="cuda"))
    others = (("known_region_scope", lambda: diff.known_region_scope(model, *region)), ("measurement_scope", lambda: diff.measurement_scope(model, y, 2)),
              ("dps_scope", lambda: diff.dps_scope(model, y, 2, zeta=0.1)),
              ("loss_guidance_scope", lambda: diff.loss_guidance_scope(model, lambda x0, tt: x0.sum(), scale=1.0)))
    for name, other in others:
        for outer, inner in ((other, scope), (scope, other)):
            with pytest.raises(NotImplementedError, match=name + " together with steering_scope"):
                with outer():
                    with inner():
                        diff.p_sample(model, x, t, model_kwargs=kw)
    for kwargs, name in ((dict(use_gradient_method=True), "use_gradient_method"), (dict(return_attn_weights=True), "return_attn_weights")):
        with pytest.raises(NotImplementedError, match=name):
            with scope():
                diff.p_sample(model, x, t, model_kwargs=kw, **kwargs)
    with pytest.raises(ValueError, match="no multiple of particles"):
        with scope():
            diff.p_sample(model, x[:4], t[:4], model_kwargs={k: (v[:4] if torch.is_tensor(v) else v) for k, v in kw.items()})
    for kwargs, name in ((dict(measurement=y, sr_scale=2, sigma_y=0.0), "sigma_y"), (dict(measurement=y, sr_scale=2, sigma_y=-1.0), "sigma_y"),
                         (dict(measurement=y, sr_scale=2), "sigma_y"), (dict(reward_fn=reward, ess_threshold=1.5), "ess_threshold"),
                         (dict(reward_fn=reward, ess_threshold=-0.1), "ess_threshold"), (dict(reward_fn=reward, measurement=y, sigma_y=1.0), "exactly one"),
                         (dict(), "exactly one"), (dict(reward_fn=reward, scale=float("nan")), "scale")):
        with pytest.raises(ValueError, match=name):
            diff.steering_scope(model, particles=K_, **kwargs)
    with pytest.raises(ValueError, match="particles"):
        diff.steering_scope(model, reward, particles=257)
    # a learned variance: the step's own refusal, in front of everything else
    lmodel, ldiff = engine(_cfg(learn_sigma=True))
    with pytest.raises(AssertionError, match="learned variance"):
        with ldiff.steering_scope(lmodel, reward, particles=K_):
            ldiff.p_sample(lmodel, x, t, model_kwargs=kw)
    # the window executor: a callback cannot be captured; the cut steps, a known region, a measurement, B and the samplers
    with pytest.raises(NotImplementedError, match="reward_fn"):
        WindowExecutor(model, diff).begin(x, kw, particles=K_, reward_fn=reward)
    with pytest.raises(NotImplementedError, match="reward_fn"):
        with scope():
            WindowExecutor(model, diff).begin(x, kw)
    pk = dict(particles=K_, particle_measurement=y, particle_sr_scale=2, sigma_y=1.0)
    for wex, kwargs, name in ((WindowExecutor(model, diff, prefix_cache=True), {}, "prefix_cache"), (WindowExecutor(model, diff, suffix_skip=True), {}, "suffix_skip"),
                              (WindowExecutor(model, diff), dict(known_src=region[0], known_mask=region[1]), "known region"),
                              (WindowExecutor(model, diff), dict(measurement=y, sr_scale=2), "a measurement"),
                              (WindowExecutor(model, diff), dict(sampler="ddim", eta=0.0), "eta = 0"), (WindowExecutor(model, diff), dict(sampler="dpmpp_2m"), "dpmpp_2m"),
                              (WindowExecutor(model, diff), dict(sampler="unipc"), "unipc")):
        with pytest.raises(NotImplementedError, match=name):
            wex.begin(x, kw, **kwargs, **pk)
    with pytest.raises(ValueError, match="no multiple"):
        WindowExecutor(model, diff).begin(x, kw, **dict(pk, particles=4))
    with pytest.raises(ValueError, match="sigma_y"):
        WindowExecutor(model, diff).begin(x, kw, **dict(pk, sigma_y=0.0))
    # ... and the engine itself, behind Python's back: the callback state inside a window, the cut steps
    L = _lib.lib()
    for set_args, wex, name in (((K_, 1.0, 0.5, None, 1, 0, 0.0), WindowExecutor(model, diff), "callback between two steps cannot be captured"),
                                ((K_, 1.0, 0.5, _lib.ptr(y), 2, 0, 1.0), WindowExecutor(model, diff, prefix_cache=True), "prefix cache"),
                                ((K_, 1.0, 0.5, _lib.ptr(y), 2, 0, 1.0), WindowExecutor(model, diff, suffix_skip=True), "suffix skip")):
        _lib.check(L.vd_set_particles(model._handle, *set_args))
        try:
            with pytest.raises(_lib.VdError, match=name):
                wex.begin(x, kw)
        finally:
            _lib.check(L.vd_set_particles(model._handle, 0, 0.0, 0.0, None, 1, 0, 0.0))
            L.vd_set_window_prefix_cache(model._handle, 0)
            L.vd_set_window_suffix_skip(model._handle, 0)
    assert L.vd_set_particles(model._handle, K_, 1.0, 0.5, _lib.ptr(y), 2, 0, 0.0) != 0 and b"sigma_y" in L.vd_last_error()
    assert L.vd_set_particles(model._handle, K_, 1.0, 1.5, None, 1, 0, 0.0) != 0 and b"ess_threshold" in L.vd_last_error()
    assert L.vd_particles(model._handle) == 0
    again = diff.p_sample(model, x, t, model_kwargs=kw)
    assert torch.isfinite(again["sample"]).all() and "ancestors" not in again
