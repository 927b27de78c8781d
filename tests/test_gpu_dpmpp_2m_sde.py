"""GPU: dpmpp_2m_sde_sample (this project's extension: SDE-DPM-Solver++(2M), the stochastic second-order multistep sampler) -- the fused
pass, its noise, the law of its samples, the step on the network, its loops, its window graph, infer_video and the scopes -- against the
float64 restatement of the pass and the closed-form variance of the analytic model (tests/dpmpp_2m_sde_restated.py; the reference has
no such sampler, so there is no fixture), against the CPU oracle's network, and against itself (executor vs eager calls).  Every bound
is derived in dpmpp_2m_sde_restated.py, none is measured."""
import numpy as np
import pytest
import torch

from dpmpp_2m_restated import denoiser_coef
from dpmpp_2m_sde_restated import coefficients, final_variance, rounding_bound, start_variance, step_fp64, tables
from helpers import ATOL, RTOL, close
from test_gpu_dpmpp_2m import _denoised_fn, _rand_window, _t, _window_kw, tiny
from video_diffusion_amd import _lib
from video_diffusion_amd.executor import WindowExecutor
from video_diffusion_amd.script_util import create_gaussian_diffusion

pytestmark = pytest.mark.gpu
PER = 3 * 32 * 32


def _randn(shape, seed, offset):
    out = torch.empty(shape, device="cuda")
    _lib.check(_lib.lib().vd_randn(_lib.ptr(out), out.numel(), seed, offset, _lib.current_stream()))
    return out


def _pass(model, x, d_in, prev, t, clip, noise=None, seed=0, offset=0, sample=None, xstart=None):
    """vd_dpmpp_2m_sde_from_xstart on (B, per) tensors -> (sample, D_t)."""
    sample = torch.empty_like(x) if sample is None else sample
    xstart = torch.empty_like(x) if xstart is None else xstart
    _lib.check(_lib.lib().vd_dpmpp_2m_sde_from_xstart(model._handle, x.shape[0], x[0].numel(), _lib.ptr(x), _lib.ptr(d_in), _lib.ptr(prev),
                                                      _lib.ptr(t), clip, _lib.ptr(noise), seed, offset, _lib.ptr(sample), _lib.ptr(xstart),
                                                      _lib.current_stream()))
    return sample, xstart


def _check(diff, ts, x, d_t, d_prev, z, sample, tag):
    """sample against the float64 restatement fed the step's own float32 x, D_t, D_prev and z, per element inside the derived bound;
    ts: one index per item.  Returns the worst |d| / bound."""
    xn, dn, zn, sn = (v.detach().cpu().numpy().reshape(len(ts), -1) for v in (x, d_t, z, sample))
    pn = None if d_prev is None else d_prev.detach().cpu().numpy().reshape(len(ts), -1)
    worst = 0.0
    for b, tv in enumerate(ts):
        args = (xn[b], dn[b], None if pn is None else pn[b], zn[b], *tables(diff, tv), tv == 0)
        want, lim = step_fp64(*args)[0], rounding_bound(*args)
        err = np.abs(sn[b] - want)
        ratio = float((err / np.maximum(lim, 1e-300)).max())
        worst = max(worst, ratio)
        assert (err <= lim).all(), (tag, b, tv, ratio, float(err.max()))
    print(f"{tag}: max |d| / bound = {worst:.3f}")
    return worst


def _inputs(B, per, seed):
    g = torch.Generator().manual_seed(seed)
    x = (1.5 * torch.randn(B, per, generator=g)).cuda()
    d_in = (0.8 * torch.randn(B, per, generator=g)).cuda()                       # about a fifth beyond +-1: the clamp matters
    prev = (torch.rand(B, per, generator=g) * 2 - 1).cuda()
    z = torch.randn(B, per, generator=g).cuda()
    return x, d_in, prev, z


# ---------------------------------------------------------------------------------------------------------------- 1
def test_the_pass_per_element_against_float64():
    """The pass alone (vd_dpmpp_2m_sde_from_xstart, explicit noise), per element inside the bound of dpmpp_2m_sde_restated.rounding_bound:
    B = 3 with t = (0, N - 1, interior) per item; with and without history; clip on and off; history aliasing pred_xstart; sample
    aliasing x; per = 3 * 32 * 32, per = 4 (the smallest the 16-byte form takes) and per = 1 (the smallest of all); an odd per and a
    tensor 4 bytes off alignment (both served element by element: same values); B * per just above 4096 * 256 groups of four (the
    grid-stride loop's second trip); an item whose t is out of range (all its outputs NaN, its neighbours' bits untouched); a
    non-finite x_0.  (`hist_on` = 0 over a non-null history is a window graph's state: test_window_executor_runs_the_step_as_a_graph.)
    Measured on an MI355X: worst |d| / bound 0.324 over all cases (the second-trip case); the unaligned form gave the 16-byte form's bits."""
    model, diff = tiny()
    diff._bind(model)
    N = diff.num_timesteps
    ts = [0, N - 1, 4]
    tt = torch.tensor(ts, device="cuda")
    worst = 0.0
    for per in (PER, 4, 1, 1153):
        x, d_in, prev, z = _inputs(3, per, seed=per)
        for hist in (None, prev):
            for clip in (1, 0):
                sample, d_t = _pass(model, x, d_in, hist, tt, clip, noise=z)
                assert torch.equal(d_t, d_in.clamp(-1, 1) if clip else d_in)     # D_t: the x_0 handed in, clamped -- never the extrapolated D
                worst = max(worst, _check(diff, ts, x, d_t, hist, z, sample, f"per={per} hist={hist is not None} clip={clip}"))
                assert torch.equal(sample[0], d_t[0])                            # t = 0: the sample is D_0 -- no noise, no history
        # history kept in place (what the window graph does), and the sample written over x
        want_s, want_d = _pass(model, x, d_in, prev, tt, 1, noise=z)
        buf = prev.clone()
        got_s, got_d = _pass(model, x, d_in, buf, tt, 1, noise=z, xstart=buf)
        assert torch.equal(got_s, want_s) and torch.equal(buf, want_d) and got_d is buf
        xa = x.clone()
        got_s, _ = _pass(model, xa, d_in, prev, tt, 1, noise=z, sample=xa)
        assert torch.equal(xa, want_s) and got_s is xa
        # the weight multiplies the DIFFERENCE: a history equal to D_t itself is no history
        none_s, none_d = _pass(model, x, d_in, None, tt, 1, noise=z)
        same_s, _ = _pass(model, x, d_in, none_d, tt, 1, noise=z)
        assert torch.equal(same_s, none_s) and not torch.equal(want_s[2], none_s[2])
    # pred_xstart may be NULL: the same sample
    x, d_in, prev, z = _inputs(3, PER, seed=PER)
    want_s, want_d = _pass(model, x, d_in, prev, tt, 1, noise=z)
    only = torch.empty_like(x)
    _lib.check(_lib.lib().vd_dpmpp_2m_sde_from_xstart(model._handle, 3, PER, _lib.ptr(x), _lib.ptr(d_in), _lib.ptr(prev), _lib.ptr(tt), 1,
                                                      _lib.ptr(z), 0, 0, _lib.ptr(only), None, _lib.current_stream()))
    assert torch.equal(only, want_s)
    # a tensor 4 bytes off alignment is served element by element: inside the bound, and here the same bits
    off = torch.empty(3 * PER + 1, device="cuda")[1:].view(3, PER)
    off.copy_(x)
    assert off.data_ptr() % 16 == 4
    un_s, un_d = _pass(model, off, d_in, prev, tt, 1, noise=z)
    worst = max(worst, _check(diff, ts, x, un_d, prev, z, un_s, "x 4 bytes off alignment"))
    print(f"unaligned form bit-equal to the 16-byte form: {torch.equal(un_s, want_s)}")
    # an out-of-range t poisons its item and nothing else
    for bad in (N, -1):
        s, d = _pass(model, x, d_in, prev, torch.tensor([0, bad, 4], device="cuda"), 1, noise=z)
        assert torch.isnan(s[1]).all() and torch.isnan(d[1]).all()
        assert torch.equal(s[0], want_s[0]) and torch.equal(s[2], want_s[2]) and torch.equal(d[0], want_d[0]) and torch.equal(d[2], want_d[2])
    model.check_device_errors()                                                  # the network-free entry poisons only
    # a non-finite x_0 (NaN, and an infinity, which leaves as NaN too) sets the sticky bit and touches no other element
    bad_in = d_in.clone()
    bad_in[1, 7], bad_in[2, 9] = float("nan"), float("inf")
    s, d = _pass(model, x, bad_in, prev, tt, 1, noise=z)
    assert torch.isnan(s[1, 7]) and torch.isnan(d[1, 7]) and torch.isnan(s[2, 9]) and torch.isnan(d[2, 9])
    assert torch.isfinite(s).sum() == s.numel() - 2
    with pytest.raises(FloatingPointError):
        model.check_device_errors()
    model.check_device_errors()
    # just above 4096 blocks of 256 groups of four: the loop's second trip
    per = 4 * (4096 * 256 // 2 + 1)
    x, d_in, prev, z = _inputs(2, per, seed=8)
    sample, d_t = _pass(model, x, d_in, prev, torch.tensor([3, 6], device="cuda"), 1, noise=z)
    assert 2 * per // 4 > 4096 * 256
    worst = max(worst, _check(diff, [3, 6], x, d_t, prev, z, sample, f"per={per} (second trip)"))
    print(f"worst |d| / bound over all cases = {worst:.3f}")


def test_the_eps_path_per_element_and_a_start_x_input():
    """vd_dpmpp_2m_sde_sample (the network in front, explicit noise): pred_xstart is the pass's head on the returned network output
    -- two rounded products and a subtraction, then the clamp -- and the sample stays inside the bound on the step's own x, D_t, D_prev
    and z; on a START_X model the network output is D_t itself.  Measured on an MI355X: worst |d| / bound 0.335 (EPSILON), 0.337 (START_X)."""
    for start_x in (False, True):
        model, diff = tiny(predict_xstart=True) if start_x else tiny()
        diff._bind(model)
        N = diff.num_timesteps
        c = _rand_window(2, 6, 32, 2, seed=11)
        kw = model._pack_kwargs(c["x"].cuda(), _window_kw(c))
        x = c["x"].cuda()
        z = torch.randn(x.shape, generator=torch.Generator().manual_seed(12)).cuda()
        prev = (torch.rand(x.shape, generator=torch.Generator().manual_seed(13)) * 2 - 1).cuda()
        ts = [N - 2, 1]
        tt = torch.tensor(ts, device="cuda")
        sample, d_t, eps = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        _lib.check(_lib.lib().vd_dpmpp_2m_sde_sample(model._handle, 2, 6, *model._window_ptrs(x, kw), _lib.ptr(tt), _lib.ptr(prev), kw["obs_mode"], 1,
                                                     _lib.ptr(z), 0, 0, _lib.ptr(sample), _lib.ptr(d_t), _lib.ptr(eps), _lib.current_stream()))
        model.check_device_errors()
        if start_x:
            assert torch.equal(d_t, eps.clamp(-1, 1))
        else:
            for b, tv in enumerate(ts):
                a, bb = tables(diff, tv)[:2]
                xb, eb = x[b].double().cpu().numpy(), eps[b].double().cpu().numpy()
                want = np.clip(a * xb - bb * eb, -1.0, 1.0)
                lim = 2.0 ** -23 * (np.abs(a * xb) + np.abs(bb * eb))            # the two products and the difference: three roundings
                assert (np.abs(d_t[b].cpu().numpy() - want) <= lim).all()
        _check(diff, ts, x, d_t, prev, z, sample, f"eps path start_x={start_x}")


# ---------------------------------------------------------------------------------------------------------------- 2
def test_noise_identity_with_ddim_at_eta_one():
    """Same (seed, offset), no history: the sample is ddim_sample's at eta = 1 (vd_posterior_from_xstart, mode 1) -- both lie inside the
    bound of the same float64 value, so they differ by at most twice it -- and the z the pass implies, (sample - mean) / sigma
    recovered in float64, is vd_randn's element for that index within bound / sigma.  Whether the two samples are bit-equal is
    printed, not required (measured on an MI355X: they are not bit-equal; the worst difference was 0.12 of twice the bound)."""
    model, diff = tiny()
    diff._bind(model)
    N = diff.num_timesteps
    L = _lib.lib()
    x, d_in, _, _ = _inputs(2, PER, seed=21)
    seed, offset = 1234567, 4096
    z = _randn(x.shape, seed, offset)
    equal = []
    for ts in ([N - 1, 1], [5, 2]):
        tt = torch.tensor(ts, device="cuda")
        got, d_t = _pass(model, x, d_in, None, tt, 1, noise=None, seed=seed, offset=offset)
        assert torch.equal(got, _pass(model, x, d_in, None, tt, 1, noise=z)[0])  # the draw IS vd_randn's element i
        ddim = torch.empty_like(x)
        _lib.check(L.vd_posterior_from_xstart(model._handle, 1, 2, PER, _lib.ptr(x), _lib.ptr(d_in), _lib.ptr(tt), 1, 1.0, None, seed, offset,
                                              _lib.ptr(ddim), None, None, _lib.current_stream()))
        equal.append(bool(torch.equal(ddim, got)))
        for b, tv in enumerate(ts):
            args = (x[b].cpu().numpy(), d_t[b].cpu().numpy(), None, z[b].cpu().numpy(), *tables(diff, tv), False)
            lim = rounding_bound(*args)
            assert (np.abs(got[b].double().cpu().numpy() - ddim[b].double().cpu().numpy()) <= 2.0 * lim).all(), tv
            mean = step_fp64(*args)[3]
            sigma = coefficients(*tables(diff, tv)[2:4])[0]
            z_rec = (got[b].double().cpu().numpy() - mean) / sigma
            assert (np.abs(z_rec - z[b].double().cpu().numpy()) <= lim / sigma).all(), tv
    print(f"bit-equal to vd_posterior_from_xstart(mode 1, eta = 1): {equal}")
    # the entries that take a mode keep refusing every other value
    out = torch.empty_like(x)
    for mode in (2, 3, 4, 5, -1):
        assert L.vd_posterior_from_xstart(model._handle, mode, 2, PER, _lib.ptr(x), _lib.ptr(d_in), _lib.ptr(_t(2, 3)), 1, 1.0, None, 0, 0,
                                          _lib.ptr(out), None, None, _lib.current_stream()) != 0
        assert L.vd_posterior_update(model._handle, mode, 2, PER, _lib.ptr(x), _lib.ptr(d_in), _lib.ptr(_t(2, 3)), 1, 1.0, None, 0, 0,
                                     _lib.ptr(out), None, _lib.current_stream()) != 0
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 3
def test_law_of_the_final_sample_on_the_device():
    """n = 2^20 independent scalar chains on the analytic model (s = 0.5, logsnr40) through vd_dpmpp_2m_sde_from_xstart with Philox
    noise from a fixed seed: the variance of the result against the restatement's PREDICTED variance for this schedule (not s^2),
    |ratio - 1| <= 5 sqrt(2 / n) = 6.9e-3 -- five standard errors of a variance estimate.  Measured on an MI355X: Var = 2.548865e-01 against 2.549270e-01 predicted, |ratio - 1| = 1.59e-4."""
    model, _ = tiny()
    s, n, seed = 0.5, 2 ** 20, 20221118
    diff = create_gaussian_diffusion(timestep_respacing="logsnr40")
    try:
        diff._bind(model)
        acp = diff.alphas_cumprod
        x = _randn((1, n), seed, 0) * float(np.sqrt(start_variance(s, acp[-1])))
        prev = None
        for k, tv in enumerate(range(diff.num_timesteps - 1, -1, -1)):
            d = x * float(np.float32(denoiser_coef(s, acp[tv])))
            x, prev = _pass(model, x, d, prev, _t(1, tv), 0, noise=None, seed=seed, offset=(k + 1) * n)
    finally:
        model._bound_schedule = None                                             # the next test binds its own schedule again
    got = float((x.double() ** 2).mean())                                        # the mean is zero by symmetry: the second moment
    want = final_variance(diff, s)
    print(f"Var = {got:.6e}, predicted {want:.6e} (s^2 = {s * s}), |ratio - 1| = {abs(got / want - 1):.2e}, bar {5 * np.sqrt(2 / n):.2e}")
    assert abs(float(x.double().mean())) <= 5 * np.sqrt(want / n)
    assert abs(got / want - 1.0) <= 5.0 * np.sqrt(2.0 / n)
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 4
_oracles = {}


def _oracle(start_x):
    if start_x not in _oracles:
        import video_diffusion_amd as vda
        from helpers import synth_sd
        from oracle.unet_ref import UNetRef
        from test_gpu_dpmpp_2m import TINY
        model, diff = tiny(predict_xstart=True) if start_x else tiny()
        cfg = {**vda.video_model_and_diffusion_defaults(), **TINY, **({"predict_xstart": True} if start_x else {})}
        _oracles[start_x] = UNetRef(cfg, synth_sd(model.param_specs()))
    return _oracles[start_x]


@pytest.mark.parametrize("case", ["x_0", "x_t", "x_t_minus_1", "denoised_fn", "predict_xstart"])
def test_the_step_on_the_network_along_a_chain(case):
    """Four steps from the last index, each fed its predecessor's sample and x_0 prediction, noise from torch.manual_seed: the sample
    against the CPU oracle's network output at the same input, pushed through the float64 step with the same noise and history, at the
    tolerance test_gpu_dpmpp_2m.py uses for this chain (the network's error dominates); pred_xstart against ddim_sample's for the same
    input, as that test holds it; and the sample inside the derived bound of the float64 step fed the step's own D_t.  (pred_xstart
    against the oracle's is printed, not held to that tolerance: at the last index of logsnr10 sqrt_recipm1 = 157 multiplies the
    network's 2e-6 into 4e-4 in front of the clamp, while the sample sees it times sqrt(abp) sqrt_recipm1 - c < 4.)"""
    start_x = case == "predict_xstart"
    model, diff = tiny(predict_xstart=True) if start_x else tiny()
    net = _oracle(start_x)
    c = _rand_window(2, 6, 32, 2, seed=70)
    kw = _window_kw(c, case if case.startswith("x_") else "x_0")
    if case == "x_t_minus_1":
        kw["x_t_minus_1"] = (c["x0"] * 0.5).cuda()
    okw = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in kw.items()}
    fn = _denoised_fn if case == "denoised_fn" else None
    N = diff.num_timesteps
    tmap = torch.tensor(diff.timestep_map)
    x, prev = c["x"].cuda(), None
    for tv in range(N - 1, N - 5, -1):
        before = x.clone()
        torch.manual_seed(700 + tv)
        out = diff.dpmpp_2m_sde_sample(model, x, _t(2, tv), prev_xstart=prev, denoised_fn=fn, model_kwargs=kw)
        torch.manual_seed(700 + tv)
        z = torch.randn_like(x)                                                  # the step's draw: the first one behind the seed
        assert set(out) == {"sample", "pred_xstart"} and torch.equal(x, before) and out["sample"].data_ptr() != x.data_ptr()
        assert float(out["pred_xstart"].abs().max()) <= 1.0
        _check(diff, [tv, tv], x, out["pred_xstart"], prev, z, out["sample"], f"{case} t={tv}")
        # the oracle's network at the same x, then the float64 step
        o = net(x.cpu(), tmap[torch.tensor([tv, tv])], **okw).double()
        a, b, ab, abp, w = tables(diff, tv)
        d64 = o if start_x else a * x.cpu().double() - b * o
        if fn is not None:
            d64 = fn(d64)
        d64 = d64.clamp(-1, 1)
        ref = diff.ddim_sample(model, x, _t(2, tv), denoised_fn=fn, model_kwargs=kw, eta=1.0)
        close(out["pred_xstart"], ref["pred_xstart"], atol=ATOL, rtol=RTOL)
        print(f"{case} t={tv}: max |pred_xstart - oracle's| = {float((out['pred_xstart'].cpu().double() - d64).abs().max()):.3e}")
        want = step_fp64(x.cpu().numpy(), d64.numpy(), None if prev is None else prev.cpu().numpy(), z.cpu().numpy(), a, b, ab, abp, w, tv == 0)[0]
        close(out["sample"].cpu(), torch.from_numpy(want).float(), atol=ATOL, rtol=RTOL)
        x, prev = out["sample"], out["pred_xstart"]
    assert torch.isfinite(x).all()
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 5
def test_loops_chain_the_step_and_differ_from_ddim_behind_the_first_step():
    model, diff = tiny()
    c = _rand_window(2, 6, 32, 2, seed=80)
    kw = _window_kw(c)
    x_T = c["x"].cuda()
    N = diff.num_timesteps
    torch.manual_seed(81)
    outs = list(diff.dpmpp_2m_sde_sample_loop_progressive(model, tuple(x_T.shape), noise=x_T, model_kwargs=kw))
    assert len(outs) == N and all(set(o) == {"sample", "pred_xstart"} for o in outs)
    torch.manual_seed(81)
    x, prev = x_T, None
    for k, tv in enumerate(range(N - 1, -1, -1)):
        o = diff.dpmpp_2m_sde_sample(model, x, _t(2, tv), prev_xstart=prev, model_kwargs=kw)
        assert torch.equal(o["sample"], outs[k]["sample"]) and torch.equal(o["pred_xstart"], outs[k]["pred_xstart"]), tv
        x, prev = o["sample"], o["pred_xstart"]
    torch.manual_seed(81)
    final = diff.dpmpp_2m_sde_sample_loop(model, tuple(x_T.shape), noise=x_T, model_kwargs=kw)
    assert torch.is_tensor(final) and torch.equal(final, x) and torch.isfinite(final).all()
    torch.manual_seed(82)
    assert not torch.equal(diff.dpmpp_2m_sde_sample_loop(model, tuple(x_T.shape), noise=x_T, model_kwargs=kw), final)   # it is stochastic
    # ddim_sample_loop at eta = 1 under the same seed draws the same noise: the first step agrees within the two bounds, the second differs
    torch.manual_seed(81)
    ddim = list(diff.ddim_sample_loop_progressive(model, tuple(x_T.shape), noise=x_T, model_kwargs=kw, eta=1.0))
    torch.manual_seed(81)
    z = torch.randn_like(x_T)
    assert torch.equal(ddim[0]["pred_xstart"], outs[0]["pred_xstart"])
    args = (x_T.cpu().numpy().reshape(2, -1), outs[0]["pred_xstart"].cpu().numpy().reshape(2, -1), None, z.cpu().numpy().reshape(2, -1),
            *tables(diff, N - 1), False)
    lim = rounding_bound(*args)
    d0 = np.abs(ddim[0]["sample"].double().cpu().numpy() - outs[0]["sample"].double().cpu().numpy()).reshape(2, -1)
    print(f"first step against ddim eta = 1: max |d| / (2 bound) = {(d0 / (2 * lim)).max():.3f}, bit-equal {torch.equal(ddim[0]['sample'], outs[0]['sample'])}")
    assert (d0 <= 2.0 * lim).all()
    d1 = (ddim[1]["sample"] - outs[1]["sample"]).abs().max()
    assert float(d1) > 1e-3 and not torch.equal(ddim[-1]["sample"], final)
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 6
def _chain(model, diff, x_init, kw, seed, ops, src=None, mask=None, keep=()):
    """The window's documented arithmetic from the eager entries: op k owns the Philox range [k n, (k + 1) n), n = B per; a step draws
    its noise at k n (vd_randn, handed in as a tensor) and, with a region, its merge noise at k n + n // 4; a jump draws at k n and
    drops the history."""
    L = _lib.lib()
    B, T, _, S, _ = x_init.shape
    n = x_init.numel()
    lat = kw["latent_mask"].reshape(-1).float().contiguous()
    x, prev, kept = x_init.clone(), None, {}
    for k, (op, tv) in enumerate(ops):
        tt = _t(B, tv)
        if op == "jump":
            out = torch.empty_like(x)
            _lib.check(L.vd_q_jump(model._handle, B, T, S * S, _lib.ptr(x), _lib.ptr(lat), _lib.ptr(tt), _lib.ptr(_randn(x.shape, seed, k * n)), 0, 0,
                                   _lib.ptr(out), _lib.current_stream()))
            x, prev = out, None
        else:
            x, prev = diff._fused_step(4, model, x, tt, True, kw, noise=_randn(x.shape, seed, k * n), prev_xstart=prev)
            if src is not None:
                z = _randn(x.shape, seed, k * n + n // 4)
                _lib.check(L.vd_known_merge(model._handle, B, T, S * S, _lib.ptr(x), _lib.ptr(src), _lib.ptr(mask), _lib.ptr(lat), _lib.ptr(tt),
                                            _lib.ptr(z), 0, 0, _lib.current_stream()))
        if k + 1 in keep:
            kept[k + 1] = x.clone()
    return x, kept


def test_window_executor_runs_the_step_as_a_graph():
    """sampler='dpmpp_2m_sde': history and Philox state both live in the graph.  The window is bit-equal to the eager chain fed the same
    Philox noise: two windows of one shape on ONE graph (the second one's first step without history although the buffer holds the
    first window's: `hist_on` = 0 over a non-null history), run(k) then run(), a later t_start, 'x_0' / 'x_t' / 'x_t_minus_1' as handed;
    eta is no part of the signature; jump() drops the history; the re-noising 'x_t_minus_1' form is served."""
    model, diff = tiny()
    diff._bind(model)
    N = diff.num_timesteps
    ex = WindowExecutor(model, diff)
    steps = [("step", tv) for tv in range(N - 1, -1, -1)]
    g0 = None
    for wi, (n_obs, obsf) in enumerate([(2, "x_0"), (2, "x_0"), (2, "x_t"), (3, "x_t_minus_1")]):
        c = _rand_window(2, 6, 32, n_obs, seed=900 + wi)
        kw = _window_kw(c, obsf)
        if obsf == "x_t_minus_1":
            kw["x_t_minus_1"] = (c["x0"] * 0.5).cuda()
        x_init = c["x"].cuda()
        ex.begin(x_init, kw, sampler="dpmpp_2m_sde", seed=50 + wi, renoise=False, eta=0.25 * wi)
        assert ex._left == N
        if wi == 0:
            g0 = ex.graphs
        if wi == 1:
            assert ex.graphs == g0                                               # same signature (eta is not read): the first window's graph
        got_mid = ex.run(3).clone()
        got = ex.run().clone()
        with pytest.raises(_lib.VdError, match="t would pass 0"):
            ex.run(1)
        want, kept = _chain(model, diff, x_init, kw, 50 + wi, steps, keep=(3,))
        assert torch.equal(kept[3], got_mid), (wi, obsf, float((kept[3] - got_mid).abs().max()))
        assert torch.equal(want, got) and torch.isfinite(got).all(), (wi, obsf, float((want - got).abs().max()))
        if wi == 1:                                                              # a later start on the same graph: without history at t = 6
            ex.begin(x_init, kw, sampler="dpmpp_2m_sde", seed=60, t_start=6, renoise=False)
            assert ex.graphs == g0 and ex._left == 7
            assert torch.equal(ex.run().clone(), _chain(model, diff, x_init, kw, 60, steps[N - 7:])[0])
            # the eager step handed the Philox state instead of a tensor draws the same noise
            o = diff._dpmpp_2m_sde(model, x_init, _t(2, 6), None, True, None, kw, philox=(60, 0))
            assert torch.equal(o["sample"], _chain(model, diff, x_init, kw, 60, steps[N - 7:N - 6])[0])
    model.check_device_errors()
    # it differs from the 'ddim' window at eta = 1 under the same seed (same noise, same first step up to rounding) and from 'dpmpp_2m'
    c = _rand_window(2, 6, 32, 2, seed=950)
    kw, x_init = _window_kw(c), c["x"].cuda()
    sde = ex.begin(x_init, kw, sampler="dpmpp_2m_sde", seed=7).run().clone()
    g = ex.graphs
    assert not torch.equal(ex.begin(x_init, kw, sampler="ddim", eta=1.0, seed=7).run().clone(), sde) and ex.graphs == g + 1
    assert not torch.equal(ex.begin(x_init, kw, sampler="dpmpp_2m").run().clone(), sde) and ex.graphs == g + 2
    assert torch.equal(ex.begin(x_init, kw, sampler="dpmpp_2m_sde", seed=7).run().clone(), sde) and ex.graphs == g + 2
    # the re-noising 'x_t_minus_1' form (the observed frames drawn inside the graph from the second half of the step's range): served
    kw2 = _window_kw(c, "x_t_minus_1")
    a = ex.begin(x_init, kw2, sampler="dpmpp_2m_sde", seed=8, renoise=True).run().clone()
    b = ex.begin(x_init, kw2, sampler="dpmpp_2m_sde", seed=8, renoise=True).run().clone()
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert not torch.equal(a, ex.begin(x_init, kw2, sampler="dpmpp_2m_sde", seed=8, renoise=False).run().clone())
    # jump() drops the history (a window with a known region): run(3), jump(2), run() against the eager walk
    from test_gpu_known_region import _window_region
    src, mask, _ = _window_region(c, seed=951)
    ops = [("step", N - 1 - i) for i in range(3)] + [("jump", N - 3), ("jump", N - 2)] + [("step", tv) for tv in range(N - 2, -1, -1)]
    ex.begin(x_init, kw, sampler="dpmpp_2m_sde", seed=9, known_src=src, known_mask=mask)
    ex.run(3)
    up = ex.jump(2).clone()
    got = ex.run().clone()
    want, kept = _chain(model, diff, x_init, kw, 9, ops, src, mask, keep=(5,))
    assert torch.equal(kept[5], up) and torch.equal(want, got), float((want - got).abs().max())
    model.check_device_errors()


def test_window_with_suffix_skip_leaves_every_read_frame_bit_identical():
    model, diff = tiny()
    plain, skip = WindowExecutor(model, diff), WindowExecutor(model, diff, suffix_skip=True)
    for wi, (B, T, n_obs, obsf) in enumerate([(2, 6, 2, "x_0"), (3, 5, 4, "x_t_minus_1")]):
        c = _rand_window(B, T, 32, n_obs, seed=960 + wi)
        read = ~((c["obs_mask"].reshape(B, T) == 1) & (c["latent_mask"].reshape(B, T) == 0))
        kw = _window_kw(c, obsf)
        x_init = c["x"].cuda()
        want = plain.begin(x_init, kw, sampler="dpmpp_2m_sde", seed=3, renoise=False).run().clone().cpu()
        skip.begin(x_init, kw, sampler="dpmpp_2m_sde", seed=3, renoise=False)
        assert skip.suffix_frames == int(read.sum())
        got = skip.run().clone().cpu()
        assert torch.isfinite(got[read]).all() and torch.equal(got[read], want[read]), (wi, float((got[read] - want[read]).abs().max()))
    model.check_device_errors()


def test_missing_weight_row_fails_by_name():
    model, diff = tiny(timestep_respacing="logsnr5")
    diff._bind(model)
    L = _lib.lib()
    x = torch.randn(2, PER).cuda()
    tab = diff._device_tables()
    tm = np.ascontiguousarray(np.array(diff.timestep_map, dtype=np.int32))
    try:
        _lib.check(L.vd_set_schedule(model._handle, diff.num_timesteps, _lib.ptr(tab), _lib.ptr(tm), 1.0))
        with pytest.raises(_lib.VdError, match="dpmpp_2m_sde_sample: no multistep weight row.*vd_set_multistep_weights"):
            _pass(model, x, x, None, _t(2, 2), 1, noise=x)
        c = _rand_window(2, 6, 32, 2, seed=3)
        model._bound_schedule = diff                                             # keep the step from re-binding: the row stays dropped
        with pytest.raises(_lib.VdError, match="dpmpp_2m_sde_sample: no multistep weight row"):
            diff.dpmpp_2m_sde_sample(model, c["x"].cuda(), _t(2, 2), model_kwargs=_window_kw(c))
        with pytest.raises(_lib.VdError, match=r"sampler 4 \(dpmpp_2m_sde_sample\): no multistep weight row"):
            WindowExecutor(model, diff).begin(c["x"].cuda(), _window_kw(c), sampler="dpmpp_2m_sde")
    finally:
        model._bound_schedule = None
    diff._bind(model)
    _pass(model, x, x, None, _t(2, 2), 1, noise=x)
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 7
def test_infer_video_graph_and_eager_agree_to_the_bit():
    from video_diffusion_amd.video_sample import infer_video
    model, diff = tiny()
    g = torch.Generator().manual_seed(10)
    batch = (torch.rand(2, 12, 3, 32, 32, generator=g) * 2 - 1).cuda()
    out = {}
    for executor in ("eager", "graph"):
        torch.manual_seed(101)
        out[executor], _ = infer_video("autoreg", model, diff, batch, 6, 2, 4, sampler="dpmpp_2m_sde", executor=executor)
    eager = out["eager"]
    assert eager.shape == (2, 12, 3, 32, 32) and np.isfinite(eager).all()
    assert np.array_equal(eager, out["graph"])
    assert np.array_equal(eager[:, :2], batch[:, :2].cpu().numpy()) and np.abs(eager[:, 2:]).max() > 0
    torch.manual_seed(101)
    ddim, _ = infer_video("autoreg", model, diff, batch, 6, 2, 4, sampler="ddim", executor="eager")
    assert not np.array_equal(ddim, eager)
    torch.manual_seed(102)
    assert not np.array_equal(infer_video("autoreg", model, diff, batch, 6, 2, 4, sampler="dpmpp_2m_sde")[0], eager)   # another seed, other frames
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 8
def test_cfg_and_guidance_scopes_compose():
    """Inside cfg_scale_scope the fused step is the step through denoised_fn = identity (the guided p_mean_variance with its clamp off in
    front of the network-free entry) to the bit; inside guidance_scope as well the composition by hand: both network outputs, the
    rescale op, the pass's x_0 head, the threshold op, then vd_dpmpp_2m_sde_from_xstart with its clamp off."""
    from test_gpu_guidance import B, FE, T, _kw, _noise, _rescale, _threshold, _window
    from test_gpu_guidance import _t as _tg, tiny as gtiny
    for start_x in (False, True):
        model, diff = gtiny(predict_xstart=True) if start_x else gtiny()
        diff._bind(model)
        c = _window(50)
        kw, nz, x, t = _kw(c), _noise(51), c["x"], _tg(5)
        prev = (0.3 * x).clamp(-1, 1)
        w, phi, p = 2.0, 0.7, 0.995
        with diff.cfg_scale_scope(model, w):
            got = diff._dpmpp_2m_sde(model, x, t, prev, True, None, kw, noise=nz)
            via = diff._dpmpp_2m_sde(model, x, t, prev, True, lambda v: v, kw, noise=nz)
        plain = diff._dpmpp_2m_sde(model, x, t, prev, True, None, kw, noise=nz)
        assert torch.equal(got["sample"], via["sample"]) and torch.equal(got["pred_xstart"], via["pred_xstart"])
        assert not torch.equal(got["sample"], plain["sample"])
        # by hand
        lat = c["latent_mask"].reshape(B, T).contiguous()
        out_c = diff.p_mean_variance(model, x, t, clip_denoised=False, model_kwargs=kw)["eps"]
        out_u = diff.p_mean_variance(model, x, t, clip_denoised=False, model_kwargs=_kw(c, zero_obs=True))["eps"]
        out = _rescale(out_c.view(B, T, FE), out_u.view(B, T, FE), w, lat, phi)[0].view_as(x)
        if start_x:
            x0 = out
        else:
            x0, dummy = torch.empty_like(x), torch.empty_like(x)
            _lib.check(_lib.lib().vd_posterior_update(model._handle, 0, B, x[0].numel(), _lib.ptr(x), _lib.ptr(out), _lib.ptr(t), 0, 0.0, _lib.ptr(nz),
                                                      0, 0, _lib.ptr(dummy), _lib.ptr(x0), _lib.current_stream()))
        x0 = _threshold(x0.view(B, T, FE), lat, p)[0].view_as(x)
        flat = lambda v: v.reshape(B, -1)                                        # noqa: E731
        want_s, want_d = _pass(model, flat(x), flat(x0), flat(prev), t, 0, noise=flat(nz))
        with diff.guidance_scope(model, cfg_rescale=phi, dynamic_threshold=p):
            with diff.cfg_scale_scope(model, w):
                g2 = diff._dpmpp_2m_sde(model, x, t, prev, True, None, kw, noise=nz)
        assert torch.equal(flat(g2["pred_xstart"]), want_d) and torch.equal(flat(g2["sample"]), want_s), float((flat(g2["sample"]) - want_s).abs().max())
        assert not torch.equal(g2["sample"], got["sample"])
        model.check_device_errors()


def test_known_region_and_measurement_scopes_compose_and_dps_refuses():
    from test_gpu_known_region import _flat, _np, _window_region, merged
    from measurement_restated import measure_fp64
    from test_gpu_measurement import _final_bound, _project, _window_measurement
    model, diff = tiny()
    N = diff.num_timesteps
    L = _lib.lib()
    c = _rand_window(2, 6, 32, 2, seed=30)
    kw, x = _window_kw(c), c["x"].cuda()
    lat = kw["latent_mask"].reshape(-1).float().contiguous()
    src, mask, z = _window_region(c, seed=31)
    noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(32)).cuda()
    prev = (torch.rand(x.shape, generator=torch.Generator().manual_seed(33)) * 2 - 1).cuda()
    flat = lambda v: v.reshape(2, -1)                                            # noqa: E731
    sel = torch.from_numpy(merged(_flat(mask)[0], _np(kw["latent_mask"]).reshape(2, 6))).view(x.shape).cuda()
    for tv in (N - 1, 3, 0):
        tt = _t(2, tv)
        plain, plain_x0 = diff._fused_step(4, model, x, tt, True, kw, noise=noise, prev_xstart=prev)
        # known region: the merge pass behind the plain step, by hand
        with diff.known_region_scope(model, src, mask, known_noise=z):
            got, got_x0 = diff._fused_step(4, model, x, tt, True, kw, noise=noise, prev_xstart=prev)
        want = plain.clone()
        _lib.check(L.vd_known_merge(model._handle, 2, 6, 32 * 32, _lib.ptr(want), _lib.ptr(src), _lib.ptr(mask), _lib.ptr(lat), _lib.ptr(tt),
                                    _lib.ptr(z), 0, 0, _lib.current_stream()))
        assert torch.equal(got, want) and torch.equal(got_x0, plain_x0) and not torch.equal(got, plain)
        if tv == 0:
            assert torch.equal(got[sel], src[sel])                               # the last step: known pixels bit-exact
        # measurement: the projection in front of the network-free entry, by hand
        for s, gray in ((4, False), (1, True)):
            y = _window_measurement(c, s, gray, seed=71)
            with diff.measurement_scope(model, y, s, gray):
                got, got_x0 = diff._fused_step(4, model, x, tt, True, kw, noise=noise, prev_xstart=prev)
            want_x0 = _project(model, plain_x0, y, kw["latent_mask"].reshape(2, 6), s, gray)
            want_s, want_d = _pass(model, flat(x), flat(want_x0), flat(prev), tt, 0, noise=flat(noise))
            assert torch.equal(got_x0, want_x0) and torch.equal(flat(got), want_s) and torch.equal(want_d, flat(want_x0))
            if tv == 0:                                                          # the last step returns the projected x_0: A(sample) = y up to rounding
                assert torch.equal(got, got_x0)
                a_err = np.abs(measure_fp64(_np(got), s, gray) - _np(y))[:, 2:]
                assert (a_err <= _final_bound(_np(got), _np(y), s, gray)[:, 2:]).all()         # the bound test_gpu_measurement.py derives
    with diff.known_region_scope(model, src, mask):
        with pytest.raises(NotImplementedError, match="denoised_fn inside known_region_scope"):
            diff.dpmpp_2m_sde_sample(model, x, _t(2, 3), denoised_fn=lambda v: v, model_kwargs=kw)
    y = _window_measurement(c, 4, False, seed=72)
    with diff.dps_scope(model, y, 4, zeta=0.5):
        with pytest.raises(_lib.VdError, match="dpmpp_2m_sde_sample inside dps_scope is not served"):
            diff.dpmpp_2m_sde_sample(model, x, _t(2, 3), model_kwargs=kw)
    model._require_guidance()                                                    # (the backward image: checked before the sampler)
    rc = L.vd_dps_step(model._handle, 2, 6, *model._window_ptrs(x, model._pack_kwargs(x, kw)), _lib.ptr(_t(2, 3)), 0, 1, 4, 0.0, _lib.ptr(noise),
                       _lib.ptr(y), 4, 0, 0.5, _lib.ptr(torch.empty_like(x)), None, None, None, _lib.current_stream())
    assert rc != 0 and b"p_sample (0) or ddim_sample (1), got sampler 4" in L.vd_last_error()
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 9
def test_nothing_else_moved():
    """A p_sample, a ddim_sample and a dpmpp_2m_sample step give the same bits before and after a dpmpp_2m_sde step on the same engine."""
    model, diff = tiny()
    c = _rand_window(2, 6, 32, 2, seed=90)
    kw, x = _window_kw(c), c["x"].cuda()
    noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(91)).cuda()
    prev = (torch.rand(x.shape, generator=torch.Generator().manual_seed(92)) * 2 - 1).cuda()
    tt = _t(2, 4)

    def others():
        return [diff._fused_step(0, model, x, tt, True, kw, noise=noise), diff._fused_step(1, model, x, tt, True, kw, eta=0.5, noise=noise),
                diff._fused_step(3, model, x, tt, True, kw, prev_xstart=prev)]

    before = others()
    sde = diff._fused_step(4, model, x, tt, True, kw, noise=noise, prev_xstart=prev)
    WindowExecutor(model, diff).begin(x, kw, sampler="dpmpp_2m_sde", seed=1).run(2)
    after = others()
    for (s0, d0), (s1, d1) in zip(before, after):
        assert torch.equal(s0, s1) and torch.equal(d0, d1)
    assert all(not torch.equal(sde[0], s) for s, _ in before)
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- RePaint
def test_repaint_loop_is_first_order_after_a_jump_and_the_window_walk_equals_the_eager_one():
    from test_gpu_known_region import _flat, _np, _window_region, merged
    from video_diffusion_amd.respace import repaint_schedule
    from video_diffusion_amd.video_sample import infer_video
    model, diff = tiny()
    N = diff.num_timesteps
    c = _rand_window(2, 6, 32, 2, seed=50)
    kw = _window_kw(c)
    src, mask, _ = _window_region(c, seed=51)
    shape = tuple(c["x"].shape)
    sel = torch.from_numpy(merged(_flat(mask)[0], _np(kw["latent_mask"]).reshape(2, 6))).view(shape).cuda()
    x_T = c["x"].cuda()
    torch.manual_seed(53)
    outs = list(diff.repaint_sample_loop_progressive(model, shape, src, mask, sampler="dpmpp_2m_sde", jump_length=2, n_resample=2, noise=x_T,
                                                     model_kwargs=dict(kw)))
    ops = repaint_schedule(N - 1, 2, 2)
    assert [(o["op"], o["t"]) for o in outs] == ops
    assert torch.equal(outs[-1]["sample"][sel], src[sel]) and torch.isfinite(outs[-1]["sample"]).all()
    # the same walk by hand under the same seed: the history is dropped at every jump
    torch.manual_seed(53)
    x, prev = x_T, None
    with diff.known_region_scope(model, src, mask):
        for k, (op, tv) in enumerate(ops):
            if op == "jump":
                x, prev = diff.q_jump(x, _t(2, tv), latent_mask=kw["latent_mask"], model=model), None
            else:
                o = diff.dpmpp_2m_sde_sample(model, x, _t(2, tv), prev_xstart=prev, model_kwargs=kw)
                x, prev = o["sample"], o["pred_xstart"]
            assert torch.equal(x, outs[k]["sample"]), (k, op, tv)
    # WindowExecutor.run_repaint: the eager walk fed the same vd_randn noise
    ex = WindowExecutor(model, diff)
    ex.begin(x_T, kw, sampler="dpmpp_2m_sde", seed=54, known_src=src, known_mask=mask)
    got = ex.run_repaint(jump_length=3, n_resample=2).clone()
    want, _ = _chain(model, diff, x_T, kw, 54, repaint_schedule(N - 1, 3, 2), src, mask)
    assert ex._left == 0 and torch.equal(got, want) and torch.equal(got[sel], src[sel]), float((got - want).abs().max())
    # infer_video with a known region and jumps: the two executors agree to the bit
    g = torch.Generator().manual_seed(60)
    batch = (torch.rand(2, 10, 3, 32, 32, generator=g) * 2 - 1).cuda()
    kmask = (torch.rand(10, 32, 32, generator=g) < 0.5).float()
    out = {}
    for executor in ("eager", "graph"):
        torch.manual_seed(61)
        out[executor] = infer_video("autoreg", model, diff, batch, 6, 2, 4, sampler="dpmpp_2m_sde", executor=executor, known_mask=kmask,
                                    jump_length=2, n_resample=2)[0]
    assert np.array_equal(out["eager"], out["graph"]) and np.isfinite(out["eager"]).all()
    known = (kmask != 0).numpy()[None, :, None].repeat(2, 0).repeat(3, 2)
    assert np.array_equal(out["eager"][:, 2:][known[:, 2:]], batch.cpu().numpy()[:, 2:][known[:, 2:]])
    model.check_device_errors()
