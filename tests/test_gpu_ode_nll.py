"""GPU: the probability-flow ODE likelihood (this project's extension; diffusion.ode_nll_loop, eps_vjp) -- the three kernels per element
against the float64 restatement (tests/ode_nll_restated.py) inside its counted bounds, eps_vjp against autograd through the CPU oracle at the
bars of test_use_gradient_method_vs_oracle_autograd, the Hutchinson trace against the engine's own vjp and the oracle's, the loop of both
orders against the same loop composed in torch on the oracle, every refusal by its message, and the video_nll job.  The model is the DPS
oracle case (B = 2, T = 5, 2 observed, 64 channels, 32 x 32), restated here.  Nothing is tuned on the code under test except the two
chain bars of test_loop_against_the_oracle_loop, which cannot be derived and are 4 x what an MI355X gave (its docstring)."""
import pickle
from argparse import Namespace

import numpy as np
import pytest
import torch

import ode_nll_restated as R
import video_diffusion_amd as vda
from helpers import ATOL, RTOL, close, synth_sd
from step_nll_restated import ratio, tables
from test_gpu_backward import cfg_of, window
from test_gpu_dpmpp_2m import _rand_window, tiny
from test_gpu_dps import _dps_call
from test_gpu_engine import KEYS, _oracle, engine
from test_gpu_known_region import _np, _same_bits
from video_diffusion_amd import _lib

pytestmark = pytest.mark.gpu
ORACLE_CFG = dict(T=8, image_size=32, num_channels=64, num_res_blocks=1, rp_alpha=8, rp_beta=8, rp_gamma=8, timestep_respacing="ddim50")


def _dev(v, misalign=False):
    """A float32 device copy; misalign: at an address 4 bytes off 16."""
    v = torch.as_tensor(v).float()
    if not misalign:
        return v.cuda().contiguous()
    buf = torch.empty(v.numel() + 1, device="cuda")
    out = buf[1:].view(v.shape)
    out.copy_(v)
    assert out.data_ptr() % 16 == 4
    return out


def _offsets(v):
    return torch.tensor(list(v), dtype=torch.int64, device="cuda")


def _rademacher(lat, fe, seed, offsets, probe, misalign=False):
    lat = np.asarray(lat, np.float32)
    B, T = lat.shape
    out, lat_d, off = _dev(np.full((B, T, fe), 7.0, np.float32), misalign), _dev(lat.reshape(-1)), _offsets(offsets)     # (held until the launch)
    _lib.check(_lib.lib().vd_rademacher(_lib.ptr(out), _lib.ptr(lat_d), B, T, fe, seed, _lib.ptr(off), probe, _lib.current_stream()))
    return _np(out)


def _masked_dot(a, b, lat, misalign=False):
    B, T, fe = a.shape
    out = torch.full((B,), 7.0, dtype=torch.float64, device="cuda")
    a_d, b_d, lat_d = _dev(a, misalign), _dev(b, misalign), _dev(np.asarray(lat, np.float32).reshape(-1))
    _lib.check(_lib.lib().vd_op_masked_dot(_lib.ptr(a_d), _lib.ptr(b_d), _lib.ptr(lat_d), B, T, fe, _lib.ptr(out), _lib.current_stream()))
    return _np(out)


# ---------------------------------------------------------------------------------------------------------------- 1 kernels
@pytest.mark.parametrize("fe", [48, 7, 130])
def test_rademacher_per_element(fe):
    """+-1 on latent frames, 0 elsewhere, the documented bit of the documented Philox word; 48: 16-byte stores, 7 and 130: element by
    element (130 crosses a Philox block inside a frame); an item alone and a misaligned output have the same bits."""
    lat = [[1, 0, 1], [0, 1, 1]]
    seed, offs, probe = 2 ** 63 + 11, [5, (1 << 40) + 3], 2
    got = _rademacher(lat, fe, seed, offs, probe)
    for b in range(2):
        want = R.rademacher(seed, offs[b], probe, 3, fe, lat[b])
        assert _same_bits(got[b], want), b
        assert np.isin(got[b][np.asarray(lat[b]) == 1], (-1.0, 1.0)).all() and not got[b][np.asarray(lat[b]) == 0].any()
        alone = _rademacher([lat[b]], fe, seed, [offs[b]], probe)
        assert _same_bits(alone[0], got[b]), b
    assert _same_bits(_rademacher(lat, fe, seed, offs, probe, misalign=True), got)
    assert not _same_bits(_rademacher(lat, fe, seed, offs, probe + 1), got)
    torch.cuda.synchronize()


def test_rademacher_mean_of_a_million():
    """|mean| <= 5 / sqrt(n) at n = 2^20 (five standard deviations of a fair +-1), more than one block and more than one grid stride."""
    n = 1 << 20
    v = _rademacher([[1]], n, 7, [0], 0)
    assert np.isin(v, (-1.0, 1.0)).all() and abs(float(v.mean(dtype=np.float64))) <= 5.0 / np.sqrt(n)


@pytest.mark.parametrize("T,fe", [(1, 1), (1, 3), (1, 4099), (3, 4000), (2, 70000)])
def test_masked_dot_against_float64(T, fe):
    """Per-item element counts 1, 3 and 4099 (ragged: no multiple of four), 12000 (16-byte loads, 12 blocks) and 140000 (the 64-block cap:
    a thread walks more than one group); inside n 2^-53 sum|a b|; a rerun and misaligned inputs (the scalar form) give the same bits."""
    rng = np.random.default_rng(100 + fe)
    B = 3
    a = (rng.standard_normal((B, T, fe)) * np.exp(rng.uniform(-3, 3, (B, T, fe)))).astype(np.float32)
    b = rng.standard_normal((B, T, fe)).astype(np.float32)
    lat = np.ones((B, T), np.float32)
    if T > 1:
        lat[0, 0] = 0
        lat[2, 1] = 0
    m = R.elem_mask(lat, a.shape)
    want, bound = R.masked_dot_fp64(a, b, m)
    got = _masked_dot(a, b, lat)
    r = ratio(got, want, bound)
    print(f"T={T} fe={fe}: max |d| / bound = {r.max():.3f}")
    assert (r <= 1.0).all()
    assert np.array_equal(_masked_dot(a, b, lat), got) and np.array_equal(_masked_dot(a, b, lat, misalign=True), got)
    for i in range(B):                                       # an item alone: the same bits
        assert np.array_equal(_masked_dot(a[i:i + 1], b[i:i + 1], lat[i:i + 1]), got[i:i + 1])
    zero = _masked_dot(a, b, np.zeros((B, T)))
    assert np.array_equal(zero, np.zeros(B)) and not np.signbit(zero).any()


@pytest.mark.parametrize("fe", [192, 7])
def test_heun_pass_against_float64(fe):
    """i = 0, the middle and N - 2 (one item each), a frame that is not latent; 192: 16-byte accesses, 7: element by element."""
    model, diff = tiny()
    diff._bind(model)
    tab = tables(diff)
    N = tab["NT"]
    t = np.array([0, N // 2, N - 2])
    B, T = 3, 3
    rng = np.random.default_rng(fe)
    x, e1, e2 = (rng.standard_normal((B, T, fe)).astype(np.float32) for _ in range(3))
    x *= 3
    lat = np.array([[1, 0, 1], [1, 1, 0], [0, 1, 1]], np.float32)
    m = R.elem_mask(lat, x.shape)
    co = lambda row, d: tab[row][t + d].reshape(B, 1, 1)                      # noqa: E731
    want, bound = R.heun_bound(x, e1, e2, co("sa", 0), co("sa", 1), co("srm1", 0), co("srm1", 1), m)

    def call(misalign=False, t_in=t):
        out = _dev(np.full(x.shape, 7.0, np.float32), misalign)
        x_d, e1_d, e2_d, t_d, lat_d = _dev(x, misalign), _dev(e1, misalign), _dev(e2, misalign), torch.as_tensor(t_in).long().cuda(), _dev(lat.reshape(-1))
        _lib.check(_lib.lib().vd_op_ode_heun(model._handle, B, T, fe, _lib.ptr(x_d), _lib.ptr(e1_d), _lib.ptr(e2_d), _lib.ptr(t_d), _lib.ptr(lat_d),
                                             _lib.ptr(out), _lib.current_stream()))
        return _np(out)
    got = call()
    r = ratio(got, want, bound)
    print(f"fe={fe}: max |d| / bound = {r[m].max():.3f}")
    assert (r <= 1.0).all()
    assert _same_bits(got[~m], x[~m])                                        # frames that are not latent: bit copies
    assert np.abs(got[m] - x[m]).max() > 1e-3
    assert _same_bits(call(misalign=True), got)
    model.check_device_errors()
    bad = call(t_in=np.array([0, N - 1, N - 2]))                              # no next level behind N - 1: the item is NaN, the others keep their bits
    assert np.isnan(bad[1]).all() and _same_bits(bad[[0, 2]], got[[0, 2]])
    with pytest.raises(IndexError):
        model.check_device_errors()
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 2 eps_vjp
def _oracle_case(masks, respacing="ddim50"):
    """The DPS oracle case: B = 2, T = 5, 2 observed, 64 channels, 32 x 32."""
    cfg = {**vda.video_model_and_diffusion_defaults(), **ORACLE_CFG, "timestep_respacing": respacing}
    model, diff, ora = _oracle(cfg)
    c = _rand_window(2, 5, 32, 2, seed=725)
    if masks == "marg_and_padding":                 # frame 2 kinda-marginalised, frame 4 in none of the masks
        c["latent_mask"][:, 2] = 0
        c["kinda_marg_mask"][:, 2] = 1
        c["latent_mask"][:, 4] = 0
    return model, diff, ora, c


def _kw(c):
    kw = {k: v.cuda() for k, v in c.items() if k != "x"}
    return dict(kw, x_t_minus_1=kw["x0"], observed_frames="x_0")


def _oracle_vjp(ora, c, x, ti, cots):
    """eps and [(d eps / d x)^T cot for cot in cots] by torch.autograd through the oracle's network at respaced index ti."""
    kwo = dict(x0=c["x0"], obs_mask=c["obs_mask"], latent_mask=c["latent_mask"], kinda_marg_mask=c["kinda_marg_mask"],
               frame_indices=c["frame_indices"], x_t_minus_1=c["x0"])
    x = x.detach().clone().requires_grad_(True)
    tm = torch.tensor(ora.s.timestep_map, dtype=torch.long)[torch.full((x.shape[0],), ti)]
    with torch.enable_grad():
        eps = ora.net.with_grad(x, tm, **kwo)
        grads = [torch.autograd.grad((eps * cot).sum(), x, retain_graph=True)[0] for cot in cots]
    return eps.detach(), grads


@pytest.mark.parametrize("masks", ["plain", "marg_and_padding"])
def test_eps_vjp_against_oracle_autograd(masks):
    """A Gaussian cotangent at t = 30; the bars are the project's own for this backward pass (test_use_gradient_method_vs_oracle_autograd:
    atol = 2e-4 max|want|, rtol = 1e-3), eps at the step tests' ATOL / RTOL."""
    model, diff, ora, c = _oracle_case(masks)
    cot = torch.randn(c["x"].shape, generator=torch.Generator().manual_seed(41))
    eps_want, (want,) = _oracle_vjp(ora, c, c["x"], 30, [cot])
    out = diff.eps_vjp(model, c["x"].cuda(), torch.tensor([30, 30]).cuda(), cot.cuda(), _kw(c))
    scale = float(want.abs().max())
    err = (out["vjp"].cpu() - want).abs()
    print(f"{masks}: max |vjp - ref| = {float(err.max()):.3e} = {float(err.max()) / scale:.3e} max |ref|; eps {float((out['eps'].cpu() - eps_want).abs().max()):.3e}")
    assert scale > 0 and not out["vjp"][:, :2].any()                          # observed frames are constants: exactly 0
    if masks == "marg_and_padding":
        assert want[:, 4].abs().max() > 0 and not want[:, 2].any()            # padding enters the network, a marginalised frame does not
    close(out["vjp"].cpu(), want, atol=2e-4 * scale, rtol=1e-3)
    close(out["eps"].cpu(), eps_want, atol=ATOL, rtol=RTOL)
    # linear in the cotangent, through the rescaling: 2^-20 cot gives 2^-20 vjp to the bit
    small = diff.eps_vjp(model, c["x"].cuda(), torch.tensor([30, 30]).cuda(), cot.cuda() * 2.0 ** -20, _kw(c))
    assert _same_bits(small["vjp"] * 2.0 ** 20, out["vjp"]) and _same_bits(small["eps"], out["eps"])
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 3 trace
def _eval(diff, model, x, ti, kw, K=1, seed=0, offsets=None, probe0=0, probes=None, want_next=False):
    base, xs, tt, pk = diff._vjp_window(model, x, torch.full((x.shape[0],), ti, dtype=torch.long, device="cuda"), kw)
    off = _offsets(offsets if offsets is not None else [b << 40 for b in range(x.shape[0])])
    return diff._ode_eval(base, xs, tt, pk, K, seed, off, probe0, probes, want_next)


def _probe_tensor(c, seed, offsets, probe0, K):
    lat = c["latent_mask"].reshape(2, 5).numpy()
    return torch.stack([torch.from_numpy(_rademacher(lat, 3 * 32 * 32, seed, offsets, probe0 + k)).view(2, 5, 3, 32, 32) for k in range(K)]).cuda()


@pytest.mark.parametrize("masks", ["plain", "marg_and_padding"])
def test_trace_against_the_vjp_and_the_oracle(masks):
    model, diff, ora, c = _oracle_case(masks)
    kw, x = _kw(c), c["x"].cuda()
    seed, offs = 9, [3, (1 << 40) + 17]
    v = _probe_tensor(c, seed, offs, 4, 1)                                    # the kernel's own probe number 4, as a caller's tensor
    lat = c["latent_mask"].reshape(2, 5).numpy()
    m = R.elem_mask(lat, (2, 5, 3 * 32 * 32))
    eps, tr, _ = _eval(diff, model, x, 30, kw, probes=v)
    # (a) the float64 dot of the probe with the engine's own eps_vjp output, inside the masked-dot bound
    own = diff.eps_vjp(model, x, torch.tensor([30, 30]).cuda(), v[0], kw)
    want, bound = R.masked_dot_fp64(_np(v[0]).reshape(2, 5, -1), _np(own["vjp"]).reshape(2, 5, -1), m)
    r = ratio(_np(tr), want, bound)
    print(f"{masks}: trace {_np(tr)} vs own vjp: max |d| / bound = {r.max():.3f}")
    assert (r <= 1.0).all() and _same_bits(eps, own["eps"])
    # (b) the oracle's v^T J^T v: |d| <= sum_j |v_j| (2e-4 max|g| + 1e-3 |g_j|) from the bars of the vjp test
    _, (g,) = _oracle_vjp(ora, c, c["x"], 30, [v[0].cpu()])
    gn, vn = g.numpy().reshape(2, 5, -1).astype(np.float64), _np(v[0]).reshape(2, 5, -1).astype(np.float64)
    ref = np.where(m, vn * gn, 0.0).reshape(2, -1).sum(axis=1)
    lim = np.where(m, np.abs(vn) * (2e-4 * np.abs(gn).max() + 1e-3 * np.abs(gn)), 0.0).reshape(2, -1).sum(axis=1)
    print(f"  vs oracle: {ref}, |d| / bound = {np.abs(_np(tr) - ref) / lim}")
    assert (np.abs(_np(tr) - ref) <= lim).all() and (np.abs(ref) > 0).all()
    # (c) the built-in probe at (seed, offsets, 4): the same bits
    eps_b, tr_b, _ = _eval(diff, model, x, 30, kw, seed=seed, offsets=offs, probe0=4)
    assert np.array_equal(_np(tr_b), _np(tr)) and _same_bits(eps_b, eps)
    # (d) K = 3 is the float64 mean of three K = 1 calls at consecutive probe numbers, inside 3 ulp (the tape serves all three)
    _, tr3, _ = _eval(diff, model, x, 30, kw, K=3, seed=seed, offsets=offs, probe0=4)
    ones = [_np(_eval(diff, model, x, 30, kw, seed=seed, offsets=offs, probe0=4 + k)[1]) for k in range(3)]
    mean = (ones[0] + ones[1] + ones[2]) / 3.0
    assert (np.abs(_np(tr3) - mean) <= 3 * np.spacing(np.abs(mean))).all() and not np.array_equal(ones[0], ones[1])
    # and with caller's probes, K = 3, an item alone has the batch's bits
    v3 = _probe_tensor(c, seed, offs, 4, 3)
    assert np.array_equal(_np(_eval(diff, model, x, 30, kw, K=3, probes=v3)[1]), _np(tr3))
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 4 loop
# 4 x the worst |difference| to the oracle's loop measured on an MI355X (order 1: x_T 9.350e-06, logp 8.288e-03 of -3.99e4; order 2: x_T 8.822e-06,
# logp 9.868e-04 of -4.06e4 -- 2e-7 and 2e-8 of the value, 1e-9 bits/dim)
X_T_BAR = {1: 4 * 9.350e-06, 2: 4 * 8.822e-06}
LOGP_BAR = {1: 4 * 8.288e-03, 2: 4 * 9.868e-04}


def _oracle_loop(ora, c, x0, probes, order):
    """ode_nll_loop composed in torch on the oracle: float32 network and autograd, the chain and the sums in float64."""
    acp = np.asarray(ora.s.alphas_cumprod, np.float64)
    lat = c["latent_mask"].reshape(2, 5).numpy()
    m = torch.from_numpy(np.ascontiguousarray(R.elem_mask(lat, tuple(x0.shape))))

    def point(x, i, e):
        eps, (g,) = _oracle_vjp(ora, c, x.float(), i, [probes[e, 0].cpu()])
        tr = torch.where(m, probes[e, 0].cpu().double() * g.double(), torch.zeros((), dtype=torch.float64)).reshape(2, -1).sum(dim=1)
        return eps.double().numpy(), tr.numpy()
    calls = []

    def eps_fn(x, i):
        calls.append(point(torch.from_numpy(x), i, len(calls)))
        return calls[-1][0]
    trace_fn = lambda x, i: calls[-1][1]                                     # noqa: E731
    return R.ode_nll_fp64(eps_fn, trace_fn, x0.double().numpy(), lat, acp, order)


@pytest.mark.parametrize("order", [1, 2])
def test_loop_against_the_oracle_loop(order):
    """ddim5 (4 steps) with fixed probes against the same loop on the oracle (eight forward + backward passes at order 2).  x_T and logp
    cannot be bounded from first principles through a chain that amplifies the network's 2e-6 per step: the bars are 4 x the worst
    |difference| an MI355X gave: max |x_T - oracle| 9.35e-6 (order 1) and 8.82e-6 (order 2), max |logp - oracle| 8.29e-3 and 9.87e-4 on
    logp = -4.0e4 (X_T_BAR / LOGP_BAR); box-to-box variation of clocks does not change arithmetic.  delta_logp is the float64 sum of the weights times the returned
    traces (rtol 1e-12); order 1's x_T is ddim_reverse_sample_loop(clip_denoised=False, t_end=N-2) on the latent frames within that loop
    test's bar (1e-2 at the chain's end; not bit-equal: the taped forward folds GroupNorm differently)."""
    model, diff, ora, c = _oracle_case("plain", respacing="ddim5")
    N = diff.num_timesteps
    assert N == 5
    x0 = torch.rand(c["x"].shape, generator=torch.Generator().manual_seed(77)) * 2 - 1
    lat = c["latent_mask"].reshape(2, 5).numpy()
    probes = torch.stack([torch.from_numpy(_rademacher(lat, 3 * 32 * 32, 21, [0, 1 << 40], e)).view(1, 2, 5, 3, 32, 32) for e in range((N - 1) * order)]).cuda()
    out = diff.ode_nll_loop(model, x0.cuda(), model_kwargs=_kw(c), order=order, probes=probes)
    assert set(out) == {"total_bpd", "logp", "prior_logp", "delta_logp", "trace", "x_T"} | ({"trace_corr"} if order == 2 else set())
    assert out["trace"].shape == (2, N - 1) and out["logp"].dtype == torch.float64 and out["x_T"].dtype == torch.float32
    w, wc = diff.ode_nll_weights(order)
    delta = (_np(out["trace"]) * w).sum(axis=1) + ((_np(out["trace_corr"]) * wc).sum(axis=1) if order == 2 else 0.0)
    np.testing.assert_allclose(_np(out["delta_logp"]), delta, rtol=1e-12, atol=0)
    m = R.elem_mask(lat, tuple(x0.shape))
    logp, bpd, prior, D = R.totals(_np(out["x_T"]).astype(np.float64), m, delta, R.terms(diff.alphas_cumprod)["const"])
    np.testing.assert_allclose(_np(out["logp"]), logp, rtol=1e-12, atol=0)
    np.testing.assert_allclose(_np(out["total_bpd"]), bpd, rtol=1e-12, atol=0)
    assert _same_bits(_np(out["x_T"])[~m], x0.numpy()[~m])                    # observed frames do not move
    want = _oracle_loop(ora, c, x0, probes, order)
    dx = float(np.abs(_np(out["x_T"]) - want["x_T"]).max())
    dl = float(np.abs(_np(out["logp"]) - want["logp"]).max())
    print(f"order {order}: MEASURED max |x_T - oracle| = {dx:.3e}, max |logp - oracle| = {dl:.3e} (logp {_np(out['logp'])}, bpd {_np(out['total_bpd'])}, "
          f"oracle bpd {want['bpd']})")
    assert dx <= X_T_BAR[order] and dl <= LOGP_BAR[order]
    if order == 1:
        enc = diff.ddim_reverse_sample_loop(model, x0.cuda(), clip_denoised=False, model_kwargs=_kw(c), t_end=N - 2)
        close(torch.from_numpy(_np(out["x_T"])[m]), _np(enc)[m], atol=1e-2, rtol=1e-2)
    # the built-in probes are vd_rademacher's at (seed, item_offset[b], e K + k): the same loop on those tensors has the same bits
    offs = [7, (1 << 40) + 2]
    built = diff.ode_nll_loop(model, x0.cuda(), model_kwargs=_kw(c), order=order, n_probes=2, seed=5, item_offset=offs)
    handed = torch.stack([torch.stack([torch.from_numpy(_rademacher(lat, 3 * 32 * 32, 5, offs, e * 2 + k)).view(2, 5, 3, 32, 32) for k in range(2)])
                          for e in range((N - 1) * order)]).cuda()
    same = diff.ode_nll_loop(model, x0.cuda(), model_kwargs=_kw(c), order=order, n_probes=2, probes=handed)
    assert all(np.array_equal(_np(built[k]), _np(same[k])) for k in built) and not np.array_equal(_np(built["trace"]), _np(out["trace"]))
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 5 refusals
def test_every_refusal_by_its_message():
    model, diff, ora, c = _oracle_case("plain")
    kw, x = _kw(c), c["x"].cuda()
    t = torch.tensor([30, 30]).cuda()
    L = _lib.lib()

    def both(match, exc=_lib.VdError, **over):
        k2 = dict(kw, **over)
        with pytest.raises(exc, match=match):
            diff.eps_vjp(model, x, t, x, k2)
        with pytest.raises(exc, match=match):
            diff.ode_nll_loop(model, x, model_kwargs=k2)
    both("observed_frames must be x_0", observed_frames="x_t")
    with diff.cfg_scale_scope(model, 2.0):
        both(r"together with cfg_scale != 1")
    with diff.guidance_scope(model, cfg_rescale=0.5):
        both("together with guidance_rescale")
    with diff.guidance_scope(model, dynamic_threshold=0.9):
        both("together with dynamic_threshold")
    with diff.known_region_scope(model, x, torch.ones(2, 5, 1, 32, 32, device="cuda")):
        both("inside known_region_scope is not served", exc=NotImplementedError)
    y = vda.gaussian_diffusion.measure(c["x"], 4, False)
    with diff.dps_scope(model, y, 4, zeta=0.5):
        both("inside dps_scope is not served")
    ones = torch.ones(2, 5, 32, 32, device="cuda")
    _lib.check(L.vd_set_known_region(model._handle, _lib.ptr(x), _lib.ptr(ones), None, 0, 0))
    try:
        both("together with a known region")                                  # the engine's own state, set as a step sets it
    finally:
        _lib.check(L.vd_set_known_region(model._handle, None, None, None, 0, 0))
    with diff.measurement_scope(model, y, 4):
        both("together with a measurement")
    model._attn_capture(2, 5)
    try:
        both("together with return_attn_weights")
    finally:
        model._attn_release()
    with pytest.raises(ValueError, match="the clamp has no density"):
        diff.ode_nll_loop(model, x, model_kwargs=kw, clip_denoised=True)
    # the entry itself: n_probes, and a null probe source
    base, xs, tt, pk = diff._vjp_window(model, x, t, kw)
    for K in (0, 65):
        with pytest.raises(_lib.VdError, match="n_probes must be 1..64"):
            diff._ode_eval(base, xs, tt, pk, K, 0, _offsets([0, 1]), 0, None, False)
    # 33 frames, a START_X model, learn_sigma and a backward image that is not on the device: engines of their own
    cfg = {**vda.video_model_and_diffusion_defaults(), **dict(T=33, image_size=32, num_channels=32, num_res_blocks=1, rp_alpha=4, rp_beta=4, rp_gamma=4,
                                                              timestep_respacing="ddim5")}
    m33, d33 = engine(cfg)
    w = _rand_window(1, 33, 32, 2, seed=1)
    for name, call in (("eps_vjp", lambda: d33.eps_vjp(m33, w["x"].cuda(), torch.tensor([1]).cuda(), w["x"].cuda(), _kw(w))),
                       ("ode_nll", lambda: d33.ode_nll_loop(m33, w["x"].cuda(), model_kwargs=_kw(w)))):
        with pytest.raises(_lib.VdError, match=f"{name}: windows of at most 32 frames .*got 33"):
            call()
    small = dict(T=4, image_size=32, num_channels=32, num_res_blocks=1, rp_alpha=4, rp_beta=4, rp_gamma=4, timestep_respacing="ddim5")
    w = _rand_window(1, 4, 32, 2, seed=2)
    mx, dx = engine({**vda.video_model_and_diffusion_defaults(), **small, "predict_xstart": True})
    with pytest.raises(_lib.VdError, match="ode_nll: epsilon-prediction models only"):
        dx.ode_nll_loop(mx, w["x"].cuda(), model_kwargs=_kw(w))
    with pytest.raises(_lib.VdError, match="eps_vjp: epsilon-prediction models only"):
        dx.eps_vjp(mx, w["x"].cuda(), torch.tensor([1]).cuda(), w["x"].cuda(), _kw(w))
    # learn_sigma and a backward image that is not on the device: the entries themselves (no tensor is read before the refusal)
    def raw(m, name):
        held = (w["x"].cuda(), torch.tensor([1]).cuda(), torch.zeros(1, 4, dtype=torch.long).cuda())
        p, tt, fi = (_lib.ptr(v) for v in held)
        if name == "vd_eps_vjp":
            return L.vd_eps_vjp(m._handle, 1, 4, p, p, p, p, p, fi, tt, 0, p, None, p, None)
        return L.vd_ode_nll_eval(m._handle, 1, 4, p, p, p, p, p, fi, tt, 0, 1, 0, fi, 0, None, None, fi, None, None)
    ml, dl = engine({**vda.video_model_and_diffusion_defaults(), **small, "learn_sigma": True})
    dl._bind(ml)
    fresh, df = vda.create_video_model_and_diffusion(**{k: {**vda.video_model_and_diffusion_defaults(), **small}[k] for k in KEYS})
    fresh.load_state_dict(synth_sd(fresh.param_specs()))
    fresh.to("cuda").eval()
    df._bind(fresh)
    for name, what in (("vd_eps_vjp", b"eps_vjp"), ("vd_ode_nll_eval", b"ode_nll")):
        assert raw(ml, name) != 0 and what + b": learn_sigma is not served" in L.vd_last_error()
        assert raw(fresh, name) != 0 and what + b": the backward-data weight image is not on the device" in L.vd_last_error()
    # a plain step afterwards still works, with the bits it had before
    torch.manual_seed(3)
    a = diff.p_sample(model, x, t, model_kwargs=kw)["sample"]
    diff.eps_vjp(model, x, t, x, kw)
    torch.manual_seed(3)
    b = diff.p_sample(model, x, t, model_kwargs=kw)["sample"]
    assert _same_bits(a, b) and torch.isfinite(a).all()
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 6 workspace
def test_results_do_not_depend_on_where_the_workspace_tail_lies():
    """The four differentiated entries (use_gradient_method, dps, eps_vjp, ode_nll) keep their own buffers at the END of the engine's
    workspace.  On one engine of its own (cfg_of(12): 32 x 32, 64 channels): each entry on a window of B = 2, T = 4 (one observed frame,
    frame 3 of item 1 padding), then eps_vjp at B = 2, T = 12, which grows the workspace and so moves that end, then the four small calls
    again: every output has the bits it had.  The kernels use no floating-point atomics, so nothing but an address may differ.  A plain
    p_sample behind all of it has the bits it had on the engine while it was fresh."""
    cfg = cfg_of(12)
    model, diff = vda.create_video_model_and_diffusion(**{k: cfg[k] for k in KEYS})
    model.load_state_dict(synth_sd(model.param_specs()))
    model.to("cuda").eval()

    def case(T, pad, seed):
        c = window(2, T, 32, 1, seed=seed, pad=pad)
        kw = {k: v.cuda() for k, v in c.items() if k != "x"}
        return c["x"].cuda(), dict(kw, x_t_minus_1=kw["x0"], observed_frames="x_0")
    x, kw = case(4, [[], [3]], 404)
    big_x, big_kw = case(12, [[], [11]], 412)
    g = torch.Generator().manual_seed(405)
    n1, n2, cot = (torch.randn(x.shape, generator=g).cuda() for _ in range(3))
    y = vda.gaussian_diffusion.measure(torch.rand(tuple(x.shape), generator=g) * 2 - 1, 4, False)
    t = torch.tensor([30, 30]).cuda()

    def small_calls():
        out = {}
        guided = diff._guided(model, x, t, True, kw, noise2=n2, want_sample=True, _noise=n1)
        out.update({f"guided.{k}": guided[k] for k in ("mean", "pred_xstart", "grad", "sample")})
        dps = _dps_call(diff, model, 0, x, t, kw, 0.0, n1, y, 4, False, 0.5)
        out.update({f"dps.{k}": dps[k] for k in ("sample", "pred_xstart", "grad", "residual_norm")})
        vjp = diff.eps_vjp(model, x, t, cot, kw)
        out.update({f"eps_vjp.{k}": vjp[k] for k in ("eps", "vjp")})
        out.update(zip(("ode_nll.eps", "ode_nll.trace", "ode_nll.x_next"),
                       _eval(diff, model, x, 30, kw, K=2, seed=9, offsets=[3, (1 << 40) + 17], want_next=True)))
        return {k: _np(v) for k, v in out.items()}
    torch.manual_seed(3)
    plain = _np(diff.p_sample(model, x, t, model_kwargs=kw)["sample"])          # the engine is fresh: no differentiated pass has run on it
    before = small_calls()
    assert len(before) == 13 and all(np.isfinite(v).all() for v in before.values())
    assert np.abs(before["guided.grad"]).max() > 0 and np.abs(before["dps.grad"]).max() > 0 and np.abs(before["eps_vjp.vjp"]).max() > 0
    assert torch.isfinite(diff.eps_vjp(model, big_x, t, torch.ones_like(big_x), big_kw)["vjp"]).all()
    after = small_calls()
    for k, v in before.items():
        assert _same_bits(after[k], v), k
    torch.manual_seed(3)
    assert _same_bits(_np(diff.p_sample(model, x, t, model_kwargs=kw)["sample"]), plain)
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 7 job
def test_job_writes_what_the_loop_returns(tmp_path, monkeypatch):
    """video_nll --method ode on two synthetic videos from a checkpoint file: the pickles hold what run_ode_evaluation returns for the item's
    own Philox range, a second run skips finished videos, and --method elbo writes what it wrote before the flag existed."""
    from video_diffusion_amd import video_nll
    cfg = {**vda.video_model_and_diffusion_defaults(), **dict(T=4, image_size=32, num_channels=32, num_res_blocks=1, rp_alpha=4, rp_beta=4, rp_gamma=4,
                                                              timestep_respacing="ddim5")}
    model, diff = engine(cfg)
    ck = tmp_path / "checkpoints" / "e" / "ema_50.pt"
    ck.parent.mkdir(parents=True)
    torch.save({"state_dict": synth_sd(model.param_specs()), "config": {**cfg, "max_frames": 4}, "step": 50}, ck)
    vids = (torch.randint(0, 256, (2, 6, 3, 32, 32), generator=torch.Generator().manual_seed(3)).float() / 127.5 - 1)
    np.save(tmp_path / "v.npy", vids.numpy())
    monkeypatch.chdir(tmp_path)
    base = dict(checkpoint_path=str(ck), videos=str(tmp_path / "v.npy"), synthetic=False, inference_mode="autoreg", T=None, max_frames=None,
                obs_length=2, step_size=2, batch_size=2, num_videos=0, timestep_respacing="ddim5", use_ddim=False, eval_dir=None, seed=11,
                image_size=32, num_channels=32, num_res_blocks=1, indices=None, task_id=None, indices_path=None, clip_denoised=True, optimality=None)
    torch.manual_seed(11)
    before = video_nll.run(Namespace(**base), device=torch.device("cuda", 0))                    # no `method` attribute: the job as it was
    elbo_files = sorted((tmp_path / before / "elbos").glob("*.pkl"))
    elbo_before = [open(p, "rb").read() for p in elbo_files]
    out = video_nll.run(Namespace(**base, method="ode", ode_order=2, ode_probes=2, ode_seed=5, no_dequantize=False), device=torch.device("cuda", 0))
    assert out == before
    windows = [([0, 1], [2, 3]), ([2, 3], [4, 5])]
    want = [video_nll.run_ode_evaluation(model, diff, vids, [o] * 2, [l] * 2, order=2, n_probes=2, seed=5,
                                         item_offset=[(i * 2 + wi) << 40 for i in range(2)]) for wi, (o, l) in enumerate(windows)]
    names = [tmp_path / out / "ode_nll" / f"ode_{i}_order2_k2_seed5_respaceddim5.pkl" for i in range(2)]
    for i, p in enumerate(names):
        rec = pickle.load(open(p, "rb"))
        assert set(rec) == {"total_bpd", "logp", "prior_logp", "delta_logp", "trace", "trace_corr"}
        for k, v in rec.items():
            assert v.shape == (2,) and np.array_equal(v, np.stack([w[k][i] for w in want])), (i, k)
        assert np.isfinite(rec["total_bpd"]).all()
    # dequantisation moved the latent frames by less than one bin and left the observed ones alone; without it the numbers differ
    plain = video_nll.run_ode_evaluation(model, diff, vids, [[0, 1]] * 2, [[2, 3]] * 2, order=2, n_probes=2, seed=5, dequantize=False)
    assert not np.array_equal(plain["logp"], want[0]["logp"])
    x0 = vids[:, :4].cuda().contiguous()
    deq = torch.empty_like(x0)
    lat = torch.tensor([0, 0, 1, 1] * 2, dtype=torch.float32, device="cuda")
    off = _offsets([0 + video_nll.ODE_DEQUANT_OFFSET, (1 << 40) + video_nll.ODE_DEQUANT_OFFSET])
    _lib.check(_lib.lib().vd_dequantize(_lib.ptr(x0), _lib.ptr(lat), 2, 4, 3 * 32 * 32, 5, _lib.ptr(off), _lib.ptr(deq), _lib.current_stream()))
    d = _np(deq - x0)
    assert not d[:, :2].any() and (d[:, 2:] >= 0).all() and (d[:, 2:] < 2 / 256 + 1e-7).all() and abs(d[:, 2:].mean() - 1 / 256) < 1e-4
    # a second run skips the finished videos: the files are not written again
    stamp = [p.stat().st_mtime_ns for p in names]
    video_nll.run(Namespace(**base, method="ode", ode_order=2, ode_probes=2, ode_seed=5, no_dequantize=False), device=torch.device("cuda", 0))
    assert [p.stat().st_mtime_ns for p in names] == stamp
    # --method elbo: byte for byte what the job wrote without the flag, under the same seed
    for p in elbo_files:
        p.unlink()
    torch.manual_seed(11)
    video_nll.run(Namespace(**base, method="elbo"), device=torch.device("cuda", 0))
    assert [open(p, "rb").read() for p in elbo_files] == elbo_before
    model.check_device_errors()
