"""GPU: unipc_sample (this project's extension: UniPC, data prediction, multistep order 2, bh2) -- the fused pass per element, its third
order on the device, the step on the network, its loops, its window graph, infer_video and the scopes -- against the float64 restatement
of the pass (tests/unipc_restated.py; the reference has no such sampler, so there is no fixture) and against itself (executor vs eager
calls).  Every bound is derived in unipc_restated.py, none is measured."""
import numpy as np
import pytest
import torch

from dpmpp_2m_restated import denoiser_coef, rel_err, start
from helpers import ATOL, RTOL, close
from test_gpu_dpmpp_2m import _denoised_fn, _rand_window, _t, _window_kw, tiny
from unipc_restated import coefficients, order_conditions, rounding_bound, step_fp64
from video_diffusion_amd import _lib
from video_diffusion_amd.executor import WindowExecutor
from video_diffusion_amd.script_util import create_gaussian_diffusion

pytestmark = pytest.mark.gpu
PER = 1152                                          # the pass alone: items of 1152 floats, 288 groups of four each


def _pass(model, x, d_in, state, count, t, clip, inplace=False, sample=None, want_xstart=True):
    """vd_unipc_from_xstart on (B, per) tensors -> (sample, D_t, state written).  state: (base, D1, D2) or None; inplace: the state
    written is the state read (clones of the caller's, which stay as they are)."""
    sample = torch.empty_like(x) if sample is None else sample
    xstart = torch.empty_like(x) if want_xstart else None
    ins = (None, None, None) if state is None else tuple(state)
    if inplace:
        ins = outs = tuple(v.clone() for v in state)
    else:
        outs = tuple(torch.empty_like(x) for _ in range(3))
    _lib.check(_lib.lib().vd_unipc_from_xstart(model._handle, x.shape[0], x[0].numel(), _lib.ptr(x), _lib.ptr(d_in), *(_lib.ptr(v) for v in ins),
                                               count, _lib.ptr(t), clip, _lib.ptr(sample), _lib.ptr(xstart), *(_lib.ptr(v) for v in outs),
                                               _lib.current_stream()))
    return sample, xstart, outs


def _check(diff, ts, count, x, d_t, state, xc, sample, tag):
    """x^c and the sample against the float64 restatement fed the step's own float32 x~, D_t and state, per element inside the derived
    bound; ts: one index per item.  Returns the worst |d| / bound."""
    tab = diff._unipc_rows().astype(np.float32)                                  # the float32 casts the engine is handed
    flat = lambda v: None if v is None else v.detach().cpu().numpy().reshape(len(ts), -1)  # noqa: E731
    xn, dn, cn, sn = flat(x), flat(d_t), flat(xc), flat(sample)
    st = (None, None, None) if state is None else tuple(flat(v) for v in state[:3])
    worst = 0.0
    for b, tv in enumerate(ts):
        n, c, p = coefficients(tab, tv, count)
        args = (xn[b], dn[b], *(None if v is None else v[b] for v in st), n, c, p)
        want_c, want_s = step_fp64(*args)
        lim_c, lim_s = rounding_bound(*args)
        if n == 0:
            assert np.array_equal(cn[b], xn[b]), (tag, b, tv)                    # no corrector: x^c is x~ itself
        err_c, err_s = np.abs(cn[b] - want_c), np.abs(sn[b] - want_s)
        ratio = max(float((err_c / np.maximum(lim_c, 1e-300)).max()) if n else 0.0, float((err_s / np.maximum(lim_s, 1e-300)).max()))
        worst = max(worst, ratio)
        assert (err_c <= lim_c).all() and (err_s <= lim_s).all(), (tag, b, tv, n, ratio)
    print(f"{tag}: max |d| / bound = {worst:.3f}")
    return worst


def _inputs(B, per, seed, offset=False):
    """x~, the x_0 handed in (about a fifth beyond +-1: the clamp matters) and a state; offset: every tensor 4 bytes off 16-byte alignment."""
    g = torch.Generator().manual_seed(seed)

    def dev(v):
        if not offset:
            return v.cuda()
        buf = torch.empty(B * per + 1, device="cuda")[1:].view(B, per)
        buf.copy_(v)
        assert buf.data_ptr() % 16 == 4
        return buf
    x = dev(1.5 * torch.randn(B, per, generator=g))
    d_in = dev(0.8 * torch.randn(B, per, generator=g))
    state = tuple(dev(v) for v in (1.5 * torch.randn(B, per, generator=g), torch.rand(B, per, generator=g) * 2 - 1, torch.rand(B, per, generator=g) * 2 - 1))
    return x, d_in, state


# ---------------------------------------------------------------------------------------------------------------- 1
def test_the_pass_per_element_against_float64():
    """The pass alone (vd_unipc_from_xstart), x^c and the sample per element inside unipc_restated.rounding_bound -- 4 roundings into x^c,
    3 more into the sample, 7 on the longest path, each 2^-24 of the sum of the terms' magnitudes: B = 5 with t = (N-1, N-2, N-3, 1, 0)
    per item; count 0, 1, 2 and 5; clip on and off; state out of place and in place; per = 1152 (16-byte accesses) and per = 77 with
    every tensor 4 bytes off alignment (element by element); sample aliasing x; pred_xstart NULL; the grid-stride loop's second trip;
    an item whose t is out of range (all its outputs NaN, the state included, its neighbours' bits untouched, no flag); a non-finite
    x_0 (NaN, bit 1).  Measured on an MI355X: worst |d| / bound 0.889 over all cases (the second-trip case, 4.2 M elements), 0.739 at
    per = 1152, 0.560 at per = 77; the element-by-element form gave the 16-byte form's bits."""
    model, diff = tiny()
    diff._bind(model)
    N = diff.num_timesteps
    ts = [N - 1, N - 2, N - 3, 1, 0]
    tt = torch.tensor(ts, device="cuda")
    worst = 0.0
    for per, offset in ((PER, False), (77, True)):
        x, d_in, state = _inputs(5, per, seed=per, offset=offset)
        for count in (0, 1, 2, 5):
            for clip in (1, 0):
                st = state if count else None
                sample, d_t, outs = _pass(model, x, d_in, st, count, tt, clip)
                assert torch.equal(d_t, d_in.clamp(-1, 1) if clip else d_in)     # D_t: the x_0 handed in, clamped
                assert torch.equal(outs[1], d_t)                                 # the state's D1 is D_t
                for b, tv in enumerate(ts):                                      # ... and its D2 the D1 read, where the order reaches it
                    n = min(count, N - 1 - tv)
                    assert torch.equal(outs[2][b], state[1][b] if n >= 1 else torch.zeros_like(x[b])), (count, tv)
                worst = max(worst, _check(diff, ts, count, x, d_t, st, outs[0], sample, f"per={per} count={count} clip={clip}"))
                assert torch.equal(sample[4], d_t[4])                            # t = 0: the sample is D_0
                if count:                                                        # the state in place (what the window graph does): same bits
                    s2, d2, outs2 = _pass(model, x, d_in, state, count, tt, clip, inplace=True)
                    assert torch.equal(s2, sample) and torch.equal(d2, d_t) and all(torch.equal(a, b) for a, b in zip(outs, outs2))
        # a count without a state counts nothing: with state pointers but count = 0 the state is not read either
        s0, _, o0 = _pass(model, x, d_in, None, 0, tt, 1)
        s1, _, o1 = _pass(model, x, d_in, state, 0, tt, 1)
        assert torch.equal(s0, s1) and all(torch.equal(a, b) for a, b in zip(o0, o1))
        # the orders differ where the schedule has room for them (item 3: t = 1), and agree where it has none (item 0: t = N - 1)
        by_count = [_pass(model, x, d_in, state, c, tt, 1)[0] for c in (0, 1, 2)]
        assert not torch.equal(by_count[0][3], by_count[1][3]) and not torch.equal(by_count[1][3], by_count[2][3])
        assert torch.equal(by_count[0][0], by_count[2][0]) and torch.equal(by_count[1][1], by_count[2][1])
        # the sample written over x, and pred_xstart NULL: the same sample
        want_s, want_d, want_o = _pass(model, x, d_in, state, 2, tt, 1)
        xa = x.clone()
        got_s, _, _ = _pass(model, xa, d_in, state, 2, tt, 1, sample=xa)
        assert torch.equal(xa, want_s) and got_s is xa
        assert torch.equal(_pass(model, x, d_in, state, 2, tt, 1, want_xstart=False)[0], want_s)
        # an out-of-range t poisons its item, state included, and nothing else; the network-free entry raises no flag
        for bad in (N, -1):
            s, d, o = _pass(model, x, d_in, state, 2, torch.tensor([N - 1, N - 2, bad, 1, 0], device="cuda"), 1)
            assert all(torch.isnan(v[2]).all() for v in (s, d, *o))
            for b in (0, 1, 3, 4):
                assert all(torch.equal(v[b], w[b]) for v, w in zip((s, d, *o), (want_s, want_d, *want_o))), (bad, b)
        model.check_device_errors()
        # a non-finite x_0 (NaN, and an infinity, which leaves as NaN too) sets the sticky bit and touches no other element
        bad_in = d_in.clone()
        bad_in[1, 7], bad_in[3, 9] = float("nan"), float("inf")
        s, d, o = _pass(model, x, bad_in, state, 2, tt, 1)
        for v in (s, d, o[0], o[1]):
            assert torch.isnan(v[1, 7]) and torch.isnan(v[3, 9]) and torch.isfinite(v).sum() == v.numel() - 2
        with pytest.raises(FloatingPointError):
            model.check_device_errors()
        model.check_device_errors()
    # the two forms give the same values: the aligned tensors' bits from the element-by-element form (x alone 4 bytes off)
    x, d_in, state = _inputs(5, PER, seed=PER)
    want_s, _, want_o = _pass(model, x, d_in, state, 2, tt, 1)
    off = torch.empty(5 * PER + 1, device="cuda")[1:].view(5, PER)
    off.copy_(x)
    un_s, _, un_o = _pass(model, off, d_in, state, 2, tt, 1)
    assert torch.equal(un_s, want_s) and torch.equal(un_o[0], want_o[0])
    # just above 4096 blocks of 256 groups of four: the loop's second trip
    per = 4 * (4096 * 256 // 2 + 1)
    x, d_in, state = _inputs(2, per, seed=8)
    assert 2 * per // 4 > 4096 * 256
    sample, d_t, outs = _pass(model, x, d_in, state, 2, torch.tensor([3, 6], device="cuda"), 1)
    worst = max(worst, _check(diff, [3, 6], 2, x, d_t, state, outs[0], sample, f"per={per} (second trip)"))
    print(f"worst |d| / bound over all cases = {worst:.3f}")
    model.check_device_errors()


def test_missing_rows_fail_by_name():
    model, diff = tiny(timestep_respacing="logsnr5")
    diff._bind(model)
    L = _lib.lib()
    x = torch.randn(2, PER).cuda()
    tab = diff._device_tables()
    tm = np.ascontiguousarray(np.array(diff.timestep_map, dtype=np.int32))
    try:
        _lib.check(L.vd_set_schedule(model._handle, diff.num_timesteps, _lib.ptr(tab), _lib.ptr(tm), 1.0))     # drops the rows
        with pytest.raises(_lib.VdError, match="unipc_sample: no coefficient rows.*vd_set_unipc_rows"):
            _pass(model, x, x, None, 0, _t(2, 2), 1)
        c = _rand_window(2, 6, 32, 2, seed=3)
        model._bound_schedule = diff                                             # keep the step from re-binding: the rows stay dropped
        with pytest.raises(_lib.VdError, match="unipc_sample: no coefficient rows"):
            diff.unipc_sample(model, c["x"].cuda(), _t(2, 2), model_kwargs=_window_kw(c))
        with pytest.raises(_lib.VdError, match=r"sampler 5 \(unipc_sample\): no coefficient rows"):
            WindowExecutor(model, diff).begin(c["x"].cuda(), _window_kw(c), sampler="unipc")
        rows = np.ascontiguousarray(diff._unipc_rows().astype(np.float32))
        assert L.vd_set_unipc_rows(model._handle, diff.num_timesteps + 1, _lib.ptr(rows)) != 0 and b"bound schedule" in L.vd_last_error()
    finally:
        model._bound_schedule = None
    diff._bind(model)
    _pass(model, x, x, None, 0, _t(2, 2), 1)
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 2
def _device_chain(model, diff, s, x0, sampler):
    """The analytic model's chain on the device, D computed in torch: 'unipc' through vd_unipc_from_xstart with the state in place,
    'dpmpp_2m' through vd_dpmpp_2m_from_xstart."""
    L = _lib.lib()
    coef = [float(np.float32(denoiser_coef(s, a))) for a in diff.alphas_cumprod]
    x, B = x0.clone(), x0.shape[0]
    state, prev = tuple(torch.zeros_like(x) for _ in range(3)), None
    for count, tv in enumerate(range(diff.num_timesteps - 1, -1, -1)):
        d, nxt = x * coef[tv], torch.empty_like(x)
        if sampler == "unipc":
            _lib.check(L.vd_unipc_from_xstart(model._handle, B, PER, _lib.ptr(x), _lib.ptr(d), *(_lib.ptr(v) for v in state), count, _lib.ptr(_t(B, tv)),
                                              0, _lib.ptr(nxt), None, *(_lib.ptr(v) for v in state), _lib.current_stream()))
        else:
            cur = torch.empty_like(x)
            _lib.check(L.vd_dpmpp_2m_from_xstart(model._handle, B, PER, _lib.ptr(x), _lib.ptr(d), _lib.ptr(prev), _lib.ptr(_t(B, tv)), 0,
                                                 _lib.ptr(nxt), _lib.ptr(cur), _lib.current_stream()))
            prev = cur
        x = nxt
    return x


@pytest.mark.parametrize("s", [0.5, 1.0])
def test_third_order_on_the_device(s):
    """The analytic model's chain through vd_unipc_from_xstart (and dpmpp_2m's through vd_dpmpp_2m_from_xstart): the four conditions of
    the CPU restatement hold for the device results.  Measured on an MI355X for s = 0.5 / 1.0: E_U(20) / E_U(40) = 8.92 / 7.98,
    E_2M(40) / E_U(40) = 3.38 / 3.14, E_2M(20) / E_U(20) = 1.54 / 1.54, E_U(10) / E_2M(10) = 1.60 / 1.38; E_U(40) = 1.062e-3 / 1.182e-3,
    the float32 numpy chain's figures."""
    model, _ = tiny()
    eu, e2m = {}, {}
    try:
        for n in (10, 20, 40):
            diff = create_gaussian_diffusion(timestep_respacing=f"logsnr{n}")
            diff._bind(model)
            x, exact = start(s, diff.alphas_cumprod[-1], 2 * PER, seed=7)
            x = torch.from_numpy(x).view(2, PER).cuda()
            eu[n] = rel_err(_device_chain(model, diff, s, x, "unipc").cpu().numpy().reshape(-1), exact)
            e2m[n] = rel_err(_device_chain(model, diff, s, x, "dpmpp_2m").cpu().numpy().reshape(-1), exact)
            print(f"s={s} logsnr{n}: E_U = {eu[n]:.3e}, E_2M = {e2m[n]:.3e}")
    finally:
        model._bound_schedule = None                                             # the next test binds its own schedule again
    for name, value, holds in order_conditions(eu, e2m):
        print(f"s={s}: {name}: {value:.3f}")
        assert holds, (s, name, value)
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("case", ["x_0", "x_t", "x_t_minus_1", "denoised_fn", "predict_xstart"])
def test_the_step_on_the_network_along_a_chain(case):
    """Five steps from the last index, each fed its predecessor's sample and state: pred_xstart equals ddim_sample's for the same input
    at the step tolerance, the first step's sample is eta = 0 DDIM's, x^c and the sample stay inside the derived bound of the float64
    restatement fed the step's own x~, D_t and state, and behind the first step the sample differs from dpmpp_2m_sample's for the same
    input and history (the corrector moved the point the predictor starts from).  Measured on an MI355X: worst |d| / bound 0.930
    (predict_xstart, t = 7)."""
    model, diff = tiny(predict_xstart=True) if case == "predict_xstart" else tiny()
    assert diff.model_mean_type.name == ("START_X" if case == "predict_xstart" else "EPSILON")
    c = _rand_window(2, 6, 32, 2, seed=70)
    kw = _window_kw(c, case if case.startswith("x_") else "x_0")
    if case == "x_t_minus_1":
        kw["x_t_minus_1"] = (c["x0"] * 0.5).cuda()
    fn = _denoised_fn if case == "denoised_fn" else None
    N = diff.num_timesteps
    x, state = c["x"].cuda(), None
    for k, tv in enumerate(range(N - 1, N - 6, -1)):
        before = x.clone()
        kept = None if state is None else tuple(v.clone() for v in state[:3])
        out = diff.unipc_sample(model, x, _t(2, tv), state=state, denoised_fn=fn, model_kwargs=kw)
        assert set(out) == {"sample", "pred_xstart", "state"} and torch.equal(x, before) and out["sample"].data_ptr() != x.data_ptr()
        assert len(out["state"]) == 4 and out["state"][3] == k + 1
        if state is not None:                                                    # the state handed in is left as it was
            assert all(torch.equal(a, b) for a, b in zip(kept, state[:3]))
            assert all(a.data_ptr() != b.data_ptr() for a, b in zip(out["state"][:3], state[:3]))
        assert float(out["pred_xstart"].abs().max()) <= 1.0 and torch.equal(out["state"][1], out["pred_xstart"])
        ref = diff.ddim_sample(model, x, _t(2, tv), denoised_fn=fn, model_kwargs=kw, eta=0.0)
        close(out["pred_xstart"], ref["pred_xstart"], atol=ATOL, rtol=RTOL)
        _check(diff, [tv, tv], k, x, out["pred_xstart"], state, out["state"][0], out["sample"], f"{case} t={tv}")
        if state is None:                                                        # without state the step IS eta = 0 DDIM
            close(out["sample"], ref["sample"], atol=ATOL, rtol=RTOL)
        else:
            two_m = diff.dpmpp_2m_sample(model, x, _t(2, tv), prev_xstart=state[1], denoised_fn=fn, model_kwargs=kw)
            assert torch.equal(two_m["pred_xstart"], out["pred_xstart"]) and not torch.equal(two_m["sample"], out["sample"])
        x, state = out["sample"], out["state"]
    assert torch.isfinite(x).all()
    model.check_device_errors()


def test_a_non_finite_network_output_is_nan_and_sets_bit_1():
    """The eps path: a latent pixel beyond fp16's range makes the network output non-finite; the pass keeps it NaN (not clamped to +-1),
    writes it into the state as it is, and sets bit 1 of the device flags."""
    model, diff = tiny()
    c = _rand_window(2, 6, 32, 2, seed=75)
    kw, x = _window_kw(c), c["x"].cuda()
    x[0, -1, 0, 3, 3] = 7.0e4
    out = diff.unipc_sample(model, x, _t(2, 4), model_kwargs=kw)
    assert not torch.isfinite(out["sample"]).all() and not torch.isfinite(out["pred_xstart"]).all() and not torch.isfinite(out["state"][1]).all()
    with pytest.raises(FloatingPointError):
        model.check_device_errors()
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 4
def test_loops_chain_the_step():
    model, diff = tiny()
    c = _rand_window(2, 6, 32, 2, seed=80)
    kw = _window_kw(c)
    x_T = c["x"].cuda()
    N = diff.num_timesteps
    outs = list(diff.unipc_sample_loop_progressive(model, tuple(x_T.shape), noise=x_T, model_kwargs=kw))
    assert len(outs) == N and all(set(o) == {"sample", "pred_xstart", "state"} for o in outs)
    x, state = x_T, None
    for k, tv in enumerate(range(N - 1, -1, -1)):
        o = diff.unipc_sample(model, x, _t(2, tv), state=state, model_kwargs=kw)
        assert torch.equal(o["sample"], outs[k]["sample"]) and torch.equal(o["pred_xstart"], outs[k]["pred_xstart"]), tv
        x, state = o["sample"], o["state"]
    final = diff.unipc_sample_loop(model, tuple(x_T.shape), noise=x_T, model_kwargs=kw)
    assert torch.is_tensor(final) and torch.equal(final, x) and torch.isfinite(final).all()
    assert torch.equal(final, outs[-1]["pred_xstart"])                           # the last step returns D_0
    assert torch.equal(diff.unipc_sample_loop(diff._wrap_model(model), tuple(x_T.shape), noise=x_T, model_kwargs=kw), final)
    assert not torch.equal(diff.dpmpp_2m_sample_loop(model, tuple(x_T.shape), noise=x_T, model_kwargs=kw), final)
    assert not torch.equal(diff.ddim_sample_loop(model, tuple(x_T.shape), noise=x_T, model_kwargs=kw), final)
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 5
def _eager(model, diff, x_init, kw, n_steps, t_start, keep=()):
    """unipc_sample step by step from t_start, the first one without state; returns the last sample and those kept."""
    x, state, kept = x_init.clone(), None, {}
    for step in range(n_steps):
        o = diff.unipc_sample(model, x, _t(x.shape[0], t_start - step), state=state, model_kwargs=kw)
        x, state = o["sample"], o["state"]
        if step + 1 in keep:
            kept[step + 1] = x
    return x, kept


def test_window_executor_runs_the_step_as_a_graph():
    """sampler='unipc': the captured step is map_t -> forward -> unipc_kernel in place (the three state tensors in place too) -> t -= 1,
    steps += 1.  The window is bit-equal to the eager chain: two windows of one shape on ONE graph (the second one's first step
    without state although the buffers hold the first window's), a later t_start (first-order there), run(k) then run(),
    'x_0' / 'x_t' / 'x_t_minus_1' as handed; the re-noising form and a known region are refused by name."""
    model, diff = tiny()
    diff._bind(model)
    N = diff.num_timesteps
    ex = WindowExecutor(model, diff)
    g0 = None
    for wi, (n_obs, obsf) in enumerate([(2, "x_0"), (2, "x_0"), (2, "x_t"), (3, "x_t_minus_1")]):
        c = _rand_window(2, 6, 32, n_obs, seed=900 + wi)
        kw = _window_kw(c, obsf)
        if obsf == "x_t_minus_1":
            kw["x_t_minus_1"] = (c["x0"] * 0.5).cuda()
        x_init = c["x"].cuda()
        ex.begin(x_init, kw, sampler="unipc", seed=wi, renoise=False)
        assert ex._left == N
        if wi == 0:
            g0 = ex.graphs
        if wi == 1:
            assert ex.graphs == g0                                               # same signature: the first window's graph
        got_mid = ex.run(3).clone()
        got = ex.run().clone()
        with pytest.raises(_lib.VdError, match="t would pass 0"):
            ex.run(1)
        want, kept = _eager(model, diff, x_init, kw, N, N - 1, keep=(3,))
        assert torch.equal(kept[3], got_mid), (wi, obsf, float((kept[3] - got_mid).abs().max()))
        assert torch.equal(want, got) and torch.isfinite(got).all(), (wi, obsf, float((want - got).abs().max()))
        if wi == 1:                                                              # a later start on the same graph: first-order at t = 6
            ex.begin(x_init, kw, sampler="unipc", t_start=6)
            assert ex.graphs == g0 and ex._left == 7
            first = ex.run(1).clone()
            assert torch.equal(first, diff.unipc_sample(model, x_init, _t(2, 6), model_kwargs=kw)["sample"])
            assert torch.equal(ex.run().clone(), _eager(model, diff, x_init, kw, 7, 6)[0])
    model.check_device_errors()
    # `sampler` is part of the graph key, and the window differs from dpmpp_2m's
    c = _rand_window(2, 6, 32, 2, seed=950)
    kw, x_init = _window_kw(c), c["x"].cuda()
    uni = ex.begin(x_init, kw, sampler="unipc").run().clone()
    g = ex.graphs
    assert not torch.equal(ex.begin(x_init, kw, sampler="dpmpp_2m").run().clone(), uni) and ex.graphs == g + 1
    assert torch.equal(ex.begin(x_init, kw, sampler="unipc").run().clone(), uni) and ex.graphs == g + 1
    # the re-noising 'x_t_minus_1' form draws noise inside the graph: refused, by name and reason
    with pytest.raises(_lib.VdError, match="unipc_sample.*draws no noise"):
        ex.begin(x_init, _window_kw(c, "x_t_minus_1"), sampler="unipc", renoise=True)
    # a known region: refused by the executor and by the engine, by name
    from test_gpu_known_region import _window_region
    src, mask, _ = _window_region(c, seed=951)
    with pytest.raises(NotImplementedError, match="sampler='unipc' together with a known region"):
        ex.begin(x_init, kw, sampler="unipc", known_src=src, known_mask=mask)
    with diff.known_region_scope(model, src, mask):
        with pytest.raises(NotImplementedError, match="unipc_sample inside known_region_scope is not served"):
            diff.unipc_sample(model, x_init, _t(2, 3), model_kwargs=kw)
    L = _lib.lib()
    pk = model._pack_kwargs(x_init, kw)
    out = torch.empty_like(x_init)
    _lib.check(L.vd_set_known_region(model._handle, _lib.ptr(src), _lib.ptr(mask), None, 0, 0))
    try:
        rc = L.vd_unipc_sample(model._handle, 2, 6, *model._window_ptrs(x_init, pk), _lib.ptr(_t(2, 3)), None, None, None, 0, pk["obs_mode"], 1,
                               _lib.ptr(out), None, None, None, None, None, _lib.current_stream())
        assert rc != 0 and b"unipc_sample together with a known region" in L.vd_last_error()
        rc = L.vd_window_begin(model._handle, 2, 6, _lib.ptr(ex.x), *model._window_ptrs(x_init, pk)[1:], pk["obs_mode"], 5, 1, 0.0, 0, 0, N - 1,
                               ex.stream.cuda_stream)
        assert rc != 0 and b"sampler 5 (unipc_sample) together with a known region" in L.vd_last_error()
    finally:
        _lib.check(L.vd_set_known_region(model._handle, None, None, None, 0, 0))
    y = torch.zeros(2, 6, 3, 8, 8, device="cuda")
    with diff.dps_scope(model, y, 4, zeta=0.5):
        with pytest.raises(_lib.VdError, match="unipc_sample inside dps_scope is not served"):
            diff.unipc_sample(model, x_init, _t(2, 3), model_kwargs=kw)
    model.check_device_errors()


def test_window_with_suffix_skip_leaves_every_read_frame_bit_identical():
    model, diff = tiny()
    plain, skip = WindowExecutor(model, diff), WindowExecutor(model, diff, suffix_skip=True)
    for wi, (B, T, n_obs, obsf) in enumerate([(2, 6, 2, "x_0"), (3, 5, 4, "x_t_minus_1")]):
        c = _rand_window(B, T, 32, n_obs, seed=960 + wi)
        read = ~((c["obs_mask"].reshape(B, T) == 1) & (c["latent_mask"].reshape(B, T) == 0))
        kw = _window_kw(c, obsf)
        x_init = c["x"].cuda()
        want = plain.begin(x_init, kw, sampler="unipc", renoise=False).run().clone().cpu()
        skip.begin(x_init, kw, sampler="unipc", renoise=False)
        assert skip.suffix_frames == int(read.sum())
        got = skip.run().clone().cpu()
        assert torch.isfinite(got[read]).all() and torch.equal(got[read], want[read]), (wi, float((got[read] - want[read]).abs().max()))
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 6
def test_infer_video_graph_and_eager_agree_to_the_bit():
    from video_diffusion_amd.video_sample import infer_video
    model, diff = tiny()
    g = torch.Generator().manual_seed(10)
    batch = (torch.rand(2, 12, 3, 32, 32, generator=g) * 2 - 1).cuda()
    eager, _ = infer_video("autoreg", model, diff, batch, 6, 2, 4, sampler="unipc", executor="eager")
    graph, _ = infer_video("autoreg", model, diff, batch, 6, 2, 4, sampler="unipc", executor="graph")
    assert eager.shape == (2, 12, 3, 32, 32) and np.isfinite(eager).all()
    assert np.array_equal(eager, graph)
    assert np.array_equal(eager[:, :2], batch[:, :2].cpu().numpy()) and np.abs(eager[:, 2:]).max() > 0
    two_m, _ = infer_video("autoreg", model, diff, batch, 6, 2, 4, sampler="dpmpp_2m", executor="eager")
    assert not np.array_equal(two_m, eager)
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 7
def test_cfg_scale_and_measurement_compose():
    """cfg_scale = 2 differs from w = 1, and w = 1 is the plain step to the bit -- state included; inside measurement_scope the state
    holds the projected D_t, and at t = 0 the step returns it: A(sample) = y inside the bound test_gpu_measurement.py derives."""
    from measurement_restated import measure_fp64
    from test_gpu_known_region import _np
    from test_gpu_measurement import _final_bound, _project, _window_measurement
    model, diff = tiny()
    c = _rand_window(2, 6, 32, 2, seed=30)
    kw, x = _window_kw(c), c["x"].cuda()
    first = diff.unipc_sample(model, x, _t(2, 9), model_kwargs=kw)
    state = first["state"]
    plain = diff.unipc_sample(model, first["sample"], _t(2, 8), state=state, model_kwargs=kw)
    with diff.cfg_scale_scope(model, 2.0):
        guided = diff.unipc_sample(model, first["sample"], _t(2, 8), state=state, model_kwargs=kw)
    with diff.cfg_scale_scope(model, 1.0):
        one = diff.unipc_sample(model, first["sample"], _t(2, 8), state=state, model_kwargs=kw)
    assert not torch.equal(guided["sample"], plain["sample"]) and not torch.equal(guided["pred_xstart"], plain["pred_xstart"])
    assert torch.equal(one["sample"], plain["sample"]) and all(torch.equal(a, b) for a, b in zip(one["state"][:3], plain["state"][:3]))
    loop_w2 = diff.unipc_sample_loop(model, tuple(x.shape), noise=x, model_kwargs=kw, cfg_scale=2.0)
    assert torch.isfinite(loop_w2).all() and not torch.equal(loop_w2, diff.unipc_sample_loop(model, tuple(x.shape), noise=x, model_kwargs=kw))
    # measurement: the projection in front of the pass
    for s, gray in ((4, False), (1, True)):
        y = _window_measurement(c, s, gray, seed=71)
        for tv in (5, 0):
            free = diff.unipc_sample(model, x, _t(2, tv), state=state, model_kwargs=kw)
            with diff.measurement_scope(model, y, s, gray):
                got = diff.unipc_sample(model, x, _t(2, tv), state=state, model_kwargs=kw)
            want_x0 = _project(model, free["pred_xstart"], y, kw["latent_mask"].reshape(2, 6), s, gray)
            assert torch.equal(got["pred_xstart"], want_x0) and torch.equal(got["state"][1], want_x0)   # the projected D_t is what the state holds
            if tv == 0:                                                          # the last step returns the projected x_0: A(sample) = y up to rounding
                assert torch.equal(got["sample"], got["pred_xstart"])
                a_err = np.abs(measure_fp64(_np(got["sample"]), s, gray) - _np(y))[:, 2:]
                assert (a_err <= _final_bound(_np(got["sample"]), _np(y), s, gray)[:, 2:]).all()
    with diff.measurement_scope(model, y, 1, True):
        with pytest.raises(_lib.VdError, match="denoised_fn inside measurement_scope is not served"):
            diff.unipc_sample(model, x, _t(2, 3), denoised_fn=lambda v: v, model_kwargs=kw)
    model.check_device_errors()


def test_nothing_else_moved():
    """A p_sample, a ddim_sample, a dpmpp_2m_sample and a dpmpp_2m_sde_sample step give the same bits before and after unipc steps and a
    unipc window on the same engine."""
    model, diff = tiny()
    c = _rand_window(2, 6, 32, 2, seed=90)
    kw, x = _window_kw(c), c["x"].cuda()
    noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(91)).cuda()
    prev = (torch.rand(x.shape, generator=torch.Generator().manual_seed(92)) * 2 - 1).cuda()
    tt = _t(2, 4)

    def others():
        return [diff._fused_step(0, model, x, tt, True, kw, noise=noise), diff._fused_step(1, model, x, tt, True, kw, eta=0.5, noise=noise),
                diff._fused_step(3, model, x, tt, True, kw, prev_xstart=prev), diff._fused_step(4, model, x, tt, True, kw, noise=noise, prev_xstart=prev)]

    before = others()
    uni = diff.unipc_sample(model, x, tt, state=(x, prev, prev, 2), model_kwargs=kw)
    WindowExecutor(model, diff).begin(x, kw, sampler="unipc").run(3)
    after = others()
    for (s0, d0), (s1, d1) in zip(before, after):
        assert torch.equal(s0, s1) and torch.equal(d0, d1)
    assert all(not torch.equal(uni["sample"], s) for s, _ in before)
    model.check_device_errors()
