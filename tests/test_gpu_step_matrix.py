"""GPU: the option matrix of one denoise step (tests/step_matrix_cases.py), one test per row.  FreeU, cfg_scale and guidance rescale,
dynamic thresholding, a measurement or linear measurement, the sampler pass, a known region or particle steering stack inside ONE launch
sequence (csrc/engine.hip: step_launches) and share its scratch; every row runs that stack at the three entries and checks

  served   the fused step at three timesteps against the composition of tests/step_compose.py -- entries with per-element tests of their
           own, in step_launches' order -- to the bit; p_mean_variance against the same composition; a three-step window graph against the
           eager chain of fused steps at the window's Philox offsets, the carried history included; the graph's key against a row that
           differs in one option;
  refused  by name, in front of any launch, with the engine's option state untouched;
  ignored  (a known region and particles under p_mean_variance) the bits of the entry without the option;

and that each of the three is what `status` says it is.  Bit equality throughout: both sides run the same deterministic kernels on the
same inputs.  That holds for the rows under the window prefix cache too: the cache regroups only the fp64 partial sums of the GroupNorms
(include/vd_amd.h: vd_set_window_prefix_cache), and at this configuration their float32 results have kept every bit."""

import numpy as np
import pytest
import torch

import step_compose as sc
import step_matrix_cases as sm
from test_gpu_guidance import tiny
from video_diffusion_amd import _lib
from video_diffusion_amd.executor import WindowExecutor
from video_diffusion_amd.gaussian_diffusion import SAMPLERS

pytestmark = pytest.mark.gpu
ROWS = sm.matrix_rows()
REFUSALS = (_lib.VdError, NotImplementedError)
_windows, _restorations, _executors, _graphs = {}, {}, {}, {}
STEPS = 3


def _model(case):
    model, diff = tiny(predict_xstart=True) if case.model == "xstart" else tiny()
    diff._bind(model)
    if case.model not in _graphs:
        _graphs[case.model] = dict(seen=set())
        _warm(model, diff, case.model)
    return model, diff


def _window(B):
    if B not in _windows:
        _windows[B] = sc.matrix_window(B, 700 + B)
    return _windows[B]


def _restoration(kind, B):
    if (kind, B) not in _restorations:
        _restorations[kind, B] = sc.restoration_of(kind, _window(B), 800 + B)
    return _restorations[kind, B]


def _executor(model, diff, tag, switch):
    """One executor per model and window switch, kept for the whole module: its buffers' addresses are part of every graph's key."""
    if (tag, switch) not in _executors:
        _executors[tag, switch] = WindowExecutor(model, diff, prefix_cache=switch == "prefix_cache", suffix_skip=switch == "suffix_skip")
    return _executors[tag, switch]


def _begin(ex, diff, model, case, seed):
    name, eta = sm.SAMPLER[case.sampler]
    c = _window(sm.batch(case))
    R = _restoration(case.restoration, sm.batch(case))
    with sc.model_scopes(diff, model, case), sc.restoration_scope(diff, model, R):
        ex.begin(c["x"], sc._kw(c), t_start=0 if SAMPLERS[name].up else STEPS - 1, seed=seed, sampler=name, eta=eta, renoise=False,
                 cfg_scale=sm.GUIDANCE[case.guidance][0])


def _warm(model, diff, tag):
    """Every engine buffer at the largest size a row needs, before a graph is counted: a buffer that grows drops the captured graphs."""
    ex = _executor(model, diff, tag, "warm")
    for case in (sm.Case("unipc", tag, "w2_phi0.7_p0.9", "adaptive", "linear", "none"), sm.Case("p_sample", tag, "w2", "adaptive", "part_blur5", "none"),
                 sm.Case("dpmpp_2m_sde", tag, "off", "off", "part_linear", "none")):
        c = _window(4)
        R = sc.restoration_of(case.restoration, c, 899)
        name, eta = sm.SAMPLER[case.sampler]
        with sc.model_scopes(diff, model, case), sc.restoration_scope(diff, model, R):
            ex.begin(c["x"], sc._kw(c), t_start=STEPS - 1, seed=1, sampler=name, eta=eta, renoise=False, cfg_scale=sm.GUIDANCE[case.guidance][0])
        ex.run(1)
    torch.cuda.synchronize()


def _counted_begin(ex, diff, model, case, seed):
    """begin() with the graph count checked: a key begun before on this executor finds its graph, a new one captures exactly one.  (_warm
    has grown every engine buffer: a graph count that falls means one grew all the same and dropped the captured graphs.)"""
    st = _graphs[case.model]
    name, eta = sm.SAMPLER[case.sampler]
    key = (case.switch, sm.batch(case), name, None if name == "dpmpp_2m_sde" else eta, case.guidance, case.freeu, case.restoration)
    pre = ex.graphs
    _begin(ex, diff, model, case, seed)
    post = ex.graphs
    new = key not in st["seen"]
    assert post >= pre, f"{sm.case_id(case)}: an engine buffer grew inside begin() and dropped {pre} captured graphs: _warm does not cover this row"
    assert post == pre + (1 if new else 0), (sm.case_id(case), pre, post, "a new key" if new else "a key begun before")
    st["seen"].add(key)


def _carry_for(row, x, k):
    """What an eager step at the k-th of the three timesteps is handed: nothing at the first (a chain's first step), a history or a state
    of two finished steps at the others."""
    if row.carry is None or k == 0:
        return None
    if row.carry == "prev_xstart":
        return (0.3 * x).clamp(-1, 1)
    return ((0.9 * x).contiguous(), (0.3 * x).clamp(-1, 1), (-0.2 * x).clamp(-1, 1), 2)


def _check_out(got, want, row, tag):
    assert sc.same(got["pred_xstart"], want["pred_xstart"]), (tag, "pred_xstart", float((got["pred_xstart"] - want["pred_xstart"]).abs().max()))
    assert sc.same(got["sample"], want["sample"]), (tag, "sample", float((got["sample"] - want["sample"]).abs().max()))
    if row.carry == "state":
        assert got["state"][3] == want["state"][3]
        for j in range(3):
            assert sc.same(got["state"][j], want["state"][j]), (tag, "state", j)
    assert torch.isfinite(got["sample"]).all(), tag


@pytest.mark.parametrize("index", range(len(ROWS)), ids=[sm.case_id(r) for r in ROWS])
def test_row(index):
    case = ROWS[index]
    model, diff = _model(case)
    name, eta = sm.SAMPLER[case.sampler]
    row = SAMPLERS[name]
    w = sm.GUIDANCE[case.guidance][0]
    B = sm.batch(case)
    c, R = _window(B), _restoration(case.restoration, B)
    kw, x = sc._kw(c), c["x"]
    N = diff.num_timesteps
    times = (0, N // 2, N - 2) if row.up else (N - 1, N // 2, 0)
    noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(900 + index)).cuda()
    z = torch.randn(x.shape, generator=torch.Generator().manual_seed(901 + index)).cuda()
    u = torch.tensor([[0.37, 0.61], [0.83, 0.12]], dtype=torch.float64)
    off = case._replace(guidance="off", freeu="off", restoration="none", switch="none")
    plain = sc.fused_step(diff, model, off, x, sc._tb(B, times[1]), kw, noise=noise)
    assert sc.engine_state(model) == sc.ENGINE_OFF
    seen = {}

    # ---- the step entry
    status = sm.status(case, "step")
    if status == "served":
        moved = []
        for k, tv in enumerate(times):
            carry = _carry_for(row, x, k)
            want = sc.compose_step(model, diff, case, c, R, tv, noise, carry, known_noise=z)
            if sm.particles(case):                                               # what the step must do behind these tensors, before it runs
                uk, pw, st, r, bar = sc.restated_particles(R, want, tv == 0, 950 + 10 * index + k)
                anc = torch.from_numpy(pw["ancestors"]).long().cuda()
                want = dict(want, sample=want["sample"][anc], pred_xstart=want["pred_xstart"][anc])
            uniforms = (lambda tt, uk=uk: torch.from_numpy(uk)) if sm.particles(case) else None
            with sc.model_scopes(diff, model, case), sc.restoration_scope(diff, model, R, known_noise=z, uniforms=uniforms):
                got = sc.fused_step(diff, model, case, x, sc._tb(B, tv), kw, noise=noise, carry=carry)
            if sm.particles(case):
                assert {"ancestors", "log_weights", "ess"} <= set(got), sorted(got)
                assert np.array_equal(got["ancestors"].cpu().numpy(), pw["ancestors"]), (sm.case_id(case), tv, got["ancestors"].tolist(), pw["ancestors"])
                lw = got["log_weights"].cpu().numpy()
                assert (np.abs(lw - st["logw"].reshape(-1)) <= np.where(st["logw"].reshape(-1) == 0.0, 0.0, bar)).all(), (sm.case_id(case), tv, lw, r, bar)
                if tv == 0:
                    assert np.array_equal(got["chosen"].cpu().numpy(), pw["chosen"]) and np.array_equal(pw["ancestors"], np.arange(B))
                else:
                    assert "chosen" not in got
                    moved.append(bool(pw["resampled"].any()))
            else:
                assert "ancestors" not in got
            _check_out(got, want, row, (sm.case_id(case), tv))
        assert not sm.particles(case) or any(moved), (sm.case_id(case), "no step at t > 0 resampled")
        seen["step"] = "served"
    else:
        assert status[0] == "refused"
        with pytest.raises(REFUSALS) as ei:
            with sc.model_scopes(diff, model, case), sc.restoration_scope(diff, model, R, known_noise=z, uniforms=lambda tt: u):
                sc.fused_step(diff, model, case, x, sc._tb(B, times[1]), kw, noise=noise)
        assert sm.fragment_in(status[1], str(ei.value)), (status[1], str(ei.value))
        assert sc.engine_state(model) == sc.ENGINE_OFF
        seen["step"] = "refused"

    # ---- p_mean_variance inside the same scopes
    status = sm.status(case, "p_mean_variance")
    assert status in ("served", "ignored")
    for tv in times:
        t = sc._tb(B, tv)
        with sc.model_scopes(diff, model, case):
            with sc.restoration_scope(diff, model, R, known_noise=z, uniforms=lambda tt: u):
                pmv = diff.p_mean_variance(model, x, t, model_kwargs=kw, cfg_scale=w)
            bare = diff.p_mean_variance(model, x, t, model_kwargs=kw, cfg_scale=w) if status == "ignored" else None
        want = sc.compose_step(model, diff, case, c, R, tv, noise)
        assert sc.same(pmv["pred_xstart"], want["x0"]) and sc.same(pmv["mean"], want["mean"]), (sm.case_id(case), tv)
        if status == "ignored":                                                   # the entry without the option, to the bit
            assert sc.same(pmv["pred_xstart"], bare["pred_xstart"]) and sc.same(pmv["mean"], bare["mean"]) and sc.same(pmv["eps"], bare["eps"])
    seen["p_mean_variance"] = status

    # ---- the window
    status = sm.status(case, "window")
    ex = _executor(model, diff, case.model, case.switch)
    seed = 1000 + index
    if status == "served":
        _counted_begin(ex, diff, model, case, seed)
        assert sc.engine_state(model) == sc.ENGINE_OFF                           # engine state for the length of begin() only: run() needs no scope
        trace = []
        for _ in range(STEPS):
            xk = ex.run(1).clone()
            trace.append((xk, sc.window_history(ex, name, B)))
        eager = sc.eager_window(model, diff, case, c, R, seed, STEPS, 0 if row.up else STEPS - 1)
        read = torch.ones(B, sc.T_, dtype=torch.bool, device="cuda")
        if case.switch == "suffix_skip":                                         # the purely observed frames' entries are meaningless (vd_set_window_suffix_skip)
            read = ~((c["obs_mask"].reshape(B, -1) == 1) & (c["latent_mask"].reshape(B, -1) == 0))
            assert 0 < ex.suffix_frames == int(read.sum()) < B * sc.T_
        if case.switch == "prefix_cache":
            assert ex.cached_frames == B * sc.T_ - int((~((c["obs_mask"].reshape(B, -1) == 1) & (c["latent_mask"].reshape(B, -1) == 0))).sum()) > 0
        for k, ((xg, hg), (xe, carry)) in enumerate(zip(trace, eager)):
            assert sc.same(xg[read], xe[read]) and torch.isfinite(xg[read]).all(), (sm.case_id(case), "window step", k, float((xg - xe)[read].abs().max()))
            if row.carry == "prev_xstart":
                assert sc.same(hg[0][read], carry[read]), (sm.case_id(case), "history", k)
            elif row.carry == "state":
                for j, h in enumerate((hg[1], hg[0], hg[2])):                   # (x^c, D_{t+1}, D_{t+2}): the engine keeps D_{t+1} in the history buffer
                    assert sc.same(h[read], carry[j][read]), (sm.case_id(case), "state", j, k)
        # keyed by every option that changes the launches: a row that differs in one value is another graph, this row finds its own again
        partner = sm.keying_partner(case, index)
        if partner is not None:
            _counted_begin(ex, diff, model, partner, seed)
        pre = ex.graphs
        _counted_begin(ex, diff, model, case, seed)
        assert ex.graphs == pre
        again = ex.run(STEPS)
        assert sc.same(again[read], trace[-1][0][read]), (sm.case_id(case), "begun again")
        seen["window"] = "served"
    else:
        assert status[0] == "refused"
        pre = ex.graphs
        with pytest.raises(REFUSALS) as ei:
            _begin(ex, diff, model, case, seed)
        assert sm.fragment_in(status[1], str(ei.value)), (status[1], str(ei.value))
        assert ex.graphs == pre and sc.engine_state(model) == sc.ENGINE_OFF      # in front of any launch: nothing captured, nothing left set
        seen["window"] = "refused"

    # ---- agreement, and the engine as it was
    for entry in sm.ENTRIES:
        s = sm.status(case, entry)
        assert seen[entry] == (s if isinstance(s, str) else s[0]), (entry, s, seen[entry])
    assert sc.engine_state(model) == sc.ENGINE_OFF
    after = sc.fused_step(diff, model, off, x, sc._tb(B, times[1]), kw, noise=noise)
    assert sc.same(after["sample"], plain["sample"]) and sc.same(after["pred_xstart"], plain["pred_xstart"])
    model.check_device_errors()


def test_window_history_refusals_by_name():
    """vd_window_history, the entry the history check reads through: refused by name without an armed window, for another B or T, for a
    sampler that carries nothing, and for UniPC's two further tensors under a sampler that carries one; served, it changes nothing."""
    model, diff = tiny(timestep_respacing="ddim5")                              # an engine of its own: no window has been begun on it
    diff._bind(model)
    L, h = _lib.lib(), model._handle
    c = _window(2)
    x, kw = c["x"], sc._kw(c)
    out = [torch.empty_like(x) for _ in range(3)]
    ex = WindowExecutor(model, diff)
    call = lambda B, T, *ptrs: L.vd_window_history(h, B, T, *ptrs, ex.stream.cuda_stream)     # noqa: E731
    assert call(2, sc.T_, _lib.ptr(out[0]), None, None) != 0 and b"no window is armed" in L.vd_last_error()
    ex.begin(x, kw, sampler="p_sample", seed=1)
    assert call(2, sc.T_, _lib.ptr(out[0]), None, None) != 0 and b"p_sample carries no history" in L.vd_last_error()
    ex.begin(x, kw, sampler="dpmpp_2m")
    ex.run(1)
    assert call(3, sc.T_, _lib.ptr(out[0]), None, None) != 0 and b"B and T are the armed window's" in L.vd_last_error()
    assert call(2, sc.T_ + 1, _lib.ptr(out[0]), None, None) != 0 and b"B and T are the armed window's" in L.vd_last_error()
    assert call(2, sc.T_, _lib.ptr(out[0]), _lib.ptr(out[1]), None) != 0 and b"carries one tensor, not UniPC's three" in L.vd_last_error()
    want = diff.dpmpp_2m_sample(model, x, sc._tb(2, diff.num_timesteps - 1), model_kwargs=kw)
    before = ex.x.clone()
    hist = sc.window_history(ex, "dpmpp_2m", 2)[0]
    assert sc.same(hist, want["pred_xstart"]) and sc.same(ex.x, before) and sc.same(before, want["sample"])
    assert sc.same(ex.run(1), diff.dpmpp_2m_sample(model, want["sample"], sc._tb(2, diff.num_timesteps - 2), prev_xstart=hist, model_kwargs=kw)["sample"])
    ex.begin(x, kw, sampler="unipc")
    ex.run(1)
    hist, ubase, ud2 = sc.window_history(ex, "unipc", 2)
    state = diff.unipc_sample(model, x, sc._tb(2, diff.num_timesteps - 1), model_kwargs=kw)["state"]
    assert sc.same(ubase, state[0]) and sc.same(hist, state[1]) and sc.same(ud2, state[2]) and state[3] == 1
    model.check_device_errors()
