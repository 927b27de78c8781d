"""GPU: which engine state a captured window graph depends on -- one test per row of tests/window_state_cases.py, and four sequences
the rows do not reach (weights reloaded on a live model, the eviction of prefix stores, growth and return, a graph hit on new contents).

The invariant is the comment above drop_window_graphs() in csrc/engine.hip: whatever replaces an address or a value a captured graph
holds drops every graph first.  Each row runs: a window of two steps, whose bits are the eager chain's; the change; the bookkeeping of
the row's class (graph count, generation, the refusal) BEFORE anything is replayed; a window again, whose bits are the eager chain's
under the new state.  Between a change of class DROPS and the next begin() the only vd_window_run is one of 0 steps, which launches
nothing: on a library whose setter forgets to drop, the row fails at `graphs == 0` and no stale graph is ever replayed.

The yardstick is the chain of fused eager steps at the window's Philox offsets (tests/step_compose.py: eager_window), to the bit: both
sides run the same deterministic kernels on the same inputs, so nothing is measured and nothing has a tolerance."""
import re

import numpy as np
import pytest
import torch

import step_compose as sc
import step_matrix_cases as sm
import video_diffusion_amd as vda
import window_state_cases as ws
from video_diffusion_amd import _lib
from video_diffusion_amd.executor import WindowExecutor
from video_diffusion_amd.gaussian_diffusion import check_separable_operator, gaussian_kernel, resize_matrix, separable_pinv
from video_diffusion_amd.weights_init import synth_param

pytestmark = pytest.mark.gpu
KEYS = vda.video_model_and_diffusion_defaults().keys()
TINY = dict(T=6, image_size=32, num_channels=32, num_res_blocks=1, rp_alpha=6, rp_beta=6, rp_gamma=6, timestep_respacing="ddim10")
T_START, SEED = 3, 4321                                                          # four steps are left: two, the change, two
BASE = sm.Case("p_sample", "eps", "off", "off", "none", "none")
NONE = dict(kind="none")
_state, _windows, _restorations, _sds, _keep = {}, {}, {}, {}, []


# ------------------------------------------------------------------------------------------------ models, windows, executors
def _sd(specs, second=False):
    """The synthetic weights, or a second set of them (another generator key per parameter; the same scales by kind of parameter)."""
    if second not in _sds:
        _sds[second] = {n: torch.from_numpy(synth_param(("second/" + n) if second else n, s)) for n, s in specs}
    return _sds[second]


def _fresh(second=False):
    """A model of its own: no buffer of its engine has grown yet."""
    cfg = {**vda.video_model_and_diffusion_defaults(), **TINY}
    model, diff = vda.create_video_model_and_diffusion(**{k: cfg[k] for k in KEYS})
    model.load_state_dict(_sd(model.param_specs(), second))
    model.to("cuda")
    model.eval()
    diff._bind(model)
    return model, diff


def _case(over):
    return BASE._replace(**over)


def _window(B):
    if B not in _windows:
        _windows[B] = sc.matrix_window(B, 700 + B)
    return _windows[B]


def _restoration(kind, B):
    if (kind, B) not in _restorations:
        _restorations[kind, B] = sc.restoration_of(kind, _window(B), 800 + B)
    return _restorations[kind, B]


def _shared():
    """The model most rows share, with every engine buffer at the largest size a row needs: a buffer that grows drops the graphs, which
    is what the growth rows are about (they take models of their own)."""
    if "shared" not in _state:
        model, diff = _fresh()
        ex = _executor(model, diff)
        for case in (sm.Case("unipc", "eps", "w2_phi0.7_p0.9", "adaptive", "linear", "none"), sm.Case("p_sample", "eps", "w2", "adaptive", "part_blur5", "none"),
                     sm.Case("dpmpp_2m_sde", "eps", "off", "off", "part_linear", "none"), sm.Case("p_sample", "eps", "off", "off", "part_cell4", "none")):
            c, R = _window(4), _restoration(case.restoration, 4)
            _begin(ex, model, diff, case, c, R)
            ex.run(1)
            _eager(model, diff, case, c, R, 1)
        torch.cuda.synchronize()
        _state["shared"] = (model, diff)
    return _state["shared"]


def _executor(model, diff, **kw):
    """An executor of its own per test, kept alive for the module: its buffers' addresses are part of every key, so no key of one test
    is a key of another."""
    ex = WindowExecutor(model, diff, **kw)
    _keep.append(ex)
    return ex


def _generation(model):
    return int(_lib.lib().vd_window_generation(model._handle))


def _kw(c, observed_frames="x_0"):
    return dict(sc._kw(c), observed_frames=observed_frames)


def _begin(ex, model, diff, case, c, R=NONE, observed_frames="x_0", seed=SEED):
    """begin() inside the row's scopes -> (graph count, generation) inside them in front of begin(): behind the setters the scopes call."""
    name, eta = sm.SAMPLER[case.sampler]
    with sc.model_scopes(diff, model, case), sc.restoration_scope(diff, model, R):
        pre = (ex.graphs, _generation(model))
        ex.begin(c["x"], _kw(c, observed_frames), t_start=T_START, seed=seed, sampler=name, eta=eta, renoise=observed_frames == "x_t_minus_1",
                 cfg_scale=sm.GUIDANCE[case.guidance][0])
    return pre


def _eager_xtm1(model, diff, c, steps, seed):
    """'x_t_minus_1' as p_sample_loop runs it: every step re-noises the clean observed frames to t - 1 with the second half of its Philox
    range (test_gpu_engine.py: test_window_executor_equals_eager_steps_bit_for_bit)."""
    L = _lib.lib()
    cur = c["x"].clone()
    B, T = cur.shape[:2]
    per = cur[0].numel()
    k = model._pack_kwargs(cur, _kw(c, "x_t_minus_1"))
    x0 = c["x0"].float().contiguous()
    out = []
    for step in range(steps):
        t, t_prev = sc._tb(B, T_START - step), sc._tb(B, T_START - step - 1)
        nz, obs_src, nxt = sc._randn(cur.shape, seed, step * B * per + B * per // 2), torch.empty_like(cur), torch.empty_like(cur)
        _lib.check(L.vd_q_sample(model._handle, B, per, _lib.ptr(x0), _lib.ptr(t_prev), _lib.ptr(nz), _lib.ptr(obs_src), _lib.current_stream()))
        _lib.check(L.vd_p_sample(model._handle, B, T, _lib.ptr(cur), _lib.ptr(obs_src), _lib.ptr(k["obs_mask"]), _lib.ptr(k["latent_mask"]),
                                 _lib.ptr(k["kinda_marg_mask"]), _lib.ptr(k["frame_indices"]), _lib.ptr(t), 2, 1, None, seed, step * B * per,
                                 _lib.ptr(nxt), None, None, _lib.current_stream()))
        cur = nxt
        out.append(cur)
    return out


def _eager(model, diff, case, c, R=NONE, steps=2, observed_frames="x_0", seed=SEED):
    """The samples of the eager chain under the row's state, one per step."""
    if observed_frames == "x_t_minus_1":
        assert case == BASE
        return _eager_xtm1(model, diff, c, steps, seed)
    return [x for x, _ in sc.eager_window(model, diff, case, c, R, seed, steps, T_START)]


def _same(got, want, what):
    assert sc.same(got, want) and torch.isfinite(got).all(), (what, float((got - want).abs().max()))


def _invalidated(ex):
    """A run of 0 steps: launches nothing, and says whether the armed window is still good."""
    with pytest.raises(_lib.VdError, match="window graphs invalidated"):
        ex.run(0)


# ------------------------------------------------------------------------------------------------ the recipes of kind 'call'
def _h(model):
    return _lib.lib(), model._handle


def move_weight_storage(model, diff):
    L, h = _h(model)
    new = model._wbuf.clone()
    torch.cuda.synchronize()
    _lib.check(L.vd_set_weight_storage(h, _lib.ptr(new), new.numel() * 4))
    model._wbuf = new


def host_weight_storage(model, diff):
    L, h = _h(model)
    model._host_image = torch.zeros(model._wbuf.numel())
    _lib.check(L.vd_set_weight_storage_host(h, _lib.ptr(model._host_image), model._host_image.numel() * 4))


def device_weight_storage(model, diff):
    L, h = _h(model)
    _lib.check(L.vd_set_weight_storage(h, _lib.ptr(model._wbuf), model._wbuf.numel() * 4))


def mark_weights_loaded(model, diff):
    model.mark_weights_received()


def set_bwd_weight_storage(model, diff):
    L, h = _h(model)
    nbytes = L.vd_bwd_weights_bytes(h)
    new = torch.zeros(max(nbytes // 4, 4), dtype=torch.float32, device=model.device)
    _lib.check(L.vd_set_bwd_weight_storage(h, _lib.ptr(new), nbytes, 0))
    model._wbuf_bwd = new
    model._upload_bwd()


def load_weight_bwd(model, diff):
    model._upload_bwd()


def reupload_freqs(model, diff):
    model._upload_freqs()


def set_schedule(model, diff):
    L, h = _h(model)
    tab = diff._device_tables()
    tmap, scale = diff._timestep_map_and_scale()
    tm = np.ascontiguousarray(np.array(tmap, dtype=np.int32))
    _lib.check(L.vd_set_schedule(h, diff.num_timesteps, _lib.ptr(tab), _lib.ptr(tm), float(np.float32(scale))))
    model._bound_schedule = None                                                 # the rows of the schedule that went are gone with it


def rebind(model, diff):
    model._bound_schedule = None
    diff._bind(model)


def set_multistep_weights(model, diff):
    L, h = _h(model)
    w = np.ascontiguousarray(diff._multistep_weights().astype(np.float32))
    _lib.check(L.vd_set_multistep_weights(h, diff.num_timesteps, _lib.ptr(w)))


def set_unipc_rows(model, diff):
    L, h = _h(model)
    rows = np.ascontiguousarray(diff._unipc_rows().astype(np.float32))
    _lib.check(L.vd_set_unipc_rows(h, diff.num_timesteps, _lib.ptr(rows)))


def set_jump_rows(model, diff):
    L, h = _h(model)
    sa, sb = (np.ascontiguousarray(r.astype(np.float32)) for r in diff._jump_rows())
    _lib.check(L.vd_set_jump_rows(h, diff.num_timesteps, _lib.ptr(sa), _lib.ptr(sb)))


def flip_mean_type(model, diff):
    L, h = _h(model)
    _lib.check(L.vd_set_model_mean_type(h, 1))


def restore_mean_type(model, diff):
    L, h = _h(model)
    _lib.check(L.vd_set_model_mean_type(h, 0))


def toggle_prefix_cache(model, diff):
    L, h = _h(model)
    _lib.check(L.vd_set_window_prefix_cache(h, 1))


def toggle_suffix_skip(model, diff):
    L, h = _h(model)
    _lib.check(L.vd_set_window_suffix_skip(h, 1))


def window_switches_off(model, diff):
    L, h = _h(model)
    _lib.check(L.vd_set_window_prefix_cache(h, 0))
    _lib.check(L.vd_set_window_suffix_skip(h, 0))


def arm_attn_capture(model, diff):
    model._held_attn = model._attn_capture(2, sc.T_)


def clear_attn_capture(model, diff):
    model._attn_release()
    model._held_attn = None


PREPARE = {"load_weight_bwd": lambda model, diff: model.enable_guidance(), "set_bwd_weight_storage": lambda model, diff: model.enable_guidance()}


# ------------------------------------------------------------------------------------------------ one test per row
def _run_call(row):
    model, diff = _shared()
    rec = row.recipe
    apply, restore = globals()[rec["apply"]], globals()[rec["restore"]] if rec["restore"] else None
    if rec["apply"] in PREPARE:
        PREPARE[rec["apply"]](model, diff)
    ex, c = _executor(model, diff), _window(2)
    g0 = ex.graphs
    _begin(ex, model, diff, BASE, c)
    assert ex.graphs == g0 + 1
    A = ex.run(2).clone()
    want = _eager(model, diff, BASE, c, steps=4)
    _same(A, want[1], "the window in front of the change")
    g, gen = ex.graphs, _generation(model)
    assert g == g0 + 1
    apply(model, diff)
    try:
        if row.cls == ws.DROPS:
            assert ex.graphs == 0, f"{row.name} left {ex.graphs} captured graphs alive"
            assert _generation(model) == gen                                     # the engine's refusal, not the executor's _gen check, stops the run
            _invalidated(ex)
            if rec["refusal"]:
                with pytest.raises(_lib.VdError, match=re.escape(rec["refusal"])):
                    _begin(ex, model, diff, BASE, c)
                assert ex.graphs == 0
        elif row.cls == ws.NOT_CAPTURED:
            assert (ex.graphs, _generation(model)) == (g, gen)
            _same(ex.run(2).clone(), want[3], "the window in flight, behind the change")
        else:
            assert row.cls == ws.REFUSED
            assert (ex.graphs, _generation(model)) == (g, gen)
            with pytest.raises(_lib.VdError, match=re.escape(rec["refusal"])):
                _begin(ex, model, diff, BASE, c)
            assert (ex.graphs, _generation(model)) == (g, gen)
    finally:
        if restore:
            restore(model, diff)
    pre = _begin(ex, model, diff, BASE, c)
    assert ex.graphs == (1 if row.cls == ws.DROPS else g) and pre[0] == ex.graphs - (1 if row.cls == ws.DROPS else 0)
    got = ex.run(2).clone()
    _same(got, _eager(model, diff, BASE, c)[1], "the window behind the change")
    _same(got, A, "the state is the one the first window ran under")
    model.check_device_errors()


def _run_options(row):
    model, diff = _shared()
    before, after = _case(row.recipe["before"]), _case({**row.recipe["before"], **row.recipe["after"]})
    B = 4 if sm.particles(before) or sm.particles(after) else 2
    c, Ra, Rb = _window(B), _restoration(before.restoration, B), _restoration(after.restoration, B)
    ex = _executor(model, diff)
    g0 = ex.graphs
    _begin(ex, model, diff, before, c, Ra)
    assert ex.graphs == g0 + 1
    A = ex.run(2).clone()
    _same(A, _eager(model, diff, before, c, Ra)[1], "before")
    gen = _generation(model)
    assert ex.graphs == g0 + 1
    pre = _begin(ex, model, diff, after, c, Rb)
    assert pre == (g0 + 1, gen), f"{row.name} itself touched the graphs or the generation"
    assert ex.graphs == g0 + 2, "the option is not in the key: the window found the graph of the old value"
    got = ex.run(2).clone()
    _same(got, _eager(model, diff, after, c, Rb)[1], "after")
    assert not sc.same(got, A), "the recipe's change does not act on the bits"
    pre = _begin(ex, model, diff, before, c, Ra)
    assert pre[0] == g0 + 2 and ex.graphs == g0 + 2, "the old value back did not find the old graph"
    _same(ex.run(2).clone(), A, "the old value back")
    model.check_device_errors()


def _varied(R, vary):
    if vary == "taps":
        return dict(R, steer=dict(blur_kernel=gaussian_kernel(5, 2.0)))
    A = resize_matrix(sc.S_, sc.S_ // 2, mode="bilinear")
    a_h, a_w = check_separable_operator(A, A)
    return dict(R, A=(A, A), a=(a_h, a_w), P=(separable_pinv(a_h, 1e-3)[0], separable_pinv(a_w, 1e-3)[0]))


def _run_restoration_content(row):
    model, diff = _shared()
    case = _case(dict(restoration=row.recipe["restoration"]))
    B = sm.batch(case)
    c, R1 = _window(B), _restoration(case.restoration, B)
    R2 = _varied(R1, row.recipe["vary"])
    ex = _executor(model, diff)
    g0 = ex.graphs
    _begin(ex, model, diff, case, c, R1)
    assert ex.graphs == g0 + 1
    A = ex.run(2).clone()
    _same(A, _eager(model, diff, case, c, R1)[1], "before")
    gen = _generation(model)
    pre = _begin(ex, model, diff, case, c, R2)
    assert pre == (g0 + 1, gen) and ex.graphs == g0 + 1, "new content of the same shape is the same graph"
    got = ex.run(2).clone()
    _same(got, _eager(model, diff, case, c, R2)[1], "after")
    assert not sc.same(got, A), "the recipe's change does not act on the bits"
    model.check_device_errors()


def _run_reload(row):
    model, diff = _fresh()
    ex, c = _executor(model, diff), _window(2)
    _begin(ex, model, diff, BASE, c)
    A = ex.run(2).clone()
    _same(A, _eager(model, diff, BASE, c)[1], "before")
    g, gen = ex.graphs, _generation(model)
    assert g == 1
    model.load_state_dict(_sd(model.param_specs(), second=True))
    assert (ex.graphs, _generation(model)) == (g, gen)
    pre = _begin(ex, model, diff, BASE, c)
    assert pre[0] == g and ex.graphs == g
    got = ex.run(2).clone()
    _same(got, _eager(model, diff, BASE, c)[1], "after")
    assert not sc.same(got, A)
    model.check_device_errors()


def _run_growth_eager(row):
    model, diff = _fresh()
    ex, c2, c4 = _executor(model, diff), _window(2), _window(4)
    _begin(ex, model, diff, BASE, c2)
    A = ex.run(2).clone()
    _same(A, _eager(model, diff, BASE, c2)[1], "the small window")
    assert ex.graphs == 1
    gen = _generation(model)
    _eager(model, diff, BASE, c4, steps=1)                                       # the growth event: an eager step at B = 4
    assert ex.graphs == 0, f"{row.name}: the workspace moved under {ex.graphs} captured graphs"
    assert _generation(model) == gen
    _invalidated(ex)
    _begin(ex, model, diff, BASE, c2)
    assert ex.graphs == 1
    _same(ex.run(2).clone(), A, "the small window again")
    model.check_device_errors()


def _run_growth_begin(row):
    rec = row.recipe
    case, obsf = _case(dict(rec["options"], sampler=rec["sampler"])), rec["observed_frames"]
    model, diff = _fresh()
    ex, c2, c4 = _executor(model, diff), _window(2), _window(4)
    R2, R4 = _restoration(case.restoration, 2), _restoration(case.restoration, 4)
    _begin(ex, model, diff, BASE, c4)                                            # beforehand: the workspace and the step counters at B = 4
    ex.run(1)
    assert ex.graphs == 1
    _begin(ex, model, diff, case, c2, R2, obsf)
    assert ex.graphs == 2
    A = ex.run(2).clone()
    _begin(ex, model, diff, case, c4, R4, obsf)                                  # the growth event
    assert ex.graphs == 1, f"{row.name}: {ex.graphs - 1} graphs outlived the buffer they point into"
    big = ex.run(2).clone()
    _begin(ex, model, diff, case, c2, R2, obsf)
    assert ex.graphs == 2
    again = ex.run(2).clone()
    # the eager chains last: they size buffers of their own
    _same(A, _eager(model, diff, case, c2, R2, observed_frames=obsf)[1], "the small window")
    _same(big, _eager(model, diff, case, c4, R4, observed_frames=obsf)[1], "the large window")
    _same(again, A, "the small window again")
    model.check_device_errors()


@pytest.mark.parametrize("row", ws.ROWS, ids=ws.row_id)
def test_row(row):
    globals()["_run_" + row.recipe["kind"]](row)


# ------------------------------------------------------------------------------------------------ sequences the rows do not reach
def _read_frames(c):
    B, T = c["x"].shape[:2]
    return ~((c["obs_mask"].reshape(B, T) == 1) & (c["latent_mask"].reshape(B, T) == 0))


@pytest.mark.parametrize("switch", ["plain", "prefix_cache", "suffix_skip"])
def test_weights_reloaded_on_a_live_model(switch):
    """load_state_dict on a model whose graphs exist repacks into the storage the graphs read: the count stays, a graph hit under the
    prefix cache rebuilds its store from the new weights, and the bits are those of a fresh model loaded with the second weights (under
    the suffix skip: on the frames a caller reads)."""
    opts = {switch: True} if switch != "plain" else {}
    model, diff = _fresh()
    ex, c = _executor(model, diff, **opts), _window(2)
    read = _read_frames(c) if switch == "suffix_skip" else torch.ones(2, sc.T_, dtype=torch.bool, device="cuda")
    _begin(ex, model, diff, BASE, c)
    A = ex.run(2).clone()
    g = ex.graphs
    assert g == 1 and (ex.cached_frames == 2) == (switch == "prefix_cache") and (ex.suffix_frames > 0) == (switch == "suffix_skip")
    model.load_state_dict(_sd(model.param_specs(), second=True))
    assert ex.graphs == g
    _begin(ex, model, diff, BASE, c)
    assert ex.graphs == g and (ex.cached_frames == 2) == (switch == "prefix_cache")
    got = ex.run(2).clone()
    model2, diff2 = _fresh(second=True)
    ex2 = _executor(model2, diff2, **opts)
    _begin(ex2, model2, diff2, BASE, c)
    want = ex2.run(2).clone()
    _same(got[read], want[read], switch)
    assert not sc.same(got[read], A[read])
    if switch == "plain":
        _same(got, _eager(model, diff, BASE, c)[1], "eager on the reloaded model")
    model.check_device_errors()


def _pattern_window(observed, seed):
    """B = 2, T = 6: item 0 observes the frames `observed`, item 1 nothing; every other frame is latent."""
    g = torch.Generator().manual_seed(seed)
    B, T, S = 2, sc.T_, sc.S_
    obs = torch.zeros(B, T, 1, 1, 1)
    obs[0, list(observed)] = 1
    x0 = (torch.rand(B, T, 3, S, S, generator=g) * 2 - 1) * obs
    return dict(x=(1.5 * torch.randn(B, T, 3, S, S, generator=g)).cuda(), x0=x0.cuda(), obs_mask=obs.cuda(), latent_mask=(1 - obs).cuda(),
                kinda_marg_mask=torch.zeros(B, T, 1, 1, 1).cuda(), frame_indices=torch.arange(T).view(1, T).repeat(B, 1).cuda(), xtm1=x0.cuda())


def test_prefix_store_eviction_keeps_four_stores_and_a_valid_current_window():
    """capture_window: at most four graphs keep a prefix store; a fifth pattern releases the oldest and erases it from the vector, and
    win_cur must name the new graph behind the erase (vd_window_prefix_frames reads win_graphs[win_cur]).  Five patterns, then the first
    again: the engine's graph count is the plain executor's one graph plus min(patterns so far, 4), every window's bits are the plain
    executor's, and the evicted pattern's second window gives its first window's bits."""
    model, diff = _fresh()
    plain, cached = _executor(model, diff), _executor(model, diff, prefix_cache=True)
    patterns = [(0,), (0, 1), (0, 1, 2), (1,), (2, 3), (0,)]
    counts, first = [], None
    for i, observed in enumerate(patterns):
        c = _pattern_window(observed, 900 + len(observed) * 10 + observed[0])
        _begin(plain, model, diff, BASE, c, seed=SEED + i % 5)
        want = plain.run(2).clone()
        _begin(cached, model, diff, BASE, c, seed=SEED + i % 5)
        counts.append(cached.graphs)
        assert cached.cached_frames == len(observed), (i, cached.cached_frames)
        got = cached.run(2).clone()
        _same(got, want, ("pattern", i))
        if i == 0:
            first = got
    assert counts == [2, 3, 4, 5, 5, 5], counts
    _same(got, first, "the evicted pattern, captured again")
    model.check_device_errors()


def test_growth_and_return():
    """B = 1, then B = 2, then B = 1: the larger window moves the workspace and drops the graphs, the second small window captures
    again and gives the first one's bits."""
    model, diff = _fresh()
    ex, c2 = _executor(model, diff), _window(2)
    c1 = {k: v[:1].contiguous() for k, v in c2.items()}
    counts, runs = [], []
    for c in (c1, c2, c1):
        _begin(ex, model, diff, BASE, c)
        counts.append(ex.graphs)
        runs.append(ex.run(2).clone())
    assert counts == [1, 1, 2], counts
    _same(runs[2], runs[0], "B = 1 again")
    _same(runs[0], _eager(model, diff, BASE, c1)[1], "B = 1")
    _same(runs[1], _eager(model, diff, BASE, c2)[1], "B = 2")
    model.check_device_errors()


def test_a_graph_hit_serves_new_contents_at_the_same_addresses():
    """Without the prefix cache and the suffix skip a graph depends on the addresses of the window tensors, not on what they hold: new
    masks, frame indices, observations and x in the executor's buffers are a graph hit, and the bits are the eager chain's on them."""
    model, diff = _shared()
    ex, c = _executor(model, diff), _window(2)
    g0 = ex.graphs
    _begin(ex, model, diff, BASE, c)
    A = ex.run(2).clone()
    assert ex.graphs == g0 + 1
    d = {k: v.clone() for k, v in sc.matrix_window(2, 977).items()}
    d["obs_mask"][1, 0] = 1                                                      # item 1 now observes its first frame ...
    d["latent_mask"][1, 0] = 0
    d["x0"][1, 0] = torch.rand(3, sc.S_, sc.S_, generator=torch.Generator().manual_seed(5)).cuda() * 2 - 1
    d["kinda_marg_mask"][0, 2] = 0                                               # ... item 0 marginalises none, and its frame 2 is latent
    d["latent_mask"][0, 2] = 1
    d["frame_indices"] = (d["frame_indices"] * 2 + 1).contiguous()
    bufs = ex._bufs[2, sc.T_]
    ptrs = {k: v.data_ptr() for k, v in bufs.items()}
    pre = _begin(ex, model, diff, BASE, d)
    assert pre[0] == g0 + 1 and ex.graphs == g0 + 1
    assert {k: v.data_ptr() for k, v in bufs.items()} == ptrs and torch.equal(bufs["frame_indices"], d["frame_indices"])
    got = ex.run(2).clone()
    _same(got, _eager(model, diff, BASE, d)[1], "the new contents")
    assert not sc.same(got, A)
    model.check_device_errors()
