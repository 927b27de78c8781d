"""No GPU: pixel-mask inpainting (this project's extension, RePaint) -- repaint_schedule against the walk written from the paper's
nested loops, the mask validation and the gather of a video-sized mask per window, the refusals that need no engine, the scope on a
stand-in library, and the float32 restatement of the merge and the jump against its own float64 inside the derived bounds."""
import inspect

import numpy as np
import pytest
import torch

from known_region_restated import (jump_rows, known_merge_bound, known_merge_f32, known_merge_fp64, merged, q_jump_bound, q_jump_f32,
                                   q_jump_fp64, repaint_schedule_ref, repaint_steps)
from step_nll_restated import F, ratio, tables
from video_diffusion_amd import _lib, video_sample
from video_diffusion_amd.executor import WindowExecutor
from video_diffusion_amd.gaussian_diffusion import GaussianDiffusion, check_known_region
from video_diffusion_amd.respace import repaint_schedule
from video_diffusion_amd.script_util import create_gaussian_diffusion


# ---------------------------------------------------------------------------------------------------------------- the schedule
def test_repaint_schedule():
    assert repaint_schedule(3, 2, 2) == [("step", 3), ("step", 2), ("jump", 2), ("jump", 3), ("step", 3), ("step", 2), ("step", 1), ("step", 0)]
    for t_start in range(0, 14):
        assert repaint_schedule(t_start, 3, 1) == [("step", t) for t in range(t_start, -1, -1)]          # r = 1: the plain descent
        for j in range(1, 7):
            for r in range(1, 5):
                ops = repaint_schedule(t_start, j, r)
                assert ops == repaint_schedule_ref(t_start, j, r), (t_start, j, r)
                assert sum(op == "step" for op, _ in ops) == repaint_steps(t_start, j, r)
                assert sum(op == "jump" for op, _ in ops) == repaint_steps(t_start, j, r) - (t_start + 1)
                assert all(0 <= t <= t_start for _, t in ops) and ops[-1] == ("step", 0)
                level = t_start                              # the walk is connected: a step at t takes x_t to x_{t-1}, a jump at t x_{t-1} to x_t
                for op, t in ops:
                    assert t == (level if op == "step" else level + 1), (t_start, j, r)
                    level = t - 1 if op == "step" else t
                assert level == -1
    for bad in (dict(jump_length=0), dict(jump_length=1.5), dict(n_resample=0), dict(n_resample=-1), dict(t_start=-1)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            repaint_schedule(**{**dict(t_start=5, jump_length=2, n_resample=2), **bad})


# ---------------------------------------------------------------------------------------------------------------- validation, gather
def test_mask_validation():
    src = torch.zeros(2, 3, 3, 4, 4)
    for m in (torch.ones(2, 3, 1, 4, 4), torch.ones(2, 3, 4, 4, dtype=torch.bool), torch.ones(2, 3, 4, 4, dtype=torch.uint8),
              torch.zeros(2, 3, 4, 4, dtype=torch.float64)):
        s, mm = check_known_region(src, m)
        assert s.dtype == mm.dtype == torch.float32 and mm.shape == (2, 3, 4, 4) and s.shape == src.shape
    for m, what in ((torch.full((2, 3, 4, 4), 0.5), "0 and 1 only"), (torch.full((2, 3, 4, 4), 2, dtype=torch.uint8), "0 and 1 only"),
                    (torch.ones(2, 3, 4, 4, dtype=torch.int64), "bool, uint8 or float"), (torch.ones(2, 3, 3, 4, 4), "known_mask must be"),
                    (torch.ones(3, 4, 4), "known_mask must be"), (np.ones((2, 3, 4, 4)), "known_mask must be")):
        with pytest.raises(ValueError, match=what):
            check_known_region(src, m)
    with pytest.raises(ValueError, match="known_src must be"):
        check_known_region(torch.zeros(2, 3, 1, 4, 4), torch.ones(2, 3, 4, 4))


def test_video_mask_is_gathered_per_window_like_x0():
    B, T, H, W = 2, 7, 4, 5
    g = torch.Generator().manual_seed(1)
    batch = torch.rand(B, T, 3, H, W, generator=g)
    mask3 = torch.rand(T, H, W, generator=g) < 0.5
    m, src = video_sample.video_known_region(batch, mask3 * 7)                   # nonzero = known
    assert m.shape == (B, T, H, W) and m.dtype == torch.float32 and torch.equal(m[0], mask3.float()) and torch.equal(m[1], m[0])
    assert torch.equal(src, batch)
    mask4 = torch.rand(B, T, H, W, generator=g) < 0.5
    other = -batch
    m, src = video_sample.video_known_region(batch, mask4, other)
    assert torch.equal(m, mask4.float()) and torch.equal(src, other)
    # per-item frame indices (the adaptive-* modes): item i's rows are its own frames, in the window's order
    fi = torch.tensor([[0, 5, 2, 3], [6, 1, 4, 2]])
    gm, gs = video_sample.gather_window(m, fi), video_sample.gather_window(src, fi)
    assert gm.shape == (B, 4, H, W) and gs.shape == (B, 4, 3, H, W)
    for i in range(B):
        for w, f in enumerate(fi[i].tolist()):
            assert torch.equal(gm[i, w], mask4[i, f].float()) and torch.equal(gs[i, w], other[i, f])
    # the shared-index form infer_video builds for the other modes is the same gather
    same = torch.tensor([1, 2, 6]).repeat(B, 1)
    assert torch.equal(video_sample.gather_window(src, same), src[:, [1, 2, 6]])
    check_known_region(gs, gm)
    for bad in (torch.ones(H, W), torch.ones(B, T, 1, H, W), torch.ones(T + 1, H, W)):
        with pytest.raises(ValueError, match="known_mask must be"):
            video_sample.video_known_region(batch, bad)
    with pytest.raises(ValueError, match="known_video must be"):
        video_sample.video_known_region(batch, mask3, batch[:, :3])


# ---------------------------------------------------------------------------------------------------------------- refusals
class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the engine was touched: {name}")


def test_refusals_that_need_no_engine(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: _Untouchable())
    diff = create_gaussian_diffusion(timestep_respacing="ddim10")
    batch, mask = torch.zeros(1, 4, 3, 8, 8), torch.ones(4, 8, 8)
    model = _Untouchable()
    for opt in ("use_gradient_method", "prefix_cache", "suffix_skip"):
        with pytest.raises(NotImplementedError, match=f"{opt} together with known_mask"):
            video_sample.infer_video("autoreg", model, diff, batch, 4, 2, known_mask=mask, **{opt: True})
    with pytest.raises(NotImplementedError, match="n_resample > 1 together with save_all_timesteps"):
        video_sample.infer_video("autoreg", model, diff, batch, 4, 2, known_mask=mask, n_resample=2, save_all_timesteps=True)
    with pytest.raises(ValueError, match="jump_length"):
        video_sample.infer_video("autoreg", model, diff, batch, 4, 2, known_mask=mask, jump_length=0)
    with pytest.raises(ValueError, match="known_mask must be"):
        video_sample.infer_video("autoreg", model, diff, batch, 4, 2, known_mask=torch.ones(8, 8))
    x = torch.zeros(1, 2, 3, 8, 8)
    for opt in ("prefix_cache", "suffix_skip"):
        ex = WindowExecutor.__new__(WindowExecutor)
        ex.prefix_cache, ex.suffix_skip, ex.model = opt == "prefix_cache", opt == "suffix_skip", object()
        with pytest.raises(NotImplementedError, match=f"{opt} together with a known region"):
            ex.begin(x, {}, known_src=x, known_mask=torch.ones(1, 2, 8, 8))
    ex = WindowExecutor.__new__(WindowExecutor)
    ex.prefix_cache = ex.suffix_skip = False
    ex.model = object()
    with pytest.raises(NotImplementedError, match="ddim_reverse' together with a known region"):
        ex.begin(x, {}, sampler="ddim_reverse", known_src=x, known_mask=torch.ones(1, 2, 8, 8))
    with pytest.raises(ValueError, match="given together"):
        ex.begin(x, {}, known_src=x)
    with pytest.raises(ValueError, match="0 and 1 only"):
        ex.begin(x, {}, known_src=x, known_mask=torch.full((1, 2, 8, 8), 0.25))
    with pytest.raises(ValueError, match="against a window"):
        ex.begin(x, {}, known_src=torch.zeros(1, 3, 3, 8, 8), known_mask=torch.ones(1, 3, 8, 8))
    # the keyword surface
    sig = inspect.signature(video_sample.infer_video).parameters
    for name, default in (("known_mask", None), ("known_video", None), ("jump_length", 1), ("n_resample", 1)):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == default
    p = inspect.signature(GaussianDiffusion.repaint_sample_loop).parameters
    assert list(p) == ["self", "model", "shape", "known_src", "known_mask", "sampler", "jump_length", "n_resample", "noise", "clip_denoised",
                       "model_kwargs", "eta", "cfg_scale", "progress"]
    assert list(inspect.signature(GaussianDiffusion.q_jump).parameters) == ["self", "x", "t", "latent_mask", "noise", "model"]
    for name in ("vd_set_known_region", "vd_known_region", "vd_known_merge", "vd_set_jump_rows", "vd_q_jump", "vd_window_jump"):
        assert name in _lib.SIGNATURES
    args = video_sample.build_parser().parse_args(["--known_mask", "m.npy", "--n_resample", "3", "--jump_length", "2"])
    assert (args.known_mask, args.known_videos, args.jump_length, args.n_resample) == ("m.npy", None, 2, 3)
    assert video_sample.run_postfix(args) == "_known_j2r3"
    plain = video_sample.build_parser().parse_args([])
    assert (plain.known_mask, plain.jump_length, plain.n_resample) == (None, 1, 1) and video_sample.run_postfix(plain) == ""


class _FakeLib:
    """Stand-in for the library: the region the engine holds, and every call that set it."""

    def __init__(self):
        self.region, self.sets = None, []

    def vd_set_known_region(self, handle, src, mask, noise, seed, offset):
        self.region = None if src is None else (src.value, mask.value, None if noise is None else noise.value)
        self.sets.append(self.region)
        return 0


class _FakeModel:
    _handle = 17
    device = torch.device("cpu")


def test_scope_sets_restores_and_nests(monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    model = _FakeModel()
    diff = create_gaussian_diffusion(timestep_respacing="ddim10")
    model._bound_schedule = diff                                                 # (bound already: no upload)
    a, b = torch.zeros(1, 2, 3, 4, 4), torch.ones(1, 2, 3, 4, 4)
    m = torch.ones(1, 2, 1, 4, 4, dtype=torch.bool)
    with diff.known_region_scope(model, a, m):
        outer = fake.region
        assert outer is not None and outer[2] is None and outer[0] == model._known_region["src"].data_ptr()
        with diff.known_region_scope(model, b, m, known_noise=a):
            assert fake.region[0] == model._known_region["src"].data_ptr() != outer[0]
            assert torch.equal(model._known_region["src"], b) and model._known_region["mask"].shape == (1, 2, 4, 4)
        assert fake.region == outer and torch.equal(model._known_region["src"], a)
    assert fake.region is None and model._known_region is None
    with pytest.raises(RuntimeError, match="boom"):
        with diff.known_region_scope(model, a, m):
            raise RuntimeError("boom")
    assert fake.region is None and model._known_region is None
    before = len(fake.sets)
    with pytest.raises(ValueError, match="0 and 1 only"):
        with diff.known_region_scope(model, a, m.float() * 0.5):
            pass
    assert len(fake.sets) == before
    with diff.known_region_scope(model, a, m):
        for call, what in ((lambda: diff.ddim_reverse_sample(model, a, torch.tensor([1])), "ddim_reverse_sample"),
                           (lambda: diff.p_sample(model, a, torch.tensor([1]), denoised_fn=lambda v: v), "denoised_fn"),
                           (lambda: diff.ddim_sample(model, a, torch.tensor([1]), denoised_fn=lambda v: v), "denoised_fn"),
                           (lambda: diff.dpmpp_2m_sample(model, a, torch.tensor([1]), denoised_fn=lambda v: v), "denoised_fn"),
                           (lambda: diff.p_sample(model, a, torch.tensor([1]), use_gradient_method=True), "use_gradient_method"),
                           (lambda: diff.p_mean_variance(model, a, torch.tensor([1]), use_gradient_method=True), "use_gradient_method")):
            with pytest.raises(NotImplementedError, match=f"{what} inside known_region_scope"):
                call()
    assert "extension" in GaussianDiffusion.known_region_scope.__doc__ and "Draw order" in GaussianDiffusion.known_region_scope.__doc__


def test_jump_rows_are_taken_in_float64():
    diff = create_gaussian_diffusion(timestep_respacing="")
    sa, sb = diff._jump_rows()
    assert sa.dtype == sb.dtype == np.float64 and np.array_equal(sa, np.sqrt(1.0 - diff.betas)) and np.array_equal(sb, np.sqrt(diff.betas))
    r = jump_rows(diff.betas)
    assert np.array_equal(r[0], sa.astype(F)) and np.array_equal(r[1], sb.astype(F))
    # why the rows are uploaded: sqrt(1 - float32(alpha)) at beta = 1e-4 is off by far more than a float32 rounding of sqrt(beta)
    lossy = np.sqrt(F(1.0) - (1.0 - diff.betas).astype(F))
    assert abs(float(lossy[0]) - sb[0]) / sb[0] > 100 * 2.0 ** -24 and abs(float(r[1][0]) - sb[0]) / sb[0] < 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("hw", [64, 49])
def test_restatement_against_its_own_float64(hw):
    diff = create_gaussian_diffusion(timestep_respacing="ddim250")
    tab, N = tables(diff), diff.num_timesteps
    rows = jump_rows(diff.betas)
    rs = np.random.RandomState(3)
    B, T = 3, 4
    g, z = rs.randn(B, T, 3, hw).astype(F), rs.randn(B, T, 3, hw).astype(F)
    k = rs.uniform(-1, 1, (B, T, 3, hw)).astype(F)
    mask = (rs.rand(B, T, hw) < 0.5).astype(F)
    lat = np.ones((B, T), F)
    lat[:, 1] = 0
    sel = merged(mask, lat)
    assert sel.any() and not sel[:, 1].any()
    for t in ([0, 1, N - 1], [N // 2, 0, 2], [1, N, -1]):
        got = known_merge_f32(tab, g, k, mask, lat, t, z)
        want, lim = known_merge_bound(tab, g, k, mask, lat, t, z)
        assert np.array_equal(np.nan_to_num(want, nan=7.0), np.nan_to_num(known_merge_fp64(tab, g, k, mask, lat, t, z), nan=7.0))
        r = ratio(got, want, lim)
        assert (r <= 1.0).all() and (lim[~sel] == 0).all(), (t, float(r.max()))
        for b, tv in enumerate(t):
            if not 0 <= tv < N:
                assert np.isnan(got[b]).all() and np.isnan(want[b]).all()
                continue
            assert np.array_equal(got[b][~sel[b]], g[b][~sel[b]])
            if tv == 0:
                assert np.array_equal(got[b][sel[b]], k[b][sel[b]])
            else:                                                                # q_sample at t - 1, not at t
                sa, s1 = np.float64(tab["sa"][tv - 1]), np.float64(tab["s1"][tv - 1])
                assert np.allclose(want[b][sel[b]], (sa * k[b] + s1 * z[b])[sel[b]], rtol=1e-12, atol=0)
        gj = q_jump_f32(rows, g, lat, t, z)
        wj, lj = q_jump_bound(rows, g, lat, t, z)
        assert np.array_equal(np.nan_to_num(wj, nan=7.0), np.nan_to_num(q_jump_fp64(rows, g, lat, t, z), nan=7.0))
        r = ratio(gj, wj, lj)
        assert (r <= 1.0).all(), (t, float(r.max()))
        for b, tv in enumerate(t):
            if 0 <= tv < N:
                assert np.array_equal(gj[b, 1], g[b, 1]) and not np.array_equal(gj[b, 0], g[b, 0])
                assert np.allclose(wj[b, 0], np.sqrt(1 - diff.betas[tv]) * g[b, 0] + np.sqrt(diff.betas[tv]) * z[b, 0], rtol=1e-6, atol=1e-7)
            else:
                assert np.isnan(gj[b]).all()
    # a seeded mistake is caught: noising to t instead of t - 1 leaves the bound
    wrong = known_merge_f32(tab, g, k, mask, lat, [3, 3, 3], z)
    want, lim = known_merge_bound(tab, g, k, mask, lat, [2, 2, 2], z)
    assert (ratio(wrong, want, lim)[sel] > 1.0).any()
