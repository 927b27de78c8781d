"""No GPU: cfg_scale (classifier-free guidance on the observed frames, this project's extension) -- the keyword surface, the refusals that
need no engine, the scope that sets and restores the engine's scale (on a stand-in library), the float64 restatement of the combine
pass and the command line."""
import inspect

import numpy as np
import pytest
import torch

import video_diffusion_amd as vda
from cfg_restated import combine_fp64, rounding_bound
from video_diffusion_amd import _lib, gaussian_diffusion
from video_diffusion_amd.executor import WindowExecutor
from video_diffusion_amd.gaussian_diffusion import GaussianDiffusion
from video_diffusion_amd.script_util import create_gaussian_diffusion


# ---------------------------------------------------------------------------------------------------------------- surface
def test_keyword_surface():
    for f in (GaussianDiffusion.p_sample, GaussianDiffusion.ddim_sample, GaussianDiffusion.p_mean_variance,
              GaussianDiffusion.p_sample_loop, GaussianDiffusion.p_sample_loop_progressive, GaussianDiffusion.ddim_sample_loop,
              GaussianDiffusion.ddim_sample_loop_progressive, GaussianDiffusion.dpmpp_2m_sample_loop,
              GaussianDiffusion.dpmpp_2m_sample_loop_progressive, WindowExecutor.begin, WindowExecutor.sample_window):
        p = list(inspect.signature(f).parameters.values())
        assert p[-1].name == "cfg_scale" and p[-1].default == 1.0, f.__qualname__       # after the existing ones
    from video_diffusion_amd.video_sample import infer_video
    p = inspect.signature(infer_video).parameters["cfg_scale"]
    assert p.default == 1.0 and p.kind is inspect.Parameter.KEYWORD_ONLY
    # the steps that keep the parameter lists they were introduced with take their scale from the scope
    assert "cfg_scale" not in inspect.signature(GaussianDiffusion.dpmpp_2m_sample).parameters
    assert "cfg_scale" not in inspect.signature(GaussianDiffusion.ddim_reverse_sample).parameters
    assert "extension" in GaussianDiffusion.cfg_scale_scope.__doc__ and "dpmpp_2m_sample" in GaussianDiffusion.cfg_scale_scope.__doc__
    assert _lib.SIGNATURES["vd_set_cfg_scale"] == (_lib._I, [_lib._P, _lib._F])
    assert _lib.SIGNATURES["vd_cfg_scale"] == (_lib._F, [_lib._P])
    assert _lib.SIGNATURES["vd_op_cfg_combine"] == (_lib._I, [_lib._P, _lib._P, _lib._F, _lib._L, _lib._P, _lib._P])


def test_the_built_library_exports_the_entries_and_defaults_to_one():
    L = _lib.lib()
    for name in ("vd_set_cfg_scale", "vd_cfg_scale", "vd_op_cfg_combine"):
        assert hasattr(L, name)
    model, _ = vda.create_video_model_and_diffusion(**{**vda.video_model_and_diffusion_defaults(), **dict(
        T=4, image_size=32, num_channels=32, num_res_blocks=1, rp_alpha=4, rp_beta=4, rp_gamma=4)})
    assert L.vd_cfg_scale(model._handle) == 1.0
    for bad in (float("nan"), float("inf")):
        assert L.vd_set_cfg_scale(model._handle, bad) != 0 and b"finite" in L.vd_last_error()
    assert L.vd_set_cfg_scale(model._handle, -0.5) == 0 and L.vd_cfg_scale(model._handle) == -0.5
    assert L.vd_set_cfg_scale(model._handle, 1.0) == 0 and L.vd_cfg_scale(model._handle) == 1.0
    assert L.vd_cfg_scale(None) == 1.0


# ---------------------------------------------------------------------------------------------------------------- refusals
class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the engine was touched: {name}")


def test_refusals_that_need_no_engine(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: _Untouchable())
    diff = create_gaussian_diffusion(timestep_respacing="ddim10")
    x, t = torch.zeros(1, 2, 3, 8, 8), torch.tensor([3])
    model = _Untouchable()
    for f in (diff.p_sample, diff.p_mean_variance):
        with pytest.raises(NotImplementedError, match="return_attn_weights together with cfg_scale != 1"):
            f(model, x, t, model_kwargs={}, return_attn_weights=True, cfg_scale=2.0)
        with pytest.raises(NotImplementedError, match="use_gradient_method together with cfg_scale != 1"):
            f(model, x, t, model_kwargs={}, use_gradient_method=True, cfg_scale=0.0)
        with pytest.raises(ValueError, match="finite"):
            f(model, x, t, model_kwargs={}, cfg_scale=float("inf"))
    with pytest.raises(NotImplementedError, match="use_gradient_method together with cfg_scale != 1"):
        next(diff.p_sample_loop_progressive(model, (1, 2, 3, 8, 8), noise=x, model_kwargs=dict(observed_frames="x_0", x0=x), device="cpu",
                                            use_gradient_method=True, cfg_scale=2.0))
    with pytest.raises(ValueError, match="finite"):
        diff.ddim_sample(model, x, t, model_kwargs={}, cfg_scale=float("nan"))
    with pytest.raises(ValueError, match="finite"):
        diff.cfg_scale_scope(model, float("nan"))
    for opt in ("prefix_cache", "suffix_skip"):
        ex = WindowExecutor.__new__(WindowExecutor)                              # (the constructor needs a device; begin() must refuse before it does)
        ex.prefix_cache, ex.suffix_skip = opt == "prefix_cache", opt == "suffix_skip"
        with pytest.raises(NotImplementedError, match=f"{opt} together with cfg_scale != 1"):
            ex.begin(x, {}, cfg_scale=2.0)
        with pytest.raises(NotImplementedError, match=f"{opt} together with cfg_scale != 1"):
            ex.sample_window(x, {}, cfg_scale=-1.0)
        with pytest.raises(ValueError, match="finite"):
            ex.begin(x, {}, cfg_scale=float("inf"))


# ---------------------------------------------------------------------------------------------------------------- the scope
class _FakeLib:
    """Stand-in for the library: the engine's scale and every call that set it."""

    def __init__(self):
        self.scale, self.sets = 1.0, []

    def vd_set_cfg_scale(self, handle, w):
        self.sets.append(w)
        self.scale = w
        return 0

    def vd_cfg_scale(self, handle):
        return self.scale


class _FakeModel:
    _handle = 17


def test_scope_sets_the_scale_and_puts_back_what_it_found(monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    model = _FakeModel()
    with gaussian_diffusion._cfg_scope(model, 1.0):
        pass
    assert fake.sets == []                                                       # w = 1: the engine is not touched
    with gaussian_diffusion._cfg_scope(model, 2.0):
        assert fake.scale == 2.0
    assert fake.scale == 1.0 and fake.sets == [2.0, 1.0]
    with pytest.raises(RuntimeError, match="boom"):
        with gaussian_diffusion._cfg_scope(model, 0.0):
            assert fake.scale == 0.0
            raise RuntimeError("boom")
    assert fake.scale == 1.0
    # the public scope, and a keyword inside it: back to the scope's value, then to 1
    diff = create_gaussian_diffusion(timestep_respacing="ddim10")
    model._bound_schedule = diff                                                 # (bound already: no upload)
    with diff.cfg_scale_scope(model, 3.0):
        assert fake.scale == 3.0
        with gaussian_diffusion._cfg_scope(model, 1.0):
            assert fake.scale == 3.0                                             # the keyword's default leaves the scope's value
        with gaussian_diffusion._cfg_scope(model, 0.5):
            assert fake.scale == 0.5
        assert fake.scale == 3.0
    assert fake.scale == 1.0


# ---------------------------------------------------------------------------------------------------------------- restatement
def test_restatement_known_answers():
    c = np.array([1.0, 0.5, -0.25, 0.0, np.inf, 1e30], np.float32)
    u = np.array([0.0, 0.5, 0.75, -0.0, 1.0, -1e30], np.float32)
    g, d, ok = combine_fp64(c, u, 2.0)
    assert ok.tolist() == [True, True, True, True, False, True]
    assert g[:4].tolist() == [2.0, 0.5, -1.25, 0.0] and g[5] == np.float64(np.float32(-1e30)) + 2.0 * np.float64(np.float32(1e30) - np.float32(-1e30))
    assert d.dtype == np.float32 and d[:4].tolist() == [1.0, 0.0, -1.0, 0.0]
    for w in (0.0, 1.0, 1.5, 7.5, -1.0):
        g, d, ok = combine_fp64(c, u, w)
        if w == 0.0:
            assert np.array_equal(g[ok], u[ok].astype(np.float64))
        if w == 1.0:
            assert np.array_equal(g[:4], c[:4].astype(np.float64))
        lim = rounding_bound(u, w, d)
        assert (lim[ok] >= 2.0 ** -126).all() and np.isfinite(lim[ok]).all()
        # the float32 fma of the same operands (float64 product and sum are exact enough to round once) stays inside the bound
        f32 = (u[ok].astype(np.float64) + np.float64(np.float32(w)) * d[ok].astype(np.float64)).astype(np.float32)
        assert (np.abs(f32.astype(np.float64) - g[ok]) <= lim[ok]).all()


# ---------------------------------------------------------------------------------------------------------------- command line
class _Recording:
    """Stand-in sampler (no GPU here), as tests/test_host_logic.py's: records what reaches it, leaves x unchanged."""
    num_timesteps = 2

    def __init__(self):
        self.calls = []

    def p_sample(self, model, x, t, **kw):
        self.calls.append(("p_sample", kw.get("cfg_scale")))
        return {"sample": x}

    def ddim_sample(self, model, x, t, eta=0.0, **kw):
        self.calls.append(("ddim", kw.get("cfg_scale")))
        return {"sample": x}


def _job(tmp_path, argv):
    from video_diffusion_amd import video_sample
    args = video_sample.build_parser().parse_args(
        ["--inference_mode", "autoreg", "--T", "6", "--max_frames", "4", "--obs_length", "2", "--step_size", "2", "--batch_size", "2",
         "--num_videos", "2", "--timestep_respacing", "ddim2", "--image_size", "32", "--num_channels", "32", "--num_res_blocks", "1",
         "--eval_dir", str(tmp_path / "out")] + argv)
    diff = _Recording()

    def create(**kw):
        model, _ = vda.create_video_model_and_diffusion(**kw)
        return model, diff

    return video_sample.run(args, create=create, device=torch.device("cpu")), diff, args


def test_command_line_option_reaches_the_step_and_names_the_run_directory(tmp_path):
    from video_diffusion_amd import video_sample
    ap = video_sample.build_parser()
    assert ap.parse_args([]).cfg_scale == 1.0 and ap.parse_args(["--cfg_scale", "2.0"]).cfg_scale == 2.0
    assert ap.parse_args(["--cfg_scale", "-0.5"]).cfg_scale == -0.5
    with pytest.raises(SystemExit):
        ap.parse_args(["--cfg_scale", "strong"])
    out, diff, _ = _job(tmp_path / "a", ["--cfg_scale", "2.0"])
    assert out.name == "autoreg_4_2_6_2_cfg2"
    assert diff.calls == [("p_sample", 2.0)] * 4                                 # two windows of two steps
    out1, diff1, _ = _job(tmp_path / "b", ["--cfg_scale", "1.0"])
    out0, diff0, _ = _job(tmp_path / "c", [])
    assert out1.name == out0.name == "autoreg_4_2_6_2"                           # byte for byte the name without the option
    assert diff1.calls == diff0.calls == [("p_sample", 1.0)] * 4
    out_d, diff_d, _ = _job(tmp_path / "d", ["--sampler", "ddim", "--cfg_scale", "1.5"])
    assert out_d.name == "autoreg_4_2_6_2_ddim_cfg1.5" and diff_d.calls == [("ddim", 1.5)] * 4
    from argparse import Namespace
    assert video_sample.run_postfix(Namespace()) == "" and video_sample.run_postfix(Namespace(sampler="dpmpp_2m", cfg_scale=-0.5)) == "_dpmpp_2m_cfg-0.5"
