"""No GPU: guidance rescale and dynamic thresholding (this project's extensions) -- the float64 restatements against the textbook formula
and torch.quantile, the scope that sets and restores the engine's two values (on a stand-in library), the validation that needs no
engine, the command line, and the built library's entries."""
import inspect
from argparse import Namespace

import numpy as np
import pytest
import torch

import video_diffusion_amd as vda
from guidance_restated import rescale_factor_fp64, rescale_fp64, threshold_fp64, threshold_s_fp64
from video_diffusion_amd import _lib, gaussian_diffusion
from video_diffusion_amd.gaussian_diffusion import GaussianDiffusion
from video_diffusion_amd.script_util import create_gaussian_diffusion


# ---------------------------------------------------------------------------------------------------------------- restatements
def test_rescale_restatement_equals_the_textbook_formula():
    """Lin et al. 2023, eq. 15-16: x_rescaled = x_cfg std(x_pos) / std(x_cfg), x_final = phi x_rescaled + (1 - phi) x_cfg, i.e.
    g (phi std_c / std_g + 1 - phi), with the standard deviations over the latent frames of each item."""
    g = np.random.default_rng(3)
    B, T, E = 3, 5, 48
    c = (g.standard_normal((B, T, E)) * 0.7 + 0.2).astype(np.float32)
    out_g = (c * 1.8 + g.standard_normal((B, T, E)) * 0.3).astype(np.float32)
    lat = np.array([[0, 0, 1, 1, 1], [1, 0, 0, 0, 0], [0, 0, 0, 0, 0]], np.float32)
    for phi in (0.0, 0.3, 0.7, 1.0):
        out, f = rescale_fp64(c, out_g, lat, phi)
        assert f[2] == 1.0 and np.array_equal(out[2], out_g[2].astype(np.float64))         # no latent frame
        for b in (0, 1):
            m = lat[b] == 1
            sc, sg = c[b][m].astype(np.float64).std(), out_g[b][m].astype(np.float64).std()
            book = out_g[b][m].astype(np.float64) * (phi * sc / sg + 1.0 - phi)
            np.testing.assert_allclose(out[b][m], book, rtol=2.0 ** -23, atol=0)            # (the restatement rounds f to float32: 2^-24)
            np.testing.assert_allclose(f[b], phi * sc / sg + 1.0 - phi, rtol=1e-14)
            assert np.array_equal(out[b][~m], out_g[b][~m].astype(np.float64))              # other frames pass through
        if phi == 0.0:
            assert (f == 1.0).all()
    # sigma_g = 0: the factor is 1, not a division by zero
    flat = np.full((1, 2, 8), 0.25, np.float32)
    assert rescale_factor_fp64(c[:1, :2, :8], flat, np.ones((1, 2)), 0.7)[0] == 1.0


@pytest.mark.parametrize("n", [1, 2, 7, 200, 4097])
@pytest.mark.parametrize("p", [0.5, 0.995, 1.0, 0.123])
def test_threshold_restatement_equals_torch_quantile(n, p):
    """s before the max is torch.quantile(|x|.double(), p) (linear interpolation).  torch evaluates the interpolation as a lerp, which
    for a weight >= 0.5 runs from the upper value down: the same real number, rounded elsewhere -- two float64 roundings apart at most."""
    g = np.random.default_rng(n)
    x = (g.standard_normal((2, 1, n)) * 3).astype(np.float32)
    lat = np.ones((2, 1), np.float32)
    s, s32 = threshold_s_fp64(x, lat, p)
    for b in range(2):
        want = float(torch.quantile(torch.from_numpy(np.abs(x[b])).double().flatten(), p))
        assert abs(s[b] - want) <= 4 * np.spacing(want), (s[b], want)
        assert s32[b] == max(np.float32(s[b]), np.float32(1))
    if p == 1.0:
        assert s[0] == np.abs(x[0]).max()
    if n == 1:
        assert s[0] == abs(x[0, 0, 0])


def test_threshold_restatement_known_answers():
    x = np.array([[[0.5, -3.0, 2.0, -0.0], [9.0, -9.0, np.nan, 0.1]]], np.float32)          # frame 1 is observed
    lat = np.array([[1, 0]], np.float32)
    out, s32 = threshold_fp64(x, lat, 1.0)
    assert s32[0] == 3.0 and np.allclose(out[0, 0], [0.5 / 3, -1.0, 2.0 / 3, 0.0])
    assert out[0, 1, :2].tolist() == [1.0, -1.0] and np.isnan(out[0, 1, 2]) and out[0, 1, 3] == np.float64(np.float32(0.1))
    out, s32 = threshold_fp64(x, lat, 0.5)                                                   # |x| sorted 0 .5 2 3: h = 1.5 -> 1.25
    assert s32[0] == 1.25 and np.allclose(out[0, 0], [0.4, -1.0, 1.0, 0.0])
    small = np.array([[[0.5, -0.9, 0.0, 1.0]]], np.float32)                                  # max <= 1: the static clamp
    out, s32 = threshold_fp64(small, np.ones((1, 1)), 0.995)
    assert s32[0] == 1.0 and np.array_equal(out[0, 0], small[0, 0].astype(np.float64))
    bad = x.copy()
    bad[0, 0, 1] = np.inf                                                                    # a latent value that is not finite
    out, s32 = threshold_fp64(bad, lat, 0.5)
    assert np.isnan(s32[0]) and np.isnan(out[0, 0]).all() and out[0, 1, 0] == 1.0
    out, s32 = threshold_fp64(x, np.zeros((1, 2)), 0.5)                                      # no latent frame
    assert s32[0] == 1.0 and out[0, 0].tolist() == [0.5, -1.0, 1.0, 0.0]


# ---------------------------------------------------------------------------------------------------------------- the scope
class _FakeLib:
    """Stand-in for the library: the engine's two values and every call that set them."""

    def __init__(self):
        self.phi, self.p, self.sets = 0.0, 0.0, []

    def vd_set_guidance_rescale(self, handle, v):
        self.sets.append(("phi", v))
        self.phi = v
        return 0

    def vd_guidance_rescale(self, handle):
        return self.phi

    def vd_set_dynamic_threshold(self, handle, v):
        self.sets.append(("p", v))
        self.p = v
        return 0

    def vd_dynamic_threshold(self, handle):
        return self.p


class _FakeModel:
    _handle = 17


def test_scope_sets_restores_and_nests(monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    model = _FakeModel()
    diff = create_gaussian_diffusion(timestep_respacing="ddim10")
    model._bound_schedule = diff                                                 # (bound already: no upload)
    with diff.guidance_scope(model, cfg_rescale=0.7, dynamic_threshold=0.995):
        assert (fake.phi, fake.p) == (0.7, 0.995)
        with diff.guidance_scope(model, dynamic_threshold=0.5):                  # an inner scope sets both: the rescale is off inside
            assert (fake.phi, fake.p) == (0.0, 0.5)
        assert (fake.phi, fake.p) == (0.7, 0.995)
        with diff.guidance_scope(model):                                         # the defaults: both off
            assert (fake.phi, fake.p) == (0.0, 0.0)
        assert (fake.phi, fake.p) == (0.7, 0.995)
    assert (fake.phi, fake.p) == (0.0, 0.0)
    with pytest.raises(RuntimeError, match="boom"):
        with diff.guidance_scope(model, cfg_rescale=1.0):
            assert (fake.phi, fake.p) == (1.0, 0.0)
            raise RuntimeError("boom")
    assert (fake.phi, fake.p) == (0.0, 0.0)
    p = inspect.signature(GaussianDiffusion.guidance_scope).parameters
    assert list(p) == ["self", "model", "cfg_rescale", "dynamic_threshold"]
    assert p["cfg_rescale"].default == 0.0 and p["dynamic_threshold"].default is None
    assert "extension" in GaussianDiffusion.guidance_scope.__doc__ and "latent" in GaussianDiffusion.guidance_scope.__doc__


# ---------------------------------------------------------------------------------------------------------------- validation
class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the engine was touched: {name}")


def test_validation_touches_no_engine(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: _Untouchable())
    from video_diffusion_amd.video_sample import infer_video
    diff = create_gaussian_diffusion(timestep_respacing="ddim10")
    model = _Untouchable()
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"cfg_rescale.*\[0, 1\]"):
            diff.guidance_scope(model, cfg_rescale=bad)
        with pytest.raises(ValueError, match="cfg_rescale"):
            infer_video("autoreg", model, diff, torch.zeros(1, 4, 3, 8, 8), 4, 2, cfg_rescale=bad)
    for bad in (0.0, -0.5, 1.0001, float("nan")):
        with pytest.raises(ValueError, match=r"dynamic_threshold.*\(0, 1\]"):
            diff.guidance_scope(model, dynamic_threshold=bad)
        with pytest.raises(ValueError, match="dynamic_threshold"):
            infer_video("autoreg", model, diff, torch.zeros(1, 4, 3, 8, 8), 4, 2, dynamic_threshold=bad)
    assert gaussian_diffusion._check_guidance(0.5, None) == (0.5, 0.0) and gaussian_diffusion._check_guidance(0, 1) == (0.0, 1.0)
    for opt in ("use_gradient_method", "prefix_cache", "suffix_skip"):
        with pytest.raises(NotImplementedError, match=f"{opt} together with cfg_rescale / dynamic_threshold"):
            infer_video("autoreg", model, diff, torch.zeros(1, 4, 3, 8, 8), 4, 2, dynamic_threshold=0.9, **{opt: True})
    sig = inspect.signature(infer_video).parameters
    for name, default in (("cfg_rescale", 0.0), ("dynamic_threshold", None)):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == default


# ---------------------------------------------------------------------------------------------------------------- command line
class _Recording:
    """Stand-in sampler (no GPU here): records the guidance scope it runs in and what reaches the step."""
    num_timesteps = 2

    def __init__(self):
        self.calls, self.scopes, self.inside = [], [], None

    def guidance_scope(self, model, cfg_rescale=0.0, dynamic_threshold=None):
        import contextlib

        @contextlib.contextmanager
        def scope():
            self.scopes.append((cfg_rescale, dynamic_threshold))
            self.inside = (cfg_rescale, dynamic_threshold)
            try:
                yield
            finally:
                self.inside = None
        return scope()

    def p_sample(self, model, x, t, **kw):
        self.calls.append(("p_sample", kw.get("cfg_scale"), self.inside))
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

    return video_sample.run(args, create=create, device=torch.device("cpu")), diff


def test_command_line_options_reach_the_scope_and_name_the_run_directory(tmp_path):
    from video_diffusion_amd import video_sample
    ap = video_sample.build_parser()
    d = ap.parse_args([])
    assert d.cfg_rescale == 0.0 and d.dynamic_threshold is None
    a = ap.parse_args(["--cfg_rescale", "0.7", "--dynamic_threshold", "0.995"])
    assert a.cfg_rescale == 0.7 and a.dynamic_threshold == 0.995
    with pytest.raises(SystemExit):
        ap.parse_args(["--dynamic_threshold", "high"])
    out, diff = _job(tmp_path / "a", ["--cfg_scale", "2.0", "--cfg_rescale", "0.7", "--dynamic_threshold", "0.995"])
    assert out.name == "autoreg_4_2_6_2_cfg2_resc0.7_dt0.995"
    assert diff.scopes == [(0.7, 0.995)]                                         # one scope around the whole of infer_video's work
    assert diff.calls == [("p_sample", 2.0, (0.7, 0.995))] * 4                   # two windows of two steps, all inside it
    out_t, diff_t = _job(tmp_path / "b", ["--dynamic_threshold", "1.0"])
    assert out_t.name == "autoreg_4_2_6_2_dt1" and diff_t.calls == [("p_sample", 1.0, (0.0, 1.0))] * 4
    out0, diff0 = _job(tmp_path / "c", [])
    assert out0.name == "autoreg_4_2_6_2"                                        # a default run keeps its directory name
    assert diff0.scopes == [] and diff0.calls == [("p_sample", 1.0, None)] * 4   # and enters no scope
    assert video_sample.run_postfix(Namespace()) == ""
    assert video_sample.run_postfix(Namespace(sampler="ddim", cfg_scale=1.5, cfg_rescale=1.0, dynamic_threshold=None)) == "_ddim_cfg1.5_resc1"


# ---------------------------------------------------------------------------------------------------------------- the library
def test_signature_rows():
    I, P, F, L = _lib._I, _lib._P, _lib._F, _lib._L  # noqa: E741
    assert _lib.SIGNATURES["vd_set_guidance_rescale"] == (I, [P, F]) and _lib.SIGNATURES["vd_guidance_rescale"] == (F, [P])
    assert _lib.SIGNATURES["vd_set_dynamic_threshold"] == (I, [P, F]) and _lib.SIGNATURES["vd_dynamic_threshold"] == (F, [P])
    assert _lib.SIGNATURES["vd_op_cfg_rescale"] == (I, [P, P, F, P, I, I, L, F, P, P, P])
    assert _lib.SIGNATURES["vd_op_dynamic_threshold"] == (I, [P, P, I, I, L, F, P, P, P])


def test_the_built_library_exports_the_entries_and_defaults_to_off():
    L = _lib.lib()
    for name in ("vd_set_guidance_rescale", "vd_guidance_rescale", "vd_set_dynamic_threshold", "vd_dynamic_threshold",
                 "vd_op_cfg_rescale", "vd_op_dynamic_threshold"):
        assert hasattr(L, name)
    model, _ = vda.create_video_model_and_diffusion(**{**vda.video_model_and_diffusion_defaults(), **dict(
        T=4, image_size=32, num_channels=32, num_res_blocks=1, rp_alpha=4, rp_beta=4, rp_gamma=4)})
    h = model._handle
    assert L.vd_guidance_rescale(h) == 0.0 and L.vd_dynamic_threshold(h) == 0.0
    for bad in (-0.25, 1.5, float("nan")):
        assert L.vd_set_guidance_rescale(h, bad) != 0 and b"[0, 1]" in L.vd_last_error()
        assert L.vd_set_dynamic_threshold(h, bad) != 0 and b"(0, 1]" in L.vd_last_error()
    assert L.vd_guidance_rescale(h) == 0.0 and L.vd_dynamic_threshold(h) == 0.0
    assert L.vd_set_guidance_rescale(h, 0.5) == 0 and L.vd_guidance_rescale(h) == 0.5
    assert L.vd_set_dynamic_threshold(h, 1.0) == 0 and L.vd_dynamic_threshold(h) == 1.0
    assert L.vd_set_guidance_rescale(h, 0.0) == 0 and L.vd_set_dynamic_threshold(h, 0.0) == 0
    assert L.vd_guidance_rescale(None) == 0.0 and L.vd_dynamic_threshold(None) == 0.0
