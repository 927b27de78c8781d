"""No GPU: diffusion posterior sampling (this project's extension, DPS) -- the float64 restatement's cotangent against torch autograd
of ||y - measure(x_0)|| for every operator with the clamp on and off, the float32 restatement of the kernels' order inside the derived
bound, every refusal of the scope, of the window executor and of infer_video by message on a stand-in library, the scope's nesting, the
job's option and run-directory suffix, and the C ABI's names."""
import contextlib
import inspect

import numpy as np
import pytest
import torch

from dps_restated import RHO_MIN, assert_unambiguous, dps_bound, dps_f32, dps_fp64, seed_inputs
from measurement_restated import OPERATORS
from step_nll_restated import ratio, tables
from video_diffusion_amd import _lib, video_sample
from video_diffusion_amd.executor import WindowExecutor
from video_diffusion_amd.gaussian_diffusion import GaussianDiffusion, check_zeta, measure
from video_diffusion_amd.script_util import create_gaussian_diffusion

SIZES = {1: 7, 2: 6, 4: 12, 8: 16}                                             # H = W per scale: odd, no multiple of 4, more than one cell


@pytest.fixture(scope="module")
def tab():
    return tables(create_gaussian_diffusion(timestep_respacing="ddim50"))


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("s,gray", OPERATORS)
def test_cotangent_is_autograd_of_the_residual_norm(tab, s, gray, clip):
    """q (through the clamp), d eps and d_x of the float64 restatement against torch.autograd.grad of rho_b in float64."""
    xt, eps, t, y, lat = seed_inputs(tab, 2, 3, SIZES[s], s, gray, clip, seed=11 + s)
    assert_unambiguous(tab, xt, eps, t, y, lat, s, gray, clip)
    ex = dps_fp64(tab, xt, eps, t, y, lat, s, gray, clip)
    a = torch.tensor(tab["sr"][t].astype(np.float64)).reshape(-1, 1, 1, 1, 1)
    b = torch.tensor(tab["srm1"][t].astype(np.float64)).reshape(-1, 1, 1, 1, 1)
    X = torch.tensor(xt.astype(np.float64), requires_grad=True)
    E = torch.tensor(eps.astype(np.float64), requires_grad=True)
    x0r = a * X - b * E
    x0r.retain_grad()
    x0 = x0r.clamp(-1, 1) if clip else x0r
    r = (torch.tensor(y.astype(np.float64)) - measure(x0, s, gray)) * torch.tensor(lat.astype(np.float64)).reshape(2, 3, 1, 1, 1)
    rho = r.reshape(2, -1).pow(2).sum(dim=1).sqrt()
    rho.sum().backward()
    assert np.allclose(rho.detach().numpy(), ex["rho"], rtol=1e-13, atol=0) and (ex["rho"] >= RHO_MIN).all()
    for got, want in ((ex["q"] * ex["mask"], x0r.grad), (ex["deps"], E.grad), (ex["dxd"], X.grad)):
        assert np.allclose(got, want.numpy(), rtol=1e-11, atol=1e-15), float(np.abs(got - want.numpy()).max())
    assert not ex["deps"][:, 1].any() and not ex["dxd"][:, 1].any() and ex["deps"][:, 0].any()        # the frame that is not latent
    if clip:
        assert (~ex["mask"]).mean() > 0.15 and not ex["dxd"][~ex["mask"]].any()                     # a quarter sits beyond the clamp


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("s,gray", OPERATORS)
def test_float32_restatement_inside_the_bound(tab, s, gray, clip):
    xt, eps, t, y, lat = seed_inputs(tab, 2, 3, SIZES[s], s, gray, clip, seed=31 + s)
    assert_unambiguous(tab, xt, eps, t, y, lat, s, gray, clip)
    f32 = dps_f32(tab, xt, eps, t, y, lat, s, gray, clip)
    lim = dps_bound(tab, xt, eps, t, y, lat, s, gray, clip)
    for k in ("deps", "dxd", "rho"):
        want, bound = lim[k]
        r = ratio(f32[k], want, bound)
        assert r.max() <= 1.0, (k, float(r.max()))
        assert f32[k].dtype == np.float32
    # the bound is a rounding bound, not a tolerance: a relative 1e-3 on the largest element is far outside it (the head's
    # cancellation a x - b eps at a late t costs a few 1e-6 of x_0, and the residual is a tenth of that scale)
    want, bound = lim["dxd"]
    i = np.unravel_index(np.argmax(np.abs(want)), want.shape)
    assert abs(want[i]) * 1e-3 > bound[i] > 0


def test_empty_and_zero_items(tab):
    """An item without a latent frame, and an item whose residual is exactly 0: rho = 0, every cotangent 0, bound 0, no NaN."""
    xt, eps, t, y, lat = seed_inputs(tab, 2, 2, 8, 2, False, True, seed=5)
    lat[0] = 0
    ex = dps_fp64(tab, xt, eps, t, y, lat, 2, False, True)
    f32 = dps_f32(tab, xt, eps, t, y, lat, 2, False, True)
    lim = dps_bound(tab, xt, eps, t, y, lat, 2, False, True)
    for d in (ex, f32):
        assert d["rho"][0] == 0 and not d["deps"][0].any() and not d["dxd"][0].any() and d["rho"][1] > 0
        assert all(np.isfinite(d[k]).all() for k in ("rho", "deps", "dxd"))
    assert lim["rho"][1][0] == 0 and not lim["deps"][1][0].any()
    with pytest.raises(AssertionError, match="within the head's bound of 1"):
        xb, eb = xt.copy(), eps.copy()
        xb[1, 0, 0, 0, 0], eb[1, 0, 0, 0, 0] = np.float32(1.0) / tab["sr"][t[1]], 0.0          # x_0r = 1 up to rounding
        assert_unambiguous(tab, xb, eb, t, y, lat, 2, False, True)
    with pytest.raises(AssertionError, match="below"):
        y0 = y.copy()
        y0[1] = dps_fp64(tab, xt, eps, t, y, lat, 2, False, True)["x0"][1].reshape(2, 3, 4, 2, 4, 2).mean(axis=(3, 5)).astype(np.float32)
        assert_unambiguous(tab, xt, eps, t, y0, lat, 2, False, True)


# ---------------------------------------------------------------------------------------------------------------- the scope
class _FakeLib:
    """Stand-in for the library: the engine's guidance switches; a step that reaches vd_dps_step is recorded."""

    def __init__(self):
        self.cfg, self.phi, self.p, self.steps = 1.0, 0.0, 0.0, []

    def vd_cfg_scale(self, handle):
        return self.cfg

    def vd_guidance_rescale(self, handle):
        return self.phi

    def vd_dynamic_threshold(self, handle):
        return self.p

    def vd_dps_step(self, *args):
        self.steps.append(args)
        return 0


class _FakeModel:
    _handle = 17
    device = torch.device("cpu")
    guidance_asked = 0

    def _require_guidance(self):
        self.guidance_asked += 1

    def _pack_kwargs(self, x, kw):
        return dict(obs_src=x, obs_mask=x, latent_mask=x, kinda_marg_mask=x, frame_indices=x, obs_mode=0)

    @staticmethod
    def _window_ptrs(x, kw):
        return (1, 2, 3, 4, 5, 6)


def _fake(monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    monkeypatch.setattr(_lib, "current_stream", lambda: None)
    model = _FakeModel()
    diff = create_gaussian_diffusion(timestep_respacing="ddim10")
    model._bound_schedule = diff                                                 # (bound already: no upload)
    return fake, model, diff


def test_scope_sets_restores_and_nests(monkeypatch):
    fake, model, diff = _fake(monkeypatch)
    ya, yb = torch.zeros(1, 2, 3, 2, 2), torch.ones(1, 2, 1, 8, 8)
    with diff.dps_scope(model, ya, scale=4, zeta=0.5):
        outer = model._dps
        assert (outer["scale"], outer["gray"], outer["zeta"]) == (4, False, 0.5) and torch.equal(outer["y"], ya)
        with diff.dps_scope(model, yb, gray=True, zeta=2):
            assert (model._dps["scale"], model._dps["gray"], model._dps["zeta"]) == (1, True, 2.0)
        assert model._dps is outer
    assert model._dps is None
    with pytest.raises(RuntimeError, match="boom"):
        with diff.dps_scope(model, ya, 4, zeta=1.0):
            raise RuntimeError("boom")
    assert model._dps is None
    for bad, kw, what in ((ya, dict(scale=3, zeta=1.0), "cell size"), (ya, dict(scale=1, zeta=1.0), "identity"),
                          (ya, dict(scale=4, gray=True, zeta=1.0), "y must be"), (ya * float("nan"), dict(scale=4, zeta=1.0), "finite"),
                          (torch.zeros(3, 2, 2), dict(scale=4, zeta=1.0), "y must be a"), (ya, dict(scale=4, zeta=-0.1), "finite and not negative"),
                          (ya, dict(scale=4, zeta=float("nan")), "finite and not negative"), (ya, dict(scale=4, zeta=float("inf")), "finite and not negative"),
                          (ya, dict(scale=4, zeta="1"), "must be a number"), (ya, dict(scale=4, zeta=None), "must be a number")):
        with pytest.raises(ValueError, match=what):
            with diff.dps_scope(model, bad, **kw):
                pass
    with pytest.raises(TypeError, match="zeta"):                                 # zeta is required
        with diff.dps_scope(model, ya, 4):
            pass
    assert model._dps is None and check_zeta(0) == 0.0 and check_zeta(np.float32(0.25)) == 0.25
    doc = GaussianDiffusion.dps_scope.__doc__
    assert "extension" in doc and "DPS" in doc and "No claim about restoration quality" in doc


def test_every_refusal_of_the_scope_by_message(monkeypatch):
    fake, model, diff = _fake(monkeypatch)
    x, t = torch.zeros(1, 2, 3, 8, 8), torch.tensor([1])
    y = torch.zeros(1, 2, 3, 2, 2)
    fn = lambda v: v                                                             # noqa: E731
    wex = WindowExecutor.__new__(WindowExecutor)                                 # (its constructor makes a stream: no device here)
    wex.model = model
    with diff.dps_scope(model, y, 4, zeta=0.5):
        for call, what in ((lambda: diff.dpmpp_2m_sample(model, x, t), "dpmpp_2m_sample"),
                           (lambda: diff.ddim_reverse_sample(model, x, t), "ddim_reverse_sample"),
                           (lambda: diff.p_sample(model, x, t, denoised_fn=fn), "denoised_fn"),
                           (lambda: diff.ddim_sample(model, x, t, denoised_fn=fn), "denoised_fn"),
                           (lambda: diff.p_sample(model, x, t, use_gradient_method=True), "use_gradient_method"),
                           (lambda: diff.p_sample(model, x, t, return_attn_weights=True), "return_attn_weights"),
                           (lambda: diff.p_sample(model, x, t, cfg_scale=2.0), "cfg_scale != 1"),
                           (lambda: diff.ddim_sample(model, x, t, cfg_scale=0.0), "cfg_scale != 1"),
                           (lambda: wex.begin(x, {}), "WindowExecutor.begin")):
            with pytest.raises(_lib.VdError, match=f"{what} inside dps_scope is not served"):
                call()
        for attr, value, what in (("cfg", 2.0, "cfg_scale != 1 .cfg_scale_scope."), ("phi", 0.5, "guidance_scope with cfg_rescale or dynamic_threshold set"),
                                  ("p", 0.9, "guidance_scope with cfg_rescale or dynamic_threshold set")):
            setattr(fake, attr, value)
            with pytest.raises(_lib.VdError, match=f"{what} inside dps_scope is not served"):
                diff.p_sample(model, x, t, model_kwargs={})
            setattr(fake, attr, _FakeLib().__dict__[attr])
        for attr, what in (("_known_region", "known_region_scope"), ("_measurement", "measurement_scope")):
            setattr(model, attr, dict(y=y, scale=4, gray=False))
            with pytest.raises(_lib.VdError, match=f"{what} inside dps_scope is not served"):
                diff.ddim_sample(model, x, t, model_kwargs={})
            setattr(model, attr, None)
        with pytest.raises(ValueError, match="dps_scope: y"):
            diff.p_sample(model, x[:, :1], t, model_kwargs={})
        assert not fake.steps and model.guidance_asked == 0                      # none of them reached the engine
        # what is left reaches vd_dps_step with the scope's operator and step size, after the backward image was asked for
        out = diff.ddim_sample(model, x, t, model_kwargs={}, eta=0.5)
        assert set(out) == {"sample", "pred_xstart", "grad", "residual_norm"} and out["residual_norm"].shape == (1,)
        out = diff.p_sample(model, x, t, model_kwargs={})
        assert set(out) == {"sample", "pred_xstart", "attn", "grad", "residual_norm"} and out["grad"].shape == x.shape
        assert model.guidance_asked == 2 and len(fake.steps) == 2
        ddim, plain = fake.steps
        assert ddim[12:14] == (1, 0.5) and plain[12:14] == (0, 0.0)              # sampler, eta
        assert plain[16:19] == (4, 0, 0.5)                                       # scale, gray, zeta
    with pytest.raises(NotImplementedError, match="epsilon-prediction models only"):
        dx = create_gaussian_diffusion(timestep_respacing="ddim10", predict_xstart=True)
        model._bound_schedule = dx
        with dx.dps_scope(model, y, 4, zeta=0.5):
            dx.p_sample(model, x, t, model_kwargs={})


# ---------------------------------------------------------------------------------------------------------------- infer_video and the job
class _StubModel:
    device = torch.device("cpu")

    def check_device_errors(self):
        pass


class _StubDiffusion:
    """Two steps per window; records the DPS setting every window's steps ran under."""
    num_timesteps = 2

    def __init__(self):
        self.windows, self._d = [], None

    @contextlib.contextmanager
    def dps_scope(self, model, y, scale=1, gray=False, *, zeta):
        self._d = (y.clone(), scale, gray, zeta)
        try:
            yield
        finally:
            self._d = None

    def p_sample(self, model, x, t, clip_denoised=True, model_kwargs=None, **kw):
        if int(t[0]) == self.num_timesteps - 1:
            self.windows.append((model_kwargs["frame_indices"].clone(), self._d))
        assert self._d is not None
        return {"sample": x + 1.0, "pred_xstart": x}


def test_infer_video_runs_dps_in_place_of_the_projection():
    B, T, H = 2, 9, 8
    batch = torch.rand(B, T, 3, H, H, generator=torch.Generator().manual_seed(0))
    y = measure(batch, 4, True) + 0.25
    diff = _StubDiffusion()                                                      # (it has no measurement_scope: entering one would raise)
    video_sample.infer_video("autoreg", _StubModel(), diff, batch, 5, 2, measurement=y, sr_scale=4, gray=True, dps_zeta=0.75)
    assert len(diff.windows) >= 2
    for fi, (yw, scale, gray, zeta) in diff.windows:
        assert (scale, gray, zeta) == (4, True, 0.75)
        for i in range(B):
            for w, f in enumerate(fi[i].tolist()):
                assert torch.equal(yw[i, w], y[i, f])                            # gathered per window exactly as the projection's
    base = dict(measurement=y, sr_scale=4, gray=True, dps_zeta=0.5)
    for kw, err, what in ((dict(dps_zeta=0.5), ValueError, "dps_zeta needs a measurement"),
                          (dict(base, dps_zeta=-1.0), ValueError, "finite and not negative"),
                          (dict(base, executor="graph"), _lib.VdError, "executor='graph' together with dps_zeta is not served"),
                          (dict(base, prefix_cache=True), _lib.VdError, "prefix_cache together with dps_zeta is not served"),
                          (dict(base, suffix_skip=True), _lib.VdError, "suffix_skip together with dps_zeta is not served"),
                          (dict(base, sampler="dpmpp_2m"), _lib.VdError, "sampler='dpmpp_2m' together with dps_zeta is not served"),
                          (dict(base, cfg_scale=2.0), _lib.VdError, "cfg_scale != 1 together with dps_zeta is not served"),
                          (dict(base, cfg_rescale=0.5), _lib.VdError, "cfg_rescale together with dps_zeta is not served"),
                          (dict(base, dynamic_threshold=0.9), _lib.VdError, "dynamic_threshold together with dps_zeta is not served"),
                          (dict(base, use_gradient_method=True), _lib.VdError, "use_gradient_method together with a measurement"),
                          (dict(base, known_mask=torch.ones(T, H, H)), _lib.VdError, "known region"),
                          (dict(base, sr_scale=2), ValueError, "y must be")):
        with pytest.raises(err, match=what):
            video_sample.infer_video("autoreg", object(), object(), batch, 5, 2, **kw)   # before anything touches the engine


def test_option_suffix_and_names(tmp_path):
    parse = video_sample.build_parser().parse_args
    for argv, suffix in ((["--measurement", "y.npy", "--sr_scale", "4", "--dps_zeta", "0.5"], "_sr4_dps0.5"),
                         (["--measurement", "y.npy", "--gray", "--dps_zeta", "2"], "_gray_dps2"),
                         (["--measurement", "y.npy", "--sr_scale", "8", "--gray", "--dps_zeta", "0"], "_sr8gray_dps0"),
                         (["--measurement", "y.npy", "--sr_scale", "4", "--sampler", "ddim", "--dps_zeta", "1.25"], "_ddim_sr4_dps1.25"),
                         (["--measurement", "y.npy", "--sr_scale", "4"], "_sr4")):
        assert video_sample.run_postfix(parse(argv)) == suffix
    assert parse([]).dps_zeta is None and video_sample.run_postfix(parse([])) == ""
    y = np.zeros((3, 4, 3, 2, 2), np.float32)
    np.save(tmp_path / "y.npy", y)
    args = parse(["--measurement", str(tmp_path / "y.npy"), "--sr_scale", "4", "--dps_zeta", "0.5"])
    args._batch_ids = [2, 0]
    assert video_sample._measurement_options(args, torch.zeros(2, 4, 3, 8, 8))["dps_zeta"] == 0.5
    args = parse(["--measurement", str(tmp_path / "y.npy"), "--sr_scale", "4"])
    args._batch_ids = [2, 0]
    assert "dps_zeta" not in video_sample._measurement_options(args, torch.zeros(2, 4, 3, 8, 8))
    with pytest.raises(ValueError, match="--dps_zeta needs --measurement"):
        video_sample._measurement_options(parse(["--dps_zeta", "0.5"]), torch.zeros(2, 4, 3, 8, 8))
    sig = inspect.signature(video_sample.infer_video).parameters
    assert sig["dps_zeta"].kind is inspect.Parameter.KEYWORD_ONLY and sig["dps_zeta"].default is None
    sig = inspect.signature(GaussianDiffusion.dps_scope).parameters
    assert list(sig) == ["self", "model", "y", "scale", "gray", "zeta"] and sig["zeta"].default is inspect.Parameter.empty
    for name in ("vd_dps_step", "vd_op_dps_seed"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["vd_dps_step"][1]) == 24 and len(_lib.SIGNATURES["vd_op_dps_seed"][1]) == 18
    assert "dps.hip" in _lib.SOURCES
    header = open(_lib.HEADER).read()
    assert "int vd_dps_step(" in header and "int vd_op_dps_seed(" in header
