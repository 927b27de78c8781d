"""No GPU: loss-guided sampling (this project's extension) -- the float32 restatement of the seed and final arithmetic
(tests/loss_guidance_restated.py) against float64 torch autograd through an analytic stand-in network eps = M x with the clamp on and
off, the norm's bound, the host checks of the scope (scale, exactly one function), every refusal of the scope by message on a stand-in
library, the abort when the caller's function raises, infer_video's refusals, the job's options, its run-directory suffix and the
MODULE:FUNCTION import."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from loss_guidance_restated import F, U, final_f32, fma32, grad_f32, multiplier_f32, norm_fp64, rows, seed_f32
from video_diffusion_amd import _lib, video_sample
from video_diffusion_amd.executor import WindowExecutor
from video_diffusion_amd.gaussian_diffusion import GaussianDiffusion, check_loss_guidance, loss_guidance_step_scale
from video_diffusion_amd.script_util import create_gaussian_diffusion


# ---------------------------------------------------------------------------------------------------------------- the restatement
def _standin(clip, seed):
    """B = 2, T = 3, 4 x 4 frames, frame 1 not latent; eps = M x per item with a random M.  About a third of x_0 lies beyond +-1, none
    within 1e-3 of it (the clamp's mask is then the same in float32 and float64)."""
    g = torch.Generator().manual_seed(seed)
    B, T, H = 2, 3, 4
    n = T * 3 * H * H
    diff = create_gaussian_diffusion(timestep_respacing="ddim50")
    t = np.array([12, 3])
    a, b = rows(diff, t)
    x = torch.randn(B, T, 3, H, H, generator=g).float()
    M = (torch.randn(B, n, n, generator=g) / n ** 0.5).float()
    lat = np.array([[1, 0, 1], [1, 0, 1]], np.float32)
    for _ in range(50):
        eps = torch.einsum("bij,bj->bi", M.double(), x.reshape(B, n).double()).reshape(x.shape)
        x0 = torch.from_numpy(a.astype(np.float64)) * x.double() - torch.from_numpy(b.astype(np.float64)) * eps
        near = (x0.abs() - 1).abs() < 1e-3
        if not near.any():
            break
        x = torch.where(near, x * 1.01, x)
    assert not near.any()
    return diff, t, a, b, x, M, lat


@pytest.mark.parametrize("clip", [True, False])
def test_restated_gradient_is_autograd_through_the_clamp(clip):
    """g = a c_r - b J^T c_r is the gradient of loss(clamp(x_0(x_t))) with respect to x_t: the float32 restatement of the seed, M^T as
    the backward pass in float64, against torch.autograd in float64.  Bound per element: d_eps, d_x and the float32 cast of the cotangent
    are one rounding of 2^-24 each on their own magnitude, carried through |M|^T -- 3 * 2^-24 (|d_x| + |M|^T |d_eps|)."""
    diff, t, a, b, x, M, lat = _standin(clip, 5)
    B, n = x.shape[0], x[0].numel()
    w = torch.randn(x.shape, generator=torch.Generator().manual_seed(6)).double()
    lat_t = torch.from_numpy(lat.astype(np.float64)).reshape(B, 3, 1, 1, 1)
    X = x.double().requires_grad_(True)
    eps = torch.einsum("bij,bj->bi", M.double(), X.reshape(B, n)).reshape(x.shape)
    x0r = torch.from_numpy(a.astype(np.float64)) * X - torch.from_numpy(b.astype(np.float64)) * eps
    x0 = x0r.clamp(-1, 1) if clip else x0r
    x0.retain_grad()
    loss = ((w * x0).tanh().pow(2) * lat_t).sum()                 # what the loss says about frames that are not latent is ignored
    loss.backward()
    want = X.grad.numpy()
    cot = x0.grad.numpy().astype(F)                               # the caller's cotangent, as the engine is handed it
    cot_all = cot + (1 - lat.reshape(B, 3, 1, 1, 1)).astype(F) * F(3.0)      # junk on the frame that is not latent: never read
    de, dx, x0r32 = seed_f32(a, b, x.numpy(), eps.detach().numpy().astype(F), cot_all, lat, clip)
    Mt = M.double().numpy().transpose(0, 2, 1)
    vjp = np.einsum("bij,bj->bi", Mt, de.astype(np.float64).reshape(B, n)).reshape(x.shape)
    got = dx.astype(np.float64) + vjp
    lim = 3 * U * (np.abs(dx) + np.einsum("bij,bj->bi", np.abs(Mt), np.abs(de).astype(np.float64).reshape(B, n)).reshape(x.shape)) + 1e-300
    r = np.abs(got - want) / lim
    print(f"clip={clip}: max |g - autograd| / bound = {r.max():.3f}; max |g| = {np.abs(want).max():.3e}")
    assert (r <= 1.0).all() and np.abs(want).max() > 1e-3
    assert not de[:, 1].any() and not dx[:, 1].any() and de[:, 0].any() and dx[:, 2].any()
    beyond = np.abs(x0r32) > 1
    assert 0.1 < beyond.mean() < 0.6
    if clip:
        assert not dx[beyond].any() and not de[beyond].any()
    else:
        assert dx[beyond & (lat.reshape(B, 3, 1, 1, 1) == 1)].any()


def test_seed_edges_and_final_arithmetic():
    diff = create_gaussian_diffusion(timestep_respacing="ddim50")
    a, b = rows(diff, np.array([0, 50]))
    assert np.isnan(a[1]).all() and np.isfinite(a[0]).all()
    x = np.ones((2, 1, 3, 2, 2), F)
    de, dx, _ = seed_f32(a, b, x, x, x, np.ones((2, 1), F), True)
    assert np.isnan(de[1]).all() and np.isnan(dx[1]).all() and np.isfinite(de[0]).all()       # t outside the schedule: NaN on the item
    cot = x.copy()
    cot[0, 0, 0, 0, 0] = np.inf
    de, dx, _ = seed_f32(a, b, 0 * x, 0 * x, cot, np.ones((2, 1), F), False)
    assert np.isinf(dx[0, 0, 0, 0, 0]) and np.isfinite(dx[0, 0, 1]).all()                      # a cotangent that is not finite propagates
    # fma32 against exact rational arithmetic on a tie and around it
    assert fma32(F(1), F(1), F(2.0 ** -24)) == F(1) and fma32(F(1), F(1 + 2.0 ** -23), F(2.0 ** -24)) == F(1 + 2.0 ** -22)
    g = np.random.default_rng(0).standard_normal((2, 3, 3, 4, 4)).astype(F)
    plain = np.random.default_rng(1).standard_normal(g.shape).astype(F)
    lat = np.array([[0, 1, 1], [1, 0, 1]], F)
    n, lim = norm_fp64(g, lat)
    for bi in range(2):
        assert abs(n[bi] - np.sqrt((g[bi][lat[bi] == 1].astype(np.float64) ** 2).sum())) <= 1e-12 * n[bi] and 0 < lim[bi] < 1e-6 * n[bi]
    m = multiplier_f32([0.5, 2.0], n.astype(F))
    out = final_f32(m, g, plain, lat)
    want = plain.astype(np.float64) - m.astype(np.float64).reshape(2, 1, 1, 1, 1) * g
    sel = np.broadcast_to(lat.reshape(2, 3, 1, 1, 1) == 1, g.shape)
    assert np.array_equal(out[~sel], plain[~sel]) and np.abs(out[sel] - want[sel]).max() <= U * np.abs(want[sel]).max() * 1.01
    assert np.array_equal(final_f32(multiplier_f32([0.0, 0.0]), g, plain, lat), plain)         # scale 0: the plain step's bits
    assert np.array_equal(multiplier_f32([1.0, 1.0], np.array([0.0, 4.0], F)), np.array([0.0, 0.25], F))
    assert np.array_equal(grad_f32(g, plain, 0.25), (g + plain * F(0.25)).astype(F))


# ---------------------------------------------------------------------------------------------------------------- the host checks
def test_scale_and_function_checks():
    fn = lambda x0, t: x0                                                        # noqa: E731
    assert check_loss_guidance(fn, None, 0) == 0.0 and check_loss_guidance(None, fn, np.float32(0.25)) == 0.25
    sc = lambda t: 1.0                                                           # noqa: E731
    assert check_loss_guidance(fn, None, sc) is sc
    for lf, cf in ((None, None), (fn, fn)):
        with pytest.raises(ValueError, match="exactly one of loss_fn and cotangent_fn"):
            check_loss_guidance(lf, cf, 1.0)
    with pytest.raises(ValueError, match="must be callable"):
        check_loss_guidance(3, None, 1.0)
    for bad in (-0.1, float("nan"), float("inf"), 1e39, "1", None, True):
        with pytest.raises(ValueError, match="finite and not negative|must be a number"):
            check_loss_guidance(fn, None, bad)
    t = torch.tensor([3, 3])
    assert loss_guidance_step_scale(0.5, t, 2).tolist() == [0.5, 0.5]
    assert loss_guidance_step_scale(lambda tt: 0.1 * float(tt[0]), t, 2).dtype == torch.float32
    assert loss_guidance_step_scale(lambda tt: torch.tensor([1.0, 2.0], dtype=torch.float64), t, 2).tolist() == [1.0, 2.0]
    assert loss_guidance_step_scale(lambda tt: torch.tensor(4.0), t, 2).tolist() == [4.0, 4.0]
    for bad, what in ((lambda tt: -1.0, "finite and not negative"), (lambda tt: float("nan"), "finite and not negative"),
                      (lambda tt: torch.tensor([1.0, float("inf")]), "finite and not negative"),
                      (lambda tt: torch.tensor([1.0, -2.0]), "finite and not negative"),
                      (lambda tt: torch.tensor([1.0, 2.0, 3.0]), "3 values for a batch of 2"), (lambda tt: "x", "must be a number")):
        with pytest.raises(ValueError, match=what):
            loss_guidance_step_scale(bad, t, 2)


class _FakeLib:
    """The entries a step inside loss_guidance_scope reaches, recording what they were handed."""

    def __init__(self):
        self.cfg, self.phi, self.p = 1.0, 0.0, 0.0
        self.calls, self.ticket, self.finish_rc = [], 40, 0

    def vd_cfg_scale(self, handle):
        return self.cfg

    def vd_guidance_rescale(self, handle):
        return self.phi

    def vd_dynamic_threshold(self, handle):
        return self.p

    def vd_guide_begin(self, *args):
        self.ticket += 1
        ctypes.cast(args[-2], ctypes.POINTER(ctypes.c_ulonglong))[0] = self.ticket
        self.calls.append(("begin", args))
        return 0

    def vd_guide_finish(self, *args):
        self.calls.append(("finish", args))
        return self.finish_rc

    def vd_guide_abort(self, *args):
        self.calls.append(("abort", args))
        return 0

    def vd_last_error(self):
        return b"loss_guidance: no taped pass is held for this ticket (stand-in)"


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
    monkeypatch.setattr(_lib, "current_stream", lambda: 99)
    model = _FakeModel()
    diff = create_gaussian_diffusion(timestep_respacing="ddim10")
    model._bound_schedule = diff
    return fake, model, diff


def test_scope_sets_restores_nests_and_a_step_is_begin_callback_finish(monkeypatch):
    fake, model, diff = _fake(monkeypatch)
    x, t = torch.zeros(1, 2, 3, 8, 8), torch.tensor([1])
    seen = []

    def loss(x0, tt):
        assert x0.requires_grad and x0.is_leaf and torch.is_grad_enabled() and tt.dtype == torch.int64
        seen.append(("loss", len(fake.calls)))
        return (x0 * 2).sum(dim=(2, 3, 4))                                       # any shape: its sum is differentiated

    def cotan(x0, tt):
        assert not x0.requires_grad
        seen.append(("cot", len(fake.calls)))
        return torch.full_like(x0, 3.0)

    with diff.loss_guidance_scope(model, loss, scale=0.5):
        outer = model._loss_guidance
        assert outer["loss_fn"] is loss and outer["cotangent_fn"] is None and outer["scale"] == 0.5 and outer["normalize"] is False
        with diff.loss_guidance_scope(model, cotangent_fn=cotan, scale=lambda tt: 2.0, normalize=True):
            assert model._loss_guidance["cotangent_fn"] is cotan and model._loss_guidance["normalize"] is True
            out = diff.ddim_sample(model, x, t, model_kwargs={}, eta=0.5)
            assert set(out) == {"sample", "pred_xstart", "grad", "grad_norm"} and out["grad_norm"].shape == (1,)
        assert model._loss_guidance is outer
        with torch.no_grad():
            out = diff.p_sample(model, x, t, model_kwargs={})
        assert set(out) == {"sample", "pred_xstart", "attn", "grad"} and out["grad"].shape == x.shape
    assert model._loss_guidance is None and model.guidance_asked == 2
    assert seen == [("cot", 1), ("loss", 3)]                                     # the caller's function runs between begin and finish
    (b1, a1), (f1, g1), (b2, a2), (f2, g2) = fake.calls
    assert (b1, f1, b2, f2) == ("begin", "finish", "begin", "finish")
    assert a1[12:14] == (1, 0.5) and a2[12:14] == (0, 0.0)                       # sampler, eta
    assert g1[1] == 41 and g2[1] == 42 and g1[4] == 1 and g2[4] == 0             # the ticket begin handed out; normalize
    assert a1[-1] == 99 and g1[-1] == 99                                         # one stream for both calls
    assert g2[7] is None and g1[7] is not None                                   # grad_norm only when normalised
    with pytest.raises(RuntimeError, match="boom"):
        with diff.loss_guidance_scope(model, loss, scale=1.0):
            raise RuntimeError("boom")
    assert model._loss_guidance is None
    with pytest.raises(TypeError, match="scale"):                                # scale is required
        with diff.loss_guidance_scope(model, loss):
            pass
    with pytest.raises(ValueError, match="exactly one"):
        with diff.loss_guidance_scope(model, loss, cotangent_fn=cotan, scale=1.0):
            pass
    assert "grad" not in _plain_keys(diff, model, x, t, monkeypatch)             # outside the scope: the plain step's dict
    doc = GaussianDiffusion.loss_guidance_scope.__doc__
    assert "extension" in doc and "no taped pass is held for this ticket" in doc and "PiGDM" in doc and "No claim" in doc


def _plain_keys(diff, model, x, t, monkeypatch):
    monkeypatch.setattr(diff, "_fused_step", lambda *a, **k: (x, x))
    return set(diff.p_sample(model, x, t, model_kwargs={}))


def test_a_function_that_raises_aborts_and_a_stale_ticket_surfaces(monkeypatch):
    fake, model, diff = _fake(monkeypatch)
    x, t = torch.zeros(1, 2, 3, 8, 8), torch.tensor([1])

    def boom(x0, tt):
        raise KeyError("mine")

    with diff.loss_guidance_scope(model, boom, scale=1.0):
        with pytest.raises(KeyError, match="mine"):
            diff.p_sample(model, x, t, model_kwargs={})
    assert [c[0] for c in fake.calls] == ["begin", "abort"]
    fake.calls.clear()
    for bad, what in ((lambda x0, tt: x0[:, :1], "the cotangent must be a float32 tensor"), (lambda x0, tt: x0.double(), "float32"),
                      (lambda x0, tt: None, "float32")):
        with diff.loss_guidance_scope(model, cotangent_fn=bad, scale=1.0):
            with pytest.raises(ValueError, match=what):
                diff.ddim_sample(model, x, t, model_kwargs={})
    assert [c[0] for c in fake.calls] == ["begin", "abort"] * 3
    fake.calls.clear()
    with diff.loss_guidance_scope(model, lambda x0, tt: x0.detach().sum() * 0 + 1.0, scale=1.0):      # does not depend on x0: a zero cotangent
        with pytest.raises(RuntimeError):
            diff.p_sample(model, x, t, model_kwargs={})           # (autograd itself refuses a result without a graph: the caller's error)
    assert [c[0] for c in fake.calls] == ["begin", "abort"]
    fake.calls.clear()
    with diff.loss_guidance_scope(model, lambda x0, tt: (x0[:, :0]).sum(), scale=1.0):                  # a graph that never reaches x0's values
        diff.p_sample(model, x, t, model_kwargs={})
    assert [c[0] for c in fake.calls] == ["begin", "finish"]
    fake.finish_rc = -1                                                          # the engine dropped the pass in between
    with diff.loss_guidance_scope(model, cotangent_fn=lambda x0, tt: x0, scale=1.0):
        with pytest.raises(_lib.VdError, match="no taped pass is held for this ticket"):
            diff.p_sample(model, x, t, model_kwargs={})
    with diff.loss_guidance_scope(model, cotangent_fn=lambda x0, tt: x0, scale=lambda tt: -1.0):
        n = len(fake.calls)
        with pytest.raises(ValueError, match="finite and not negative"):
            diff.p_sample(model, x, t, model_kwargs={})
        assert len(fake.calls) == n                                              # checked on the host before the engine is touched


def test_every_refusal_of_the_scope_by_message(monkeypatch):
    fake, model, diff = _fake(monkeypatch)
    x, t = torch.zeros(1, 2, 3, 8, 8), torch.tensor([1])
    fn = lambda v: v                                                             # noqa: E731
    wex = WindowExecutor.__new__(WindowExecutor)                                 # (its constructor makes a stream: no device here)
    wex.model = model
    with diff.loss_guidance_scope(model, cotangent_fn=lambda x0, tt: x0, scale=0.5):
        for call, what in ((lambda: diff.dpmpp_2m_sample(model, x, t), "dpmpp_2m_sample"),
                           (lambda: diff.dpmpp_2m_sde_sample(model, x, t), "dpmpp_2m_sde_sample"),
                           (lambda: diff.unipc_sample(model, x, t), "unipc_sample"),
                           (lambda: diff.ddim_reverse_sample(model, x, t), "ddim_reverse_sample"),
                           (lambda: diff.p_sample(model, x, t, denoised_fn=fn), "denoised_fn"),
                           (lambda: diff.ddim_sample(model, x, t, denoised_fn=fn), "denoised_fn"),
                           (lambda: diff.p_sample(model, x, t, use_gradient_method=True), "use_gradient_method"),
                           (lambda: diff.p_sample(model, x, t, return_attn_weights=True), "return_attn_weights"),
                           (lambda: diff.p_sample(model, x, t, cfg_scale=2.0), "cfg_scale != 1"),
                           (lambda: diff.ddim_sample(model, x, t, cfg_scale=0.0), "cfg_scale != 1"),
                           (lambda: wex.begin(x, {}), "WindowExecutor.begin")):
            with pytest.raises(_lib.VdError, match=f"{what} inside loss_guidance_scope is not served"):
                call()
        for attr, value, what in (("cfg", 2.0, "cfg_scale != 1 .cfg_scale_scope."), ("phi", 0.5, "guidance_scope with cfg_rescale or dynamic_threshold set"),
                                  ("p", 0.9, "guidance_scope with cfg_rescale or dynamic_threshold set")):
            setattr(fake, attr, value)
            with pytest.raises(_lib.VdError, match=f"{what} inside loss_guidance_scope is not served"):
                diff.p_sample(model, x, t, model_kwargs={})
            setattr(fake, attr, _FakeLib().__dict__[attr])
        for attr, what in (("_known_region", "known_region_scope"), ("_measurement", "measurement_scope"), ("_dps", "dps_scope")):
            setattr(model, attr, dict(y=x, scale=4, gray=False, zeta=1.0))
            with pytest.raises(_lib.VdError, match=f"{what} inside loss_guidance_scope is not served"):
                diff.ddim_sample(model, x, t, model_kwargs={})
            setattr(model, attr, None)
        assert not fake.calls and model.guidance_asked == 0                      # none of them reached the engine
    with pytest.raises(NotImplementedError, match="loss_guidance_scope with predict_xstart=True: epsilon-prediction models only"):
        dx = create_gaussian_diffusion(timestep_respacing="ddim10", predict_xstart=True)
        model._bound_schedule = dx
        with dx.loss_guidance_scope(model, cotangent_fn=lambda x0, tt: x0, scale=0.5):
            dx.p_sample(model, x, t, model_kwargs={})


# ---------------------------------------------------------------------------------------------------------------- infer_video and the job
def test_infer_video_refusals():
    batch = torch.rand(2, 9, 3, 8, 8, generator=torch.Generator().manual_seed(0))
    fn = lambda x0, t: x0                                                        # noqa: E731
    base = dict(loss_fn=fn, loss_scale=0.5)
    for kw, err, what in ((dict(loss_fn=fn), ValueError, "need a step size"), (dict(loss_scale=0.5), ValueError, "exactly one of loss_fn and cotangent_fn"),
                          (dict(base, cotangent_fn=fn), ValueError, "exactly one of loss_fn and cotangent_fn"),
                          (dict(base, loss_scale=-1.0), ValueError, "finite and not negative"),
                          (dict(base, executor="graph"), _lib.VdError, "executor='graph' together with loss_fn / cotangent_fn .loss_guidance_scope. is not served"),
                          (dict(base, prefix_cache=True), _lib.VdError, "prefix_cache together with loss_fn"),
                          (dict(base, suffix_skip=True), _lib.VdError, "suffix_skip together with loss_fn"),
                          (dict(base, sampler="dpmpp_2m"), _lib.VdError, "sampler='dpmpp_2m' together with loss_fn"),
                          (dict(base, sampler="dpmpp_2m_sde"), _lib.VdError, "sampler='dpmpp_2m_sde' together with loss_fn"),
                          (dict(base, sampler="unipc"), _lib.VdError, "sampler='unipc' together with loss_fn"),
                          (dict(base, use_gradient_method=True), _lib.VdError, "use_gradient_method together with loss_fn"),
                          (dict(base, known_mask=torch.ones(9, 8, 8)), _lib.VdError, "known_mask together with loss_fn"),
                          (dict(base, measurement=torch.zeros(2, 9, 3, 2, 2), sr_scale=4), _lib.VdError, "a measurement together with loss_fn"),
                          (dict(base, cfg_scale=2.0), _lib.VdError, "cfg_scale != 1 together with loss_fn"),
                          (dict(base, cfg_rescale=0.5), _lib.VdError, "cfg_rescale together with loss_fn"),
                          (dict(base, dynamic_threshold=0.9), _lib.VdError, "dynamic_threshold together with loss_fn")):
        with pytest.raises(err, match=what):
            video_sample.infer_video("autoreg", object(), object(), batch, 5, 2, **kw)   # before anything touches the engine


def test_job_options_suffix_and_function_import(tmp_path, monkeypatch):
    parse = video_sample.build_parser().parse_args
    for argv, suffix in ((["--loss_guidance", "m:f", "--loss_guidance_scale", "0.5"], "_lg0.5"),
                         (["--loss_guidance", "m:f", "--loss_guidance_scale", "2", "--sampler", "ddim", "--loss_guidance_normalize"], "_ddim_lg2"),
                         (["--loss_guidance", "m:f", "--loss_guidance_scale", "0"], "_lg0"), ([], "")):
        assert video_sample.run_postfix(parse(argv)) == suffix
    d = parse([])
    assert d.loss_guidance is None and d.loss_guidance_scale is None and not d.loss_guidance_normalize and not d.loss_guidance_cotangent
    (tmp_path / "my_losses.py").write_text("def bright(x0, t):\n    return -x0.mean()\n\nnot_a_function = 3\n")
    monkeypatch.syspath_prepend(str(tmp_path))
    f = video_sample.import_function("my_losses:bright")
    assert float(f(torch.ones(2), None)) == -1.0
    o = video_sample._loss_guidance_options(parse(["--loss_guidance", "my_losses:bright", "--loss_guidance_scale", "0.25"]))
    assert o == dict(loss_fn=f, cotangent_fn=None, loss_scale=0.25, loss_normalize=False)
    o = video_sample._loss_guidance_options(parse(["--loss_guidance", "my_losses:bright", "--loss_guidance_scale", "1", "--loss_guidance_cotangent",
                                                   "--loss_guidance_normalize"]))
    assert o == dict(loss_fn=None, cotangent_fn=f, loss_scale=1.0, loss_normalize=True)
    assert video_sample._loss_guidance_options(parse([])) == {}
    for spec, what in (("my_losses", "expected MODULE:FUNCTION"), (":f", "expected MODULE:FUNCTION"), ("my_losses:", "expected MODULE:FUNCTION"),
                       ("no_such_module_here:f", "cannot import module"), ("my_losses:missing", "has no callable 'missing'"),
                       ("my_losses:not_a_function", "has no callable")):
        with pytest.raises(ValueError, match=what):
            video_sample.import_function(spec)
    with pytest.raises(ValueError, match="--loss_guidance needs --loss_guidance_scale"):
        video_sample._loss_guidance_options(parse(["--loss_guidance", "my_losses:bright"]))
    for argv in (["--loss_guidance_scale", "1"], ["--loss_guidance_normalize"], ["--loss_guidance_cotangent"]):
        with pytest.raises(ValueError, match="needs --loss_guidance MODULE:FUNCTION"):
            video_sample._loss_guidance_options(parse(argv))
    sig = inspect.signature(video_sample.infer_video).parameters
    for name, default in (("loss_fn", None), ("cotangent_fn", None), ("loss_scale", None), ("loss_normalize", False)):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default is default
    sig = inspect.signature(GaussianDiffusion.loss_guidance_scope).parameters
    assert list(sig) == ["self", "model", "loss_fn", "cotangent_fn", "scale", "normalize"] and sig["scale"].default is inspect.Parameter.empty
    assert sig["cotangent_fn"].kind is inspect.Parameter.KEYWORD_ONLY and sig["loss_fn"].default is None
    for name, n in (("vd_guide_begin", 19), ("vd_guide_finish", 9), ("vd_guide_abort", 1), ("vd_op_guide_seed", 14)):
        assert len(_lib.SIGNATURES[name][1]) == n
    assert "guide.hip" in _lib.SOURCES
    header = open(_lib.HEADER).read()
    for name in ("vd_guide_begin", "vd_guide_finish", "vd_guide_abort", "vd_op_guide_seed"):
        assert f"int {name}(" in header
    assert "must stay alive" in header and "no taped pass is held for this ticket" in header
