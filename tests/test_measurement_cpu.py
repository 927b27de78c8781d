"""No GPU: zero-shot restoration (this project's extension, DDNM) -- the float64 restatement of the cell-mean operator and its
projection (A A^+ = I, idempotence), the float32 restatement of the kernel's summation order inside the derived bound, measure()
against the restatement, every ValueError of check_measurement, the scope on a stand-in library, the job's options and run-directory
suffixes, and infer_video's per-window gather of a measurement on a stub."""
import contextlib
import inspect

import numpy as np
import pytest
import torch

from measurement_restated import (OPERATORS, cell_mean_of, cells, measure_fp64, project_bound, project_f32, project_fp64, replicate,
                                  second_application_bound, served, uncells)
from step_nll_restated import F, U, ratio
from video_diffusion_amd import _lib, video_sample
from video_diffusion_amd.executor import WindowExecutor
from video_diffusion_amd.gaussian_diffusion import GaussianDiffusion, check_measurement, measure, measurement_shape
from video_diffusion_amd.script_util import create_gaussian_diffusion

SHAPES = {1: (7, 7), 2: (6, 10), 4: (12, 8), 8: (8, 16)}                     # (H, W) per scale: odd, no multiple of 4, more than one cell


def _video(s, seed=0, B=2, T=3, dtype=F):
    rs = np.random.RandomState(seed)
    H, W = SHAPES[s]
    return rs.uniform(-1.5, 1.5, (B, T, 3, H, W)).astype(dtype)


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("s,gray", OPERATORS)
def test_restatement_is_a_projection(s, gray):
    x = _video(s, 1, dtype=np.float64)
    B, T = x.shape[:2]
    lat = np.ones((B, T))
    n = s * s * (3 if gray else 1)
    v = cells(x, s, gray)
    assert v.shape[-1] == n and np.array_equal(uncells(v, s, gray, x.shape), x)
    y = np.random.RandomState(2).uniform(-1, 1, measure_fp64(x, s, gray).shape)
    # A A^+ = I, to the bit: the mean of n equal values
    assert np.allclose(measure_fp64(replicate(y, s, gray, x.shape), s, gray), y, rtol=1e-15, atol=0)
    out = project_fp64(x, y, lat, s, gray)
    assert np.allclose(measure_fp64(out, s, gray), y, rtol=0, atol=1e-14)        # A(out) = y
    assert np.allclose(project_fp64(out, y, lat, s, gray), out, rtol=0, atol=1e-14)   # idempotent
    # the null-space part is untouched: out - x is constant over every cell
    dv = cells(out - x, s, gray)
    assert np.allclose(dv, dv[..., :1], rtol=0, atol=1e-14)
    # frames that are not latent keep their values
    lat[:, 1] = 0
    out = project_fp64(x, y, lat, s, gray)
    assert np.array_equal(out[:, 1], x[:, 1]) and not np.array_equal(out[:, 0], x[:, 0])
    assert served(s, gray) and not served(1, False) and not served(3, False)


@pytest.mark.parametrize("s,gray", OPERATORS)
def test_float32_restatement_inside_the_bound(s, gray):
    x = _video(s, 3)
    B, T = x.shape[:2]
    lat = np.ones((B, T), F)
    lat[:, 1] = 0
    y = np.random.RandomState(4).uniform(-1, 1, measure_fp64(x, s, gray).shape).astype(F)
    got = project_f32(x, y, lat, s, gray)
    want, lim = project_bound(x, y, lat, s, gray)
    r = ratio(got, want, lim)
    assert (r <= 1.0).all(), float(r.max())
    assert np.array_equal(got[:, 1], x[:, 1]) and (lim[:, 1] == 0).all() and (lim[:, 0] > 0).all()
    n = s * s * (3 if gray else 1)
    assert (lim[:, 0] <= (n + 3) * U * 4.0).all()                                # |x| <= 1.5, |y| <= 1: the bound is a few n u
    # A(out) = y within the cell mean of the bound; a second application moves nothing beyond its bound
    assert (np.abs(measure_fp64(got, s, gray) - y)[:, 0] <= measure_fp64(lim, s, gray)[:, 0]).all()
    again = project_f32(got, y, lat, s, gray)
    w2, l2 = second_application_bound(got, y, lat, s, gray, lim)
    assert (ratio(again, w2, l2) <= 1.0).all()
    # a seeded mistake leaves the bound: the cell sum divided by the cell's size without the channels
    if gray:
        wrong = x + replicate(y - measure_fp64(x, s, gray) * 3, s, gray, x.shape)
        assert (ratio(wrong.astype(F), want, lim)[:, 0] > 1.0).any()
    # a cell with an Inf comes out not finite, every other cell is as before
    xi = x.copy()
    xi[0, 0, 1, 0, 0] = np.inf
    gi = project_f32(xi, y, lat, s, gray)
    bad = ~np.isfinite(cell_mean_of(np.where(np.isfinite(xi), 0.0, np.inf), s, gray))
    assert bad.any() and not np.isfinite(gi[bad]).any() and np.array_equal(gi[~bad], got[~bad])


# ---------------------------------------------------------------------------------------------------------------- measure, checks
@pytest.mark.parametrize("s,gray", OPERATORS)
def test_measure_against_the_restatement(s, gray):
    x = _video(s, 5, dtype=np.float64)
    y = measure(torch.from_numpy(x), s, gray)
    assert y.dtype == torch.float64 and tuple(y.shape) == measurement_shape(x.shape, s, gray) == measure_fp64(x, s, gray).shape
    assert np.allclose(y.numpy(), measure_fp64(x, s, gray), rtol=0, atol=1e-14)
    y32 = measure(torch.from_numpy(x.astype(F)), s, gray)
    n = s * s * (3 if gray else 1)
    assert y32.dtype == torch.float32 and np.abs(y32.numpy() - measure_fp64(x.astype(F), s, gray)).max() <= (n + 1) * U * 1.5
    assert GaussianDiffusion.measure is measure                                  # diffusion.measure(video, scale, gray)
    y_ok = check_measurement(y, x.shape, s, gray)
    assert y_ok.dtype == torch.float32 and y_ok.is_contiguous()


def test_every_value_error_of_check_measurement():
    shape = (2, 3, 3, 8, 8)
    y = torch.zeros(2, 3, 3, 4, 4)
    check_measurement(y, shape, 2, False)
    for scale in (3, 0, 16, -2, 2.0, "4", True, None):
        with pytest.raises(ValueError, match="the cell size must be one of 2, 4, 8, or 1 together with gray=True"):
            check_measurement(y, shape, scale, False)
    with pytest.raises(ValueError, match="scale=1 with gray=False is the identity"):
        check_measurement(torch.zeros(2, 3, 3, 8, 8), shape, 1, False)
    check_measurement(torch.zeros(2, 3, 1, 8, 8), shape, 1, True)
    for bad_shape in ((2, 3, 3, 6, 8), (2, 3, 3, 8, 6)):
        with pytest.raises(ValueError, match="must be divisible by scale=4"):
            check_measurement(y, bad_shape, 4, False)
    for bad_shape in ((2, 3, 1, 8, 8), (3, 3, 8, 8)):
        with pytest.raises(ValueError, match=r"a video is \(B, T, 3, H, W\)"):
            check_measurement(y, bad_shape, 2, False)
    for bad in (torch.zeros(2, 3, 1, 4, 4), torch.zeros(2, 3, 3, 2, 2), torch.zeros(2, 2, 3, 4, 4), torch.zeros(3, 4, 4), np.zeros((2, 3, 3, 4, 4)), None):
        with pytest.raises(ValueError, match=r"y must be \(2, 3, 3, 4, 4\)"):
            check_measurement(bad, shape, 2, False)
    with pytest.raises(ValueError, match=r"y must be \(2, 3, 1, 4, 4\)"):
        check_measurement(y, shape, 2, True)
    for v in (float("nan"), float("inf"), -float("inf")):
        z = y.clone()
        z[1, 2, 0, 3, 3] = v
        with pytest.raises(ValueError, match="y must be finite"):
            check_measurement(z, shape, 2, False)
    with pytest.raises(ValueError, match="a .B, T, 3, H, W. tensor"):
        measure(np.zeros(shape), 2, False)
    with pytest.raises(ValueError, match="identity"):
        measure(torch.zeros(shape), 1, False)


# ---------------------------------------------------------------------------------------------------------------- the scope
class _FakeLib:
    """Stand-in for the library: the measurement the engine holds, and every call that set it."""

    def __init__(self):
        self.meas, self.sets = None, []

    def vd_set_measurement(self, handle, y, scale, gray):
        self.meas = None if y is None else (y.value, scale, gray)
        self.sets.append(self.meas)
        return 0


class _FakeModel:
    _handle = 17
    device = torch.device("cpu")


def test_scope_sets_restores_nests_and_refuses(monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    model = _FakeModel()
    diff = create_gaussian_diffusion(timestep_respacing="ddim10")
    model._bound_schedule = diff                                                 # (bound already: no upload)
    x = torch.zeros(1, 2, 3, 8, 8)
    ya, yb = torch.zeros(1, 2, 3, 2, 2), torch.ones(1, 2, 1, 8, 8)
    with diff.measurement_scope(model, ya, scale=4):
        outer = fake.meas
        assert outer == (model._measurement["y"].data_ptr(), 4, 0)
        with diff.measurement_scope(model, yb, gray=True):
            assert fake.meas == (model._measurement["y"].data_ptr(), 1, 1) and fake.meas[0] != outer[0]
        assert fake.meas == outer and torch.equal(model._measurement["y"], ya)
    assert fake.meas is None and model._measurement is None
    with pytest.raises(RuntimeError, match="boom"):
        with diff.measurement_scope(model, ya, 4):
            raise RuntimeError("boom")
    assert fake.meas is None and model._measurement is None
    before = len(fake.sets)
    for bad, kw, what in ((ya, dict(scale=3), "cell size"), (ya, dict(scale=1), "identity"), (ya, dict(scale=4, gray=True), "y must be"),
                          (ya * float("nan"), dict(scale=4), "finite"), (torch.zeros(3, 2, 2), dict(scale=4), "y must be a")):
        with pytest.raises(ValueError, match=what):
            with diff.measurement_scope(model, bad, **kw):
                pass
    assert len(fake.sets) == before                                              # a refused measurement never reached the engine
    t = torch.tensor([1])
    with diff.measurement_scope(model, ya, 4):
        for call, what in ((lambda: diff.ddim_reverse_sample(model, x, t), "ddim_reverse_sample"),
                           (lambda: diff.p_sample(model, x, t, denoised_fn=lambda v: v), "denoised_fn"),
                           (lambda: diff.ddim_sample(model, x, t, denoised_fn=lambda v: v), "denoised_fn"),
                           (lambda: diff.dpmpp_2m_sample(model, x, t, denoised_fn=lambda v: v), "denoised_fn"),
                           (lambda: diff.p_mean_variance(model, x, t, denoised_fn=lambda v: v), "denoised_fn"),
                           (lambda: diff.p_sample(model, x, t, use_gradient_method=True), "use_gradient_method"),
                           (lambda: diff.p_mean_variance(model, x, t, use_gradient_method=True), "use_gradient_method")):
            with pytest.raises(_lib.VdError, match=f"{what} inside measurement_scope is not served"):
                call()
    assert "extension" in GaussianDiffusion.measurement_scope.__doc__ and "DDNM" in GaussianDiffusion.measurement_scope.__doc__


# ---------------------------------------------------------------------------------------------------------------- the job's options
def test_options_suffixes_and_keyword_surface():
    parse = video_sample.build_parser().parse_args
    for argv, want, suffix in ((["--measurement", "y.npy", "--sr_scale", "4"], ("y.npy", 4, False), "_sr4"),
                               (["--measurement", "y.npy", "--gray"], ("y.npy", 1, True), "_gray"),
                               (["--measurement", "y.npy", "--sr_scale", "4", "--gray"], ("y.npy", 4, True), "_sr4gray"),
                               (["--measurement", "y.npy", "--sr_scale", "8", "--gray", "true"], ("y.npy", 8, True), "_sr8gray"),
                               (["--measurement", "y.npy", "--sr_scale", "2"], ("y.npy", 2, False), "_sr2")):
        args = parse(argv)
        assert (args.measurement, args.sr_scale, args.gray) == want
        assert video_sample.run_postfix(args) == suffix
    args = parse(["--measurement", "y.npy", "--sr_scale", "4", "--sampler", "ddim", "--cfg_scale", "2"])
    assert video_sample.run_postfix(args) == "_ddim_cfg2_sr4"                     # appended the way '_known' is: last
    plain = parse([])
    assert (plain.measurement, plain.sr_scale, plain.gray) == (None, 1, False) and video_sample.run_postfix(plain) == ""
    with pytest.raises(SystemExit):
        parse(["--sr_scale", "3"])
    sig = inspect.signature(video_sample.infer_video).parameters
    for name, default in (("measurement", None), ("sr_scale", 1), ("gray", False)):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == default
    sig = inspect.signature(WindowExecutor.begin).parameters
    for name, default in (("measurement", None), ("sr_scale", 1), ("gray", False)):
        assert sig[name].default == default
    assert list(inspect.signature(GaussianDiffusion.measurement_scope).parameters) == ["self", "model", "y", "scale", "gray"]
    for name in ("vd_set_measurement", "vd_measurement", "vd_measurement_project"):
        assert name in _lib.SIGNATURES
    assert "measure.hip" in _lib.SOURCES


def test_job_reads_the_measurement_rows_of_its_batch(tmp_path):
    y = np.random.RandomState(0).randn(5, 6, 1, 2, 2).astype(F)
    path = tmp_path / "y.npy"
    np.save(path, y)
    args = video_sample.build_parser().parse_args(["--measurement", str(path), "--sr_scale", "4", "--gray"])
    args._batch_ids = [3, 1]
    kw = video_sample._measurement_options(args, torch.zeros(2, 4, 3, 8, 8))
    assert kw["sr_scale"] == 4 and kw["gray"] is True and np.array_equal(kw["measurement"].numpy(), y[[3, 1], :4])
    assert video_sample._measurement_options(video_sample.build_parser().parse_args([]), torch.zeros(2, 4, 3, 8, 8)) == {}
    np.save(path, y[0])
    with pytest.raises(ValueError, match="--measurement is"):
        video_sample._measurement_options(args, torch.zeros(2, 4, 3, 8, 8))


# ---------------------------------------------------------------------------------------------------------------- infer_video's gather
class _StubModel:
    device = torch.device("cpu")

    def check_device_errors(self):
        pass


class _StubDiffusion:
    """Two steps per window; records the measurement and the frame indices every window's steps ran under."""
    num_timesteps = 2

    def __init__(self):
        self.windows, self._y = [], None

    @contextlib.contextmanager
    def measurement_scope(self, model, y, scale=1, gray=False):
        self._y = (y.clone(), scale, gray)
        try:
            yield
        finally:
            self._y = None

    def ddim_sample(self, model, x, t, clip_denoised=True, model_kwargs=None, eta=0.0, cfg_scale=1.0):
        if int(t[0]) == self.num_timesteps - 1:
            self.windows.append((model_kwargs["frame_indices"].clone(), model_kwargs["latent_mask"].clone(), self._y))
        assert self._y is not None
        return {"sample": x + 1.0, "pred_xstart": x}


def test_infer_video_gathers_the_measurement_per_window():
    B, T, H = 2, 9, 8
    g = torch.Generator().manual_seed(0)
    batch = torch.rand(B, T, 3, H, H, generator=g)
    y = measure(batch, 4, True) + 0.25
    diff = _StubDiffusion()
    out, _ = video_sample.infer_video("autoreg", _StubModel(), diff, batch, 5, 2, sampler="ddim", measurement=y, sr_scale=4, gray=True)
    assert len(diff.windows) >= 2
    seen = set()
    for fi, lat, (yw, scale, gray) in diff.windows:
        assert (scale, gray) == (4, True) and yw.shape == (B, fi.shape[1], 1, 2, 2)
        for i in range(B):
            for w, f in enumerate(fi[i].tolist()):
                assert torch.equal(yw[i, w], y[i, f])                            # gathered by the frame indices, exactly as x0 is
        seen |= {f for w, f in enumerate(fi[0].tolist()) if float(lat.reshape(B, -1)[0, w]) == 1}
    assert seen == set(range(2, T))
    assert np.array_equal(out[:, :2], batch[:, :2].numpy())                      # the observed frames come from `batch`
    # without a measurement no scope is entered
    diff2 = _StubDiffusion()
    diff2.ddim_sample = lambda model, x, t, **kw: {"sample": x, "pred_xstart": x}
    diff2.measurement_scope = None
    video_sample.infer_video("autoreg", _StubModel(), diff2, batch, 5, 2, sampler="ddim")
    # the checks run before anything touches the engine
    for kw, err, what in ((dict(measurement=y, sr_scale=2, gray=True), ValueError, "y must be"),
                          (dict(measurement=y * float("inf"), sr_scale=4, gray=True), ValueError, "finite"),
                          (dict(measurement=y, sr_scale=4, gray=True, known_mask=torch.ones(T, H, H)), _lib.VdError, "known region"),
                          (dict(measurement=y, sr_scale=4, gray=True, use_gradient_method=True), _lib.VdError, "use_gradient_method")):
        with pytest.raises(err, match=what):
            video_sample.infer_video("autoreg", object(), object(), batch, 5, 2, **kw)
