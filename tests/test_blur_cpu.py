"""CPU: deblurring (this project's extension) -- the restatement (tests/blur_restated.py) against torch.nn.functional.conv2d and autograd
in float64, the adjoint identity, the float32 restatement inside its own bound, the host helpers blur / gaussian_kernel /
check_blur_kernel rule by rule, the parser's options and the run directory, and the new names in the C ABI and the signatures."""
import inspect

import numpy as np
import pytest
import torch

from blur_restated import (RHO_MIN, SHAPES, apply_bound, assert_unambiguous, blur_f32, blur_fp64, deblur_bound, deblur_f32, deblur_fp64,
                           gaussian_taps, one_hot_taps, random_taps, seed_inputs, shifted)
from step_nll_restated import ratio, tables
from video_diffusion_amd import _lib, video_sample
from video_diffusion_amd.executor import WindowExecutor
from video_diffusion_amd.gaussian_diffusion import GaussianDiffusion, blur, check_blur_kernel, gaussian_kernel
from video_diffusion_amd.script_util import create_gaussian_diffusion

SMALL = [s for s in SHAPES if s[0] * s[1] <= 32 * 32]


@pytest.fixture(scope="module")
def tab():
    return tables(create_gaussian_diffusion(timestep_respacing="ddim50"))


def _conv(x, w):
    x, w = torch.as_tensor(x, dtype=torch.float64), torch.as_tensor(w, dtype=torch.float64)
    k = w.shape[0]
    return torch.nn.functional.conv2d(x.reshape(-1, 1, *x.shape[-2:]), w.reshape(1, 1, k, k), padding=k // 2).reshape(x.shape)


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("H,W,k", SHAPES)
def test_restatement_is_conv2d_and_its_adjoint(H, W, k):
    g = np.random.default_rng(100 + H + W + k)
    w = random_taps(k, seed=k)
    u, v = g.standard_normal((2, 2, 3, H, W)), g.standard_normal((2, 2, 3, H, W))
    Au = blur_fp64(u, w)
    assert np.allclose(Au, _conv(u, w).numpy(), rtol=1e-12, atol=1e-13)
    # <A u, v> = <u, A^T v>: the adjoint is exact with zero padding
    lhs, rhs = float((Au * v).sum()), float((u * blur_fp64(v, w, adjoint=True)).sum())
    assert abs(lhs - rhs) <= 1e-11 * max(1.0, abs(lhs))
    # ... and it is autograd's
    U_ = torch.tensor(u, requires_grad=True)
    (_conv(U_, w) * torch.tensor(v)).sum().backward()
    assert np.allclose(U_.grad.numpy(), blur_fp64(v, w, adjoint=True), rtol=1e-12, atol=1e-13)
    # a one-hot tap off centre is a pure shift, for A and for A^T, in both arithmetics, to the bit
    c = k // 2
    for di, dj in {(0, 0), (-c, c), (c, -min(c, 1)), (min(c, 2), c)}:
        u32 = u.astype(np.float32)
        assert np.array_equal(blur_f32(u32, one_hot_taps(k, c + di, c + dj)), shifted(u32, di, dj))
        assert np.array_equal(blur_f32(u32, one_hot_taps(k, c - di, c - dj), adjoint=True), shifted(u32, di, dj))
        assert np.array_equal(blur_fp64(u, one_hot_taps(k, c + di, c + dj)), shifted(u, di, dj))
    if c:                                                              # zeros enter at the two edges the shift leaves
        s = shifted(np.ones((H, W)), -c, c)
        assert not s[:min(c, H)].any() and not s[:, max(W - c, 0):].any() and (H <= c or W <= c or s[c:, :W - c].all())


@pytest.mark.parametrize("H,W,k", SMALL)
@pytest.mark.parametrize("kind", ["random", "gaussian"])
def test_float32_apply_inside_the_bound(H, W, k, kind):
    w = random_taps(k, seed=3 * k) if kind == "random" else gaussian_taps(k)
    x = np.random.default_rng(7 + k).standard_normal((2, 2, 3, H, W)).astype(np.float32)
    for adj in (False, True):
        want, bound = apply_bound(x, w, adj)
        r = ratio(blur_f32(x, w, adj), want, bound)
        assert r.max() <= 1.0, (adj, float(r.max()))
        # a rounding bound, not a tolerance: well below a relative 1e-4 of the largest output
        assert bound.max() < 1e-4 * np.abs(want).max()


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("H,W,k", [(8, 8, 3), (6, 10, 5), (7, 7, 1), (12, 8, 7)])
def test_cotangent_is_autograd_of_the_residual_norm(tab, H, W, k, clip):
    """q (through the clamp), d eps and d_x of the float64 restatement against torch.autograd.grad of rho_b through conv2d in float64;
    the float32 restatement inside the derived bound."""
    w = random_taps(k, seed=40 + k)
    xt, eps, t, y, lat = seed_inputs(tab, 2, 3, H, W, w, clip, seed=11 + k)
    assert_unambiguous(tab, xt, eps, t, y, lat, w, clip)
    ex = deblur_fp64(tab, xt, eps, t, y, lat, w, clip)
    a = torch.tensor(tab["sr"][t].astype(np.float64)).reshape(-1, 1, 1, 1, 1)
    b = torch.tensor(tab["srm1"][t].astype(np.float64)).reshape(-1, 1, 1, 1, 1)
    X = torch.tensor(xt.astype(np.float64), requires_grad=True)
    E = torch.tensor(eps.astype(np.float64), requires_grad=True)
    x0r = a * X - b * E
    x0r.retain_grad()
    x0 = x0r.clamp(-1, 1) if clip else x0r
    r = (torch.tensor(y.astype(np.float64)) - _conv(x0, w)) * torch.tensor(lat.astype(np.float64)).reshape(2, 3, 1, 1, 1)
    rho = r.reshape(2, -1).pow(2).sum(dim=1).sqrt()
    rho.sum().backward()
    assert np.allclose(rho.detach().numpy(), ex["rho"], rtol=1e-13, atol=0) and (ex["rho"] >= RHO_MIN).all()
    for got, want in ((ex["q"] * ex["mask"], x0r.grad), (ex["deps"], E.grad), (ex["dxd"], X.grad)):
        assert np.allclose(got, want.numpy(), rtol=1e-11, atol=1e-15), float(np.abs(got - want.numpy()).max())
    assert not ex["deps"][:, 1].any() and not ex["dxd"][:, 1].any() and ex["deps"][:, 0].any()        # the frame that is not latent
    if clip:
        assert (~ex["mask"]).mean() > 0.15 and not ex["dxd"][~ex["mask"]].any()
    f32 = deblur_f32(tab, xt, eps, t, y, lat, w, clip)
    lim = deblur_bound(tab, xt, eps, t, y, lat, w, clip)
    for name in ("deps", "dxd", "rho"):
        want, bound = lim[name]
        rr = ratio(f32[name], want, bound)
        assert rr.max() <= 1.0 and f32[name].dtype == np.float32, (name, float(rr.max()))
    want, bound = lim["dxd"]
    i = np.unravel_index(np.argmax(np.abs(want)), want.shape)
    assert abs(want[i]) * 1e-2 > bound[i] > 0                          # a rounding bound, not a tolerance


def test_empty_and_zero_items(tab):
    w = gaussian_taps(3)
    xt, eps, t, y, lat = seed_inputs(tab, 2, 2, 8, 8, w, True, seed=5)
    lat[0] = 0
    ex, lim = deblur_fp64(tab, xt, eps, t, y, lat, w, True), deblur_bound(tab, xt, eps, t, y, lat, w, True)
    assert ex["rho"][0] == 0 and not ex["deps"][0].any() and np.isfinite(ex["deps"]).all() and lim["rho"][1][0] == 0
    assert not lim["deps"][1][0].any() and ex["rho"][1] > 0
    f32 = deblur_f32(tab, xt, eps, t, y, lat, w, True)
    assert f32["rho"][0] == 0 and not f32["deps"][0].any() and np.isfinite(f32["dxd"]).all()


# ---------------------------------------------------------------------------------------------------------------- the host helpers
def test_blur_is_conv2d_and_keeps_float64():
    g = torch.Generator().manual_seed(2)
    v = torch.rand(2, 3, 3, 9, 7, generator=g, dtype=torch.float64)
    w = torch.tensor(random_taps(5, seed=1))
    y = blur(v, w)
    assert y.dtype == torch.float64 and y.shape == v.shape and y.is_contiguous()
    assert np.allclose(y.numpy(), blur_fp64(v.numpy(), w.numpy()), rtol=1e-13, atol=1e-14)
    y32 = blur(v.float(), w.numpy())
    assert y32.dtype == torch.float32 and np.allclose(y32.numpy(), y.numpy(), atol=1e-5)
    assert blur(v.half(), w).dtype == torch.float32
    w64 = torch.rand(3, 3, generator=g, dtype=torch.float64)           # float64 taps on a float64 video are taken as given
    assert np.allclose(blur(v, w64).numpy(), blur_fp64(v.numpy(), w64.numpy()), rtol=1e-13, atol=1e-14)
    assert GaussianDiffusion.blur is blur and GaussianDiffusion.gaussian_kernel is gaussian_kernel
    for bad in (v[0], torch.zeros(1, 2, 1, 4, 4), "no"):
        with pytest.raises(ValueError, match=r"blur: a \(B, T, 3, H, W\) tensor"):
            blur(bad, w)


def test_gaussian_kernel():
    for size, sigma in ((1, 1.0), (3, 0.5), (9, 2.0), (15, 3.5)):
        w = gaussian_kernel(size, sigma)
        assert w.dtype == torch.float32 and w.shape == (size, size)
        assert np.array_equal(w.numpy(), gaussian_taps(size, sigma))   # normalised in float64, rounded once
        assert abs(float(w.double().sum()) - 1.0) < size * size * 2.0 ** -24 and torch.equal(w, w.T) and torch.equal(w, w.flip(0, 1))
        assert float(w[size // 2, size // 2]) == float(w.max())
    for size in (0, 2, 17, -3, 3.0, True, None):
        with pytest.raises(ValueError, match="size=.* must be an odd integer in .1, 15."):
            gaussian_kernel(size, 1.0)
    for sigma in (0, -1.0, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="sigma=.* must be positive and finite"):
            gaussian_kernel(3, sigma)


def test_check_blur_kernel_every_rule():
    ok = check_blur_kernel(np.arange(9.0).reshape(3, 3))
    assert ok.dtype == torch.float32 and ok.shape == (3, 3) and ok.is_contiguous() and ok.device.type == "cpu"
    assert torch.equal(check_blur_kernel(torch.ones(15, 15, dtype=torch.float64)), torch.ones(15, 15))
    assert torch.equal(check_blur_kernel([[2]]), torch.tensor([[2.0]]))
    neg = torch.tensor(random_taps(7, seed=2))
    assert torch.equal(check_blur_kernel(neg.T), neg.T.contiguous())   # signed, asymmetric, not normalised, not contiguous: served
    for bad, what in ((torch.ones(3), "2-D and square"), (torch.ones(3, 5), "2-D and square"), (torch.ones(1, 3, 3), "2-D and square"),
                      (torch.ones(0, 0), "2-D and square"), (torch.ones(4, 4), "k=4 must be odd"), (torch.ones(17, 17), "k=17 must be at most 15"),
                      (torch.tensor([[float("nan")]]), "must be finite"), (torch.tensor([[1.0, 0, 0], [0, float("inf"), 0], [0, 0, 0]]), "must be finite"),
                      (torch.tensor([[1e39]], dtype=torch.float64), "must be finite"), (torch.zeros(3, 3), "must not be all zero"),
                      (torch.ones(3, 3, dtype=torch.bool), "must hold real numbers"), (torch.ones(3, 3, dtype=torch.complex64), "must hold real numbers"),
                      (object(), "2-D"), (None, "2-D")):
        with pytest.raises(ValueError, match=what):
            check_blur_kernel(bad)


# ---------------------------------------------------------------------------------------------------------------- options and names
def test_options_suffix_and_names(tmp_path, capsys):
    ap = video_sample.build_parser()
    parse = lambda argv: video_sample.check_particle_arguments(ap, ap.parse_args(argv))      # noqa: E731
    np.save(tmp_path / "k.npy", random_taps(7, seed=1))
    kf = str(tmp_path / "k.npy")
    for argv, suffix in ((["--measurement", "y.npy", "--blur_kernel", kf, "--dps_zeta", "0.5"], "_blur7_dps0.5"),
                         (["--measurement", "y.npy", "--blur_sigma", "1.5", "--blur_size", "9", "--dps_zeta", "2", "--sampler", "ddim"], "_ddim_blur9_dps2"),
                         (["--measurement", "y.npy", "--blur_sigma", "1", "--dps_zeta", "1"], "_blur7_dps1"),
                         (["--measurement", "y.npy", "--blur_sigma", "9", "--dps_zeta", "1"], "_blur15_dps1"),
                         (["--measurement", "y.npy", "--blur_kernel", kf, "--particles", "4", "--measurement_sigma", "0.1"], "_blur7_smc4"),
                         (["--measurement", "y.npy", "--sr_scale", "4", "--dps_zeta", "0.5"], "_sr4_dps0.5")):
        assert video_sample.run_postfix(parse(argv)) == suffix
    a = parse([])
    assert a.blur_kernel is None and a.blur_sigma is None and a.blur_size is None and video_sample.blur_kernel_of(a) is None
    w = video_sample.blur_kernel_of(parse(["--measurement", "y.npy", "--blur_sigma", "1.5", "--blur_size", "9", "--dps_zeta", "1"]))
    assert torch.equal(w, gaussian_kernel(9, 1.5))
    for argv, what in ((["--measurement", "y.npy", "--blur_kernel", kf], "need --dps_zeta Z, or --particles K with --measurement_sigma"),
                       (["--blur_kernel", kf, "--dps_zeta", "1"], "need --measurement"),
                       (["--measurement", "y.npy", "--blur_kernel", kf, "--blur_sigma", "1", "--dps_zeta", "1"], "two kernels"),
                       (["--measurement", "y.npy", "--blur_size", "5", "--dps_zeta", "1", "--sr_scale", "4"], "--blur_size needs --blur_sigma"),
                       (["--measurement", "y.npy", "--blur_sigma", "0", "--dps_zeta", "1"], "--blur_sigma S: positive"),
                       (["--measurement", "y.npy", "--blur_sigma", "1", "--blur_size", "4", "--dps_zeta", "1"], "--blur_size N: odd"),
                       (["--measurement", "y.npy", "--blur_sigma", "1", "--dps_zeta", "1", "--sr_scale", "4"], "together with --sr_scale or --gray"),
                       (["--measurement", "y.npy", "--blur_sigma", "1", "--dps_zeta", "1", "--gray"], "together with --sr_scale or --gray")):
        with pytest.raises(SystemExit):
            parse(argv)
        assert what in capsys.readouterr().err, argv
    # the job's keywords: y has the video's shape; either the gradient step or the particles' reward
    np.save(tmp_path / "y.npy", np.zeros((3, 4, 3, 8, 8), np.float32))
    yf = str(tmp_path / "y.npy")
    args = parse(["--measurement", yf, "--blur_kernel", kf, "--dps_zeta", "0.5"])
    args._batch_ids = [2, 0]
    kw = video_sample._measurement_options(args, torch.zeros(2, 4, 3, 8, 8))
    assert set(kw) == {"measurement", "blur_kernel", "dps_zeta"} and kw["measurement"].shape == (2, 4, 3, 8, 8) and kw["blur_kernel"].shape == (7, 7)
    args = parse(["--measurement", yf, "--blur_sigma", "1", "--particles", "2", "--measurement_sigma", "0.2"])
    args._batch_ids = [1]
    kw = video_sample._measurement_options(args, torch.zeros(1, 4, 3, 8, 8))
    assert set(kw) == {"particle_measurement", "sigma_y", "blur_kernel"} and kw["sigma_y"] == 0.2


def test_infer_video_refusals_before_the_engine():
    batch = torch.zeros(1, 5, 3, 8, 8)
    w = gaussian_kernel(3, 1.0)
    run = lambda **kw: video_sample.infer_video("autoreg", object(), object(), batch, 5, 2, **kw)      # noqa: E731
    with pytest.raises(_lib.VdError, match="blur_kernel without dps_zeta or particles is not served: measurement_scope together with a blur is "
                                           "refused, the exact projection has no pseudo-inverse"):
        run(measurement=batch, blur_kernel=w)
    with pytest.raises(ValueError, match="blur_kernel needs a measurement"):
        run(blur_kernel=w, dps_zeta=0.5)
    with pytest.raises(ValueError, match="blur_kernel together with sr_scale or gray"):
        run(measurement=batch, blur_kernel=w, dps_zeta=0.5, sr_scale=4)
    with pytest.raises(ValueError, match="k=4 must be odd"):
        run(measurement=batch, blur_kernel=torch.ones(4, 4), dps_zeta=0.5)
    with pytest.raises(ValueError, match="y must have the video's shape"):
        run(measurement=torch.zeros(1, 5, 3, 4, 4), blur_kernel=w, dps_zeta=0.5)
    with pytest.raises(ValueError, match="y must have the video's shape"):
        run(measurement=torch.zeros(1, 5, 3, 4, 4), blur_kernel=w, particles=2, sigma_y=0.1, sampler="ddim", eta=1.0)
    with pytest.raises(_lib.VdError, match="executor='graph' together with dps_zeta is not served"):
        run(measurement=batch, blur_kernel=w, dps_zeta=0.5, executor="graph")
    with pytest.raises(NotImplementedError, match="at eta = 0 together with particles is not served"):
        run(measurement=batch, blur_kernel=w, particles=2, sigma_y=0.1, sampler="ddim")


def test_signatures_and_the_c_abi():
    P = inspect.Parameter
    sig = inspect.signature(GaussianDiffusion.deblur_scope).parameters
    assert list(sig) == ["self", "model", "y", "kernel", "zeta"] and sig["zeta"].kind is P.KEYWORD_ONLY and sig["zeta"].default is P.empty
    sig = inspect.signature(GaussianDiffusion.steering_scope).parameters
    assert sig["blur_kernel"].kind is P.KEYWORD_ONLY and sig["blur_kernel"].default is None
    assert sig["sr_scale"].default == 1 and sig["gray"].default is False
    for fn in (video_sample.infer_video, WindowExecutor.begin, WindowExecutor.sample_window):
        assert inspect.signature(fn).parameters["blur_kernel"].default is None, fn
    assert inspect.signature(video_sample.infer_video).parameters["blur_kernel"].kind is P.KEYWORD_ONLY
    # the scopes this feature stands beside keep their parameter lists
    assert list(inspect.signature(GaussianDiffusion.dps_scope).parameters) == ["self", "model", "y", "scale", "gray", "zeta"]
    assert list(inspect.signature(GaussianDiffusion.measurement_scope).parameters) == ["self", "model", "y", "scale", "gray"]
    header = open(_lib.HEADER).read()
    for name, n in (("vd_set_blur_kernel", 3), ("vd_blur_kernel", 2), ("vd_deblur_step", 22), ("vd_op_deblur_seed", 18), ("vd_op_blur", 10),
                    ("vd_set_particle_blur", 2), ("vd_particle_blur", 1)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n, name
        assert f"int {name}(" in header, name
    assert len(_lib.SIGNATURES["vd_deblur_step"][1]) == len(_lib.SIGNATURES["vd_dps_step"][1]) - 2      # vd_dps_step's list without scale, gray
    assert len(_lib.SIGNATURES["vd_set_particles"][1]) == 8                                             # unchanged
    assert "blur.hip" in _lib.SOURCES
    src = open(_lib.os.path.join(_lib._CSRC, "blur.hip")).read()
    for kernel in ("blur_residual_kernel", "blur_seed_kernel", "blur_apply_kernel"):
        assert f"void {kernel}(" in src
    assert "atomicAdd" not in src                                                                       # no floating-point atomics
