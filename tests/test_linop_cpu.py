"""CPU: separable linear measurements -- the host helpers against torch's own resampler, `blur` and `measure` in float64, the truncated
pseudo-inverse, every ValueError by message, and the float32 restatement (tests/linop_restated.py) inside the restated bound of the
float64 one for every operator shape the GPU tests use.  No engine is touched."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import linop_restated as lr
from step_nll_restated import ratio, tables
from video_diffusion_amd import _lib, gaussian_diffusion as gd
from video_diffusion_amd.gaussian_diffusion import (blur, blur_matrix, box_matrix, check_separable_operator, gaussian_kernel, measure,
                                                    measure_separable, resize_matrix, separable_pinv)
from video_diffusion_amd.script_util import create_gaussian_diffusion

# float64 rounding of a sum of at most 128 terms of magnitude max|x| (128 * 2^-53 = 1.4e-14), with headroom: not a tuning knob
BAR = 1e-13
RESIZE_PAIRS = [(64, 16), (32, 16), (128, 16), (128, 32), (32, 8)]


def _video(n, seed, B=2, T=2):
    return torch.rand(B, T, 3, n, n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2 - 1


def _gauss1d(k, sigma):
    ax = torch.arange(k, dtype=torch.float64) - k // 2
    g = torch.exp(-(ax * ax) / (2.0 * sigma ** 2))
    return g / g.sum()


@pytest.mark.parametrize("mode", ["bicubic", "bilinear"])
@pytest.mark.parametrize("n,m", RESIZE_PAIRS)
def test_resize_matrix_is_torchs_resampler(n, m, mode):
    A = resize_matrix(n, m, mode)
    assert A.shape == (m, n) and A.dtype == torch.float64
    x = _video(n, 10 + n + m)
    want = TF.interpolate(x.reshape(-1, 3, n, n), size=(m, m), mode=mode, antialias=True, align_corners=False).reshape(2, 2, 3, m, m)
    got = measure_separable(x, A, A)
    err = float((got - want).abs().max())
    print(f"{mode} {n}->{m}: max |A x A^T - interpolate| = {err:.2e}")
    assert got.dtype == torch.float64 and err <= BAR * float(x.abs().max())
    assert float((A.sum(dim=1) - 1).abs().max()) <= BAR                             # a resampler keeps a constant


def test_resize_matrix_without_antialias_and_rectangular():
    x = _video(32, 5)[..., :, :24]
    A_h, A_w = resize_matrix(32, 8, "bilinear", antialias=False), resize_matrix(24, 12, "bicubic", antialias=False)
    for ax_h, ax_w, mode in ((A_h, resize_matrix(24, 12, "bilinear", antialias=False), "bilinear"),
                             (resize_matrix(32, 8, "bicubic", antialias=False), A_w, "bicubic")):
        want = TF.interpolate(x.reshape(-1, 3, 32, 24), size=(8, 12), mode=mode, antialias=False, align_corners=False).reshape(2, 2, 3, 8, 12)
        assert float((measure_separable(x, ax_h, ax_w) - want).abs().max()) <= BAR * float(x.abs().max())


@pytest.mark.parametrize("n,k,sigma", [(64, 9, 2.0), (32, 7, 1.5), (16, 15, 4.0), (8, 15, 3.0)])
def test_blur_matrix_zeros_is_blur(n, k, sigma):
    g = _gauss1d(k, sigma)
    A = blur_matrix(n, g)
    x = _video(n, 20 + n)
    want = blur(x, torch.outer(g, g))
    got = measure_separable(x, A, A)
    assert A.shape == (n, n) and float((got - want).abs().max()) <= BAR * float(x.abs().max())
    # an asymmetric kernel pins the orientation: correlation, as `blur`
    w = torch.tensor([0.5, 0.25, 0.0, -1.0, 2.0], dtype=torch.float64)[:min(5, 2 * (n // 2) - 1)]
    a, b = blur_matrix(n, w), blur_matrix(n, w.flip(0))
    assert float((measure_separable(x, a, b) - blur(x, torch.outer(w, w.flip(0)))).abs().max()) <= BAR * 4 * float(x.abs().max())


def test_blur_matrix_padding_and_stride():
    n, g = 12, _gauss1d(5, 1.0)
    x = torch.rand(1, 1, n, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    for padding, mode in (("reflect", "reflect"), ("circular", "circular"), ("zeros", "constant")):
        for stride in (1, 2, 3, 5):
            A = blur_matrix(n, g, stride=stride, padding=padding)
            want = TF.conv1d(TF.pad(x, (2, 2), mode=mode), g.reshape(1, 1, 5), stride=stride).reshape(-1)
            assert A.shape == (-(-n // stride), n)
            assert float((A @ x.reshape(-1) - want).abs().max()) <= BAR
    assert torch.equal(blur_matrix(6, [1.0]), torch.eye(6, dtype=torch.float64))


@pytest.mark.parametrize("n,s", [(8, 2), (32, 4), (64, 8), (12, 4), (128, 8), (8, 1)])
def test_box_matrix_is_measure(n, s):
    A = box_matrix(n, s)
    x = _video(n, 30 + n)
    assert A.shape == (n // s, n)
    if s > 1:
        assert float((measure_separable(x, A, A) - measure(x, s)).abs().max()) <= BAR * float(x.abs().max())
    else:
        assert torch.equal(A, torch.eye(n, dtype=torch.float64))


def test_measure_separable_dtypes():
    A = resize_matrix(8, 2)
    x = _video(8, 1)
    assert measure_separable(x, A, A).dtype == torch.float64 and measure_separable(x.float(), A, A).dtype == torch.float32
    assert measure_separable(x.half(), A, A).dtype == torch.float32
    a32 = check_separable_operator(A, A)[0]
    assert torch.equal(measure_separable(x.float(), A, A), a32 @ x.float() @ a32.T)
    diff = create_gaussian_diffusion(timestep_respacing="ddim50")
    assert torch.equal(diff.measure_separable(x, A, A), measure_separable(x, A, A))


@pytest.mark.parametrize("n,m", RESIZE_PAIRS)
def test_pinv_full_rank_bicubic(n, m):
    A = resize_matrix(n, m)
    P, rank = separable_pinv(A)
    assert rank == m and P.shape == (n, m) and P.dtype == torch.float32
    S = torch.linalg.svdvals(A)
    print(f"bicubic {n}->{m}: sigma_max / sigma_min = {float(S[0] / S[-1]):.3f}, max |P| = {float(P.abs().max()):.3f}")
    # A P A = A in float64 on the unrounded pseudo-inverse; the float32 P is its single rounding
    U_, S_, Vh = torch.linalg.svd(A, full_matrices=False)
    Pex = (Vh.T / S_) @ U_.T
    assert float((A @ Pex @ A - A).abs().max()) <= 1e-12
    assert torch.equal(P, Pex.to(torch.float32))
    a32, p32 = A.float(), P
    print(f"  float32: max |A P - I| = {float((a32 @ p32 - torch.eye(m)).abs().max()):.2e}")


def test_pinv_truncates_an_ill_conditioned_blur():
    A = blur_matrix(64, _gauss1d(9, 2.0))
    S = torch.linalg.svdvals(A)
    P, rank = separable_pinv(A, rtol=1e-3)
    assert rank == 62 == int((S > 1e-3 * S[0]).sum()), (rank, float(S[-1]))
    assert float(P.abs().max()) <= 51.0 * 1.01
    full, rank_full = separable_pinv(A, rtol=0.0)
    assert rank_full == 64 and float(full.abs().max()) > float(P.abs().max())       # the dropped directions carry the largest entries
    # on the kept subspace the truncated inverse is exact: A P A v = A v for v in the span of the kept right vectors
    _, _, Vh = torch.linalg.svd(A)
    v = Vh[:62].T @ torch.randn(62, 3, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    assert float((A @ (P.double() @ (A @ v)) - A @ v).abs().max()) <= 1e-4              # P is float32: 51 * 2^-24 * |A v|


def test_value_errors_by_message():
    ok = np.eye(4, dtype=np.float32)
    for bad, what in (((np.zeros(4), ok), "A_h must be 2-D"), ((ok, np.zeros((2, 2, 2))), "A_w must be 2-D"),
                      ((np.zeros((4, 4)), ok), "A_h must not be all zero"), ((ok, np.full((2, 4), np.nan)), "A_w must be finite"),
                      ((np.ones((5, 4)), ok), "M <= n"), ((np.ones((2, 129)), ok), "at most 128"), ((ok.astype(bool), ok), "real numbers"),
                      ((ok.astype(np.complex64), ok), "real numbers"), (("no", ok), "A_h must be")):
        with pytest.raises(ValueError, match=what):
            check_separable_operator(*bad)
    a, b = check_separable_operator(np.ones((2, 4), np.float64), torch.ones(3, 4, dtype=torch.int32))
    assert a.dtype == b.dtype == torch.float32 and a.is_contiguous() and a.device.type == "cpu"
    for kw, what in ((dict(rtol=-1e-3), "rtol"), (dict(rtol=1.0), "rtol"), (dict(rtol="x"), "rtol"), (dict(rtol=True), "rtol")):
        with pytest.raises(ValueError, match=what):
            separable_pinv(ok, **kw)
    with pytest.raises(ValueError, match="finite and not all zero"):
        separable_pinv(np.zeros((2, 4)))
    for args, what in (((0, 1), "n=0"), ((129, 4), "n=129"), ((8, 9), "at most n"), ((8, 0), "m=0"), ((8.0, 2), "n=8.0")):
        with pytest.raises(ValueError, match=what):
            resize_matrix(*args)
    with pytest.raises(ValueError, match="'bicubic' or 'bilinear'"):
        resize_matrix(8, 2, mode="nearest")
    for args, kw, what in (((8, [1.0, 2.0]), {}, "odd number"), ((8, [[1.0]]), {}, "1-D"), ((8, [float("inf")]), {}, "finite"),
                           ((8, [1.0]), dict(stride=0), "stride"), ((8, [1.0]), dict(stride=9), "stride"), ((8, [1.0]), dict(padding="same"), "padding"),
                           ((2, [1.0] * 5), dict(padding="reflect"), "reflect padding needs"), ((200, [1.0]), {}, "n=200")):
        with pytest.raises(ValueError, match=what):
            blur_matrix(*args, **kw)
    for args, what in (((8, 3), "divides"), ((8, 0), "positive integer"), ((8, 2.0), "positive integer"), ((0, 1), "n=0")):
        with pytest.raises(ValueError, match=what):
            box_matrix(*args)
    x = torch.zeros(1, 1, 3, 8, 8)
    for args, what in (((torch.zeros(1, 3, 8, 8), ok, ok), r"\(B, T, 3, H, W\)"), ((x, ok, ok), "against planes of"), (("x", ok, ok), r"\(B, T, 3, H, W\)")):
        with pytest.raises(ValueError, match=what):
            measure_separable(*args)
    A = resize_matrix(8, 2)
    for y, what in ((torch.zeros(1, 1, 3, 2, 3), "y must be"), (torch.full((1, 1, 3, 2, 2), float("nan")), "must be finite"), (None, "y must be")):
        with pytest.raises(ValueError, match=what):
            gd.check_linear_measurement(y, (1, 1, 3, 8, 8), A, A)
    with pytest.raises(ValueError, match="the columns are H and W"):
        gd.check_linear_measurement(torch.zeros(1, 1, 3, 2, 2), (1, 1, 3, 16, 8), A, A)


def test_the_library_lists_the_source_and_the_entries():
    assert "linop.hip" in _lib.SOURCES
    src = open(_lib.os.path.join(_lib._CSRC, "linop.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "atomicAdd" not in src
    header = open(_lib.HEADER).read()
    for name in ("vd_set_linear_operator", "vd_linear_operator", "vd_set_linear_measurement", "vd_linear_measurement", "vd_linear_dps_step",
                 "vd_set_particle_linear", "vd_particle_linear", "vd_op_linop", "vd_op_linear_project", "vd_op_linear_dps_seed"):
        assert name in _lib.SIGNATURES and f"int {name}(" in header, name


# ---------------------------------------------------------------------------------------------------------------- the restatement
def _tab():
    return tables(create_gaussian_diffusion(timestep_respacing="ddim50"))


@pytest.mark.parametrize("H,W,Mh,Mw", lr.SHAPES)
def test_f32_restatement_inside_the_bound(H, W, Mh, Mw):
    """Every output of the float32 restatement lies inside the restated bound of the float64 one: the three uses of the product, the
    residual and seed passes with the clamp on and off, the projection and its identity."""
    tab = _tab()
    B, T = 2, 3 if H <= 72 else 2
    A_h, A_w = lr.random_operator(H, W, Mh, Mw, seed=H + W + Mh)
    P_h, P_w = (separable_pinv(A)[0].numpy() for A in (A_h, A_w))
    g = np.random.default_rng(H * 7 + Mw)
    x = g.standard_normal((B, T, 3, H, W)).astype(np.float32)
    ym = g.standard_normal((B, T, 3, Mh, Mw)).astype(np.float32)
    for name, (L, R), X in (("forward", lr.forward(A_h, A_w), x), ("adjoint", lr.adjoint(A_h, A_w), ym), ("back", (P_h, P_w), ym)):
        want, lim = lr.two_bound(L, X, R)
        r = ratio(lr.two_f32(L, X, R), want, lim)
        print(f"{(H, W, Mh, Mw)} {name}: max |f32 - f64| / bound = {r.max():.3f}")
        assert (r <= 1.0).all(), name
    for clip in (True, False):
        xt, eps, t, y, lat = lr.seed_inputs(tab, B, T, H, W, A_h, A_w, clip, seed=40 + H + Mw)
        lr.assert_unambiguous(tab, xt, eps, t, y, lat, A_h, A_w, clip)
        f32, lim = lr.linop_f32(tab, xt, eps, t, y, lat, A_h, A_w, clip), lr.linop_bound(tab, xt, eps, t, y, lat, A_h, A_w, clip)
        for k in ("r", "rho", "deps", "dxd"):
            r = ratio(f32[k], *lim[k])
            print(f"{(H, W, Mh, Mw)} clip={clip} {k}: max / bound = {r.max():.3f}")
            assert (r <= 1.0).all(), (k, clip)
        assert not f32["deps"][:, 1].any() and f32["deps"][:, 0].any()
        x0 = f32["x0"]
        got = lr.project_f32(x0, y, lat, A_h, A_w, P_h, P_w, clip)
        r = ratio(got, *lr.project_bound(x0, y, lat, A_h, A_w, P_h, P_w, clip))
        assert (r <= 1.0).all() and np.array_equal(got[:, 1], np.clip(x0[:, 1], -1, 1) if clip else x0[:, 1])
        gap = np.abs(lr.two_fp64(A_h, got, A_w) - y.astype(np.float64))
        room = lr.identity_bound(x0, y, lat, A_h, A_w, P_h, P_w, clip)
        sel = np.broadcast_to(lat.reshape(B, T, 1, 1, 1) == 1, y.shape)
        print(f"{(H, W, Mh, Mw)} clip={clip} A x0' - y: max {gap[sel].max():.2e}, max / bound {(gap[sel] / room[sel]).max():.3f}")
        assert (gap[sel] <= room[sel]).all()
