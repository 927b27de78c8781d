"""GPU: separable linear measurements (this project's extension) -- the two-sided product in its three uses, the projection and the
residual and seed passes per element against the float64 restatement (tests/linop_restated.py) inside its derived bound and against the
float32 restatement to the bit; selection and permutation matrices as pure moves; the projected step under three samplers against the
restated projection of the plain step's own x_0, and A pred_xstart = y inside the derived bound; box_matrix against measurement_scope;
linear_dps_scope's gradient against autograd through the CPU oracle at the bars of test_gpu_blur.py, its identities bit for bit; particle
steering on the operator against a reward_fn that computes the same in torch, graph against eager, matrices changed between two windows;
infer_video, the video_sample job, 32 / 33 / 40 frames, and every refusal by message.  Nothing here is tuned on the code under test."""
import numpy as np
import pytest
import torch

import linop_restated as lr
import particle_restated as pr
from helpers import close
from step_nll_restated import ratio, tables
from test_gpu_dpmpp_2m import _rand_window, _t, _window_kw, tiny
from test_gpu_dps import ORACLE_CFG, _dev, _fma32, _plain_xstart
from test_gpu_engine import _oracle
from test_gpu_known_region import _np, _same_bits
from test_gpu_long_window import engine as long_engine, kwargs_of, rand_window, tiny_cfg
from test_gpu_measurement import MODES, _from_xstart
from test_gpu_particles import _cfg, _group_window, _margin, _noise, _randn, _tt, G_, K_, T_
import video_diffusion_amd as vda
from video_diffusion_amd import _lib, inference_util
from video_diffusion_amd.executor import WindowExecutor
from video_diffusion_amd.gaussian_diffusion import (blur_matrix, box_matrix, check_separable_operator, measure, measure_separable,
                                                    resize_matrix, separable_pinv)

pytestmark = pytest.mark.gpu


def _apply(x, L, R, misalign=False):
    """vd_op_linop -> numpy: Z = L x R^T of every trailing plane of x."""
    x = np.asarray(x, np.float32)
    Q, U = x.shape[-2:]
    planes = x.size // (Q * U)
    P, S = L.shape[0], R.shape[0]
    x_d, l_d, r_d = _dev(x, misalign), _dev(np.ascontiguousarray(L)), _dev(np.ascontiguousarray(R))
    out = _dev(np.full(x.shape[:-2] + (P, S), 7.0, np.float32), misalign)
    _lib.check(_lib.lib().vd_op_linop(planes, Q, U, _lib.ptr(x_d), _lib.ptr(l_d), P, _lib.ptr(r_d), S, _lib.ptr(out), _lib.current_stream()))
    return _np(out)


def _project(model, x0, y, lat, A_h, A_w, P_h, P_w, clip=False, misalign=False):
    """vd_op_linear_project on device copies -> the projected x_0 as numpy."""
    x0 = np.asarray(x0, np.float32)
    B, T, _, H, W = x0.shape
    out = _dev(x0, misalign)
    mats = [_dev(np.ascontiguousarray(m)) for m in (A_h, A_w, P_h, P_w)]
    y_d, l_d = _dev(y), _dev(lat).reshape(-1).contiguous()
    _lib.check(_lib.lib().vd_op_linear_project(model._handle, B, T, H, W, _lib.ptr(out), _lib.ptr(y_d), _lib.ptr(l_d), _lib.ptr(mats[0]),
                                               A_h.shape[0], _lib.ptr(mats[1]), A_w.shape[0], _lib.ptr(mats[2]), _lib.ptr(mats[3]),
                                               1 if clip else 0, _lib.current_stream()))
    return _np(out)


def _seed(model, xt, eps, t, clip, y, lat, A_h, A_w, misalign=False):
    """vd_op_linear_dps_seed -> (d_eps, d_x, rho, pred_xstart) as numpy arrays."""
    B, T, _, H, W = xt.shape
    x_d, e_d = _dev(xt, misalign), _dev(eps, misalign)
    t_d = torch.as_tensor(t).long().cuda()
    y_d, l_d = _dev(y, misalign), _dev(lat).reshape(-1).contiguous()
    a_h, a_w = _dev(np.ascontiguousarray(A_h)), _dev(np.ascontiguousarray(A_w))
    outs = [_dev(np.full(xt.shape, 7.0, np.float32), misalign) for _ in range(3)]
    rho = torch.full((B,), 7.0, device="cuda")
    _lib.check(_lib.lib().vd_op_linear_dps_seed(model._handle, B, T, H, W, _lib.ptr(x_d), _lib.ptr(e_d), _lib.ptr(t_d), 1 if clip else 0,
                                                _lib.ptr(y_d), _lib.ptr(l_d), _lib.ptr(a_h), A_h.shape[0], _lib.ptr(a_w), A_w.shape[0],
                                                _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(rho), _lib.ptr(outs[2]), _lib.current_stream()))
    return _np(outs[0]), _np(outs[1]), _np(rho), _np(outs[2])


def _pinvs(A_h, A_w, rtol=1e-3):
    return tuple(separable_pinv(A, rtol)[0].numpy() for A in (A_h, A_w))


def _BT(H):
    return (2, 3) if H <= 72 else (2, 2)


# ---------------------------------------------------------------------------------------------------------------- 1: the operator
@pytest.mark.parametrize("H,W,Mh,Mw", lr.SHAPES)
def test_product_per_element(H, W, Mh, Mw):
    """Forward, adjoint and back-projection: per element inside the restated bound of float64, and the float32 restatement's bits; a
    rerun, an operand 4 bytes off alignment (the scalar load form) and item b alone give the same bits."""
    B, T = _BT(H)
    A_h, A_w = lr.random_operator(H, W, Mh, Mw, seed=H + W + Mh)
    P_h, P_w = _pinvs(A_h, A_w)
    g = np.random.default_rng(H * 7 + Mw)
    x = g.standard_normal((B, T, 3, H, W)).astype(np.float32)
    ym = g.standard_normal((B, T, 3, Mh, Mw)).astype(np.float32)
    for name, (L, R), X in (("forward", lr.forward(A_h, A_w), x), ("adjoint", lr.adjoint(A_h, A_w), ym), ("back", (P_h, P_w), ym)):
        got = _apply(X, L, R)
        want, lim = lr.two_bound(L, X, R)
        r = ratio(got, want, lim)
        same = _same_bits(got, lr.two_f32(L, X, R))
        print(f"{(H, W, Mh, Mw)} {name}: max |d| / bound = {r.max():.3f}; f32 restatement equal: {same}")
        assert got.shape == want.shape and (r <= 1.0).all(), (name, float(r.max()))
        assert same, name
        assert _same_bits(_apply(X, L, R), got) and _same_bits(_apply(X, L, R, misalign=True), got)
        for b in range(B):
            assert _same_bits(_apply(X[b:b + 1], L, R), got[b:b + 1]), (name, b)
    # <A u, v> = <u, A^T v> on the device's own outputs: the two differ by what the per-element bounds allow, summed
    (_, bA), (_, bAt) = lr.two_bound(A_h, x, A_w), lr.two_bound(*lr.adjoint(A_h, A_w)[:1], ym, lr.adjoint(A_h, A_w)[1])
    gA, gAt = _apply(x, A_h, A_w).astype(np.float64), _apply(ym, *lr.adjoint(A_h, A_w)).astype(np.float64)
    gap = abs(float((gA * ym).sum() - (x.astype(np.float64) * gAt).sum()))
    room = float((bA * np.abs(ym)).sum() + (np.abs(x) * bAt).sum())
    assert gap <= room * (1 + 1e-9)


@pytest.mark.parametrize("H,W,Mh,Mw", lr.SHAPES)
def test_selection_and_permutation_move_bits(H, W, Mh, Mw):
    """Rows of the identity select, a permutation matrix permutes: every sum has one term 1 * v among zeros, so the output holds the
    input's bits -- orientation of both factors and of the transposed use, with no bound in sight."""
    g = np.random.default_rng(H + 3 * W)
    x = g.standard_normal((2, 2, 3, H, W)).astype(np.float32)
    rows, cols = np.sort(g.choice(H, Mh, replace=False)), np.sort(g.choice(W, Mw, replace=False))
    S_h, S_w = np.eye(H, dtype=np.float32)[rows], np.eye(W, dtype=np.float32)[cols]
    sel = _apply(x, S_h, S_w)
    assert _same_bits(sel, x[..., rows, :][..., :, cols])
    back = _apply(sel, *lr.adjoint(S_h, S_w))                                     # the adjoint scatters them back, zeros elsewhere
    want = np.zeros_like(x)
    want[np.ix_(range(2), range(2), range(3), rows, cols)] = x[np.ix_(range(2), range(2), range(3), rows, cols)]
    assert _same_bits(back, want)
    ph, pw = g.permutation(H), g.permutation(W)
    assert _same_bits(_apply(x, np.eye(H, dtype=np.float32)[ph], np.eye(W, dtype=np.float32)[pw]), x[..., ph, :][..., :, pw])


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("H,W,Mh,Mw", lr.SHAPES)
def test_project_and_seed_per_element(H, W, Mh, Mw, clip):
    """B = 2, frame 1 not latent.  vd_op_linear_dps_seed: d eps, d_x, rho inside the derived bound and the float32 restatement's bits;
    pred_xstart the sampler pass's bits; the frame that is not latent exactly 0.  vd_op_linear_project on that x_0: per element inside
    the bound, the restatement's bits, A x_0' = y inside the derived bound, the frame that is not latent keeps its bits."""
    model, diff = tiny()
    diff._bind(model)
    tab = tables(diff)
    B, T = _BT(H)
    A_h, A_w = lr.random_operator(H, W, Mh, Mw, seed=100 + H + W + Mh)
    P_h, P_w = _pinvs(A_h, A_w)
    xt, eps, t, y, lat = lr.seed_inputs(tab, B, T, H, W, A_h, A_w, clip, seed=2000 + 10 * H + W + Mh)
    lr.assert_unambiguous(tab, xt, eps, t, y, lat, A_h, A_w, clip)
    de, dx, rho, xs = _seed(model, xt, eps, t, clip, y, lat, A_h, A_w)
    lim = lr.linop_bound(tab, xt, eps, t, y, lat, A_h, A_w, clip)
    f32 = lr.linop_f32(tab, xt, eps, t, y, lat, A_h, A_w, clip)
    for name, got in (("deps", de), ("dxd", dx), ("rho", rho)):
        want, bound = lim[name]
        r = ratio(got, want, bound)
        print(f"{(H, W, Mh, Mw)} clip={clip} {name}: max |d| / bound = {r.max():.3f}; f32 restatement equal: {_same_bits(got, f32[name])}")
        assert got.shape == want.shape and (r <= 1.0).all(), (name, float(r.max()))
    assert _same_bits(de, f32["deps"]) and _same_bits(dx, f32["dxd"])
    assert not de[:, 1].any() and not dx[:, 1].any() and de[:, 0].any() and dx[:, 0].any() and (T < 3 or dx[:, 2].any())
    assert _same_bits(xs, _plain_xstart(model, xt, eps, t, clip)) and _same_bits(xs, f32["x0"])
    if clip:
        beyond = np.abs(f32["x0"]) == 1.0
        assert 0.15 < beyond.mean() < 0.35 and not dx[beyond].any()
    for again in (_seed(model, xt, eps, t, clip, y, lat, A_h, A_w), _seed(model, xt, eps, t, clip, y, lat, A_h, A_w, misalign=True)):
        assert all(_same_bits(a, b) for a, b in zip(again, (de, dx, rho, xs)))
    for b in range(B):
        alone = _seed(model, xt[b:b + 1], eps[b:b + 1], t[b:b + 1], clip, y[b:b + 1], lat[b:b + 1], A_h, A_w)
        assert all(_same_bits(a, v[b:b + 1]) for a, v in zip(alone, (de, dx, rho, xs))), b
    # the projection of an x_0 handed in: the unclamped head's, so that the entry's own clamp has work to do
    x0 = _plain_xstart(model, xt, eps, t, False)
    got = _project(model, x0, y, lat, A_h, A_w, P_h, P_w, clip)
    r = ratio(got, *lr.project_bound(x0, y, lat, A_h, A_w, P_h, P_w, clip))
    same = _same_bits(got, lr.project_f32(x0, y, lat, A_h, A_w, P_h, P_w, clip))
    print(f"{(H, W, Mh, Mw)} clip={clip} project: max |d| / bound = {r.max():.3f}; f32 restatement equal: {same}")
    assert (r <= 1.0).all() and same
    assert _same_bits(got[:, 1], np.clip(x0[:, 1], -1, 1) if clip else x0[:, 1]) and not np.array_equal(got[:, 0], x0[:, 0])
    gap = np.abs(lr.two_fp64(A_h, got, A_w) - y.astype(np.float64))
    room = lr.identity_bound(x0, y, lat, A_h, A_w, P_h, P_w, clip)
    sel = np.broadcast_to(lat.reshape(B, T, 1, 1, 1) == 1, y.shape)
    print(f"  A x0' - y: max {gap[sel].max():.2e}, max / bound {(gap[sel] / room[sel]).max():.3f}")
    assert (gap[sel] <= room[sel]).all()
    assert _same_bits(_project(model, x0, y, lat, A_h, A_w, P_h, P_w, clip, misalign=True), got)
    for b in range(B):
        assert _same_bits(_project(model, x0[b:b + 1], y[b:b + 1], lat[b:b + 1], A_h, A_w, P_h, P_w, clip), got[b:b + 1]), b
    model.check_device_errors()


def test_seed_edges():
    """An item with no latent frame: rho = 0, no gradient, no NaN; an index outside the schedule poisons its item and sets the error bit."""
    model, diff = tiny()
    diff._bind(model)
    tab = tables(diff)
    H, W, Mh, Mw = 12, 8, 5, 3
    A_h, A_w = lr.random_operator(H, W, Mh, Mw, seed=5)
    xt, eps, t, y, lat = lr.seed_inputs(tab, 2, 3, H, W, A_h, A_w, True, seed=77)
    de, dx, rho, xs = _seed(model, xt, eps, t, True, y, lat, A_h, A_w)
    lat0 = lat.copy()
    lat0[0] = 0
    de0, dx0, rho0, xs0 = _seed(model, xt, eps, t, True, y, lat0, A_h, A_w)
    assert rho0[0] == 0 and not de0[0].any() and not dx0[0].any() and np.isfinite(de0).all() and np.isfinite(dx0).all()
    assert _same_bits(de0[1], de[1]) and _same_bits(rho0[1:], rho[1:]) and _same_bits(xs0, xs)
    model.check_device_errors()
    tb = t.copy()
    tb[0] = tab["NT"]
    deb, dxb, rhob, xsb = _seed(model, xt, eps, tb, True, y, lat, A_h, A_w)
    assert np.isnan(deb[0]).all() and np.isnan(dxb[0]).all() and np.isnan(rhob[0]) and np.isnan(xsb[0]).all()
    assert _same_bits(deb[1], de[1]) and _same_bits(dxb[1], dx[1]) and _same_bits(rhob[1:], rho[1:]) and _same_bits(xsb[1], xs[1])
    with pytest.raises(IndexError):
        model.check_device_errors()
    model.check_device_errors()


def test_entry_refusals():
    model, diff = tiny()
    diff._bind(model)
    L, h = _lib.lib(), model._handle
    x, out = torch.zeros(1, 1, 3, 8, 8, device="cuda"), torch.empty(1, 1, 3, 8, 8, device="cuda")
    m = torch.ones(128, 128, device="cuda")
    lat, t = torch.ones(1, device="cuda"), torch.zeros(1, dtype=torch.long, device="cuda")
    op = lambda P, S, o=out, Q=8, U=8: L.vd_op_linop(3, Q, U, _lib.ptr(x), _lib.ptr(m), P, _lib.ptr(m), S, _lib.ptr(o), _lib.current_stream())  # noqa: E731
    for P, S in ((0, 4), (4, 0), (129, 4), (4, 129), (-1, 4)):
        assert op(P, S) != 0 and b"every side in 1 .. 128" in L.vd_last_error()
    assert op(4, 4, Q=0) != 0 and b"every side in 1 .. 128" in L.vd_last_error()
    assert op(4, 4, o=x) != 0 and b"out == x" in L.vd_last_error()
    assert op(4, 4) == 0
    sides = b"1 <= Mh <= H <= 128 and 1 <= Mw <= W <= 128"
    proj = lambda Mh, Mw: L.vd_op_linear_project(h, 1, 1, 8, 8, _lib.ptr(out), _lib.ptr(x), _lib.ptr(lat), _lib.ptr(m), Mh, _lib.ptr(m), Mw,  # noqa: E731
                                                 _lib.ptr(m), _lib.ptr(m), 0, _lib.current_stream())
    seed = lambda Mh, Mw: L.vd_op_linear_dps_seed(h, 1, 1, 8, 8, _lib.ptr(x), _lib.ptr(x), _lib.ptr(t), 1, _lib.ptr(x), _lib.ptr(lat), _lib.ptr(m),  # noqa: E731
                                                  Mh, _lib.ptr(m), Mw, _lib.ptr(out), _lib.ptr(out), None, None, _lib.current_stream())
    for Mh, Mw in ((0, 4), (9, 4), (4, 9), (4, -1)):
        assert proj(Mh, Mw) != 0 and sides in L.vd_last_error()
        assert seed(Mh, Mw) != 0 and sides in L.vd_last_error()
    assert proj(8, 1) == 0 and seed(1, 8) == 0
    # the engine's operator: NULL clears; the rules; what is installed
    mh, mw = _lib._I(0), _lib._I(0)
    assert L.vd_linear_operator(h, mh, mw) == 0 and mh.value == 0 and mw.value == 0
    a = np.ones((8, 32), np.float32)
    p = np.ones((32, 8), np.float32)
    for args, what in (((a, 0, a, 8, None, None), sides), ((a, 33, a, 8, None, None), sides), ((a, 8, a, 8, p, None), b"P_h and P_w come together"),
                       ((np.zeros((8, 32), np.float32), 8, a, 8, None, None), b"must not be all zero"),
                       ((a, 8, np.full((8, 32), np.inf, np.float32), 8, None, None), b"must be finite"),
                       ((a, 8, a, 8, np.full((32, 8), np.nan, np.float32), p), b"must be finite")):
        ptrs = [_lib.ptr(v) if isinstance(v, np.ndarray) else v for v in args]
        assert L.vd_set_linear_operator(h, *ptrs) != 0 and what in L.vd_last_error(), what
    yd = torch.zeros(2, 6, 3, 8, 8, device="cuda")
    assert L.vd_set_linear_measurement(h, _lib.ptr(yd)) != 0 and b"no operator is installed" in L.vd_last_error()
    assert L.vd_set_particle_linear(h, 1) != 0 and b"no operator is installed" in L.vd_last_error()
    _lib.check(L.vd_set_linear_operator(h, _lib.ptr(a), 8, _lib.ptr(a), 8, None, None))
    assert L.vd_linear_operator(h, mh, mw) == 1 and (mh.value, mw.value) == (8, 8)
    assert L.vd_set_linear_measurement(h, _lib.ptr(yd)) != 0 and b"has no back-projection" in L.vd_last_error()
    _lib.check(L.vd_set_linear_operator(h, _lib.ptr(a), 8, _lib.ptr(a), 8, _lib.ptr(p), _lib.ptr(p)))
    assert L.vd_linear_operator(h, mh, mw) == 2
    _lib.check(L.vd_set_linear_measurement(h, _lib.ptr(yd)))
    assert L.vd_linear_measurement(h) == 1
    assert L.vd_set_linear_operator(h, None, 0, None, 0, None, None) != 0 and b"clear that first" in L.vd_last_error()
    a4 = np.ones((4, 32), np.float32)
    assert L.vd_set_linear_operator(h, _lib.ptr(a4), 4, _lib.ptr(a), 8, _lib.ptr(p), _lib.ptr(p)) != 0 and b"keep its shape" in L.vd_last_error()
    assert L.vd_set_measurement(h, _lib.ptr(yd), 4, 0) == 0                       # the cell-mean measurement beside it: the step refuses
    c = _rand_window(2, 6, 32, 2, seed=1)
    kw, xw = _window_kw(c), c["x"].cuda()
    with pytest.raises(_lib.VdError, match=r"a linear measurement \(vd_set_linear_measurement\) together with a measurement \(vd_set_measurement\)"):
        diff._fused_step(0, model, xw, _t(2, 3), True, kw, noise=torch.zeros_like(xw))
    _lib.check(L.vd_set_measurement(h, None, 1, 0))
    _lib.check(L.vd_set_linear_measurement(h, None))
    _lib.check(L.vd_set_particle_linear(h, 1))
    assert L.vd_particle_linear(h) == 1 and L.vd_set_linear_operator(h, None, 0, None, 0, None, None) != 0 and b"switch that off first" in L.vd_last_error()
    taps = np.ones((3, 3), np.float32)
    _lib.check(L.vd_set_blur_kernel(h, _lib.ptr(taps), 3))
    assert L.vd_set_particle_blur(h, 1) != 0 and b"vd_set_particle_blur together with vd_set_particle_linear is not served" in L.vd_last_error()
    _lib.check(L.vd_set_particle_linear(h, 0))
    _lib.check(L.vd_set_particle_blur(h, 1))
    assert L.vd_set_particle_linear(h, 1) != 0 and b"vd_set_particle_linear together with vd_set_particle_blur is not served" in L.vd_last_error()
    _lib.check(L.vd_set_particle_blur(h, 0))
    _lib.check(L.vd_set_blur_kernel(h, None, 0))
    _lib.check(L.vd_set_linear_operator(h, None, 0, None, 0, None, None))
    assert L.vd_linear_operator(h, mh, mw) == 0 and L.vd_particle_linear(h) == 0 and L.vd_linear_measurement(h) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 2: the projected step
def _step_operators():
    """Bicubic x4, and a stride-2 reflect-padded 9-tap sigma = 2 Gaussian: (name, A_h, A_w) for the tiny model's 32 x 32 planes."""
    ax = torch.arange(9, dtype=torch.float64) - 4
    g = torch.exp(-(ax * ax) / 8.0)
    return [("bicubic4", resize_matrix(32, 8), resize_matrix(32, 8)),
            ("gauss9s2", blur_matrix(32, g / g.sum(), stride=2, padding="reflect"), blur_matrix(32, g / g.sum(), stride=2, padding="reflect"))]


def _window_y(c, A_h, A_w, seed):
    g = torch.Generator().manual_seed(seed)
    return measure_separable(torch.rand(tuple(c["x"].shape), generator=g) * 2 - 1, A_h, A_w).cuda()


@pytest.mark.parametrize("op", [0, 1], ids=["bicubic4", "gauss9s2"])
@pytest.mark.parametrize("sampler,eta", [("p_sample", 0.0), ("ddim", 0.5), ("dpmpp_2m", 0.0)])
def test_the_projected_step(sampler, eta, op):
    """B = 2, 2 observed of 6 frames: pred_xstart inside the scope is the plain step's x_0 projected -- vd_op_linear_project's bits, the
    restatement's bits, inside its bound -- the sample is the sampler pass on it with clip off, A pred_xstart = y on the latent frames
    inside the derived bound, p_mean_variance agrees, and the plain step behind the scope keeps its bits."""
    model, diff = tiny()
    N = diff.num_timesteps
    name, A_h, A_w = _step_operators()[op]
    a_h, a_w = (a.numpy() for a in check_separable_operator(A_h, A_w))
    c = _rand_window(2, 6, 32, 2, seed=70)
    kw, x = _window_kw(c), c["x"].cuda()
    lat = _np(kw["latent_mask"]).reshape(2, 6)
    y = _window_y(c, A_h, A_w, seed=71)
    noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(72)).cuda()
    prev = (torch.rand(x.shape, generator=torch.Generator().manual_seed(73)) * 2 - 1).cuda() if sampler == "dpmpp_2m" else None
    mode = MODES[sampler]
    L = _lib.lib()
    for tv in (N - 1, 3, 0):
        tt = _t(2, tv)
        plain, plain_x0 = diff._fused_step(mode, model, x, tt, True, kw, eta=eta, noise=noise, prev_xstart=prev)
        with diff.linear_measurement_scope(model, y, A_h, A_w) as scope:
            assert L.vd_linear_measurement(model._handle) == 1 and L.vd_linear_operator(model._handle, None, None) == 2
            got, got_x0 = diff._fused_step(mode, model, x, tt, True, kw, eta=eta, noise=noise, prev_xstart=prev)
            pmv = diff.p_mean_variance(model, x, tt, clip_denoised=True, model_kwargs=kw)
        assert L.vd_linear_measurement(model._handle) == 0 and L.vd_linear_operator(model._handle, None, None) == 0
        p_h, p_w = _pinvs(a_h, a_w)
        assert scope.rank_h == np.linalg.matrix_rank(a_h.astype(np.float64), tol=1e-3 * np.linalg.norm(a_h.astype(np.float64), 2))
        x0n, yn = _np(plain_x0), _np(y)
        want_x0 = _project(model, x0n, yn, lat, a_h, a_w, p_h, p_w)
        assert _same_bits(got_x0, want_x0) and not torch.equal(got_x0, plain_x0)
        assert torch.equal(got_x0[:, :2], plain_x0[:, :2])                                          # observed frames: unprojected
        assert _same_bits(want_x0, lr.project_f32(x0n, yn, lat, a_h, a_w, p_h, p_w))
        r = ratio(_np(got_x0), *lr.project_bound(x0n, yn, lat, a_h, a_w, p_h, p_w))
        gap = np.abs(lr.two_fp64(a_h, _np(got_x0), a_w) - yn.astype(np.float64))[:, 2:]
        room = lr.identity_bound(x0n, yn, lat, a_h, a_w, p_h, p_w)[:, 2:]
        print(f"{name} {sampler} t={tv}: rank {scope.rank_h}; x0' max |d| / bound = {r.max():.3f}; A x0' - y: max {gap.max():.2e}, max / bound {(gap / room).max():.3f}")
        assert (r <= 1.0).all() and (gap <= room).all()
        want, want_xs = _from_xstart(model, mode, x, got_x0, tt, eta, noise, prev)
        assert torch.equal(got, want) and torch.equal(want_xs, got_x0), float((got - want).abs().max())
        assert torch.equal(pmv["pred_xstart"], got_x0)
        assert torch.equal(pmv["mean"], _from_xstart(model, 0, x, got_x0, tt, 0.0, None, None, want_mean=True))
        if tv == 0:
            assert torch.equal(got, got_x0)
        again, again_x0 = diff._fused_step(mode, model, x, tt, True, kw, eta=eta, noise=noise, prev_xstart=prev)
        assert torch.equal(again, plain) and torch.equal(again_x0, plain_x0)
    model.check_device_errors()


def test_back_override_and_guidance():
    """back=(P_h, P_w) is used as given; under cfg_scale = 2 with dynamic thresholding the projection acts on the thresholded x_0."""
    model, diff = tiny()
    N = diff.num_timesteps
    _, A_h, A_w = _step_operators()[0]
    a_h, a_w = (a.numpy() for a in check_separable_operator(A_h, A_w))
    c = _rand_window(2, 6, 32, 2, seed=74)
    kw, x = _window_kw(c), c["x"].cuda()
    lat = _np(kw["latent_mask"]).reshape(2, 6)
    y = _window_y(c, A_h, A_w, seed=75)
    noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(76)).cuda()
    p_h, p_w = (0.5 * np.ascontiguousarray(a.T) for a in (a_h, a_w))              # not a pseudo-inverse at all: taken as given
    tt = _t(2, 3)
    _, plain_x0 = diff._fused_step(0, model, x, tt, True, kw, noise=noise)
    with diff.linear_measurement_scope(model, y, A_h, A_w, back=(p_h, p_w)) as scope:
        _, got_x0 = diff._fused_step(0, model, x, tt, True, kw, noise=noise)
    assert scope.rank_h is None and scope.rank_w is None
    assert _same_bits(got_x0, _project(model, _np(plain_x0), _np(y), lat, a_h, a_w, p_h, p_w))
    p_h, p_w = _pinvs(a_h, a_w)
    for mode, tv in ((0, N - 2), (1, 2), (3, 0)):
        tt = _t(2, tv)
        with diff.guidance_scope(model, dynamic_threshold=0.9):
            _, thr_x0 = diff._fused_step(mode, model, x, tt, True, kw, noise=noise, cfg_scale=2.0)
            with diff.linear_measurement_scope(model, y, A_h, A_w):
                got, got_x0 = diff._fused_step(mode, model, x, tt, True, kw, noise=noise, cfg_scale=2.0)
        assert _same_bits(got_x0, _project(model, _np(thr_x0), _np(y), lat, a_h, a_w, p_h, p_w))
        want, _ = _from_xstart(model, mode, x, got_x0, tt, 0.0, noise, None)
        assert torch.equal(got, want)
    model.check_device_errors()


def test_box_matrix_against_measurement_scope():
    """box_matrix(32, 4) through the new scope and measurement_scope(sr4) restate the same float64 projection, each inside its own bound:
    this file's for the two-sided product, measurement_restated's for the cell mean."""
    from measurement_restated import project_bound as cell_bound
    model, diff = tiny()
    A = box_matrix(32, 4)
    a = check_separable_operator(A, A)[0].numpy()
    P = separable_pinv(A)[0].numpy()
    assert np.array_equal(P, np.where(a > 0, np.float32(1), np.float32(0)).T)     # the pseudo-inverse of the cell mean replicates
    c = _rand_window(2, 6, 32, 2, seed=78)
    kw, x = _window_kw(c), c["x"].cuda()
    lat = _np(kw["latent_mask"]).reshape(2, 6)
    truth = torch.rand(tuple(x.shape), generator=torch.Generator().manual_seed(79)) * 2 - 1
    y = measure(truth, 4).cuda()
    noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(80)).cuda()
    tt = _t(2, 3)
    _, plain_x0 = diff._fused_step(0, model, x, tt, True, kw, noise=noise)
    with diff.linear_measurement_scope(model, y, A, A):
        _, lin_x0 = diff._fused_step(0, model, x, tt, True, kw, noise=noise)
    with diff.measurement_scope(model, y, 4):
        _, cell_x0 = diff._fused_step(0, model, x, tt, True, kw, noise=noise)
    x0n, yn = _np(plain_x0), _np(y)
    want_cell, lim_cell = cell_bound(x0n, yn, lat, 4, False)
    want_lin, lim_lin = lr.project_bound(x0n, yn, lat, a, a, P, P)
    assert np.abs(want_cell - want_lin).max() <= 1e-13                           # one float64 value
    r_lin, r_cell = ratio(_np(lin_x0), want_lin, lim_lin), ratio(_np(cell_x0), want_cell, lim_cell)
    print(f"box 4: linear max |d| / bound = {r_lin.max():.3f}, cell mean max |d| / bound = {r_cell.max():.3f}")
    assert (r_lin <= 1.0).all() and (r_cell <= 1.0).all()
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 3: linear_dps_scope
def _oracle_grad(ora, c, t, y, A_h, A_w):
    """The residual norm composed in torch on the oracle's network -> (grad of sum_b rho_b w.r.t. x_t, rho)."""
    sch = ora.s
    kwo = dict(x0=c["x0"], obs_mask=c["obs_mask"], latent_mask=c["latent_mask"], kinda_marg_mask=c["kinda_marg_mask"],
               frame_indices=c["frame_indices"], x_t_minus_1=c["x0"])
    x = c["x"].detach().clone().requires_grad_(True)
    tm = torch.tensor(sch.timestep_map, dtype=t.dtype)[t]
    coef = lambda tabl: torch.from_numpy(np.asarray(tabl))[t].float().view(-1, 1, 1, 1, 1)      # noqa: E731
    with torch.enable_grad():
        eps = ora.net.with_grad(x, tm, **kwo)
        x0 = (coef(sch.sqrt_recip_alphas_cumprod) * x - coef(sch.sqrt_recipm1_alphas_cumprod) * eps).clamp(-1, 1)
        r = (y - A_h @ x0 @ A_w.T) * c["latent_mask"]
        rho = r.reshape(r.shape[0], -1).pow(2).sum(dim=1).sqrt()
        g, = torch.autograd.grad(rho.sum(), x)
    return g, rho.detach()


def _dps_call(diff, model, mode, x, tt, kw, eta, noise, y, A_h, A_w, zeta):
    with diff.linear_dps_scope(model, y, A_h, A_w, zeta=zeta):
        diff._step(mode, model, x, tt, True, None, kw, eta, noise)
    return diff._last_dps


@pytest.mark.parametrize("case", [("bicubic4", 0, 0.0, "plain"), ("gauss9s2", 1, 0.5, "plain"), ("bicubic4", 0, 0.0, "marg_and_padding")],
                         ids=lambda c: f"{c[0]}-mode{c[1]}-{c[3]}")
def test_step_gradient_vs_oracle_autograd(case):
    """The bars are test_gpu_blur.py::test_step_gradient_vs_oracle_autograd's own: the same backward pass against the same oracle."""
    kind, mode, eta, masks = case
    cfg = {**vda.video_model_and_diffusion_defaults(), **ORACLE_CFG}
    model, diff, ora = _oracle(cfg)
    c = _rand_window(2, 5, 32, 2, seed=725)
    if masks == "marg_and_padding":
        c["latent_mask"][:, 2] = 0
        c["kinda_marg_mask"][:, 2] = 1
        c["latent_mask"][:, 4] = 0
    _, A_h, A_w = _step_operators()[0 if kind == "bicubic4" else 1]
    a_h, a_w = check_separable_operator(A_h, A_w)
    g = torch.Generator().manual_seed(31)
    y = measure_separable(torch.rand(c["x"].shape, generator=g) * 2 - 1, a_h, a_w)
    y = y + 0.1 * torch.randn(y.shape, generator=g)
    noise = torch.randn(c["x"].shape, generator=g)
    t = torch.tensor([30, 30])
    want, want_rho = _oracle_grad(ora, c, t, y, a_h, a_w)
    kw = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in c.items() if k != "x"}
    kw.update(x_t_minus_1=kw["x0"], observed_frames="x_0")
    out = _dps_call(diff, model, mode, c["x"].cuda(), t.cuda(), kw, eta, noise, y, A_h, A_w, 0.5)
    scale = float(want.abs().max())
    err = (out["grad"].cpu() - want).abs()
    print(f"{case}: max |grad - ref| = {float(err.max()):.3e} = {float(err.max()) / scale:.3e} max |ref|; rho {out['residual_norm'].tolist()} ref {want_rho.tolist()}")
    assert scale > 0 and not out["grad"][:, :2].any()
    if masks == "marg_and_padding":
        assert want[:, 4].abs().max() > 0
    close(out["grad"].cpu(), want, atol=2e-4 * scale, rtol=1e-3)
    lat = _np(c["latent_mask"]).reshape(2, 5)
    x0 = _np(out["pred_xstart"]).astype(np.float64)
    rho, lim = lr.seed_bound(x0, np.zeros_like(x0), _np(y.float()), lat, a_h.numpy(), a_w.numpy())["rho"]
    r = ratio(_np(out["residual_norm"]), rho, lim)
    print(f"  residual_norm: max |d| / bound = {r.max():.3f}")
    assert (r <= 1.0).all() and (rho > 1e-3).all()
    model.check_device_errors()


@pytest.mark.parametrize("mode,eta", [(0, 0.0), (1, 0.5)])
def test_dps_step_identities_bit_for_bit(mode, eta):
    model, diff = tiny()
    N = diff.num_timesteps
    c = _rand_window(2, 6, 32, 2, seed=170)
    kw, x = _window_kw(c), c["x"].cuda()
    lat = _np(kw["latent_mask"]).reshape(2, 6) == 1
    _, A_h, A_w = _step_operators()[1]
    g = torch.Generator().manual_seed(171)
    y = measure_separable(torch.rand(tuple(x.shape), generator=g) * 2 - 1, A_h, A_w).float()
    y = y + 0.1 * torch.randn(y.shape, generator=g)
    noise = torch.randn(x.shape, generator=g).cuda()
    zeta = 0.75
    for tv in (N - 1, 3, 0):
        tt = _t(2, tv)
        plain, plain_x0 = diff._fused_step(mode, model, x, tt, True, kw, eta=eta, noise=noise)
        out = _dps_call(diff, model, mode, x, tt, kw, eta, noise, y, A_h, A_w, zeta)
        got, grad = _np(out["sample"]), _np(out["grad"])
        assert torch.equal(out["pred_xstart"], plain_x0)
        assert _same_bits(got[~lat], _np(plain)[~lat])
        assert _same_bits(got[lat], _fma32(np.float32(-zeta), grad[lat], _np(plain)[lat]))
        assert not grad[:, :2].any() and np.abs(grad[lat]).max() > 0 and not np.array_equal(got[lat], _np(plain)[lat])
        zero = _dps_call(diff, model, mode, x, tt, kw, eta, noise, y, A_h, A_w, 0.0)
        assert torch.equal(zero["sample"], plain) and torch.equal(zero["pred_xstart"], plain_x0)     # zeta = 0: the plain step entirely
        assert torch.equal(zero["grad"], out["grad"]) and torch.equal(zero["residual_norm"], out["residual_norm"])
        again, again_x0 = diff._fused_step(mode, model, x, tt, True, kw, eta=eta, noise=noise)
        assert torch.equal(again, plain) and torch.equal(again_x0, plain_x0)     # a plain step behind a guided one: its usual bits
    L, mh, mw = _lib.lib(), _lib._I(0), _lib._I(0)
    with diff.linear_dps_scope(model, y, A_h, A_w, zeta=zeta):
        assert L.vd_linear_operator(model._handle, mh, mw) == 1 and (mh.value, mw.value) == (16, 16)
        with diff.linear_dps_scope(model, y[..., :8, :8], resize_matrix(32, 8), resize_matrix(32, 8), zeta=0.1):      # scopes nest and restore
            assert L.vd_linear_operator(model._handle, mh, mw) == 1 and (mh.value, mw.value) == (8, 8)
        assert L.vd_linear_operator(model._handle, mh, mw) == 1 and (mh.value, mw.value) == (16, 16)
        torch.manual_seed(9)
        o = (diff.p_sample(model, x, _t(2, 3), model_kwargs=kw) if mode == 0 else diff.ddim_sample(model, x, _t(2, 3), model_kwargs=kw, eta=eta))
    assert L.vd_linear_operator(model._handle, mh, mw) == 0
    torch.manual_seed(9)
    n1 = torch.randn_like(x)
    want = _dps_call(diff, model, mode, x, _t(2, 3), kw, eta, n1, y, A_h, A_w, zeta)
    assert torch.equal(o["sample"], want["sample"]) and torch.equal(o["grad"], want["grad"]) and o["residual_norm"].shape == (2,)
    assert "grad" not in diff.p_sample(model, x, _t(2, 3), model_kwargs=kw)
    model.check_device_errors()


def test_dps_loop_is_the_chain_of_steps():
    model, diff = tiny(timestep_respacing="logsnr3")
    c = _rand_window(2, 6, 32, 2, seed=180)
    kw, x = _window_kw(c), c["x"].cuda()
    _, A_h, A_w = _step_operators()[0]
    y = _window_y(c, A_h, A_w, seed=181)
    with diff.linear_dps_scope(model, y, A_h, A_w, zeta=0.4):
        torch.manual_seed(11)
        got, _ = diff.p_sample_loop(model, tuple(x.shape), noise=x, model_kwargs=dict(kw))
        torch.manual_seed(11)
        noises = [torch.randn_like(x) for _ in range(3)]
        img = x
        for k, tv in enumerate((2, 1, 0)):
            img, _ = diff._step(0, model, img, _t(2, tv), True, None, kw, 0.0, noises[k])
    assert torch.equal(got, img) and torch.isfinite(got).all()
    with diff.linear_dps_scope(model, y, A_h, A_w, zeta=0.4):
        torch.manual_seed(11)
        d = diff.ddim_sample_loop(model, tuple(x.shape), noise=x, model_kwargs=dict(kw), eta=0.5)
        img = x
        for k, tv in enumerate((2, 1, 0)):
            img, _ = diff._step(1, model, img, _t(2, tv), True, None, kw, 0.5, noises[k])
    assert torch.equal(d, img)
    model.check_device_errors()


def test_window_of_32_frames_runs_and_33_is_refused():
    model, diff = long_engine(tiny_cfg(40, num_channels=64, timestep_respacing="ddim50"))
    A = resize_matrix(32, 8)
    for T, n_obs in ((32, 8), (33, 8)):
        c = rand_window(1, T, 32, n_obs, seed=41)
        kw = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in c.items() if k != "x"}
        kw.update(x_t_minus_1=kw["x0"], observed_frames="x_0")
        x = c["x"].cuda()
        y = measure_separable(torch.rand(tuple(x.shape), generator=torch.Generator().manual_seed(42)) * 2 - 1, A, A)
        with diff.linear_dps_scope(model, y, A, A, zeta=0.5):
            if T == 33:
                with pytest.raises(_lib.VdError, match=r"linear_dps: windows of at most 32 frames.*got 33"):
                    diff.p_sample(model, x, _t(1, 30), model_kwargs=kw)
                continue
            torch.manual_seed(1)
            o = diff.p_sample(model, x, _t(1, 30), model_kwargs=kw)
        assert torch.isfinite(o["sample"]).all() and torch.isfinite(o["grad"]).all() and float(o["residual_norm"][0]) > 0
        assert not o["grad"][:, :n_obs].any() and o["grad"][:, n_obs:].abs().max() > 0
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 4: the window graph
@pytest.mark.parametrize("sampler,eta", [("p_sample", 0.0), ("dpmpp_2m", 0.0)])
def test_projection_window_graph(sampler, eta):
    """begin(measurement=, operator=), run(): to the bit the eager chain of steps inside the scope (dpmpp_2m, which draws no noise); a
    begin() inside the scope arms the same graph; other matrices of equal shape need no new capture and
    change the result; a window without a measurement on the same executor is the plain window."""
    model, diff = tiny(timestep_respacing="logsnr3")
    diff._bind(model)
    L = _lib.lib()
    (_, A_h, A_w), (_, B_h, B_w) = _step_operators()[0], ("bilinear4", resize_matrix(32, 8, "bilinear"), resize_matrix(32, 8, "bilinear"))
    c = _rand_window(2, 6, 32, 2, seed=90)
    kw, x = _window_kw(c, "x_t_minus_1"), c["x"].cuda()
    y = _window_y(c, A_h, A_w, seed=91)
    wex = WindowExecutor(model, diff)
    kwargs = dict(seed=5, sampler=sampler, eta=eta, renoise=False)
    plain = wex.begin(x, kw, **kwargs).run().clone()
    n0 = L.vd_window_graphs(model._handle)
    got = wex.begin(x, kw, measurement=y, operator=(A_h, A_w), **kwargs).run().clone()
    n1 = L.vd_window_graphs(model._handle)
    assert n1 == n0 + 1 and not torch.equal(got, plain)
    assert L.vd_linear_measurement(model._handle) == 0
    with diff.linear_measurement_scope(model, y, A_h, A_w):
        again = wex.begin(x, kw, **kwargs).run().clone()
    assert torch.equal(again, got) and L.vd_window_graphs(model._handle) == n1
    # eager: the chain of steps inside the scope on the same draws (dpmpp_2m draws none)
    if sampler == "dpmpp_2m":
        with diff.linear_measurement_scope(model, y, A_h, A_w):
            img, prev = x, None
            for tv in (2, 1, 0):
                o = diff.dpmpp_2m_sample(model, img, _t(2, tv), prev_xstart=prev, model_kwargs=kw)
                img, prev = o["sample"], o["pred_xstart"]
        assert torch.equal(img, got)
    other = wex.begin(x, kw, measurement=y, operator=(B_h, B_w), **kwargs).run().clone()
    assert L.vd_window_graphs(model._handle) == n1 and not torch.equal(other, got)
    assert torch.equal(wex.begin(x, kw, **kwargs).run(), plain)
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 5: steering
def _lin_measurement(truth, K, A_h, A_w, sigma, seed):
    y = measure_separable(truth, A_h, A_w)
    y = y + sigma * torch.randn(y.shape, generator=torch.Generator().manual_seed(seed))
    return y.repeat_interleave(K, dim=0).cuda()


def _torch_reward(y, A_h, A_w, lat, sigma):
    """reward_fn: r = -||y - A x0||^2 / (2 sigma^2) over the latent frames, in float64 through measure_separable in torch."""
    a_h, a_w = (a.double() for a in check_separable_operator(A_h, A_w))

    def fn(x0, tt):
        r = (y.double().cpu() - a_h @ x0.double().cpu() @ a_w.T) * lat.double().cpu().view(x0.shape[0], -1, 1, 1, 1)
        return (-(r * r).flatten(1).sum(1) / (2.0 * sigma * sigma)).to(x0.device)
    return fn


def test_builtin_reward_against_reward_fn():
    """test_gpu_blur.py::test_builtin_blur_reward_against_reward_fn on this operator: under ess_threshold 0 the log-weights against the
    reward_fn's inside the bar derived from the residual norm's bound; under ess_threshold 1 the same ancestors, samples and x_0 to the bit."""
    model, diff = long_engine(_cfg())
    c, truth = _group_window(G_, K_, T_, 43)
    B, sigma, lam = G_ * K_, 1.5, 1.0
    S = truth.shape[-1]
    A_h, A_w = resize_matrix(S, S // 4), resize_matrix(S, S // 4)
    a_h, a_w = (a.numpy() for a in check_separable_operator(A_h, A_w))
    y = _lin_measurement(truth, K_, A_h, A_w, 0.1, 7)
    kw, x = kwargs_of(c), c["x"].cuda()
    fn = _torch_reward(y, A_h, A_w, kw["latent_mask"], sigma)
    for t in (6, 0):
        noise = _noise(x.shape, 50 + t)
        plain = diff._step(0, model, x, _tt(B, t), True, None, kw, 0.0, noise)
        u = torch.tensor([[0.37, 0.61], [0.83, 0.12]], dtype=torch.float64)
        got = {}
        for tau in (0.0, 1.0):
            with diff.steering_scope(model, particles=K_, scale=lam, ess_threshold=tau, measurement=y, operator=(A_h, A_w), sigma_y=sigma, uniforms=lambda _t: u):
                assert _lib.lib().vd_particle_linear(model._handle) == 1
                sb, xb = diff._step(0, model, x, _tt(B, t), True, None, kw, 0.0, noise)
                a = diff._last_steer
            with diff.steering_scope(model, fn, particles=K_, scale=lam, ess_threshold=tau, uniforms=lambda _t: u):
                sf, xf = diff._step(0, model, x, _tt(B, t), True, None, kw, 0.0, noise)
                f = diff._last_steer
            got[tau] = (a, f)
            assert torch.equal(a["ancestors"], f["ancestors"]) and torch.equal(sb, sf) and torch.equal(xb, xf), (t, tau)
            anc = a["ancestors"].long()
            assert torch.equal(sb, plain[0][anc]) and torch.equal(xb, plain[1][anc])
        a, f = got[0.0]
        x0n = _np(plain[0] if t == 0 else plain[1]).astype(np.float64)
        latn = _np(kw["latent_mask"]).reshape(B, -1)
        rho, d = lr.seed_bound(x0n, np.zeros_like(x0n), _np(y).astype(np.float64), latn, a_h, a_w)["rho"]
        bar = lam * (2 * rho * d + d * d) / (2 * sigma ** 2)
        lb, lf = a["log_weights"].cpu().numpy(), f["log_weights"].cpu().numpy()
        assert np.allclose(lf, -lam * rho ** 2 / (2 * sigma ** 2), rtol=1e-12)
        print(f"t={t}: log-weights {lb}, max |d| / bar = {(np.abs(lb - lf) / bar).max():.3f}, bar {bar.max():.3e}")
        assert (np.abs(lb - lf) <= bar).all() and np.ptp(lb[:K_]) > 0
        assert torch.equal(a["ancestors"].cpu(), torch.arange(B, dtype=torch.int32))
        st = pr.new_state(G_, K_)
        want = pr.particle_weights(st, (lf / lam).reshape(G_, K_), lam, 1.0, u.numpy(), np.full(G_, t == 0))
        assert _margin(want, u.numpy(), np.full(G_, t == 0)) > 4 * bar.max()
        assert np.array_equal(got[1.0][0]["ancestors"].cpu().numpy(), want["ancestors"])
    L = _lib.lib()
    assert L.vd_particles(model._handle) == 0 and L.vd_particle_linear(model._handle) == 0 and L.vd_linear_operator(model._handle, None, None) == 0
    model.check_device_errors()


def _graph_window(wex, c, y, op, sampler, eta, seed, sigma, tau, steps):
    wex.begin(c["x"].cuda(), kwargs_of(c), seed=seed, sampler=sampler, eta=eta, particles=K_, particle_measurement=y, operator=op,
              sigma_y=sigma, ess_threshold=tau)
    trace = []
    for _ in range(steps):
        x = wex.run(1).clone()
        trace.append((x, wex.particle_state()["ancestors"].clone()))
    return trace, wex.particle_state()


def _eager_window(model, diff, c, y, op, sampler, eta, seed, sigma, tau, steps):
    """test_gpu_blur._eager_window with this operator: eager steps that repeat the graph's draws."""
    kw, x = kwargs_of(c), c["x"].cuda()
    B, n = x.shape[0], x.numel()
    trace, prev, out = [], None, None
    NT = diff.num_timesteps
    with diff.steering_scope(model, particles=K_, ess_threshold=tau, measurement=y, operator=op, sigma_y=sigma,
                             uniforms=None if sampler == "dpmpp_2m_sde" else (lambda tt: (seed, (NT - 1 - int(tt[0])) * n))):
        for k in range(steps):
            t = _tt(B, NT - 1 - k)
            if sampler == "dpmpp_2m_sde":
                out = diff._dpmpp_2m_sde(model, x, t, prev, True, None, kw, philox=(seed, k * n))
                prev = out["pred_xstart"]
            else:
                sample, _ = diff._step(0 if sampler == "p_sample" else 1, model, x, t, True, None, kw, eta, _randn(n, seed, k * n).view(x.shape))
                out = dict(diff._last_steer, sample=sample)
            x = out["sample"]
            trace.append((x, out["ancestors"].cpu()))
    return trace, out


def _same_windows(eager, last, graph, state):
    for k, ((xe, ae), (xg, ag)) in enumerate(zip(eager, graph)):
        assert torch.equal(xe, xg) and torch.equal(ae, ag), k
    assert torch.equal(last["chosen"].cpu(), state["chosen"]) and torch.equal(last["log_weights"].cpu(), state["log_weights"])


def test_steering_graph_against_eager_and_matrices_changed_between_windows():
    model, diff = long_engine(_cfg(respacing="ddim5"))
    c, truth = _group_window(G_, K_, T_, 81)
    S = truth.shape[-1]
    op1, op2 = (resize_matrix(S, S // 4),) * 2, (resize_matrix(S, S // 4, "bilinear"),) * 2
    y = _lin_measurement(truth, K_, *op1, 0.1, 8)
    L = _lib.lib()
    wex = WindowExecutor(model, diff)
    steps = diff.num_timesteps
    graph1, state1 = _graph_window(wex, c, y, op1, "dpmpp_2m_sde", 0.0, 1234567, 1.5, 0.9, steps)
    n_graphs = L.vd_window_graphs(model._handle)
    eager1, last1 = _eager_window(model, diff, c, y, op1, "dpmpp_2m_sde", 0.0, 1234567, 1.5, 0.9, steps)
    _same_windows(eager1, last1, graph1, state1)
    graph2, state2 = _graph_window(wex, c, y, op2, "dpmpp_2m_sde", 0.0, 1234567, 1.5, 0.9, steps)
    assert L.vd_window_graphs(model._handle) == n_graphs                       # equal shape: the same graph, replayed on the new matrices
    eager2, last2 = _eager_window(model, diff, c, y, op2, "dpmpp_2m_sde", 0.0, 1234567, 1.5, 0.9, steps)
    _same_windows(eager2, last2, graph2, state2)
    assert not torch.equal(state2["log_weights"], state1["log_weights"])
    op3 = (resize_matrix(S, S // 8),) * 2                                       # (a smaller y: no engine buffer grows, which would drop the graphs)
    _graph_window(wex, c, _lin_measurement(truth, K_, *op3, 0.1, 8), op3, "dpmpp_2m_sde", 0.0, 1234567, 1.5, 0.9, 1)
    assert L.vd_window_graphs(model._handle) == n_graphs + 1                   # another shape: another graph
    assert L.vd_particles(model._handle) == 0 and L.vd_particle_linear(model._handle) == 0
    model.check_device_errors()


def test_window_of_40_frames_runs():
    """Beyond the gradient scope's 32 frames: linear_dps_scope refuses by name, the projection and the steered step and window graph run."""
    model, diff = long_engine(_cfg(40, respacing="ddim5"))
    c, truth = _group_window(1, K_, 40, 91, n_obs=3)
    S = truth.shape[-1]
    op = (resize_matrix(S, S // 4),) * 2
    y = _lin_measurement(truth, K_, *op, 0.1, 9)
    kw, x, B = kwargs_of(c), c["x"].cuda(), K_
    with pytest.raises(_lib.VdError, match="linear_dps: windows of at most 32 frames"):
        with diff.linear_dps_scope(model, y, *op, zeta=0.5):
            diff.p_sample(model, x, _tt(B, 4), model_kwargs=kw)
    with diff.linear_measurement_scope(model, y, *op):
        sample, xstart = diff._step(0, model, x, _tt(B, 0), True, None, kw, 0.0, _noise(x.shape, 92))
    a = check_separable_operator(*op)[0].numpy()
    gap = np.abs(lr.two_fp64(a, _np(xstart), a) - _np(y).astype(np.float64))[:, 3:]
    # a ceiling from the formats, not the derived bound (test_the_projected_step holds that): three nested sums of at most 32 terms in
    # fp32, gamma_96 = 5.8e-6, on |A| |P| |A| |x| <= 1.5^2 1.31^2 1.5^2 3 < 17
    assert torch.isfinite(sample).all() and gap.max() <= 1e-4
    plain = diff._step(0, model, x, _tt(B, 4), True, None, kw, 0.0, _noise(x.shape, 92))
    with diff.steering_scope(model, particles=K_, ess_threshold=1.0, measurement=y, operator=op, sigma_y=1.0):
        sample, xstart = diff._step(0, model, x, _tt(B, 4), True, None, kw, 0.0, _noise(x.shape, 92))
        st = diff._last_steer
    anc = st["ancestors"].long()
    assert torch.isfinite(sample).all() and torch.equal(sample, plain[0][anc]) and torch.equal(xstart, plain[1][anc])
    trace, state = _graph_window(WindowExecutor(model, diff), c, y, op, "p_sample", 0.0, 77, 1.0, 1.0, diff.num_timesteps)
    assert torch.isfinite(trace[-1][0]).all() and 0 <= int(state["chosen"][0]) < K_
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 6: the job
def test_infer_video_and_the_job(tmp_path, monkeypatch):
    from video_diffusion_amd import video_sample as vs
    model, diff = tiny(timestep_respacing="logsnr3")
    g = torch.Generator().manual_seed(60)
    batch = (torch.rand(2, 10, 3, 32, 32, generator=g) * 2 - 1).cuda()
    op = (resize_matrix(32, 8), resize_matrix(32, 8))
    a = check_separable_operator(*op)[0].numpy()
    y = measure_separable(torch.rand(2, 10, 3, 32, 32, generator=g) * 2 - 1, *op)
    outs = {}
    for ex in ("eager", "graph"):
        torch.manual_seed(61)
        outs[ex], _ = vs.infer_video("autoreg", model, diff, batch, 6, 2, 4, measurement=y, operator=op, executor=ex, sampler="dpmpp_2m")
        gap = np.abs(lr.two_fp64(a, outs[ex], a) - y.numpy().astype(np.float64))[:, 2:]
        print(f"infer_video {ex}: A x - y on the generated frames: max {gap.max():.2e}")
        # (the ceiling of test_window_of_40_frames_runs: gamma_96 times |A| |P| |A| |x| < 17)
        assert np.isfinite(outs[ex]).all() and np.array_equal(outs[ex][:, :2], batch[:, :2].cpu().numpy()) and gap.max() <= 1e-4
    assert np.array_equal(outs["eager"], outs["graph"])                          # dpmpp_2m draws no noise: both executors, the same bits
    # the eager chain per window, inside linear_dps_scope
    torch.manual_seed(61)
    out, _ = vs.infer_video("autoreg", model, diff, batch, 6, 2, 4, measurement=y, operator=op, dps_zeta=0.3)
    torch.manual_seed(61)
    samples = torch.zeros_like(batch).cpu()
    samples[:, :2] = batch[:, :2].cpu()
    for obs_i, lat_i in inference_util.inference_strategies["autoreg"](video_length=10, num_obs=2, max_frames=6, step_size=4, optimal_schedule_path=None):
        fi = torch.tensor(list(obs_i) + list(lat_i))
        x0 = samples[:, fi].clone().cuda()
        obs_mask, latent_mask, km = vs.get_masks(x0, len(obs_i))
        kw = dict(frame_indices=fi.repeat(2, 1).cuda(), x0=x0, obs_mask=obs_mask.cuda(), latent_mask=latent_mask.cuda(), kinda_marg_mask=km.cuda(),
                  x_t_minus_1=x0, observed_frames="x_0")
        local = x0.clone()
        with diff.linear_dps_scope(model, y[:, fi], *op, zeta=0.3):
            for tv in (2, 1, 0):
                local = diff.p_sample(model, local, _t(2, tv), model_kwargs=kw)["sample"]
        samples[:, list(lat_i)] = local[:, -len(lat_i):].cpu()
    assert np.array_equal(out, samples.numpy()) and np.isfinite(out).all()
    for ex in ("eager", "graph"):
        torch.manual_seed(62)
        smc, _ = vs.infer_video("autoreg", model, diff, batch, 6, 2, 4, measurement=y, operator=op, particles=2, sigma_y=0.5, executor=ex)
        assert smc.shape == out.shape and np.isfinite(smc).all() and np.array_equal(smc[:, :2], batch[:, :2].cpu().numpy())
    for bad, what in ((dict(operator=op, sr_scale=4), "leave them at their defaults"), (dict(operator=op, measurement=None), "operator needs a measurement"),
                      (dict(operator=(op[0],)), "operator is a pair"), (dict(operator=op, operator_rtol=2.0), "rtol"),
                      (dict(operator=op, measurement=y[..., :4, :]), "y must be")):
        with pytest.raises(ValueError, match=what):
            vs.infer_video("autoreg", model, diff, batch, 6, 2, 4, **{**dict(measurement=y), **bad})
    model.check_device_errors()
    # the job: --sr_kernel bicubic, and the two matrix files with --dps_zeta; the suffixed run directories
    vids = (torch.rand(2, 8, 3, 32, 32, generator=g) * 2 - 1)
    np.save(tmp_path / "videos.npy", vids.numpy())
    np.save(tmp_path / "y.npy", measure_separable(vids, *op).numpy())
    np.save(tmp_path / "ah.npy", op[0].numpy())
    np.save(tmp_path / "aw.npy", op[1].numpy())
    monkeypatch.chdir(tmp_path)
    ap = vs.build_parser()
    common = ["--videos", str(tmp_path / "videos.npy"), "--inference_mode", "autoreg", "--max_frames", "6", "--obs_length", "2", "--step_size", "4",
              "--batch_size", "2", "--timestep_respacing", "logsnr3", "--image_size", "32", "--num_channels", "32", "--num_res_blocks", "1",
              "--sampler", "ddim", "--eval_dir", str(tmp_path / "out"), "--measurement", str(tmp_path / "y.npy")]
    for extra, tail in ((["--sr_scale", "4", "--sr_kernel", "bicubic"], "_ddim_lin8x8"),
                        (["--operator_h", str(tmp_path / "ah.npy"), "--operator_w", str(tmp_path / "aw.npy"), "--dps_zeta", "0.5"], "_ddim_lin8x8_dps0.5"),
                        (["--sr_scale", "4", "--sr_kernel", "bilinear", "--particles", "2", "--measurement_sigma", "0.5", "--eta", "1.0"], "_ddim_lin8x8_smc2")):
        args = vs.check_particle_arguments(ap, ap.parse_args(common + extra))
        out_dir = vs.run(args, device=torch.device("cuda", 0))
        assert str(out_dir).endswith(tail), out_dir
        for i in range(2):
            f = np.load(out_dir / "samples" / f"sample_{i:04d}-0.npy")
            assert f.dtype == np.uint8 and f.shape == (8, 3, 32, 32) and np.array_equal(f[:2], vs.to_uint8(vids.numpy()[i])[:2])
    for bad, what in ((["--operator_h", "a.npy"], "come together"), (["--sr_kernel", "bicubic"], "needs --sr_scale"),
                      (["--sr_scale", "4", "--sr_kernel", "bicubic", "--gray"], "are not served")):
        with pytest.raises(SystemExit):
            vs.check_particle_arguments(ap, ap.parse_args(common + bad))


# ---------------------------------------------------------------------------------------------------------------- 7: refusals
def test_every_refusal_by_message():
    model, diff = tiny()
    diff._bind(model)
    L = _lib.lib()
    c = _rand_window(2, 6, 32, 2, seed=195)
    kw, x = _window_kw(c), c["x"].cuda()
    A = resize_matrix(32, 8)
    y = _window_y(c, A, A, seed=196)
    fn = lambda v: v                                                             # noqa: E731
    tt = _t(2, 3)
    with diff.linear_dps_scope(model, y, A, A, zeta=0.5):
        for call, what in ((lambda: diff.dpmpp_2m_sample(model, x, tt, model_kwargs=kw), "dpmpp_2m_sample"),
                           (lambda: diff.dpmpp_2m_sde_sample(model, x, tt, model_kwargs=kw), "dpmpp_2m_sde_sample"),
                           (lambda: diff.unipc_sample(model, x, tt, model_kwargs=kw), "unipc_sample"),
                           (lambda: diff.ddim_reverse_sample(model, x, tt, model_kwargs=kw), "ddim_reverse_sample"),
                           (lambda: diff.p_sample(model, x, tt, denoised_fn=fn, model_kwargs=kw), "denoised_fn"),
                           (lambda: diff.p_sample(model, x, tt, model_kwargs=kw, use_gradient_method=True), "use_gradient_method"),
                           (lambda: diff.p_sample(model, x, tt, model_kwargs=kw, return_attn_weights=True), "return_attn_weights"),
                           (lambda: diff.ddim_sample(model, x, tt, model_kwargs=kw, cfg_scale=2.0), "cfg_scale != 1"),
                           (lambda: WindowExecutor(model, diff).begin(x, kw), "WindowExecutor.begin")):
            with pytest.raises(_lib.VdError, match=f"{what} inside linear_dps_scope is not served"):
                call()
        with diff.cfg_scale_scope(model, 2.0):
            with pytest.raises(_lib.VdError, match="cfg_scale != 1 .cfg_scale_scope. inside linear_dps_scope"):
                diff.p_sample(model, x, tt, model_kwargs=kw)
        for opts in (dict(cfg_rescale=0.5), dict(dynamic_threshold=0.9)):
            with diff.guidance_scope(model, **opts):
                with pytest.raises(_lib.VdError, match="guidance_scope with cfg_rescale or dynamic_threshold set inside linear_dps_scope"):
                    diff.p_sample(model, x, tt, model_kwargs=kw)
        with diff.known_region_scope(model, torch.zeros_like(x), torch.ones(2, 6, 32, 32, device="cuda")):
            with pytest.raises(_lib.VdError, match="known_region_scope inside linear_dps_scope"):
                diff.p_sample(model, x, tt, model_kwargs=kw)
        with diff.measurement_scope(model, y, 4):
            with pytest.raises(_lib.VdError, match="measurement_scope inside linear_dps_scope"):
                diff.ddim_sample(model, x, tt, model_kwargs=kw)
        with diff.linear_measurement_scope(model, y, A, A):
            with pytest.raises(_lib.VdError, match="linear_measurement_scope inside linear_dps_scope"):
                diff.ddim_sample(model, x, tt, model_kwargs=kw)
        with pytest.raises(ValueError, match="linear_dps_scope: y must be"):
            diff.ddim_sample(model, x[:, :4], tt, model_kwargs={k: (v[:, :4] if torch.is_tensor(v) else v) for k, v in kw.items()})
        with pytest.raises(NotImplementedError, match="linear_dps_scope together with steering_scope is not served"):
            with diff.steering_scope(model, lambda x0, t: x0.flatten(1).sum(1), particles=2):
                diff.p_sample(model, x, tt, model_kwargs=kw)
    with diff.linear_measurement_scope(model, y, A, A):
        for call, what in ((lambda: diff.ddim_reverse_sample(model, x, tt, model_kwargs=kw), "ddim_reverse_sample"),
                           (lambda: diff.p_sample(model, x, tt, denoised_fn=fn, model_kwargs=kw), "denoised_fn"),
                           (lambda: diff.p_sample(model, x, tt, model_kwargs=kw, use_gradient_method=True), "use_gradient_method"),
                           (lambda: diff.p_mean_variance(model, x, tt, denoised_fn=fn, model_kwargs=kw), "denoised_fn")):
            with pytest.raises(_lib.VdError, match=f"{what} inside linear_measurement_scope is not served"):
                call()
        with diff.known_region_scope(model, torch.zeros_like(x), torch.ones(2, 6, 32, 32, device="cuda")):
            with pytest.raises(_lib.VdError, match=r"a linear measurement \(vd_set_linear_measurement\) together with a known region"):
                diff.p_sample(model, x, tt, model_kwargs=kw)
        with diff.measurement_scope(model, y, 4):
            with pytest.raises(_lib.VdError, match=r"a linear measurement \(vd_set_linear_measurement\) together with a measurement"):
                diff.p_sample(model, x, tt, model_kwargs=kw)
        with pytest.raises(NotImplementedError, match="linear_measurement_scope together with steering_scope is not served"):
            with diff.steering_scope(model, lambda x0, t: x0.flatten(1).sum(1), particles=2):
                diff.p_sample(model, x, tt, model_kwargs=kw)
        with pytest.raises(ValueError, match="linear_measurement_scope: y must be"):
            diff.ddim_sample(model, x[:, :4], tt, model_kwargs={k: (v[:, :4] if torch.is_tensor(v) else v) for k, v in kw.items()})
        for flag in ("prefix_cache", "suffix_skip"):
            with pytest.raises(_lib.VdError, match=rf"a linear measurement \(vd_set_linear_measurement\) together with the window {flag.replace('_', ' ')}"):
                WindowExecutor(model, diff, **{flag: True}).begin(x, kw)
        with pytest.raises(_lib.VdError, match=r"ddim_reverse_sample together with a linear measurement"):
            WindowExecutor(model, diff).begin(x, _window_kw(c, "x_t_minus_1"), sampler="ddim_reverse", renoise=False)
        model._require_guidance()
        with pytest.raises(_lib.VdError, match="eps_vjp together with a linear measurement"):
            diff.eps_vjp(model, x, tt, torch.ones_like(x), model_kwargs=kw)
    for bad, what in ((dict(zeta=-1.0), "zeta"), (dict(A_h=torch.ones(9, 8)), "M <= n"), (dict(A_h=torch.zeros(8, 32)), "all zero"),
                      (dict(y=y[0]), r"y must be a \(B, T, 3, Mh, Mw\) tensor"), (dict(y=y[..., :4]), "y must be"),
                      (dict(y=torch.full_like(y, float("inf"))), "y must be finite")):
        args = dict(y=y, A_h=A, A_w=A, zeta=0.5)
        args.update(bad)
        with pytest.raises(ValueError, match=what):
            diff.linear_dps_scope(model, args["y"], args["A_h"], args["A_w"], zeta=args["zeta"])
        if "zeta" not in bad:
            with pytest.raises(ValueError, match=what):
                diff.linear_measurement_scope(model, args["y"], args["A_h"], args["A_w"])
    with pytest.raises(TypeError):
        diff.linear_dps_scope(model, y, A, A)                                        # zeta is required
    for kwargs, what in ((dict(back=(torch.ones(32, 8),)), "back is a pair"), (dict(back=(torch.ones(8, 32), torch.ones(32, 8))), "P_h must be"),
                         (dict(rtol=1.5), "rtol")):
        with pytest.raises(ValueError, match=what):
            diff.linear_measurement_scope(model, y, A, A, **kwargs)
    for kwargs, what in ((dict(operator=(A, A)), "needs measurement= and sigma_y="), (dict(operator=(A, A), measurement=y, sigma_y=1.0, sr_scale=2), "leave them at their defaults"),
                         (dict(operator=(A, A), measurement=y, sigma_y=1.0, blur_kernel=torch.ones(3, 3)), "leave them at their defaults"),
                         (dict(operator=(A,), measurement=y, sigma_y=1.0), "operator is a pair"), (dict(operator=(A, A), measurement=y), "sigma_y")):
        with pytest.raises(ValueError, match=what):
            diff.steering_scope(model, (lambda x0, t: x0.flatten(1).sum(1)) if "measurement" not in kwargs else None, particles=2, **kwargs)
    for kwargs, what in ((dict(operator=(A, A)), "give one of them"), (dict(operator=(A, A), measurement=y, particle_measurement=y), "give one of them"),
                         (dict(operator=(A, A), measurement=y, sr_scale=4), "leave them at their defaults")):
        with pytest.raises(ValueError, match=what):
            WindowExecutor(model, diff).begin(x, kw, **kwargs)
    # the engine's own refusals of the step entry, by message
    model._require_guidance()
    pk = model._pack_kwargs(x, kw)
    sample, xs = torch.empty_like(x), torch.empty_like(x)
    noise, yd = torch.zeros_like(x), y.cuda().float().contiguous()

    def step(m=model, sampler=0, zeta=0.5):
        return L.vd_linear_dps_step(m._handle, 2, 6, *m._window_ptrs(x, pk), _lib.ptr(tt), pk["obs_mode"], 1, sampler, 0.0, _lib.ptr(noise),
                                    _lib.ptr(yd), zeta, _lib.ptr(sample), _lib.ptr(xs), None, None, _lib.current_stream())
    assert step() != 0 and b"linear_dps: no operator is installed" in L.vd_last_error()
    a32 = check_separable_operator(A, A)[0]
    _lib.check(L.vd_set_linear_operator(model._handle, _lib.ptr(a32), 8, _lib.ptr(a32), 8, None, None))
    for kwargs, what in ((dict(sampler=2), b"linear_dps: p_sample (0) or ddim_sample (1)"), (dict(zeta=-1.0), b"linear_dps: zeta must be finite and not negative"),
                         (dict(zeta=float("nan")), b"zeta must be finite and not negative")):
        assert step(**kwargs) != 0 and what in L.vd_last_error(), kwargs
    for setter, value, off, what in ((L.vd_set_cfg_scale, 2.0, 1.0, b"linear_dps together with cfg_scale != 1"),
                                     (L.vd_set_guidance_rescale, 0.5, 0.0, b"linear_dps together with guidance_rescale"),
                                     (L.vd_set_dynamic_threshold, 0.9, 0.0, b"linear_dps together with dynamic_threshold")):
        _lib.check(setter(model._handle, value))
        assert step() != 0 and what in L.vd_last_error()
        _lib.check(setter(model._handle, off))
    with diff.measurement_scope(model, y, 4):
        assert step() != 0 and b"linear_dps together with a measurement" in L.vd_last_error()
    assert step() == 0                                                           # the engine is as it was: the step runs
    _lib.check(L.vd_set_linear_operator(model._handle, None, 0, None, 0, None, None))
    mx, dx_ = tiny(predict_xstart=True)
    with dx_.linear_dps_scope(mx, y, A, A, zeta=0.5):
        with pytest.raises(NotImplementedError, match="linear_dps_scope with predict_xstart=True: epsilon-prediction models only"):
            dx_.p_sample(mx, x, tt, model_kwargs=kw)
    torch.cuda.synchronize()
    model.check_device_errors()
