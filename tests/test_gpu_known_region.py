"""GPU: pixel-mask inpainting (this project's extension, RePaint) -- the merge pass and the forward jump per element against the
float64 restatement (tests/known_region_restated.py) inside bounds derived by the interval helpers of tests/step_nll_restated.py, the
step on the network against the plain step, the window graph and the loops against the eager chain of plain step + vd_known_merge +
vd_q_jump fed vd_randn noise at the documented Philox offsets, infer_video and the video_sample job.  Bit equality or a derived bound
throughout; nothing here is tuned on the code under test."""
import numpy as np
import pytest
import torch

from known_region_restated import (jump_noise_f32, jump_rows, known_merge_bound, known_merge_f32, merge_noise_f32, merged,
                                   q_jump_bound, q_jump_f32)
from step_compose import MODES, _eager_chain, _randn
from step_nll_restated import normal_bound, normal_fp64, ratio, tables
from test_gpu_dpmpp_2m import _rand_window, _t, _window_kw, tiny
from video_diffusion_amd import _lib
from video_diffusion_amd.executor import WindowExecutor
from video_diffusion_amd.respace import repaint_schedule

pytestmark = pytest.mark.gpu


def _np(v):
    return v.detach().cpu().numpy()


def _bits(v):
    return np.ascontiguousarray(_np(v) if torch.is_tensor(v) else v).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _region(B, T, H, W, seed, lat_off=None):
    """g, k, z (B, T, 3, H, W), a pixel mask that differs per frame and per item (about half known, whole groups of four on both sides)
    and lat (B, T) with frame `lat_off` of every item not latent."""
    g = torch.Generator().manual_seed(seed)
    sample = torch.randn(B, T, 3, H, W, generator=g)
    src = torch.rand(B, T, 3, H, W, generator=g) * 2 - 1
    z = torch.randn(B, T, 3, H, W, generator=g)
    mask = (torch.rand(B, T, H, W, generator=g) < 0.5).float()
    mask[:, :, 0, : min(W, 4)] = 0                                               # a group of four that stays unknown
    mask[:, :, H - 1, : min(W, 4)] = 1                                           # ... and one that is known throughout
    mask[0, 0] = 0                                                               # a latent frame without a known pixel
    lat = torch.ones(B, T)
    if lat_off is not None:
        lat[:, lat_off] = 0
    return sample, src, z, mask, lat


def _merge(model, sample, src, mask, lat, t, noise=None, seed=0, offset=0, misalign=False):
    """vd_known_merge on device copies -> the merged sample (numpy, (B, T, 3, hw)).  misalign: `sample` at an address 4 bytes off."""
    B, T, _, H, W = sample.shape
    d = [v.cuda().contiguous() for v in (src, mask, lat.reshape(-1))]
    if misalign:
        buf = torch.empty(sample.numel() + 1, device="cuda")
        s = buf[1:].view(sample.shape)
        s.copy_(sample)
        assert s.data_ptr() % 16 == 4
    else:
        s = sample.cuda().clone()
    nz = None if noise is None else noise.cuda().contiguous()
    tt = torch.as_tensor(t, dtype=torch.int64).cuda()
    _lib.check(_lib.lib().vd_known_merge(model._handle, B, T, H * W, _lib.ptr(s), _lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]), _lib.ptr(tt),
                                         _lib.ptr(nz), seed, offset, _lib.current_stream()))
    return _np(s).reshape(B, T, 3, H * W)


def _flat(*vs):
    return [_np(v).reshape(*v.shape[:-2], -1) if v.dim() > 2 else _np(v) for v in vs]


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("H", [8, 7])
def test_merge_pass_per_element(H):
    """vd_known_merge, B = 2, T = 3, 8 x 8 frames (four elements per thread) and 7 x 7 (element by element), frame 1 not latent."""
    model, diff = tiny()
    diff._bind(model)
    tab, N = tables(diff), diff.num_timesteps
    B, T = 2, 3
    sample, src, z, mask, lat = _region(B, T, H, H, seed=11, lat_off=1)
    g, k, zz, m = _flat(sample, src, z, mask)
    latn = _np(lat)
    sel = merged(m, latn)
    assert sel.any() and not sel[:, 1].any() and not sel[0, 0].any() and (~sel[:, 0]).any()
    uniform = {}
    for tv in (0, 1, N - 1):
        t = [tv] * B
        got = _merge(model, sample, src, mask, lat, t, noise=z)
        want, lim = known_merge_bound(tab, g, k, m, latn, t, zz)
        r = ratio(got, want, lim)
        print(f"H={H} t={tv} explicit noise: max |d| / bound = {r[sel].max():.3f}; f32 restatement equal: {_same_bits(got, known_merge_f32(tab, g, k, m, latn, t, zz))}")
        assert np.array_equal(_bits(got)[~sel], _bits(g)[~sel])                  # unknown pixels, the non-latent frame: the input's bits
        assert (r <= 1.0).all(), (tv, float(r.max()))
        if tv == 0:
            assert np.array_equal(_bits(got)[sel], _bits(k)[sel])                # t = 0: the source itself
        else:
            assert not np.array_equal(got[sel], k[sel])
        uniform[tv] = got
        # in-kernel Philox: element i of the stream at offset + (B per) // 4; the device's logf / sincosf are allowed normal_bound
        for seed, off in ((5, 0), (2 ** 63 + 11, 2 ** 32 - 2)):
            got_p = _merge(model, sample, src, mask, lat, t, seed=seed, offset=off)
            n = g.size
            zp = merge_noise_f32(seed, off, g.shape)
            _, rad = normal_fp64(seed, off + n // 4, np.arange(n))
            want, lim = known_merge_bound(tab, g, k, m, latn, t, zp)
            s1 = float(tab["s1"][max(tv - 1, 0)]) if tv >= 1 else 0.0
            lim = lim + np.where(sel, s1 * normal_bound(rad).reshape(g.shape), 0.0)
            r = ratio(got_p, want, lim)
            print(f"H={H} t={tv} Philox({seed}, {off}): max |d| / bound = {r[sel].max():.3f}")
            assert np.array_equal(_bits(got_p)[~sel], _bits(g)[~sel]) and (r <= 1.0).all(), (tv, seed, float(r.max()))
            if tv >= 1:
                assert not np.array_equal(got_p[sel], got[sel])
    # mixed t per item: bit-equal to the uniform calls
    for ts in ([1, N - 1], [N - 1, 0]):
        got = _merge(model, sample, src, mask, lat, ts, noise=z)
        for b, tv in enumerate(ts):
            assert _same_bits(got[b], uniform[tv][b]), (ts, b)
    # an index outside the schedule: NaN for that item only
    for bad in (N, -1):
        got = _merge(model, sample, src, mask, lat, [1, bad], noise=z)
        assert _same_bits(got[0], uniform[1][0]) and np.isnan(got[1]).all()
    # the scalar path on the same data: an unaligned sample tensor gives the aligned call's bits
    for tv in (0, N - 1):
        assert _same_bits(_merge(model, sample, src, mask, lat, [tv] * B, noise=z, misalign=True), uniform[tv])
        assert _same_bits(_merge(model, sample, src, mask, lat, [tv] * B, seed=5, offset=3, misalign=True),
                          _merge(model, sample, src, mask, lat, [tv] * B, seed=5, offset=3))
    model.check_device_errors()                                                  # the merge sets no error bit of its own


# ---------------------------------------------------------------------------------------------------------------- 2
def _jump(model, x, lat, t, noise=None, seed=0, offset=0, inplace=False):
    B, T, _, H, W = x.shape
    xs = x.cuda().clone()
    out = xs if inplace else torch.full_like(xs, 7.0)
    nz = None if noise is None else noise.cuda().contiguous()
    tt = torch.as_tensor(t, dtype=torch.int64).cuda()
    rc = _lib.lib().vd_q_jump(model._handle, B, T, H * W, _lib.ptr(xs), _lib.ptr(lat.reshape(-1).cuda()), _lib.ptr(tt), _lib.ptr(nz), seed, offset,
                              _lib.ptr(out), _lib.current_stream())
    _lib.check(rc)
    return _np(out)


@pytest.mark.parametrize("H", [8, 7])
def test_jump_per_element(H):
    model, diff = tiny()
    diff._bind(model)
    N = diff.num_timesteps
    rows = jump_rows(diff.betas)
    B, T = 2, 3
    x, _, z, _, lat = _region(B, T, H, H, seed=21, lat_off=2)
    xn, zn, latn = _np(x), _np(z), _np(lat)
    is_lat = np.broadcast_to(latn.reshape(B, T, 1, 1, 1) == 1, xn.shape)
    uniform = {}
    for tv in (0, 1, N - 1):
        got = _jump(model, x, lat, [tv] * B, noise=z)
        want, lim = q_jump_bound(rows, xn.reshape(B, T, 3, -1), latn, [tv] * B, zn.reshape(B, T, 3, -1))
        r = ratio(got.reshape(want.shape), want, lim)
        print(f"H={H} t={tv}: max |d| / bound = {r.max():.3f}; f32 restatement equal: "
              f"{_same_bits(got.reshape(want.shape), q_jump_f32(rows, xn.reshape(B, T, 3, -1), latn, [tv] * B, zn.reshape(B, T, 3, -1)))}")
        assert (r <= 1.0).all(), (tv, float(r.max()))
        assert np.array_equal(_bits(got)[~is_lat], _bits(xn)[~is_lat]) and not np.array_equal(got[is_lat], xn[is_lat])
        assert _same_bits(_jump(model, x, lat, [tv] * B, noise=z, inplace=True), got)
        uniform[tv] = got
        seed, off = 9, 1000
        got_p = _jump(model, x, lat, [tv] * B, seed=seed, offset=off)
        zp = jump_noise_f32(seed, off, (B, T, 3, H * H))
        _, rad = normal_fp64(seed, off, np.arange(xn.size))
        want, lim = q_jump_bound(rows, xn.reshape(B, T, 3, -1), latn, [tv] * B, zp)
        lim = lim + np.where(is_lat.reshape(want.shape), float(rows[1][tv]) * normal_bound(rad).reshape(want.shape), 0.0)
        r = ratio(got_p.reshape(want.shape), want, lim)
        print(f"H={H} t={tv} Philox: max |d| / bound = {r.max():.3f}")
        assert (r <= 1.0).all(), (tv, float(r.max()))
    got = _jump(model, x, lat, [N - 1, 1], noise=z)
    assert _same_bits(got[0], uniform[N - 1][0]) and _same_bits(got[1], uniform[1][1])
    for bad in (N, -1):
        got = _jump(model, x, lat, [1, bad], noise=z)
        assert _same_bits(got[0], uniform[1][0]) and np.isnan(got[1]).all()
    model.check_device_errors()


def test_jump_rows_belong_to_the_schedule():
    model, diff = tiny(timestep_respacing="logsnr5")
    diff._bind(model)
    L = _lib.lib()
    r6 = np.zeros(6, np.float32)
    assert L.vd_set_jump_rows(model._handle, 6, _lib.ptr(r6), _lib.ptr(r6)) != 0 and b"bound schedule" in L.vd_last_error()
    x, _, z, _, lat = _region(2, 3, 8, 8, seed=22)
    _jump(model, x, lat, [1, 2], noise=z)
    tab = diff._device_tables()
    tm = np.ascontiguousarray(np.array(diff.timestep_map, dtype=np.int32))
    try:
        _lib.check(L.vd_set_schedule(model._handle, diff.num_timesteps, _lib.ptr(tab), _lib.ptr(tm), 1.0))      # drops the rows
        with pytest.raises(_lib.VdError, match="vd_set_jump_rows"):
            _jump(model, x, lat, [1, 2], noise=z)
    finally:
        model._bound_schedule = None
    diff._bind(model)
    _jump(model, x, lat, [1, 2], noise=z)
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 3
def _window_region(c, seed):
    """known_src, known_mask (B, T, S, S) and known noise for the window `c`; every frame gets known and unknown pixels."""
    B, T, _, S, _ = c["x"].shape
    g = torch.Generator().manual_seed(seed)
    src = (torch.rand(B, T, 3, S, S, generator=g) * 2 - 1).cuda()
    mask = (torch.rand(B, T, S, S, generator=g) < 0.5).float().cuda()
    z = torch.randn(B, T, 3, S, S, generator=g).cuda()
    return src, mask, z


def _check_merged(diff, plain, got, src, mask, lat, tv, z, tag):
    """got against the merge of the plain step's sample: unknown pixels and non-latent frames bit-equal, merged ones inside the bound."""
    B, T = plain.shape[:2]
    g, k, zz, m = _flat(plain, src, z, mask)
    latn = _np(lat).reshape(B, T)
    sel = merged(m, latn)
    want, lim = known_merge_bound(tables(diff), g, k, m, latn, [tv] * B, zz)
    gotn = _np(got).reshape(g.shape)
    r = ratio(gotn, want, lim)
    print(f"{tag} t={tv}: merged {int(sel.sum())} of {sel.size}, max |d| / bound = {r.max():.3f}")
    assert sel.any() and np.array_equal(_bits(gotn)[~sel], _bits(g)[~sel]) and (r <= 1.0).all(), (tag, tv, float(r.max()))
    if tv == 0:
        assert np.array_equal(_bits(gotn)[sel], _bits(k)[sel])


@pytest.mark.parametrize("sampler,eta", [("p_sample", 0.0), ("ddim", 0.0), ("ddim", 0.5), ("dpmpp_2m", 0.0)])
def test_the_step_on_the_network(sampler, eta):
    """B = 2, 2 observed of 6 frames: with the same sampler noise the step inside the scope is the plain step with the merge behind it."""
    model, diff = tiny()
    N = diff.num_timesteps
    c = _rand_window(2, 6, 32, 2, seed=30)
    kw, x = _window_kw(c), c["x"].cuda()
    src, mask, z = _window_region(c, seed=31)
    noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(32)).cuda()
    prev = (torch.rand(x.shape, generator=torch.Generator().manual_seed(33)) * 2 - 1).cuda() if sampler == "dpmpp_2m" else None
    mode = MODES[sampler]
    for tv in (N - 1, 3, 0):
        plain, plain_x0 = diff._fused_step(mode, model, x, _t(2, tv), True, kw, eta=eta, noise=noise, prev_xstart=prev)
        with diff.known_region_scope(model, src, mask, known_noise=z):
            assert _lib.lib().vd_known_region(model._handle) == 1
            got, got_x0 = diff._fused_step(mode, model, x, _t(2, tv), True, kw, eta=eta, noise=noise, prev_xstart=prev)
        assert _lib.lib().vd_known_region(model._handle) == 0
        assert torch.equal(got_x0, plain_x0)                                     # pred_xstart stays the model's own
        _check_merged(diff, plain, got, src, mask, kw["latent_mask"], tv, z, f"{sampler} eta={eta}")
        again, _ = diff._fused_step(mode, model, x, _t(2, tv), True, kw, eta=eta, noise=noise, prev_xstart=prev)
        assert torch.equal(again, plain)                                         # behind the scope: the plain step
    model.check_device_errors()


def test_the_step_under_guidance_and_the_refusals():
    model, diff = tiny()
    N = diff.num_timesteps
    c = _rand_window(2, 6, 32, 2, seed=34)
    kw, x = _window_kw(c), c["x"].cuda()
    src, mask, z = _window_region(c, seed=35)
    noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(36)).cuda()
    tv = N - 2
    with diff.guidance_scope(model, dynamic_threshold=0.9):
        plain, plain_x0 = diff._fused_step(0, model, x, _t(2, tv), True, kw, noise=noise, cfg_scale=2.0)
        with diff.known_region_scope(model, src, mask, known_noise=z):
            got, got_x0 = diff._fused_step(0, model, x, _t(2, tv), True, kw, noise=noise, cfg_scale=2.0)
    unguided, _ = diff._fused_step(0, model, x, _t(2, tv), True, kw, noise=noise)
    assert not torch.equal(plain, unguided) and torch.equal(got_x0, plain_x0)
    _check_merged(diff, plain, got, src, mask, kw["latent_mask"], tv, z, "cfg_scale=2 dynamic_threshold=0.9")
    # scopes nest and restore; the scope draws its noise behind the sampler's when none is fixed
    src2 = -src
    with diff.known_region_scope(model, src, mask, known_noise=z):
        with diff.known_region_scope(model, src2, mask, known_noise=z):
            inner, _ = diff._fused_step(1, model, x, _t(2, 0), True, kw, noise=noise)
        outer, _ = diff._fused_step(1, model, x, _t(2, 0), True, kw, noise=noise)
    sel = torch.from_numpy(merged(_flat(mask)[0], _np(kw["latent_mask"]).reshape(2, 6))).view(2, 6, 3, 32, 32).cuda()
    assert torch.equal(inner[sel], src2[sel]) and torch.equal(outer[sel], src[sel])
    torch.manual_seed(37)
    with diff.known_region_scope(model, src, mask):
        drawn = diff.p_sample(model, x, _t(2, tv), model_kwargs=kw)["sample"]
    torch.manual_seed(37)
    n1, n2 = torch.randn_like(x), torch.randn_like(x)
    with diff.known_region_scope(model, src, mask, known_noise=n2):
        fixed, _ = diff._fused_step(0, model, x, _t(2, tv), True, kw, noise=n1)
    assert torch.equal(drawn, fixed)
    with diff.known_region_scope(model, src, mask):
        with pytest.raises(NotImplementedError, match="ddim_reverse_sample inside known_region_scope"):
            diff.ddim_reverse_sample(model, x, _t(2, 3), model_kwargs=kw)
        with pytest.raises(NotImplementedError, match="denoised_fn inside known_region_scope"):
            diff.p_sample(model, x, _t(2, 3), denoised_fn=lambda v: v, model_kwargs=kw)
        with pytest.raises(NotImplementedError, match="denoised_fn inside known_region_scope"):
            diff.dpmpp_2m_sample(model, x, _t(2, 3), denoised_fn=lambda v: v, model_kwargs=kw)
        with pytest.raises(NotImplementedError, match="use_gradient_method inside known_region_scope"):
            diff.p_sample(model, x, _t(2, 3), model_kwargs=kw, use_gradient_method=True)
        # the engine refuses the reverse step by name as well
        L = _lib.lib()
        tt, out = _t(2, 3), torch.empty_like(x)
        pk = model._pack_kwargs(x, kw)
        rc = L.vd_ddim_reverse_sample(model._handle, 2, 6, *model._window_ptrs(x, pk), _lib.ptr(tt), pk["obs_mode"], 1, _lib.ptr(out), None, None,
                                      _lib.current_stream())
        assert rc != 0 and b"ddim_reverse_sample together with a known region" in L.vd_last_error()
    assert _lib.lib().vd_known_region(model._handle) == 0
    with pytest.raises(ValueError, match="0 and 1 only"):
        diff.known_region_scope(model, src, mask * 0.5).__enter__()
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 4, 5
@pytest.mark.parametrize("sampler,eta", [("p_sample", 0.0), ("ddim", 0.5), ("dpmpp_2m", 0.0)])
def test_window_graph_with_a_region_and_jumps(sampler, eta):
    """begin(known...), run(3), jump(2), run(): to the bit the eager chain; a second window reuses the graph; a window without a
    region on the same executor is today's window."""
    model, diff = tiny()
    diff._bind(model)
    N = diff.num_timesteps
    ex = WindowExecutor(model, diff)
    ops = [("step", N - 1 - i) for i in range(3)] + [("jump", N - 3), ("jump", N - 2)] + [("step", tv) for tv in range(N - 2, -1, -1)]
    graphs = None
    for wi in range(2):
        c = _rand_window(2, 6, 32, 2, seed=400 + wi)
        kw, x_init = _window_kw(c), c["x"].cuda()
        src, mask, _ = _window_region(c, seed=410 + wi)
        ex.begin(x_init, kw, sampler=sampler, eta=eta, seed=40 + wi, known_src=src, known_mask=mask)
        assert _lib.lib().vd_known_region(model._handle) == 0                    # engine state for the length of begin() only
        if wi == 0:
            graphs = ex.graphs
        assert ex.graphs == graphs and ex._left == N
        mid = ex.run(3).clone()
        up = ex.jump(2).clone()
        assert ex._left == N - 1
        got = ex.run().clone()
        with pytest.raises(_lib.VdError, match="t would pass 0"):
            ex.run(1)
        want, kept = _eager_chain(model, diff, sampler, eta, x_init, kw, src, mask, 40 + wi, ops, keep=(3, 5))
        assert torch.equal(kept[3], mid), (wi, float((kept[3] - mid).abs().max()))
        assert torch.equal(kept[5], up), (wi, float((kept[5] - up).abs().max()))
        assert torch.equal(want, got) and torch.isfinite(got).all(), (wi, float((want - got).abs().max()))
        sel = torch.from_numpy(merged(_flat(mask)[0], _np(kw["latent_mask"]).reshape(2, 6))).view(got.shape).cuda()
        assert torch.equal(got[sel], src[sel])                                   # the window ends on the source's bits
    # without a region, on the same executor and buffers: the window as it always was
    c = _rand_window(2, 6, 32, 2, seed=420)
    kw, x_init = _window_kw(c), c["x"].cuda()
    ex.begin(x_init, kw, sampler=sampler, eta=eta, seed=44)
    with pytest.raises(_lib.VdError, match="no known region"):
        ex.jump(1)
    got = ex.run().clone()
    plain_ops = [("step", tv) for tv in range(N - 1, -1, -1)]
    want, _ = _eager_chain(model, diff, sampler, eta, x_init, kw, None, None, 44, plain_ops)
    assert torch.equal(want, got)
    model.check_device_errors()


def test_window_refusals():
    model, diff = tiny()
    diff._bind(model)
    N = diff.num_timesteps
    L = _lib.lib()
    c = _rand_window(2, 6, 32, 2, seed=430)
    kw, x_init = _window_kw(c), c["x"].cuda()
    src, mask, z = _window_region(c, seed=431)
    ex = WindowExecutor(model, diff)
    ex.begin(x_init, kw, sampler="ddim", seed=1, known_src=src, known_mask=mask)
    with pytest.raises(_lib.VdError, match="t would pass num_timesteps - 1"):
        ex.jump(1)
    ex.run(2)
    ex.jump(2)
    with pytest.raises(_lib.VdError, match="t would pass num_timesteps - 1"):
        ex.jump(1)
    assert ex._left == N
    with pytest.raises(NotImplementedError, match="ddim_reverse' together with a known region"):
        ex.begin(x_init, kw, sampler="ddim_reverse", known_src=src, known_mask=mask)
    for opt in ("prefix_cache", "suffix_skip"):
        with pytest.raises(NotImplementedError, match=f"{opt} together with a known region"):
            WindowExecutor(model, diff, **{opt: True}).begin(x_init, kw, known_src=src, known_mask=mask)
    # the engine's own refusals, by name: the two switches, explicit noise and sampler 2 in a window with a region
    bufs = ex._buffers(2, 6)
    ks, km = ex._known_buffers(2, 6)
    win = (model._handle, 2, 6, _lib.ptr(bufs["x"]), _lib.ptr(bufs["obs_src"]), _lib.ptr(bufs["obs_mask"]), _lib.ptr(bufs["latent_mask"]),
           _lib.ptr(bufs["kinda_marg_mask"]), _lib.ptr(bufs["frame_indices"]), 0)
    tail = (1, 0.0, 1, 0, N - 1, ex.stream.cuda_stream)
    try:
        _lib.check(L.vd_set_known_region(model._handle, _lib.ptr(ks), _lib.ptr(km), None, 0, 0))
        for setter, name in ((L.vd_set_window_prefix_cache, b"window prefix cache"), (L.vd_set_window_suffix_skip, b"window suffix skip")):
            _lib.check(setter(model._handle, 1))
            rc = L.vd_window_begin(*win, 1, *tail)
            _lib.check(setter(model._handle, 0))
            assert rc != 0 and b"known region" in L.vd_last_error() and name in L.vd_last_error()
        assert L.vd_window_begin(*win, 2, *tail) != 0 and b"ddim_reverse_sample" in L.vd_last_error()
        _lib.check(L.vd_set_known_region(model._handle, _lib.ptr(ks), _lib.ptr(km), _lib.ptr(z), 0, 0))
        assert L.vd_window_begin(*win, 1, *tail) != 0 and b"known_noise must be NULL" in L.vd_last_error()
        assert L.vd_set_known_region(model._handle, _lib.ptr(ks), None, None, 0, 0) != 0 and b"together" in L.vd_last_error()
    finally:
        _lib.check(L.vd_set_known_region(model._handle, None, None, None, 0, 0))
    torch.cuda.synchronize()
    model.check_device_errors()


def test_loops():
    model, diff = tiny()
    N = diff.num_timesteps
    c = _rand_window(2, 6, 32, 2, seed=50)
    kw = _window_kw(c)
    src, mask, _ = _window_region(c, seed=51)
    shape = tuple(c["x"].shape)
    sel = torch.from_numpy(merged(_flat(mask)[0], _np(kw["latent_mask"]).reshape(2, 6))).view(shape).cuda()
    # n_resample = 1 is p_sample_loop inside the scope, draw for draw
    torch.manual_seed(52)
    got = diff.repaint_sample_loop(model, shape, src, mask, model_kwargs=dict(kw))
    torch.manual_seed(52)
    with diff.known_region_scope(model, src, mask):
        want, _ = diff.p_sample_loop(model, shape, model_kwargs=dict(kw))
    assert torch.equal(got, want) and torch.equal(got[sel], src[sel]) and torch.isfinite(got).all()
    torch.manual_seed(52)
    plain, _ = diff.p_sample_loop(model, shape, model_kwargs=dict(kw))
    assert not torch.equal(plain[sel], src[sel])
    # the progressive form yields exactly the ops of repaint_schedule
    for sampler in ("ddim", "dpmpp_2m"):
        torch.manual_seed(53)
        outs = list(diff.repaint_sample_loop_progressive(model, shape, src, mask, sampler=sampler, jump_length=2, n_resample=2,
                                                         model_kwargs=dict(kw)))
        ops = repaint_schedule(N - 1, 2, 2)
        assert [(o["op"], o["t"]) for o in outs] == ops and len(ops) == N + 2 * 2 * ((N - 1) // 2)
        assert all(("pred_xstart" in o) == (o["op"] == "step") and set(o) <= {"op", "t", "sample", "pred_xstart"} for o in outs)
        final = outs[-1]["sample"]
        assert torch.equal(final[sel], src[sel]) and torch.isfinite(final).all()
    with pytest.raises(ValueError, match="jump_length"):
        diff.repaint_sample_loop(model, shape, src, mask, jump_length=0, model_kwargs=dict(kw))
    # WindowExecutor.run_repaint: the eager walk fed the same vd_randn noise
    ex = WindowExecutor(model, diff)
    x_init = c["x"].cuda()
    for sampler, eta in (("p_sample", 0.0), ("dpmpp_2m", 0.0)):
        ex.begin(x_init, kw, sampler=sampler, eta=eta, seed=54, known_src=src, known_mask=mask)
        got = ex.run_repaint(jump_length=3, n_resample=2).clone()
        assert ex._left == 0
        want, _ = _eager_chain(model, diff, sampler, eta, x_init, kw, src, mask, 54, repaint_schedule(N - 1, 3, 2))
        assert torch.equal(got, want) and torch.equal(got[sel], src[sel]), (sampler, float((got - want).abs().max()))
        again = ex.sample_window(x_init, kw, sampler=sampler, eta=eta, seed=54, known_src=src, known_mask=mask, jump_length=3, n_resample=2)
        assert torch.equal(again, want)
    model.check_device_errors()


# ---------------------------------------------------------------------------------------------------------------- 6
def test_infer_video_and_the_job(tmp_path, monkeypatch):
    from video_diffusion_amd import video_sample as vs
    model, diff = tiny()
    g = torch.Generator().manual_seed(60)
    batch = (torch.rand(2, 10, 3, 32, 32, generator=g) * 2 - 1).cuda()
    mask = torch.rand(10, 32, 32, generator=g) < 0.5
    run = lambda **k: vs.infer_video("autoreg", model, diff, batch, 6, 2, 4, **k)[0]      # noqa: E731
    known = np.broadcast_to(mask.numpy()[None, :, None], (2, 10, 3, 32, 32))
    src = batch.cpu().numpy()
    out = {}
    for executor in ("eager", "graph"):
        torch.manual_seed(61)
        out[executor] = run(sampler="dpmpp_2m", executor=executor, known_mask=mask)
    assert np.array_equal(out["eager"], out["graph"]) and np.isfinite(out["eager"]).all()
    got = out["eager"]
    assert np.array_equal(got[:, 2:][known[:, 2:]], src[:, 2:][known[:, 2:]])   # known pixels of every generated frame: the source
    assert (got[:, 2:][~known[:, 2:]] != src[:, 2:][~known[:, 2:]]).any() and np.array_equal(got[:, :2], src[:, :2])
    torch.manual_seed(61)
    jumps = run(sampler="dpmpp_2m", executor="eager", known_mask=mask, jump_length=2, n_resample=2)
    torch.manual_seed(61)
    assert np.array_equal(jumps, run(sampler="dpmpp_2m", executor="graph", known_mask=mask, jump_length=2, n_resample=2))
    assert np.array_equal(jumps[:, 2:][known[:, 2:]], src[:, 2:][known[:, 2:]]) and not np.array_equal(jumps, got)
    # a source of its own, per item masks, stochastic samplers: the known pixels come from it
    other = -batch
    mask_b = torch.stack([mask, ~mask])
    for sampler, executor in (("p_sample", "eager"), ("ddim", "graph")):
        o = run(sampler=sampler, executor=executor, known_mask=mask_b, known_video=other, cfg_scale=1.5)
        kb = np.broadcast_to(mask_b.numpy()[:, :, None], o.shape)
        assert np.array_equal(o[:, 2:][kb[:, 2:]], -src[:, 2:][kb[:, 2:]]) and np.isfinite(o).all()
    # an all-zero mask is infer_video without the option
    zero = torch.zeros(10, 32, 32)
    for sampler, executor in (("dpmpp_2m", "graph"), ("dpmpp_2m", "eager"), ("p_sample", "eager")):
        torch.manual_seed(62)
        a = run(sampler=sampler, executor=executor, known_mask=zero)
        torch.manual_seed(62)
        assert np.array_equal(a, run(sampler=sampler, executor=executor)), (sampler, executor)
    for bad in (dict(prefix_cache=True, executor="graph"), dict(suffix_skip=True, executor="graph"), dict(use_gradient_method=True)):
        with pytest.raises(NotImplementedError, match="together with known_mask"):
            run(known_mask=mask, **bad)
    with pytest.raises(NotImplementedError, match="save_all_timesteps"):
        run(known_mask=mask, n_resample=2, save_all_timesteps=True)
    model.check_device_errors()
    # the job: --known_mask (H, W), --known_videos; the files' known pixels are to_uint8 of the source
    vids = (torch.rand(2, 8, 3, 32, 32, generator=g) * 2 - 1).numpy()
    kv = (torch.rand(2, 8, 3, 32, 32, generator=g) * 2 - 1).numpy()
    m2 = (torch.rand(32, 32, generator=g) < 0.5).numpy()
    np.save(tmp_path / "videos.npy", vids)
    np.save(tmp_path / "known.npy", kv)
    np.save(tmp_path / "mask.npy", m2.astype(np.uint8))
    monkeypatch.chdir(tmp_path)
    args = vs.build_parser().parse_args(
        ["--videos", str(tmp_path / "videos.npy"), "--inference_mode", "autoreg", "--max_frames", "6", "--obs_length", "2", "--step_size", "4",
         "--batch_size", "2", "--timestep_respacing", "logsnr5", "--image_size", "32", "--num_channels", "32", "--num_res_blocks", "1",
         "--sampler", "ddim", "--eval_dir", str(tmp_path / "out"), "--known_mask", str(tmp_path / "mask.npy"), "--known_videos",
         str(tmp_path / "known.npy"), "--jump_length", "2", "--n_resample", "2"])
    out_dir = vs.run(args, device=torch.device("cuda", 0))
    assert str(out_dir).endswith("_ddim_known_j2r2")
    for i in range(2):
        f = np.load(out_dir / "samples" / f"sample_{i:04d}-0.npy")
        assert f.dtype == np.uint8 and f.shape == (8, 3, 32, 32)
        km = np.broadcast_to(m2[None, None], f.shape)
        assert np.array_equal(f[2:][km[2:]], vs.to_uint8(kv[i])[2:][km[2:]]) and np.array_equal(f[:2], vs.to_uint8(vids[i])[:2])
        assert (f[2:][~km[2:]] != vs.to_uint8(kv[i])[2:][~km[2:]]).any()
