"""GPU: windows of 33..128 frames (vd_max_window_frames).  The long-window temporal attention (csrc/attn_temporal_long.hip),
the long form of the temporal GroupNorm and of the attention-weights maps, and every caller of the forward at such a window,
against an fp64 statement of the operator, the CPU oracle, and golden vectors of the imported reference."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import video_diffusion_amd as vda
from attn_temporal_restated import attn_ref
from helpers import close, load_npz, synth_sd
from oracle.sampler_ref import SamplerRef
from oracle.schedule_ref import ScheduleRef
from oracle.unet_ref import UNetRef
from video_diffusion_amd import _lib

pytestmark = pytest.mark.gpu
TOL = dict(atol=1e-4, rtol=1e-4)
KEYS = vda.video_model_and_diffusion_defaults().keys()
_cache = {}


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def dev(t):
    return t.to("cuda").contiguous()


def engine(cfg):
    key = json.dumps(cfg, sort_keys=True)
    if key not in _cache:
        model, diff = vda.create_video_model_and_diffusion(**{k: cfg[k] for k in KEYS})
        model.load_state_dict(synth_sd(model.param_specs()))
        model.to("cuda")
        model.eval()
        _cache[key] = (model, diff)
    return _cache[key]


def oracle(cfg):
    model, diff = engine(cfg)
    net = UNetRef(cfg, synth_sd(model.param_specs()))
    sched = ScheduleRef(cfg["diffusion_steps"], cfg["noise_schedule"], cfg["timestep_respacing"], cfg["sigma_small"],
                        cfg["rescale_timesteps"])
    return model, diff, SamplerRef(sched, net)


def kwargs_of(c, observed_frames="x_0"):
    return dict(frame_indices=c["frame_indices"].cuda(), x0=c["x0"].cuda(), obs_mask=c["obs_mask"].cuda(),
                latent_mask=c["latent_mask"].cuda(), kinda_marg_mask=c["kinda_marg_mask"].cuda(),
                x_t_minus_1=c["x0"].cuda(), observed_frames=observed_frames)


def rand_window(B, T, S, n_obs, seed, n_pad=0):
    """n_obs observed frames, then latent frames, then n_pad padding frames that are in none of the masks."""
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(B, T, 3, S, S, generator=g) * 2 - 1
    x0[:, n_obs:] = 0
    x = torch.randn(B, T, 3, S, S, generator=g)
    obs = torch.zeros(B, T, 1, 1, 1)
    obs[:, :n_obs] = 1
    lat = 1 - obs
    if n_pad:
        lat[:, T - n_pad:] = 0
    return dict(x=x, x0=x0, obs_mask=obs, latent_mask=lat, kinda_marg_mask=torch.zeros(B, T, 1, 1, 1),
                frame_indices=torch.arange(T).view(1, T).repeat(B, 1))


def tiny_cfg(T, **over):
    return {**vda.video_model_and_diffusion_defaults(), **dict(T=T, image_size=32, num_channels=32, num_res_blocks=1,
                                                               rp_alpha=T, rp_beta=T, rp_gamma=T, timestep_respacing="ddim250"),
            **over}


def test_max_window_frames_is_128():
    assert _lib.lib().vd_max_window_frames() == 128


# ---------------------------------------------------------------------------------------------------- the operator
# (B, T, HW, C, heads, rpe, mask, allow, hot): head dims 16, 32, 64, 96, 128 and 24 (a multiple of 8, not of 16); pixel
# counts divisible by 16 (matrix-pipe kernel) and ragged (generic kernel); mask "half": every other frame of item 0 and the
# middle frame are padding; "pad16": the last 20 frames are padding, so whole 16-key tiles are masked for the real rows;
# hot: one key's logits x40 (the online softmax's rescale).
CASES = [
    (2, 33, 16, 64, 4, True, "half", 1, False),
    (2, 40, 32, 128, 4, True, "pad16", 0, False),
    (1, 48, 16, 192, 2, True, "pad16", 1, False),
    (2, 64, 32, 256, 2, True, None, 0, True),
    (1, 97, 16, 128, 4, True, "pad16", 0, True),
    (2, 128, 16, 192, 2, True, "half", 0, False),
    (1, 128, 16, 256, 2, False, "pad16", 0, True),
    (2, 48, 48, 96, 1, False, None, 0, False),
    (2, 40, 16, 64, 2, False, "half", 1, True),
    (2, 64, 16, 128, 8, True, "pad16", 1, False),
    (2, 40, 10, 48, 2, True, "pad16", 0, False),
    (1, 64, 21, 96, 4, True, "half", 1, True),
    (2, 33, 7, 128, 1, True, None, 0, False),
    (1, 128, 5, 64, 2, False, "pad16", 0, False),
    (2, 97, 16, 160, 1, True, "half", 0, False),
]


@pytest.mark.parametrize("B,T,HW,C,heads,rpe,mask,allow,hot", CASES)
def test_attention_temporal_long(B, T, HW, C, heads, rpe, mask, allow, hot):
    qkv = rnd(B, T, HW, 3 * C, seed=T) * 1.5
    if hot:
        qkv[:, T // 3, :, C:2 * C] *= 40.0                         # one key frame with logits x40
    Rk, Rq, Rv = (rnd(B, T, T, C, seed=s) for s in (1, 2, 3))
    m = None
    if mask == "half":
        m = torch.ones(B, T)
        m[:, T // 2] = 0
        m[0, ::2] = 0
    elif mask == "pad16":
        m = torch.ones(B, T)
        m[:, T - 20:] = 0
    out = torch.empty(B, T, HW, C, device="cuda")
    bufs = [dev(qkv)] + [dev(r) if rpe else None for r in (Rk, Rq, Rv)] + [dev(m) if m is not None else None]
    _lib.check(_lib.lib().vd_op_attn_temporal(*[_lib.ptr(b) for b in bufs], B, T, HW, C, heads, allow, _lib.ptr(out),
                                              _lib.current_stream()))
    torch.cuda.synchronize()
    ref = attn_ref(qkv, *(Rk, Rq, Rv) if rpe else (None, None, None), m, allow, B, T, HW, C, heads)
    got = out.cpu()
    assert torch.isfinite(got).all()
    close(got, ref.float(), **TOL)
    if B > 1:                                                        # the last item on its own: the same bits
        one = torch.empty(1, T, HW, C, device="cuda")
        b1 = [bufs[0][B - 1:].contiguous()] + [None if r is None else r[B - 1:].contiguous() for r in bufs[1:]]
        _lib.check(_lib.lib().vd_op_attn_temporal(*[_lib.ptr(b) for b in b1], 1, T, HW, C, heads, allow, _lib.ptr(one),
                                                  _lib.current_stream()))
        torch.cuda.synchronize()
        assert torch.equal(one[0], out[B - 1])


def test_attention_temporal_above_the_bound_is_refused():
    B, T, HW, C = 1, 129, 16, 64
    qkv = torch.zeros(B, T, HW, 3 * C, device="cuda")
    out = torch.empty(B, T, HW, C, device="cuda")
    with pytest.raises(_lib.VdError, match="128"):
        _lib.check(_lib.lib().vd_op_attn_temporal(_lib.ptr(qkv), None, None, None, None, B, T, HW, C, 2, 0, _lib.ptr(out),
                                                  _lib.current_stream()))


@pytest.mark.parametrize("B,T,HW,C,mean", [(2, 33, 20, 128, 0.0), (1, 64, 17, 512, 0.0), (2, 128, 9, 256, 0.0),
                                           (1, 128, 12, 64, 0.0), (1, 64, 8, 384, 30.0), (2, 40, 5, 32, 0.0)])
def test_gn_temporal_long(B, T, HW, C, mean):
    """GroupNorm32 on the (B*HW, C, T) view (unet.py:472-475) at 33..128 frames; C = 32 and 64 take the per-channel
    partials (channels per group not a multiple of 4); mean 30: the fp64 statistics keep the variance (E[x^2] - mean^2 = 901 - 900)."""
    x = rnd(B, T, HW, C, seed=T + C) + mean
    gamma, beta = rnd(C, seed=1) + 1, rnd(C, seed=2)
    y = torch.empty(B, T, HW, C, device="cuda")
    bufs = [dev(x), dev(gamma), dev(beta)]
    _lib.check(_lib.lib().vd_op_gn_temporal(_lib.ptr(bufs[0]), _lib.ptr(bufs[1]), _lib.ptr(bufs[2]), B, T, HW, C,
                                            _lib.ptr(y), _lib.current_stream()))
    torch.cuda.synchronize()
    ref = F.group_norm(x.double().permute(0, 2, 3, 1).reshape(B * HW, C, T), 32, gamma.double(), beta.double(), eps=1e-5)
    close(y.cpu(), ref.view(B, HW, C, T).permute(0, 3, 1, 2).float(), atol=2e-5, rtol=2e-5)


# ---------------------------------------------------------------------------------------------------- the engine
def golden_window(rec):
    """x, model kwargs and t of the fixture's shared window (int8 codes, exact in fp32)."""
    x = torch.from_numpy(rec["x_q"]).float() / 32
    c = dict(x0=torch.from_numpy(rec["x0_q"]).float() / 127, obs_mask=torch.from_numpy(rec["obs_mask"]),
             latent_mask=torch.from_numpy(rec["latent_mask"]), kinda_marg_mask=torch.from_numpy(rec["kinda_marg_mask"]),
             frame_indices=torch.from_numpy(rec["frame_indices"]))
    return x, c, torch.from_numpy(rec["t"])


@pytest.mark.parametrize("case", ["rpe", "nopad", "table"])
def test_eps_matches_reference_golden_long(case):
    """unet_tiny_long.npz (tools/golden/long_window.py: unet_tiny_long): T = 48, B = 2, 8 padding frames in no mask; RPE nets with both
    padding rules, and the bucket tables."""
    rec = load_npz("unet_tiny_long.npz")
    cfg = json.loads(str(rec[f"{case}_cfg_json"]))
    model, diff = engine(cfg)
    x, c, t = golden_window(rec)
    got, _ = diff._wrap_model(model)(x.cuda(), t.cuda(), **kwargs_of(c))
    close(got[..., ::4, ::4].cpu(), rec[f"{case}_eps"], **TOL)


@pytest.mark.parametrize("B,T,n_obs,n_pad", [(2, 40, 10, 0), (1, 128, 32, 20)])
def test_tiny_model_long_windows_vs_oracle(B, T, n_obs, n_pad):
    cfg = tiny_cfg(T)
    model, diff, ora = oracle(cfg)
    c = rand_window(B, T, 32, n_obs, seed=T, n_pad=n_pad)
    c["frame_indices"] = (c["frame_indices"] * 3 + 1) % (2 * T + 1)
    t = torch.tensor([60] * B)
    kw = {k: v for k, v in c.items() if k != "x"}
    want = ora.eps(c["x"], t, kw)
    got, _ = diff._wrap_model(model)(c["x"].cuda(), t.cuda(), **kwargs_of(c))
    close(got.cpu(), want, **TOL)


def test_default_model_48_frames_vs_oracle():
    """Default 64x64 model (116 M parameters), one clip of 48 frames: the head dims 96 and 128 of the production attention
    levels on the long-window matrix-pipe kernel."""
    cfg = {**vda.video_model_and_diffusion_defaults(), **dict(T=48, image_size=64, rp_alpha=48, rp_beta=48, rp_gamma=48,
                                                              timestep_respacing="ddim250")}
    model, diff, ora = oracle(cfg)
    c = rand_window(1, 48, 64, 16, seed=48)
    t = torch.tensor([200])
    kw = {k: v for k, v in c.items() if k != "x"}
    want = ora.eps(c["x"], t, kw)
    got, _ = diff._wrap_model(model)(c["x"].cuda(), t.cuda(), **kwargs_of(c))
    close(got.cpu(), want, **TOL)


def test_return_attn_weights_48_frames_matches_reference_golden():
    """return_attn_weights at T = 48: the temporal maps (B*HW, T, T), head-averaged softmax weights, on the chunked long
    form of the maps kernel; the fixture holds every STRIDE-th map.  Softmax weights are in [0, 1]: 2e-5 absolute."""
    rec = load_npz("unet_tiny_long.npz")
    cfg = json.loads(str(rec["rpe_cfg_json"]))
    model, diff = engine(cfg)
    x, c, t = golden_window(rec)
    eps, attn = diff._wrap_model(model)(x.cuda(), t.cuda(), return_attn_weights=True, **kwargs_of(c))
    maps = attn["temporal"]
    assert len(maps) == int(rec["attn_n_temporal"])
    stride = int(rec["stride"])
    for i, m in enumerate(maps):
        assert tuple(m.shape) == tuple(rec[f"attn_temporal_{i}_shape"])
        close(m[::stride].cpu(), rec[f"attn_temporal_{i}"], atol=2e-5, rtol=1e-4)
        assert abs(float(m.sum(-1).mean()) - 1.0) < 1e-4
    close(eps[..., ::4, ::4].cpu(), rec["rpe_eps"], **TOL)


# ---------------------------------------------------------------------------------------------------- the callers
def test_infer_video_autoreg_max_frames_40_vs_oracle(monkeypatch):
    """scripts/video_sample.py:50-190 with --max_frames 40: a 56-frame video in autoregressive windows of 40 frames, against
    the same loop on the CPU oracle with the identical noise draws."""
    from video_diffusion_amd import gaussian_diffusion as gdm
    from video_diffusion_amd import inference_util as iu
    from video_diffusion_amd.video_sample import get_masks, infer_video
    cfg = tiny_cfg(40, timestep_respacing="ddim3")
    model, diff, ora = oracle(cfg)
    B, T, obs_len, max_frames, step = 1, 56, 24, 40, 16
    g = torch.Generator().manual_seed(5)
    batch = torch.rand(B, T, 3, 32, 32, generator=g) * 2 - 1
    draws = []
    gen = torch.Generator().manual_seed(77)

    def fake_randn_like(x, *a, **k):
        z = torch.randn(x.shape, generator=gen)
        draws.append(z)
        return z.to(x.device)

    monkeypatch.setattr(gdm.th, "randn_like", fake_randn_like)
    got, _ = infer_video("autoreg", model, diff, batch.cuda(), max_frames, obs_len, step, executor="eager")
    monkeypatch.undo()

    samples = torch.zeros_like(batch)
    samples[:, :obs_len] = batch[:, :obs_len]
    it, k = iter(draws), 0
    for obs_idx, lat_idx in iu.inference_strategies["autoreg"](video_length=T, num_obs=obs_len, max_frames=max_frames,
                                                                step_size=step):
        x0 = torch.cat([samples[:, obs_idx], samples[:, lat_idx]], dim=1).clone()
        fi = torch.tensor(obs_idx + lat_idx).repeat(B, 1)
        om, lm, km = get_masks(x0, len(obs_idx))
        kw = dict(x0=x0, obs_mask=om, latent_mask=lm, kinda_marg_mask=km, frame_indices=fi)
        local = x0.clone()
        for ts in range(diff.num_timesteps)[::-1]:
            local = ora.p_sample(local, torch.tensor([ts] * B), kw, next(it))["sample"]
        samples[:, lat_idx] = local[:, -len(lat_idx):]
        k += 1
        assert x0.shape[1] > 32                                       # every window is a long one
    assert len(draws) == k * diff.num_timesteps and k >= 2
    err = np.abs(got - samples.numpy())
    assert err.mean() < 2e-4, err.mean()
    close(got, samples.numpy(), atol=3e-2, rtol=1e-2)
    assert np.array_equal(got[:, :obs_len], batch[:, :obs_len].numpy())


def test_window_executor_40_frames_suffix_skip_and_prefix_cache_vs_eager():
    """The graph executor at T = 40: with suffix_skip every frame the caller reads is bit-identical to the plain executor's;
    with the prefix cache as well, equal up to the fp64 regrouping of the GroupNorm sums."""
    from video_diffusion_amd.executor import WindowExecutor
    cfg = tiny_cfg(40, num_channels=64, timestep_respacing="ddim4")
    model, diff = engine(cfg)
    plain, skip, both = WindowExecutor(model, diff), WindowExecutor(model, diff, suffix_skip=True), \
        WindowExecutor(model, diff, prefix_cache=True, suffix_skip=True)
    B, T, n_obs = 2, 40, 12
    c = rand_window(B, T, 32, n_obs, seed=40)
    read = ~((c["obs_mask"].reshape(B, T) == 1) & (c["latent_mask"].reshape(B, T) == 0))
    kw = kwargs_of(c)
    x_init = c["x"].cuda().clone()
    want = plain.begin(x_init, kw, seed=4040).run().clone().cpu()
    assert torch.isfinite(want).all()
    skip.begin(x_init, kw, seed=4040)
    assert skip.suffix_frames == int(read.sum())
    got = skip.run().clone().cpu()
    assert torch.equal(got[read], want[read])
    both.begin(x_init, kw, seed=4040)
    got2 = both.run().clone().cpu()
    close(got2[read], want[read], atol=2e-6, rtol=2e-6)
    assert not torch.equal(got[~read], want[~read])                    # really skipped
    model.check_device_errors()


def test_use_gradient_method_stays_at_32_frames():
    cfg = tiny_cfg(40, num_channels=64)
    model, diff = engine(cfg)
    B, T = 1, 40
    c = rand_window(B, T, 32, 8, seed=41)
    kw = kwargs_of(c)
    x = c["x"].cuda()
    t = torch.tensor([100] * B, device="cuda")
    with pytest.raises(_lib.VdError, match=r"use_gradient_method.*32"):
        diff.p_sample(model, x, t, model_kwargs=kw, use_gradient_method=True)
    # the engine still serves a 40-frame forward afterwards
    eps, _ = diff._wrap_model(model)(x, t, **kw)
    assert torch.isfinite(eps).all() and eps.shape == x.shape
    with pytest.raises(_lib.VdError, match="128"):
        big = rand_window(1, 129, 32, 8, seed=42)
        diff._wrap_model(model)(big["x"].cuda(), t, **kwargs_of(big))
