"""GPU: the engine across model widths, head counts, attention layouts and image sizes (tests/golden/unet_configs.npz; the cases
and the CPU oracle's share: tests/config_sweep_cases.py, licensed by tests/test_config_sweep_cpu.py).  vd_engine::build() picks the
conv kernel per layer from the width, the GroupNorm form from C / 32, the GEMM tiles, the weight packing and the concat widths from
the level widths, and the executor's prefix cache and suffix skip from where the attention layers sit: every whole-model test
elsewhere builds 32, 64 or 128 channels with 4 heads and attention at 16 and 8.

Forward: eps against the reference's strided fixture and against the oracle on every element.  Backward: eps_vjp against
torch.autograd through the oracle.  Executor: a ddim3 window against its eager replay, with the suffix skip and the prefix cache.
The other two arithmetic modes: tools/mode_check.py (test_gpu_ops.py::test_every_arithmetic_mode_end_to_end)."""
import pytest
import torch

import video_diffusion_amd as vda
from attn_temporal_restated import attn_ref
from config_sweep_cases import BACKWARD_TAGS, EXECUTOR_TAGS, REFUSED, SERVED, case, oracle, oracle_eps, oracle_kw, outside
from helpers import ATOL, RTOL, close, synth_sd
from video_diffusion_amd import _lib

pytestmark = pytest.mark.gpu
KEYS = vda.video_model_and_diffusion_defaults().keys()
_models = {}


def engine(tag, respacing=None):
    """The model of a configuration on the closed-form weights, built once per (configuration, respacing)."""
    if (tag, respacing) not in _models:
        cfg = dict(case(tag)["cfg"])
        if respacing:
            cfg["timestep_respacing"] = respacing
        model, diff = vda.create_video_model_and_diffusion(**{k: cfg[k] for k in KEYS})
        model.load_state_dict(synth_sd(model.param_specs()))
        model.to("cuda")
        model.eval()
        _models[(tag, respacing)] = (model, diff)
    return _models[(tag, respacing)]


def device_kw(c):
    return dict(frame_indices=c["frame_indices"].cuda(), x0=c["x0"].cuda(), obs_mask=c["obs_mask"].cuda(), latent_mask=c["latent_mask"].cuda(),
                kinda_marg_mask=c["kinda_marg_mask"].cuda(), x_t_minus_1=c["x0"].cuda(), observed_frames="x_0")


def test_the_cases_are_the_sweep():
    assert set(BACKWARD_TAGS) <= set(SERVED) and set(EXECUTOR_TAGS) <= set(SERVED) and len(SERVED) == 9 and len(REFUSED) == 2


@pytest.mark.parametrize("tag", SERVED)
def test_eps_matches_reference_and_oracle(tag):
    k = case(tag)
    c, s = k["c"], k["stride"]
    model, diff = engine(tag)
    eps, _ = diff._wrap_model(model)(c["x"].cuda(), k["t"].cuda(), **device_kw(c))
    model.check_device_errors()
    got = eps.cpu()
    assert got.shape == c["x"].shape and bool(torch.isfinite(got).all())
    bad_f, err_f, ratio_f = outside(got[..., ::s, ::s], k["eps"])
    bad_o, err_o, ratio_o = outside(got, oracle_eps(tag))
    print(f"CONFIG_SWEEP | {tag} | vs reference (every {s}th pixel) max |d| {err_f:.3e} = {ratio_f:.3f} of the bound | "
          f"vs oracle (every element) max |d| {err_o:.3e} = {ratio_o:.3f} of the bound | |eps| up to {float(k['eps'].abs().max()):.2f}")
    assert bad_f == 0 and bad_o == 0, (tag, bad_f, err_f, bad_o, err_o)


@pytest.mark.parametrize("tag", BACKWARD_TAGS)
def test_eps_vjp_matches_oracle_autograd(tag):
    """A seeded Gaussian cotangent at t = 120 of ddim250, as test_gpu_ode_nll.py::test_eps_vjp_against_oracle_autograd and at its bars:
    atol = 2e-4 max|want|, rtol = 1e-3; eps at ATOL / RTOL; the observed frame's rows exactly zero."""
    k = case(tag)
    c = k["c"]
    model, diff = engine(tag)
    ora = oracle(tag)
    cot = torch.randn(c["x"].shape, generator=torch.Generator().manual_seed(41))
    x = c["x"].detach().clone().requires_grad_(True)
    tm = torch.tensor(ora.s.timestep_map, dtype=torch.long)[k["t"]]
    with torch.enable_grad():
        eps_want = ora.net.with_grad(x, tm, **oracle_kw(c))
        want, = torch.autograd.grad((eps_want * cot).sum(), x)
    out = diff.eps_vjp(model, c["x"].cuda(), k["t"].cuda(), cot.cuda(), device_kw(c))
    model.check_device_errors()
    scale = float(want.abs().max())
    err = (out["vjp"].cpu() - want).abs()
    print(f"CONFIG_SWEEP_VJP | {tag} | max |vjp - ref| = {float(err.max()):.3e} = {float(err.max()) / scale:.3e} max |ref| | "
          f"eps {float((out['eps'].cpu() - eps_want.detach()).abs().max()):.3e}")
    assert scale > 0 and not out["vjp"][:, :1].any() and not want[:, :1].any()        # the observed frame is a constant
    close(out["vjp"].cpu(), want, atol=2e-4 * scale, rtol=1e-3)
    close(out["eps"].cpu(), eps_want.detach(), atol=ATOL, rtol=RTOL)


@pytest.mark.parametrize("tag", EXECUTOR_TAGS)
def test_window_executor_equals_eager_and_its_shortcuts_keep_the_read_frames(tag):
    """timestep_respacing="ddim3".  (a) A whole window through the graph executor equals the eager vd_p_sample steps with the same
    counter-based noise, bit for bit (test_gpu_engine.py::test_window_executor_equals_eager_steps_bit_for_bit).  (b) suffix_skip
    leaves every frame that is not a pure observation bit-identical.  (c) With the prefix cache as well, within the 2e-6 + 2e-6 |ref|
    of test_window_executor_40_frames_suffix_skip_and_prefix_cache_vs_eager (GroupNorm sums folded in another fp64 grouping).
    (d) suffix_frames and cached_frames are the counts the masks imply: B x 2 latent frames, B x 1 observed frame."""
    from video_diffusion_amd.executor import WindowExecutor
    c = case(tag)["c"]
    model, diff = engine(tag, "ddim3")
    diff._bind(model)
    assert diff.num_timesteps == 3
    L = _lib.lib()
    kw = device_kw(c)
    B, T = c["x"].shape[:2]
    x_init = c["x"].cuda().clone()
    seed = 9600
    want = WindowExecutor(model, diff).begin(x_init, kw, seed=seed).run().clone()
    assert bool(torch.isfinite(want).all())
    # (a) the eager replay
    cur, per = x_init.clone(), x_init[0].numel()
    pk = model._pack_kwargs(cur, kw)
    for step, ti in enumerate(range(diff.num_timesteps)[::-1]):
        t = torch.full((B,), ti, dtype=torch.int64, device="cuda")
        nxt = torch.empty_like(cur)
        _lib.check(L.vd_p_sample(model._handle, B, T, _lib.ptr(cur), _lib.ptr(pk["obs_src"]), _lib.ptr(pk["obs_mask"]), _lib.ptr(pk["latent_mask"]),
                                 _lib.ptr(pk["kinda_marg_mask"]), _lib.ptr(pk["frame_indices"]), _lib.ptr(t), pk["obs_mode"], 1, None, seed,
                                 step * B * per, _lib.ptr(nxt), None, None, _lib.current_stream()))
        cur = nxt
    assert torch.equal(cur, want), float((cur - want).abs().max())
    # (b) - (d)
    read = ~((c["obs_mask"].reshape(B, T) == 1) & (c["latent_mask"].reshape(B, T) == 0))
    assert int(read.sum()) == B * (T - 1)
    skip, both = WindowExecutor(model, diff, suffix_skip=True), WindowExecutor(model, diff, prefix_cache=True, suffix_skip=True)
    skip.begin(x_init, kw, seed=seed)
    assert skip.suffix_frames == int(read.sum()) and skip.cached_frames == 0
    got = skip.run().clone().cpu()
    assert torch.equal(got[read], want.cpu()[read])
    assert not torch.equal(got[~read], want.cpu()[~read])                             # really skipped
    both.begin(x_init, kw, seed=seed)
    assert both.suffix_frames == int(read.sum()) and both.cached_frames == int((~read).sum()) == B
    got2 = both.run().clone().cpu()
    bad, err, ratio = outside(got2[read], want.cpu()[read], atol=2e-6, rtol=2e-6)
    print(f"CONFIG_SWEEP_EXECUTOR | {tag} | prefix cache + suffix skip vs plain max |d| {err:.3e} = {ratio:.3f} of the bound")
    assert bad == 0, (bad, err)
    model.check_device_errors()


def test_forward_has_no_token_ceiling_and_the_backward_names_its_own():
    """attention_resolutions="64,16" at 64 x 64: 4096 tokens per frame at the first level.  vd_create accepts it, the forward serves it
    (eps against the oracle on every element; the oracle's weights take the engine's names and shapes, which the reference has not
    seen for this configuration); the backward-data pass serves 1024 tokens, refuses by name, and the model serves a forward afterwards.
    One item and its first two frames of the 64 x 64 window: the oracle's 4096 x 4096 score matrices are 0.5 GB per tensor even so."""
    from oracle.unet_ref import UNetRef
    from config_sweep_cases import sampler
    k = dict(case("w64_att32_s64"))
    c = {name: v[:1, :2].contiguous() for name, v in k["c"].items()}
    k["t"] = k["t"][:1]
    cfg = dict(k["cfg"], attention_resolutions="64,16")
    model, diff = vda.create_video_model_and_diffusion(**{key: cfg[key] for key in KEYS})
    sd = synth_sd(model.param_specs())
    model.load_state_dict(sd)
    model.to("cuda")
    model.eval()
    want = sampler(cfg, UNetRef(cfg, sd)).eps(c["x"], k["t"], oracle_kw(c))
    eps, _ = diff._wrap_model(model)(c["x"].cuda(), k["t"].cuda(), **device_kw(c))
    model.check_device_errors()
    bad, err, ratio = outside(eps.cpu(), want)
    print(f"CONFIG_SWEEP | 4096 tokens | vs oracle (every element) max |d| {err:.3e} = {ratio:.3f} of the bound")
    assert bad == 0, (bad, err)
    with pytest.raises(_lib.VdError, match=r"spatial attention backward.*L <= 1024"):
        diff.eps_vjp(model, c["x"].cuda(), k["t"].cuda(), torch.ones_like(c["x"]).cuda(), device_kw(c))
    again, _ = diff._wrap_model(model)(c["x"].cuda(), k["t"].cuda(), **device_kw(c))
    model.check_device_errors()
    assert torch.equal(again, eps)


def test_temporal_ceiling_stays_at_the_forward_and_names_the_head_dim():
    """The temporal attention's LDS ceiling moves with T, so it is checked where T is known.  No model that vd_create accepts reaches
    it (the spatial attention stops at head dim 128, the ceiling at T = 32 is 272): the operator is asked directly.  Head dim 280
    at T = 32 is refused by name, nothing is written, and the same width at T = 16 is served, against the fp64 restatement."""
    B, HW, C, heads = 1, 3, 280, 1
    g = torch.Generator().manual_seed(280)
    qkv32 = torch.randn(B, 32, HW, 3 * C, generator=g).cuda()
    out = torch.full((B, 32, HW, C), -7.25e30, device="cuda")
    rc = _lib.lib().vd_op_attn_temporal(_lib.ptr(qkv32), None, None, None, None, B, 32, HW, C, heads, 0, _lib.ptr(out), _lib.current_stream())
    torch.cuda.synchronize()
    with pytest.raises(_lib.VdError, match=r"temporal attention: head dim too large.*head dim 280 .*T = 32"):
        _lib.check(rc)
    assert bool((out == -7.25e30).all())
    qkv16 = qkv32[:, :16].contiguous()
    got = torch.full((B, 16, HW, C), float("nan"), device="cuda")
    _lib.check(_lib.lib().vd_op_attn_temporal(_lib.ptr(qkv16), None, None, None, None, B, 16, HW, C, heads, 0, _lib.ptr(got), _lib.current_stream()))
    torch.cuda.synchronize()
    ref = attn_ref(qkv16.cpu(), None, None, None, None, 0, B, 16, HW, C, heads)
    close(got.cpu(), ref.float(), atol=ATOL, rtol=RTOL)
