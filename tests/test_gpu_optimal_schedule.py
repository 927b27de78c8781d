"""GPU: the scoring path of the observed-frame search -- the eps-mse kernel alone (vd_op_eps_mse) against a float64 restatement,
the whole entry (GaussianDiffusion.score_windows -> vd_score_windows) against the CPU oracle, the suffix skip against the full
forward, and the job (video_optimal_schedule.run) against the oracle at every pick, resumed, and read back by video_sample.

The bar is the NLL tests' own (test_gpu_engine: atol 2e-5, rtol 1e-3 on per-item means)."""
import json
from argparse import ArgumentParser

import numpy as np
import pytest
import torch

import video_diffusion_amd as vda
from helpers import close, synth_sd
from oracle.losses_ref import mean_flat
from oracle.sampler_ref import SamplerRef, _coef
from oracle.schedule_ref import ScheduleRef
from oracle.unet_ref import UNetRef
from video_diffusion_amd import _lib
from video_diffusion_amd import video_optimal_schedule as vos

pytestmark = pytest.mark.gpu
KEYS = vda.video_model_and_diffusion_defaults().keys()
ATOL, RTOL = 2e-5, 1e-3
S = 32
_cache = {}


def config(T, num_channels=32, respacing="ddim10", **over):
    return {**vda.video_model_and_diffusion_defaults(), **dict(T=T, image_size=S, num_channels=num_channels, num_res_blocks=1,
                                                               rp_alpha=T, rp_beta=T, rp_gamma=T, timestep_respacing=respacing), **over}


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
    key = "oracle" + json.dumps(cfg, sort_keys=True)
    if key not in _cache:
        model, _ = engine(cfg)
        sched = ScheduleRef(cfg["diffusion_steps"], cfg["noise_schedule"], cfg["timestep_respacing"], cfg["sigma_small"],
                            cfg["rescale_timesteps"])
        _cache[key] = SamplerRef(sched, UNetRef(cfg, synth_sd(model.param_specs())))
    return _cache[key]


def philox_noise(shape, seed, offsets):
    """What the engine draws for a batch: item b = vd_randn(per, seed, offsets[b])."""
    out = torch.empty(shape, device="cuda")
    per = out[0].numel()
    for b, off in enumerate(offsets):
        _lib.check(_lib.lib().vd_randn(_lib.ptr(out[b]), per, seed, int(off), _lib.current_stream()))
    torch.cuda.synchronize()
    return out


def window(B, T, obs_sets, lat_sets, seed):
    """x_start uniform in [-1, 1] and the masks of a ragged batch: frames in neither set are padding."""
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(B, T, 3, S, S, generator=g) * 2 - 1
    obs, lat = torch.zeros(B, T, 1, 1, 1), torch.zeros(B, T, 1, 1, 1)
    for b in range(B):
        obs[b, list(obs_sets[b])] = 1
        lat[b, list(lat_sets[b])] = 1
    x0 = x0 * (obs + lat)                                          # padding frames are zeros (video_nll.run_bpd_evaluation)
    fidx = torch.stack([torch.randperm(3 * T, generator=g)[:T].sort().values for _ in range(B)]) * (obs + lat).view(B, T).long()
    return x0, dict(frame_indices=fidx, obs_mask=obs, latent_mask=lat, kinda_marg_mask=torch.zeros(B, T, 1, 1, 1))


def on_gpu(kw):
    return {k: v.cuda() for k, v in kw.items()}


# ------------------------------------------------------------------------------------------------ the kernel alone
def eps_mse(model, diff, x0, eps, t, lat, clip, seed, offsets, noise=None):
    diff._bind(model)
    B, T = x0.shape[:2]
    out = torch.empty(B, dtype=torch.float64, device="cuda")
    off = torch.tensor(offsets, dtype=torch.int64, device="cuda")
    args = [x0.cuda().contiguous(), eps.cuda().contiguous(), t.cuda(), lat.reshape(B * T).cuda().contiguous()]
    nz = None if noise is None else noise.cuda().contiguous()
    _lib.check(_lib.lib().vd_op_eps_mse(model._handle, B, T, _lib.ptr(args[0]), _lib.ptr(args[1]), _lib.ptr(args[2]), int(clip),
                                        _lib.ptr(args[3]), seed, _lib.ptr(off), _lib.ptr(nz), _lib.ptr(out), _lib.current_stream()))
    torch.cuda.synchronize()
    return out.cpu()


def mse_restated(diff, x0, eps, z, t, lat, clip, start_x):
    """calc_bpd_loop_subsampled's `mse` (gaussian_diffusion.py:975-990) in float64 on the fp32 inputs; the coefficients are the
    float32 casts _extract_into_tensor hands the arithmetic."""
    def c(tab):
        return torch.from_numpy(np.asarray(tab)[t.numpy()].astype(np.float32)).double().view(-1, 1, 1, 1, 1)
    x0, eps, z = x0.double(), eps.double(), z.double()
    xt = c(diff.sqrt_alphas_cumprod) * x0 + c(diff.sqrt_one_minus_alphas_cumprod) * z
    sr, srm1 = c(diff.sqrt_recip_alphas_cumprod), c(diff.sqrt_recipm1_alphas_cumprod)
    pred = eps if start_x else sr * xt - srm1 * eps
    if clip:
        pred = pred.clamp(-1, 1)
    e = (sr * xt - pred) / srm1
    return mean_flat((e - z) ** 2, lat.double())


# (B, T, t, latent sets): one block per item; per-item t = 0 / mid / last with different latent sets, padding, an item with no
# latent frame; T = 33 (25 blocks per item)
KERNEL_SHAPES = {
    "1x1": (1, 1, [4], [{0}]),
    "3x6": (3, 6, [0, 5, 9], [{2, 3, 4, 5}, {1, 4}, set()]),
    "1x33": (1, 33, [7], [set(range(5, 33))]),
}


@pytest.mark.parametrize("clip,start_x", [(1, 0), (0, 0), (1, 1)])
@pytest.mark.parametrize("shape", sorted(KERNEL_SHAPES))
def test_eps_mse_kernel_vs_float64(shape, clip, start_x):
    B, T, t, lats = KERNEL_SHAPES[shape]
    cfg = config(4, predict_xstart=bool(start_x))
    model, _ = engine(config(4))
    diff = engine(cfg)[1] if start_x else engine(config(4))[1]
    g = torch.Generator().manual_seed(100 + B * T)
    x0 = torch.rand(B, T, 3, S, S, generator=g) * 2 - 1
    eps = torch.randn(B, T, 3, S, S, generator=g) * (0.6 if start_x else 1.0)
    lat = torch.zeros(B, T, 1, 1, 1)
    for b in range(B):
        lat[b, list(lats[b])] = 1
    t = torch.tensor(t)
    seed, offsets = 1234, [11 + 100000 * b for b in range(B)]
    z = philox_noise(x0.shape, seed, offsets).cpu()
    got = eps_mse(model, diff, x0, eps, t, lat, clip, seed, offsets)
    want = mse_restated(diff, x0, eps, z, t, lat, clip, start_x)
    print(f"\nERR eps_mse {shape} clip={clip} start_x={start_x} got {got.tolist()} max|d| {(got - want).abs().max():.3e}")
    close(got, want, atol=ATOL, rtol=RTOL)
    assert torch.equal(got, eps_mse(model, diff, x0, eps, t, lat, clip, seed, offsets, noise=z))      # given noise = the Philox draw
    assert torch.equal(got, eps_mse(model, diff, x0, eps, t, lat, clip, seed, offsets))                # deterministic
    for b in range(B):
        if not lats[b]:
            assert got[b].item() == 0.0
        else:
            assert got[b].item() > 0.0
    model.check_device_errors()
    engine(config(4))[1]._bind(model)


def test_eps_mse_kernel_flags():
    model, diff = engine(config(4))
    B, T = 2, 3
    g = torch.Generator().manual_seed(5)
    x0 = torch.rand(B, T, 3, S, S, generator=g) * 2 - 1
    eps = torch.randn(B, T, 3, S, S, generator=g)
    lat = torch.zeros(B, T, 1, 1, 1)
    lat[:, 1:] = 1
    model.check_device_errors()
    bad = eps.clone()
    bad[1, 2, 0, 3, 3] = float("inf")
    got = eps_mse(model, diff, x0, bad, torch.tensor([3, 3]), lat, 1, 7, [0, 50000])
    assert torch.isfinite(got[0]) and not torch.isfinite(got[1])
    with pytest.raises(FloatingPointError):
        model.check_device_errors()
    bad = eps.clone()
    bad[0, 0, 0, 0, 0] = float("inf")                              # frame 0 is not latent: never read, no flag
    assert torch.isfinite(eps_mse(model, diff, x0, bad, torch.tensor([3, 3]), lat, 1, 7, [0, 50000])).all()
    model.check_device_errors()
    got = eps_mse(model, diff, x0, eps, torch.tensor([3, diff.num_timesteps]), lat, 1, 7, [0, 50000])
    assert torch.isfinite(got[0]) and torch.isnan(got[1])
    with pytest.raises(IndexError):
        model.check_device_errors()
    model.check_device_errors()                                    # the flags are cleared by the read


# ------------------------------------------------------------------------------------------------ the whole entry
def oracle_scores(ora, x0, t, kw, noise):
    """SamplerRef.q_sample + mean_variance + the oracle's mse expression (calc_bpd_loop_subsampled)."""
    s = ora.s
    x_t = ora.q_sample(x0, t, noise)
    pred = ora.mean_variance(x_t, t, dict(kw, x0=x0), clip=True)["pred_xstart"]
    e = (_coef(s.sqrt_recip_alphas_cumprod, t, x_t) * x_t - pred) / _coef(s.sqrt_recipm1_alphas_cumprod, t, x_t)
    return mean_flat((e - noise) ** 2, kw["latent_mask"])


# B = 2 x T = 6 (ragged: padding in item 1) and one window of 33 frames (the long-window kernels)
ENTRY_CASES = {
    "2x6": (6, 2, 6, [{0, 1}, {0, 1, 2}], [{2, 3, 4, 5}, {3, 4}], [9, 2]),
    "1x33": (33, 1, 33, [set(range(5))], [set(range(5, 33))], [6]),
}


def entry_case(name):
    if ("entry", name) not in _cache:
        Tm, B, T, obs, lat, t = ENTRY_CASES[name]
        cfg = config(Tm)
        model, diff = engine(cfg)
        x0, kw = window(B, T, obs, lat, seed=40 + T)
        seed, offsets = 99, [3 + 200000 * b for b in range(B)]
        noise = philox_noise(x0.shape, seed, offsets)
        want = oracle_scores(oracle(cfg), x0, torch.tensor(t), kw, noise.cpu())
        _cache[("entry", name)] = (model, diff, x0, kw, torch.tensor(t), seed, offsets, noise, want)
    return _cache[("entry", name)]


@pytest.mark.parametrize("name", sorted(ENTRY_CASES))
def test_score_windows_vs_oracle(name):
    model, diff, x0, kw, t, seed, offsets, noise, want = entry_case(name)
    got = diff.score_windows(model, x0.cuda(), t.cuda(), on_gpu(kw), None, seed, offsets, suffix_skip=False)
    assert got.dtype == torch.float64 and got.shape == (x0.shape[0],)
    print(f"\nERR score_windows {name} got {got.tolist()} want {want.tolist()}")
    close(got.cpu(), want.double(), atol=ATOL, rtol=RTOL)
    given = diff.score_windows(model, x0.cuda(), t.cuda(), on_gpu(kw), None, 0, [0] * len(offsets), suffix_skip=False, noise=noise)
    assert torch.equal(given, got)                                 # the explicit-noise form, to the bit
    model.check_device_errors()


def test_score_windows_raises_for_a_bad_timestep():
    model, diff, x0, kw, t, seed, offsets, _, _ = entry_case("2x6")
    with pytest.raises(IndexError):                                # a host t: as the reference's table lookup
        diff.score_windows(model, x0.cuda(), torch.tensor([0, diff.num_timesteps]), on_gpu(kw), None, seed, offsets)
    got = diff.score_windows(model, x0.cuda(), torch.tensor([0, diff.num_timesteps]).cuda(), on_gpu(kw), None, seed, offsets)
    assert torch.isfinite(got[0]) and torch.isnan(got[1])
    with pytest.raises(IndexError):
        model.check_device_errors()


# ------------------------------------------------------------------------------------------------ suffix skip
@pytest.mark.parametrize("name", ["ragged", "1x33"])
def test_suffix_skip_is_exact(name):
    """The suffix of the network on the latent frames only: the same float64 scores, to the bit."""
    if name == "1x33":
        model, diff, x0, kw, t, seed, offsets, _, _ = entry_case("1x33")
    else:                                                          # different latent sets per item, padding, one item all latent
        model, diff = engine(config(6))
        x0, kw = window(4, 6, [{0, 1}, {0, 1, 2}, {0}, set()], [{2, 3, 4, 5}, {3, 4}, {1}, set(range(6))], seed=8)
        t, seed, offsets = torch.tensor([9, 0, 4, 6]), 17, [5, 300000, 600000, 900000]
    full = diff.score_windows(model, x0.cuda(), t.cuda(), on_gpu(kw), None, seed, offsets, suffix_skip=False)
    skip = diff.score_windows(model, x0.cuda(), t.cuda(), on_gpu(kw), None, seed, offsets, suffix_skip=True)
    print(f"\nsuffix skip {name}: {skip.tolist()}")
    assert torch.isfinite(full).all() and (full > 0).all()
    assert torch.equal(skip, full)
    assert torch.equal(diff.score_windows(model, x0.cuda(), t.cuda(), on_gpu(kw), None, seed, offsets, suffix_skip=False), full)
    model.check_device_errors()


# ------------------------------------------------------------------------------------------------ the job
def test_job_vs_oracle_resume_and_sampling(tmp_path, monkeypatch):
    """video_optimal_schedule.run from a checkpoint file on 8 videos: T = 8, obs_length 2, max_frames 4, step_size 2, autoreg,
    subset 4, 2 timesteps = 6 picks, 21 candidate evaluations.  The CPU oracle scores every candidate of every pick on the
    observed set the engine's search has reached, with the noise read back from vd_randn at the job's own offsets."""
    from video_diffusion_amd import inference_util as iu
    from video_diffusion_amd import video_sample as vs
    cfg = config(4, respacing="ddim5")
    model, _ = engine(cfg)
    ora = oracle(cfg)
    ck = tmp_path / "my-checkpoints" / "exp3" / "ema_0.9999_100.pt"
    ck.parent.mkdir(parents=True)
    saved_cfg = {k: v for k, v in cfg.items() if k != "timestep_respacing"}
    saved_cfg.update(timestep_respacing="", max_frames=4)
    torch.save({"state_dict": synth_sd(model.param_specs()), "config": saved_cfg, "step": 100}, ck)
    vids = torch.rand(8, 8, 3, S, S, generator=torch.Generator().manual_seed(31)) * 2 - 1
    np.save(tmp_path / "videos.npy", vids.numpy())
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("SLURM_ARRAY_TASK_ID", raising=False)
    opts = [str(ck), "--videos", str(tmp_path / "videos.npy"), "--inference_mode", "autoreg", "--optimality", "linspace-t", "--T", "8",
            "--obs_length", "2", "--max_frames", "4", "--step_size", "2", "--timestep_respacing", "ddim5", "--batch_size", "5",
            "--seed", "3"]
    job = opts + ["--subset_size", "4", "--num_timesteps", "2"]
    picks = []
    path = vos.run(vos.build_parser().parse_args(job), device=torch.device("cuda", 0), on_pick=picks.append)
    assert str(path) == "results/exp3/ema_0.9999_100_respaceddim5/autoreg_optimal-linspace-t_4_2_8_2/optimal_schedule.pt"
    schedule = torch.load(path)
    assert sorted(schedule) == [0, 1, 2] and all(len(v) == 2 for v in schedule.values())
    assert len(picks) == 6 and sum(len(p["candidates"]) for p in picks) == 21
    blocks = (4 * 3 * S * S + 3) // 4
    worst = 0.0
    for p in picks:                                                # no pick is exempted
        nv, nc = len(p["videos"]), len(p["candidates"])
        offs = [vos.noise_offset(p["step"], p["pick"], v, 8, blocks) for v in p["videos"]]
        n_slots = len(p["obs"]) + 1 + len(p["latent"])
        noise = philox_noise((nv, n_slots, 3, S, S), 3, offs).cpu()
        want = torch.zeros(nc, nv, dtype=torch.float64)
        for ci, c in enumerate(p["candidates"]):
            frames = sorted(p["obs"] + [c]) + p["latent"]
            x0 = vids[p["videos"]][:, frames]
            om = torch.zeros(nv, n_slots, 1, 1, 1)
            om[:, :n_slots - len(p["latent"])] = 1
            kw = dict(frame_indices=torch.tensor(frames).repeat(nv, 1), obs_mask=om, latent_mask=1 - om, kinda_marg_mask=torch.zeros_like(om))
            want[ci] = oracle_scores(ora, x0, torch.tensor(p["t"]), kw, noise).double()
        got = torch.from_numpy(p["scores"])
        print(f"\nERR job step {p['step']} pick {p['pick']} candidates {p['candidates']} best {p['best']} "
              f"max|d| {(got - want).abs().max():.3e} oracle means {want.mean(1).tolist()}")
        worst = max(worst, close(got, want, atol=ATOL, rtol=RTOL))
        means = want.mean(1)                                       # (the search's metric is this times window length x num_timesteps)
        lowest = float(means.min())
        assert float(means[p["candidates"].index(p["best"])]) <= lowest + 2 * (ATOL + RTOL * abs(lowest))
        assert p["best"] in schedule[p["step"]]
    # interrupted after the third pick, resumed: the same file, the same scores
    eval2 = tmp_path / "second"
    calls = []

    def killed_after_three(scorer):
        def wrapped(*a):
            if len(calls) >= 3:
                raise KeyboardInterrupt
            calls.append(1)
            return scorer(*a)
        return wrapped

    with pytest.raises(KeyboardInterrupt):
        vos.run(vos.build_parser().parse_args(job + ["--eval_dir", str(eval2)]), device=torch.device("cuda", 0), scorer_wrap=killed_after_three)
    partial = torch.load(vos.partial_path_of(eval2 / "autoreg_optimal-linspace-t_4_2_8_2" / "optimal_schedule.pt"))
    assert partial == {0: schedule[0], 1: [picks[2]["best"]]}
    resumed = []
    path2 = vos.run(vos.build_parser().parse_args(job + ["--eval_dir", str(eval2)]), device=torch.device("cuda", 0), on_pick=resumed.append)
    assert torch.load(path2) == schedule and len(resumed) == 3
    assert torch.load(vos.partial_path_of(path2)) == torch.load(vos.partial_path_of(path))
    for a, b in zip(resumed, picks[3:]):
        assert (a["step"], a["pick"], a["candidates"], a["best"]) == (b["step"], b["pick"], b["candidates"], b["best"])
        assert np.array_equal(a["scores"], b["scores"])
    # video_sample --optimality linspace-t with the same options reads that file and conditions on exactly those frames
    seen = []
    real_next = iu.InferenceStrategyBase.__next__

    def recording_next(self):
        out = real_next(self)
        seen.append(out)
        return out

    monkeypatch.setattr(iu.InferenceStrategyBase, "__next__", recording_next)
    ap = vs.add_job_arguments(ArgumentParser())
    out = vs.run(ap.parse_args(opts + ["--indices", "0", "1"]), device=torch.device("cuda", 0))
    assert out == path.parent
    assert [o for o, _ in seen] == [schedule[k] for k in range(3)] and [l for _, l in seen] == [[2, 3], [4, 5], [6, 7]]
    assert sorted(f.name for f in (out / "samples").iterdir()) == ["sample_0000-0.npy", "sample_0001-0.npy"]
