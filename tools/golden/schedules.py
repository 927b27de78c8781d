"""Integer and float64-table fixtures: retained-step sets, diffusion schedules, frame schedulers, parameter names."""
import contextlib
import io
import signal

import torch

from . import _reference
from ._common import save_json, tiny_cfg


def space_timesteps(out):
    """Retained-step sets / error cases (respace.py:7-58)."""
    respace = _reference.load().respace
    cases = []
    for n, sec in [(1000, "ddim250"), (1000, "250"), (1000, "ddim50"), (1000, "10,15,20"), (1000, "ddim300"),
                   (1000, "1000"), (1000, "ddim1000"), (100, "ddim10"), (300, "10,15,20"), (1000, "ddim5"),
                   (1000, "ddim100"), (1000, "50,50"), (1000, "600,600")]:
        try:
            cases.append(dict(n=n, spec=sec, steps=sorted(respace.space_timesteps(n, sec))))
        except ValueError as e:
            cases.append(dict(n=n, spec=sec, error=str(e)))
    return [save_json(out, "space_timesteps.json", cases)]


def schedules(out):
    """float64 tables + timestep_map (respace.py:68-82, gaussian_diffusion.py:123-172), one file per schedule."""
    su = _reference.load().su
    paths = []
    for tag, kw in [("linear1000_ddim250", dict(steps=1000, noise_schedule="linear", timestep_respacing="ddim250")),
                    ("linear1000_full", dict(steps=1000, noise_schedule="linear", timestep_respacing="")),
                    ("linear1000_ddim50", dict(steps=1000, noise_schedule="linear", timestep_respacing="ddim50")),
                    ("cosine1000_ddim100", dict(steps=1000, noise_schedule="cosine", timestep_respacing="ddim100")),
                    ("linear1000_ddim5_small", dict(steps=1000, noise_schedule="linear", timestep_respacing="ddim5",
                                                    sigma_small=True))]:
        d = su.create_gaussian_diffusion(rescale_timesteps=True, rescale_learned_sigmas=True, **kw)
        rec = dict(kw=kw, timestep_map=list(d.timestep_map), num_timesteps=d.num_timesteps)
        for name in ["betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod",
                     "sqrt_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod",
                     "posterior_variance", "posterior_log_variance_clipped", "posterior_mean_coef1",
                     "posterior_mean_coef2"]:
            rec[name] = [float.hex(float(v)) for v in getattr(d, name)]
        paths.append(save_json(out, f"schedule_{tag}.json", rec))
    return paths


def schedulers(out):
    """(obs, latent) index sequences of the fixed frame schedulers (inference_util.py)."""
    iu = _reference.load().iu
    cases = []
    for mode, args in [("autoreg", (16, 4, 10, 1)), ("independent", (16, 4, 16, 12)), ("autoreg", (300, 36, 20, 7)),
                       ("exp-past", (16, 4, 16, 4)), ("autoreg", (500, 36, 20, 10)), ("autoreg", (16, 0, 10, 1)),
                       ("hierarchy-2", (300, 36, 20, 10)), ("really-independent", (30, 4, 10, 5)),
                       ("independent", (40, 6, 12, 5)), ("exp-past", (64, 8, 20, 5)),
                       ("mixed-autoreg-independent", (60, 10, 20, 5)), ("hierarchy-3", (300, 36, 20, 10)),
                       ("hierarchy-2", (100, 10, 15, 5)), ("cwvae", (100, 36, 20, 10)),
                       ("google", (64, 8, 16, 8))]:
        if mode not in iu.inference_strategies:
            continue
        try:
            it = iter(iu.inference_strategies[mode](video_length=args[0], num_obs=args[1], max_frames=args[2],
                                                    step_size=args[3], optimal_schedule_path=None))
            seq = [[[int(i) for i in o], [int(i) for i in l]] for o, l in it]
            cases.append(dict(mode=mode, args=list(args), seq=seq))
        except Exception as e:  # noqa: BLE001 -- record what the reference does, including failures
            cases.append(dict(mode=mode, args=list(args), error=type(e).__name__))
    return [save_json(out, "schedulers.json", dict(modes=sorted(iu.inference_strategies.keys()), cases=cases))]


def schedulers_more(out):
    """The goal-directed / visualisation / frameskip schedules (inference_util.py:534-776), integer logic."""
    iu = _reference.load().iu
    cases = []
    for mode, args in [("goal-directed-autoreg", (30, 4, 10, 3)), ("goal-directed-autoreg", (64, 8, 20, 5)),
                       ("goal-directed-mixed", (40, 6, 12, 4)), ("goal-directed-mixed", (64, 8, 20, 5)),
                       ("goal-directed-hierarchy-2", (100, 10, 20, 5)), ("goal-directed-hierarchy-2", (64, 8, 16, 4)),
                       ("ho-et-al-for-vis", (64, 0, 16, 8)), ("ho-et-al-for-vis", (40, 0, 16, 8)),
                       ("baby-cond-ho-et-al-for-vis", (30, 4, 7, 3)),
                       ("google", (64, 8, 16, 8)), ("google", (100, 4, 16, 8)), ("google", (37, 5, 16, 8)),
                       ("like-google", (64, 8, 16, 8)), ("like-google", (50, 5, 12, 4)), ("like-google", (30, 1, 10, 3))]:
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                it = iter(iu.inference_strategies[mode](video_length=args[0], num_obs=args[1], max_frames=args[2],
                                                        step_size=args[3]))
                seq = []
                for o, l in it:
                    seq.append([[int(i) for i in o], [int(i) for i in l]])
                    if len(seq) > 400:
                        raise RuntimeError("does not terminate")
            cases.append(dict(mode=mode, args=list(args), seq=seq))
        except Exception as e:  # noqa: BLE001 -- record what the reference does, including failures
            cases.append(dict(mode=mode, args=list(args), error=type(e).__name__))
    return [save_json(out, "schedulers_more.json", dict(modes=sorted(iu.inference_strategies.keys()), cases=cases))]


def schedulers_adaptive(out):
    """`adaptive-autoreg` / `adaptive-hierarchy-N` (inference_util.py:137-229,421-531) pick the observed frames of a window
    per batch item by farthest-point selection on frame embeddings.  The reference supports two embeddings: the raw frames
    (distance='l2') and LPIPS features (distance='lpips', what scripts/video_sample.py passes; needs the pretrained AlexNet
    of the `lpips` package, which is not available offline).  The l2 variant is pure arithmetic on the sample tensor and is
    what is pinned here: seeded synthetic videos, the full (obs per item, latents per item) sequence or the exception type."""
    iu = _reference.load().iu
    cases = []
    for mode, (T, n_obs, max_frames, step), B, seed in [
            ("adaptive-autoreg", (20, 4, 8, 3), 2, 1), ("adaptive-autoreg", (16, 0, 6, 2), 3, 2), ("adaptive-autoreg", (30, 6, 10, 5), 1, 3),
            ("adaptive-hierarchy-2", (30, 4, 8, 4), 2, 4), ("adaptive-hierarchy-2", (40, 6, 12, 5), 2, 5),
            ("adaptive-hierarchy-3", (60, 6, 12, 4), 1, 6), ("adaptive-hierarchy-2", (20, 0, 8, 4), 2, 7)]:
        v = torch.rand(B, T, 3, 4, 4, generator=torch.Generator().manual_seed(seed)) * 2 - 1
        rec = dict(mode=mode, args=[T, n_obs, max_frames, step], B=B, seed=seed)
        seq = []

        def on_alarm(signum, frame):
            raise TimeoutError("the reference does not terminate on this case")
        signal.signal(signal.SIGALRM, on_alarm)           # a watchdog, not a measurement
        signal.alarm(20)
        try:
            it = iter(iu.inference_strategies[mode](distance="l2", video_length=T, num_obs=n_obs, max_frames=max_frames,
                                                    step_size=step, optimal_schedule_path=None))
            while len(seq) < 200:
                it.set_videos(v)
                try:
                    obs, lat = next(it)
                except StopIteration:
                    break
                seq.append([[[int(i) for i in o] for o in obs], [[int(i) for i in l] for l in lat]])
            rec["seq"] = seq
        except Exception as e:  # noqa: BLE001 -- record what the reference does, including failures
            rec["error"] = type(e).__name__
            rec["seq_before_error"] = seq
        finally:
            signal.alarm(0)
        cases.append(rec)
        print(mode, rec["args"], "steps", len(rec.get("seq", rec.get("seq_before_error", []))), rec.get("error"))
    return [save_json(out, "schedulers_adaptive.json", dict(cases=cases))]


def param_specs(out):
    """state_dict name -> shape (unet.py constructors), built on the meta device."""
    su = _reference.load().su
    rec = {}
    for tag, cfg in [("tiny", tiny_cfg("ddim250")), ("tiny_table", tiny_cfg("ddim250", use_rpe_net=False)),
                     ("default64", {**su.video_model_and_diffusion_defaults(), **dict(T=16, image_size=64, rp_alpha=16,
                                                                                   rp_beta=16, rp_gamma=16)}),
                     ("default128", {**su.video_model_and_diffusion_defaults(), **dict(T=16, image_size=128,
                                                                                    rp_alpha=16, rp_beta=16,
                                                                                    rp_gamma=16)})]:
        with torch.device("meta"):
            model, _ = su.create_video_model_and_diffusion(**cfg)
        rec[tag] = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    return [save_json(out, "param_specs.json", rec)]
