"""The sampling LOOPS and the NLL path, seeded through torch's global CPU generator: the tests replay the same generator, so
the draw ORDER (including the loops' RNG-consuming side draws) is part of what is pinned."""
import json

import numpy as np
import torch

from . import _reference
from ._common import build, denoised_fn, kwargs_of, make_inputs, save_npz, tiny_cfg


def _inputs(seed, fidx_rows):
    return make_inputs(2, 4, 32, 2, seed=seed, fidx_rows=fidx_rows, draw=("x0",), zero_latent_x0=False)


def loops(out):
    """GaussianDiffusion.p_sample_loop (gaussian_diffusion.py:450-595) and ddim_sample_loop (:670-748, eta 0 and 1) on the
    tiny ddim5 config.  p_sample_loop calls `.cuda()`: inside this producer Tensor.cuda / Tensor.to('cuda') are identity."""
    cfg = tiny_cfg("ddim5")
    model, diff = build(cfg)
    inp = _inputs(21, [[0, 1, 2, 3], [4, 5, 8, 11]])
    shape = tuple(inp["x0"].shape)
    rec = dict(cfg_json=np.array(json.dumps(cfg)), **{k: v.numpy() for k, v in inp.items()})
    with _reference.cuda_is_identity():
        for obsf, seed in [("x_0", 101), ("x_t_minus_1", 102), ("x_t", 103)]:
            torch.manual_seed(seed)
            kw = kwargs_of(inp, obsf, with_xtm1=False)
            steps = [o["sample"].numpy().copy() for o in diff.p_sample_loop_progressive(model, shape, model_kwargs=kw)]
            assert len(steps) == diff.num_timesteps
            torch.manual_seed(seed)
            final, attns = diff.p_sample_loop(model, shape, model_kwargs=kwargs_of(inp, obsf, with_xtm1=False))
            assert attns == {} and np.array_equal(final.numpy(), steps[-1])
            rec[f"p_{obsf}_seed"] = np.array(seed)
            rec[f"p_{obsf}_step0"] = steps[0]
            rec[f"p_{obsf}_final"] = steps[-1]
            rec[f"p_{obsf}_random_t"] = kw["random_t"].numpy()          # left in model_kwargs by the last iteration
            rec[f"p_{obsf}_x_t_minus_1"] = kw["x_t_minus_1"].numpy()
        for eta, seed in [(0.0, 201), (1.0, 202)]:
            torch.manual_seed(seed)
            kw = kwargs_of(inp, "x_0")
            steps = [o["sample"].numpy().copy() for o in diff.ddim_sample_loop_progressive(model, shape, model_kwargs=kw, eta=eta)]
            torch.manual_seed(seed)
            final = diff.ddim_sample_loop(model, shape, model_kwargs=dict(kw), eta=eta)
            assert torch.is_tensor(final) and np.array_equal(final.numpy(), steps[-1])
            rec[f"ddim_eta{int(eta)}_seed"] = np.array(seed)
            rec[f"ddim_eta{int(eta)}_step0"] = steps[0]
            rec[f"ddim_eta{int(eta)}_final"] = steps[-1]
    return [save_npz(out, "loops_tiny.npz", **rec)]


THIN = 3        # ddim_reverse: an array no later step reads as its input keeps every THIN-th row and column


def ddim_reverse(out):
    """GaussianDiffusion.ddim_reverse_sample (gaussian_diffusion.py:636-668), the deterministic DDIM step from x_t to x_{t+1}, on
    the inputs of `loops`.  The reference has no loop for it: a chain here is x = x0 at t = 0, then t = 1..4 each on the previous
    step's 'sample'.  'x_0' (clip on): every step's 'sample' and 'pred_xstart'; 'x_t' and 'x_t_minus_1' (model_kwargs['x_t_minus_1']
    = x0, read as it is): step 0 and the final sample; a clip_denoised=False chain; the predict_xstart=True config of `xstart`
    at t = 0, 120, 249 on x = x0; `denoised_fn` (steps.denoised's function) at t = 0 and t = 2 of the 'x_0' chain.
    A 'sample' that a recorded later step starts from is whole; every other array is thinned to [..., ::THIN, ::THIN]
    (`<name>_thin`), which keeps the file under loops_tiny.npz's size."""
    cfg = tiny_cfg("ddim5")
    model, diff = build(cfg)
    inp = _inputs(21, [[0, 1, 2, 3], [4, 5, 8, 11]])
    x0 = inp["x0"]
    B = x0.shape[0]
    rec = dict(cfg_json=np.array(json.dumps(cfg)), thin=np.array(THIN), **{k: v.numpy() for k, v in inp.items()})

    def thin(v):
        return np.ascontiguousarray(v.numpy()[..., ::THIN, ::THIN])

    def step(model, diff, x, tv, obsf="x_0", clip=True, fn=None):
        return diff.ddim_reverse_sample(model, x, torch.tensor([tv] * B), clip_denoised=clip, denoised_fn=fn,
                                        model_kwargs=kwargs_of(inp, obsf))

    def chain(obsf, clip):
        x, outs = x0, []
        for tv in range(diff.num_timesteps):
            outs.append(step(model, diff, x, tv, obsf, clip))
            assert set(outs[-1]) == {"sample", "pred_xstart"}
            x = outs[-1]["sample"]
        return outs

    with torch.no_grad():
        for tv, o in enumerate(chain("x_0", True)):
            rec[f"x_0_t{tv}_sample"] = o["sample"].numpy()
            rec[f"x_0_t{tv}_pred_xstart_thin"] = thin(o["pred_xstart"])
        for obsf in ("x_t", "x_t_minus_1"):
            outs = chain(obsf, True)
            rec[f"{obsf}_t0_sample_thin"] = thin(outs[0]["sample"])
            rec[f"{obsf}_final_thin"] = thin(outs[-1]["sample"])
        outs = chain("x_0", False)
        for tv, o in enumerate(outs):
            rec[f"noclip_t{tv}_sample_thin"] = thin(o["sample"])
            rec[f"noclip_t{tv}_pred_xstart_thin"] = thin(o["pred_xstart"])
        rec["noclip_t3_sample"] = outs[3]["sample"].numpy()              # what the t = 4 step (alpha_bar_next = 0) starts from
        for tv in (0, 2):
            x = x0 if tv == 0 else torch.from_numpy(rec[f"x_0_t{tv - 1}_sample"])
            o = step(model, diff, x, tv, fn=denoised_fn)
            rec[f"denoised_t{tv}_sample_thin"], rec[f"denoised_t{tv}_pred_xstart_thin"] = thin(o["sample"]), thin(o["pred_xstart"])
        cfg_x = tiny_cfg("ddim250", predict_xstart=True)
        model_x, diff_x = build(cfg_x)
        assert diff_x.model_mean_type.name == "START_X"
        rec["xstart_cfg_json"] = np.array(json.dumps(cfg_x))
        for tv in (0, 120, 249):
            for clip in (True, False):
                o = step(model_x, diff_x, x0, tv, clip=clip)
                tag = f"xstart_t{tv}_clip{int(clip)}"
                rec[tag + "_sample_thin"], rec[tag + "_pred_xstart_thin"] = thin(o["sample"]), thin(o["pred_xstart"])
    return [save_npz(out, "ddim_reverse_tiny.npz", **rec)]


def nll(out):
    """p_mean_variance (:229-372), _vb_terms_bpd (:750-790), _prior_bpd (:909-926) and calc_bpd_loop_subsampled (:928-1002)
    with explicit latent_mask, t_seq = all 5 steps."""
    cfg = tiny_cfg("ddim5")
    model, diff = build(cfg)
    inp = _inputs(22, [[0, 1, 2, 3], [2, 3, 6, 7]])
    x0 = inp["x0"]
    B = x0.shape[0]
    rec = dict(cfg_json=np.array(json.dumps(cfg)), **{k: v.numpy() for k, v in inp.items()})
    kw = kwargs_of(inp, "x_0")
    g = torch.Generator().manual_seed(5)
    noise = torch.randn(x0.shape, generator=g)
    rec["noise"] = noise.numpy()
    with _reference.cuda_is_identity():
        for tv in (4, 2, 0):
            t = torch.tensor([tv] * B)
            x_t = diff.q_sample(x0, t, noise=noise)
            mv = diff.p_mean_variance(model, x_t, t, clip_denoised=True, model_kwargs=dict(kw))
            assert set(mv) >= {"mean", "variance", "log_variance", "pred_xstart"}
            for k in ("mean", "variance", "log_variance", "pred_xstart"):
                rec[f"t{tv}_{k}"] = mv[k].numpy()
            rec[f"t{tv}_x_t"] = x_t.numpy()
            for clip in (True, False):
                vb = diff._vb_terms_bpd(model, x_start=x0, x_t=x_t, t=t, clip_denoised=clip, model_kwargs=dict(kw),
                                        latent_mask=inp["latent_mask"])
                rec[f"t{tv}_vb_clip{int(clip)}"] = vb["output"].numpy()
            vb_nomask = diff._vb_terms_bpd(model, x_start=x0, x_t=x_t, t=t, clip_denoised=True, model_kwargs=dict(kw))
            rec[f"t{tv}_vb_nomask"] = vb_nomask["output"].numpy()
        rec["prior_bpd"] = diff._prior_bpd(x0, latent_mask=inp["latent_mask"]).numpy()
        rec["prior_bpd_nomask"] = diff._prior_bpd(x0).numpy()
        torch.manual_seed(301)
        m = diff.calc_bpd_loop_subsampled(model, x0, clip_denoised=True, model_kwargs=dict(kw), latent_mask=inp["latent_mask"])
        rec["bpd_seed"] = np.array(301)
        for k, v in m.items():
            rec[f"bpd_{k}"] = v.numpy()
        torch.manual_seed(302)
        t_seq = np.array([[4, 1], [0, 3]])                                  # 2-D: one row of timesteps per batch item (:958-963)
        m2 = diff.calc_bpd_loop_subsampled(model, x0, clip_denoised=True, model_kwargs=dict(kw), latent_mask=inp["latent_mask"],
                                           t_seq=t_seq)
        rec["bpd2_seed"] = np.array(302)
        rec["bpd2_t_seq"] = t_seq
        for k, v in m2.items():
            rec[f"bpd2_{k}"] = v.numpy()
    return [save_npz(out, "nll_tiny.npz", **rec)]


def nll_xstart(out):
    """The NLL path with predict_xstart=True (ModelMeanType.START_X): _vb_terms_bpd (gaussian_diffusion.py:750-790) at
    t = 4, 2, 0, clip on / off, masked and unmasked, and calc_bpd_loop_subsampled (:928-1002) from a seeded global generator."""
    cfg = tiny_cfg("ddim5", predict_xstart=True)
    model, diff = build(cfg)
    inp = make_inputs(2, 4, 32, 2, seed=52, fidx_rows=[[0, 1, 2, 3], [2, 3, 6, 7]], zero_latent_x0=False)
    x0 = inp["x0"]
    B = x0.shape[0]
    rec = dict(cfg_json=np.array(json.dumps(cfg)), **{k: v.numpy() for k, v in inp.items()})
    kw = kwargs_of(inp)
    with torch.no_grad():
        for tv in (4, 2, 0):
            t = torch.tensor([tv] * B)
            x_t = diff.q_sample(x0, t, noise=inp["noise"])
            rec[f"t{tv}_x_t"] = x_t.numpy()
            for clip in (True, False):
                vb = diff._vb_terms_bpd(model, x_start=x0, x_t=x_t, t=t, clip_denoised=clip, model_kwargs=dict(kw), latent_mask=inp["latent_mask"])
                rec[f"t{tv}_vb_clip{int(clip)}"] = vb["output"].numpy()
                rec[f"t{tv}_pred_xstart_clip{int(clip)}"] = vb["pred_xstart"].numpy()
            rec[f"t{tv}_vb_nomask"] = diff._vb_terms_bpd(model, x_start=x0, x_t=x_t, t=t, clip_denoised=True, model_kwargs=dict(kw))["output"].numpy()
        torch.manual_seed(311)
        m = diff.calc_bpd_loop_subsampled(model, x0, clip_denoised=True, model_kwargs=dict(kw), latent_mask=inp["latent_mask"])
        rec["bpd_seed"] = np.array(311)
        for k, v in m.items():
            rec[f"bpd_{k}"] = v.numpy()
    return [save_npz(out, "nll_xstart_tiny.npz", **rec)]
