"""Single steps of the tiny model: eps at Boundary A, per-block activations, p_sample / ddim_sample / p_mean_variance dicts
with recorded noise, and the config variants (denoised_fn, predict_xstart, cond_emb_type, learn_sigma, attention maps)."""
import json

import numpy as np
import torch

from . import _reference
from ._common import FixedNoise, build, denoised_fn, kwargs_of, make_inputs, npy, save_npz, tiny_cfg


def _inputs_a():
    return make_inputs(2, 4, 32, 2, seed=11, fidx_rows=[[0, 1, 2, 3], [5, 6, 9, 12]])


def _unet(out, tag, cfg, cases):
    model, diff = build(cfg)
    wrapped = diff._wrap_model(model)
    rec = dict(cfg_json=np.array(json.dumps(cfg)))
    for ci, (inp, t_val, obsf) in enumerate(cases):
        B = inp["x"].shape[0]
        t = torch.tensor([t_val] * B)
        with torch.no_grad():
            eps, _ = wrapped(inp["x"], t, **kwargs_of(inp, obsf))
        for k, v in npy(inp).items():
            rec[f"c{ci}_{k}"] = v
        rec[f"c{ci}_t"] = t.numpy()
        rec[f"c{ci}_observed_frames"] = np.array(obsf)
        rec[f"c{ci}_eps"] = eps.numpy()
    return [save_npz(out, f"unet_{tag}.npz", **rec)]


def unet_tiny(out):
    """eps at Boundary A for several t / masks / frame_indices / observed_frames."""
    a = _inputs_a()
    b = make_inputs(1, 3, 32, 1, seed=12, fidx_rows=[[7, 2, 30]])
    b["kinda_marg_mask"][:, 2] = 1          # one kinda-marginal frame, neither obs nor latent
    b["latent_mask"][:, 2] = 0
    c = _inputs_c()
    return _unet(out, "tiny", tiny_cfg("ddim250"), [(a, 249, "x_0"), (a, 0, "x_0"), (b, 100, "x_0"), (c, 17, "x_0"),
                                                   (a, 200, "x_t"), (a, 200, "x_t_minus_1")])


def _inputs_c():
    c = make_inputs(2, 4, 32, 2, seed=13, fidx_rows=[[0, 1, 2, 3], [3, 2, 1, 0]])
    c["latent_mask"][0, 3] = 0              # a padded frame: exercises the temporal attention mask
    return c


def unet_tiny_table(out):
    return _unet(out, "tiny_table", tiny_cfg("ddim250", use_rpe_net=False, rp_alpha=2, rp_beta=4, rp_gamma=8),
                 [(_inputs_a(), 123, "x_0")])


def unet_tiny_frameenc(out):
    return _unet(out, "tiny_frameenc", tiny_cfg("ddim250", use_frame_encoding=True, enforce_position_invariance=True,
                                                allow_interactions_between_padding=False), [(_inputs_c(), 60, "x_0")])


def unet_tiny_noss(out):
    return _unet(out, "tiny_noss", tiny_cfg("ddim250", use_scale_shift_norm=False, use_spatial_encoding=False,
                                            num_res_blocks=2), [(_inputs_a(), 5, "x_0")])


def blocks(out):
    """Strided slices of per-block activations of the unet_tiny model at t = 249."""
    model, diff = build(tiny_cfg("ddim250"))
    inp, t_val = _inputs_a(), 249
    caps = {}

    def hook(name):
        def f(mod, args, kwargs, out):
            caps[name] = out if torch.is_tensor(out) else out[0]
        return f

    hs = [model.time_embed.register_forward_hook(hook("emb"), with_kwargs=True),
          model.input_blocks[0].register_forward_hook(hook("in0"), with_kwargs=True),
          model.input_blocks[1].register_forward_hook(hook("in1"), with_kwargs=True),
          model.input_blocks[2].register_forward_hook(hook("in2"), with_kwargs=True),
          model.input_blocks[3][0].register_forward_hook(hook("in3_res"), with_kwargs=True),
          model.input_blocks[3][1].temporal_attention.register_forward_hook(hook("in3_tattn"), with_kwargs=True),
          model.input_blocks[3][1].register_forward_hook(hook("in3_attn"), with_kwargs=True),
          model.middle_block.register_forward_hook(hook("mid"), with_kwargs=True),
          model.output_blocks[0].register_forward_hook(hook("out0"), with_kwargs=True),
          model.output_blocks[-1].register_forward_hook(hook("out_last"), with_kwargs=True)]
    B = inp["x"].shape[0]
    with torch.no_grad():
        diff._wrap_model(model)(inp["x"], torch.tensor([t_val] * B), **kwargs_of(inp))
    for h in hs:
        h.remove()
    rec = {}
    for k, v in caps.items():
        v = v.detach()
        if v.dim() == 4 and k != "in3_tattn":          # (N,C,H,W): keep a strided slice
            v = v[:, ::4, ::3, ::3]
        elif k == "in3_tattn":                          # (B, HW, C, T)
            v = v[:, ::7, ::4, :]
        rec[k] = v.numpy().copy()
    return [save_npz(out, "blocks_tiny.npz", t=np.array(t_val), **rec)]


def psample(out):
    """p_sample / ddim_sample dicts with explicit noise."""
    model, diff = build(tiny_cfg("ddim250"))
    inp = _inputs_a()
    rec = {}
    B = inp["x"].shape[0]
    for t_val in [diff.num_timesteps - 1, diff.num_timesteps - 2, 1, 0]:
        t = torch.tensor([t_val] * B)
        mv = diff.p_mean_variance(model, inp["x"], t, clip_denoised=True, model_kwargs=kwargs_of(inp))
        nz = (t != 0).float().view(-1, 1, 1, 1, 1)
        sample = mv["mean"] + nz * torch.exp(0.5 * mv["log_variance"]) * inp["noise"]   # gaussian_diffusion.py:438-443
        rec[f"t{t_val}_mean"] = mv["mean"].numpy()
        rec[f"t{t_val}_pred_xstart"] = mv["pred_xstart"].numpy()
        rec[f"t{t_val}_log_variance"] = mv["log_variance"][:, 0, 0, 0, 0].numpy()
        rec[f"t{t_val}_variance"] = mv["variance"][:, 0, 0, 0, 0].numpy()
        rec[f"t{t_val}_sample"] = sample.numpy()
        # p_sample itself, with randn_like pinned to the recorded noise
        orig = torch.randn_like
        torch.randn_like = lambda x, *a, **k: inp["noise"]
        try:
            ps = diff.p_sample(model, inp["x"], t, clip_denoised=True, model_kwargs=kwargs_of(inp))
            rec[f"t{t_val}_psample"] = ps["sample"].numpy()
            for eta in (0.0, 1.0):
                dd = diff.ddim_sample(model, inp["x"], t, clip_denoised=True, model_kwargs=kwargs_of(inp), eta=eta)
                rec[f"t{t_val}_ddim_eta{int(eta)}"] = dd["sample"].numpy()
        finally:
            torch.randn_like = orig
        assert np.array_equal(rec[f"t{t_val}_psample"], rec[f"t{t_val}_sample"])
    qs = diff.q_sample(inp["x0"], torch.tensor([3] * B), noise=inp["noise"])
    rec["q_sample_t3"] = qs.numpy()
    for k, v in npy(inp).items():
        rec[k] = v
    return [save_npz(out, "psample_tiny.npz", **rec)]


def window(out):
    """scripts/video_sample.py:149-168 with the 5-step 'ddim5' respacing and recorded noise."""
    cfg = tiny_cfg("ddim5")
    inp = _inputs_a()
    model, diff = build(cfg)
    g = torch.Generator().manual_seed(77)
    noises = [torch.randn(inp["x"].shape, generator=g) for _ in range(diff.num_timesteps)]
    it = iter(noises)
    orig = torch.randn_like
    torch.randn_like = lambda x, *a, **k: next(it)
    try:
        B = inp["x"].shape[0]
        local = inp["x0"].clone()
        traj = []
        for timestep in list(range(diff.num_timesteps))[::-1]:
            local = diff.p_sample(model, local, t=torch.tensor([timestep] * B), clip_denoised=True,
                                  model_kwargs=kwargs_of(inp))["sample"]
            traj.append(local.numpy().copy())
    finally:
        torch.randn_like = orig
    return [save_npz(out, "window_tiny.npz", noises=np.stack([n.numpy() for n in noises]), final=traj[-1], step0=traj[0],
                     cfg_json=np.array(json.dumps(cfg)), **npy(inp))]


_WITH_NOISE2 = ("x0", "x", "noise", "noise2")


def denoised(out):
    """p_sample / ddim_sample / p_mean_variance with a `denoised_fn` (gaussian_diffusion.py:319-324)."""
    cfg = tiny_cfg("ddim250")
    model, diff = build(cfg)
    inp = make_inputs(2, 4, 32, 2, 11, [[0, 1, 2, 3], [5, 6, 9, 12]], draw=_WITH_NOISE2)
    rec = dict(cfg_json=json.dumps(cfg), **{k: v.numpy() for k, v in inp.items()})
    with torch.no_grad():
        for t_val in [249, 120, 0]:
            t = torch.tensor([t_val] * 2)
            for clip in (True, False):
                tag = f"t{t_val}_clip{int(clip)}"
                with FixedNoise(inp["noise"]):
                    o = diff.p_sample(model, inp["x"], t, clip_denoised=clip, denoised_fn=denoised_fn, model_kwargs=kwargs_of(inp))
                rec[tag + "_psample"], rec[tag + "_pred_xstart"] = o["sample"].numpy(), o["pred_xstart"].numpy()
                pm = diff.p_mean_variance(model, inp["x"], t, clip_denoised=clip, denoised_fn=denoised_fn, model_kwargs=kwargs_of(inp))
                rec[tag + "_mean"] = pm["mean"].numpy()
                for eta in (0.0, 1.0):
                    with FixedNoise(inp["noise"]):
                        o = diff.ddim_sample(model, inp["x"], t, clip_denoised=clip, denoised_fn=denoised_fn,
                                             model_kwargs=kwargs_of(inp), eta=eta)
                    rec[tag + f"_ddim_eta{int(eta)}"] = o["sample"].numpy()
    return [save_npz(out, "denoised_fn_tiny.npz", **rec)]


def xstart(out):
    """predict_xstart=True (ModelMeanType.START_X, script_util.py:429-431, gaussian_diffusion.py:326-341): p_sample /
    ddim_sample (eta 0, 1) / p_mean_variance dicts at t = 249, 120, 1, 0, clip on and off, recorded noise."""
    cfg = tiny_cfg("ddim250", predict_xstart=True)
    model, diff = build(cfg)
    assert diff.model_mean_type.name == "START_X"
    inp = _inputs_a()
    x, noise, kw, B = inp["x"], inp["noise"], kwargs_of(inp), 2
    rec = dict(cfg_json=json.dumps(cfg), **npy(inp))
    real_randn = torch.randn_like
    torch.randn_like = lambda v, **k: noise.clone()            # p_sample / ddim_sample draw th.randn_like(x): the recorded noise
    try:
        with torch.no_grad():
            for t_val in [249, 120, 1, 0]:
                t = torch.tensor([t_val] * B)
                for clip in (True, False):
                    tag = f"t{t_val}_clip{int(clip)}"
                    pm = diff.p_mean_variance(model, x, t, clip_denoised=clip, model_kwargs=dict(kw))
                    rec[tag + "_mean"] = pm["mean"].numpy()
                    rec[tag + "_pred_xstart"] = pm["pred_xstart"].numpy()
                    ps = diff.p_sample(model, x, t, clip_denoised=clip, model_kwargs=dict(kw))
                    rec[tag + "_psample"] = ps["sample"].numpy()
                    for eta in (0.0, 1.0):
                        dd = diff.ddim_sample(model, x, t, clip_denoised=clip, model_kwargs=dict(kw), eta=eta)
                        rec[tag + f"_ddim_eta{int(eta)}"] = dd["sample"].numpy()
    finally:
        torch.randn_like = real_randn
    return [save_npz(out, "xstart_tiny.npz", **rec)]


def attn(out):
    """return_attn_weights=True: the {'temporal': [...], 'spatial': [...]} lists (unet.py:457-466,799-836)."""
    cfg = tiny_cfg("ddim250")
    model, diff = build(cfg)
    inp = make_inputs(2, 4, 32, 2, 31, [[0, 1, 2, 3], [5, 6, 9, 12]], draw=_WITH_NOISE2)
    rec = dict(cfg_json=json.dumps(cfg), **{k: v.numpy() for k, v in inp.items()})
    with torch.no_grad():
        t = torch.tensor([100, 100])
        with FixedNoise(inp["noise"]):
            o = diff.p_sample(model, inp["x"], t, clip_denoised=True, model_kwargs=kwargs_of(inp), return_attn_weights=True)
        rec["psample"] = o["sample"].numpy()
        for kind in ("temporal", "spatial"):
            rec[f"n_{kind}"] = len(o["attn"][kind])
            for i, a in enumerate(o["attn"][kind]):
                rec[f"{kind}_{i}_shape"] = np.array(a.shape)
                # the 256 x 256 spatial maps are stored every 8th query row (2 MB each otherwise)
                rec[f"{kind}_{i}"] = (a[:, ::8] if a.shape[1] > 64 else a).numpy()
                print(kind, i, tuple(a.shape))
        pm = diff.p_mean_variance(model, inp["x"], t, model_kwargs=kwargs_of(inp), return_attn_weights=True)
        assert len(pm["attn"]["temporal"]) == len(o["attn"]["temporal"])
    return [save_npz(out, "attn_tiny.npz", **rec)]


def attn_denoised(out):
    """return_attn_weights TOGETHER with denoised_fn (gaussian_diffusion.py:274-324 allows it): p_sample and
    p_mean_variance dicts + the per-block head-averaged attention maps."""
    cfg = tiny_cfg("ddim250")
    model, diff = build(cfg)
    inp = make_inputs(2, 4, 32, 2, seed=53, fidx_rows=[[0, 1, 2, 3], [5, 6, 9, 12]], zero_latent_x0=False)
    inp["x0"][:, 2:] = 0
    rec = dict(cfg_json=np.array(json.dumps(cfg)), **{k: v.numpy() for k, v in inp.items()})
    with torch.no_grad():
        t = torch.tensor([120, 120])
        with FixedNoise(inp["noise"]):
            o = diff.p_sample(model, inp["x"], t, clip_denoised=True, denoised_fn=denoised_fn, model_kwargs=kwargs_of(inp), return_attn_weights=True)
        rec["psample"], rec["pred_xstart"] = o["sample"].numpy(), o["pred_xstart"].numpy()
        for kind in ("temporal", "spatial"):
            rec[f"n_{kind}"] = np.array(len(o["attn"][kind]))
            for i, a in enumerate(o["attn"][kind]):
                rec[f"{kind}_{i}_shape"] = np.array(a.shape)
                rec[f"{kind}_{i}"] = (a[:, ::8] if a.shape[1] > 64 else a).numpy()
        pm = diff.p_mean_variance(model, inp["x"], t, clip_denoised=True, denoised_fn=denoised_fn, model_kwargs=kwargs_of(inp), return_attn_weights=True)
        rec["pmv_mean"] = pm["mean"].numpy()
        assert len(pm["attn"]["temporal"]) == len(o["attn"]["temporal"])
    return [save_npz(out, "attn_denoised_tiny.npz", **rec)]


def variants(out):
    """cond_emb_type in {duplicate, all-initzero, t=0} (unet.py:932-947,1014-1019) and learn_sigma=True (LEARNED_RANGE variance,
    gaussian_diffusion.py:277-298; script_util.py:129-131,424-428): eps at Boundary A, p_sample / ddim_sample / p_mean_variance."""
    rec = {}
    for name, over in [("dup", dict(cond_emb_type="duplicate")), ("allz", dict(cond_emb_type="all-initzero")), ("t0", dict(cond_emb_type="t=0")),
                       ("ls", dict(learn_sigma=True))]:
        cfg = tiny_cfg("ddim250", **over)
        model, diff = build(cfg)
        inp = make_inputs(2, 4, 32, 2, 41 + len(name), [[0, 1, 2, 3], [5, 6, 9, 12]], draw=_WITH_NOISE2)
        inp["obs_mask"][1] = 0                       # batch item 1 has no observed frame ('t=0' writes -1 through an expanded tensor:
        inp["latent_mask"][1] = 1                    # a whole batch item gets it as soon as one of its frames is observed)
        inp["x0"][1] = 0
        rec[name + "_cfg_json"] = json.dumps(cfg)
        for k, v in inp.items():
            if k != "noise2":
                rec[f"{name}_{k}"] = v.numpy()
        with torch.no_grad():
            for t_val in [100, 0]:
                t = torch.tensor([t_val] * 2)
                tag = f"{name}_t{t_val}"
                eps, _ = diff._wrap_model(model)(inp["x"], t, **kwargs_of(inp))
                rec[tag + "_out"] = eps.numpy()
                if cfg["learn_sigma"]:
                    # the reference cannot sample with a learned variance on video tensors: its own assert fails
                    # (gaussian_diffusion.py:283, C = x.shape[1] = T); record that, it is the behaviour to mirror
                    try:
                        diff.p_sample(model, inp["x"], t, clip_denoised=True, model_kwargs=kwargs_of(inp))
                        rec[tag + "_psample_error"] = "none"
                    except AssertionError:
                        rec[tag + "_psample_error"] = "AssertionError"
                    continue
                with FixedNoise(inp["noise"]):
                    o = diff.p_sample(model, inp["x"], t, clip_denoised=True, model_kwargs=kwargs_of(inp))
                rec[tag + "_psample"], rec[tag + "_pred_xstart"] = o["sample"].numpy(), o["pred_xstart"].numpy()
                with FixedNoise(inp["noise"]):
                    o = diff.ddim_sample(model, inp["x"], t, clip_denoised=True, model_kwargs=kwargs_of(inp), eta=1.0)
                rec[tag + "_ddim_eta1"] = o["sample"].numpy()
        print(name, "out", rec[f"{name}_t100_out"].shape, "var_type", diff.model_var_type)
    return [save_npz(out, "variants_tiny.npz", **rec)]


def probe_no_cond_marg():
    """do_cond_marg=False cannot be constructed in the reference: create_video_model passes cond_emb_type to UNetVideoModel,
    whose UNetModel.__init__ does not take it (script_util.py:275-300): TypeError.  The mirror raises the same.  Writes no
    fixture; the result is printed."""
    su = _reference.load().su
    cfg = su.video_model_and_diffusion_defaults()
    cfg.update(T=4, image_size=32, num_channels=32, num_res_blocks=1, rp_alpha=4, rp_beta=4, rp_gamma=4, do_cond_marg=False)
    try:
        su.create_video_model_and_diffusion(**cfg)
        print("do_cond_marg=False: constructed (unexpected)")
    except TypeError as e:
        print("do_cond_marg=False ->", type(e).__name__, e)
