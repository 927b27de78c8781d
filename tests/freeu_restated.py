"""FreeU (Si, Huang, Jiang, Liu, CVPR 2024) restated: the two operators the decoder applies to the halves of a concat in float64, the
published code's FFT form of the filter, the oracle UNet that runs them (FreeUNetRef), and the model cases the CPU and the GPU tests
share -- the CPU test licenses the parameters (they move eps far beyond the comparison tolerance), the GPU test compares.  Nothing
returned from a cached function here may be written to."""
import functools
import math

import torch

from helpers import ATOL, synth_sd
from oracle.sampler_ref import SamplerRef
from oracle.schedule_ref import ScheduleRef
from oracle.unet_ref import UNetRef


# ------------------------------------------------------------------------------------------------ the operators, planes last
def filter_fft(x, s):
    """The published form on float64 planes (..., S, S): fft2 -> fftshift -> the box [S//2 - 1 : S//2 + 1]^2 (threshold 1) times s
    -> ifftshift -> ifft2 -> .real."""
    S = x.shape[-1]
    X = torch.fft.fftshift(torch.fft.fftn(x.to(torch.float64), dim=(-2, -1)), dim=(-2, -1))
    M = torch.ones(S, S, dtype=torch.float64)
    c = S // 2
    M[c - 1:c + 1, c - 1:c + 1] = s
    return torch.fft.ifftn(torch.fft.ifftshift(X * M, dim=(-2, -1)), dim=(-2, -1)).real


def filter_closed(x, s):
    """The closed form on float64 planes (..., S, S): x + (s - 1) / S^2 (m0 + ci cos(th i) + si sin(th i) + cj cos(th j) + sj sin(th j)
    + cd cos(th (i + j)) + sd sin(th (i + j))), the seven coefficients being the sums of x against the same seven functions."""
    x = x.to(torch.float64)
    S = x.shape[-1]
    th = 2.0 * math.pi / S
    i = torch.arange(S, dtype=torch.float64).view(S, 1).expand(S, S)
    j = torch.arange(S, dtype=torch.float64).view(1, S).expand(S, S)
    upd = x.sum((-2, -1), keepdim=True).expand_as(x).clone()
    for f in (torch.cos(th * i), torch.sin(th * i), torch.cos(th * j), torch.sin(th * j), torch.cos(th * (i + j)), torch.sin(th * (i + j))):
        upd = upd + (x * f).sum((-2, -1), keepdim=True) * f
    return x + (s - 1.0) / (S * S) * upd


def structure_map(h):
    """g of the adaptive form for float64 h (N, C, S, S): the channel mean, min-max normalised per frame; a constant frame gives 0 (the
    published code divides 0 by 0 there)."""
    m = h.to(torch.float64).mean(1, keepdim=True)
    lo, hi = m.amin((2, 3), keepdim=True), m.amax((2, 3), keepdim=True)
    span = hi - lo
    return torch.where(span != 0, (m - lo) / torch.where(span != 0, span, torch.ones_like(span)), torch.zeros_like(m))


def backbone(h, b, adaptive):
    """float64 h (N, C, S, S) -> h': the first C // 2 channels times b (plain) or (b - 1) g + 1 (adaptive), the others as they are."""
    h = h.to(torch.float64)
    H = h.shape[1] // 2
    out = h.clone()
    out[:, :H] = h[:, :H] * (((b - 1.0) * structure_map(h) + 1.0) if adaptive else b)
    return out


def rounding_bound(ref64, x):
    """One float32 rounding of a float64-exact value, plus float64's own error where the update cancels against x."""
    return 2.0 ** -23 * ref64.abs() + 2.0 ** -40 * float(x.abs().max())


# ------------------------------------------------------------------------------------------------ the oracle network
class FreeUNetRef(UNetRef):
    """UNetRef whose decoder applies FreeU: at the two lowest-resolution levels (stage 1: the first num_res_blocks + 1 output blocks,
    stage 2: the next) every block reads cat([h', skip']).  The plain scale is the float32 multiply the engine states; the adaptive scale
    and the filter are float64 rounded once."""

    def __init__(self, cfg, sd, b=(1.0, 1.0), s=(1.0, 1.0), adaptive=False):
        super().__init__(cfg, sd)
        self.fu_b, self.fu_s, self.fu_adaptive = tuple(b), tuple(s), bool(adaptive)

    def freeu(self, h, skip, stage):
        b, s = self.fu_b[stage], self.fu_s[stage]
        if b != 1.0:
            if self.fu_adaptive:
                h = backbone(h, b, True).float()
            else:
                H = h.shape[1] // 2
                h = torch.cat([h[:, :H] * b, h[:, H:]], dim=1)
        if s != 1.0:
            skip = filter_closed(skip, s).float()
        return h, skip

    def torso(self, x5, t_frames, fidx, mask, B, T):
        from oracle.unet_ref import gn, silu, sinus_embedding
        topo, mc = self.topo, self.cfg["num_channels"]
        per = self.cfg["num_res_blocks"] + 1
        emb = self.lin(silu(self.lin(sinus_embedding(t_frames, mc), "time_embed.0")), "time_embed.2")
        hs, h = [], x5
        for i, blk in enumerate(topo["input"]):
            h = self.run_block(blk, f"input_blocks.{i}", h, emb, fidx, mask, T)
            hs.append(h)
            if i + 1 == topo["n_before_attn"]:
                if self.cfg.get("use_spatial_encoding", True):
                    h = h + self.p("spatial_encoding")
                if self.cfg.get("use_frame_encoding", False):
                    fi = fidx.float()
                    if self.cfg.get("enforce_position_invariance", False):
                        fi = fi - fi.mean(dim=1, keepdim=True)
                    fe = sinus_embedding(fi.reshape(-1), h.shape[1], max_period=self.cfg["T"] * 10)
                    h = h + fe.view(B * T, -1, 1, 1)
        h = self.run_block(topo["middle"], "middle_block", h, emb, fidx, mask, T)
        for i, blk in enumerate(topo["output"]):
            skip = hs.pop()
            if i // per < 2:
                h, skip = self.freeu(h, skip, i // per)
            h = self.run_block(blk, f"output_blocks.{i}", torch.cat([h, skip], dim=1), emb, fidx, mask, T)
        return self.conv(silu(gn(h, self.p("out.0.weight"), self.p("out.0.bias"))), "out.2")


# ------------------------------------------------------------------------------------------------ the shared model cases
# The constants of the GPU model tests.  Started from b = (1.4, 1.2), s = (0.6, 0.8); tests/test_freeu_cpu.py asserts that with THESE
# the oracle's eps moves by at least 100 x the comparison tolerance on every case, so that an engine that ran no FreeU pass could not pass.
B_CONST, S_CONST = (1.4, 1.2), (0.6, 0.8)
EPS_ATOL = EPS_RTOL = ATOL                              # test_gpu_engine.py's tolerance on eps of these models
SWEEP_TAG = "w32_att8_rb3_s32"                          # a fixture configuration: four blocks per stage, attention at 8 only


def _defaults():
    import video_diffusion_amd as vda
    return vda.video_model_and_diffusion_defaults()


def model_cfg(name):
    if name == "tiny":                                  # 32 channels, two blocks per stage
        return {**_defaults(), **dict(T=4, image_size=32, num_channels=32, num_res_blocks=1, rp_alpha=4, rp_beta=4, rp_gamma=4,
                                      timestep_respacing="ddim10")}
    if name == "w64_rb2":                               # 64 channels, three blocks per stage
        return {**_defaults(), **dict(T=4, image_size=32, num_channels=64, num_res_blocks=2, rp_alpha=4, rp_beta=4, rp_gamma=4,
                                      timestep_respacing="ddim10")}
    if name == "w64_s64":                               # stage 2 at 16 x 16 with 192 channels out: see wide_window
        return {**_defaults(), **dict(T=4, image_size=64, num_channels=64, num_res_blocks=1, rp_alpha=4, rp_beta=4, rp_gamma=4,
                                      timestep_respacing="ddim10")}
    from config_sweep_cases import case
    return dict(case(SWEEP_TAG)["cfg"])


@functools.lru_cache(maxsize=None)
def window(name):
    """(x, t, oracle kwargs) of a case, CPU tensors.  tiny: B = 2, T = 4, one observed frame per item and, in item 1, one padding frame
    (neither observed nor latent)."""
    if name == "sweep":
        from config_sweep_cases import case, oracle_kw
        k = case(SWEEP_TAG)
        return k["c"]["x"], k["t"], oracle_kw(k["c"])
    B, T = (2, 4) if name == "tiny" else (1, 3)
    g = torch.Generator().manual_seed(17 if name == "tiny" else 18)
    x0 = torch.rand(B, T, 3, 32, 32, generator=g) * 2 - 1
    obs = torch.zeros(B, T, 1, 1, 1)
    obs[:, :1] = 1
    lat = 1 - obs
    if name == "tiny":
        lat[1, T - 1] = 0
    x0 = x0 * obs
    x = torch.randn(B, T, 3, 32, 32, generator=g)
    fidx = torch.arange(T).view(1, T).repeat(B, 1) * 2
    kw = dict(x0=x0, obs_mask=obs, latent_mask=lat, kinda_marg_mask=torch.zeros(B, T, 1, 1, 1), frame_indices=fidx,
              observed_frames="x_0", x_t_minus_1=x0)
    return x, torch.tensor([7] * B), kw


def _specs(name):
    if name == "sweep":
        from config_sweep_cases import case
        return case(SWEEP_TAG)["specs"]
    import video_diffusion_amd as vda
    cfg = model_cfg(name)
    model, _ = vda.create_video_model_and_diffusion(**{k: cfg[k] for k in _defaults().keys()})
    return model.param_specs()


@functools.lru_cache(maxsize=None)
def oracle(name, adaptive=None):
    """SamplerRef over the case's network on the closed-form weights: adaptive None = the plain UNetRef, False / True = FreeUNetRef."""
    cfg = model_cfg(name)
    sd = synth_sd(_specs(name))
    net = UNetRef(cfg, sd) if adaptive is None else FreeUNetRef(cfg, sd, B_CONST, S_CONST, adaptive)
    sched = ScheduleRef(cfg["diffusion_steps"], cfg["noise_schedule"], cfg["timestep_respacing"], cfg["sigma_small"], cfg["rescale_timesteps"])
    return SamplerRef(sched, net)


@functools.lru_cache(maxsize=None)
def oracle_eps(name, adaptive=None, zero_obs=False):
    x, t, kw = window(name)
    if zero_obs:
        kw = dict(kw, obs_mask=torch.zeros_like(kw["obs_mask"]))
    return oracle(name, adaptive).eps(x, t, kw)


# A window whose stage-2 blocks take the engine's OTHER ResBlock forms: 32 items of 4 frames at 64 x 64 are 128 frames, so the 1x1 skip
# convolution of a 16 x 16 block with 192 channels out has 256 x 2 = 512 tiles of 128 x 128 and runs on that tile, where it writes the
# block's activation image itself and the first GroupNorm's (A, B) pairs -- and with them the statistics of the modified halves -- are
# folded ahead of it, outside the transient the small models fold them in.  Items do not interact, so the oracle runs on two of them.
WIDE_B, WIDE_ITEMS = 32, (0, 31)


@functools.lru_cache(maxsize=None)
def wide_window():
    B, T = WIDE_B, 4
    g = torch.Generator().manual_seed(19)
    x0 = torch.rand(B, T, 3, 64, 64, generator=g) * 2 - 1
    obs = torch.zeros(B, T, 1, 1, 1)
    obs[:, :1] = 1
    x0 = x0 * obs
    x = torch.randn(B, T, 3, 64, 64, generator=g)
    kw = dict(x0=x0, obs_mask=obs, latent_mask=1 - obs, kinda_marg_mask=torch.zeros(B, T, 1, 1, 1),
              frame_indices=torch.arange(T).view(1, T).repeat(B, 1), observed_frames="x_0", x_t_minus_1=x0)
    return x, torch.tensor([6] * B), kw


@functools.lru_cache(maxsize=None)
def wide_oracle_eps(adaptive=None):
    """eps of the items WIDE_ITEMS of the wide window."""
    x, t, kw = wide_window()
    pick = list(WIDE_ITEMS)
    sub = {k: (v[pick] if torch.is_tensor(v) else v) for k, v in kw.items()}
    return oracle("w64_s64", adaptive).eps(x[pick], t[pick], sub)
