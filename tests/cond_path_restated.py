"""CPU references of the conditioning-path kernels (csrc/misc.hip), for tests/test_gpu_cond_path.py: plain torch, float64 where
arithmetic is involved, exact where the kernel only moves or selects data.  Wherever oracle/unet_ref.py states the operation, the
reference here IS that statement (UNetRef.rpe_R, UNetRef.with_grad, sinus_embedding's argument); tests/test_cond_path_cpu.py
exercises every helper without a GPU."""
import math

import torch
import torch.nn.functional as F

from oracle.unet_ref import UNetRef

# (alpha, beta, gamma) -> {distance d: bucket}: the integer distances at which alpha + log(d / alpha) / log(gamma / alpha) * (beta - alpha)
# is an exact integer before RPE.get_bucket_ids truncates it -- in float32 and in float64 alike.  One ulp low in a device logf selects the
# neighbouring table row there.
EXACT_INTEGER_DISTANCES = {
    (2, 4, 8): {4: 3, 8: 4},
    (4, 8, 16): {8: 6, 16: 8},
    (2, 8, 32): {8: 5, 32: 8},
    (3, 7, 20): {20: 7},
    (4, 12, 256): {32: 8, 256: 12},
    (8, 16, 64): {64: 16},
}
DEGENERATE = (6, 6, 6)                      # alpha == beta == gamma: what every other test of the suite uses
WINDOW = 128                                # longest window of the engine (vd_max_window_frames)

_BASE_CFG = dict(image_size=32, num_channels=32, num_res_blocks=1, num_heads=1, attention_resolutions="16,8")


def ref_net(sd=None, **cfg):
    """A UNetRef that is asked for single statements of the network only (no weights beyond `sd`)."""
    return UNetRef({**_BASE_CFG, **cfg}, sd or {})


# ---------------------------------------------------------------------------------------------- bucket table
def bucket_value(d, al, be, ga, dtype):
    """The value RPE.get_bucket_ids truncates, for a positive distance d > alpha, in the given precision (no minimum, no cast)."""
    x = torch.tensor(float(d), dtype=dtype)
    return (al + torch.log(x / al) / torch.tensor(math.log(ga / al), dtype=dtype) * (be - al)).item()


def bucket_rows_ref(dist, al, be, ga):
    """Table row (0 .. 2 beta, negative ids wrapped as torch indexing wraps them) that UNetRef.rpe_R's table branch selects for every
    entry of the int64 distance tensor `dist` (B, T, T): the branch itself, in CPU float32, on a table whose row i holds i."""
    nb = 2 * int(be) + 1
    net = ref_net({"p.lookup_table_weight": torch.arange(nb, dtype=torch.float32)[:, None]},
                  use_rpe_net=False, rp_alpha=al, rp_beta=be, rp_gamma=ga)
    return net.rpe_R("p", dist, None, 1)[..., 0].long()


def bucket_gather_ref(table, dist, al, be, ga):
    net = ref_net({"p.lookup_table_weight": table}, use_rpe_net=False, rp_alpha=al, rp_beta=be, rp_gamma=ga)
    return net.rpe_R("p", dist, None, table.shape[1])


def covering_fidx(ga):
    """Frame-index rows (B, T <= WINDOW) whose pairwise differences contain every integer in [-(gamma + 3), gamma + 3]: the row
    0 .. gamma + 3 and its reverse, cut into rows that share frame 0 where it is longer than a window."""
    top = int(ga) + 3
    if top + 1 <= WINDOW:
        rows = [list(range(top + 1))]
    else:
        rows = []
        for lo in range(1, top + 1, WINDOW - 1):
            chunk = list(range(lo, min(lo + WINDOW - 1, top + 1)))
            fill = [v for v in range(1, WINDOW) if v not in chunk][:WINDOW - 1 - len(chunk)]      # a short last chunk: any other frames
            rows.append([0] + chunk + fill)
    return torch.tensor(rows + [r[::-1] for r in rows], dtype=torch.int64)


def distances(fidx):
    return fidx.unsqueeze(-1) - fidx.unsqueeze(-2)                      # (B, T, T): fi[b, t] - fi[b, s], as UNetRef.attention


# ---------------------------------------------------------------------------------------------- RPENet hidden layer
def rpe_hidden_ref(te, W, b, fidx):
    """silu(te[b, t] + W . [log(1 + max(d, 0)), log(1 + max(-d, 0)), d == 0] + bias) in float64: te (B, T, C), W (C, 3), b (C,)."""
    d = distances(fidx).double()
    feat = torch.stack([torch.log(1 + d.clamp(min=0)), torch.log(1 + (-d).clamp(min=0)), (d == 0).double()], dim=-1)
    return F.silu(te.double()[:, :, None, :] + feat @ W.double().T + b.double())


# ---------------------------------------------------------------------------------------------- embeddings
def freq_table(half, max_period):
    """The table vd_set_freqs receives (nn.py:99-101 in the reference's own float32 expression)."""
    return torch.exp(-math.log(max_period) * torch.arange(start=0, end=half, dtype=torch.float32) / half).contiguous()


def sinus_ref(t, freqs, dim):
    """float64 cos | sin of the float32 product t * f (one rounding, the same on both sides); zero last column for an odd dim."""
    args = (t[:, None].float() * freqs[None]).double()
    e = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    if dim % 2:
        e = torch.cat([e, torch.zeros_like(e[:, :1])], dim=-1)
    return e


def frame_t_ref(fidx, center):
    fi = fidx.float()
    return fi - fi.mean(dim=1, keepdim=True) if center else fi


# ---------------------------------------------------------------------------------------------- stem assembly
class _StemInput(UNetRef):
    """UNetRef.with_grad up to the call of the network proper: keeps x5, t_frames and the attention mask it was about to hand over."""

    def torso(self, x5, t_frames, fidx, mask, B, T):
        self.seen = (x5, t_frames, mask)
        return torch.zeros(B * T, self.out_ch, x5.shape[2], x5.shape[3])


COND_NAMES = ("channel", "duplicate", "t=0")                             # vd_config::cond_emb_type 0, 1, 2
OBS_NAMES = ("x_0", "x_t", "x_t_minus_1")                                # observed_frames 0, 1, 2


def im2col_k_tap_major(x5, Kpad):
    """(N, Cs, H, W) -> (N, H*W, Kpad): F.unfold's 3x3 patches (k = channel * 9 + tap) reordered to k = tap * Cs + channel, zero-padded."""
    N, Cs, H, W = x5.shape
    cols = F.unfold(x5, 3, padding=1).view(N, Cs, 9, H * W).permute(0, 3, 2, 1).reshape(N, H * W, 9 * Cs)
    return F.pad(cols, (0, Kpad - 9 * Cs))


def assemble_ref(x, x0, xtm1, obs, lat, km, t_model, cond_mode, obs_t_mode, Kpad):
    """x, x0, xtm1 (B, T, 3, H, W); masks (B, T, 1, 1, 1); t_model (B,) -> im2col (B*T, H*W, Kpad), t_frames (B*T,), amask (B*T,)."""
    net = _StemInput({**_BASE_CFG, "cond_emb_type": COND_NAMES[cond_mode]}, {})
    net(x, t_model, x0=x0, obs_mask=obs, latent_mask=lat, kinda_marg_mask=km, observed_frames=OBS_NAMES[obs_t_mode], x_t_minus_1=xtm1)
    x5, t_frames, mask = net.seen
    return im2col_k_tap_major(x5, Kpad), t_frames.float().contiguous(), mask.reshape(-1).float().contiguous()


# ---------------------------------------------------------------------------------------------- posenc / row moves
def posenc_ref(x, P, femb):
    """x (nfr, HW, C) + P (HW, C) + femb (nfr, C), float32, in that order."""
    y = x
    if P is not None:
        y = y + P[None]
    if femb is not None:
        y = y + femb[:, None, :]
    return y


def scatter_stats_ref(src, rows, dst):
    """src (n, split, C, 2) float64 summed over split IN ORDER into dst[rows[i]] (a copy of dst is returned)."""
    out = dst.clone()
    for i, f in enumerate(rows):
        v = torch.zeros_like(src[i, 0])
        for sp in range(src.shape[1]):
            v = v + src[i, sp]
        out[f] = v
    return out
