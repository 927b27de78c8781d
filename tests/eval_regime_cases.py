"""Inputs of the evaluation kernels' launch-regime tests, shared by tests/test_eval_regimes_cpu.py (which keeps them honest without a
GPU) and the GPU tests in tests/test_gpu_metrics.py and tests/test_gpu_lpips.py.

  * WIDE_CASES: frame sizes at which `vd_frame_metrics` leaves the full 32-row strip (W >= 240), and `check_wide_plan`, the
    properties of the launch plan (`vd_frame_metrics_plan`) that prove which regime a case ran.
  * `lpips_chunk_restated`: the frames per pass of `vd_lpips_embed`, from `lpips.layer_sizes`.
  * `zero_norm_weights` / `zero_norm_frames` / `zero_vector_masks`: frames with pixels whose feature vector is all zero at every tap.
  * `int_embeddings`: integer-valued embeddings whose squared distances are exact in float32.
"""
import torch

from lpips_restated import SHIFT, synth_weights, taps_restated
from video_diffusion_amd.lpips import layer_sizes

# (H, W): one strip with one output row; one strip per output row; the same at an odd width; the last width of the 32-row strip and
# the first below it; a short last strip with threads walking two columns; an odd width whose plane is no multiple of 4 floats
WIDE_CASES = [(7, 1024), (12, 1024), (9, 1023), (40, 239), (40, 240), (70, 300), (60, 263)]
WIN = 7
THREADS = 256
LDS_TILE_BYTES = 60 * 1024


def check_wide_plan(H, W, rows_tile, nstrips, groups):
    """The regime of a wide case, as properties of the plan."""
    if W == 239:
        assert rows_tile == 32, (H, W, rows_tile)                          # the boundary pair: the last full tile ...
    if W == 240:
        assert rows_tile < 32, (H, W, rows_tile)                           # ... and the first shrunken one
    if W >= 1023:
        assert rows_tile == WIN and nstrips == H - (WIN - 1), (H, W, rows_tile, nstrips)     # one strip per output row
    if (H, W) != (7, 1024):
        assert nstrips > 1, (H, W, nstrips)
    if W >= 263:
        assert W - (WIN - 1) > THREADS and groups == 1, (H, W, groups)     # every thread walks more than one column
    # what any plan must satisfy: the window fits a strip, both planes of a strip fit the tile, the strips cover the output rows once
    assert WIN <= rows_tile <= 32 and groups >= 1
    assert 2 * 4 * ((rows_tile * W + 3) // 4 * 4) <= LDS_TILE_BYTES
    step = rows_tile - (WIN - 1)
    assert (nstrips - 1) * step < H - (WIN - 1) <= nstrips * step


def lpips_chunk_restated(H, W):
    """Frames per pass of vd_lpips_embed: 2^26 workspace floats over the per-frame activations a1 | p1 | a2 | p2 | a3 | a4 | a5, at most
    65535 (the tap kernel's grid.y), at least 1."""
    (h1, w1), (h2, w2), (h3, w3) = layer_sizes(H, W)[:3]
    per = h1 * w1 * 64 + h2 * w2 * (64 + 192) + h3 * w3 * (192 + 384 + 256 + 256)
    return max(1, min(65535, (1 << 26) // per))


def zero_norm_weights():
    """The synthetic weights with every conv bias replaced by -|bias|: a pixel whose receptive field is the ScalingLayer's shift colour
    (zero after the layer) gets only its bias, and ReLU leaves nothing."""
    w = synth_weights(0)
    for k in range(1, 6):
        w[f"conv{k}.bias"] = -w[f"conv{k}.bias"].abs()
    return w


# (W, flat, taps of frame 0 that hold all-zero AND non-zero vectors).  A tap's pixel is zero when its whole receptive field is flat: conv1
# column x reads input columns 4x - 2 .. 4x + 8, each pool column j its input's 2j .. 2j + 2, conv2 column j its input's j - 2 .. j + 2, conv3..5
# j - 1 .. j + 1.  Column 0 of taps 1..5 so needs input columns up to 8, 32, 64, 80, 96 flat.  At 64 x 64 with 40 flat columns taps 1 and 2 have
# zero vectors; taps 3..5 (3 x 3 maps whose every pixel sees the noise) cannot have one next to a non-zero one at any flat width, so
# the 64 x 192 frames with 100 flat columns are there for them.
ZERO_NORM_CASES = [(64, 40, (1, 2)), (192, 100, (1, 2, 3, 4, 5))]


def zero_norm_frames(W=64, flat=40):
    """(2, 3, 64, W) float32: frame 0 is the shift colour in columns 0..flat-1 and noise in the rest, frame 1 the shift colour everywhere."""
    x = torch.tensor(SHIFT, dtype=torch.float32).view(1, 3, 1, 1).repeat(2, 1, 64, W)
    x[0, :, :, flat:] = torch.rand(3, 64, W - flat, generator=torch.Generator().manual_seed(77)) * 2 - 1
    return x


def zero_vector_masks(frames, w):
    """Per tap, (N, h*w) bool: the pixels whose fp64 feature vector is all zero; and whether every feature is finite."""
    taps = taps_restated(frames, w)
    return [(a == 0).all(dim=1).reshape(a.shape[0], -1) for a in taps], all(bool(torch.isfinite(a).all()) for a in taps)


INT_D, INT_MAX = 64, 8


def int_embeddings(ncand, seed, B=2):
    """(B, ncand, 64) float64 with integer entries in [-8, 8]; item b > 0 is a permutation of item 0's candidates.  A squared distance is
    an integer of at most 64 * 16^2 = 16384 < 2^24, so every partial sum is exact in float32 whatever its order."""
    g = torch.Generator().manual_seed(seed)
    e0 = torch.randint(-INT_MAX, INT_MAX + 1, (ncand, INT_D), generator=g).to(torch.float64)
    return torch.stack([e0] + [e0[torch.randperm(ncand, generator=g)] for _ in range(B - 1)])
