"""GPU: the return_attn_weights kernels of csrc/backward.hip -- attn_temporal_weights_kernel (T <= 32), attn_temporal_weights_long_kernel
(query chunks of 32) and attn_spatial_weights_kernel (query tiles of 16) -- alone, through vd_op_attn_temporal_weights and
vd_op_attn_spatial_weights, per element against the float64 restatement of tests/attn_weights_restated.py.  The case lists and what
each case reaches are in the restated module.  Every output lies between sentinel pads and is prefilled with NaN.

Bound (R.maps_bound): |got - ref| <= max(4 e32, FLOOR) max ref per element, the FLOOR part never above the project's bar for softmax
weights 2e-5 + 1e-4 ref; e32 is the error of the float32 run of the same restatement on the CPU (with one key's logits x40 it is the
whole bound: float32 rounding of logits of several hundred, carried into the exponent), FLOOR is three times the largest error
measured on an MI355X over the file's cases WITHOUT a hot key, relative to max ref:

    kernel family                          measured max |got - ref| / max ref     float32 restatement, max     FLOOR (3 x measured)
    temporal (both kernels), no hot key    1.53e-06 (T 128, F 128, RPE, "half")   1.01e-06                     R.FLOOR_TEMPORAL = 4.6e-6
    temporal, hot key                      3.84e-06 (T 33, F 24: e32 3.60e-06)    3.90e-06                     (4 e32 = 1.4e-5 there)
    spatial, no hot key                    7.84e-07 (L 1024, F 128)               1.80e-06                     R.FLOOR_SPATIAL = 2.4e-6
    spatial, hot key                       1.60e-06 (L 100, F 64: e32 1.29e-06)   1.29e-06                     (4 e32 = 5.2e-6 there)

The kernels' error follows the float32 restatement's case by case (0.4 to 2.5 times e32, 3.6 times in one hot-key case of T = 7
whose e32 is 9.6e-08): __expf and the float32 dot products lose what float32 loses.

Besides the bound: a masked entry is exactly 0, every row sums to 1 within T (L) times the bound, everything is finite and >= 0, the
last item (frame) alone gives the bits it has inside the batch.  Each case prints `ATTN_WEIGHTS_CASE | family | case | err e32 worst
err/bound`."""
import functools

import pytest
import torch

import attn_temporal_restated as RT
import attn_weights_restated as R
from helpers import Guarded
from video_diffusion_amd import _lib

pytestmark = pytest.mark.gpu
SEEN = {}                                      # (family, hot) -> largest err of the cases that ran


def dev(t):
    return None if t is None else t.to("cuda").contiguous()


def run_temporal(qkv, Rk, Rq, m, allow, heads, expect=0):
    B, T, HW, C3 = qkv.shape
    out = Guarded(B * HW, T, T)
    bufs = [dev(qkv), dev(Rk), dev(Rq), dev(m)]
    rc = _lib.lib().vd_op_attn_temporal_weights(*[_lib.ptr(t) for t in bufs], B, T, HW, C3 // 3, heads, allow, _lib.ptr(out.t), _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == expect, _lib.lib().vd_last_error().decode()
    return out


def run_spatial(qkv, heads, expect=0):
    N, L, C3 = qkv.shape
    out = Guarded(N, L, L)
    buf = dev(qkv)
    rc = _lib.lib().vd_op_attn_spatial_weights(_lib.ptr(buf), N, L, C3 // 3, heads, _lib.ptr(out.t), _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == expect, _lib.lib().vd_last_error().decode()
    return out


def check_maps(family, c, hot, got, ref, ref32, floor, rows):
    """The assertions every map shares; returns nothing.  rows: entries per softmax row."""
    got = got.double()
    bound, e32, scale = R.maps_bound(ref, ref32, floor)
    err = float((got - ref).abs().max()) / scale
    worst = float(((got - ref).abs() / bound).max())
    print(f"ATTN_WEIGHTS_CASE | {family}{' hot' if hot else ''} | {R.label(c)} | err {err:.3e} e32 {e32:.3e} worst err/bound {worst:.3f}")
    SEEN[(family, hot)] = max(SEEN.get((family, hot), 0.0), err)
    assert bool((got >= 0).all())
    assert worst <= 1.0, (err, e32, worst)
    assert float((got.sum(-1) - 1.0).abs().max()) <= rows * float(bound.max())


@functools.lru_cache(maxsize=None)
def temporal_reference(c):
    B, T, HW, C, heads, rpe, mask, allow, hot = c
    x = R.temporal_inputs(c)
    return x, R.temporal_maps(*x, allow, B, T, HW, C, heads), R.temporal_maps(*x, allow, B, T, HW, C, heads, dtype=torch.float32)


@pytest.mark.parametrize("c", R.TEMPORAL_CASES, ids=[R.label(c) for c in R.TEMPORAL_CASES])
def test_temporal_maps_per_element(c):
    B, T, HW, C, heads, rpe, mask, allow, hot = c
    (qkv, Rk, Rq, m), ref, ref32 = temporal_reference(c)
    got = run_temporal(qkv, Rk, Rq, m, allow, heads).read()
    check_maps("temporal", c, hot, got, ref, ref32, R.FLOOR_TEMPORAL, T)
    if m is not None:
        masked = ~RT.allowed_pairs(m, allow, B, T)                                       # B T T
        assert masked.any() and bool((got.view(B, HW, T, T)[masked.view(B, 1, T, T).expand(B, HW, T, T)] == 0).all())
    if mask == "allpad" and not allow:                                                   # item 0: only the diagonal is allowed
        assert torch.equal(got.view(B, HW, T, T)[0], torch.eye(T).expand(HW, T, T))
    if B > 1:
        one = run_temporal(qkv[-1:], None if Rk is None else Rk[-1:], None if Rq is None else Rq[-1:], None if m is None else m[-1:],
                           allow, heads).read()
        assert torch.equal(one, got[(B - 1) * HW:])


@functools.lru_cache(maxsize=None)
def spatial_reference(c):
    N, L, C, heads, hot = c
    qkv = R.spatial_inputs(c)
    return qkv, R.spatial_maps(qkv, N, L, C, heads), R.spatial_maps(qkv, N, L, C, heads, dtype=torch.float32)


@pytest.mark.parametrize("c", R.SPATIAL_CASES, ids=[R.label(c) for c in R.SPATIAL_CASES])
def test_spatial_maps_per_element(c):
    N, L, C, heads, hot = c
    qkv, ref, ref32 = spatial_reference(c)
    got = run_spatial(qkv, heads).read()
    check_maps("spatial", c, hot, got, ref, ref32, R.FLOOR_SPATIAL, L)
    if N > 1:
        assert torch.equal(run_spatial(qkv[-1:], heads).read(), got[-1:])


def test_measured_maxima():
    """The figures of the table above, from this run (this test runs after the cases)."""
    print("ATTN_WEIGHTS_MAXIMA | " + " ".join(f"{f}{'_hot' if h else ''} {v:.3e}" for (f, h), v in sorted(SEEN.items()))
          + f" | FLOOR temporal {R.FLOOR_TEMPORAL:.3e} spatial {R.FLOOR_SPATIAL:.3e}")
    assert {f for f, _ in SEEN} == {"temporal", "spatial"}


@pytest.mark.parametrize("T,C,heads,why", [(129, 64, 4, "shape"), (128, 192, 1, "head dim too large"), (32, 1024, 1, "head dim too large"),
                                           (8, 66, 4, "shape")])
def test_temporal_refusals_by_message(T, C, heads, why):
    """More than 128 frames, a head dim whose rows exceed the launcher's 150 KiB of LDS (in either kernel), C not divisible by heads:
    refused by name before any launch."""
    qkv = torch.zeros(1, T, 1, 3 * C)
    out = run_temporal(qkv, None, None, None, 1, heads, expect=-1)
    msg = _lib.lib().vd_last_error().decode()
    assert "temporal attention weights" in msg and why in msg, msg
    assert out.untouched()


@pytest.mark.parametrize("L,C,heads,why", [(16, 12, 2, "shape"), (16, 64, 3, "shape"), (2048, 32, 2, "sequence too long")])
def test_spatial_refusals_by_message(L, C, heads, why):
    """A head dim that is no multiple of 4, C not divisible by heads, and 16 score rows past 150 KiB of LDS: refused by name."""
    qkv = torch.zeros(1, L, 3 * C)
    out = run_spatial(qkv, heads, expect=-1)
    msg = _lib.lib().vd_last_error().decode()
    assert "spatial attention weights" in msg and why in msg, msg
    assert out.untouched()
