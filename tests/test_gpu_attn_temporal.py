"""GPU: every instantiation of the temporal-attention kernels (csrc/attn_temporal.hip: 20 for T <= 32; csrc/attn_temporal_long.hip:
18 for T = 33..128) and the temporal GroupNorm (csrc/norm.hip), element by element against float64.

The attention cases are compared with tests/attn_temporal_restated.py (checked against explicit loops in test_attn_temporal_cpu.py)
in the unit of their own output row -- S = max over the allowed s and the head's features of |v_s + Rv[t,s]| -- so a case whose v
is 1e-3 is held as tightly as one whose v is 100.  vd_attn_temporal_variant() names the instantiation a shape runs on (the
launchers dispatch through the same function): every case states the one it is here for, and the coverage test holds the table
to all 38.
"""
import ctypes
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as F

from attn_temporal_restated import attn_ref, row_scale, scaled_error
from video_diffusion_amd import _lib

pytestmark = pytest.mark.gpu

SENTINEL = -7777.25


# ---------------------------------------------------------------------------------------------------- the case table
# kern: ("M", NT, JM, EXACT) attn_temporal_mfma_kernel | ("V", PB, TMAX) attn_temporal_kernel | ("LM", NJ) attn_temporal_long_mfma_kernel |
#       ("LG",) attn_temporal_long_kernel; the RPE argument of the name is the case's rpe
# mask: None | "diff" (item 0: frames 0 and T//2 are padding; the last item: frame T-1 is -- the masks differ between the items) |
#       "last" (frame T-1 padding: the clamped loads of frames past T alias it) | "first" (frame 0 padding, frame T-1 real) |
#       "one" (exactly one real frame, T//2) | "ones" | "zeros" | "tail" (the last max(1, T//4) frames, at T > 32 the last 20: whole key tiles)
# mags: magnitudes of (q, k, v); Rk, Rq, Rv are scaled like k, q, v
# hot:  None | "first" (key frame min(1, T-1)) | "last" (key frame T-1): that frame's k x 40
# padx: the padding frames' q, k, v are 1e3 times larger; the error is taken over the real frames' rows
Case = namedtuple("Case", "B T HW C heads rpe kern mask allow mags hot padx", defaults=(None, 0, (1.5, 1.5, 1.5), None, False))


def variant_name(c):
    r = "true" if c.rpe else "false"
    k = c.kern
    if k[0] == "M":
        return f"attn_temporal_mfma_kernel<{k[1]},{k[2]},{r},{'true' if k[3] else 'false'}>"
    if k[0] == "V":
        return f"attn_temporal_kernel<{k[1]},{k[2]},{r}>"
    if k[0] == "LM":
        return f"attn_temporal_long_mfma_kernel<{k[1]},{r}>"
    return f"attn_temporal_long_kernel<{r}>"


def label(c):
    s = f"{'.'.join(str(int(x)) if isinstance(x, bool) else str(x) for x in c.kern)}-{'rpe' if c.rpe else 'plain'}-B{c.B}T{c.T}HW{c.HW}F{c.C // c.heads}h{c.heads}"
    if c.mask:
        s += f"-{c.mask}{c.allow}"
    if c.mags != (1.5, 1.5, 1.5):
        s += "-mag" + "_".join(f"{m:g}" for m in c.mags)
    if c.hot:
        s += f"-hot{c.hot}"
    if c.padx:
        s += "-padx"
    return s


M1_4, M1_6X, M1_8X, M1_8, M2_4, M2_8 = ("M", 1, 4, False), ("M", 1, 6, True), ("M", 1, 8, True), ("M", 1, 8, False), ("M", 2, 4, False), ("M", 2, 8, False)
V4_16, V2_16, V4_32, V2_32 = ("V", 4, 16), ("V", 2, 16), ("V", 4, 32), ("V", 2, 32)

VARIANT_CASES = [
    # ---- matrix pipe, T <= 32 (pixels % 16 == 0, F % 16 == 0, F <= 128).  Frame-tile edges T = 1, 3, 4, 5, 12, 13, 15, 16 (F = 32,
    # 80, 112: not the exact shapes), 17, 20, 29, 31, 32
    Case(2, 16, 16, 96, 1, True, M1_6X, "diff", 1),               # the default models' two exact shapes, with and without RPE
    Case(2, 16, 16, 192, 2, False, M1_6X, "last", 0),
    Case(1, 16, 32, 128, 1, True, M1_8X),
    Case(2, 16, 16, 128, 1, False, M1_8X, "diff", 0),
    Case(2, 1, 16, 16, 1, True, M1_4),
    Case(1, 3, 16, 64, 2, True, M1_4, "first", 1),
    Case(1, 4, 48, 32, 2, True, M1_4, "last", 0),                 # three pixel blocks
    Case(2, 5, 32, 64, 1, False, M1_4, "diff", 1),
    Case(1, 16, 16, 32, 1, True, M1_4),                           # T = 16, F = 32
    Case(2, 12, 16, 96, 1, True, M1_8, "diff", 0),                # the default 116 M model at a 12-frame window: 6 of 8 waves in phase B
    Case(1, 15, 16, 80, 1, True, M1_8, "last", 1),
    Case(1, 16, 16, 112, 1, True, M1_8, "first", 0),              # T = 16, F = 112
    Case(2, 13, 16, 128, 1, True, M1_8),
    Case(2, 12, 16, 192, 2, False, M1_8, "last", 1),
    Case(1, 16, 16, 80, 1, False, M1_8, "diff", 0),               # T = 16, F = 80
    Case(2, 17, 16, 16, 1, True, M2_4, "diff", 0),
    Case(1, 32, 16, 64, 1, True, M2_4, "last", 1),
    Case(2, 20, 16, 48, 1, False, M2_4, "diff", 1),
    Case(1, 29, 16, 32, 1, False, M2_4, "last", 0),
    Case(2, 31, 16, 80, 1, True, M2_8, "diff", 1),
    Case(1, 32, 16, 128, 1, True, M2_8),
    Case(1, 17, 16, 96, 1, True, M2_8, "last", 0),
    Case(2, 29, 16, 112, 1, False, M2_8, "first", 0),
    Case(1, 20, 32, 96, 1, False, M2_8, "last", 1),
    # ---- VALU blocks, T <= 32: pixel edges HW = 1, 3, 5, 17 for both PB (ragged last block), head dims 8, 24, 136 (above 128 at
    # pixels % 16 == 0), 272 (the largest accepted at T = 32); PB = 2 where the 4-pixel block's LDS exceeds 96 KB
    Case(2, 13, 5, 48, 2, True, V4_16, "diff", 0),
    Case(1, 1, 1, 8, 1, True, V4_16),
    Case(1, 15, 17, 16, 2, True, V4_16, "last", 1),
    Case(1, 12, 16, 136, 1, True, V4_16, "first", 0),
    Case(2, 4, 3, 16, 2, False, V4_16, "diff", 1),
    Case(1, 16, 17, 24, 1, False, V4_16, "last", 0),
    Case(2, 16, 5, 184, 1, True, V2_16, "diff", 1),
    Case(1, 13, 3, 232, 1, True, V2_16, "last", 0),
    Case(2, 16, 17, 184, 1, False, V2_16, "diff", 0),
    Case(1, 15, 1, 200, 1, False, V2_16),
    Case(2, 20, 5, 48, 2, True, V4_32, "diff", 0),
    Case(1, 32, 17, 8, 1, True, V4_32, "last", 1),
    Case(1, 20, 16, 136, 1, True, V4_32),
    Case(2, 31, 3, 24, 1, False, V4_32, "diff", 1),
    Case(1, 17, 1, 40, 1, False, V4_32, "last", 0),
    Case(2, 32, 5, 80, 1, True, V2_32, "diff", 0),
    Case(1, 20, 17, 144, 1, True, V2_32, "last", 1),
    Case(1, 32, 3, 272, 1, True, V2_32, "first", 0),              # the envelope: about 146 KB of LDS
    Case(2, 29, 3, 96, 1, False, V2_32, "diff", 0),
    Case(1, 32, 1, 272, 1, False, V2_32),
    # ---- long windows: every NJ with and without RPE, and the generic kernel
    Case(2, 33, 16, 16, 1, True, ("LM", 1), "diff", 0),
    Case(1, 40, 16, 16, 1, False, ("LM", 1), "tail", 0),
    Case(1, 48, 16, 32, 1, True, ("LM", 2), "tail", 1),
    Case(2, 33, 16, 64, 2, False, ("LM", 2), "diff", 1),
    Case(2, 40, 16, 48, 1, True, ("LM", 3), "tail", 0),
    Case(1, 64, 16, 48, 1, False, ("LM", 3)),
    Case(1, 97, 16, 64, 1, True, ("LM", 4), "diff", 1),
    Case(2, 48, 32, 64, 1, False, ("LM", 4), "tail", 0),
    Case(2, 33, 16, 80, 1, True, ("LM", 5)),
    Case(1, 128, 16, 80, 1, False, ("LM", 5), "tail", 0),
    Case(1, 40, 16, 96, 1, True, ("LM", 6), "last", 0),
    Case(2, 64, 16, 96, 1, False, ("LM", 6), "diff", 1),
    Case(1, 128, 16, 112, 1, True, ("LM", 7), "tail", 0),
    Case(2, 40, 16, 112, 1, False, ("LM", 7), "diff", 0),
    Case(1, 48, 16, 128, 1, True, ("LM", 8), "diff", 0),
    Case(1, 33, 32, 128, 1, False, ("LM", 8), "last", 1),
    Case(2, 40, 5, 48, 2, True, ("LG",), "tail", 0),
    Case(1, 97, 3, 136, 1, False, ("LG",), "diff", 1),
]

# The four shapes every operand family and mask pattern below runs on: matrix pipe at T <= 16 and at T > 16 (ragged T: clamped frames),
# VALU, long
BASES = [(2, 12, 16, 192, 2, True, M1_8), (2, 20, 16, 64, 2, True, M2_4), (2, 13, 5, 48, 2, True, V4_16), (2, 40, 16, 64, 2, True, ("LM", 2))]
MAGS = [(1e-3, 1.0, 1e-3), (30.0, 0.5, 100.0), (1e-6, 1e-6, 1e3), (8.0, 8.0, 1.0)]               # (1.5, 1.5, 1.5) is the default of every other case
FAMILY_CASES = [Case(*b, "diff", 1, mags=m) for b in BASES for m in MAGS] + \
    [Case(*b, None, 0, hot=h) for b in BASES for h in ("first", "last")] + \
    [Case(*b, "tail", 0, padx=True) for b in BASES]
MASK_CASES = [Case(*b, m, a) for b in BASES for m, a in (("last", 0), ("first", 0), ("last", 1), ("first", 1), ("one", 0), ("one", 1), ("zeros", 0))]
CASES = VARIANT_CASES + FAMILY_CASES + MASK_CASES

# test_gpu_long_window.py's table, case by case
LONG_TABLE_VARIANTS = [
    "attn_temporal_long_mfma_kernel<1,true>", "attn_temporal_long_mfma_kernel<2,true>", "attn_temporal_long_mfma_kernel<6,true>",
    "attn_temporal_long_mfma_kernel<8,true>", "attn_temporal_long_mfma_kernel<2,true>", "attn_temporal_long_mfma_kernel<6,true>",
    "attn_temporal_long_mfma_kernel<8,false>", "attn_temporal_long_mfma_kernel<6,false>", "attn_temporal_long_mfma_kernel<2,false>",
    "attn_temporal_long_mfma_kernel<1,true>", "attn_temporal_long_kernel<true>", "attn_temporal_long_kernel<true>",
    "attn_temporal_long_kernel<true>", "attn_temporal_long_kernel<false>", "attn_temporal_long_kernel<true>",
]

ALL_VARIANTS = [f"attn_temporal_mfma_kernel<{nt},{jm},{r},{x}>" for nt, jm, x in ((1, 6, "true"), (1, 8, "true"), (1, 4, "false"), (1, 8, "false"),
                                                                                (2, 4, "false"), (2, 8, "false")) for r in ("true", "false")] + \
    [f"attn_temporal_kernel<{pb},{tm},{r}>" for pb in (2, 4) for tm in (16, 32) for r in ("true", "false")] + \
    [f"attn_temporal_long_mfma_kernel<{nj},{r}>" for nj in range(1, 9) for r in ("true", "false")] + \
    [f"attn_temporal_long_kernel<{r}>" for r in ("true", "false")]


def variant_of(T, HW, C, heads, rpe):
    """(1 = a kernel | 0 = refused, name) from the library's own selection: no launch."""
    buf = ctypes.create_string_buffer(128)
    rc = _lib.lib().vd_attn_temporal_variant(T, HW, C, heads, int(rpe), buf, len(buf))
    assert rc in (0, 1), rc
    return rc, buf.value.decode()


def test_every_instantiation_is_run_and_every_case_runs_the_one_it_names():
    from test_gpu_long_window import CASES as long_table
    assert len(ALL_VARIANTS) == 38 and len(set(ALL_VARIANTS)) == 38
    assert len(long_table) == len(LONG_TABLE_VARIANTS)
    seen = set()
    for c in CASES:
        rc, name = variant_of(c.T, c.HW, c.C, c.heads, c.rpe)
        assert rc == 1 and name == variant_name(c), (label(c), name)
        assert variant_of(c.T, c.HW, c.C, c.heads, c.rpe) == (rc, name)
        seen.add(name)
    for (B, T, HW, C, heads, rpe, *_), want in zip(long_table, LONG_TABLE_VARIANTS):
        rc, name = variant_of(T, HW, C, heads, rpe)
        assert rc == 1 and name == want, ((B, T, HW, C, heads, rpe), name)
        seen.add(name)
    missing = sorted(set(ALL_VARIANTS) - seen)
    print(f"temporal attention: {len(seen & set(ALL_VARIANTS))} of {len(ALL_VARIANTS)} instantiations run at op level")
    assert not missing and seen <= set(ALL_VARIANTS), (missing, sorted(seen - set(ALL_VARIANTS)))
    assert len(set(label(c) for c in CASES)) == len(CASES)
    assert all(c.B <= 2 and c.HW <= 48 for c in CASES)


# ---------------------------------------------------------------------------------------------------- inputs and the launch
def make_mask(c):
    B, T = c.B, c.T
    if c.mask is None:
        return None
    m = torch.ones(B, T)
    if c.mask == "diff":
        m[0, 0] = 0
        m[0, T // 2] = 0
        m[B - 1, T - 1] = 0
    elif c.mask == "last":
        m[:, T - 1] = 0
    elif c.mask == "first":
        m[:, 0] = 0
    elif c.mask == "one":
        m[:] = 0
        m[:, T // 2] = 1
    elif c.mask == "zeros":
        m[:] = 0
    elif c.mask == "tail":
        m[:, T - (20 if T > 32 else max(1, T // 4)):] = 0
    else:
        assert c.mask == "ones"
    return m


def make_inputs(c):
    """(qkv [B][T][HW][3C], (Rk, Rq, Rv) or Nones, mask or None) on the CPU, float32."""
    B, T, HW, C = c.B, c.T, c.HW, c.C
    g = torch.Generator().manual_seed(1000 * T + 10 * HW + C)
    qm, km, vm = c.mags
    qkv = torch.cat([torch.randn(B, T, HW, C, generator=g) * s for s in (qm, km, vm)], -1)
    R = (None, None, None)
    if c.rpe:
        R = tuple(torch.randn(B, T, T, C, generator=g) * s for s in (km, qm, vm))          # Rk like k, Rq like q, Rv like v
    if c.hot:
        qkv[:, min(1, T - 1) if c.hot == "first" else T - 1, :, C:2 * C] *= 40.0
    m = make_mask(c)
    if c.padx:
        qkv[(m == 0)[:, :, None, None].expand_as(qkv)] *= 1e3
    return qkv.contiguous(), R, m


def launch(qkv, R, m, B, T, HW, C, heads, allow):
    """vd_op_attn_temporal into the middle of a larger buffer: (out [B][T][HW][C] on the device, untouched).  The margins hold a
    sentinel in two rows' worth of floats before and after the output; untouched says whether both still do (stray writes only)."""
    n, pad = B * T * HW * C, 2 * C
    buf = torch.full((n + 2 * pad,), SENTINEL, device="cuda")
    out = buf[pad:pad + n].view(B, T, HW, C)
    _lib.check(_lib.lib().vd_op_attn_temporal(_lib.ptr(qkv), *[_lib.ptr(r) for r in R], _lib.ptr(m), B, T, HW, C, heads, allow,
                                              _lib.ptr(out), _lib.current_stream()))
    torch.cuda.synchronize()
    untouched = bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + n:] == SENTINEL).all())
    return out, untouched


def dev(t):
    return None if t is None else t.to("cuda").contiguous()


@pytest.mark.parametrize("c", [pytest.param(c, id=label(c)) for c in CASES])
def test_attention_temporal_per_element(c):
    """e = max over elements of |out - ref| / S_row against the fp64 restatement; required: e_got <= max(4 e_f32, 2e-6), e_f32 being
    the same measure of a plain fp32 torch-CPU evaluation of the same restatement (factor and floor are those of
    test_attention_spatial_accuracy_over_magnitudes).  The kernels accumulate in fp32 like that evaluation, in another order: no
    term of their own is added to the bound.  Every output is finite, the margins around the output are untouched, and the last
    item of a batch run alone gives the same bits.  Measured figures: docs/LAB_NOTES.md."""
    B, T, HW, C, heads = c.B, c.T, c.HW, c.C, c.heads
    qkv, R, m = make_inputs(c)
    d_qkv, d_R, d_m = dev(qkv), tuple(dev(r) for r in R), dev(m)
    out, untouched = launch(d_qkv, d_R, d_m, B, T, HW, C, heads, c.allow)
    got = out.cpu()
    ref = attn_ref(qkv, *R, m, c.allow, B, T, HW, C, heads)
    f32 = attn_ref(qkv, *R, m, c.allow, B, T, HW, C, heads, dtype=torch.float32)
    S = row_scale(qkv, R[2], m, c.allow, B, T, HW, C, heads)
    rows = (m == 1) if c.padx else None
    finite = bool(torch.isfinite(got).all())
    e_got = scaled_error(got, ref, S, rows) if finite else float("nan")
    e_f32 = scaled_error(f32, ref, S, rows)
    print(f"ATTN_TEMPORAL_CASE | {label(c)} | {variant_name(c)} | {e_got:.2e} | {e_f32:.2e}")
    assert finite
    assert untouched
    assert e_got <= max(4.0 * e_f32, 2e-6), (e_got, e_f32)
    if B > 1:
        one, ok1 = launch(d_qkv[B - 1:].contiguous(), tuple(None if r is None else r[B - 1:].contiguous() for r in d_R),
                          None if d_m is None else d_m[B - 1:].contiguous(), 1, T, HW, C, heads, c.allow)
        assert ok1 and torch.equal(one[0], out[B - 1])


@pytest.mark.parametrize("base", BASES, ids=[label(Case(*b)) for b in BASES])
def test_masks_that_forbid_nothing_give_the_bits_of_no_mask(base):
    """All ones with either allow value, and all zeros with allow = 1 (padding attends padding), forbid no pair: bit-equal to mask = None."""
    c = Case(*base)
    qkv, R, _ = make_inputs(c)
    d_qkv, d_R = dev(qkv), tuple(dev(r) for r in R)
    want, ok = launch(d_qkv, d_R, None, c.B, c.T, c.HW, c.C, c.heads, 0)
    assert ok and bool(torch.isfinite(want).all())
    for fill, allow in ((1.0, 0), (1.0, 1), (0.0, 1)):
        m = torch.full((c.B, c.T), fill, device="cuda")
        got, ok = launch(d_qkv, d_R, m, c.B, c.T, c.HW, c.C, c.heads, allow)
        assert ok and torch.equal(got, want), (fill, allow)


# ---------------------------------------------------------------------------------------------------- the envelope
@pytest.mark.parametrize("T,HW,C,heads,text", [(32, 3, 280, 1, "head dim too large"), (32, 16, 560, 2, "head dim too large"),
                                               (16, 16, 12, 1, "head dim multiple of 8"), (40, 16, 40, 2, "head dim multiple of 8")])
def test_head_dims_outside_the_envelope_are_refused_without_a_launch(T, HW, C, heads, text):
    """T = 32: F = 272 is the largest head dim (VARIANT_CASES runs it), F = 280 needs more than 150 KB of LDS for a 2-pixel block."""
    rc, name = variant_of(T, HW, C, heads, False)
    assert rc == 0 and name.startswith("refused: ") and text in name
    qkv = torch.zeros(1, T, HW, 3 * C, device="cuda")
    with pytest.raises(_lib.VdError, match="head dim"):
        launch(qkv, (None, None, None), None, 1, T, HW, C, heads, 0)
    buf = torch.full((T * HW * C,), SENTINEL, device="cuda")                               # nothing was launched: nothing is written
    rc = _lib.lib().vd_op_attn_temporal(_lib.ptr(qkv), None, None, None, None, 1, T, HW, C, heads, 0, _lib.ptr(buf), _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == -1 and bool((buf == SENTINEL).all())
    assert variant_of(32, 3, 272, 1, True) == (1, "attn_temporal_kernel<2,32,true>")


# ---------------------------------------------------------------------------------------------------- temporal GroupNorm
# (B, T, HW, C, mean, std).  C = 32, 96, 160, 992: channels per group 1, 3, 5, 31 -> the generic kernel (idle threads at 96 and
# 160: 240 of 256 work); 384, 768, 1024 -> the quad kernel (768: one pixel per block, a quarter of it idle); T <= 16 and T > 16 are
# the two TMAX; HW = 1, 5 and one above a multiple of the block's pixel count 256 / (C / 4); the last two are the long form.
GN_CASES = [
    (2, 1, 33, 32, 0.0, 1.0), (2, 16, 11, 96, 30.0, 1.0), (2, 17, 7, 160, 0.0, 1.0), (2, 32, 5, 384, 100.0, 0.01),
    (2, 16, 5, 768, 0.0, 1.0), (2, 17, 1, 992, 30.0, 1.0), (2, 32, 3, 1024, 0.0, 1.0), (2, 1, 5, 1024, 100.0, 0.01),
    (2, 16, 1, 160, 100.0, 0.01), (2, 32, 11, 96, 0.0, 1.0), (2, 17, 3, 384, 30.0, 1.0), (2, 16, 33, 32, 100.0, 0.01),
    (2, 32, 2, 768, 30.0, 1.0), (2, 1, 1, 992, 0.0, 1.0),
    (2, 33, 5, 96, 30.0, 1.0), (1, 128, 3, 384, 100.0, 0.01),
]


@pytest.mark.parametrize("B,T,HW,C,mean,std", GN_CASES)
def test_groupnorm_temporal_per_element(B, T, HW, C, mean, std):
    """GroupNorm32 on the (B*HW, C, T) view (unet.py:472-475) against F.group_norm in fp64, under a bound derived from the kernel's
    arithmetic -- fp64 statistics, then A = rstd*gamma, B = beta - mean*A, y = x*A + B in fp32:

        |got - ref| <= 2^-23 (|x A| + 3 |mean A| + |beta| + |y|)      A, mean, y from the fp64 reference

    (eight fp32 roundings at 2^-24 each: rstd and A on x A; the fp32 mean, rstd, A and the product on mean A; B; y).  Nothing in it
    is measured.  A mean of 100 at std 0.01 keeps its variance only because the sums are fp64."""
    g = torch.Generator().manual_seed(100 * T + C + HW)
    x = torch.randn(B, T, HW, C, generator=g) * std + mean
    gamma, beta = torch.randn(C, generator=g) + 1, torch.randn(C, generator=g)
    n, pad = B * T * HW * C, 2 * C
    buf = torch.full((n + 2 * pad,), SENTINEL, device="cuda")
    y = buf[pad:pad + n].view(B, T, HW, C)
    bufs = [dev(x), dev(gamma), dev(beta)]
    _lib.check(_lib.lib().vd_op_gn_temporal(*[_lib.ptr(b) for b in bufs], B, T, HW, C, _lib.ptr(y), _lib.current_stream()))
    torch.cuda.synchronize()
    assert bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + n:] == SENTINEL).all())
    got = y.cpu().double()
    assert bool(torch.isfinite(got).all())
    xd = x.double().permute(0, 2, 3, 1).reshape(B * HW, C, T)                            # the reference's view
    ref = F.group_norm(xd, 32, gamma.double(), beta.double(), eps=1e-5)
    grp = xd.reshape(B * HW, 32, -1)
    mu = grp.mean(-1, keepdim=True)
    var = ((grp - mu) ** 2).mean(-1, keepdim=True)
    cg = C // 32
    A = ((var + 1e-5).rsqrt().expand(-1, -1, cg).reshape(B * HW, C) * gamma.double()).unsqueeze(-1)     # [B*HW][C][1]
    mu = mu.expand(-1, -1, cg).reshape(B * HW, C, 1)
    bound = 2.0 ** -23 * ((xd * A).abs() + 3 * (mu * A).abs() + beta.double().abs().view(1, C, 1) + ref.abs())
    err = (got.view(B, T, HW, C).permute(0, 2, 3, 1).reshape(B * HW, C, T) - ref).abs()
    worst = float((err / bound).max())
    print(f"GN_TEMPORAL_CASE | B{B} T{T} HW{HW} C{C} mean {mean:g} std {std:g} | max err/bound {worst:.3f}")
    assert worst <= 1.0, worst
