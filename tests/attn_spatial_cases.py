"""The case table of the spatial-attention per-element tests, its input builder and run_case(): imported by
tests/test_gpu_attn_spatial.py (the test process' own VD_MATH) and by tools/attn_spatial_check.py (a child process per other mode).
Not a test file.

Every case names the (head dim F, waves NW) pair of attn_spatial_split_kernel<F,F16,NW> it is there for (VD_MATH=fp32: attn_spatial_kernel<F>
whatever NW says); vd_attn_spatial_variant() -- the table launch_attn_spatial dispatches through -- must give that name.  N <= 2 and
L <= 320 throughout: a case takes milliseconds on the GPU and its fp64 reference (tests/attn_spatial_restated.py) well under a second.
"""
import ctypes
from collections import namedtuple

import torch

from attn_spatial_restated import attn_ref, row_scale, scaled_errors
from video_diffusion_amd import _lib

MODES = {0: "f16x3", 1: "bf16x6", 2: "fp32"}
HEAD_DIMS = (8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 96, 112, 128)
SENTINEL = -7777.25
FACTOR, FLOOR = 4.0, 2e-6            # e_got <= max(FACTOR e_f32, FLOOR): test_attention_spatial_accuracy_over_magnitudes / test_attention_temporal_per_element

# kind: "plain" | "mags" (query row 3 x 7, row 20 x 1e-2: one 32-query tile) | "hot-first" | "hot-full" | "hot-tail" (one key's k x 40: key 5,
#       a key of the last full tile, the last key -- of the partial last tile where L % 32 != 0) | "zeroq" (query rows 7 and L - 1 are zero) |
#       "samek" (all keys equal) | "aligned" (query row 9 against every key: scores around -1e4) | "range-v" | "range-k" (elements of
#       |x| in [2^15, 7e4] in frame 0, head 0)
# mags: magnitudes of (q, k, v)
# nw:   the NW the case is there for (L <= 64: 2, L <= 128: 4, above: 8 -- stated per case, not computed)
Case = namedtuple("Case", "N L C heads kind mags nw", defaults=("plain", (1.5, 1.5, 1.5), None))


def head_dim(c):
    return c.C // c.heads


def variant_name(c, mode):
    if mode == "fp32":
        return f"attn_spatial_kernel<{head_dim(c)}>"
    return f"attn_spatial_split_kernel<{head_dim(c)},{'true' if mode == 'f16x3' else 'false'},{c.nw}>"


def all_variants(mode):
    """The names of every instantiation of a mode, from the head dims and NW values alone."""
    if mode == "fp32":
        return [f"attn_spatial_kernel<{F}>" for F in HEAD_DIMS]
    return [f"attn_spatial_split_kernel<{F},{'true' if mode == 'f16x3' else 'false'},{nw}>" for F in HEAD_DIMS for nw in (2, 4, 8)]


def label(c):
    s = f"F{head_dim(c)}.NW{c.nw}-N{c.N}L{c.L}h{c.heads}"
    if c.kind != "plain":
        s += f"-{c.kind}"
    if c.mags != (1.5, 1.5, 1.5):
        s += "-mag" + "_".join(f"{m:g}" for m in c.mags)
    return s


# ---- one row per head dim: (F, heads, L at NW = 2 with one key tile, L at NW = 2 with two key tiles, L at NW = 4, L at NW = 8).
# One and two key tiles both need L <= 64, i.e. NW = 2: 52 cases for the 39 (F, NW) pairs.  Per row: one tile (no second prefetch,
# no double buffering), exactly two (stage without prefetch), three or more, and L % 32 = 0, 1 and 31.  Over the rows every L of
#   NW 2: 1, 16, 31, 32, 33, 64    NW 4: 65, 96, 100, 127, 128    NW 8: 129, 255, 256, 257, 290
# L = 257, 290: two blocks along x at NW = 8, the second with seven or more wholly invalid waves.  heads = 2: head 1 starts at F in each third.
VARIANT_ROWS = [
    (8, 2, 1, 64, 127, 257), (16, 1, 16, 33, 128, 255), (24, 2, 31, 64, 65, 290), (32, 1, 32, 33, 127, 256),
    (40, 2, 31, 33, 96, 129), (48, 1, 32, 64, 65, 255), (56, 2, 16, 33, 127, 256), (64, 1, 31, 64, 100, 257),
    (80, 2, 32, 33, 96, 255), (96, 1, 1, 64, 127, 290), (112, 2, 31, 33, 128, 129), (128, 2, 1, 64, 127, 256),
    (72, 2, 31, 33, 100, 257),           # 288 channels on 4 heads: num_channels 96 at its third level
]
VARIANT_CASES = [Case(2, L, F * heads, heads, nw=nw) for F, heads, *Ls in VARIANT_ROWS for L, nw in zip(Ls, (2, 2, 4, 8))]

# The four shapes every operand family runs on: (F, L, NW), heads = 2, N = 2
BASES = [(64, 256, 8), (40, 100, 4), (128, 290, 8), (24, 33, 2)]
MAGS = [(1.0, 1.0, 1.0), (1e-3, 1.0, 1e-3), (30.0, 0.5, 100.0), (1e-6, 1e-6, 1e3), (200.0, 0.05, 1e-4)]     # test_attention_spatial_accuracy_over_magnitudes


def _base(F, L, nw, kind, mags=(1.5, 1.5, 1.5)):
    return Case(2, L, 2 * F, 2, kind, mags, nw)


FAMILY_CASES = [_base(*b, "mags", m) for b in BASES for m in MAGS] + \
    [_base(*b, k) for b in BASES for k in ("hot-first", "hot-full", "hot-tail", "zeroq", "samek", "aligned")]
RANGE_CASES = [_base(*b, k) for b in BASES for k in ("range-v", "range-k")]
CASES = VARIANT_CASES + FAMILY_CASES + RANGE_CASES

# f16x3 only, by label: cases whose excess over the bound was traced to the documented 22-bit operands (test_gpu_attn_spatial.py's
# docstring has the derivation and the measured figures).  bf16x6 and fp32 get none.
F16X3_ALLOWANCE_LABELS = frozenset({"F24.NW2-N2L33h2-hot-first"})


def range_keys(L):
    """The keys that carry out-of-range elements: key 2, and the last two keys (the partial last tile where L % 32 != 0)."""
    return (2, L - 2, L - 1)


def make_inputs(c):
    """qkv [N][L][3C] on the CPU, float32."""
    N, L, C, heads, Fd = c.N, c.L, c.C, c.heads, head_dim(c)
    g = torch.Generator().manual_seed(100000 * heads + 1000 * L + C)
    q, k, v = (torch.randn(N, L, C, generator=g) * m for m in c.mags)
    kind = c.kind
    if kind == "mags":
        q[:, 3] *= 7.0
        q[:, 20] *= 1e-2
    elif kind.startswith("hot-"):
        key = {"hot-first": 5, "hot-full": (L // 32) * 32 - 3, "hot-tail": L - 1}[kind]
        k[:, key] *= 40.0
    elif kind == "zeroq":
        q[0, 7] = 0.0
        q[1, L - 1] = 0.0
    elif kind == "samek":
        k[:] = k[:, :1]
    elif kind == "aligned":
        # every key's features take the signs of one pattern s, query row 9 is -A s: score_j = -A F^-0.5 sum_f |k_jf|, about -1e4
        s = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
        k = k.abs() * s
        q[0, 9] = -(1e4 / (1.2 * Fd ** 0.5)) * s
    elif kind in ("range-v", "range-k"):
        t = v if kind == "range-v" else k
        k2, k1, k0 = range_keys(L)
        t[0, k2, 1] = 40001.3                      # beyond 2^15, yet its scaled remainder (1.3 x 4096) stays inside fp16: f16x3 may carry it
        t[0, k1, 0] = 32768.0 + 15.998             # the remainder times 2^12 rounds to fp16's infinity
        t[0, k0, Fd - 1] = -7.0e4                  # beyond fp16 itself
        t[0, k0, 3] = 32768.0                      # 2^15 exactly
    return torch.cat([q, k, v], -1).contiguous()


def variant_of(L, C, heads):
    """(1 = a kernel | 0 = refused, name) from the library's own selection: no launch."""
    buf = ctypes.create_string_buffer(160)
    rc = _lib.lib().vd_attn_spatial_variant(L, C, heads, buf, len(buf))
    assert rc in (0, 1), rc
    return rc, buf.value.decode()


def process_mode():
    return MODES[_lib.lib().vd_math_mode()]


def launch(qkv, N, L, C, heads):
    """vd_op_attn_spatial reading qkv from the middle of a buffer whose margins hold NaN and writing into the middle of a buffer prefilled
    with NaN whose margins (2 C floats on both sides) hold a sentinel: (out [N][L][C] on the device, margins untouched)."""
    nq, mq = N * L * 3 * C, 2 * 3 * C
    src = torch.full((nq + 2 * mq,), float("nan"), device="cuda")
    src[mq:mq + nq] = qkv.reshape(-1).to("cuda")
    n, pad = N * L * C, 2 * C
    buf = torch.full((n + 2 * pad,), float("nan"), device="cuda")
    buf[:pad] = SENTINEL
    buf[pad + n:] = SENTINEL
    out = buf[pad:pad + n].view(N, L, C)
    _lib.check(_lib.lib().vd_op_attn_spatial(_lib.ptr(src[mq:]), N, L, C, heads, _lib.ptr(out), _lib.current_stream()))
    torch.cuda.synchronize()
    untouched = bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + n:] == SENTINEL).all())
    return out, untouched


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run_case(c):
    """Launch a case in the process' own mode and measure it: a dict of plain numbers, strings and booleans (one JSON line of the tool)."""
    N, L, C, heads, Fd = c.N, c.L, c.C, c.heads, head_dim(c)
    mode = process_mode()
    rc, name = variant_of(L, C, heads)
    qkv = make_inputs(c)
    out, untouched = launch(qkv, N, L, C, heads)
    got = out.cpu()
    ref = attn_ref(qkv, N, L, C, heads)
    f32 = attn_ref(qkv, N, L, C, heads, dtype=torch.float32)
    S = row_scale(qkv, N, L, C, heads)
    e = scaled_errors(got, ref, S)                                                      # [N][L][heads][F]
    fin = torch.isfinite(got).reshape(N, L, heads, Fd)
    e_f32 = float(scaled_errors(f32, ref, S).max())
    r = {"label": label(c), "kind": c.kind, "variant": name, "variant_rc": rc, "expected_variant": variant_name(c, mode), "mode": mode,
         "finite": bool(fin.all()), "e_got": float(e.max()) if bool(fin.all()) else float("nan"), "e_f32": e_f32,
         "margins_untouched": untouched}
    # sum_f |q'_f k_f| at its largest (query, key): the scale of a score's own rounding (the f16x3 allowance reads it)
    x = qkv.double().reshape(N, L, 3, heads, Fd).permute(2, 0, 3, 1, 4).abs()
    r["qk_abs_max"] = float((x[0] * Fd ** -0.5 @ x[1].transpose(-1, -2)).max())
    again, ok2 = launch(qkv, N, L, C, heads)
    r["rerun_same_bits"] = ok2 and same_bits(again, out)
    if N > 1:
        one, ok1 = launch(qkv[N - 1:].contiguous(), 1, L, C, heads)
        r["last_frame_alone_same_bits"] = ok1 and same_bits(one[0], out[N - 1])
    if c.kind.startswith("range-"):
        clean = torch.ones(N, L, heads, dtype=torch.bool)
        clean[0, :, 0] = False                                                          # everything but (frame 0, head 0)
        r["nonfinite"] = int((~fin).sum())
        r["e_finite"] = float(e[fin].max()) if bool(fin.any()) else 0.0                 # over the elements that are numbers
        r["clean_finite"] = bool(fin[clean].all())
        r["e_clean"] = float(e[clean].max()) if r["clean_finite"] else float("nan")     # frame 1 and head 1
    return r


def bound(r):
    b = max(FACTOR * r["e_f32"], FLOOR)
    if r["mode"] == "f16x3" and r["label"] in F16X3_ALLOWANCE_LABELS:
        b += 2.0 ** -21 * (1.0 + 2.0 * r["qk_abs_max"])
    return b


def failures(r):
    """What a measured case (run_case's dict, or a line of the tool) fails: a list of strings, empty if it passes."""
    bad = []
    b = bound(r)
    if r["variant_rc"] != 1 or r["variant"] != r["expected_variant"]:
        bad.append(f"runs {r['variant']}, the case names {r['expected_variant']}")
    if not r["margins_untouched"]:
        bad.append("the margins around the output were written")
    if not r["rerun_same_bits"]:
        bad.append("a second launch gave other bits")
    if not r.get("last_frame_alone_same_bits", True):
        bad.append("the last frame alone gave other bits")
    if r["kind"].startswith("range-"):
        if not r["e_finite"] <= b:
            bad.append(f"a finite output is wrong: e {r['e_finite']:.3e} > {b:.3e}")
        if not r["clean_finite"]:
            bad.append("a non-finite value outside (frame 0, head 0)")
        elif not r["e_clean"] <= b:
            bad.append(f"frame 1 / head 1: e {r['e_clean']:.3e} > {b:.3e}")
        if r["mode"] != "f16x3" and not r["finite"]:
            bad.append(f"{r['nonfinite']} non-finite outputs in a mode that carries the fp32 range")
    else:
        if not r["finite"]:
            bad.append("non-finite outputs")
        elif not r["e_got"] <= b:
            bad.append(f"e_got {r['e_got']:.3e} > max({FACTOR:g} x e_f32 {r['e_f32']:.3e}, {FLOOR:g}) = {b:.3e}")
    return bad


def case_line(r):
    e_got = r["e_finite"] if r["kind"].startswith("range-") else r["e_got"]
    return f"ATTN_SPATIAL_CASE | {r['label']} | {r['variant']} | {r['mode']} | {e_got:.2e} | {r['e_f32']:.2e}"
