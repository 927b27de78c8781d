"""The spatial GroupNorm path of csrc/norm.hip restated from exact sums, with rounding-count bounds and a line-by-line emulation.

What is restated: GroupNorm32 with eps 1e-5 (nn.py:15-17) on an NHWC frame, optionally followed by FiLM,
`h * (1 + scale) + shift` (unet.py:185-198), optionally by SiLU:

    mean, var of each (frame, group) over HW x C/32 values;  rstd = 1 / sqrt(var + eps)
    A = rstd gamma (1 + scale),  B = (beta - mean rstd gamma)(1 + scale) + shift,  y = silu?(x A + B)

THE REFERENCE.  The kernels' statistics are fp64 themselves, so an fp64 sum cannot judge them.  Every sum here is taken with
math.fsum on the fp32 values (the exact sum, rounded once), and the rounding of that result is recovered with a second fsum
(`exact_sum` returns hi + lo, exact to about 2^-106 of the sum).  A square of an fp32 value is exact in fp64, so the same holds
for the sums of squares.  mean and var are formed from those sums in rational arithmetic (fractions.Fraction: no cancellation
error in E[x^2] - E[x]^2), then rstd, A, B and y in numpy's long double (64-bit significand; asserted), whose own roundings
(2^-64) are 2^-11 of the `u` the bounds count in.

THE BOUNDS.  u = 2^-53 (fp64), e = 2^-24 (fp32); first order in both; nothing in them is measured.
  Table entry of a pixel range of m rows (gn_stats_partial: each term converted to fp64 exactly, its square exact, m - 1 fp64
  additions in whatever order, each off by at most u times a partial sum that is at most the sum of magnitudes):
        |d Sx| <= (m-1) u S|x|            |d Sxx| <= (m-1) u Sxx             (an empty range writes exact zeros)
  Group of m = cnt = HW C/32 terms (the range sums, then the lanes, then the channels: m - 1 additions in all, any order):
        dmean = (m+1) u S|x| / cnt
              the m - 1 additions, the division, and one u to spare
        dvar  = (m+4) u (Sxx/cnt + 2 |mean| S|x|/cnt)
              Sxx/cnt: m - 1 additions + the division; mean^2: 2 |mean| dmean + the product's rounding u mean^2 <= u |mean| S|x|/cnt;
              the subtraction u var <= u Sxx/cnt
        rho   = dvar / (2 (var + eps)) + 4u + e
              relative error of the fp32 rstd: d(var+eps)^-1/2 to first order -- hence the CONDITION dvar <= 0.01 (var + eps),
              asserted on every input; + eps, sqrt, 1/x at u each (the first halved by the square root: 2.5 u, 4 u allowed);
              the cast to fp32, e
  Without FiLM (A = fl(rstd32 gamma), B = fl(beta - fl(mean32 A))):
        |dA| <= |A| (rho + e)
        |dB| <= |mean A| (rho + 3e) + dmean |A| + e (|beta| + |mean A|)
              mean A: A's rho + e, the cast of mean e, the product e; the error of the mean itself dmean |A|; the subtraction's
              rounding e |B| <= e (|beta| + |mean A|)
  With FiLM (sc = fl(1 + scale), A = fl(A0 sc), B = fl(fl(B0 sc) + shift)):
        |dA| <= |A| (rho + 3e)                                     A0's rho + e, sc e, the product e
        |dB| <= |sc| dB0 (1 + 2e) + 3e |B0 sc| + e |shift|          sc e, the product e, the sum e (|B0 sc| + |shift|)
  mr_out (what the backward pass reads):  mean to dmean + e |mean|,  rstd to rho rstd
  y = fl(fl(x A) + B) (or one fma):
        |dy| <= |x| dA + dB + 2e (|x A| + |B|)                      the product e |x A|, the sum e |y| <= e (|x A| + |B|)
        with SiLU: 1.1 times that (|silu'| <= 1.1) + SILU_TOL (1 + |silu|), the project's bound on silu_f (conv_gemm_cases.py)
  affine_act_kernel alone is given A and B: the same with dA = dB = 0.
  EXACT DATA (the dyadic and the constant family: every partial sum is a multiple of 2^-12 below 2^53 2^-12, so no addition
  rounds): tables are compared for equality, and the group bounds are evaluated with m = 0.

THE EMULATION (`emulate_*`) follows the three kernels line by line in numpy: fp64 running sums per pixel lane and range, the
lanes in ascending order, the table walks of gn_final_affine_kernel (eight lanes, four accumulators, the xor butterfly) and of
affine_act_fold_kernel (pixel lanes, then channels ascending), then the fp32 fold in the kernels' order.  test_gn_spatial_cpu.py
holds it to the bounds on every GPU case, so a GPU failure points at a kernel and not at the yardstick.
"""
import functools
import math
from fractions import Fraction
from typing import NamedTuple

import numpy as np
import torch

from conv_gemm_cases import SILU_TOL

U = 2.0 ** -53
E = 2.0 ** -24
EPS = 1e-5
LD = np.longdouble
SENTINEL = -7.5e8


# ---------------------------------------------------------------------------------------------------- cases
class Data(NamedTuple):
    N: int
    HW: int
    C0: int
    C1: int            # 0: no concat
    family: str        # n01 | m30 | dyadic | const

    @property
    def C(self):
        return self.C0 + self.C1

    @property
    def exact(self):
        return self.family in ("dyadic", "const")


class StatsCase(NamedTuple):
    """One vd_op_gn_stats launch over the (virtual concat of the) data at `split` pixel ranges; split 0: the library's choice."""
    data: Data
    split: int


class PipeCase(NamedTuple):
    """Tables per source at their own split -> gn_final_affine (+ mr_out), the folding pass, the activation pass."""
    data: Data
    split0: int
    split1: int
    film: bool


def ppi_of(C):
    return 256 // (C // 4)


# (C0, C1, HW, family, split).  ppi = pixels per iteration of the 256-thread block: 32 at C 32, 10 at 96 (240 threads work), 6 at 160
# (240), 2 at 384 (192), 1 at 672 (168), 896 and 1024.  A lane's unrolled loop takes rows p, p + ppi, .., p + 3 ppi while p + 3 ppi lies
# in the range: ranges of 4 ppi (one trip, no tail), 4 ppi + 1 (lane 0: trip + tail) and 4 ppi - 1 rows (the last lane: no trip), at
# ppi 10 and ppi 1 (where 4 ppi - 1 = 3 rows run no trip at all).  HW 5 at split 4: ranges of 2, 2, 1 and 0 rows.
STATS_CASES = [StatsCase(Data(2, hw, c0, c1, fam), s) for c0, c1, hw, fam, s in [
    (32, 0, 300, "n01", 1), (32, 0, 1024, "m30", 0), (32, 0, 1024, "m30", 4), (1024, 0, 64, "m30", 4), (1024, 0, 64, "n01", 1),
    (96, 0, 5, "n01", 4), (1024, 0, 5, "dyadic", 4),
    (96, 0, 80, "n01", 2), (96, 0, 82, "m30", 2), (96, 0, 78, "dyadic", 2),
    (1024, 0, 8, "dyadic", 2), (1024, 0, 10, "n01", 2), (1024, 0, 6, "m30", 2),
    (160, 0, 64, "n01", 8), (384, 0, 9, "dyadic", 2), (672, 0, 21, "n01", 4), (96, 0, 12, "const", 2),
    (48, 48, 53, "m30", 2), (4, 60, 20, "dyadic", 1), (64, 32, 40, "n01", 4), (512, 384, 24, "n01", 4),
]]

# (C0, C1, HW, family, split0, split1, film).  cg max(split) pairs per group for gn_final_affine's 8-lane, four-in-flight walk: 1, 8, 32,
# 33, 512, 160; 48, 8, 12, 112 with two tables.  The folding pass: blocks of 256 (C 32, 1024), 240 (96, 160), 192 (384), 168 (672) and 224
# (896) threads; split < ppi (C 32, split 1) and > ppi (C 1024, split 16); no head (HW < 4 ppi: C 32 HW 37, C 96 HW 5) and head plus
# tail (C 96 HW 53, C 160 HW 64); a frame cut into 2 blocks (C 32 HW 1024) and into 4 (C 1024 HW 64) -- 8 and 16 in the activation pass.
# Two tables: 16 with 1 and 1 with 4 ranges.  64 + 32 puts group 21 (channels 63 | 64, 65) across the concat, 512 + 384 group 18 (504..511
# | 512..531); 48 + 48 and 4 + 60 end a group at C0, so the next group starts on the second table's first channel.  The sources 48, 4 and
# 60 wide cannot go through vd_op_gn_stats alone (not a multiple of 32): their tables are made by hand from the exact sums; 48 + 48 at
# 16 ranges of 53 pixels has two empty ranges.
PIPE_CASES = [PipeCase(Data(2, hw, c0, c1, fam), s0, s1, film) for c0, c1, hw, fam, s0, s1, film in [
    (32, 0, 1024, "n01", 1, 0, False), (32, 0, 37, "m30", 8, 0, True), (1024, 0, 64, "n01", 1, 0, True),
    (96, 0, 53, "dyadic", 11, 0, False), (1024, 0, 16, "m30", 16, 0, True), (160, 0, 64, "n01", 32, 0, False),
    (96, 0, 5, "m30", 4, 0, False), (384, 0, 9, "dyadic", 2, 0, True), (672, 0, 21, "n01", 4, 0, False), (96, 0, 12, "const", 2, 0, True),
    (48, 48, 53, "m30", 16, 1, True), (4, 60, 20, "dyadic", 1, 4, False), (64, 32, 40, "n01", 4, 2, True),
    (512, 384, 24, "m30", 1, 4, True),
]]


def label(c):
    d = c.data
    ch = f"C{d.C0}" + (f"+{d.C1}" if d.C1 else "")
    if isinstance(c, StatsCase):
        return f"{ch}-HW{d.HW}-{d.family}-split{c.split}"
    return f"{ch}-HW{d.HW}-{d.family}-split{c.split0}" + (f"|{c.split1}" if d.C1 else "") + ("-film" if c.film else "")


# ---------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def make_data(d):
    """x0 [N][HW][C0], x1 [N][HW][C1] or None: fp32, a different draw per frame."""
    g = torch.Generator().manual_seed(7 * d.HW + 13 * d.C0 + 29 * d.C1 + len(d.family))

    def draw(c):
        shape = (d.N, d.HW, c)
        if d.family == "n01":
            return torch.randn(shape, generator=g)
        if d.family == "m30":
            return torch.randn(shape, generator=g) + 30.0
        if d.family == "dyadic":
            return 100.0 + torch.randint(-8, 9, shape, generator=g).float() / 64.0
        assert d.family == "const"
        return torch.full(shape, 3.25)
    return draw(d.C0), (draw(d.C1) if d.C1 else None)


@functools.lru_cache(maxsize=None)
def make_params(d, film):
    """gamma, beta [C]; film [N][film_ld] with scale at +0, shift at +C and film_ld > 2C (the padding is NaN: it must not be read)."""
    g = torch.Generator().manual_seed(1000 + d.C + d.HW)
    gamma, beta = torch.randn(d.C, generator=g) + 1.0, torch.randn(d.C, generator=g)
    if not film:
        return gamma, beta, None, 0
    ld = 2 * d.C + 8
    f = torch.full((d.N, ld), float("nan"))
    f[:, :d.C] = 0.5 * torch.randn(d.N, d.C, generator=g)
    f[:, d.C:2 * d.C] = torch.randn(d.N, d.C, generator=g)
    return gamma, beta, f, ld


def concat(d):
    x0, x1 = make_data(d)
    return (x0 if x1 is None else torch.cat([x0, x1], dim=2)).numpy()


# ---------------------------------------------------------------------------------------------------- exact sums
def exact_sum(vals):
    """hi + lo = the sum of the doubles in `vals` (hi: the exact sum rounded once; lo: what that rounding dropped, rounded once)."""
    hi = math.fsum(vals)
    return hi, math.fsum(vals + [-hi])


class Table(NamedTuple):
    s_hi: np.ndarray       # [N][split][C]   sum x
    s_lo: np.ndarray
    ss_hi: np.ndarray      #                 sum x^2
    ss_lo: np.ndarray
    sabs: np.ndarray       #                 sum |x|
    rows: np.ndarray       # [split]         rows of each pixel range

    def part(self):
        """The table as the kernels store it, every entry the exact sum rounded once: [N][split][C][2] doubles."""
        return np.stack([self.s_hi, self.ss_hi], axis=-1)


def ranges(HW, split):
    per = (HW + split - 1) // split
    return [(min(HW, r * per), min(HW, (r + 1) * per)) for r in range(split)]


def exact_table_of(x, split):
    """x [N][HW][C] fp32 -> the exact per-(frame, pixel range, channel) sums."""
    N, HW, C = x.shape
    x64 = x.astype(np.float64)
    out = [np.zeros((N, split, C)) for _ in range(5)]
    rg = ranges(HW, split)
    for n in range(N):
        for r, (a, b) in enumerate(rg):
            if b <= a:
                continue
            cols = x64[n, a:b].T.tolist()
            for c, v in enumerate(cols):
                out[0][n, r, c], out[1][n, r, c] = exact_sum(v)
                out[2][n, r, c], out[3][n, r, c] = exact_sum([t * t for t in v])          # exact products of fp32 values
                out[4][n, r, c] = math.fsum([abs(t) for t in v])
    return Table(*out, np.array([b - a for a, b in rg]))


@functools.lru_cache(maxsize=None)
def exact_table(d, split, source=-1):
    """source -1: the virtual concat; 0 / 1: one source alone."""
    x = concat(d) if source < 0 else make_data(d)[source].numpy()
    return exact_table_of(x, split)


def table_bounds(t, exact):
    """(bound on sum x, bound on sum x^2) per entry; zero where the sums are exact."""
    m = np.zeros_like(t.rows) if exact else np.maximum(t.rows - 1, 0)
    m = m.reshape(1, -1, 1).astype(np.float64)
    return m * U * t.sabs, m * U * t.ss_hi


def table_errors(part, t):
    """|part - exact| per entry, through hi and lo: (got - hi) is exact for doubles this close."""
    part = np.asarray(part, dtype=np.float64)
    return np.abs((part[..., 0] - t.s_hi) - t.s_lo), np.abs((part[..., 1] - t.ss_hi) - t.ss_lo)


# ---------------------------------------------------------------------------------------------------- the reference
def _ld(fr):
    """A Fraction to long double through hi + lo."""
    hi = float(fr)
    return LD(hi) + LD(float(fr - Fraction(hi)))


class Ref(NamedTuple):
    mean: np.ndarray       # [N][32] long double
    var: np.ndarray
    rstd: np.ndarray
    dmean: np.ndarray      # [N][32] float64 bounds
    dvar: np.ndarray
    rho: np.ndarray
    A: np.ndarray          # [N][C] long double
    B: np.ndarray
    dA: np.ndarray         # [N][C] float64 bounds
    dB: np.ndarray


@functools.lru_cache(maxsize=None)
def group_stats(d):
    """(mean, var, S|x|/cnt, Sxx/cnt) per (frame, group): from exact sums, in rational arithmetic."""
    assert np.finfo(LD).nmant >= 63, "the reference needs an extended-precision long double"
    x64 = concat(d).astype(np.float64)
    N, HW, C = x64.shape
    cg, cnt = C // 32, HW * (C // 32)
    mean, var = np.zeros((N, 32), LD), np.zeros((N, 32), LD)
    aabs, asq = np.zeros((N, 32)), np.zeros((N, 32))
    for n in range(N):
        for g in range(32):
            v = x64[n, :, g * cg:(g + 1) * cg].ravel().tolist()
            s, ss = exact_sum(v), exact_sum([t * t for t in v])
            m = (Fraction(s[0]) + Fraction(s[1])) / cnt
            va = max((Fraction(ss[0]) + Fraction(ss[1])) / cnt - m * m, Fraction(0))
            mean[n, g], var[n, g] = _ld(m), _ld(va)
            aabs[n, g], asq[n, g] = math.fsum([abs(t) for t in v]) / cnt, ss[0] / cnt
    return mean, var, aabs, asq


@functools.lru_cache(maxsize=None)
def reference(d, film):
    mean, var, aabs, asq = group_stats(d)
    C, cg = d.C, d.C // 32
    m = 0 if d.exact else d.HW * cg
    rstd = 1 / np.sqrt(var + LD(EPS))
    mean64, var64 = mean.astype(np.float64), var.astype(np.float64)
    dmean = (m + 1) * U * aabs
    dvar = (m + 4) * U * (asq + 2 * np.abs(mean64) * aabs)
    assert bool((dvar <= 0.01 * (var64 + EPS)).all()), "outside the first-order form: dvar > 0.01 (var + eps)"
    rho = dvar / (2 * (var64 + EPS)) + 4 * U + E
    gamma, beta, f, _ = make_params(d, film)
    gamma, beta = gamma.numpy().astype(LD), beta.numpy().astype(LD)
    ch = np.arange(C) // cg
    A0 = rstd[:, ch] * gamma                           # [N][C]
    mA = mean[:, ch] * A0
    B0 = beta - mA
    a0, ma, b0 = (np.abs(t).astype(np.float64) for t in (A0, mA, B0))
    dB0 = ma * (rho[:, ch] + 3 * E) + dmean[:, ch] * a0 + E * (np.abs(beta).astype(np.float64) + ma)
    if f is None:
        return Ref(mean, var, rstd, dmean, dvar, rho, A0, B0, a0 * (rho[:, ch] + E), dB0)
    sc = 1 + f[:, :C].numpy().astype(LD)
    sh = f[:, C:2 * C].numpy().astype(LD)
    A, B = A0 * sc, B0 * sc + sh
    asc = np.abs(sc).astype(np.float64)
    dA = np.abs(A).astype(np.float64) * (rho[:, ch] + 3 * E)
    dB = asc * dB0 * (1 + 2 * E) + 3 * E * b0 * asc + E * np.abs(sh).astype(np.float64)
    return Ref(mean, var, rstd, dmean, dvar, rho, A, B, dA, dB)


def silu_ld(v):
    return v / (1 + np.exp(-v))


def y_reference(x, A, B, dA, dB, act):
    """x [N][HW][C] fp32; A, B [N][C] long double; dA, dB their bounds (zeros: A and B are given).  -> (y long double, bound float64)."""
    xl = x.astype(LD)
    xa = xl * A[:, None, :]
    lin = xa + B[:, None, :]
    bound = np.abs(x.astype(np.float64)) * dA[:, None, :] + dB[:, None, :] \
        + 2 * E * (np.abs(xa) + np.abs(B)[:, None, :]).astype(np.float64)
    if not act:
        return lin, bound
    y = silu_ld(lin)
    return y, 1.1 * bound + SILU_TOL * (1 + np.abs(y).astype(np.float64))


def worst(got, want, bound):
    """max err / bound over the elements (0 / 0 counts as 0: an exact value under a zero bound)."""
    err = np.abs(np.asarray(got).astype(LD) - want).astype(np.float64)
    bound = np.broadcast_to(bound, err.shape)
    r = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1e-300))
    return float(r.max())


def pipe_tables(c, stats=None):
    """The one or two [N][split][Ci][2] tables of a PipeCase: `stats(x, split)` where the source can go through the statistics pass
    alone (a multiple of 32 channels, and stats given), else by hand: every entry the exact sum rounded once."""
    d, out = c.data, []
    for i, (ci, sp) in enumerate(((d.C0, c.split0), (d.C1, c.split1))):
        if ci == 0:
            out.append(None)
        elif stats is not None and ci % 32 == 0:
            out.append(stats(make_data(d)[i], sp))
        else:
            out.append(exact_table(d, sp, i).part())
    return out


# ---------------------------------------------------------------------------------------------------- the emulation
def emulate_stats(x, split, sq32=False, tail_drop_ss=False):
    """gn_stats_partial: thread (pixel lane pl, channel) adds rows p_begin + pl, + ppi, .. of its range in fp64; the block adds the lanes in
    ascending order.  (sq32 / tail_drop_ss: two deliberate mistakes the tests must catch -- the square taken in fp32; the tail loop's last
    row added to the sum but not to the sum of squares.)"""
    N, HW, C = x.shape
    ppi = ppi_of(C)
    x64 = x.astype(np.float64)
    sq = (x * x).astype(np.float64) if sq32 else x64 * x64
    part = np.zeros((N, split, C, 2))
    for n in range(N):
        for r, (a, b) in enumerate(ranges(HW, split)):
            ls, lss = np.zeros((ppi, C)), np.zeros((ppi, C))
            for pl in range(ppi):
                rows = list(range(a + pl, b, ppi))
                ntail = len(rows) % 4                   # the unrolled loop takes four rows while four remain
                for j, p in enumerate(rows):
                    ls[pl] += x64[n, p]
                    if not (tail_drop_ss and ntail and j == len(rows) - 1):
                        lss[pl] += sq[n, p]
            s, ss = np.zeros(C), np.zeros(C)
            for k in range(ppi):
                s += ls[k]
                ss += lss[k]
            part[n, r, :, 0], part[n, r, :, 1] = s, ss
    return part


def _fold32(mean, var, n, C, gamma, beta, f, b_after_sc=False):
    """The fp32 fold both kernels share: mean / rstd cast to fp32, A = rstd gamma, B = beta - mean A, then FiLM."""
    f32 = np.float32
    cg = C // 32
    mf = mean.astype(f32)
    rf = (1.0 / np.sqrt(np.maximum(var, 0.0) + 1e-5)).astype(f32)
    ch = np.arange(C) // cg
    A = rf[ch] * gamma
    B = beta - mf[ch] * A
    if f is not None:
        sc = f32(1.0) + f[n, :C]
        sh = f[n, C:2 * C]
        if b_after_sc:                              # (a deliberate mistake: B from the A that FiLM has already scaled)
            A = A * sc
            B = (beta - mf[ch] * A) * sc + sh
        else:
            A = A * sc
            B = B * sc + sh
    return A.astype(f32), B.astype(f32), mf, rf


def emulate_final_affine(part0, split0, C0, part1, split1, C, HW, gamma, beta, film, swap_split=False):
    """gn_final_affine_kernel: a group's cg x max(split) pairs dealt to 8 lanes, four accumulators per lane, (a0 + a1) + (a2 + a3), the xor
    butterfly 4, 2, 1 -> A, B [N][C], mr [N][32][2].  (swap_split: split0 used for the second table, a deliberate mistake.)"""
    N = part0.shape[0]
    cg, smax, cnt = C // 32, max(split0, split1), float(HW * (C // 32))
    items = cg * smax
    gamma, beta = gamma.numpy(), beta.numpy()
    f = None if film is None else film.numpy()
    A, B, mr = np.zeros((N, C), np.float32), np.zeros((N, C), np.float32), np.zeros((N, 32, 2), np.float32)
    for n in range(N):
        mean, var = np.zeros(32), np.zeros(32)
        for g in range(32):
            lane = np.zeros((8, 2))
            for ln in range(8):
                acc = np.zeros((4, 2))
                for it in range(ln, items, 32):
                    for u in range(4):
                        j = it + 8 * u
                        ci, sp = divmod(j, smax)
                        c = g * cg + ci
                        second = c >= C0
                        split = (split0 if swap_split else split1) if second else split0
                        if j >= items or sp >= split:
                            continue
                        acc[u] += part1[n, sp, c - C0] if second else part0[n, sp, c]
                lane[ln] = (acc[0] + acc[1]) + (acc[2] + acc[3])
            for o in (4, 2, 1):
                lane = lane + lane[np.arange(8) ^ o]
            mean[g] = lane[0, 0] / cnt
            var[g] = lane[0, 1] / cnt - mean[g] * mean[g]
        A[n], B[n], mr[n, :, 0], mr[n, :, 1] = _fold32(mean, var, n, C, gamma, beta, f)
    return A, B, mr


def emulate_fold_ab(part0, split0, C0, part1, split1, C, HW, gamma, beta, film, skip_first=False, b_after_sc=False):
    """affine_act_fold_kernel's (A, B): thread (pixel lane pl, channel) adds the ranges pl, pl + ppi, ..; the lanes ascending; the group's
    channels ascending.  (skip_first: the second table walked from pl + 1, a deliberate mistake.)"""
    N = part0.shape[0]
    ppi, cg, cnt = ppi_of(C), C // 32, float(HW * (C // 32))
    gamma, beta = gamma.numpy(), beta.numpy()
    f = None if film is None else film.numpy()
    A, B = np.zeros((N, C), np.float32), np.zeros((N, C), np.float32)
    for n in range(N):
        gs = np.zeros((C, 2))
        for tab, split, lo, hi, first in ((part0, split0, 0, C0, 0), (part1, split1, C0, C, 1 if skip_first else 0)):
            if tab is None:
                continue
            lanes = np.zeros((ppi, hi - lo, 2))
            for pl in range(ppi):
                for sp in range(pl + first, split, ppi):
                    lanes[pl] += tab[n, sp]
            for k in range(ppi):
                gs[lo:hi] += lanes[k]
        mean, var = np.zeros(32), np.zeros(32)
        for g in range(32):
            s = ss = 0.0
            for k in range(cg):
                s += gs[g * cg + k, 0]
                ss += gs[g * cg + k, 1]
            mean[g] = s / cnt
            var[g] = ss / cnt - mean[g] * mean[g]
        A[n], B[n], _, _ = _fold32(mean, var, n, C, gamma, beta, f, b_after_sc)
    return A, B


def emulate_apply(x, A, B, act):
    """The pass both activation kernels share: fp32 x A + B, then silu_f = v / (1 + exp(-v)) in fp32."""
    v = x * A[:, None, :] + B[:, None, :]
    assert v.dtype == np.float32
    if act:
        with np.errstate(over="ignore"):                # exp(-v) = inf at v < -88.7: 1 / inf = 0, as v_rcp_f32 gives
            v = v * (np.float32(1.0) / (np.float32(1.0) + np.exp(-v)))
    return v


# ---------------------------------------------------------------------------------------------------- launch geometry
def fold_launch(nfr, HW, C):
    """(threads, blocks per frame, rows per block) of launch_affine_act_fold: what the case list's comments rest on."""
    ppi, split = ppi_of(C), 1
    while nfr * split < 2048 and HW // (split * 2) >= ppi * 16:
        split *= 2
    return ppi * (C // 4), split, (HW + split - 1) // split


def act_launch(nfr, HW, C):
    ppi, split = ppi_of(C), 1
    while nfr * split < 8192 and HW // (split * 2) >= ppi * 4:
        split *= 2
    return ppi * (C // 4), split, (HW + split - 1) // split
