"""The case table of the convolution / linear per-element tests, its input builder and run_case(): imported by
tests/test_gpu_conv_gemm.py (the test process' own VD_MATH) and by tools/conv_gemm_check.py (a child process per other mode).
Not a test file.

Every case states the instantiation it is there for; vd_igemm_variant() -- the tables the launchers of csrc/igemm.hip, gemm_split.hip,
gemm_frag.hip, conv_wino.hip, conv_wino_r64.hip and conv_wino_z128.hip dispatch through -- must give that name, and the cases of a mode
must cover every name of vd_igemm_variant_list().  Activations are NHWC; a linear layer of M rows is N = M frames of H = 1.

The bound (tests/test_gpu_conv_gemm.py has the derivation): e = max over the elements of |got - ref64| / S, S the sum of the absolute
values of the element's own terms (S_w, the same through the Winograd transforms, for the Winograd kernels); e_got <= max(4 e_f32, FLOOR).
"""
import ctypes
import zlib
from collections import namedtuple

import torch

from conv_gemm_restated import conv_ref, gn_block_sums, operand, silu, wino_ref
from video_diffusion_amd import _lib

MODES = {0: "f16x3", 1: "bf16x6", 2: "fp32"}
ALL, F16_ONLY = ("f16x3", "bf16x6", "fp32"), ("f16x3",)
SENTINEL = -7777.25
PAD = 64                                   # elements of margin on both sides of every guarded buffer (whole 16-byte quads)
FACTOR = 4.0                               # attn_spatial_cases.FACTOR: the project's factor over the fp32 evaluation of the same operation
# Three fp32 roundings of quantities <= S (result, bias, residual): 3 x 2^-24 < 2^-22; f16x3 adds the 2^-21 of include/vd_amd.h (22
# significand bits on each side of a product)
FLOOR = {"f16x3": 2.0 ** -22 + 2.0 ** -21, "bf16x6": 2.0 ** -22, "fp32": 2.0 ** -22}
SILU_TOL = 2e-6                            # test_affine_act_pass: |silu_gpu(v) - silu(v)| <= 2e-6 (1 + |silu(v)|)
STATS_ATOL, STATS_RTOL = 1e-3, 1e-5        # what the tables' totals are held to in tests/test_gpu_ops.py, here per entry
# f16x3 only, by label, at most three (tests/test_gpu_conv_gemm.py's docstring has the derivation): the GroupNorm table of
# conv_wino_z128.hip under the mags family, whose entries are sums of 256 outputs of magnitude 1e3 .. 1e4 held to an ABSOLUTE 1e-3
F16X3_ALLOWANCE_LABELS = frozenset({"wino_split_k-N33H32-32x128-k3s1-res-gn-mags", "wino_split_k-N136H16-32x128-k3s1-fb-gn-mags",
                                    "wino_split_k-N129H16-32x128-k3s1-gn-mags"})
LANE_TERMS = 32                            # outputs a lane of the Winograd epilogue adds in fp32 before the partials go on in fp64 (wino_common.h)

# op:      "wino_split" vd_op_conv_wino_split | "wino_split_k" vd_op_conv_wino_split_k (scratch offered, nfr_sel) | "wino_ups"
#          vd_op_conv_wino_ups | "wino_act" vd_op_conv_wino_act | "lin_split" vd_op_linear_split(_stats) | "conv_split" vd_op_conv_split |
#          "side" vd_op_linear_split_side | "batched" vd_op_linear_batched | "frag" / "wino32" / "generic": vd_op_conv (vd_op_conv_stats)
#          with the fragment-major, the fp32 Winograd or only the [tap][Cout][Cin] weights
# N H:     frames and square source map (a linear layer of M rows: N = M, H = 1);  k: kernel size
# family:  "plain" | "impulse" | "mags" | "zero-frame" | "cancel" (make_inputs)
# subsets: frame subsets launched with nfr_sel = N must give the full launch's bits (output and table)
# variant: the instantiation the case is there for, {F} = the kernel's F16 parameter (true under f16x3); fp32v: the name under VD_MATH=fp32
#          where it differs
Case = namedtuple("Case", "op N H Cin Cout variant C0 k stride ups act aff fbias res stats family subsets zc modes fp32v",
                  defaults=(0, 3, 1, 0, 0, 0, 0, 0, 0, "plain", False, 0, ALL, None))


def label(c):
    s = f"{c.op}-N{c.N}H{c.H}-{c.Cin}"
    if c.C0 and c.C0 != c.Cin:
        s += f"c{c.C0}"
    s += f"x{c.Cout}-k{c.k}s{c.stride}"
    for flag, name in ((c.ups, "ups"), (c.act, "act"), (c.aff, "aff"), (c.fbias, "fb"), (c.res, "res"), (c.stats, "gn"), (c.subsets, "sel")):
        if flag:
            s += "-" + name
    if c.zc:
        s += f"-z{c.zc}"
    if c.family != "plain":
        s += "-" + c.family
    return s


def variant_name(c, mode):
    if mode == "fp32" and c.fp32v:
        return c.fp32v
    return c.variant.replace("{F}", "true" if mode == "f16x3" else "false")


FP32_OPS = ("frag", "wino32", "generic", "batched")       # VD_MATH=fp32: no caller hands a split image to the library (vd_igemm_variant_list holds no split row)


def cases_for(mode):
    return [c for c in CASES if mode in c.modes and (mode != "fp32" or c.op in FP32_OPS)]


# ------------------------------------------------------------------------------------------------------------------------- the table
def _r64(N, H, Cin, Cout, **kw):
    return Case("wino_split", N, H, Cin, Cout, f"conv3x3_wino_r64_kernel<{'true' if H == 8 else 'false'},{{F}}>", stats=1, **kw)


def _ups(N, H, Cin, Cout, **kw):
    return Case("wino_ups", N, H, Cin, Cout, f"conv3x3_wino_r64_ups_kernel<{'true' if H == 8 else 'false'},{{F}}>", ups=1, stats=1, **kw)


def _ksp(N, H, Cin, S, extras, **kw):
    return Case("wino_split_k", N, H, Cin, 64, f"conv3x3_wino_r64_kernel<{'true' if H == 8 else 'false'},{{F}}>+ksplit{S}",
                fbias=extras, res=extras, stats=extras, **kw)


def _z128(N, H, Cin, Cout, **kw):
    return Case("wino_split_k", N, H, Cin, Cout, "conv3x3_wino_z128_kernel<false>", stats=1, modes=F16_ONLY, **kw)


def _z128act(N, H, Cin, Cout, C0, **kw):
    return Case("wino_act", N, H, Cin, Cout, "conv3x3_wino_z128_kernel<true>", C0=C0, act=1, aff=1, stats=1, modes=F16_ONLY, **kw)


# four-frames form (H = 8): quarter-full, full and ragged last items; H = 16 | 32: N = 1..3, both item orders (N = 2 at 32 x 32: nbx = 8)
R64_CASES = [_r64(1, 8, 32, 64), _r64(4, 8, 96, 192, fbias=1, res=1), _r64(5, 8, 32, 192), _r64(10, 8, 96, 64, fbias=1, res=1),
             _r64(1, 16, 32, 64, fbias=1, res=1), _r64(3, 16, 96, 128), _r64(2, 32, 32, 64, res=1), _r64(3, 32, 96, 64, fbias=1)]
# sub-pixel form: source maps 8 and 16, Cout 64 and 128; N = 8 at 16 x 16: the grouped cout walk (nbx % 8 == 0)
UPS_CASES = [_ups(1, 8, 32, 64), _ups(5, 8, 96, 128), _ups(2, 16, 32, 128), _ups(8, 16, 32, 64), _ups(3, 16, 96, 64)]
# split-K: Cin = 128 / 192 / 256 / 384 / 512 -> 2 / 3 / 4 / 6 / 8 slices at H = 8 and 16, N = 1 and 5, with and without per-frame bias,
# residual and table; N = 40 at 16 x 16, 512 channels: 4 slices where a subset of five frames alone would get 8
KSPLIT_CASES = [_ksp(1, 8, 128, 2, 1), _ksp(5, 16, 128, 2, 0, subsets=True), _ksp(5, 8, 192, 3, 0), _ksp(1, 16, 192, 3, 1),
                _ksp(1, 8, 256, 4, 0), _ksp(5, 16, 256, 4, 1, subsets=True), _ksp(5, 8, 384, 6, 1, subsets=True), _ksp(1, 16, 384, 6, 0),
                _ksp(1, 8, 512, 8, 1), _ksp(5, 16, 512, 8, 0), _ksp(5, 8, 512, 8, 1), _ksp(1, 16, 128, 2, 1),
                _ksp(40, 16, 512, 4, 1, subsets=True)]
# conv_wino_z128.hip (f16x3): the smallest grids of >= 129 items; both item orders (136 % 8 == 0); ACT with and without concat
Z128_CASES = [_z128(33, 32, 32, 128, subsets=True, res=1), _z128(136, 16, 32, 128, subsets=True, fbias=1),
              _z128act(129, 16, 32, 128, 32, res=1), _z128act(136, 16, 64, 128, 32)]

# gemm_split.hip: (tile, smallest ragged M of its class, Cout, frames of 23 x 23 (stride 2: of 45 x 45) that reach the class as a 3x3)
GS_TILES = [("64,64", 70, 64, 2), ("64,128", 24513, 128, 47), ("128,128", 65443, 128, 124), ("128,64", 65573, 64, 124), ("128,192", 49029, 192, 93)]


def _gs(tile, act, conv):
    return f"gemm_split_kernel<{tile},{'true' if act else 'false'},{'true' if conv else 'false'},{{F}},false>"


GS_CASES = []
for tile, M, Cout, NF in GS_TILES:
    GS_CASES += [Case("lin_split", M, 1, 32, Cout, _gs(tile, 0, 0), k=1, res=1),                      # K = 32: one chunk
                 Case("lin_split", M, 1, 160, Cout, _gs(tile, 1, 0), k=1, act=1),                     # five chunks (the loop walks three at a time)
                 Case("conv_split", NF, 9 if NF == 2 else 23, 96 if NF == 2 else 32, Cout, _gs(tile, 0, 1), res=1),
                 Case("conv_split", NF + (NF == 2), 9 if NF == 2 else 45, 32, Cout, _gs(tile, 0, 1), stride=2)]
# ... and the table of the epilogue: whole frames of 64 rows, per entry
GS_CASES += [Case("lin_split", 3, 8, 32, 64, _gs("64,64", 0, 0), k=1, stats=1), Case("lin_split", 384, 8, 32, 128, _gs("64,128", 0, 0), k=1, stats=1, res=1),
             Case("lin_split", 1024, 8, 32, 128, _gs("128,128", 0, 0), k=1, stats=1), Case("lin_split", 768, 8, 32, 192, _gs("128,192", 0, 0), k=1, stats=1)]
SIDE_V = "gemm_split_kernel<128,128,false,false,{F},true>"
SIDE_CASES = [Case("side", 16, 64, 64, 128, SIDE_V, C0=32, k=1), Case("side", 16, 64, 32, 128, SIDE_V, C0=32, k=1)]
BATCHED_CASES = [Case("batched", 50, 1, 64, 64, _gs("64,64", 0, 0), k=1, zc=3, fp32v="gemm_frag_kernel<64,64,false>"),
                 Case("batched", 77, 1, 96, 96, _gs("64,64", 0, 0), k=1, zc=6, fp32v="gemm_frag_kernel<64,64,false>")]

# through vd_op_conv, as tests/test_gpu_ops.py runs them: gemm_frag.hip, conv_wino.hip, igemm.hip, one case per row
FRAG_CASES = []
for tile, M, Cout, _ in GS_TILES[:4]:
    FRAG_CASES += [Case("frag", M, 1, 64 if M == 70 else 32, Cout, f"gemm_frag_kernel<{tile},false>", C0=32, k=1, res=1),
                   Case("frag", M, 1, 32, Cout, f"gemm_frag_kernel<{tile},true>", k=1, act=1)]
WINO32_CASES = [Case("wino32", 5, 8, 32, 64, "conv3x3_wino_kernel<true>", fbias=1, res=1, stats=1),
                Case("wino32", 2, 16, 32, 64, "conv3x3_wino_kernel<false>", fbias=1, res=1, stats=1)]
GENERIC_CASES = [Case("generic", 2, 9, 64, 64, "igemm_kernel<64,64>", C0=32, stride=2, act=1, aff=1, fbias=1, res=1),
                 Case("generic", 1, 4, 32, 40, "igemm_kernel<64,64>", ups=1),
                 Case("generic", 24513, 1, 32, 128, "igemm_kernel<64,128>", k=1), Case("generic", 65443, 1, 32, 128, "igemm_kernel<128,128>", k=1, res=1),
                 Case("generic", 65573, 1, 32, 64, "igemm_kernel<128,64>", k=1)]
VARIANT_CASES = R64_CASES + UPS_CASES + KSPLIT_CASES + Z128_CASES + GS_CASES + SIDE_CASES + BATCHED_CASES + FRAG_CASES + WINO32_CASES + GENERIC_CASES

# the operand families on three base shapes per kernel file
BASES = [_r64(5, 8, 32, 64, fbias=1, res=1), _ksp(5, 16, 128, 2, 1), _ups(5, 8, 32, 64),
         _z128(33, 32, 32, 128, res=1), _z128(136, 16, 32, 128, fbias=1), _z128(129, 16, 32, 128),
         Case("lin_split", 70, 1, 96, 64, _gs("64,64", 0, 0), k=1, res=1), Case("conv_split", 2, 9, 32, 64, _gs("64,64", 0, 1), res=1),
         Case("conv_split", 3, 9, 32, 64, _gs("64,64", 0, 1), stride=2),
         Case("frag", 70, 1, 32, 64, "gemm_frag_kernel<64,64,false>", k=1, res=1), Case("frag", 45, 1, 96, 128, "gemm_frag_kernel<64,64,false>", k=1),
         Case("frag", 3, 4, 64, 64, "gemm_frag_kernel<64,64,false>", C0=32, k=1, res=1),
         Case("wino32", 5, 8, 32, 64, "conv3x3_wino_kernel<true>", fbias=1, res=1, stats=1), Case("wino32", 2, 16, 32, 64, "conv3x3_wino_kernel<false>", stats=1),
         Case("wino32", 2, 32, 32, 64, "conv3x3_wino_kernel<false>", res=1, stats=1),
         Case("generic", 2, 6, 32, 40, "igemm_kernel<64,64>", fbias=1, res=1), Case("generic", 2, 9, 32, 64, "igemm_kernel<64,64>", stride=2),
         Case("generic", 70, 1, 32, 64, "igemm_kernel<64,64>", k=1, res=1)]
FAMILIES = ("impulse", "mags", "zero-frame", "cancel")
FAMILY_CASES = [b._replace(family=f) for b in BASES for f in FAMILIES]
CASES = VARIANT_CASES + FAMILY_CASES


# ------------------------------------------------------------------------------------------------------------------------- inputs
def out_hw(c):
    pad = (c.k - 1) // 2
    return ((c.H << c.ups) + 2 * pad - c.k) // c.stride + 1


def make_inputs(c):
    """CPU float32: x [N][H][H][Cin] (x0 | x1 at C0), w OIHW, bias, and where the case has them A / B [N][Cin], fbias [N][Cout], res."""
    g = torch.Generator().manual_seed(zlib.crc32(label(c).encode()))
    N, H, Cin, Cout, k = c.N, c.H, c.Cin, c.Cout, c.k
    Z = max(c.zc, 1)
    x = torch.randn(Z * N, H, H, Cin, generator=g)
    w = torch.randn(Z * Cout, Cin, k, k, generator=g) * (3.0 / (k * k * Cin)) ** 0.5
    d = {"bias": torch.randn(Z * Cout, generator=g) * 0.3}
    Ho = out_hw(c)
    if c.aff or c.op == "side":
        d["A"], d["B"] = torch.rand(N, Cin, generator=g) + 0.75, torch.randn(N, Cin, generator=g) * 0.5
    if c.fbias:
        d["fbias"] = torch.randn(N, Cout, generator=g) * 0.5
    if c.res:
        d["res"] = torch.randn(N, Ho, Ho, Cout, generator=g)
    if c.family == "impulse":
        # one non-zero element per frame: a corner, an edge, the interior, the last corner; another channel per frame
        x.zero_()
        for f in range(N):
            y, xx = [(0, 0), (0, H // 2), (H // 2, H // 2), (H - 1, H - 1)][f % 4]
            x[f, y, xx, (5 * f + 1) % Cin] = 1.5 if f % 2 == 0 else -0.75
    elif c.family == "mags":
        x *= 10.0 ** (-3.0 + 5.0 * torch.arange(Cin) / Cin)
        w *= (10.0 ** torch.linspace(-3.0, 1.4771212547, Cout))[:, None, None, None]           # 1e-3 .. 30 across the output channels
    elif c.family == "zero-frame":
        x[N // 2] = 0.0
    elif c.family == "cancel":
        h = Cin // 2
        w[:, h:] = -w[:, :h]
        x[..., h:] = x[..., :h]
    d["x"], d["w"] = x.contiguous(), w.contiguous()
    return d


# ------------------------------------------------------------------------------------------------------------------------- the library
def L():
    return _lib.lib()


def process_mode():
    return MODES[L().vd_math_mode()]


def variant_list():
    buf = ctypes.create_string_buffer(8192)
    n = L().vd_igemm_variant_list(buf, len(buf))
    names = buf.value.decode().split()
    assert n == len(names) > 0, (n, names)
    return names


WEIGHTS = {"generic": 0, "frag": 1, "wino32": 2, "lin_split": 3, "conv_split": 3, "side": 3, "batched": 3, "wino_split": 4, "wino_split_k": 4,
           "wino_act": 4, "wino_ups": 5}


def variant_of(c, nfr=None, nfr_sel=0):
    """(1 = a kernel | 0 = refused, name) from the library's own tables: no launch."""
    buf = ctypes.create_string_buffer(200)
    wk = WEIGHTS[c.op]
    if c.op == "batched" and process_mode() == "fp32":
        wk = 1
    rc = L().vd_igemm_variant(c.k, c.stride, c.ups, c.Cin, c.C0 or c.Cin, c.Cout, nfr or c.N, nfr_sel, c.H, wk, c.act, c.aff, c.fbias, c.res,
                              int(c.op == "side"), c.zc, int(c.op == "wino_split_k"), buf, len(buf))
    assert rc in (0, 1), rc
    return rc, buf.value.decode()


def _i16(n):
    return torch.empty(n, dtype=torch.int16)


def pack(c, w):
    """The weight image of the case's entry point, through the library's host packers (their closed forms: tests/test_gpu_ops.py)."""
    O, I = w.shape[:2]
    w = w.contiguous().float()
    lib = L()
    if c.op in ("wino_split", "wino_split_k", "wino_act"):
        out = _i16(lib.vd_split_image_u16(O, 16 * I))
        _lib.check(lib.vd_pack_conv3_wino_split(_lib.ptr(w), _lib.ptr(out), O, I))
    elif c.op == "wino_ups":
        out = _i16(lib.vd_split_image_u16(4 * O, 16 * I))
        _lib.check(lib.vd_pack_conv3_wino_ups(_lib.ptr(w), _lib.ptr(out), O, I))
    elif c.op == "conv_split":
        out = _i16(lib.vd_split_image_u16(O, 9 * I))
        _lib.check(lib.vd_pack_conv3_split(_lib.ptr(w), _lib.ptr(out), O, I))
    elif c.op == "frag" or (c.op == "batched" and process_mode() == "fp32"):
        out = torch.empty(O * I)
        _lib.check(lib.vd_pack_linear_frag(_lib.ptr(w.reshape(O, I)), _lib.ptr(out), O, I))
    elif c.op in ("lin_split", "side", "batched"):
        out = _i16(lib.vd_split_image_u16(O, I))
        _lib.check(lib.vd_pack_linear_split(_lib.ptr(w.reshape(O, I)), _lib.ptr(out), O, I))
    elif c.op == "wino32":
        out = torch.empty(16 * O * I)
        _lib.check(lib.vd_pack_conv3_wino(_lib.ptr(w), _lib.ptr(out), O, I))
    else:
        out = w.permute(2, 3, 0, 1).reshape(-1).contiguous()                                  # [tap][O][I]
    return out


def guarded_in(t):
    """t on the device, read from the middle of a buffer whose margins hold NaN."""
    flat = t.reshape(-1)
    buf = torch.full((flat.numel() + 2 * PAD,), float("nan"), dtype=t.dtype, device="cuda")
    buf[PAD:PAD + flat.numel()] = flat.to("cuda")
    return buf[PAD:PAD + flat.numel()].view(t.shape)


class Guarded:
    """An output written into the middle of a NaN-filled buffer whose margins hold a sentinel."""

    def __init__(self, shape, dtype=torch.float32):
        n = 1
        for s in shape:
            n *= s
        self.n, self.buf = n, torch.full((n + 2 * PAD,), float("nan"), dtype=dtype, device="cuda")
        self.buf[:PAD] = SENTINEL
        self.buf[PAD + n:] = SENTINEL
        self.t = self.buf[PAD:PAD + n].view(shape)

    def untouched(self):
        return bool((self.buf[:PAD] == SENTINEL).all()) and bool((self.buf[PAD + self.n:] == SENTINEL).all())


def same_bits(a, b):
    it = torch.int64 if a.dtype == torch.float64 else torch.int32
    return a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def stats_shape(c, N):
    """(split, geometry, rows per block) of the case's GroupNorm table."""
    lib, Ho = L(), out_hw(c)
    if c.op == "wino_ups":
        return lib.vd_conv_ups_stats_split(c.H), "ups", 0
    if c.op == "lin_split":
        split = lib.vd_linear_stats_split(N * c.H * c.H, c.Cout, c.H * c.H)
        return split, "rows", c.H * c.H // split
    return lib.vd_conv_stats_split(Ho), "wino", 0


class Launcher:
    """The device side of a case: operands uploaded once (inputs between NaN margins), launch(frames) runs the entry point on a frame
    subset into fresh guarded outputs."""

    def __init__(self, c, d):
        self.c, self.d = c, d
        C0 = c.C0 or c.Cin
        self.C0 = C0
        self.x0 = guarded_in(d["x"][..., :C0].contiguous())
        self.x1 = guarded_in(d["x"][..., C0:].contiguous()) if C0 < c.Cin else None
        self.bias = d["bias"].to("cuda")
        self.dev = {k: d[k].to("cuda") for k in ("A", "B", "fbias", "res") if k in d}
        if c.op == "batched":
            self._batched_image()
        else:
            self.w = pack(c, d["w"]).to("cuda")

    def _batched_image(self):
        """Every problem's image and bias in one float buffer, in another order than the problems and with gaps of different sizes."""
        c, Z = self.c, self.c.zc
        self.imgs = [pack(c, self.d["w"][z * c.Cout:(z + 1) * c.Cout]) for z in range(Z)]
        self.imgs = [(i if i.dtype == torch.float32 else i.view(torch.float32)).contiguous() for i in self.imgs]
        parts, tab, cur = [], [0] * (2 * Z), 0

        def put(t, slot, gap):
            nonlocal cur
            parts.append(torch.full((gap,), float("nan")))
            cur += gap
            tab[slot] = cur
            parts.append(t)
            cur += t.numel()
            tail = -cur % 4
            parts.append(torch.full((tail,), float("nan")))
            cur += tail

        for i, z in enumerate(sorted(range(Z), key=lambda z: (z * 5 + 2) % Z)):
            put(self.imgs[z], 2 * z, 4 * (i + 1))
            put(self.d["bias"][z * c.Cout:(z + 1) * c.Cout], 2 * z + 1, 4 * ((3 * i) % 5))
        self.zbase = torch.cat(parts).to("cuda")
        self.ztab = torch.tensor(tab, dtype=torch.int64, device="cuda")
        assert len(set(tab[2 * z + 2] - tab[2 * z] for z in range(Z - 1))) > 1 or Z < 3, tab     # no constant stride

    def launch(self, frames=None, nfr_sel=0):
        """-> dict(out, stats, side: Guarded or None).  frames: a list of frame indices (gathered), None = all."""
        c, lib, p, st = self.c, L(), _lib.ptr, _lib.current_stream()
        x0, x1, dev = self.x0, self.x1, dict(self.dev)
        if frames is not None:
            idx = torch.tensor(frames, device="cuda")
            x0 = guarded_in(x0[idx])
            x1 = guarded_in(x1[idx]) if x1 is not None else None
            dev = {k: v[idx].contiguous() for k, v in dev.items()}
        N, Ho, Cout = x0.shape[0] // max(c.zc, 1), out_hw(c), c.Cout
        out = Guarded((max(c.zc, 1) * N, Ho, Ho, Cout))
        stats = side = None
        if c.stats:
            split = stats_shape(c, N)[0]
            stats = Guarded((N, split, Cout, 2), torch.float64)
        sp = p(stats.t) if stats else None
        fb, res, A, B = (p(dev[k]) if k in dev else None for k in ("fbias", "res", "A", "B"))
        fld = Cout if c.fbias else 0
        if c.op == "wino_split":
            rc = lib.vd_op_conv_wino_split(p(x0), c.Cin, N, c.H, c.H, 0, p(self.w), p(self.bias), res, fb, fld, p(out.t), Cout, sp, st)
        elif c.op == "wino_split_k":
            rc = lib.vd_op_conv_wino_split_k(p(x0), c.Cin, N, c.H, c.H, 0, p(self.w), p(self.bias), res, fb, fld, p(out.t), Cout, sp, nfr_sel, st)
        elif c.op == "wino_ups":
            rc = lib.vd_op_conv_wino_ups(p(x0), c.Cin, N, c.H, p(self.w), p(self.bias), p(out.t), Cout, sp, st)
        elif c.op == "wino_act":
            rc = lib.vd_op_conv_wino_act(p(x0), p(x1), self.C0, c.Cin, N, c.H, c.H, p(self.w), p(self.bias), A, B, res, p(out.t), Cout, sp, st)
        elif c.op == "lin_split":
            M = N * c.H * c.H
            if c.stats:
                rc = lib.vd_op_linear_split_stats(p(x0), M, c.Cin, p(self.w), p(self.bias), res, c.act, p(out.t), Cout, c.H * c.H, sp, st)
            else:
                rc = lib.vd_op_linear_split(p(x0), M, c.Cin, p(self.w), p(self.bias), res, c.act, p(out.t), Cout, st)
        elif c.op == "conv_split":
            rc = lib.vd_op_conv_split(p(x0), c.Cin, N, c.H, c.H, c.stride, p(self.w), p(self.bias), res, p(out.t), Cout, st)
        elif c.op == "side":
            side = Guarded((N, c.H, c.H, c.Cin))
            rc = lib.vd_op_linear_split_side(p(x0), p(x1), self.C0, c.Cin, N * c.H * c.H, c.H * c.H, p(self.w), p(self.bias), A, B, p(out.t), p(side.t),
                                             Cout, st)
        elif c.op == "batched":
            rc = lib.vd_op_linear_batched(p(x0), c.zc, N, c.Cin, Cout, p(self.zbase), p(self.ztab), p(out.t), st)
        elif c.op == "wino32" and c.stats:
            rc = lib.vd_op_conv_stats(p(x0), c.Cin, N, c.H, c.H, c.ups, p(self.w), p(self.bias), res, fb, fld, p(out.t), Cout, sp, st)
        else:
            kind = WEIGHTS[c.op]
            rc = lib.vd_op_conv(p(x0), p(x1), self.C0, c.Cin, N, c.H, c.H, c.ups, c.stride, (c.k - 1) // 2, c.k, p(self.w) if kind == 0 else None,
                                p(self.w) if kind == 1 else None, p(self.w) if kind == 2 else None, p(self.bias), A, B, c.act, res, fb, fld,
                                p(out.t), Cout, st)
        _lib.check(rc)
        torch.cuda.synchronize()
        return {"out": out, "stats": stats, "side": side}

    def single_problem(self, z):
        """Problem z of a batched case alone, through the single-problem entry point of the same arithmetic."""
        c, lib, p, st = self.c, L(), _lib.ptr, _lib.current_stream()
        N = c.N
        a = guarded_in(self.x0[z * N:(z + 1) * N])
        out = Guarded((N, 1, 1, c.Cout))
        img, b = self.imgs[z].to("cuda"), self.d["bias"][z * c.Cout:(z + 1) * c.Cout].to("cuda")
        if process_mode() == "fp32":
            rc = lib.vd_op_conv(p(a), None, c.Cin, c.Cin, N, 1, 1, 0, 1, 0, 1, None, p(img), None, p(b), None, None, 0, None, None, 0, p(out.t), c.Cout, st)
        else:
            rc = lib.vd_op_linear_split(p(a), N, c.Cin, p(img), p(b), None, 0, p(out.t), c.Cout, st)
        _lib.check(rc)
        torch.cuda.synchronize()
        return out


# ------------------------------------------------------------------------------------------------------------------------- references
WINO_OPS = ("wino_split", "wino_split_k", "wino_ups", "wino_act", "wino32")


F32_PIXELS = 8192      # the float32 evaluation runs on whole frames, evenly spaced, of at most this many output pixels in all


def f32_frames(c):
    """The frames e_f32 is taken over: all, or for the big shapes the first, the last and evenly spaced ones between (the maximum over
    fewer elements is no larger: the bound only tightens)."""
    per = out_hw(c) ** 2
    n = max(2, F32_PIXELS // per)
    if c.N <= n:
        return list(range(c.N))
    return sorted({round(i * (c.N - 1) / (n - 1)) for i in range(n)})


def references(c, d):
    """(ref64, S, act_allow, e_f32): the float64 result, the unit of every element, the SiLU term of ACT instantiations (0 otherwise)
    -- all [N][Ho][Ho][Cout] (batched: the problems stacked along N) -- and max |f32 - ref64| / S of the float32 CPU evaluation of the
    same algorithm: wino_ref in float32 for the Winograd kernels, for the rest conv_ref in float32 in its one defined order
    (sequential=True) over f32_frames(), the sum starting at bias + res where the kernel's accumulators do (gemm_frag.hip, gemm_split.hip)
    and receiving them last where the kernel adds them last (igemm.hip)."""
    Z, N, Cout = max(c.zc, 1), c.N, c.Cout
    ref, S, allow, e_f32 = [], [], [], 0.0
    sel = f32_frames(c)
    for z in range(Z):
        x, w, b = d["x"][z * N:(z + 1) * N], d["w"][z * Cout:(z + 1) * Cout], d["bias"][z * Cout:(z + 1) * Cout]
        C0 = c.C0 or c.Cin
        act = c.act and c.op != "side"
        aff = (d.get("A"), d.get("B")) if c.aff else (None, None)
        a64 = operand(x[..., :C0], x[..., C0:] if C0 < c.Cin else None, *aff, act=act)
        a32 = operand(x[..., :C0], x[..., C0:] if C0 < c.Cin else None, *aff, act=act, dtype=torch.float32)
        kw = dict(fbias=d.get("fbias"), res=d.get("res"))
        ref.append(conv_ref(a64, w, b, stride=c.stride, ups=c.ups, **kw))
        if c.op in WINO_OPS:
            wk = dict(kw, subpixel=c.op == "wino_ups", ups=c.ups and c.op != "wino_ups")
            S.append(wino_ref(a64, w, b, absolute=True, **wk))
            f32, fsel = wino_ref(a32, w, b, dtype=torch.float32, **wk).double(), slice(None)
        else:
            S.append(conv_ref(a64, w, b, stride=c.stride, ups=c.ups, absolute=True, **kw))
            ks = {k: (v[sel] if v is not None else None) for k, v in kw.items()}
            f32, fsel = conv_ref(a32[sel], w, b, stride=c.stride, ups=c.ups, dtype=torch.float32, sequential=True, first=c.op != "generic", **ks).double(), sel
        e_f32 = max(e_f32, float(((f32 - ref[-1][fsel]).abs() / S[-1][fsel]).max()))
        # ACT: sum_k |w_k| delta_k / S, delta_k = SILU_TOL (1 + |silu(a_k)|); a padding tap is zero after the activation: no term
        allow.append(SILU_TOL * conv_ref(1.0 + a64.abs(), w.abs(), stride=c.stride, ups=c.ups) / S[-1] if act else torch.zeros_like(S[-1]))
    return torch.cat(ref), torch.cat(S), torch.cat(allow), e_f32


def subsets_of(N):
    """Frames in another order, and a single frame."""
    return [[N - 1, 0, N // 2, 1, N - 2][:min(5, N)], [N // 2 + 1 if N > 2 else 0]]


def run_case(c):
    """Launch a case in the process' own mode and measure it: a dict of plain numbers, strings and booleans (one JSON line of the tool)."""
    mode = process_mode()
    rc, name = variant_of(c)
    r = {"label": label(c), "family": c.family, "op": c.op, "variant": name, "variant_rc": rc, "expected_variant": variant_name(c, mode), "mode": mode}
    lib = L()
    if c.op == "wino_split_k" and "+ksplit" in c.variant:
        r["ksplit"] = lib.vd_conv_wino_ksplit(c.N, c.H, c.Cin, c.Cout)
        r["ksplit_stated"] = int(c.variant.rsplit("+ksplit", 1)[1])
    if "z128" in c.variant:
        r["block_couts"] = lib.vd_conv_wino_block_couts(c.N, c.H, c.Cin, c.Cout)
    d = make_inputs(c)
    dev = Launcher(c, d)
    one = dev.launch()
    out = one["out"]
    got = out.t.cpu().double()
    ref, S, allow, e_f32 = references(c, d)
    fin = bool(torch.isfinite(got).all())
    r["finite"] = fin
    r["e_got"] = float(((got - ref).abs() / S - allow).clamp_min(0).max()) if fin else float("nan")
    r["e_f32"] = e_f32
    r["act_allow"] = float(allow.max())
    r["margins_untouched"] = out.untouched() and all(one[k] is None or one[k].untouched() for k in ("stats", "side"))
    two = dev.launch()
    r["rerun_same_bits"] = all(one[k] is None or (two[k].untouched() and same_bits(two[k].t, one[k].t)) for k in ("out", "stats", "side"))
    if c.stats:
        split, geo, rows = stats_shape(c, c.N)
        want = gn_block_sums(out.t.cpu(), geo, rows)
        tab = one["stats"].t.cpu()
        r["stats_entries"] = tab.numel()
        r["stats_finite"] = bool(torch.isfinite(tab).all())
        r["stats_excess"] = float(((tab - want).abs() - (STATS_ATOL + STATS_RTOL * want.abs())).max()) if tab.shape == want.shape else float("inf")
        # the allowance of F16X3_ALLOWANCE_LABELS: a lane's fp32 sum of LANE_TERMS values is off by at most LANE_TERMS 2^-24 sum |y| (y^2)
        lane = LANE_TERMS * 2.0 ** -24 * gn_block_sums(out.t.cpu().abs(), geo, rows)
        r["stats_excess_lane"] = float(((tab - want).abs() - (STATS_ATOL + STATS_RTOL * want.abs() + lane)).max()) if tab.shape == want.shape else float("inf")
        r["stats_split"] = split
    if c.family == "zero-frame":
        # no product term: the frame is bias + fbias + res in fp32, whichever way the kernel associates the three
        f = c.N // 2
        b, fb = d["bias"][None, None, :], (d["fbias"][f][None, None, :] if c.fbias else torch.zeros(1, 1, c.Cout))
        rs = d["res"][f] if c.res else torch.zeros(1, 1, c.Cout)
        cands = [(b + fb) + rs, b + (fb + rs), (b + rs) + fb]
        g32 = out.t[f].cpu()
        r["zero_frame_exact"] = bool(torch.stack([g32 == k for k in cands]).any(0).all())
    if c.subsets:
        ok = True
        for sel in subsets_of(c.N):
            vrc, vname = variant_of(c, nfr=len(sel), nfr_sel=c.N)
            sub = dev.launch(sel, nfr_sel=c.N)
            ok = ok and vrc == 1 and vname == name and sub["out"].untouched() and same_bits(sub["out"].t, out.t[sel])
            if c.stats:
                ok = ok and sub["stats"].untouched() and same_bits(sub["stats"].t, one["stats"].t[sel])
        r["subsets_same_bits"] = ok
        r["subset_alone_variant"] = variant_of(c, nfr=len(subsets_of(c.N)[0]))[1]           # what the subset would get without nfr_sel
    if c.op == "batched":
        r["singles_same_bits"] = all(same_bits(dev.single_problem(z).t, out.t[z * c.N:(z + 1) * c.N]) for z in range(c.zc))
    if c.op == "side":
        want = silu(operand(d["x"], None, d["A"], d["B"]))
        sd = one["side"].t.cpu()
        r["side_finite"] = bool(torch.isfinite(sd).all())
        r["side_excess"] = float(((sd.double() - want).abs() - (SILU_TOL + SILU_TOL * want.abs())).max())
        y = torch.empty_like(one["side"].t)
        _lib.check(lib.vd_op_affine_act(_lib.ptr(dev.x0), _lib.ptr(dev.x1), dev.C0, c.Cin, _lib.ptr(dev.dev["A"]), _lib.ptr(dev.dev["B"]), c.N, c.H * c.H, 1,
                                        _lib.ptr(y), _lib.current_stream()))
        torch.cuda.synchronize()
        r["side_equals_affine_act"] = same_bits(y, one["side"].t)                               # reported (docs/LAB_NOTES.md), not required
    return r


def bound(r):
    return max(FACTOR * r["e_f32"], FLOOR[r["mode"]])


def failures(r):
    """What a measured case (run_case's dict, or a line of the tool) fails: a list of strings, empty if it passes."""
    bad = []
    b = bound(r)
    if r["variant_rc"] != 1 or r["variant"] != r["expected_variant"]:
        bad.append(f"runs {r['variant']}, the case names {r['expected_variant']}")
    if "ksplit" in r and r["ksplit"] != r["ksplit_stated"]:
        bad.append(f"vd_conv_wino_ksplit gives {r['ksplit']} slices, the case states {r['ksplit_stated']}")
    if r.get("block_couts", 128) != 128:
        bad.append("vd_conv_wino_block_couts does not answer 128 on this device")
    if not r["margins_untouched"]:
        bad.append("the margins around an output were written")
    if not r["rerun_same_bits"]:
        bad.append("a second launch gave other bits")
    if not r["finite"]:
        bad.append("non-finite outputs")
    elif not r["e_got"] <= b:
        bad.append(f"e_got {r['e_got']:.3e} > max({FACTOR:g} x e_f32 {r['e_f32']:.3e}, {FLOOR[r['mode']]:.3e}) = {b:.3e}")
    allowed = r["mode"] == "f16x3" and r["label"] in F16X3_ALLOWANCE_LABELS
    if "stats_excess" in r and not (r["stats_finite"] and r["stats_excess_lane" if allowed else "stats_excess"] <= 0.0):
        bad.append(f"a GroupNorm table entry is off its block's sums by {r['stats_excess']:.3e} beyond atol {STATS_ATOL:g} + rtol {STATS_RTOL:g}")
    if not r.get("zero_frame_exact", True):
        bad.append("the zero frame is not exactly bias + fbias + res")
    if not r.get("subsets_same_bits", True):
        bad.append("a frame subset launched with nfr_sel gave other bits (or another kernel) than the full launch")
    if not r.get("singles_same_bits", True):
        bad.append("a problem of the batch alone gave other bits")
    if "side_excess" in r and not (r["side_finite"] and r["side_excess"] <= 0.0):
        bad.append(f"the side image is off SiLU(a A + B) by {r['side_excess']:.3e} beyond {SILU_TOL:g} (1 + |ref|)")
    return bad


def case_line(r):
    return f"CONV_GEMM_CASE | {r['label']} | {r['variant']} | {r['mode']} | {r['e_got']:.2e} | {r['e_f32']:.2e}"
