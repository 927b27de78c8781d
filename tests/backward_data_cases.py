"""The case table of the backward-data matrix products (vd_op_conv3_bwd_data, vd_op_linear_bwd_data: the engine's bwd_conv3 /
bwd_linear with its own argument setup), the enumeration of the calls backward() makes, and run_case(): imported by
tests/test_backward_data_cpu.py (the enumeration and the variants, host only), tests/test_gpu_backward_data.py (the test process' own
VD_MATH) and tools/backward_data_check.py (a child process for the other split mode).  Not a test file.

A case is one backward call: cls names the layer class (conv1 | conv2 | down | up: 3x3; skip | qkv | proj | stem: matrix products), O and
I are the FORWARD's outputs and inputs, so the call reads Cin' = O channels of dy and writes Cout' = I.  The bound is the one of
tests/conv_gemm_cases.py: e = max |got - ref64| / S <= max(4 e_f32, FLOOR[mode]), ref64 the float64 autograd gradient of the plain forward
(tests/backward_data_restated.py), S and e_f32 from conv_ref / wino_ref of the backward operator over a torch-made rotated / transposed
weight; nothing is taken from the kernel under test.
"""
import ctypes
import zlib
from collections import namedtuple

import torch

import backward_data_restated as R
from conv_gemm_cases import FACTOR, FLOOR, MODES, Guarded, guarded_in, same_bits
from conv_gemm_restated import conv_ref, wino_ref
from video_diffusion_amd import _lib

KIND = {"linear": 0, "stem": 1, "wino": 2, "generic": 3}             # include/vd_amd.h: vd_pack_weight_bwd
LINEAR = ("skip", "qkv", "proj", "stem")
REFUSAL = "use_gradient_method runs on the split arithmetic only"
F32_ROWS = 8192            # the float32 loop runs on whole frames, evenly spaced, of at most this many output pixels (conv_gemm_cases.f32_frames)
SCALES = (0, -20, -40)     # the magnitude family: dy * 2^k

# variant: the instantiation the case is there for, {F} = the kernel's F16 parameter; bf16v: the name under bf16x6 where it differs
# res: the call has a residual -- run out of place, and in place with `out` preloaded: the same bits
Case = namedtuple("Case", "cls N H O I variant res mags bf16v", defaults=(0, False, None))


def L():
    return _lib.lib()


def process_mode():
    return MODES[L().vd_math_mode()]


def label(c):
    return f"{c.cls}-N{c.N}H{c.H}-{c.O}to{c.I}" + ("-res" if c.res else "") + ("-mags" if c.mags else "")


def kind_of(cls, H, O, I, mode):
    """The backward image the engine gives the call (engine.hip: k3b and add_conv): Winograd-split where the map is a power of two >= 8,
    Cout' % 64 == 0 and Cin' % 32 == 0."""
    if cls in LINEAR:
        return "stem" if cls == "stem" else "linear"
    return "wino" if H >= 8 and H & (H - 1) == 0 and I % 64 == 0 and O % 32 == 0 and mode != "fp32" else "generic"


def variant_of(cls, N, H, O, I, res=0, mode=None):
    """(1 = a kernel | 0 = refused, name) of the call from the library's own tables: no launch."""
    buf = ctypes.create_string_buffer(200)
    kind = kind_of(cls, H, O, I, mode or process_mode())
    if cls in LINEAR:
        rc = L().vd_igemm_variant(1, 1, 0, O, O, R.STEM_KPAD if cls == "stem" else I, N * H * H, 0, 1, 3, 0, 0, 0, res, 0, 0, 0, buf, len(buf))
    else:
        rc = L().vd_igemm_variant(3, 1, 0, O, O, I, N, 0, H, 4 if kind == "wino" else 0, 0, 0, 0, res, 0, 0, int(kind == "wino"), buf, len(buf))
    assert rc in (0, 1), rc
    return rc, buf.value.decode()


def variant_name(c, mode):
    if mode == "bf16x6" and c.bf16v:
        return c.bf16v
    return c.variant.replace("{F}", "true" if mode == "f16x3" else "false")


# ------------------------------------------------------------------------------------------------------------------------- the calls
# the two configurations tests/test_gpu_backward.py runs guided steps on, with the frame counts of its windows
CONFIGS = [("tiny", dict(image_size=32, num_channels=64, num_res_blocks=1), (12, 24, 64)),
           ("tiny-32", dict(image_size=32, num_channels=32, num_res_blocks=1), (16, 32, 64)),
           ("default-64", dict(image_size=64), (20,))]


def backward_calls(specs, image_size):
    """[(cls, H, O, I)] of every matrix product backward() runs, read off the parameter list: a Downsample conv runs at its INPUT
    resolution (on the zero-stuffed gradient), an Upsample conv at 2H."""
    out, H = [], image_size
    for k, s in specs:
        if k == "input_blocks.0.0.weight":
            out.append(("stem", H, s[0], s[1]))
        elif k.endswith(".op.weight"):
            out.append(("down", H, s[0], s[1]))
            H //= 2
        elif k.endswith(".conv.weight"):
            H *= 2
            out.append(("up", H, s[0], s[1]))
        else:
            for tail, cls in ((".in_layers.2.weight", "conv1"), (".out_layers.3.weight", "conv2"), (".skip_connection.weight", "skip"),
                              ("attention.qkv.weight", "qkv"), ("attention.proj_out.weight", "proj")):
                if k.endswith(tail):
                    out.append((cls, H, s[0], s[1]))
    return out


def needed_variants(mode=None):
    """variant name -> [(config, N, cls, H, O, I)] over CONFIGS."""
    import video_diffusion_amd as vda
    need = {}
    for name, over, frames in CONFIGS:
        cfg = {**vda.video_model_and_diffusion_defaults(), **dict(T=8, rp_alpha=8, rp_beta=8, rp_gamma=8), **over}
        model, _ = vda.create_video_model_and_diffusion(**cfg)
        for call in sorted(set(backward_calls(model.param_specs(), cfg["image_size"]))):
            for N in frames:
                rc, v = variant_of(call[0], N, *call[1:], res=int(call[0] in ("down", "qkv")), mode=mode)
                assert rc == 1, (name, N, call, v)
                need.setdefault(v, []).append((name, N) + call)
    return need


# ------------------------------------------------------------------------------------------------------------------------- the table
def _w(tf4, s=0):
    return f"conv3x3_wino_r64_kernel<{'true' if tf4 else 'false'},{{F}}>" + (f"+ksplit{s}" if s else "")


def _gs(tile):
    return f"gemm_split_kernel<{tile},false,false,{{F}},false>"


SMALL = [
    # Winograd-split image, 8 x 8 (four-frames form) and 16 x 16; one slice (scratch offered, none taken) and 2 / 3 / 4 / 8 slices
    Case("conv1", 3, 8, 64, 192, _w(1), mags=True),                   # a concat width: Cout' a multiple of 64 but not of 128
    Case("conv2", 2, 8, 128, 128, _w(1, 2), mags=True),               # O == I: a missing transposition must not cancel (asymmetric weights)
    Case("conv1", 1, 8, 256, 320, _w(1, 4)),
    Case("conv1", 1, 8, 512, 128, _w(1, 8)),
    Case("down", 3, 8, 64, 64, _w(1), res=1),                         # zero-stuffed gradient of a 4 x 4 map, accumulated in place
    Case("conv1", 3, 16, 96, 64, _w(0)),
    Case("up", 1, 16, 128, 128, _w(0, 2), res=1),
    Case("conv1", 1, 16, 192, 64, _w(0, 3)),
    Case("conv2", 2, 32, 64, 64, _w(0)),
    # the generic fp32 kernel: maps below 8 x 8, and a Cout' that is no multiple of 64
    Case("conv1", 3, 4, 128, 256, "igemm_kernel<64,64>"),
    Case("conv2", 2, 2, 64, 64, "igemm_kernel<64,64>"),
    Case("down", 3, 4, 64, 32, "igemm_kernel<64,64>", res=1),
    Case("conv1", 2, 8, 64, 96, "igemm_kernel<64,64>", res=1),
    # matrix products
    Case("skip", 3, 4, 128, 192, _gs("64,64"), mags=True),
    Case("qkv", 2, 4, 384, 128, _gs("64,64"), res=1),
    Case("proj", 3, 8, 128, 128, _gs("64,64")),                       # O == I
    Case("stem", 3, 8, 64, 5, _gs("64,64")),
    Case("stem", 1, 16, 32, 6, _gs("64,64")),
    Case("skip", 3, 16, 32, 96, _gs("64,64"), res=1),
]
# the variants only grids of the full-size windows reach: the smallest shape of each class (tests/conv_gemm_cases.py: GS_TILES, Z128_CASES)
BIG = [
    Case("conv1", 33, 32, 32, 128, "conv3x3_wino_z128_kernel<false>", bf16v="conv3x3_wino_r64_kernel<false,false>"),
    Case("skip", 24513, 1, 32, 128, _gs("64,128")),
    Case("skip", 65443, 1, 32, 128, _gs("128,128"), res=1),
    Case("stem", 65573, 1, 32, 5, _gs("128,64")),
    Case("skip", 49029, 1, 32, 192, _gs("128,192")),
    Case("conv1", 24, 32, 32, 96, "igemm_kernel<64,128>"),
    Case("conv1", 64, 32, 32, 96, "igemm_kernel<128,128>"),
    Case("down", 64, 32, 32, 32, "igemm_kernel<128,64>", res=1),
]
CASES = SMALL + BIG


# ------------------------------------------------------------------------------------------------------------------------- one case
def make_inputs(c):
    """CPU float32: w as the checkpoint stores it, dy [N][H][H][O] (down: the zero-stuffed gradient, with d_out its source), res."""
    g = torch.Generator().manual_seed(zlib.crc32(label(c).encode()))
    k = 1 if c.cls in LINEAR and c.cls != "stem" else 3
    w = torch.randn(c.O, c.I, k, k, generator=g) * (3.0 / (k * k * c.O)) ** 0.5
    d = {"w": w.contiguous()}
    if c.cls == "down":
        d["d_out"] = torch.randn(c.N, c.H // 2, c.H // 2, c.O, generator=g)
        d["dy"] = R.zero_stuff2(d["d_out"])
    else:
        d["dy"] = torch.randn(c.N, c.H, c.H, c.O, generator=g)
    Nb = R.STEM_KPAD if c.cls == "stem" else c.I
    d["res"] = torch.randn(c.N, c.H, c.H, Nb, generator=g) if c.res else None
    return d


def pack(kind, w):
    """The backward image through the library's own packer (tests/test_backward_data_cpu.py holds it to the forward packers)."""
    O, I = w.shape[:2]
    out = torch.zeros(L().vd_bwd_image_floats(KIND[kind], O, I))
    w = w.contiguous().float()
    _lib.check(L().vd_pack_weight_bwd(_lib.ptr(w), KIND[kind], O, I, _lib.ptr(out)))
    return out


def f32_frames(N, per):
    n = max(2, F32_ROWS // per)
    return list(range(N)) if N <= n else sorted({round(i * (N - 1) / (n - 1)) for i in range(n)})


def references(c, d, kind):
    """(ref64, S, e_f32), [N][H][H][Cout']: the autograd gradient of the plain forward (+ res), the element's absolute sum over the
    backward operator, and max |f32 - ref64| / S of the float32 CPU evaluation of the same algorithm."""
    w, dy, res = d["w"], d["dy"], d["res"]
    N, H = c.N, c.H
    if c.cls == "stem":
        ref = R.stem_bwd(dy.reshape(-1, c.O), w).reshape(N, H, H, -1)
    elif c.cls in LINEAR:
        ref = R.linear_bwd(dy.reshape(-1, c.O), w.reshape(c.O, c.I)).reshape(N, H, H, -1)
    elif c.cls == "down":
        ref = R.conv_bwd(d["d_out"], w, H, stride=2)
    else:
        ref = R.conv_bwd(dy, w, H)
    if res is not None:
        ref = ref + res.double()
    wb = R.bwd_weight(w, kind if kind in ("linear", "stem") else "conv")
    if kind == "wino":
        S = wino_ref(dy.double(), wb, res=res, absolute=True)
        f32, sel = wino_ref(dy, wb, res=res, dtype=torch.float32).double(), slice(None)
    else:
        S = conv_ref(dy.double(), wb, res=res, absolute=True)
        sel = f32_frames(N, H * H)
        f32 = conv_ref(dy[sel], wb, res=None if res is None else res[sel], dtype=torch.float32, sequential=True, first=kind != "generic").double()
    S = S.clamp_min(1e-300)
    return ref, S, float(((f32 - ref[sel]).abs() / S[sel]).max())


class Launcher:
    def __init__(self, c, d, kind):
        self.c, self.kind = c, kind
        self.img = pack(kind, d["w"]).to("cuda")
        self.res = None if d["res"] is None else guarded_in(d["res"])
        self.Nb = R.STEM_KPAD if c.cls == "stem" else c.I

    def launch(self, dy, inplace=False):
        """dy: a device tensor [N][H][H][O].  -> Guarded out; inplace: out preloaded with the residual and passed as res."""
        c, p, st = self.c, _lib.ptr, _lib.current_stream()
        out = Guarded((c.N, c.H, c.H, self.Nb))
        res = self.res
        if inplace:
            out.t.copy_(self.res)
            res = out.t
        if c.cls in LINEAR:
            rc = L().vd_op_linear_bwd_data(p(dy), c.N * c.H * c.H, c.O, p(self.img), p(res), p(out.t), self.Nb, st)
        else:
            rc = L().vd_op_conv3_bwd_data(p(dy), c.N, c.H, c.O, p(self.img), KIND[self.kind], c.I, p(res), p(out.t), st)
        _lib.check(rc)
        torch.cuda.synchronize()
        return out


def err(out, ref, S):
    got = out.t.cpu().double()
    return float(((got - ref).abs() / S).max()) if bool(torch.isfinite(got).all()) else float("nan")


def run_case(c):
    """Launch a case in the process' own mode and measure it: a dict of plain numbers, strings and booleans (one JSON line of the tool)."""
    mode = process_mode()
    kind = kind_of(c.cls, c.H, c.O, c.I, mode)
    rc, name = variant_of(c.cls, c.N, c.H, c.O, c.I, c.res)
    r = {"label": label(c), "cls": c.cls, "kind": kind, "variant": name, "variant_rc": rc, "expected_variant": variant_name(c, mode), "mode": mode}
    if "+ksplit" in c.variant:
        r["ksplit"], r["ksplit_stated"] = L().vd_conv_wino_ksplit(c.N, c.H, c.O, c.I), int(c.variant.rsplit("+ksplit", 1)[1])
    d = make_inputs(c)
    dev = Launcher(c, d, kind)
    dy = guarded_in(d["dy"])
    ref, S, e_f32 = references(c, d, kind)
    one = dev.launch(dy)
    r["e_got"], r["e_f32"] = err(one, ref, S), e_f32
    r["margins_untouched"] = one.untouched()
    two = dev.launch(dy)
    r["rerun_same_bits"] = two.untouched() and same_bits(two.t, one.t)
    if c.res:
        three = dev.launch(dy, inplace=True)
        r["inplace_same_bits"] = three.untouched() and same_bits(three.t, one.t)
    if c.mags:
        # dy 2^k: as it is (recorded: what launch_grad_rescale is for), and through vd_op_grad_rescale -> the call -> * gs[1] (required)
        assert not c.res                                                                  # (linear in dy: ref and S scale with it)
        for k in SCALES:
            f = 2.0 ** k
            refk, Sk = ref * f, S * f
            g = guarded_in(d["dy"] * f)
            r[f"e_plain_2^{k}"] = err(dev.launch(g), refk, Sk)
            gs = torch.zeros(4, device="cuda")
            _lib.check(L().vd_op_grad_rescale(_lib.ptr(g), g.numel(), _lib.ptr(gs), _lib.current_stream()))
            out = dev.launch(g)
            out.t.mul_(gs[1])
            r[f"e_rescaled_2^{k}"] = err(out, refk, Sk)
            r[f"s_2^{k}"] = float(gs[0])
    return r


def bound(r):
    return max(FACTOR * r["e_f32"], FLOOR[r["mode"]])


def failures(r):
    """What a measured case (run_case's dict, or a line of the tool) fails: a list of strings, empty if it passes."""
    bad, b = [], bound(r)
    if r["variant_rc"] != 1 or r["variant"] != r["expected_variant"]:
        bad.append(f"runs {r['variant']}, the case names {r['expected_variant']}")
    if "ksplit" in r and r["ksplit"] != r["ksplit_stated"]:
        bad.append(f"vd_conv_wino_ksplit gives {r['ksplit']} slices, the case states {r['ksplit_stated']}")
    if not r["margins_untouched"]:
        bad.append("the margins around the output were written")
    if not r["rerun_same_bits"]:
        bad.append("a second launch gave other bits")
    if not r.get("inplace_same_bits", True):
        bad.append("the residual in place (res == out) gave other bits than out of place")
    if not r["e_got"] <= b:
        bad.append(f"e_got {r['e_got']:.3e} > max({FACTOR:g} x e_f32 {r['e_f32']:.3e}, {FLOOR[r['mode']]:.3e}) = {b:.3e}")
    for k in SCALES:
        key = f"e_rescaled_2^{k}"
        if key in r and not r[key] <= b:
            bad.append(f"rescaled route at dy 2^{k}: {r[key]:.3e} > {b:.3e}")
    return bad


def case_line(r):
    s = f"BWD_DATA_CASE | {r['label']} | {r['variant']} | {r['mode']} | {r['e_got']:.2e} | {r['e_f32']:.2e} | {bound(r):.2e}"
    for k in SCALES[1:]:
        if f"e_plain_2^{k}" in r:
            s += f" | 2^{k}: plain {r[f'e_plain_2^{k}']:.2e} rescaled {r[f'e_rescaled_2^{k}']:.2e}"
    return s
