"""GPU: the output head the forward runs (csrc/engine.hip: out_head() -- head_gemm_kernel in both launch forms or the generic fp32
kernel with the GroupNorm affine and SiLU in its operand load, then out_gather_kernel), through vd_op_out_head, per element against the
float64 restatement of tests/out_head_restated.py.  The case list is R.CASES, by the path vd_out_head_variant must name; every named
path is asserted to have run.  Every output lies between sentinel pads and is prefilled with NaN.

Bound (R.head_bound): |got - ref| <= max(4 e32, FLOOR) max|ref| per element, never above the project's bar 1e-4 + 1e-4 |ref|, where e32
is the error of the float32 run of the same restatement on the CPU and FLOOR = R.FLOOR = 1.3e-6 is three times the largest error
measured on an MI355X over this file's cases, relative to max|ref| (VD_MATH = f16x3, the default; the head's kernels are fp32 MFMA in
every mode):

    path             measured max |got - ref| / max|ref|      float32 restatement, max over the path's cases
    head_gemm/tpw2   3.41e-07                                 4.20e-07
    head_gemm/tpw8   2.40e-07                                 2.48e-07
    igemm/32         4.32e-07  (the largest: FLOOR = 3 x)     3.26e-07
    igemm/64         2.53e-07                                 2.53e-07

max|ref| is 24 .. 135 in these cases (the pixels at +-30), so FLOOR max|ref| is 3e-5 .. 1.8e-4 absolute before the cut at the bar.
Each case prints `OUT_HEAD_CASE | path | case | err e32 worst err/bound`, the last test the maxima of the run.
"""
import functools

import pytest
import torch

import out_head_restated as R
from helpers import Guarded
from video_diffusion_amd import _lib

pytestmark = pytest.mark.gpu
IDS = [f"{path}-{R.label(c)}" for path, c in R.ALL_CASES]
SEEN = {}                                      # path -> largest err of the cases that ran


def dev(t):
    return t.to("cuda").contiguous()


def variant(c):
    import ctypes
    name = ctypes.create_string_buffer(256)
    rc = _lib.lib().vd_out_head_variant(*c, name, 256)
    assert rc >= 0, _lib.lib().vd_last_error().decode()
    return rc, name.value.decode()


def run_head(h, A, B, w, b, host_w=False):
    """vd_op_out_head on device copies of CPU tensors (host_w: the weight stays on the CPU, the entry takes either) -> Guarded output."""
    nfr, H, W, C = h.shape
    out = Guarded(nfr, w.shape[0], H, W)
    bufs = [dev(h), dev(A), dev(B), w.contiguous() if host_w else dev(w), dev(b)]
    _lib.check(_lib.lib().vd_op_out_head(*[_lib.ptr(t) for t in bufs], nfr, H, W, C, w.shape[0], _lib.ptr(out.t), _lib.current_stream()))
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def reference(c):
    """(inputs, float64 reference, float32 run): computed once per case."""
    x = R.make_inputs(c)
    return x, R.head_ref(*x), R.head_ref(*x, dtype=torch.float32)


@pytest.mark.parametrize("path,c", R.ALL_CASES, ids=IDS)
def test_head_per_element(path, c):
    """Every output element of the case inside the bound; the path is the one the case was listed for; the last frame alone gives the
    bits it has inside the batch."""
    assert variant(c) == (1, path)
    (h, A, B, w, b), ref, ref32 = reference(c)
    got = run_head(h, A, B, w, b).read().double()
    bound, e32 = R.head_bound(ref, ref32, R.FLOOR)
    err = R.scaled_error(got, ref)
    worst = float(((got - ref).abs() / bound).max())
    print(f"OUT_HEAD_CASE | {path} | {R.label(c)} | err {err:.3e} e32 {e32:.3e} worst err/bound {worst:.3f}")
    SEEN[path] = max(SEEN.get(path, 0.0), err)
    assert worst <= 1.0, (err, e32, worst)
    if c[0] > 1:
        one = run_head(h[-1:], A[-1:], B[-1:], w, b).read()
        assert torch.equal(one[0].double(), got[-1])


def test_every_named_path_ran():
    """The four paths of vd_out_head_variant were all exercised by the cases above (this test runs after them)."""
    print("OUT_HEAD_MAXIMA | " + " ".join(f"{k} {v:.3e}" for k, v in sorted(SEEN.items())) + f" | FLOOR {R.FLOOR:.3e}")
    assert set(SEEN) == set(R.CASES), sorted(SEEN)


def test_weight_from_host_memory_gives_the_same_bits():
    """w_oihw is read with a copy that takes host or device memory."""
    c = R.CASES["igemm/32"][3]
    x, _, _ = reference(c)
    assert torch.equal(run_head(*x, host_w=True).read(), run_head(*x).read())


@pytest.mark.parametrize("c,why", [((1, 20, 20, 40, 3), "Cin must be a multiple of 32"), ((1, 32, 32, 132, 3), "Cin must be a multiple of 32"),
                                   ((1, 32, 32, 64, 4), "3 or 6 output channels"), ((1, 32, 32, 64, 8), "3 or 6 output channels"),
                                   ((0, 32, 32, 64, 3), "positive nfr, H, W and C")])
def test_refusals_by_message(c, why):
    """A shape the fallback does not take (C no multiple of 32 where head_gemm_kernel does not apply) and a Cout other than 3 | 6: refused
    by name before any launch, by the entry and by vd_out_head_variant alike; the output stays untouched."""
    nfr, H, W, C, Cout = c
    rc, name = variant(c)
    assert rc == 0 and name.startswith("refused: ") and why in name, name
    n = max(nfr, 1)
    g = torch.Generator().manual_seed(0)
    h, A, B = torch.randn(n, H, W, C, generator=g), torch.ones(n, C), torch.zeros(n, C)
    w, b = torch.randn(Cout, C, 3, 3, generator=g), torch.zeros(Cout)
    out = Guarded(n, Cout, H, W)
    bufs = [dev(h), dev(A), dev(B), dev(w), dev(b)]
    rc = _lib.lib().vd_op_out_head(*[_lib.ptr(t) for t in bufs], nfr, H, W, C, Cout, _lib.ptr(out.t), _lib.current_stream())
    assert rc == -1 and why in _lib.lib().vd_last_error().decode(), _lib.lib().vd_last_error().decode()
    assert out.untouched()
