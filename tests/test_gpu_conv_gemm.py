"""GPU: every instantiation behind launch_igemm -- gemm_split_kernel<BM,BN,ACT,CONV,F16,SIDE> (16 per split arithmetic),
conv3x3_wino_r64_kernel / conv3x3_wino_r64_ups_kernel<TF4,F16> (4), conv3x3_wino_z128_kernel<ACT> (2, f16x3), gemm_frag_kernel<BM,BN,ACT> (8),
conv3x3_wino_kernel<TF4> (2), igemm_kernel<BM,BN> (4), with split-K and wino_r64_reduce_kernel -- element by element against float64, in
all three arithmetic modes: the test process' own here, the other two through tools/conv_gemm_check.py as a child process each.

The cases (tests/conv_gemm_cases.py) are compared with tests/conv_gemm_restated.py (checked against explicit loops in
test_conv_gemm_cpu.py).  vd_igemm_variant() names the instantiation a call runs on (the launchers dispatch through the same tables): every
case states the one it is here for, and the coverage test holds the cases to every name of vd_igemm_variant_list().
"""
import json
import os
import subprocess
import sys
import time

import pytest

from conv_gemm_cases import (CASES, FLOOR, Case, case_line, cases_for, failures, label, process_mode, run_case, variant_list, variant_name,
                             variant_of, F16X3_ALLOWANCE_LABELS)

pytestmark = pytest.mark.gpu
TABLE_SIZE = {"f16x3": 36, "bf16x6": 34, "fp32": 14}


def test_every_instantiation_is_run_and_every_case_runs_the_one_it_names():
    mode = process_mode()
    names = variant_list()
    assert len(names) == len(set(names)) == TABLE_SIZE[mode]
    cases = cases_for(mode)
    seen = set()
    for c in cases:
        rc, name = variant_of(c)
        assert rc == 1 and name == variant_name(c, mode), (label(c), name)
        seen.add(name.split("+")[0])
    missing = sorted(set(names) - seen)
    print(f"conv and GEMM, {mode}: {len(seen & set(names))} of {len(names)} instantiations run at op level")
    assert not missing and seen <= set(names), (missing, sorted(seen - set(names)))
    assert len(set(label(c) for c in CASES)) == len(CASES)
    assert len(F16X3_ALLOWANCE_LABELS) <= 3 and F16X3_ALLOWANCE_LABELS <= {label(c) for c in CASES}
    # split-K: 2, 3, 4, 6 and 8 slices at both map sizes
    assert {(c.H, c.variant.rsplit("+ksplit", 1)[1]) for c in CASES if "+ksplit" in c.variant} >= {(H, str(S)) for H in (8, 16) for S in (2, 3, 4, 6, 8)}


@pytest.mark.parametrize("c", [pytest.param(c, id=label(c)) for c in CASES])
def test_conv_gemm_per_element(c):
    """e = max over the elements of |out - ref64| / S, S = |bias| + |fbias| + |res| + sum |a| |w| of the element's own sum (Winograd
    kernels: S_w = ... + |A^T| (sum_c |U| . |V|) |A|, the same sum through the transforms; the sub-pixel form over its phase kernels).
    Required: e_got <= max(4 e_f32, FLOOR), e_f32 the same measure of the float32 CPU evaluation of the same algorithm (wino_ref in
    float32 for the Winograd kernels -- Winograd's own rounding is not a kernel fault -- torch fp32 for the rest), the factor 4 the
    project's (attn_spatial_cases.FACTOR), measured against the reference, never against another kernel.  FLOOR: three fp32 roundings of
    quantities <= S (result, bias, residual) = 2^-22 in bf16x6 and fp32; f16x3 adds the 2^-21 that include/vd_amd.h documents (22
    significand bits on each side of a product).  ACT instantiations subtract, per element, sum_k |w_k| d_k / S with d_k = 2e-6 (1 +
    |silu(a_k)|), the tolerance test_affine_act_pass holds the library's SiLU to.

    Every case also: the variant the library names is the one the case states (and vd_conv_wino_ksplit / vd_conv_wino_block_couts
    answer what it states); every output is finite; the inputs are read from the middle of buffers whose margins hold NaN; output,
    GroupNorm table and side image are written into the middle of NaN-filled buffers whose sentinel margins stay untouched; a second
    launch gives the same bits; every entry of a GroupNorm table equals the sums of its own block of the stored output (atol 1e-3, rtol
    1e-5: what tests/test_gpu_ops.py holds the totals to).  zero-frame: the frame is exactly bias + fbias + res.  Cases marked sel: frame
    subsets (another order, a single frame) launched with nfr_sel = N run the full launch's kernel and give its bits, output and table.
    Batched: every problem alone gives the same bits.  Side: the image is SiLU(a A + B) at test_affine_act_pass's tolerance.

    The float32 evaluation of the direct and GEMM kernels is conv_ref(sequential=True): one product and one addition per (tap, channel)
    in a fixed order, every one rounded to float32, the sum starting at bias + res where the kernel's accumulators do (gemm_frag.hip,
    gemm_split.hip) -- the plain float32 loop of the same algorithm.  A BLAS product is no such thing: it blocks the sum by the CPU's
    vector width and thread count, its error differs from machine to machine and is a fraction of a plain loop's (1.5 ulp of S against
    6 - 14 at K = 288).  The first GPU run used it: gemm_frag_kernel<64,64,false> on frag-N3H4-64c32x64-k1s1-res-mags then measured 7.16e-07
    (12.0 ulp) against 4 x 1.73e-07, and a CPU model of the kernel's own order -- accumulator at bias + res, then 64 fma in the MFMA's k
    order, round to nearest -- gives 12.01 ulp: the kernel IS the plain float32 evaluation, in another order.  For the big shapes the
    float32 loop runs on evenly spaced frames (conv_gemm_cases.f32_frames): a maximum over fewer elements, so the bound only tightens.

    The f16x3 allowance (conv_gemm_cases.F16X3_ALLOWANCE_LABELS; f16x3 only, by label, three): the GroupNorm table of conv_wino_z128.hip
    under the mags family.  wino_common.h (wino_out_rows / wino_stats_reduce) documents the arithmetic: a lane adds its 32 outputs of an
    item (sum, and sum of squares by fma) in fp32 and hands the two floats on as doubles.  A float32 sum of n terms is off by at most
    n 2^-24 sum |y|: the entry's tolerance grows by 32 x 2^-24 x (the block's sum of |y|, of y^2).  The mags outputs reach 1e3 .. 1e4,
    a block's sum of |y| 1e5 .. 1e6, and an ABSOLUTE 1e-3 is then about one float32 rounding of a single term:

        wino_split_k-N33H32-32x128-k3s1-res-gn-mags    worst entry 6.7e-04 beyond atol + rtol |want|; 1.4e-03 inside with the lane term
        wino_split_k-N136H16-32x128-k3s1-fb-gn-mags    1.3e-03 beyond; 1.0e-03 inside
        wino_split_k-N129H16-32x128-k3s1-gn-mags       9.5e-04 beyond; 1.0e-03 inside

    Every other table -- the same family on the 8 x 8 maps (8 terms per lane), the split-K reduce kernel and the GEMM epilogue (fp64
    throughout), conv_wino.hip -- is inside the plain tolerance, and the outputs of these three cases are inside the plain bound.  (The
    GEMM epilogue sums in fp64 since the stem's offsets were found to need it; the Winograd epilogues do not, which costs nothing at the
    network's magnitudes and is noted in docs/LAB_NOTES.md.)  Measured figures of all three modes: docs/LAB_NOTES.md."""
    mode = process_mode()
    if mode not in c.modes or c not in cases_for(mode):
        pytest.skip(f"not an instantiation of {mode}: its table must not hold {c.variant}")
    r = run_case(c)
    print(case_line(r))
    assert not failures(r), (r["label"], failures(r), r)


# ---------------------------------------------------------------------------------------------------- the envelope
def test_calls_outside_the_envelope_are_refused_by_name():
    plain = Case("generic", 2, 8, 32, 64, "")
    assert variant_of(plain._replace(Cin=33))[1].startswith("refused: Cin must be a multiple of 32")
    assert variant_of(plain._replace(k=5))[1].startswith("refused: kernel size 1 or 3")
    # no 3x3 split form activates its operand (the rows were unreachable and are gone)
    rc, name = variant_of(Case("conv_split", 2, 8, 32, 64, "", act=1))
    assert rc == 0 and "activated operand" in name, name
    # the side output off the 128x128 tile
    rc, name = variant_of(Case("side", 2, 16, 64, 128, "", C0=32, k=1))
    assert rc == 0 and name.startswith("refused: side output"), name


# ---------------------------------------------------------------------------------------------------- the other two modes
CHILD_DIED = []          # a child that ended by signal or timeout: nothing more is started on the GPU
CHILD_TIMEOUT = 300      # library load and device start (some 15 s) + the cases; measured child time: see docs/LAB_NOTES.md


@pytest.mark.parametrize("mode", ["f16x3", "bf16x6", "fp32"])
def test_every_case_in_every_other_arithmetic_mode(mode):
    """VD_MATH is read once per process: tools/conv_gemm_check.py runs the same table through the same run_case() as a fresh child
    process per mode, one at a time, and every line is held to the assertions of test_conv_gemm_per_element; the variants the child ran
    are exactly that mode's table.  The process' own mode is covered above and skipped here."""
    if mode == process_mode():
        pytest.skip("the test process' own mode: the tests above run in it")
    assert not CHILD_DIED, f"the {CHILD_DIED[0]} child ended by signal or timeout: no further child is started"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "conv_gemm_check.py")], env={**os.environ, "VD_MATH": mode},
                           capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        CHILD_DIED.append(mode)
        raise
    print(f"conv and GEMM, {mode}: child ran {time.time() - t0:.0f} s of {CHILD_TIMEOUT}")
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        CHILD_DIED.append(mode)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    lines = [json.loads(s) for s in r.stdout.splitlines() if s.startswith("{")]
    summary, rows = lines[-1], lines[:-1]
    cases = cases_for(mode)
    assert summary.get("summary") is True and summary["mode"] == mode and summary["cases"] == len(rows) == len(cases)
    for c, row in zip(cases, rows):
        print(case_line(row))
        assert row["label"] == label(c) and row["mode"] == mode and row["expected_variant"] == variant_name(c, mode)
        assert not failures(row), (row["label"], failures(row), row)
    names = summary["table"]
    assert sorted({row["variant"].split("+")[0] for row in rows}) == sorted(names) and len(names) == TABLE_SIZE[mode]
    print(f"conv and GEMM, {mode}: {len(names)} of {len(names)} instantiations run at op level")
    assert summary["failed"] == [] and summary["variants"] == len(names) and FLOOR[mode] > 0
