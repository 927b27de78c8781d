#!/usr/bin/env python3
"""Every case of tests/backward_data_cases.py in ONE arithmetic mode of the library (VD_MATH is read once per process): run with
VD_MATH=f16x3 | bf16x6 (tests/test_gpu_backward_data.py starts it as a child for the split mode that is not the test process' own).
One JSON line per case -- label, variant, mode, e_got and e_f32 against the fp64 autograd gradient, the flags (margins untouched,
second launch and in-place residual bit-equal), the magnitude family; "failures" is what backward_data_cases.failures() finds in the
line (the parent asserts the same again) -- then one summary line.  An error of the
library or the device ends the run at that case: nothing more is launched."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from backward_data_cases import CASES, failures, process_mode, run_case  # noqa: E402


def main():
    mode = process_mode()
    failed, variants = [], set()
    for c in CASES:
        r = run_case(c)
        r["failures"] = failures(r)
        if r["failures"]:
            failed.append(r["label"])
        variants.add(r["variant"])
        print(json.dumps(r), flush=True)
    print(json.dumps({"summary": True, "mode": mode, "cases": len(CASES), "variants": sorted(variants), "failed": failed}), flush=True)


if __name__ == "__main__":
    main()
