#!/usr/bin/env python3
"""Every case of tests/conv_gemm_cases.py in ONE arithmetic mode of the library (VD_MATH is read once per process): run with
VD_MATH=f16x3 | bf16x6 | fp32 (tests/test_gpu_conv_gemm.py starts it as a child for every mode that is not the test process' own).
One JSON line per case -- label, variant, mode, e_got and e_f32 against the fp64 restatement, the flags (margins untouched, second
launch bit-equal, finite, table entries, frame subsets, single problems, side image); "failures" is what conv_gemm_cases.failures()
finds in the line (the parent asserts the same again) -- then one summary line with the names of vd_igemm_variant_list().  An error of
the library or the device ends the run at that case: nothing more is launched."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conv_gemm_cases import cases_for, failures, process_mode, run_case, variant_list  # noqa: E402


def main():
    mode = process_mode()
    cases = cases_for(mode)
    failed, variants = [], set()
    for c in cases:
        r = run_case(c)
        r["failures"] = failures(r)
        if r["failures"]:
            failed.append(r["label"])
        variants.add(r["variant"].split("+")[0])
        print(json.dumps(r), flush=True)
    print(json.dumps({"summary": True, "mode": mode, "cases": len(cases), "variants": len(variants), "table": variant_list(), "failed": failed}),
          flush=True)


if __name__ == "__main__":
    main()
