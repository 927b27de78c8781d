#!/usr/bin/env python3
"""Generated gfx950 code of the Winograd conv kernels, one tree against another (no GPU needed):
  python tools/wino_asm_diff.py <parent tree> <this tree> [--files conv_wino_r64.hip ...] [--flags="-DVD_R64_ABL=29"] > profiles/<tag>.txt
Every named kernel file of both trees is compiled to assembly with the product's flags (_lib._toolchain() + SOURCE_FLAGS of the SECOND
tree, --cuda-device-only -S).  Per kernel symbol: registers, scratch, LDS, and the opcode histogram split at the kernel's last v_mfma
in execution order (prologue + main loop | epilogue: the instructions behind which no MFMA can follow).  Register allocation differs between any two builds, so the text is not compared; what a refactor
of these one-wave-per-SIMD loops must keep, up to the last MFMA, is checked and printed as PASS / FAIL per kernel:
  scratch, VGPRs, AGPRs, LDS not higher (no scratch where there was none); the same number of v_mfma*, of every buffer_load* / global_load* / ds_read* / ds_write* opcode, of s_barrier;
  the same sequence of s_waitcnt immediates (the hand-placed vmcnt values are the schedule); not more instructions in total.
Exit status 1 if a kernel fails."""
import argparse
import collections
import hashlib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

FILES = ["conv_wino_r64.hip", "conv_wino_z128.hip", "conv_wino.hip"]
PKG = "video-diffusion_amd"
KEYS = [".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size"]


def load_lib(tree):
    spec = importlib.util.spec_from_file_location("_vd_lib", os.path.join(tree, PKG, "_lib.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def compile_asm(tree, src, hipcc, flags, out):
    cmd = [hipcc, *flags, "--cuda-device-only", "-S", os.path.join(tree, PKG, "csrc", src), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(" ".join(cmd) + "\n" + r.stdout + r.stderr)
    return open(out).read()


def parse(text):
    """symbol -> dict(meta, pre, epi, waits, masked_sha): pre / epi = opcode Counters up to and behind the last v_mfma"""
    lines = text.split("\n")
    meta, cur = {}, None
    for ln in lines:                                  # kernel-level keys of .amdgpu_metadata (argument entries are indented deeper)
        m = re.match(r"^(  - | {4})(\.\w+):\s*(.*)$", ln)
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
        if cur is not None:
            cur[m.group(2)] = m.group(3).strip()
            if m.group(2) == ".name":
                meta[cur[".name"]] = cur
    out = {}
    for sym, md in meta.items():
        start = next(i for i, ln in enumerate(lines) if ln.startswith(sym + ":"))
        # basic blocks: a label or the instruction behind a branch starts one
        blocks, labels, masked = [[]], {}, hashlib.sha1()
        for ln in lines[start + 1:]:
            if ln.startswith(".Lfunc_end"):
                break
            s = ln.split(";")[0].strip()
            m = re.match(r"^(\.LBB\d+_\d+):", s)
            if m:
                if blocks[-1]:
                    blocks.append([])
                labels[m.group(1)] = len(blocks) - 1
                continue
            if not s or s.startswith(".") or s.endswith(":"):
                continue
            blocks[-1].append(s)
            masked.update(re.sub(r"\b([vsa])\d+\b|\[\d+:\d+\]|\.LBB\d+_\d+", r"\1#", s).encode() + b"\n")
            if s.startswith(("s_branch", "s_cbranch", "s_endpgm", "s_setpc")):
                blocks.append([])
        succ = []
        for i, b in enumerate(blocks):
            last = b[-1].split() if b else ["-"]
            nxt = [i + 1] if i + 1 < len(blocks) else []
            if last[0] == "s_branch":
                succ.append([labels[last[1]]])
            elif last[0].startswith("s_cbranch"):
                succ.append([labels[last[-1]]] + nxt)
            elif last[0] in ("s_endpgm", "s_setpc_b64"):
                succ.append([])
            else:
                succ.append(nxt)
        # "Up to the last MFMA" in EXECUTION order: hipcc lays cold blocks of the epilogue out in front of the loop, and the sub-pixel
        # kernel holds two bodies whose structurised control flow runs one into the other.  With D = the blocks that dominate a block
        # with MFMAs (the spine of a prologue, and the loop), a block belongs to prologue + main loop if it is in D, or if the MFMA blocks
        # that its nearest dominator in D dominates all lie ahead of it (none of them reaches it): a side block of a prologue.
        n = len(blocks)
        reach = [{i} for i in range(n)]                       # reach[i]: blocks reachable from i (i included)
        changed = True
        while changed:
            changed = False
            for i in range(n - 1, -1, -1):
                new = set().union(reach[i], *(reach[j] for j in succ[i]))
                if len(new) != len(reach[i]):
                    reach[i], changed = new, True
        live = reach[0]
        pred = [[i for i in live if j in succ[i]] for j in range(n)]
        dom = [set(live) for _ in range(n)]
        dom[0] = {0}
        changed = True
        while changed:
            changed = False
            for j in sorted(live - {0}):
                new = set.intersection(*(dom[i] for i in pred[j])) | {j}
                if new != dom[j]:
                    dom[j], changed = new, True
        mf = [i for i in live if any(x.startswith("v_mfma") for x in blocks[i])]
        spine = set().union(set(), *(dom[m] for m in mf))
        in_pre = []
        for i in range(n):
            if i not in live or not mf:
                in_pre.append(False)
            elif i in spine:
                in_pre.append(True)
            else:
                s_i = max(dom[i] & spine, key=lambda d: len(dom[d]))          # the nearest dominator on a spine
                in_pre.append(not any(i in reach[m] for m in mf if s_i in dom[m]))
        pre, epi, waits, loop_waits = collections.Counter(), collections.Counter(), [], []
        for i, b in enumerate(blocks):
            last_mfma = max((k + 1 for k, x in enumerate(b) if x.startswith("v_mfma")), default=0)
            cut = 0 if not in_pre[i] else len(b) if not last_mfma or any(i in reach[j] for j in succ[i]) else last_mfma
            for k, x in enumerate(b):
                op = x.split()[0]
                (pre if k < cut else epi)[op] += 1
                if op == "s_waitcnt" and k < cut:
                    waits.append(" ".join(x.split()[1:]))
            if cut and any(x.startswith("v_mfma") for x in b):      # the waits of the blocks that issue MFMAs: the main loops themselves
                loop_waits.append([" ".join(x.split()[1:]) for x in b[:cut] if x.startswith("s_waitcnt")])
        out[kernel_key(sym)] = dict(meta=md, pre=pre, epi=epi, waits=waits, loop_waits=sorted(loop_waits), masked_sha=masked.hexdigest()[:12])
    return out


def kernel_key(sym):
    """demangled name without the argument list: a kernel keeps its key when an argument struct is renamed"""
    for filt in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "c++filt"):
        try:
            return subprocess.run([filt, sym], capture_output=True, text=True, check=True).stdout.strip().rsplit("(", 1)[0]
        except (OSError, subprocess.CalledProcessError):
            continue
    return sym


def pinned(op):
    return op.startswith(("v_mfma", "buffer_load", "global_load", "ds_read", "ds_write")) or op == "s_barrier"


def check(a, b):
    fails = []
    # (scratch: 0 stays 0; the fp32 kernel of conv_wino.hip spills 8 / 12 bytes as it stands, which must not grow)
    for k in (".private_segment_fixed_size", ".vgpr_count", ".agpr_count", ".group_segment_fixed_size"):
        if int(b["meta"].get(k, 0)) > int(a["meta"].get(k, 0)):
            fails.append(k)
    for op in sorted(set(a["pre"]) | set(b["pre"])):
        if pinned(op) and a["pre"][op] != b["pre"][op]:
            fails.append(f"{op} {a['pre'][op]} -> {b['pre'][op]}")
    if a["loop_waits"] != b["loop_waits"]:
        fails.append("s_waitcnt sequence of the blocks with MFMAs")
    elif a["waits"] != b["waits"]:
        fails.append("s_waitcnt sequence in front of the main loop")
    if sum(b["pre"].values()) > sum(a["pre"].values()):
        fails.append(f"instructions up to the last MFMA {sum(a['pre'].values())} -> {sum(b['pre'].values())}")
    return fails


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("tree")
    ap.add_argument("--files", nargs="+", default=FILES)
    ap.add_argument("--flags", default="", help="extra hipcc flags for both trees (an ablation / timing build)")
    ap.add_argument("--full", action="store_true", help="print every opcode, not only those whose counts differ")
    args = ap.parse_args()
    lib = load_lib(args.tree)
    hipcc, flags = lib._toolchain()
    bad = 0
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=min(6, os.cpu_count() or 1)) as pool:
        jobs = {(t, f): pool.submit(compile_asm, t, f, hipcc, flags + lib.SOURCE_FLAGS.get(f, []) + args.flags.split(), os.path.join(tmp, f"{i}_{f}.s"))
                for i, t in enumerate((args.parent, args.tree)) for f in args.files}
        print("flags:", " ".join(flags + args.flags.split()))
        for f in args.files:
            pa, pr = parse(jobs[(args.parent, f)].result()), parse(jobs[(args.tree, f)].result())
            for sym in sorted(set(pa) | set(pr)):
                print(f"\n== {f}: {sym}")
                if sym not in pa or sym not in pr:
                    print("   only in", "parent" if sym in pa else "tree")
                    bad += 1
                    continue
                a, b = pa[sym], pr[sym]
                for k in KEYS:
                    print(f"   {k:32s} {a['meta'].get(k, '-'):>8s} -> {b['meta'].get(k, '-'):>8s}")
                print(f"   {'instructions (..last MFMA | after)':32s} {sum(a['pre'].values())} | {sum(a['epi'].values())} -> {sum(b['pre'].values())} | {sum(b['epi'].values())}")
                print(f"   {'masked text sha':32s} {a['masked_sha']} -> {b['masked_sha']}")
                print(f"   s_waitcnt up to the last MFMA ({len(a['waits'])} -> {len(b['waits'])}): " + ("same sequence" if a["waits"] == b["waits"] else "DIFFERENT"))
                if args.full or a["waits"] != b["waits"]:
                    print("     parent: " + " , ".join(a["waits"]))
                    print("     tree: " + " , ".join(b["waits"]))
                print(f"   {'opcode':28s} {'..last MFMA':>16s} {'after':>16s}")
                for op in sorted(set(a["pre"]) | set(b["pre"]) | set(a["epi"]) | set(b["epi"])):
                    same = a["pre"][op] == b["pre"][op] and a["epi"][op] == b["epi"][op]
                    if args.full or pinned(op) or not same:
                        print(f"   {'' if same else '*'}{op:27s} {a['pre'][op]:7d} ->{b['pre'][op]:6d} {a['epi'][op]:7d} ->{b['epi'][op]:6d}")
                fails = check(a, b)
                bad += bool(fails)
                print("   " + ("PASS" if not fails else "FAIL: " + "; ".join(fails)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
