import argparse
import contextlib
import os
import shutil
import sys
import tempfile
import time

from . import MANIFEST, SKIPPED_KEYS, _reference
from ._common import REPO
from ._compare import compare
from .steps import probe_no_cond_marg


def generate(names, out):
    """Run the producers that own `names` (each once, in manifest order), writing into `out`."""
    for producer in dict.fromkeys(MANIFEST[n][0] for n in MANIFEST if n in names):
        t0 = time.time()
        with contextlib.redirect_stdout(sys.stderr):       # the producers' chatter; stdout is for the report
            wrote = producer(out)
        print(f"{producer.__module__.split('.')[-1]}.{producer.__name__}: {time.time() - t0:.0f} s ->",
              " ".join(os.path.basename(p) for p in wrote), file=sys.stderr)


def main():
    ap = argparse.ArgumentParser(prog="python -m tools.golden", description=sys.modules[__package__].__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    common = argparse.ArgumentParser(add_help=False)
    common.add_argument("--reference", default=_reference.DIR, metavar="DIR", help="the reference checkout (default %(default)s)")
    sub = ap.add_subparsers(dest="cmd", required=True)
    sub.add_parser("list", parents=[common], help="the manifest")
    for cmd, text in [("write", "(re)generate fixtures"), ("check", "regenerate into a temporary directory and compare with tests/golden/")]:
        p = sub.add_parser(cmd, parents=[common], help=text)
        p.add_argument("names", nargs="*", metavar="NAME", help="fixture files (default: all)")
    sub.choices["write"].add_argument("--out", default=os.path.join(REPO, "tests", "golden"), metavar="DIR")
    sub.add_parser("probe", parents=[common], help="do_cond_marg=False on the reference (writes nothing)")
    a = ap.parse_args()
    _reference.DIR = a.reference

    if a.cmd == "list":
        for name, (producer, seconds, full_size) in MANIFEST.items():
            print(f"{name:38s} {producer.__module__.split('.')[-1]}.{producer.__name__:20s} ~{seconds:3d} s"
                  f"{'  full-size model' if full_size else ''}")
        return 0
    if a.cmd == "probe":
        probe_no_cond_marg()
        return 0
    unknown = [n for n in a.names if n not in MANIFEST]
    if unknown:
        raise SystemExit(f"tools.golden: not in the manifest: {' '.join(unknown)}")
    names = a.names or list(MANIFEST)
    _reference.directory()                         # fail on a missing reference before any work
    committed = os.path.join(REPO, "tests", "golden")
    with tempfile.TemporaryDirectory() as tmp:
        generate(names, tmp)
        if a.cmd == "check":
            diffs = {n: d for n in names if (d := compare(os.path.join(committed, n), os.path.join(tmp, n), SKIPPED_KEYS.get(n, ())))}
            for n, d in diffs.items():
                print(f"DIFFERS {n}: {d}")
            print(f"{len(names) - len(diffs)} of {len(names)} fixtures equal the committed files")
            return 1 if diffs else 0
        os.makedirs(a.out, exist_ok=True)
        for n in names:
            dst = os.path.join(a.out, n)
            if n in SKIPPED_KEYS and os.path.exists(dst) and compare(dst, os.path.join(tmp, n), SKIPPED_KEYS[n]) is None:
                continue                           # only the stopwatch keys moved: keep the old file
            shutil.move(os.path.join(tmp, n), dst)
    return 0


if __name__ == "__main__":
    sys.exit(main())
