"""Content comparison of two fixture files: what `check` reports and what `write` uses to leave stopwatch noise alone."""
import json

import numpy as np


def _without(obj, skip):
    if isinstance(obj, dict):
        return {k: _without(v, skip) for k, v in obj.items() if k not in skip}
    if isinstance(obj, list):
        return [_without(v, skip) for v in obj]
    return obj


def _json_diff(a, b, where="$"):
    """The first place where two parsed JSON values differ, or None."""
    if type(a) is not type(b):
        return f"{where}: {type(a).__name__} != {type(b).__name__}"
    if isinstance(a, dict):
        if a.keys() != b.keys():
            return f"{where}: keys differ: {sorted(a.keys() ^ b.keys())}"
        return next((d for k in a if (d := _json_diff(a[k], b[k], f"{where}.{k}"))), None)
    if isinstance(a, list):
        if len(a) != len(b):
            return f"{where}: length {len(a)} != {len(b)}"
        return next((d for i in range(len(a)) if (d := _json_diff(a[i], b[i], f"{where}[{i}]"))), None)
    return None if a == b else f"{where}: {a!r} != {b!r}"


def _npz_diff(a, b):
    if set(a.files) != set(b.files):
        return f"key sets differ: {sorted(set(a.files) ^ set(b.files))}"
    for k in sorted(a.files):
        x, y = a[k], b[k]
        if x.dtype.kind in "US" or y.dtype.kind in "US":
            if x.dtype.kind != y.dtype.kind or x.shape != y.shape or x.tolist() != y.tolist():
                return f"key {k!r}: strings differ"
        elif x.dtype != y.dtype:
            return f"key {k!r}: dtype {x.dtype} != {y.dtype}"
        elif x.shape != y.shape:
            return f"key {k!r}: shape {x.shape} != {y.shape}"
        elif x.tobytes() != y.tobytes():
            bits = x.reshape(-1).view(np.uint8).reshape(x.size, -1) != y.reshape(-1).view(np.uint8).reshape(y.size, -1)
            with np.errstate(all="ignore"):
                delta = np.abs(x.astype(np.float64) - y.astype(np.float64)).max()
            return f"key {k!r}: max |delta| {delta:.3g}, {int(bits.any(1).sum())} of {x.size} elements differ"
    return None


def compare(path_a, path_b, skip_keys=()):
    """None when the two files hold the same content, else one line saying where they first differ.
    .npz: the same key set and, per key, the same dtype, shape and bit pattern (strings as strings); zip order and
    compression do not count.  .json: equality of the parsed objects, keys named in `skip_keys` left out at any depth."""
    if path_a.endswith(".npz"):
        with np.load(path_a) as a, np.load(path_b) as b:
            return _npz_diff(a, b)
    with open(path_a) as fa, open(path_b) as fb:
        return _json_diff(_without(json.load(fa), skip_keys), _without(json.load(fb), skip_keys))
