"""The reference's 3-class accuracy of GQN-Mazes videos (scripts/video_eval_room_seq_acc.py) on given per-frame green-pixel counts:
`_smooth_seq`, `verify_hallway` (all four outputs) and `get_single_stats`.  The script's `_count_hallway_pixels` is OpenCV followed by
`_smooth_seq(np.array(counts))`; here the OpenCV half is replaced by the given integer counts, the rest is the script's own."""
import importlib.util
import os
import sys
import types

import numpy as np

from . import _reference
from ._common import save_json

ENTRY, OUT = 1000, 500
SHORT_LENGTHS = (1, 2, 4, 5, 8, 9, 10, 12)
T_LONG = 264
MARGIN = 1e-6                # relative distance every smoothed value keeps from a value at which a decision would flip


def _script():
    """scripts/video_eval_room_seq_acc.py loaded by path; its body under __main__ does not run.  The third-party modules it
    imports at the top and never reaches from the three functions recorded here (cv2, skimage.metrics, lpips, the TensorFlow FVD module,
    the dataset module) are empty stand-ins of our own, taken out of sys.modules again once the script is loaded."""
    _reference.load()
    sk = types.ModuleType("skimage")
    skm = types.ModuleType("skimage.metrics")
    skm.peak_signal_noise_ratio = skm.structural_similarity = None
    sk.metrics = skm
    stand_ins = {"cv2": types.ModuleType("cv2"), "skimage": sk, "skimage.metrics": skm,
                 "improved_diffusion.frechet_video_distance": types.ModuleType("improved_diffusion.frechet_video_distance")}
    before = {name: sys.modules.get(name) for name in stand_ins}
    sys.modules.update(stand_ins)
    try:
        spec = importlib.util.spec_from_file_location("ref_video_eval_room_seq_acc",
                                                      os.path.join(_reference.directory(), "scripts", "video_eval_room_seq_acc.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for name, old in before.items():
            if old is None:
                sys.modules.pop(name, None)
            else:
                sys.modules[name] = old
    return mod


def _profile(T, rng, segments, noise):
    """Integer counts of T frames: piecewise linear through `segments` [(frame, level), ...] plus uniform integer noise, clipped to
    what a 31 x 64 strip can hold after erosion."""
    frames, levels = zip(*segments)
    base = np.interp(np.arange(T), frames, levels)
    return np.clip(np.rint(base + rng.integers(-noise, noise + 1, size=T)), 0, 31 * 64).astype(np.int64)


def long_sequences():
    """24 sequences of 264 frames and what each is built to be.  Room walls put a few hundred green-ish pixels into a frame at
    most; the hallway fills most of the strip."""
    rng = np.random.default_rng(20240607)
    T, seqs = T_LONG, []

    def add(kind, segments, noise=40):
        seqs.append((kind, _profile(T, rng, segments, noise)))

    for level in (0, 60, 250, 420):                                              # never enters
        add("stay", [(0, level), (T - 1, level)], noise=min(40, level))
    add("stay", [(0, 100), (100, 930), (130, 100), (T - 1, 100)], noise=20)      # comes close to 1000, does not cross
    for start in (20, 90, 170, 230):                                             # enters and stays to the end
        add("enter_stay", [(0, 80), (start, 80), (start + 15, 1800), (T - 1, 1800)])
    add("enter_stay", [(0, 50), (60, 50), (80, 1500), (120, 1500), (140, 720), (180, 720), (200, 1700), (T - 1, 1700)])   # dips to 720: never <= 500
    add("enter_stay", [(0, 50), (100, 50), (115, 1400), (150, 1400), (170, 640), (T - 1, 640)], noise=30)                 # crosses 1000, ends above 500
    for start, length in ((15, 40), (60, 100), (120, 30), (200, 35)):            # enters and comes back
        add("recover", [(0, 120), (start, 120), (start + 12, 1750), (start + length, 1750), (start + length + 12, 120), (T - 1, 120)])
    add("recover", [(0, 1800), (40, 1800), (55, 90), (T - 1, 90)])               # starts inside the hallway at frame 0, leaves
    add("recover", [(0, 1600), (30, 1600), (45, 60), (150, 60), (165, 1700), (T - 1, 1700)])   # starts inside, leaves, enters again and stays
    for gap in (40, 90):                                                         # enters twice and recovers twice
        add("recover_twice", [(0, 70), (20, 70), (32, 1800), (60, 1800), (72, 70), (72 + gap, 70), (84 + gap, 1650), (110 + gap, 1650),
                              (122 + gap, 70), (T - 1, 70)])
    add("recover_twice", [(0, 1900), (25, 1900), (40, 30), (100, 30), (112, 1500), (160, 1500), (175, 200), (T - 1, 200)])
    add("recover", [(0, 40), (50, 40), (65, 1200), (100, 1200), (115, 560), (140, 560), (150, 380), (T - 1, 380)], noise=25)  # lingers above 500 first
    add("recover", [(0, 300), (200, 300), (212, 1900), (240, 1900), (252, 300), (T - 1, 300)])
    add("stay", [(0, 480), (T - 1, 480)], noise=40)
    add("enter_stay", [(0, 0), (255, 0), (T - 1, 1984)], noise=0)                # enters in the last frames
    assert len(seqs) == 24
    return seqs


def _check_margins(counts, mod):
    """No smoothed value -- before the reference truncates it to the integer dtype of its counts -- lies within MARGIN (relative) of a
    value at which `> 1000` or `> 500` on the truncated integer would flip: another numpy build cannot change an indicator."""
    exact = mod._smooth_seq(np.asarray(counts, dtype=np.float64))
    for edge in (OUT, OUT + 1, ENTRY, ENTRY + 1):
        gap = np.abs(exact - edge).min()
        assert gap > MARGIN * edge, f"a smoothed value lies {gap:.3g} from {edge}"


def _record(mod, counts, float_every=1):
    """What the script computes for sequences with these counts (B, T), through its own verify_hallway.  `smoothed` is what the
    script itself gets (integer counts: every value truncated on store); `smoothed_float` is its _smooth_seq on the same counts as
    float64, kept for every `float_every`-th sequence."""
    counts = np.asarray(counts, dtype=np.int64)
    _check_margins(counts, mod)
    mod._count_hallway_pixels = lambda seqs: mod._smooth_seq(np.array([[int(c) for c in row] for row in seqs]))
    smoothed = mod._count_hallway_pixels(counts)
    hallway, room_stay, enter_stay, recover = mod.verify_hallway(counts, ENTRY, OUT)
    return dict(counts=counts.tolist(), smoothed=smoothed.tolist(),
                smoothed_float=mod._smooth_seq(counts.astype(np.float64))[::float_every].tolist(), float_every=float_every,
                hallway=hallway.tolist(),
                room_stay=room_stay.tolist(), hallway_enter_stay=enter_stay.tolist(), hallway_enter_recover=recover.tolist())


def room_seq(out):
    mod = _script()
    real_count = mod._count_hallway_pixels
    try:
        rng = np.random.default_rng(7)
        short = {}
        for n in SHORT_LENGTHS:                  # three sequences per length: inside from frame 0, rising, random
            rows = [np.full(n, 1800), np.linspace(300, 1900, n).round(), rng.integers(0, 1985, size=n)]
            short[str(n)] = _record(mod, np.array(rows, dtype=np.int64))
        kinds, rows = zip(*long_sequences())
        long_rec = _record(mod, np.stack(rows), float_every=3)
        long_rec["built_as"] = list(kinds)
        gt = (long_rec["room_stay"], long_rec["hallway_enter_stay"], long_rec["hallway_enter_recover"])
        sizes = [int(np.sum(np.array(m) > 0)) for m in gt]
        assert min(sizes) >= 3 and max(long_rec["hallway_enter_recover"]) >= 2, sizes
        idxs = [np.nonzero((np.array(m) > 0).astype(int))[0] for m in gt]
        names = ("room stay", "hallway enter stay", "hallway enter recover")

        # predictions: the ground truth itself, and permutations of its sequences (a prediction of another class for some videos)
        prng = np.random.default_rng(11)
        stats = []
        for perm in [np.arange(24), np.roll(np.arange(24), 1), prng.permutation(24), prng.permutation(24), np.arange(24)[::-1]]:
            pred = [np.array(m)[perm] for m in gt]
            acc = mod.get_single_stats({n: (p, i) for n, p, i in zip(names, pred, idxs)})
            stats.append(dict(perm=[int(p) for p in perm], accuracy=float(acc)))
    finally:
        mod._count_hallway_pixels = real_count
    rec = dict(entry_thresh=ENTRY, out_thresh=OUT, short=short, long=long_rec, class_sizes=sizes,
               class_members=[[int(i) for i in ix] for ix in idxs], single_stats=stats)
    return [save_json(out, "room_seq_acc.json", rec, separators=(",", ":"))]
