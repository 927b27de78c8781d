"""Host side of the video_eval_room_seq_acc job and the self-checks of its yardstick (tests/hallway_restated.py); no GPU.

The restatement is checked against known answers worked out by hand from the adopted OpenCV arithmetic, and against cv2
itself wherever cv2 can be imported.  The host code (hallway.smooth_counts / classify / three_class_accuracy) is checked against
what the reference's own functions gave (tests/golden/room_seq_acc.json).  The job runs with the restatement injected as `counts=`."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

import hallway_restated as hr
from video_diffusion_amd import hallway
from video_diffusion_amd import video_eval_room_seq_acc as job
from video_diffusion_amd.video_sample import to_uint8


# ---------------------------------------------------------------------------------------------------- the restatement
def test_tables():
    assert hr.SDIV[0] == 0 and hr.HDIV[0] == 0
    assert hr.SDIV[255] == 4096 and hr.SDIV[1] == 255 * 4096 and hr.SDIV[3] == 348160
    assert hr.HDIV[255] == 482 and hr.HDIV[1] == 122880 and hr.HDIV[7] == 17554
    i = np.arange(1, 256)
    for num, tab in ((255 * 4096, hr.SDIV), (30 * 4096, hr.HDIV)):          # no quotient is a tie: the rounding is unambiguous
        assert not np.any((2 * num) % (2 * i) == i)
        assert np.array_equal(tab[1:], (2 * num + i) // (2 * i))


PURE = {(0, 255, 0): (60, 255, 255), (255, 0, 0): (0, 255, 255), (0, 0, 255): (120, 255, 255), (255, 0, 255): (150, 255, 255),
        (77, 77, 77): (0, 0, 77), (0, 0, 0): (0, 0, 0), (255, 255, 255): (0, 0, 255), (255, 255, 0): (30, 255, 255),
        (0, 255, 255): (90, 255, 255)}

# pixel -> its HSV, by hand from the specification; three just inside and three just outside every bound of the mask
BOUNDS = {
    "H>=50": ({(89, 255, 0): (50, 255, 255), (127, 216, 81): (50, 159, 216), (66, 149, 24): (50, 214, 149)},
              {(90, 255, 0): (49, 255, 255), (102, 217, 35): (49, 214, 217), (119, 183, 82): (49, 141, 183)}),
    "H<=70": ({(0, 255, 89): (70, 255, 255), (2, 196, 66): (70, 252, 196), (4, 164, 57): (70, 249, 164)},
              {(0, 255, 90): (71, 255, 255), (91, 175, 122): (71, 122, 175), (26, 162, 74): (71, 214, 162)}),
    "S>=25": ({(230, 255, 230): (60, 25, 255), (201, 223, 204): (64, 25, 223), (129, 141, 127): (56, 25, 141)},
              {(231, 255, 231): (60, 24, 255), (202, 223, 205): (64, 24, 223), (135, 149, 136): (62, 24, 149)}),
    "V>=25": ({(0, 25, 0): (60, 255, 25), (14, 25, 14): (60, 112, 25), (4, 25, 5): (61, 214, 25)},
              {(0, 24, 0): (60, 255, 24), (11, 24, 9): (56, 159, 24), (9, 24, 11): (64, 159, 24)}),
}


def boundary_pixels():
    return np.array([p for inside, outside in BOUNDS.values() for p in list(inside) + list(outside)], dtype=np.uint8)


def test_pure_colours():
    for rgb, want in PURE.items():
        assert tuple(int(v) for v in hr.hsv(np.array(rgb, dtype=np.uint8))) == want, rgb
    assert hr.mask(np.array([(0, 255, 0)], dtype=np.uint8))[0] == 255
    for rgb in [(255, 0, 0), (0, 0, 255), (255, 0, 255), (77, 77, 77), (0, 0, 0), (255, 255, 255), (255, 255, 0), (0, 255, 255)]:
        assert hr.mask(np.array([rgb], dtype=np.uint8))[0] == 0, rgb


@pytest.mark.parametrize("bound", list(BOUNDS))
def test_mask_bounds(bound):
    inside, outside = BOUNDS[bound]
    for group, want_mask in ((inside, 255), (outside, 0)):
        for rgb, want in group.items():
            px = np.array(rgb, dtype=np.uint8)
            assert tuple(int(v) for v in hr.hsv(px)) == want, rgb
            assert int(hr.mask(px)) == want_mask, rgb


def test_negative_hue_wraps():
    # v == r and g < b: h' < 0, the floor of the arithmetic shift, then + 180
    assert tuple(int(v) for v in hr.hsv(np.array((255, 0, 1), dtype=np.uint8))) == (0, 255, 255)       # (-482 + 2048) >> 12 = 0
    assert tuple(int(v) for v in hr.hsv(np.array((255, 0, 5), dtype=np.uint8))) == (179, 255, 255)     # (-2410 + 2048) >> 12 = -1
    assert tuple(int(v) for v in hr.hsv(np.array((255, 0, 128), dtype=np.uint8))) == (165, 255, 255)


def _strip(R, W, green):
    s = np.zeros((R, W, 3), np.uint8)
    s[green] = (0, 255, 0)
    return s


def test_erosion_on_hand_made_strips():
    R, W = 31, 64
    full = np.ones((R, W), bool)
    assert hr.count_strip(_strip(R, W, full)) == R * W                      # the border does not erode
    row = np.zeros((R, W), bool); row[15] = True
    assert hr.count_strip(_strip(R, W, row)) == 0
    top = np.zeros((R, W), bool); top[0] = True
    assert hr.count_strip(_strip(R, W, top)) == W                           # row -1 does not count
    bottom = np.zeros((R, W), bool); bottom[R - 1] = True
    assert hr.count_strip(_strip(R, W, bottom)) == 0
    left = np.zeros((R, W), bool); left[:, 0] = True
    assert hr.count_strip(_strip(R, W, left)) == R                          # column -1 does not count
    right = np.zeros((R, W), bool); right[:, W - 1] = True
    assert hr.count_strip(_strip(R, W, right)) == 0
    yy, xx = np.mgrid[:R, :W]
    assert hr.count_strip(_strip(R, W, (yy + xx) % 2 == 1)) == 0            # checkerboard
    assert hr.count_strip(_strip(R, W, (yy + xx) % 2 == 0)) == 1            # ... of the other phase: (0, 0) has no in-strip neighbour
    block = np.zeros((R, W), bool); block[10:12, 20:22] = True
    m = hr.erode(hr.mask(_strip(R, W, block)))
    assert np.count_nonzero(m) == 1 and m[11, 21] == 255                    # the anchor is the block's lower right pixel
    corner = np.zeros((R, W), bool); corner[0, 0] = True
    assert hr.count_strip(_strip(R, W, corner)) == 1                        # (0, 0) keeps its own value
    band = np.zeros((R, W), bool); band[5:12] = True
    assert hr.count_strip(_strip(R, W, band)) == 6 * W


def test_counts_takes_the_strip_of_the_frame_not_the_frame():
    frames = np.zeros((2, 3, 64, 64), np.uint8)
    frames[0, 1, 13] = 255                       # the row above the strip is green: must not shield row 14 from the border rule
    frames[0, 1, 14] = 255
    frames[1, 1, 44:50] = 255                    # only row 44 is inside
    assert hr.counts(frames).tolist() == [64, 0]
    assert hr.counts(frames, rows=(13, 45)).tolist() == [128, 0]


def test_quantisation_truncates():
    u = np.arange(256, dtype=np.uint8)
    assert np.array_equal(hr.quantise((u / 255.0).astype(np.float32)), u)   # samples: the identity on all 256 levels
    gt01 = ((u.astype(np.float32) / np.float32(127.5) - 1) - (-1)) / 2      # a ground truth that was u / 127.5 - 1
    q = hr.quantise(gt01)
    assert gt01.dtype == np.float32 and int(np.sum(q != u)) == 63 and np.array_equal(u[q != u], q[q != u] + 1)
    assert q[25] == 24                           # level 25 truncates to 24 and rounds to 25: opposite sides of V >= 25


def test_restatement_against_opencv():
    """Settles the adopted arithmetic wherever OpenCV is installed; skipped elsewhere.  If it runs and disagrees, the restatement and
    the kernel are what change."""
    cv2 = pytest.importorskip("cv2")
    g = np.random.default_rng(5)
    px = np.concatenate([g.integers(0, 256, size=(1 << 16, 3), dtype=np.uint8), boundary_pixels(),
                         np.array(list(PURE), dtype=np.uint8)])
    want = cv2.cvtColor(px[None], cv2.COLOR_RGB2HSV)[0]
    assert np.array_equal(hr.hsv(px), want)
    assert np.array_equal(hr.mask(px), cv2.inRange(want[None], (50, 25, 25), (70, 255, 255))[0])
    for seed in range(20):
        strip = _random_strip(seed)
        m = cv2.inRange(cv2.cvtColor(strip, cv2.COLOR_RGB2HSV), (50, 25, 25), (70, 255, 255))
        m = cv2.erode(m, np.ones((2, 2), np.uint8), iterations=1)
        assert np.array_equal(hr.erode(hr.mask(strip)), m), seed


def _random_strip(seed, R=31, W=64):
    g = np.random.default_rng(100 + seed)
    strip = np.ascontiguousarray(g.integers(0, 256, size=(R, W, 3), dtype=np.uint8))
    for _ in range(6):                           # green-ish blobs, some touching the borders
        y0, x0 = int(g.integers(-4, R)), int(g.integers(-4, W))
        h, w = int(g.integers(2, 14)), int(g.integers(2, 24))
        blob = np.stack([g.integers(0, 90, (h, w)), g.integers(120, 256, (h, w)), g.integers(0, 90, (h, w))], -1).astype(np.uint8)
        ys, xs = slice(max(y0, 0), min(y0 + h, R)), slice(max(x0, 0), min(x0 + w, W))
        strip[ys, xs] = blob[ys.start - y0:ys.stop - y0, xs.start - x0:xs.stop - x0]
    return strip


# ---------------------------------------------------------------------------------------------------- host code against the fixture
@pytest.fixture(scope="module")
def fixture(golden_dir):
    with open(os.path.join(golden_dir, "room_seq_acc.json")) as f:
        return json.load(f)


def _records(fx):
    return [(f"short {n}", rec) for n, rec in fx["short"].items()] + [("long", fx["long"])]


def test_fixture_covers_what_it_should(fixture):
    assert sorted(int(n) for n in fixture["short"]) == [1, 2, 4, 5, 8, 9, 10, 12]
    L = fixture["long"]
    counts = np.array(L["counts"])
    assert counts.shape == (24, 264)
    assert min(fixture["class_sizes"]) >= 3 and sum(fixture["class_sizes"]) == 24
    assert max(L["hallway_enter_recover"]) >= 2                                               # enters twice, recovers twice
    assert any(h[0] == 1 for h in L["hallway"])                                               # inside the hallway at frame 0
    sm = np.array(L["smoothed"])
    assert any(e > 0 and s.max() > 1000 and s[np.argmax(s > 1000):].min() > 500 and s[np.argmax(s > 1000):].min() < 1000
               for e, s in zip(L["hallway_enter_stay"], sm))                                  # crosses 1000, dips, never falls to 500


def test_smooth_counts_against_reference(fixture):
    for name, rec in _records(fixture):
        counts = np.array(rec["counts"], dtype=np.int64)
        exact = hallway.smooth_counts(counts.astype(np.float64))
        assert exact.dtype == np.float64
        want_exact = np.array(rec["smoothed_float"])
        np.testing.assert_allclose(exact[::rec["float_every"]], want_exact, rtol=1e-9, atol=0, err_msg=name)
        # integer counts, as the job and the reference have them: every value is truncated when it is stored
        got = hallway.smooth_counts(counts)
        assert got.dtype == np.int64 and got.shape == counts.shape
        want = np.array(rec["smoothed"])
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=0, err_msg=name)
        assert np.array_equal(got, np.trunc(exact).astype(np.int64))
    one = fixture["short"]["1"]                                   # a single frame: its count over the sum of the five taps 1 .. 1/5
    assert one["counts"][0] == [1800] and one["smoothed"][0] == [600]


def test_classify_against_reference(fixture):
    for name, rec in _records(fixture):
        for smoothed in (np.array(rec["smoothed"], dtype=np.int64), hallway.smooth_counts(np.array(rec["counts"], dtype=np.int64))):
            flags, room_stay, enter_stay, recover = hallway.classify(smoothed, fixture["entry_thresh"], fixture["out_thresh"])
            assert np.array_equal(flags, np.array(rec["hallway"])), name
            assert room_stay.tolist() == rec["room_stay"], name
            assert enter_stay.tolist() == rec["hallway_enter_stay"], name
            assert recover.tolist() == rec["hallway_enter_recover"], name
    built = {"stay": (1, 0, 0), "enter_stay": (0, 1, 0), "recover": (0, 0, 1), "recover_twice": (0, 0, 2)}
    L = fixture["long"]
    for kind, *got in zip(L["built_as"], L["room_stay"], L["hallway_enter_stay"], L["hallway_enter_recover"]):
        assert tuple(got) == built[kind]


def test_three_class_accuracy_against_reference(fixture):
    L = fixture["long"]
    gt = [np.array(L[k]) for k in ("room_stay", "hallway_enter_stay", "hallway_enter_recover")]
    members = hallway.class_members(*gt)
    assert [m.tolist() for m in members] == fixture["class_members"]
    assert [len(m) for m in members] == fixture["class_sizes"]
    for case in fixture["single_stats"]:
        pred = [m[np.array(case["perm"])] for m in gt]
        assert hallway.three_class_accuracy(members, pred) == case["accuracy"]
    assert fixture["single_stats"][0]["accuracy"] == 1.0 and hallway.three_class_count(members, gt) == 24


def test_truncation_decides():
    """1000.8 stored into the integer array is 1000 and does not enter; the same counts as float64 do."""
    counts = np.array([[1000, 1000, 1000, 1000, 1004, 1000, 1000, 1000, 1000, 1000, 1000, 1000]])
    assert hallway.smooth_counts(counts)[0, 4] == 1000 and hallway.smooth_counts(counts.astype(float))[0, 4] == pytest.approx(1000.8)
    assert hallway.classify(hallway.smooth_counts(counts))[1].tolist() == [1.0]
    assert hallway.classify(hallway.smooth_counts(counts.astype(float)))[1].tolist() == [0.0]
    flat = np.full((1, 12), 1000)
    assert hallway.classify(hallway.smooth_counts(flat))[1].tolist() == [1.0]                 # never above 1000: stays in the room


# ---------------------------------------------------------------------------------------------------- the job
T, OBS, SIZE = 30, 4, 64
LOW, HIGH = 3, 25                    # band heights: (3 - 1) * 64 = 128 and (25 - 1) * 64 = 1536 pixels after erosion
STAY = [LOW] * T
ENTER = [LOW] * 14 + [HIGH] * (T - 14)
RECOVER = [LOW] * 10 + [HIGH] * 10 + [LOW] * (T - 20)
OBS_ONLY = [HIGH] * OBS + [0] * (T - OBS)                 # green in the observed frames alone: room stay once they are dropped
# video -> (ground truth, sample 0, sample 1)
SCRIPT = {0: (STAY, STAY, ENTER), 1: (ENTER, ENTER, ENTER), 3: (RECOVER, RECOVER, ENTER), 5: (OBS_ONLY, STAY, OBS_ONLY)}


def _paint(heights, seed):
    """(T, 3, 64, 64) in [-1, 1]: grey noise (r = g = b: never green) with a full-width pure green band of heights[t] rows from row 16
    of frame t.  Inside the strip its first row erodes: (h - 1) * 64 pixels are left."""
    g = np.random.default_rng(seed)
    u = np.repeat(g.integers(0, 256, size=(T, 1, SIZE, SIZE), dtype=np.uint8), 3, axis=1)
    for t, h in enumerate(heights):
        u[t, :, 16:16 + h] = np.array([0, 255, 0], np.uint8)[:, None, None]
    return u.astype(np.float32) / np.float32(127.5) - 1


def _make_eval_dir(tmp_path, size=SIZE):
    (tmp_path / "samples").mkdir()
    vids = np.zeros((6, T, 3, SIZE, SIZE), np.float32)
    for v, (gt, *samples) in SCRIPT.items():
        vids[v] = _paint(gt, v)
        for k, heights in enumerate(samples):
            np.save(tmp_path / "samples" / f"sample_{v:04d}-{k}.npy", to_uint8(_paint(heights, 100 * v + k + 1)))
    np.save(tmp_path / "samples" / "sample_0001-2.npy", to_uint8(_paint(STAY, 9)))       # a third sample: not among the first two
    np.save(tmp_path / "videos.npy", vids)
    return vids


def _args(tmp_path, **kw):
    ns = argparse.Namespace(eval_dir=str(tmp_path), videos=str(tmp_path / "videos.npy"), synthetic=False, obs_length=OBS, T=None,
                            num_samples=2, num_videos=None, entry_thresh=None, out_thresh=None, rows=None, out=None)
    for k, v in kw.items():
        setattr(ns, k, v)
    return ns


class Counts:
    """The restatement as the injected counting function."""

    def __init__(self):
        self.calls, self.frames = 0, 0

    def __call__(self, frames, rows):
        self.calls += 1
        self.frames += frames.shape[0]
        assert isinstance(frames, torch.Tensor) and frames.dtype in (torch.float32, torch.uint8) and frames.shape[1] == 3
        if frames.dtype == torch.float32:
            assert float(frames.min()) >= 0.0 and float(frames.max()) <= 1.0
        return hr.counts(frames.numpy(), rows)


def test_painted_counts():
    heights = [0, 1, 2, LOW, HIGH, 29]
    frames = hr.quantise((_paint(heights + [0] * (T - 6), 1)[:6] + 1) / 2)
    assert hr.counts(frames).tolist() == [0, 0, 64, 128, 1536, 28 * 64]


def test_job_with_restatement(tmp_path, capsys):
    _make_eval_dir(tmp_path)
    counts = Counts()
    out = tmp_path / "result.json"
    res = job.run(_args(tmp_path, out=str(out)), counts=counts)
    assert counts.calls == 2 * 4 and counts.frames == 4 * 3 * (T - OBS)      # per video: the ground truth, and its samples as one stack
    assert res["videos"] == [0, 1, 3, 5] and res["num_videos"] == 4 and res["num_samples"] == 2
    assert res["class_sizes"] == {"room_stay": 2, "hallway_enter_stay": 1, "hallway_enter_recover": 1}
    assert res["gt_indicators"] == {"room_stay": [1, 0, 0, 1], "hallway_enter_stay": [0, 1, 0, 0], "hallway_enter_recover": [0, 0, 1, 0]}
    assert res["sample_indicators"][0] == res["gt_indicators"]
    assert res["sample_indicators"][1] == {"room_stay": [0, 0, 0, 1], "hallway_enter_stay": [1, 1, 1, 0],
                                           "hallway_enter_recover": [0, 0, 0, 0]}
    assert res["gt_accuracy"] == 1.0 and res["accuracies"] == [1.0, 0.5]
    assert res["mean"] == 0.75 and res["stderr"] == 0.25 and res["max"] == 1.0      # std 0.25 / sqrt(2 - 1)
    assert res["rows"] == [14, 45] and res["entry_thresh"] == 1000 and res["out_thresh"] == 500 and res["T"] == T
    lines = capsys.readouterr().out.splitlines()
    assert lines[:7] == ["Num examples Class 1: 2", "Num examples Class 2: 1", "Num examples Class 3: 1", "3-class accuracies:",
                         "GT : acc=4/4 = 100.0%", "75.0% +- 25.0", "100.0%"]
    with open(out) as f:
        assert json.load(f) == res

    # the observed frames count when they are not dropped: video 5's ground truth then recovers, and its sample 0 is wrong
    res0 = job.run(_args(tmp_path, obs_length=0), counts=counts)
    assert res0["gt_indicators"]["hallway_enter_recover"] == [0, 0, 1, 1] and res0["accuracies"] == [0.75, 0.5]
    # --T cuts both sides: within 12 frames nobody has entered yet (video 3's two green frames smooth to 972 at the end)
    res12 = job.run(_args(tmp_path, T=12), counts=counts)
    assert res12["class_sizes"] == {"room_stay": 4, "hallway_enter_stay": 0, "hallway_enter_recover": 0}
    assert res12["accuracies"] == [1.0, 1.0] and res12["T"] == 12
    with pytest.raises(AssertionError):
        job.run(_args(tmp_path, T=T + 1), counts=counts)
    # other thresholds and rows are options: with rows 0:14 nothing green is in the strip
    res_rows = job.run(_args(tmp_path, rows=[0, 14]), counts=counts)
    assert res_rows["class_sizes"] == {"room_stay": 4, "hallway_enter_stay": 0, "hallway_enter_recover": 0}
    res_thr = job.run(_args(tmp_path, entry_thresh=100, out_thresh=50), counts=counts)          # 128 already counts as the hallway
    assert res_thr["gt_indicators"]["hallway_enter_stay"] == [1, 1, 1, 0]


def test_job_refusals(tmp_path):
    _make_eval_dir(tmp_path)
    counts = Counts()
    samples = tmp_path / "samples"
    # sample index 1 of video 3 is missing although the video has two files
    (samples / "sample_0003-1.npy").rename(samples / "sample_0003-4.npy")
    with pytest.raises(ValueError, match="video #3: no sample with index 1"):
        job.run(_args(tmp_path), counts=counts)
    (samples / "sample_0003-4.npy").unlink()
    with pytest.raises(AssertionError, match="Expected at least 2 samples for each video, but found 1 for video #3"):
        job.run(_args(tmp_path), counts=counts)
    # a wrong dtype is named before anything is computed
    np.save(samples / "sample_0003-1.npy", np.zeros((T, 3, SIZE, SIZE), np.float32))
    with pytest.raises(ValueError, match="sample_0003-1.npy: float32"):
        job.run(_args(tmp_path), counts=counts)
    np.save(samples / "sample_0003-1.npy", np.zeros((T, 3, SIZE, SIZE + 1), np.uint8))
    with pytest.raises(ValueError, match="sample_0003-1.npy"):
        job.run(_args(tmp_path), counts=counts)
    assert counts.calls == 0


def test_job_low_frames_need_rows(tmp_path):
    (tmp_path / "samples").mkdir()
    g = np.random.default_rng(0)
    vids = g.random((2, 6, 3, 32, 32), dtype=np.float32) * 2 - 1
    np.save(tmp_path / "videos.npy", vids)
    for v in range(2):
        np.save(tmp_path / "samples" / f"sample_{v:04d}-0.npy", to_uint8(vids[v]))
    counts = Counts()
    with pytest.raises(ValueError, match="lower than row 45.*--rows"):
        job.run(_args(tmp_path, num_samples=1, obs_length=2), counts=counts)
    assert counts.calls == 0
    with pytest.raises(ValueError, match="rows 7:40 do not lie inside a frame of 32 rows"):
        job.run(_args(tmp_path, num_samples=1, obs_length=2, rows=[7, 40]), counts=counts)
    res = job.run(_args(tmp_path, num_samples=1, obs_length=2, rows=[7, 23]), counts=counts)
    assert res["rows"] == [7, 23] and res["class_sizes"]["room_stay"] == 2 and res["accuracies"] == [1.0]
    assert np.isnan(res["stderr"])                                           # one sample: 0 / sqrt(0), as in the reference


def test_wrapper_refuses_before_it_looks_for_a_device():
    with pytest.raises(ValueError, match=r"\(N, 3, H, W\)"):
        hallway.hallway_counts(np.zeros((2, 4, 64, 64), np.uint8))
    with pytest.raises(ValueError, match="rows 14:45 do not lie inside a frame of 32 rows"):
        hallway.hallway_counts(torch.zeros(2, 3, 32, 32))
