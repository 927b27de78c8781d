"""GPU: the green-hallway pixel count (csrc/hallway.hip: vd_hallway_counts, vd_op_green_mask) and the video_eval_room_seq_acc job
against the numpy restatement of the adopted OpenCV arithmetic (tests/hallway_restated.py).  Everything is integer arithmetic, so
every comparison is for equality: HSV bytes, mask bytes, counts and the job's result.

Shapes: the Mazes strip (64 x 64, rows 14:45), the 128 x 128 one, frames whose planes and strips are no multiple of 4 (the kernel's
pixel-by-pixel path), strips that start or end on the frame's border, a one-row strip, and two shapes that take the remaining load
paths: (8, 6) rows 0:3 -- aligned planes, a strip of 18 values: four-pixel loads with a two-pixel tail -- and (6, 6) rows 1:4 --
aligned planes, a strip that starts at an odd offset."""
import functools

import numpy as np
import pytest
import torch

import hallway_restated as hr
from test_room_seq_cpu import BOUNDS, Counts, _args, _make_eval_dir
from video_diffusion_amd import _lib, hallway
from video_diffusion_amd import video_eval_room_seq_acc as job

pytestmark = pytest.mark.gpu

SHAPES = [((64, 64), (14, 45)), ((3, 5), (0, 3)), ((7, 9), (2, 6)), ((64, 64), (30, 31)), ((128, 128), (28, 90)), ((45, 64), (14, 45)),
          ((8, 6), (0, 3)), ((6, 6), (1, 4))]
CONTENTS = ["green", "black", "checkerboard", "blobs", "edge_blobs"]
N_BLOBS = 4                          # frames per blob content


def _greenish(g, shape):
    """Pixels most of which pass the mask, some of which sit around its bounds."""
    return np.stack([g.integers(0, 100, shape), g.integers(110, 256, shape), g.integers(0, 100, shape)], 0).astype(np.uint8)


def _frames(content, H, W, rows, seed):
    """uint8 frames (n, 3, H, W) of one content."""
    g = np.random.default_rng(seed)
    r0, r1 = rows
    if content == "green":
        f = np.zeros((1, 3, H, W), np.uint8)
        f[:, 1] = 255
    elif content == "black":
        f = np.zeros((1, 3, H, W), np.uint8)
    elif content == "checkerboard":                                          # both phases
        yy, xx = np.mgrid[:H, :W]
        f = np.zeros((2, 3, H, W), np.uint8)
        f[0, 1] = 255 * ((yy + xx) % 2 == 0)
        f[1, 1] = 255 * ((yy + xx) % 2 == 1)
    else:
        f = g.integers(0, 256, size=(N_BLOBS, 3, H, W), dtype=np.uint8)
        for n in range(N_BLOBS):
            for b in range(4):
                h, w = int(g.integers(1, max(2, (r1 - r0) // 2 + 2))), int(g.integers(1, max(2, W // 2 + 2)))
                if content == "blobs":
                    y0, x0 = int(g.integers(0, H)), int(g.integers(0, W))
                else:                                                        # an edge on the strip's first / last row and column
                    y0 = (r0, r1 - h, r0, r1 - h)[b]
                    x0 = (0, W - w, W - w, 0)[b]
                ys, xs = slice(max(y0, 0), min(y0 + h, H)), slice(max(x0, 0), min(x0 + w, W))
                f[n, :, ys, xs] = _greenish(g, (ys.stop - ys.start, xs.stop - xs.start))
    return f


def _as_float(u8, seed):
    """float32 in [0, 1] whose truncation (not its rounding) is what the restatement sees: u / 255 plus up to one level."""
    g = np.random.default_rng(seed)
    return np.clip((u8.astype(np.float64) + g.random(u8.shape) * 0.98) / 255.0, 0.0, 1.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(shape, rows, content, dtype):
    """(frames, restated counts), computed once."""
    H, W = shape
    seed = 1000 * SHAPES.index((shape, rows)) + 10 * CONTENTS.index(content)
    frames = _frames(content, H, W, rows, seed)
    if dtype == "float32":
        frames = _as_float(frames, seed + 1)
    want = hr.counts(frames, rows)
    frames.setflags(write=False)
    want.setflags(write=False)
    return frames, want


def test_blob_cases_are_not_trivial():
    """At least half of the blob cases have a restated count strictly between 0 and the strip's size (CPU arithmetic only)."""
    inside = total = 0
    for shape, rows in SHAPES:
        size = (rows[1] - rows[0]) * shape[1]
        for content in ("blobs", "edge_blobs"):
            for dtype in ("uint8", "float32"):
                want = _case(shape, rows, content, dtype)[1]
                inside += int(np.sum((want > 0) & (want < size)))
                total += len(want)
    print(f"blob frames with 0 < count < strip size: {inside} of {total}")
    assert 2 * inside >= total


def test_exhaustive_colours():
    """All 2^24 RGB triples through vd_op_green_mask in one launch: HSV and mask bytes equal the restatement's."""
    v = torch.arange(1 << 24, dtype=torch.int32, device="cuda")
    rgb = torch.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], dim=1).to(torch.uint8)
    del v
    hsv, mask = hallway.green_mask(rgb)
    rgb = rgb.cpu().numpy()
    assert 0 < np.count_nonzero(mask) < mask.size
    step = 1 << 20
    for i in range(0, 1 << 24, step):
        want = hr.hsv(rgb[i:i + step]).astype(np.int64)
        assert np.array_equal(hsv[i:i + step], want), i
        ok = (want[:, 0] >= 50) & (want[:, 0] <= 70) & (want[:, 1] >= 25) & (want[:, 2] >= 25)
        assert np.array_equal(mask[i:i + step], np.where(ok, 255, 0)), i
    # the hand-worked pixels of the CPU test, through the kernel
    for inside, outside in BOUNDS.values():
        for group, want_mask in ((inside, 255), (outside, 0)):
            for px, want_hsv in group.items():
                i = (px[0] << 16) | (px[1] << 8) | px[2]
                assert tuple(int(c) for c in hsv[i]) == want_hsv and mask[i] == want_mask, px


def test_green_mask_without_hsv_output():
    rgb = torch.tensor([[0, 255, 0], [255, 0, 0], [89, 255, 0], [90, 255, 0]], dtype=torch.uint8, device="cuda")
    mask = torch.empty(4, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().vd_op_green_mask(4, _lib.ptr(rgb), None, _lib.ptr(mask), _lib.current_stream()))
    assert mask.cpu().tolist() == [255, 0, 255, 0]


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
@pytest.mark.parametrize("shape,rows", SHAPES, ids=[f"{s[0]}x{s[1]}_rows{r[0]}-{r[1]}" for s, r in SHAPES])
def test_counts(shape, rows, dtype):
    """Every content of a shape: frame by frame (N = 1), three at a time (N = 3) and all in one launch."""
    cases = [_case(shape, rows, c, dtype) for c in CONTENTS]
    frames = np.concatenate([f for f, _ in cases])
    want = np.concatenate([w for _, w in cases])
    size = (rows[1] - rows[0]) * shape[1]
    assert want[0] == size and want[1] == 0                                  # all green keeps every pixel, all black none
    dev = torch.from_numpy(frames.copy()).cuda()
    got = hallway.hallway_counts(dev, rows)
    assert got.dtype == np.int64 and np.array_equal(got, want), (got, want)
    assert np.array_equal(hallway.hallway_counts(frames, rows), want)        # a host array
    for n in range(len(frames)):                                             # alone: a frame's count does not depend on its batch
        assert hallway.hallway_counts(dev[n:n + 1], rows).tolist() == [want[n]], n
    for n in range(0, len(frames) - 2, 3):
        assert np.array_equal(hallway.hallway_counts(dev[n:n + 3], rows), want[n:n + 3]), n


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_counts_600_frames(dtype):
    """One launch over 600 frames of the Mazes shape, and items of it launched alone."""
    g = np.random.default_rng(600)
    base = np.concatenate([_case((64, 64), (14, 45), c, dtype)[0] for c in CONTENTS])
    want_base = np.concatenate([_case((64, 64), (14, 45), c, dtype)[1] for c in CONTENTS])
    pick = g.integers(0, len(base), size=600)
    frames = torch.from_numpy(base[pick]).cuda()
    got = hallway.hallway_counts(frames)
    assert np.array_equal(got, want_base[pick])
    for n in (0, 299, 599):
        assert hallway.hallway_counts(frames[n:n + 1]).tolist() == [want_base[pick[n]]]


def test_float_quantisation_truncates():
    """A ground truth that was u / 127.5 - 1, mapped to [0, 1] in float32: the kernel's (uint8)(x * 255.0f) is numpy's truncation.
    Level 25 truncates to 24 and would round to 25: with r = b = 0 that is V = 24 (outside the mask) against V = 25 (inside)."""
    u = np.arange(256, dtype=np.uint8)
    gt01 = ((u.astype(np.float32) / np.float32(127.5) - 1) - (-1)) / 2
    q = hr.quantise(gt01)
    assert int(np.sum(q != u)) == 63 and q[25] == 24 and q[24] == 23 and q[26] == 25
    uniform = np.zeros((256, 3, 64, 64), np.float32)                          # frame u: the whole frame at green level u
    uniform[:, 1] = gt01[:, None, None]
    want = hr.counts(uniform)
    assert want.tolist() == [0] * 26 + [31 * 64] * 230                       # levels 0 .. 25 give V <= 24
    assert np.array_equal(hallway.hallway_counts(uniform), want)
    rounded = np.zeros((256, 3, 64, 64), np.uint8)
    rounded[:, 1] = u[:, None, None]
    assert hr.counts(rounded)[25] == 31 * 64                                 # what rounding would have given
    yy, xx = np.mgrid[:64, :64]
    mixed = np.zeros((2, 3, 64, 64), np.float32)                             # one frame holding all 256 levels, in 2 x 2 cells
    mixed[0, 1] = gt01[((yy // 2) * 32 + xx // 2) % 256]
    mixed[1, 1] = gt01[(yy * 64 + xx) % 256]
    want = hr.counts(mixed)
    assert 0 < want[0] < 31 * 64
    assert np.array_equal(hallway.hallway_counts(mixed), want)
    # out of range and not-a-number are clamped to 0 .. 255, not wrapped
    odd = np.zeros((1, 3, 64, 64), np.float32)
    odd[0, 1] = 7.5
    odd[0, 0, 20] = -3.0
    odd[0, 2, 22] = np.nan
    assert hallway.hallway_counts(odd).tolist() == [31 * 64]


def test_lds_limit_is_named():
    limit = hallway.max_strip()
    assert limit == 48 * 1024
    frames = torch.zeros(1, 3, 256, 256, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.VdError, match=str(limit)):
        hallway.hallway_counts(frames, rows=(0, 256))
    frames[:, 1] = 255
    assert hallway.hallway_counts(frames, rows=(0, 192)).tolist() == [limit]                 # exactly at the limit
    assert hallway.hallway_counts(frames, rows=(100, 131)).tolist() == [31 * 256]            # a normal call afterwards
    with pytest.raises(_lib.VdError, match="row0 < row1"):
        _lib.check(_lib.lib().vd_hallway_counts(1, 256, 256, 5, 5, _lib.ptr(frames), 1, _lib.ptr(frames), _lib.current_stream()))


def test_job_on_gpu_equals_job_with_restatement(tmp_path, capsys):
    _make_eval_dir(tmp_path)
    want = job.run(_args(tmp_path), counts=Counts())
    lines = capsys.readouterr().out
    got = job.run(_args(tmp_path))
    assert got == want
    assert capsys.readouterr().out == lines
    assert got["accuracies"] == [1.0, 0.5] and got["class_sizes"]["hallway_enter_recover"] == 1
