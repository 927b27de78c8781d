"""numpy restatement of the green-hallway pixel count, written from the specification (OpenCV's documented 8-bit RGB -> HSV,
`inRange` and `erode` with a 2 x 2 kernel), not from csrc/hallway.hip.  OpenCV itself is not a dependency: test_room_seq_cpu.py
compares this file with cv2 wherever cv2 can be imported.

  hsv(rgb)            (..., 3) uint8 -> (..., 3) uint8, H in 0..179
  mask(rgb)           (...,) uint8, 255 where 50 <= H <= 70, S >= 25, V >= 25
  erode(mask)         (R, W) -> (R, W): anchor (1, 1), pixels outside the strip do not count
  quantise(x01)       (x * 255).astype(uint8) in float32: a truncation
  counts(frames)      (N, 3, H, W) uint8 or float in [0, 1] -> (N,) int64
"""
import numpy as np

_I = np.arange(1, 256, dtype=np.float64)
SDIV = np.concatenate([[0], np.rint(255.0 * 4096.0 / _I)]).astype(np.int64)
HDIV = np.concatenate([[0], np.rint(180.0 * 4096.0 / (6.0 * _I))]).astype(np.int64)
LOWER, UPPER = (50, 25, 25), (70, 255, 255)


def hsv(rgb):
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.shape[-1] == 3
    r, g, b = (rgb[..., c].astype(np.int64) for c in range(3))
    v = np.maximum(np.maximum(r, g), b)
    d = v - np.minimum(np.minimum(r, g), b)
    s = (d * SDIV[v] + 2048) >> 12
    hn = np.where(v == r, g - b, np.where(v == g, b - r + 2 * d, r - g + 4 * d))
    h = (hn * HDIV[d] + 2048) >> 12            # numpy's >> on signed integers is arithmetic
    h = np.where(h < 0, h + 180, h)
    return np.stack([h, s, v], axis=-1).astype(np.uint8)


def mask(rgb):
    x = hsv(rgb).astype(np.int64)
    ok = np.ones(x.shape[:-1], dtype=bool)
    for c in range(3):
        ok &= (x[..., c] >= LOWER[c]) & (x[..., c] <= UPPER[c])
    return np.where(ok, 255, 0).astype(np.uint8)


def erode(m):
    m = np.asarray(m)
    out = m.copy()
    out[:, 1:] = np.minimum(out[:, 1:], m[:, :-1])
    out[1:, :] = np.minimum(out[1:, :], m[:-1, :])
    out[1:, 1:] = np.minimum(out[1:, 1:], m[:-1, :-1])
    return out


def quantise(x01):
    return (np.asarray(x01, dtype=np.float32) * 255).astype(np.uint8)


def count_strip(strip_rgb):
    """strip (R, W, 3) uint8 -> the number of pixels left after mask and erosion."""
    return int(np.count_nonzero(erode(mask(strip_rgb))))


def counts(frames, rows=(14, 45)):
    frames = np.asarray(frames)
    if frames.dtype != np.uint8:
        frames = quantise(frames)
    assert frames.ndim == 4 and frames.shape[1] == 3
    strips = frames[:, :, rows[0]:rows[1]].transpose(0, 2, 3, 1)
    return np.array([count_strip(s) for s in strips], dtype=np.int64)
