"""The 3-class accuracy of GQN-Mazes videos: does the agent stay in its room, enter the green hallway and stay there, or enter it and
come back -- the arithmetic of the reference's scripts/video_eval_room_seq_acc.py.

  hallway_counts        per frame, the number of green pixels that survive a 2 x 2 erosion inside rows 14..44 (`_count_hallway_pixels`
                        :126-137, there OpenCV one frame at a time), on the GPU: csrc/hallway.hip.
  smooth_counts         `_smooth_seq` (:106-123): the 9-tap triangle over a sequence's counts.
  classify              `verify_hallway` (:140-186): hysteresis on the smoothed counts -> per-frame flags and the three indicators.
  three_class_accuracy  `get_single_stats` (:198-203); three_class_count is the count `print_metrics` (:189-195) shows.

Smoothing and the state machine are N x T scalars and stay on the host in numpy: only the same expressions in the same order give
the same threshold decisions as the reference.  That includes the dtype: the reference allocates the smoothed array with
`np.zeros_like(counts)`, and its counts are integers, so every smoothed value is TRUNCATED to an integer when it is stored (1000.8
does not exceed 1000).  `smooth_counts` keeps its input's dtype for that reason, and `hallway_counts` returns int64.
"""
import numpy as np
import torch

from . import _lib
from .metrics import _device_tensor

ROWS = (14, 45)              # image[14:45]
ENTRY_THRESH = 1000
OUT_THRESH = 500
KERNEL = [i / 5.0 for i in range(1, 6)] + [i / 5.0 for i in range(4, 0, -1)]     # 1/5 .. 5/5 .. 1/5


def max_strip():
    """The largest strip (rows x W pixels) `hallway_counts` takes: its mask is held in LDS."""
    return int(_lib.lib().vd_hallway_max_strip())


def check_rows(H, rows):
    """ValueError unless 0 <= rows[0] < rows[1] <= H, before anything is launched."""
    r0, r1 = (int(r) for r in rows)
    if not 0 <= r0 < r1 <= H:
        raise ValueError(f"hallway counts: rows {r0}:{r1} do not lie inside a frame of {H} rows")
    return r0, r1


def hallway_counts_device(frames, rows=ROWS):
    """frames (N, 3, H, W), uint8 or float32 in [0, 1] (quantised as (uint8)(x * 255), truncated), contiguous on a GPU -> (N,) int32
    tensor on that GPU: the eroded green-pixel count of rows[0]:rows[1] of every frame.  Enqueued on the current stream."""
    if frames.ndim != 4 or frames.shape[1] != 3:
        raise ValueError(f"hallway counts: frames {tuple(frames.shape)} must be (N, 3, H, W)")
    if frames.dtype not in (torch.float32, torch.uint8):
        raise TypeError("hallway counts: frames uint8 or float32")
    if frames.device.type != "cuda" or not frames.is_contiguous():
        raise ValueError("hallway counts: a contiguous tensor on a GPU")
    N, _, H, W = frames.shape
    r0, r1 = check_rows(H, rows)
    counts = torch.empty(N, dtype=torch.int32, device=frames.device)
    with torch.cuda.device(frames.device):
        _lib.check(_lib.lib().vd_hallway_counts(N, H, W, r0, r1, _lib.ptr(frames), int(frames.dtype == torch.uint8),
                                                _lib.ptr(counts), _lib.current_stream()))
    return counts


def hallway_counts(frames, rows=ROWS, device=None):
    """frames (N, 3, H, W), uint8 or in [0, 1]; a tensor or an array on any device -> (N,) int64 numpy array."""
    shape = tuple(frames.shape)
    if len(shape) != 4 or shape[1] != 3:
        raise ValueError(f"hallway counts: frames {shape} must be (N, 3, H, W)")
    check_rows(shape[2], rows)
    if device is None:
        device = frames.device if isinstance(frames, torch.Tensor) and frames.device.type == "cuda" else \
            torch.device("cuda", torch.cuda.current_device())
    return hallway_counts_device(_device_tensor(frames, device), rows).cpu().numpy().astype(np.int64)


def green_mask(rgb, device=None):
    """rgb (n, 3) uint8 -> (hsv (n, 3) uint8, mask (n,) uint8 of 0 / 255) from the kernel's own per-pixel function (vd_op_green_mask)."""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    t = torch.as_tensor(rgb).to(device).contiguous()
    if t.ndim != 2 or t.shape[1] != 3 or t.dtype != torch.uint8:
        raise ValueError(f"green mask: rgb {tuple(t.shape)} {t.dtype} must be (n, 3) uint8")
    hsv = torch.empty_like(t)
    mask = torch.empty(t.shape[0], dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().vd_op_green_mask(t.shape[0], _lib.ptr(t), _lib.ptr(hsv), _lib.ptr(mask), _lib.current_stream()))
    return hsv.cpu().numpy(), mask.cpu().numpy()


def smooth_counts(seqs):
    """seqs (..., N) -> the same shape AND dtype: frame i is the triangle-weighted sum of frames i - 4 .. i + 4 (zeros outside the
    sequence) divided by the sum of the taps that fall inside it.  Integer input gives truncated integers, as in the reference.
    Below 9 frames the two end rules overlap and the first wins; the values are the reference's."""
    seqs = np.asarray(seqs)
    n, taps, half = seqs.shape[-1], len(KERNEL), len(KERNEL) // 2
    padded = np.zeros(list(seqs.shape[:-1]) + [n + taps - taps % 2])
    padded[..., half:-half] = seqs
    out = np.zeros_like(seqs)
    for i in range(n):
        if i < half:
            inside = KERNEL[half - i:]
        elif i >= n - half:
            inside = KERNEL[:-(i + half - n + 1)]
        else:
            inside = KERNEL
        out[..., i] = np.dot(padded[..., i:i + taps], KERNEL) / np.sum(inside)
    return out


def classify(smoothed, entry_thresh=ENTRY_THRESH, out_thresh=OUT_THRESH):
    """smoothed (B, T) -> (hallway (B, T), room_stay (B,), hallway_enter_stay (B,), hallway_enter_recover (B,)).  The agent enters
    at a smoothed count > entry_thresh and leaves at <= out_thresh.  room_stay: never entered; hallway_enter_stay: entered and has
    not left since; hallway_enter_recover: the number of times it left after entering (a sequence that starts inside counts)."""
    smoothed = np.asarray(smoothed)
    B, T = smoothed.shape
    hallway = np.zeros_like(smoothed)
    room_stay, enter_stay, enter_recover = np.zeros(B), np.zeros(B), np.zeros(B)
    for b in range(B):
        inside, left_once, may_recover = False, False, False
        room_stay[b] = 1.0
        for t in range(T):
            if inside:
                if smoothed[b, t] > out_thresh:
                    hallway[b, t] = 1.0
                else:
                    inside, left_once = False, True
                    enter_stay[b] = 0.0
                    if may_recover:
                        enter_recover[b] += 1
                        may_recover = False
            elif smoothed[b, t] > entry_thresh:
                hallway[b, t] = 1.0
                inside, may_recover = True, True
                room_stay[b] = 0.0
                if not left_once:
                    enter_stay[b] = 1.0
    return hallway, room_stay, enter_stay, enter_recover


def class_members(room_stay, enter_stay, enter_recover):
    """The three classes' member lists (:254-256), taken from the ground truth's indicators."""
    return tuple(np.nonzero(np.asarray(m) > 0)[0] for m in (room_stay, enter_stay, enter_recover))


def three_class_count(members, indicators):
    """The number of members whose own class indicator is > 0, over the three classes (the count `print_metrics` shows, :189-195)."""
    count = 0
    for idxs, met in zip(members, indicators):
        count += int(np.sum(np.asarray(met)[np.asarray(idxs, dtype=np.int64)] > 0))
    return count


def three_class_accuracy(members, indicators):
    """members: the ground truth's three index lists; indicators: (room_stay, enter_stay, enter_recover) of the sequences under
    test.  `three_class_count` divided by the number of sequences."""
    return three_class_count(members, indicators) / len(np.asarray(indicators[0]))
