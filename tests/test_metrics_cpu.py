"""Host side of the video_eval job and the self-checks of its yardstick (tests/metrics_restated.py); no GPU.

The job's host logic (video_eval.run: file discovery, drop of the observed frames, pickle name / keys / shapes, skip of finished modes,
the refusals) runs with the metric functions injected from the restatement, as video_sample.run takes `infer=`."""
import pickle

import numpy as np
import pytest
import torch

import metrics_restated as mr
from video_diffusion_amd import metrics as vmetrics
from video_diffusion_amd import video_eval as ve
from video_diffusion_amd.video_sample import to_uint8


def _planes(shape, seed):
    g = np.random.default_rng(seed)
    x = g.random(shape).astype(np.float32)
    y = np.clip(x + 0.1 * g.standard_normal(shape), 0, 1).astype(np.float32)
    return x, y


@pytest.mark.parametrize("H,W", [(7, 7), (8, 11), (9, 33), (33, 9), (64, 64), (100, 70), (128, 128)])
@pytest.mark.parametrize("R", [2.0, 1.0])
def test_filter_form_equals_valid_window_form(H, W, R):
    """skimage's form (uniform_filter over the whole plane, then the crop of 3 pixels) against the 7 x 7 windows that lie inside the
    plane, both in float64: the filter's border mode never reaches the cropped region."""
    x, y = _planes((H, W), H * 1000 + W)
    a, b = mr.ssim_plane(x, y, R, np.float64), mr.ssim_plane_valid(x, y, R)
    assert abs(a - b) <= 1e-13, (a, b)
    assert -1.0 <= a < 1.0


def test_uint8_to_float32_all_256_values():
    """float32 u / 255.0f equals (u / 255.0).astype(float32) for every uint8 value, in numpy and in torch (tensor divisor): a kernel may
    read the uint8 sample directly."""
    u = np.arange(256, dtype=np.uint8)
    want = mr.u8_to_float(u)
    assert want.dtype == np.float32
    assert np.array_equal(u.astype(np.float32) / np.float32(255.0), want)
    t = torch.from_numpy(u).to(torch.float32) / torch.full((), 255.0)
    assert np.array_equal(t.numpy(), want)


def test_psnr_inf_on_identical_planes():
    x, _ = _planes((16, 16), 3)
    assert mr.psnr_plane(x, x.copy()) == np.inf
    gt = np.stack([x, x, x])[None]
    pred = gt.copy()
    pred[0, 1, 2, 3] = 1.0 - pred[0, 1, 2, 3]                              # one channel differs: the frame's mean is still +inf
    s, p = mr.frame_ssim_psnr(gt, pred)
    assert p[0] == np.inf and np.isfinite(s[0])
    s, p = mr.frame_ssim_psnr(gt, gt.copy())
    assert p[0] == np.inf and abs(s[0] - 1.0) < 1e-12


def test_psnr_value():
    x = np.zeros((8, 8), np.float32)
    y = np.full((8, 8), 0.1, np.float32)
    want = 10 * np.log10(1.0 / float(np.float32(0.1) ** 2))
    assert abs(mr.psnr_plane(x, y) - want) < 1e-5


def test_below_7x7_raises_value_error():
    x, y = _planes((6, 20), 1)
    with pytest.raises(ValueError, match="win_size exceeds image extent"):
        mr.ssim_plane(x, y)
    with pytest.raises(ValueError, match="win_size exceeds image extent"):
        mr.ssim_plane_valid(x.T, y.T)
    # the package's wrapper refuses before it looks for a device
    with pytest.raises(ValueError, match="win_size exceeds image extent"):
        vmetrics.frame_ssim_psnr(np.zeros((2, 3, 6, 20), np.float32), np.zeros((2, 3, 6, 20), np.uint8))
    with pytest.raises(ValueError, match="win_size exceeds image extent"):
        vmetrics.frame_ssim_psnr(torch.zeros(2, 3, 20, 5), torch.zeros(2, 3, 20, 5))
    with pytest.raises(ValueError, match="same"):
        vmetrics.frame_ssim_psnr(torch.zeros(2, 3, 20, 20), torch.zeros(2, 3, 20, 21))


# ---------------------------------------------------------------------------------------------------- the job
T, OBS, SIZE = 6, 2, 12


def _videos():
    g = torch.Generator().manual_seed(77)
    return torch.rand(12, T, 3, SIZE, SIZE, generator=g) * 2 - 1


def _sample(vids, v, k):
    g = torch.Generator().manual_seed(1000 * v + k)
    noisy = (vids[v] + 0.2 * (k + 1) * torch.randn(vids[v].shape, generator=g)).clamp(-1, 1)
    return to_uint8(noisy.numpy())


def _make_eval_dir(tmp_path, n_samples=2, order=(11, 0, 2)):
    """Videos 0, 2 and 11 of twelve, written out of order: the pickle follows the sorted video index."""
    vids = _videos()
    (tmp_path / "samples").mkdir()
    for v in order:
        for k in range(n_samples):
            np.save(tmp_path / "samples" / f"sample_{v:04d}-{k}.npy", _sample(vids, v, k))
    np.save(tmp_path / "videos.npy", vids.numpy())
    return vids


class Calls:
    """The restatement as the injected metric functions, counting calls."""

    def __init__(self):
        self.metrics_calls, self.lpips_calls = 0, 0

    def metrics(self, gt01, pred, ssim_data_range):
        self.metrics_calls += 1
        assert gt01.dtype == torch.float32 and pred.dtype == torch.uint8 and gt01.shape == pred.shape
        assert float(gt01.min()) >= 0.0 and float(gt01.max()) <= 1.0
        return mr.frame_ssim_psnr(gt01.numpy(), pred.numpy(), ssim_data_range)

    def lpips(self, a, b):
        self.lpips_calls += 1
        assert a.dtype == torch.float32 and b.dtype == torch.float32 and a.shape == b.shape
        assert float(b.min()) >= -1.0 and float(b.max()) <= 1.0
        return ((a.double() - b.double()) ** 2).mean(dim=(1, 2, 3)).numpy()          # a stand-in that sees the [-1, 1] frames


def _args(tmp_path, modes, **kw):
    import argparse
    ns = argparse.Namespace(eval_dir=str(tmp_path), videos=str(tmp_path / "videos.npy"), synthetic=False, obs_length=OBS, modes=list(modes),
                            T=None, num_samples=None, dataset=None, dataset_partition="test", ssim_data_range=2.0, lpips_weights=None,
                            num_videos=None)
    for k, v in kw.items():
        setattr(ns, k, v)
    return ns


def test_job_discovery_drop_obs_and_pickle(tmp_path, capsys):
    vids = _make_eval_dir(tmp_path)
    found = ve.discover_samples(tmp_path)
    assert list(found) == [0, 2, 11]                                         # sorted by the video index in the names
    assert all(sorted(p.name for p in found[v]) == [f"sample_{v:04d}-0.npy", f"sample_{v:04d}-1.npy"] for v in found)
    calls = Calls()
    path = ve.run(_args(tmp_path, ["ssim", "psnr"]), metrics=calls.metrics, lpips=calls.lpips)
    assert path == tmp_path / f"metrics_3-2-{T}.pkl" and path.exists()
    with open(path, "rb") as f:
        got = pickle.load(f)
    assert sorted(got) == ["psnr", "ssim"]
    assert calls.metrics_calls == 6 and calls.lpips_calls == 0
    for m in got.values():
        assert m.shape == (3, 2, T - OBS) and m.dtype == np.float64
    # values: video i of the pickle is the i-th SORTED video index; the observed frames are dropped from both sides
    for i, v in enumerate(found):
        gt01 = ((vids[v].numpy() + 1) / 2).astype(np.float32)[OBS:]
        for k, p in enumerate(found[v]):
            ssim, psnr = mr.frame_ssim_psnr(gt01, np.load(p)[OBS:])
            assert np.array_equal(got["ssim"][i, k], ssim) and np.array_equal(got["psnr"][i, k], psnr)
    assert got["psnr"].mean() < 40                                           # noised samples, not the observed (identical) frames
    assert "Saved metrics to" in capsys.readouterr().out

    # a second run with one more mode adds to the pickle and recomputes nothing that is there
    path2 = ve.run(_args(tmp_path, ["ssim", "psnr", "lpips"]), metrics=calls.metrics, lpips=calls.lpips)
    assert path2 == path
    assert calls.metrics_calls == 6 and calls.lpips_calls == 6
    with open(path, "rb") as f:
        got2 = pickle.load(f)
    assert sorted(got2) == ["lpips", "psnr", "ssim"]
    assert np.array_equal(got2["ssim"], got["ssim"]) and np.array_equal(got2["psnr"], got["psnr"])
    assert got2["lpips"].shape == (3, 2, T - OBS) and got2["lpips"].dtype == np.float64 and (got2["lpips"] > 0).all()
    # a third run has nothing to do
    capsys.readouterr()
    ve.run(_args(tmp_path, ["all"]), metrics=calls.metrics, lpips=calls.lpips)
    out = capsys.readouterr().out
    assert "No metrics to compute." in out and "fvd is not computed here" in out
    assert calls.metrics_calls == 6 and calls.lpips_calls == 6


def test_job_T_and_num_samples_select(tmp_path):
    _make_eval_dir(tmp_path, n_samples=3)
    calls = Calls()
    path = ve.run(_args(tmp_path, ["psnr"], T=5, num_samples=2), metrics=calls.metrics)
    assert path.name == "metrics_3-2-5.pkl"
    with open(path, "rb") as f:
        got = pickle.load(f)
    assert list(got) == ["psnr"] and got["psnr"].shape == (3, 2, 5 - OBS)
    assert calls.metrics_calls == 6
    with pytest.raises(AssertionError):
        ve.run(_args(tmp_path, ["psnr"], T=T + 1), metrics=calls.metrics)


def test_job_too_few_samples_asserts(tmp_path):
    _make_eval_dir(tmp_path, n_samples=2)
    (tmp_path / "samples" / "sample_0002-1.npy").unlink()
    calls = Calls()
    with pytest.raises(AssertionError, match="Expected at least 2 samples for each video, but found 1 for video #2"):
        ve.run(_args(tmp_path, ["ssim"], num_samples=2), metrics=calls.metrics)
    assert calls.metrics_calls == 0


def test_job_refusals(tmp_path, capsys):
    _make_eval_dir(tmp_path)
    calls = Calls()
    with pytest.raises(SystemExit):                                          # at argument time
        ve.main(["--eval_dir", str(tmp_path), "--modes", "fvd"])
    assert "TF-Hub" in capsys.readouterr().err
    with pytest.raises(ValueError, match="TF-Hub"):
        ve.run(_args(tmp_path, ["ssim", "fvd"]), metrics=calls.metrics)
    # lpips without weights: before any file is read (the directory does not even exist)
    with pytest.raises(SystemExit):
        ve.main(["--eval_dir", str(tmp_path / "nowhere"), "--modes", "lpips"])
    assert "--lpips_weights" in capsys.readouterr().err
    with pytest.raises(ValueError, match="--lpips_weights"):
        ve.run(_args(tmp_path / "nowhere", ["lpips"]))
    # a sample that disagrees with the others is named before anything is computed
    bad = tmp_path / "samples" / "sample_0002-0.npy"
    np.save(bad, np.zeros((T, 3, SIZE, SIZE + 1), np.uint8))
    with pytest.raises(ValueError, match="sample_0002-0.npy"):
        ve.run(_args(tmp_path, ["ssim"]), metrics=calls.metrics)
    # ... and so is a ground truth of another size
    np.save(bad, np.zeros((T, 3, SIZE, SIZE), np.uint8))
    np.save(tmp_path / "videos.npy", np.zeros((12, T, 3, SIZE + 4, SIZE + 4), np.float32))
    with pytest.raises(ValueError, match="ground-truth video #0"):
        ve.run(_args(tmp_path, ["ssim"]), metrics=calls.metrics)
    assert calls.metrics_calls == 0
    assert not list(tmp_path.glob("metrics_*.pkl"))
