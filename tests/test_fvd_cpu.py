"""CPU: the host half of the video_fvd job -- the Frechet distance against the reference's lines restated with scipy's sqrtm
(tests/i3d_restated.py), the reading and BatchNorm folding of the I3D weights, the byte round trip of the reference, the job driven
through `run(embed=fake)`, and the SAME-padding arithmetic."""
import argparse

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import i3d_restated as ir
from video_diffusion_amd import fvd, video_fvd


# ---------------------------------------------------------------- Frechet distance
@pytest.mark.parametrize("N,D", [(1000, 400), (256, 400), (64, 400), (16, 400), (40, 16), (8, 16)])
def test_frechet_vs_restated(N, D):
    g = np.random.default_rng(N * 1000 + D)
    mix = g.standard_normal((D, D)) / np.sqrt(D)
    f1 = (g.standard_normal((N, D)) @ mix + 0.3 * g.standard_normal(D)).astype(np.float32)
    f2 = (1.2 * g.standard_normal((N, D)) @ mix.T + 0.3 * g.standard_normal(D)).astype(np.float32)
    got, want = fvd.frechet_distance(f1, f2), ir.frechet_restated(f1, f2)
    print(f"N={N} D={D}: got {got!r} want {want!r} rel {abs(got - want) / abs(want):.3e}")
    assert np.isfinite(got) and want > 0
    assert abs(got - want) <= 1e-6 * abs(want)


@pytest.mark.parametrize("N,D", [(256, 400), (8, 16), (40, 16)])
def test_frechet_identical_sets(N, D):
    f = np.random.default_rng(N + D).standard_normal((N, D)).astype(np.float32)
    d = fvd.frechet_distance(f, f.copy())
    assert abs(d) <= 1e-6 * np.trace(np.cov(f.astype(np.float64), rowvar=False))


def test_frechet_needs_two_videos():
    f = np.zeros((1, 400), dtype=np.float32)
    with pytest.raises(ValueError, match="at least 2 videos"):
        fvd.frechet_distance(f, np.zeros((5, 400), dtype=np.float32))
    with pytest.raises(ValueError, match="at least 2 videos"):
        fvd.frechet_distance(np.zeros((5, 400), dtype=np.float32), f)


# ---------------------------------------------------------------- weights
@pytest.fixture(scope="module")
def sd():
    return ir.synth_state_dict(0)


def test_weight_layouts_read_alike(sd, tmp_path):
    plain, nested, prefixed = tmp_path / "plain.pt", tmp_path / "nested.pt", tmp_path / "prefixed.pt"
    torch.save(sd, plain)
    torch.save({"state_dict": sd, "epoch": 3}, nested)
    torch.save({"module." + k: v for k, v in sd.items()}, prefixed)
    a, b, c = fvd.read_weights(plain), fvd.read_weights(nested), fvd.read_weights(prefixed)
    assert len(a) == 2 * 57 + 2 and set(a) == set(b) == set(c)
    for k in a:
        assert a[k].dtype == np.float32 and np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k])
    assert len(fvd.UNITS) == len(ir.unit_shapes()) == 57
    for (unit, cin, cout, k), (name, shape) in zip(fvd.UNITS, ir.unit_shapes()):
        assert unit == name and shape == (cout, cin, k, k, k)
        assert a[f"{unit}.weight"].shape == shape and a[f"{unit}.bias"].shape == (cout,)
    assert a["logits.weight"].shape == (400, 1024, 1, 1, 1) and a["logits.bias"].shape == (400,)


def test_missing_bn_weight_reads_as_one(sd):
    no_scale = {k: v for k, v in sd.items() if not k.endswith("bn.weight")}
    ones = {k: (torch.ones_like(v) if k.endswith("bn.weight") else v) for k, v in sd.items()}
    a, b = fvd.canonical_weights(no_scale), fvd.canonical_weights(ones)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_weight_refusals(sd):
    bad = dict(sd)
    del bad["Mixed_4c.b2a.conv3d.weight"]
    with pytest.raises(ValueError, match=r"missing key Mixed_4c\.b2a\.conv3d\.weight"):
        fvd.canonical_weights(bad)
    bad = dict(sd)
    bad["Mixed_3b.b1b.conv3d.weight"] = torch.zeros(128, 96, 3, 3, 1)
    with pytest.raises(ValueError, match=r"Mixed_3b\.b1b\.conv3d\.weight has shape \(128, 96, 3, 3, 1\), expected \(128, 96, 3, 3, 3\)"):
        fvd.canonical_weights(bad)
    bad = dict(sd)
    bad["Conv3d_2b_1x1.bn.bias"] = sd["Conv3d_2b_1x1.bn.bias"].clone()
    bad["Conv3d_2b_1x1.bn.bias"][3] = float("nan")
    with pytest.raises(ValueError, match=r"Conv3d_2b_1x1\.bn\.bias holds non-finite"):
        fvd.canonical_weights(bad)
    bad = dict(sd)
    bad["Mixed_5c.b3b.bn.running_var"] = sd["Mixed_5c.b3b.bn.running_var"].clone()
    bad["Mixed_5c.b3b.bn.running_var"][0] = -0.1
    with pytest.raises(ValueError, match=r"Mixed_5c\.b3b\.bn\.running_var has negative"):
        fvd.canonical_weights(bad)
    bad = dict(sd)
    del bad["logits.conv3d.bias"]
    with pytest.raises(ValueError, match=r"missing key logits\.conv3d\.bias"):
        fvd.canonical_weights(bad)


def test_batchnorm_fold_within_one_ulp(sd):
    """The folded weight and bias against the un-folded BatchNorm of the helper in float64: conv then F.batch_norm of a one-hot input
    gives back bias + weight column, which the float32 fold must meet within 1 ulp per entry (folded in float64, rounded once)."""
    w = fvd.canonical_weights(sd)
    for unit in ("Conv3d_1a_7x7", "Conv3d_2c_3x3", "Mixed_3b.b2a", "Mixed_4f.b1b", "Mixed_5c.b0"):
        cw = sd[f"{unit}.conv3d.weight"].to(torch.float64)
        cout = cw.shape[0]
        stat = [sd[f"{unit}.bn.{p}"].to(torch.float64) for p in ("running_mean", "running_var", "weight", "bias")]
        flat = cw.reshape(cout, -1).t().reshape(-1, cout, 1, 1, 1)             # every weight entry as a "conv output"
        full = F.batch_norm(flat, stat[0], stat[1], stat[2], stat[3], training=False, eps=ir.BN_EPS)
        zero = F.batch_norm(torch.zeros(1, cout, 1, 1, 1, dtype=torch.float64), stat[0], stat[1], stat[2], stat[3], training=False,
                            eps=ir.BN_EPS).reshape(cout)
        want_w = (full.reshape(-1, cout) - zero).t().reshape(cw.shape).numpy()
        got_w, got_b = w[f"{unit}.weight"].astype(np.float64), w[f"{unit}.bias"].astype(np.float64)
        ulp_w = np.spacing(np.abs(want_w).astype(np.float32)).astype(np.float64)
        ulp_b = np.spacing(np.abs(zero.numpy()).astype(np.float32)).astype(np.float64)
        # want_w is a difference of two float64 values of size |bias| + |w|: its own rounding error, a few float64 epsilons of that
        # size, is allowed for beside the float32 ulp (it matters only for entries near zero)
        own = 4 * np.finfo(np.float64).eps * (np.abs(zero.numpy()).max() + np.abs(want_w))
        assert (np.abs(got_w - want_w) <= ulp_w + own).all(), unit
        assert (np.abs(got_b - zero.numpy()) <= ulp_b).all(), unit


# ---------------------------------------------------------------- bytes
def test_byte_table_is_the_numpy_round_trip():
    t = video_fvd.byte_table()
    assert t.dtype == np.uint8 and t.shape == (256,)
    for u in range(256):
        npy = np.array([u], dtype=np.uint8).astype(np.float32)
        normed = -1 + 2 * npy / 255
        assert t[u] == ((normed + 1) * 255 / 2).astype(np.uint8)[0]
    diff = t.astype(np.int64) - np.arange(256)
    assert (diff != 0).sum() == 63 and set(diff.tolist()) == {0, -1}


# ---------------------------------------------------------------- the job
def _fake_embed(calls):
    proj = torch.from_numpy(np.random.default_rng(5).standard_normal((48, 400)))

    def embed(videos):
        assert videos.dtype == torch.uint8 and videos.ndim == 5 and videos.shape[2] == 3
        calls.append(tuple(videos.shape))
        v = videos.to(torch.float64)
        stats = torch.cat([v.mean(dim=(1, 3, 4)), v.std(dim=(1, 3, 4)), v[:, :14].mean(dim=(3, 4)).reshape(v.shape[0], -1)], dim=1)
        return stats @ proj
    return embed


def _job(tmp_path, n=5, T_file=14, T_gt=18, size=8, seed=0):
    g = np.random.default_rng(seed)
    (tmp_path / "samples").mkdir(parents=True, exist_ok=True)
    samples = g.integers(0, 256, (n, T_file, 3, size, size), dtype=np.uint8)
    for i in range(n):
        np.save(tmp_path / "samples" / f"sample_{i:04d}-0.npy", samples[i])
    gt = (g.random((n + 1, T_gt, 3, size, size)) * 2 - 1).astype(np.float32)
    np.save(tmp_path / "gt.npy", gt)
    args = argparse.Namespace(eval_dir=str(tmp_path), videos=str(tmp_path / "gt.npy"), synthetic=False, num_videos=n, sample_idx=0,
                              T=T_file, batch_size=None, i3d_weights=None)
    return args, samples, gt


def test_job_writes_the_distance_and_does_not_recompute(tmp_path, capsys):
    args, samples, gt = _job(tmp_path)
    calls = []
    embed = _fake_embed(calls)
    path = video_fvd.run(args, embed=embed)
    assert path == tmp_path / "fvd-5-0.txt" and path.exists()
    assert len(calls) == 10 and all(c == (1, 14, 3, 8, 8) for c in calls)
    table = video_fvd.byte_table()
    fs = np.concatenate([embed(torch.from_numpy(table[samples[i]][None])).numpy() for i in range(5)])
    gt_u8 = ((gt[:5, :14] + 1) * 255 / 2).astype(np.uint8)                    # --T cuts the ground truth's 18 frames to 14
    fg = np.concatenate([embed(torch.from_numpy(gt_u8[i][None])).numpy() for i in range(5)])
    want = fvd.frechet_distance(fs, fg)
    assert float(np.loadtxt(path)) == want and want > 0
    assert f"FVD: {want}" in capsys.readouterr().out
    del calls[:]
    assert video_fvd.run(args, embed=embed) == path
    assert calls == [] and "FVD already computed" in capsys.readouterr().out
    # --batch_size does not change the result
    args.batch_size, args.sample_idx = 3, 1
    for i in range(5):
        np.save(tmp_path / "samples" / f"sample_{i:04d}-1.npy", samples[i])
    assert float(np.loadtxt(video_fvd.run(args, embed=embed))) == want


def test_job_refusals_come_before_the_first_embed(tmp_path):
    calls = []
    embed = _fake_embed(calls)
    args, samples, _ = _job(tmp_path / "a")
    (tmp_path / "a" / "samples" / "sample_0003-0.npy").unlink()
    with pytest.raises(FileNotFoundError, match="sample_0003-0.npy"):
        video_fvd.run(args, embed=embed)
    args, samples, _ = _job(tmp_path / "b")
    np.save(tmp_path / "b" / "samples" / "sample_0002-0.npy", samples[2][:13])
    with pytest.raises(ValueError, match=r"sample_0002-0\.npy.*exactly T = 14"):
        video_fvd.run(args, embed=embed)
    args, samples, _ = _job(tmp_path / "c")
    np.save(tmp_path / "c" / "samples" / "sample_0004-0.npy", np.zeros((14, 3, 8, 6), dtype=np.uint8))
    with pytest.raises(ValueError, match=r"sample_0004-0\.npy.*ground truth"):
        video_fvd.run(args, embed=embed)
    args, samples, _ = _job(tmp_path / "d")
    args.num_videos = 7                                                          # the ground truth holds 6
    for i in (5, 6):
        np.save(tmp_path / "d" / "samples" / f"sample_{i:04d}-0.npy", samples[0])
    with pytest.raises(ValueError, match="ground truth has 6 videos.*7"):
        video_fvd.run(args, embed=embed)
    args, _, _ = _job(tmp_path / "e", T_file=8, T_gt=8)
    with pytest.raises(ValueError, match="at least 9 frames"):
        video_fvd.run(args, embed=embed)
    assert calls == []


def test_parser_refuses_without_weights(tmp_path, capsys):
    with pytest.raises(SystemExit):
        video_fvd.main(["--eval_dir", str(tmp_path), "--num_videos", "4"])
    err = capsys.readouterr().err
    assert "--i3d_weights" in err and "conv3d.weight" in err and "logits.conv3d" in err
    with pytest.raises(SystemExit):
        video_fvd.main(["--eval_dir", str(tmp_path), "--i3d_weights", "w.pt"])   # --num_videos is required
    assert "--num_videos" in capsys.readouterr().err
    args, _, _ = _job(tmp_path / "x")
    with pytest.raises(ValueError, match="--i3d_weights"):
        video_fvd.run(args)


# ---------------------------------------------------------------- shape arithmetic
@pytest.mark.parametrize("k,s", [(1, 1), (2, 2), (3, 1), (3, 2), (7, 2)])
def test_same_padding_against_the_helper(k, s):
    for size in range(5, 34):
        out, before, behind = fvd.same_pad(size, k, s)
        assert (out, before, behind) == ir.same_pads(size, k, s)
        assert out == -(-size // s) and behind - before in (0, 1) and (out - 1) * s + k <= size + before + behind
        x = torch.arange(size, dtype=torch.float64).view(1, 1, size, 1, 1) - 3.0
        y = ir.maxpool3d_same(x, (k, 1, 1), (s, 1, 1)).reshape(-1)
        assert y.shape[0] == out
        want = [max(float(x[0, 0, i, 0, 0]) for i in range(max(o * s - before, 0), min(o * s - before + k, size))) for o in range(out)]
        assert y.tolist() == want


def test_frame_limits():
    with pytest.raises(ValueError, match="at least 9 frames"):
        fvd.time_positions(8)
    assert [fvd.time_positions(T) for T in (9, 16, 17, 100, 300)] == [1, 1, 2, 12, 37]
