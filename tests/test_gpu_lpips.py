"""GPU: the LPIPS frame embedding (csrc/lpips.hip) and the device farthest-point selection, against the fp64 plain-torch
restatement of the reference's LpipsEmbedder / select_obs_indices (tests/lpips_restated.py; the pip packages `lpips` and
`torchvision` are not available, so the restatement is the yardstick), then the adaptive-* samplers and the sampling CLI with
distance='lpips' end to end.  Weights are synthetic (seeded, He-scaled convs, non-negative lin weights).

Error bound (fp32 operands and accumulation against fp64): every embedding element within 2e-5 * max|e| + 1e-5 * |e| of its tap, and every
pairwise squared distance within 1e-5 relative.  Measured on the MI355X: largest relative distance error 1.9e-7 (32x32),
8.8e-8 (64x64), 5.7e-8 (128x128), 1.6e-7 (48x40); largest absolute embedding error 6.9e-8.  The smallest relative margin of an
argmax pick in the samplers' test videos: 2.2e-3 (asserted > 100x the distance bound).

Launch regimes only large inputs select (inputs in tests/eval_regime_cases.py, kept honest on the CPU by tests/test_eval_regimes_cpu.py):
  * the chunk loop of vd_lpips_embed: 23 frames of 512 x 512 where `vd_lpips_embed_chunk` says 21 fit one pass; rows 0, 20, 21, 22 per element
    (measured: largest absolute embedding error 8.9e-9), every row equal to the bit to its frame embedded alone, no two rows equal, guard
    pads intact;
  * pixels whose feature vector is all zero (den = 0 + 1e-10): exactly 0, nothing non-finite; measured largest absolute embedding error
    on the non-zero rest 5.2e-8 (64 x 64) and 3.2e-8 (64 x 192);
  * farthest-point selection over 257, 600 and 1000 candidates (each thread of fps_pick_kernel sees up to four values before the tree),
    on integer embeddings whose distances are exact in float32: picks equal to the fp64 loop's, exact ties broken to the lowest index in
    the strided pre-pass (f + 256 duplicates f) and in the tree (f + 300 duplicates f), a NaN beyond index 256 reported."""
import os

import numpy as np
import pytest
import torch

import eval_regime_cases as rc
import video_diffusion_amd as vda
from helpers import Guarded, close, synth_sd
from lpips_restated import class_embedder, embed_parts_restated, embed_restated, select_restated, synth_weights
from video_diffusion_amd import _lib
from video_diffusion_amd import inference_util as iu
from video_diffusion_amd.lpips import LpipsAlex, embed_chunk, embedding_dim

pytestmark = pytest.mark.gpu
DIST_RTOL = 1e-5
_emb = {}


def embedder(seed=0):
    if seed not in _emb:
        _emb[seed] = (LpipsAlex.from_state_dict(_state_dict(synth_weights(seed)), "cuda:0"), synth_weights(seed))
    return _emb[seed]


def _state_dict(w):
    feat = (0, 3, 6, 8, 10)
    sd = {}
    for k in range(5):
        sd[f"net.slice{k + 1}.{feat[k]}.weight"] = w[f"conv{k + 1}.weight"]
        sd[f"net.slice{k + 1}.{feat[k]}.bias"] = w[f"conv{k + 1}.bias"]
        sd[f"lin{k}.model.1.weight"] = w[f"lin{k + 1}"].view(1, -1, 1, 1)
    return sd


def _frames(N, H, W, seed):
    """Frames in [-1, 1] with spatial structure (smooth ramps + noise): the ReLU maps are neither all-zero nor all-positive."""
    g = torch.Generator().manual_seed(seed)
    yy = torch.linspace(-1, 1, H).view(1, 1, H, 1)
    xx = torch.linspace(-1, 1, W).view(1, 1, 1, W)
    a = torch.rand(N, 3, 1, 1, generator=g) * 2 - 1
    b = torch.rand(N, 3, 1, 1, generator=g) * 2 - 1
    x = 0.5 * (a * yy + b * xx) + 0.5 * (torch.rand(N, 3, H, W, generator=g) * 2 - 1)
    return x.clamp(-1, 1)


def _pair_dist(e):
    e = e.to(torch.float64).reshape(e.shape[0], -1)
    return ((e[:, None, :] - e[None, :, :]) ** 2).sum(-1)


@pytest.mark.parametrize("H,W", [(32, 32), (64, 64), (128, 128), (48, 40), (31, 35)])
def test_embedding_vs_restated(H, W):
    """Every tap and the whole embedding against the fp64 restatement; pairwise distances within DIST_RTOL; run-to-run identical."""
    emb, w = embedder()
    N = 6
    x = _frames(N, H, W, seed=H * 1000 + W)
    got = emb(x)
    assert got.shape == (N, embedding_dim(H, W), 1, 1) and got.dtype == torch.float32 and got.device.type == "cuda"
    got = got.reshape(N, -1).cpu().to(torch.float64)
    parts = embed_parts_restated(x, w)
    off = 0
    for k, p in enumerate(parts):
        g = got[:, off:off + p.shape[1]]
        off += p.shape[1]
        err = (g - p).abs()
        bound = 2e-5 * p.abs().max() + 1e-5 * p.abs()
        assert bool((err <= bound).all()), f"tap {k + 1} at {H}x{W}: max err {err.max().item():.3e}, max|e| {p.abs().max().item():.3e}"
        assert p.abs().max() > 0
    assert off == got.shape[1]
    want = embed_restated(x, w).reshape(N, -1)
    dg, dw = _pair_dist(got), _pair_dist(want)
    off_diag = ~torch.eye(N, dtype=torch.bool)
    rel = ((dg - dw).abs() / dw)[off_diag].max().item()
    print(f"LPIPS {H}x{W}: max rel distance error {rel:.3e}, max abs embedding error {(got - want).abs().max().item():.3e}")
    assert rel <= DIST_RTOL, rel
    again = emb(x).reshape(N, -1).cpu().to(torch.float64)
    assert torch.equal(again, got)


def test_embed_batched_matches_call():
    """embed(videos, indices) on host videos = per-frame __call__ on the gathered frames, bit for bit, (B, n, D)."""
    emb, _ = embedder()
    v = _frames(2 * 7, 64, 64, seed=9).reshape(2, 7, 3, 64, 64)
    idx = [6, 2, 3, 0]
    e = emb.embed(v, idx)
    assert e.shape == (2, 4, 31872) and e.device.type == "cuda"
    ref = emb(v[:, idx].reshape(8, 3, 64, 64)).reshape(2, 4, -1)
    assert torch.equal(e, ref)


def _check_select(embs64, n, always):
    emb, _ = embedder()
    e32 = embs64.to(torch.float32)
    want = select_restated(e32.to(torch.float64), n, always)
    got = emb.select(e32.cuda(), n, always)
    assert got == want, (got, want)
    return got


def test_select_vs_host_loop():
    g = torch.Generator().manual_seed(21)
    # B > 1, different picks per item, a big D
    e = torch.randn(3, 40, 31872, generator=g, dtype=torch.float64)
    got = _check_select(e, 9, (0,))
    assert len({tuple(r) for r in got}) > 1
    # always_selected as hierarchy-2 builds them (the finished frames between the latents, two before, one after)
    e = torch.randn(2, 12, 256, generator=g, dtype=torch.float64)
    _check_select(e, 6, [5, 4, 11, 3])
    _check_select(e, 3, [5, 4, 11, 3])                                      # n < len(always_selected)
    # n greater than the number of candidates: repicks
    got = _check_select(e, 17, (2,))
    assert len(got[0]) == 17 and len(set(got[0])) < 17


def test_select_exact_ties_lowest_index():
    """Duplicated frames: exactly equal distances; the lowest candidate index wins (np.argmax), repicks stay."""
    g = torch.Generator().manual_seed(5)
    base = torch.randn(1, 4, 64, generator=g, dtype=torch.float64)
    e = torch.cat([base, base[:, [1, 2]], base[:, [1]]], dim=1)             # candidates 4, 5, 6 duplicate 1, 2, 1
    e = e.repeat(2, 1, 1)
    e[1] = e[1, [3, 2, 1, 0, 6, 5, 4]]
    got = _check_select(e, 10, (0,))
    assert all(len(row) == 10 and len(set(row)) < 10 for row in got)         # repicks once the distinct frames are used up
    assert all(5 not in row and 6 not in row for row in got[:1])            # item 0: duplicates of 1, 2 lose every tie to them
    # all-equal candidates: every pick after the first is the lowest index
    same = torch.ones(1, 5, 32, dtype=torch.float64)
    assert _check_select(same, 4, (3,)) == [[3, 0, 0, 0]]


def test_select_nan_raises():
    emb, _ = embedder()
    e = torch.randn(2, 6, 64, generator=torch.Generator().manual_seed(1))
    e[1, 4, 10] = float("nan")
    with pytest.raises(FloatingPointError):
        emb.select(e.cuda(), 3, (0,))
    # the error word is per call: a clean selection afterwards succeeds
    e[1, 4, 10] = 0.0
    assert emb.select(e.cuda(), 3, (0,)) == select_restated(e.to(torch.float64), 3, (0,))


def _tiny():
    from test_gpu_engine import _oracle
    cfg = {**vda.video_model_and_diffusion_defaults(), **dict(T=4, image_size=32, num_channels=32, num_res_blocks=1,
                                                              rp_alpha=4, rp_beta=4, rp_gamma=4, timestep_respacing="ddim5")}
    return cfg, _oracle(cfg)


def _gap(embs, n, always):
    """Smallest relative gap between the largest and the second-largest `nearest` over the argmax picks of select_restated."""
    worst = np.inf
    for b in range(embs.shape[0]):
        nearest = np.full(embs.shape[1], np.inf)
        newest = always[0]
        for i in range(1, n):
            d = ((embs[b] - embs[b, newest]) ** 2).reshape(embs.shape[1], -1).sum(1).numpy()
            nearest = np.minimum(nearest, d)
            if i < len(always):
                newest = always[i]
            else:
                s = np.sort(nearest)[::-1]
                worst = min(worst, (s[0] - s[1]) / s[0])
                newest = int(np.argmax(nearest))
    return worst


@pytest.mark.parametrize("mode,T,obs_len,max_frames,step", [("adaptive-autoreg", 8, 4, 5, 2),
                                                            ("adaptive-hierarchy-2", 10, 4, 6, 2)])
def test_infer_video_adaptive_lpips_vs_oracle(monkeypatch, mode, T, obs_len, max_frames, step):
    """infer_video(adaptive-*, distance='lpips') with the HIP embedder registered (batched embedding + device selection) against
    the oracle loop with the fp64 restated embedder on the host (select_obs_indices' own loop): identical picks, samples within the
    tolerances of test_infer_video_adaptive_autoreg_vs_oracle.  The picks' distance margins are asserted above the error bound."""
    from video_diffusion_amd import gaussian_diffusion as gdm
    from video_diffusion_amd.video_sample import get_masks, infer_video
    cfg, (model, diff, ora) = _tiny()
    emb, w = embedder()
    B = 2
    batch = torch.rand(B, T, 3, 32, 32, generator=torch.Generator().manual_seed(14)) * 2 - 1
    draws, gen = [], torch.Generator().manual_seed(15)

    def fake_randn_like(x, *a, **k):
        z = torch.randn(x.shape, generator=gen)
        draws.append(z)
        return z.to(x.device)

    picks_dev = []
    orig = iu.AdaptiveInferenceStrategyBase.select_obs_indices

    def recording(self, *a, **k):
        r = orig(self, *a, **k)
        picks_dev.append(r)
        return r
    monkeypatch.setattr(iu, "_lpips_embedder", emb)
    monkeypatch.setattr(gdm.th, "randn_like", fake_randn_like)
    monkeypatch.setattr(iu.AdaptiveInferenceStrategyBase, "select_obs_indices", recording)
    got, _ = infer_video(mode, model, diff, batch.cuda(), max_frames, obs_len, step, executor="eager", adaptive_distance="lpips")
    monkeypatch.undo()

    host = class_embedder(w)
    picks_host, gaps = [], []

    def recording_host(self, cand, n, always_selected=(0,)):
        embs = torch.stack([host(self.videos[:, i]) for i in cand], dim=1)
        gaps.append(_gap(embs, n, list(always_selected)))
        r = orig(self, cand, n, always_selected)
        picks_host.append(r)
        return r
    monkeypatch.setattr(iu, "_lpips_embedder", host)
    monkeypatch.setattr(iu.AdaptiveInferenceStrategyBase, "select_obs_indices", recording_host)
    samples = torch.zeros_like(batch)
    samples[:, :obs_len] = batch[:, :obs_len]
    sched = iter(iu.inference_strategies[mode](distance="lpips", video_length=T, num_obs=obs_len, max_frames=max_frames,
                                               step_size=step))
    it, windows = iter(draws), 0
    while True:
        sched.set_videos(samples)
        try:
            obs_idx, lat_idx = next(sched)
        except StopIteration:
            break
        fi = torch.cat([torch.tensor(obs_idx).reshape(B, -1), torch.tensor(lat_idx).reshape(B, -1)], dim=1)
        x0 = torch.stack([samples[i, f] for i, f in enumerate(fi)]).clone()
        om, lm, km = get_masks(x0, len(obs_idx[0]))
        kw = dict(x0=x0, obs_mask=om, latent_mask=lm, kinda_marg_mask=km, frame_indices=fi)
        local = x0.clone()
        for ts in range(diff.num_timesteps)[::-1]:
            local = ora.p_sample(local, torch.tensor([ts] * B), kw, next(it))["sample"]
        for i, li in enumerate(lat_idx):
            samples[i, li] = local[i, len(obs_idx[0]):]
        windows += 1
    monkeypatch.undo()
    assert windows >= 2 and len(draws) == windows * 5
    assert picks_dev == picks_host
    assert any(len(set(map(tuple, p))) > 1 for p in picks_host)             # the items' picks differ somewhere
    margin = min(gaps)
    print(f"{mode}: smallest relative margin of an argmax pick {margin:.3e}")
    assert margin > 100 * DIST_RTOL, margin
    err = np.abs(got - samples.numpy())
    assert err.mean() < 2e-4, err.mean()
    close(got, samples.numpy(), atol=3e-2, rtol=1e-2)
    assert np.array_equal(got[:, :obs_len], batch[:, :obs_len].numpy())


def test_sampling_cli_adaptive_lpips(tmp_path, monkeypatch):
    """`video_sample.main` from a checkpoint file and an LPIPS weights file (torchvision AlexNet + lpips lin file, two paths) to
    .npy with adaptive-autoreg and --adaptive_distance lpips: the files hold what infer_video with the same embedder and the same
    noise draws gives (test_infer_video_adaptive_lpips_vs_oracle's path)."""
    from video_diffusion_amd import gaussian_diffusion as gdm
    from video_diffusion_amd import video_sample as vs
    cfg, (model, diff, _) = _tiny()
    _, w = embedder()
    ck = tmp_path / "my-checkpoints" / "run" / "model_latest.pt"
    ck.parent.mkdir(parents=True)
    saved = {k: v for k, v in cfg.items() if k != "timestep_respacing"}
    saved.update(timestep_respacing="", max_frames=5)
    torch.save({"state_dict": synth_sd(model.param_specs()), "config": saved, "step": 7}, ck)
    feat = (0, 3, 6, 8, 10)
    tv = {f"features.{feat[k]}.{p}": w[f"conv{k + 1}.{p}"] for k in range(5) for p in ("weight", "bias")}
    lin = {f"lin{k}.model.1.weight": w[f"lin{k + 1}"].view(1, -1, 1, 1) for k in range(5)}
    torch.save(tv, tmp_path / "alexnet.pth")
    torch.save(lin, tmp_path / "alex.pth")
    vids = torch.rand(2, 8, 3, 32, 32, generator=torch.Generator().manual_seed(31)) * 2 - 1
    np.save(tmp_path / "videos.npy", vids.numpy())
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(iu, "_lpips_embedder", None)
    monkeypatch.setattr(vs, "_lpips_loaded", {})

    def seeded(seed):
        gen = torch.Generator().manual_seed(seed)

        def fake_randn_like(x, *a, **k):
            return torch.randn(x.shape, generator=gen).to(x.device)
        return fake_randn_like

    monkeypatch.setattr(gdm.th, "randn_like", seeded(41))
    out = vs.main([str(ck), "--videos", str(tmp_path / "videos.npy"), "--synthetic", "False", "--inference_mode", "adaptive-autoreg",
                   "--obs_length", "4", "--step_size", "2", "--batch_size", "2", "--timestep_respacing", "ddim5",
                   "--adaptive_distance", "lpips", "--lpips_weights", f"{tmp_path / 'alexnet.pth'},{tmp_path / 'alex.pth'}"])
    assert isinstance(iu._lpips_embedder, LpipsAlex)
    files = sorted(os.listdir(tmp_path / out / "samples"))
    assert files == ["sample_0000-0.npy", "sample_0001-0.npy"]
    # the same job through infer_video with the embedder the CLI loaded, the same draws
    monkeypatch.setattr(gdm.th, "randn_like", seeded(41))
    want, _ = vs.infer_video("adaptive-autoreg", model, diff, vids.cuda(), 5, 4, 2, executor="eager", adaptive_distance="lpips")
    want = vs.to_uint8(want)
    for i in range(2):
        got = np.load(tmp_path / out / "samples" / f"sample_{i:04d}-0.npy")
        assert np.array_equal(got, want[i])


# ---------------------------------------------------------------- launch regimes only large inputs select
def _check_taps(got, parts, what):
    """got (n, D) float64 against the restated per-tap pieces under the file's bound; the largest error."""
    off, worst = 0, 0.0
    for k, p in enumerate(parts):
        g = got[:, off:off + p.shape[1]]
        off += p.shape[1]
        err = (g - p).abs()
        bound = 2e-5 * p.abs().max() + 1e-5 * p.abs()
        assert bool((err <= bound).all()), f"{what}, tap {k + 1}: max err {err.max().item():.3e}, max|e| {p.abs().max().item():.3e}"
        assert p.abs().max() > 0
        worst = max(worst, err.max().item())
    assert off == got.shape[1]
    return worst


def test_embed_chunk_loop():
    """More frames than one pass takes (vd_lpips_embed_chunk(512, 512) + 2 = 23 frames of 512 x 512: a pass of 21 and a short one of 2),
    through the C entry into a guarded buffer.  Rows 0, chunk - 1, chunk and N - 1 per element and per tap against the restatement; every row
    equal to the bit to that frame embedded alone (its sums have a fixed order that no neighbour enters); no two rows equal, so a row
    written to another's place cannot pass; the pads untouched.  Measured on the MI355X: largest absolute embedding error 8.9e-9."""
    emb, w = embedder()
    H = W = 512
    chunk = embed_chunk(H, W)
    N = chunk + 2
    assert N > chunk > 1
    D = embedding_dim(H, W)
    x = _frames(N, H, W, seed=512)
    xd = x.cuda()
    g = Guarded(N, D)
    with torch.cuda.device(emb.device):
        _lib.check(_lib.lib().vd_lpips_embed(emb._h, N, H, W, _lib.ptr(xd), _lib.ptr(g.t), _lib.current_stream()))
    assert g.pads_intact(), "a pad was written"
    got = g.t
    assert bool(torch.isfinite(got).all()), "a row was not written (or is not finite)"
    for n in range(N):
        alone = emb(xd[n:n + 1]).reshape(-1)
        assert torch.equal(alone, got[n]), f"row {n} differs from frame {n} embedded alone"
        for m in range(n):
            assert not torch.equal(got[m], got[n]), f"rows {m} and {n} are equal"
    rows = [0, chunk - 1, chunk, N - 1]
    worst = _check_taps(got[rows].cpu().to(torch.float64), embed_parts_restated(x[rows], w), f"rows {rows} of {N}")
    print(f"LPIPS chunk loop {H}x{W}, N = {N}, chunk = {chunk}: max abs embedding error {worst:.3e}")


_zero_emb = {}


@pytest.mark.parametrize("W,flat,zero_taps", rc.ZERO_NORM_CASES)
def test_zero_norm_pixels(W, flat, zero_taps):
    """A pixel whose feature vector is all zero: den = sqrt(0) + 1e-10, the embedding there is exactly 0 and nothing is NaN.  Conv biases
    -|bias|, frame 0 the ScalingLayer's shift colour in its first columns and noise in the rest, frame 1 the shift colour everywhere (64 x 64
    with 40 flat columns: zero vectors at taps 1 and 2; 64 x 192 with 100: at every tap -- eval_regime_cases.ZERO_NORM_CASES)."""
    w = rc.zero_norm_weights()
    if not _zero_emb:
        _zero_emb[0] = LpipsAlex.from_state_dict(_state_dict(w), "cuda:0")
    emb = _zero_emb[0]
    x = rc.zero_norm_frames(W, flat)
    masks, finite = rc.zero_vector_masks(x, w)
    assert finite
    for k, m in enumerate(masks):
        assert bool(m[0].any()) == (k + 1 in zero_taps) and not bool(m[0].all()) and bool(m[1].all()), f"tap {k + 1}"
    got = emb(x).reshape(2, -1).cpu()
    assert got.shape[1] == embedding_dim(64, W) and bool(torch.isfinite(got).all())
    assert bool((got[1] == 0.0).all())
    parts = embed_parts_restated(x[:1], w)
    worst = _check_taps(got[:1].to(torch.float64), parts, f"zero-norm frame 0 at 64x{W}")
    off = 0
    for k, (p, m) in enumerate(zip(parts, masks)):                             # the zero vectors themselves: exactly 0, not merely small
        g = got[0, off:off + p.shape[1]].view(-1, m.shape[1])
        off += p.shape[1]
        assert bool((g[:, m[0]] == 0.0).all()), f"tap {k + 1}"
        assert bool((g[:, ~m[0]] != 0.0).any()), f"tap {k + 1}"
    print(f"LPIPS zero-norm 64x{W}: zero vectors per tap {[int(m[0].sum()) for m in masks]}, max abs embedding error {worst:.3e}")
    assert np.array_equal(emb.distance(x, x.clone()), np.zeros(2))


@pytest.mark.parametrize("ncand", [257, 600, 1000])
def test_select_many_candidates(ncand):
    """More than 256 candidates: every thread of fps_pick_kernel sees several values before the tree.  Integer embeddings make every
    squared distance exact in float32, so the picks equal the fp64 loop's with no margin to argue -- ties included (lowest index)."""
    e = rc.int_embeddings(ncand, seed=ncand)
    for always in ((0,), [5, 256, 3, ncand - 2]):
        got = _check_select(e, 12, always)
        assert got[0] != got[1] and all(len(set(row)) == 12 for row in got)
        if ncand >= 600:
            assert any(p >= 256 for row in got for p in row[len(always):])      # an argmax beyond a thread's first value


def test_select_many_candidates_ties():
    """Exactly equal maxima among more than 256 candidates: f + 256 duplicates f (the same thread meets both in its strided pre-pass),
    f + 300 duplicates f (another thread of another wave: the tree's tie-break), and 600 equal candidates."""
    for ndist in (256, 300):
        base = rc.int_embeddings(ndist, seed=ndist, B=1)
        assert len({tuple(r.tolist()) for r in base[0]}) == ndist
        got = _check_select(torch.cat([base, base], dim=1), 12, (0,))
        assert len(set(got[0])) == 12 and all(p < ndist for p in got[0]), got     # no duplicate's higher index is ever picked
    same = torch.ones(1, 600, 32, dtype=torch.float64)
    assert _check_select(same, 4, (3,)) == [[3, 0, 0, 0]]


def test_select_many_candidates_nan_raises():
    emb, _ = embedder()
    e = rc.int_embeddings(600, seed=3).to(torch.float32)
    want = select_restated(e.to(torch.float64), 3, (0,))
    e[1, 431, 10] = float("nan")
    with pytest.raises(FloatingPointError):
        emb.select(e.cuda(), 3, (0,))
    e[1, 431, 10] = 0.0
    assert emb.select(e.cuda(), 3, (0,)) == select_restated(e.to(torch.float64), 3, (0,))
    e = rc.int_embeddings(600, seed=3).to(torch.float32)
    assert emb.select(e.cuda(), 3, (0,)) == want
