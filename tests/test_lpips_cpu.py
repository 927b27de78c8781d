"""CPU: the LPIPS weight loader (three file layouts, malformed files), the embedding length, and --lpips_weights of the CLIs.
The yardstick of the shapes is tests/lpips_restated.py (a plain-torch restatement of the reference's LpipsEmbedder; the pip
packages `lpips` / `torchvision` are not available to pin against)."""
import numpy as np
import pytest
import torch

from lpips_restated import dim_restated, synth_weights
from video_diffusion_amd import inference_util
from video_diffusion_amd import lpips as vlp

FEAT = (0, 3, 6, 8, 10)


def _lpips_sd(w, lins_style=False, scaling=True):
    sd = {}
    for k in range(5):
        sd[f"net.slice{k + 1}.{FEAT[k]}.weight"] = w[f"conv{k + 1}.weight"]
        sd[f"net.slice{k + 1}.{FEAT[k]}.bias"] = w[f"conv{k + 1}.bias"]
        key = f"lins.{k}.model.1.weight" if lins_style else f"lin{k}.model.1.weight"
        sd[key] = w[f"lin{k + 1}"].view(1, -1, 1, 1)
    if scaling:
        sd["scaling_layer.shift"] = torch.tensor([-.030, -.088, -.188])[None, :, None, None]
        sd["scaling_layer.scale"] = torch.tensor([.458, .448, .450])[None, :, None, None]
    return sd


def _tv_and_lin(w):
    tv = {}
    for k in range(5):
        tv[f"features.{FEAT[k]}.weight"] = w[f"conv{k + 1}.weight"]
        tv[f"features.{FEAT[k]}.bias"] = w[f"conv{k + 1}.bias"]
    tv["classifier.1.weight"] = torch.zeros(4, 4)                      # the rest of an AlexNet checkpoint is ignored
    lin = {f"lin{k}.model.1.weight": w[f"lin{k + 1}"].view(1, -1, 1, 1) for k in range(5)}
    return tv, lin


def test_loader_layouts_agree(tmp_path):
    """A full lpips.LPIPS(net='alex') dict (lin{k} and lins.{k} spellings, with and without scaling_layer), torchvision AlexNet +
    lpips v0.1 lin file as two paths ('a,b' or a list), and the two merged into one dict: the same canonical weights."""
    w = synth_weights(3)
    tv, lin = _tv_and_lin(w)
    files = {"full": _lpips_sd(w), "full_lins": _lpips_sd(w, lins_style=True), "noscale": _lpips_sd(w, scaling=False),
             "tv": tv, "lin": lin, "merged": {**tv, **lin}}
    paths = {}
    for name, sd in files.items():
        paths[name] = str(tmp_path / f"{name}.pth")
        torch.save(sd, paths[name])
    got = [vlp.read_weights(paths["full"]), vlp.read_weights(paths["full_lins"]), vlp.read_weights(paths["noscale"]),
           vlp.read_weights(f"{paths['tv']},{paths['lin']}"), vlp.read_weights([paths["tv"], paths["lin"]]),
           vlp.read_weights(paths["merged"])]
    want = {k: v.numpy().reshape(-1) if k.startswith("lin") else v.numpy() for k, v in w.items()}
    for g in got:
        assert sorted(g) == sorted(list(want) + ["shift", "scale"])
        for k, v in want.items():
            assert g[k].dtype == np.float32 and np.array_equal(g[k], v), k
        np.testing.assert_array_equal(g["shift"], np.float32([-.030, -.088, -.188]))
        np.testing.assert_array_equal(g["scale"], np.float32([.458, .448, .450]))


def test_loader_refuses_malformed(tmp_path):
    w = synth_weights(4)
    sd = _lpips_sd(w)
    bad = dict(sd)
    bad["net.slice2.3.weight"] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(ValueError, match=r"net\.slice2\.3\.weight has shape \(192, 64, 3, 3\), expected \(192, 64, 5, 5\)"):
        vlp.canonical_weights(bad)
    bad = {k: v for k, v in sd.items() if not k.startswith("lin3")}
    with pytest.raises(ValueError, match=r"missing keys.*lin3\.model\.1\.weight \| lins\.3\.model\.1\.weight"):
        vlp.canonical_weights(bad)
    bad = {k: v for k, v in sd.items() if "slice5" not in k}
    with pytest.raises(ValueError, match=r"net\.slice5\.10\.weight \| features\.10\.weight"):
        vlp.canonical_weights(bad)
    bad = dict(sd)
    lin = sd["lin1.model.1.weight"].clone()
    lin[0, 5] = -1e-3
    bad["lin1.model.1.weight"] = lin
    with pytest.raises(ValueError, match="negative entries"):
        vlp.canonical_weights(bad)
    bad = dict(sd)
    bad["lin0.model.1.weight"] = torch.zeros(1, 32, 1, 1)
    with pytest.raises(ValueError, match="lin0.model.1.weight has shape"):
        vlp.canonical_weights(bad)
    bad = dict(sd)
    bad["scaling_layer.scale"] = torch.zeros(1, 3, 1, 1)
    with pytest.raises(ValueError, match="zero entry"):
        vlp.canonical_weights(bad)
    p = tmp_path / "list.pth"
    torch.save([1, 2], str(p))
    with pytest.raises(ValueError, match="does not hold a state dict"):
        vlp.read_weights(str(p))


@pytest.mark.parametrize("H,W", [(32, 32), (48, 40), (64, 64), (128, 128)])
def test_embedding_dim(H, W):
    from video_diffusion_amd import _lib
    d = dim_restated(H, W)
    assert vlp.embedding_dim(H, W) == d
    assert _lib.lib().vd_lpips_dim(H, W) == d
    if (H, W) == (64, 64):
        assert d == 31872
    if (H, W) == (128, 128):
        assert d == 148608


@pytest.mark.parametrize("H,W", [(8, 64), (64, 12), (18, 18), (26, 40), (30, 64)])
def test_too_small_frames(H, W):
    """A layer would be empty: torch refuses the frame in the restatement, the loader's size function raises, the C ABI says -1."""
    from video_diffusion_amd import _lib
    with pytest.raises(RuntimeError):
        dim_restated(H, W)
    with pytest.raises(ValueError, match="too small"):
        vlp.embedding_dim(H, W)
    assert _lib.lib().vd_lpips_dim(H, W) == -1


def test_smallest_frames_accepted():
    """31 is the smallest side every layer takes (conv1 7 -> pool 3 -> pool 1; at 30 conv1 gives 6 and the second pool 0)."""
    from video_diffusion_amd import _lib
    assert vlp.embedding_dim(31, 31) == dim_restated(31, 31) == _lib.lib().vd_lpips_dim(31, 31)


def _capture(monkeypatch, module, argv):
    seen = {}

    def fake_run(args, **kw):
        seen["args"] = args
        return None
    monkeypatch.setattr(module, "run", fake_run)
    module.main(argv)
    return seen["args"]


@pytest.mark.parametrize("modname", ["video_sample", "video_sample_full", "video_nll"])
def test_cli_lpips_weights(monkeypatch, capsys, modname):
    import importlib
    mod = importlib.import_module(f"video_diffusion_amd.{modname}")
    monkeypatch.setattr(inference_util, "_lpips_embedder", None)
    args = _capture(monkeypatch, mod, ["--inference_mode", "adaptive-autoreg"])
    assert args.adaptive_distance == "l2" and args.lpips_weights is None                 # defaults unchanged
    args = _capture(monkeypatch, mod, ["--inference_mode", "adaptive-autoreg", "--adaptive_distance", "lpips",
                                       "--lpips_weights", "a.pth,b.pth"])
    assert args.adaptive_distance == "lpips" and args.lpips_weights == "a.pth,b.pth"
    with pytest.raises(SystemExit) as e:
        _capture(monkeypatch, mod, ["--inference_mode", "adaptive-autoreg", "--adaptive_distance", "lpips"])
    assert e.value.code == 2
    assert "--lpips_weights" in capsys.readouterr().err
    # a registered embedder (set_lpips_embedder) still serves without the option
    monkeypatch.setattr(inference_util, "_lpips_embedder", lambda x: x)
    args = _capture(monkeypatch, mod, ["--inference_mode", "adaptive-autoreg", "--adaptive_distance", "lpips"])
    assert args.lpips_weights is None


def test_lpips_without_weights_still_refused():
    """Nothing registered: distance='lpips' raises NotImplementedError as before (the loader is opt-in)."""
    inference_util.set_lpips_embedder(None)
    it = iter(inference_util.inference_strategies["adaptive-autoreg"](distance="lpips", video_length=8, num_obs=2,
                                                                         max_frames=4, step_size=2))
    it.set_videos(torch.zeros(1, 8, 3, 32, 32))
    with pytest.raises(NotImplementedError):
        next(it)
