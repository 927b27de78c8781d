"""CPU: the configuration sweep (tests/golden/unet_configs.npz, minted by tools/golden/configs.py from the imported
reference).  The oracle is pinned against the reference's eps at every configuration, which licenses it as the full-tensor
yardstick of tests/test_gpu_config_sweep.py; the engine's parameter list is pinned against the reference's state_dict; and the
mistakes the sweep exists for -- a wrong head split, a skip concat with its halves in the wrong order -- are shown to leave
the bar by a wide margin.  Models outside the kernels' envelope are refused at creation, by name (vd_create is host-only)."""
import pytest
import torch

import video_diffusion_amd as vda
from config_sweep_cases import REFUSED, SERVED, TAGS, case, oracle, oracle_eps, oracle_kw, outside, sampler
from oracle.unet_ref import UNetRef
from video_diffusion_amd import _lib

KEYS = vda.video_model_and_diffusion_defaults().keys()


@pytest.mark.parametrize("tag", TAGS)
def test_oracle_eps_matches_reference(tag):
    k = case(tag)
    s = k["stride"]
    got = oracle_eps(tag)
    assert got.shape == k["c"]["x"].shape
    bad, worst, ratio = outside(got[..., ::s, ::s], k["eps"])
    print(f"{tag}: oracle vs reference max |d eps| = {worst:.3e} = {ratio:.3f} of the bound, |eps| up to {float(k['eps'].abs().max()):.2f}")
    assert bad == 0, (bad, worst)


@pytest.mark.parametrize("tag", SERVED)
def test_engine_param_specs_equal_reference_state_dict(tag):
    k = case(tag)
    model, _ = vda.create_video_model_and_diffusion(**{key: k["cfg"][key] for key in KEYS})
    got = [(n, tuple(int(d) for d in shape)) for n, shape in model.param_specs()]
    assert got == k["specs"]                                            # names, shapes and order


def _fraction_outside(got, ref):
    bad, _, _ = outside(got, ref)
    return bad / ref.numel()


def test_sweep_sees_a_wrong_head_count():
    """w64_h1_s64's weights and inputs (the RPE nets' shapes do not depend on the head count) evaluated with 1, 2 and 8 heads
    against 4 heads."""
    k = case("w64_h1_s64")
    sd = oracle("w64_h1_s64").net.sd
    eps = {}
    for heads in (1, 2, 4, 8):
        cfg = dict(k["cfg"], num_heads=heads)
        eps[heads] = sampler(cfg, UNetRef(cfg, sd)).eps(k["c"]["x"], k["t"], oracle_kw(k["c"]))
    assert torch.equal(eps[1], oracle_eps("w64_h1_s64"))
    for heads in (1, 2, 8):
        frac = _fraction_outside(eps[heads], eps[4])
        print(f"{heads} heads against 4: {100 * frac:.1f} % outside, max |d| = {float((eps[heads] - eps[4]).abs().max()):.3f}")
        assert frac > 0.5, (heads, frac)


class _SwappedSkip(UNetRef):
    """The oracle with the two halves of ONE decoder concat (`swap`: an output block whose h and skip are equally wide) in
    the wrong order."""
    swap = None

    def run_block(self, blk, pre, h, emb, fidx, mask, T):
        if pre == self.swap:
            half = h.shape[1] // 2
            assert blk[0][0] == "res" and blk[0][1] == 2 * half
            h = torch.cat([h[:, half:], h[:, :half]], dim=1)
        return super().run_block(blk, pre, h, emb, fidx, mask, T)


def test_sweep_sees_a_swapped_skip_concat():
    k = case("w96_s64")
    net = _SwappedSkip(k["cfg"], oracle("w96_s64").net.sd)
    assert net.topo["output"][0][0] == ("res", 768, 384)               # 384 from below + 384 skipped: a swap keeps the width
    net.swap = "output_blocks.0"
    got = sampler(k["cfg"], net).eps(k["c"]["x"], k["t"], oracle_kw(k["c"]))
    want = oracle_eps("w96_s64")
    frac = _fraction_outside(got, want)
    print(f"output_blocks.0 concat swapped: {100 * frac:.1f} % outside, max |d| = {float((got - want).abs().max()):.3f}")
    assert frac > 0.5, frac
    s = k["stride"]
    assert _fraction_outside(got[..., ::s, ::s], k["eps"]) > 0.5       # the strided fixture sees it as well


# ---------------------------------------------------------------------------------------------------- the envelope
def _create(**over):
    cfg = {**vda.video_model_and_diffusion_defaults(), **dict(T=4, image_size=32, num_channels=32, num_res_blocks=1, rp_alpha=4,
                                                              rp_beta=4, rp_gamma=4, timestep_respacing="ddim250"), **over}
    return vda.create_video_model_and_diffusion(**{key: cfg[key] for key in KEYS})


@pytest.mark.parametrize("over,words", [
    # 160 * (1, 2, 3, 4): output_blocks.0 normalises 640 + 640 channels; its 480-wide attention layers have head dim 120 as well
    (dict(image_size=64, num_channels=160), ["num_channels=160", "output_blocks.0.0.in_layers.0", "1280 channels (640 + 640", "at most 1024",
                                             "num_heads=4", "head dim 120"]),
    (dict(image_size=64, num_channels=160, num_heads=5), ["num_channels=160", "1280 channels", "at most 1024"]),
    (dict(image_size=64, num_channels=128, num_heads=1), ["num_heads=1", "input_blocks.5.1", "384 channels", "head dim 384", "128"]),
    # heads 8 on 96 channels: head dim 12 where the first level attends, 36 at 64 x 64 (288 channels); at 32 x 32 with the default
    # attention_resolutions every attention layer is 192 wide (head dim 24) and the model is served
    (dict(num_channels=96, num_heads=8, attention_resolutions="32,16,8"), ["num_heads=8", "input_blocks.1.1", "head dim 12", "multiple of 8",
                                                                          "attention_resolutions 32"]),
    (dict(image_size=64, num_channels=96, num_heads=8), ["num_heads=8", "288 channels", "head dim 36", "multiple of 8"]),
    (dict(num_channels=32, num_heads=3), ["num_heads=3", "input_blocks.3.1", "64 channels do not divide into 3 heads"]),
    (dict(image_size=64, num_channels=288, num_heads=4, attention_resolutions="8"), ["num_channels=288", "1152 channels", "at most 1024"]),
])
def test_models_outside_the_envelope_are_refused_at_creation_by_name(over, words):
    with pytest.raises(_lib.VdError) as e:
        _create(**over)
    print(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


@pytest.mark.parametrize("tag", sorted(REFUSED))
def test_sweep_configurations_the_kernels_do_not_serve_are_refused_by_name(tag):
    """Head dims 192 / 256 and 144 / 192: above the spatial attention's 128 (csrc/attn_spatial.hip).  The oracle is still pinned on
    them (test_oracle_eps_matches_reference); the engine says so at creation."""
    k = case(tag)
    with pytest.raises(_lib.VdError) as e:
        vda.create_video_model_and_diffusion(**{key: k["cfg"][key] for key in KEYS})
    print(e.value)
    for w in REFUSED[tag]:
        assert w in str(e.value), (w, str(e.value))


def test_the_envelope_limits_are_the_launchers_own():
    """The limit in the message is the constant the GroupNorm launchers test, and models at the limits exactly are created:
    512 + 512 = 1024 GroupNorm channels (w256_h8_s32), head dim 128 (512 channels on 4 heads), 4096 tokens per frame."""
    assert _lib.lib().vd_gn_max_channels() == 1024
    _create(num_channels=256, num_heads=8)
    _create(image_size=64, num_channels=128, num_heads=4)
    _create(image_size=64, num_channels=64, attention_resolutions="64,16")
    assert len(SERVED) + len(REFUSED) == len(TAGS) == 11
