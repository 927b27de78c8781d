"""FreeU without a GPU: the closed form of the skip filter against the published FFT form, the identities, the adaptive map's range,
the checks that need no engine, and the licence of the GPU model tests' constants (tests/freeu_restated.py)."""
import argparse

import pytest
import torch

from freeu_restated import (B_CONST, EPS_ATOL, S_CONST, FreeUNetRef, backbone, filter_closed, filter_fft, oracle_eps, structure_map)


@pytest.mark.parametrize("S", [2, 3, 4, 5, 7, 8, 16, 32])
def test_closed_form_equals_the_fft_form(S):
    g = torch.Generator().manual_seed(100 + S)
    x = torch.randn(3, 5, S, S, generator=g, dtype=torch.float64)
    for s in (0.2, 0.9, 1.0, 1.7):
        want, got = filter_fft(x, s), filter_closed(x, s)
        rel = float((got - want).abs().max() / want.abs().max())
        print(f"S={S} s={s}: max |closed - fft| / max |fft| = {rel:.3e}")
        assert rel <= 1e-13, (S, s, rel)
    assert not torch.equal(filter_closed(x, 0.2), x)


def test_unit_constants_are_the_identity_to_the_bit():
    x = torch.randn(2, 8, 7, 7, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    assert torch.equal(filter_closed(x, 1.0), x)
    assert torch.equal(backbone(x, 1.0, False), x) and torch.equal(backbone(x, 1.0, True), x)


def test_the_adaptive_map_lies_in_the_unit_interval_and_a_constant_frame_gives_zero():
    h = torch.randn(3, 16, 5, 5, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    h[1] = h[1] - h[1].mean(0, keepdim=True) + 0.25              # frame 1: the channel mean is 0.25 at every pixel, up to rounding ...
    h[2] = 3.0                                                   # ... and frame 2's exactly
    g = structure_map(h)
    assert g.shape == (3, 1, 5, 5) and float(g.min()) >= 0.0 and float(g.max()) <= 1.0
    assert float(g[0].min()) == 0.0 and float(g[0].max()) == 1.0
    assert not g[2].any() and torch.equal(backbone(h, 1.7, True)[2], h[2])
    out = backbone(h, 1.7, True)
    assert torch.equal(out[:, 8:], h[:, 8:]) and not torch.equal(out[0, :8], h[0, :8])
    assert torch.equal(backbone(h, 1.7, False)[:, :8], h[:, :8] * 1.7)


def test_constants_are_checked_without_an_engine():
    from video_diffusion_amd.gaussian_diffusion import check_freeu
    assert check_freeu(1.4, 1.2, 0.6, 0.8) == (1.4, 1.2, 0.6, 0.8)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="finite and > 0"):
            check_freeu(1.4, bad, 0.6, 0.8)


def test_run_directory_suffix_and_options():
    from video_diffusion_amd.video_sample import _freeu_options, run_postfix
    ns = argparse.Namespace
    assert run_postfix(ns()) == "" and _freeu_options(ns()) == {}
    assert run_postfix(ns(freeu=[1.4, 1.2, 0.6, 0.8])) == "_freeu1.4-1.2-0.6-0.8"
    assert run_postfix(ns(sampler="ddim", cfg_scale=2.0, freeu=[1.5, 1.0, 0.5, 1.0], freeu_adaptive=True)) == "_ddim_cfg2_freeu1.5-1-0.5-1a"
    assert _freeu_options(ns(freeu=[1.4, 1.2, 0.6, 0.8], freeu_adaptive=True)) == dict(freeu=(1.4, 1.2, 0.6, 0.8), freeu_adaptive=True)
    with pytest.raises(ValueError, match="needs --freeu"):
        _freeu_options(ns(freeu=None, freeu_adaptive=True))
    with pytest.raises(ValueError, match="finite and > 0"):
        _freeu_options(ns(freeu=[1.4, 1.2, 0.0, 0.8]))


@pytest.mark.parametrize("name", ["tiny", "w64_rb2", "sweep"])
@pytest.mark.parametrize("adaptive", [False, True])
def test_the_gpu_tests_constants_move_eps_far_beyond_the_tolerance(name, adaptive):
    """An engine that ran no FreeU pass must not pass the GPU comparison: with the constants of freeu_restated.py the oracle's eps differs
    from the plain oracle's by at least 100 x the comparison tolerance at its maximum."""
    plain, fu = oracle_eps(name), oracle_eps(name, adaptive)
    d = float((fu - plain).abs().max())
    print(f"{name} adaptive={adaptive}: max |eps_freeu - eps| = {d:.3e} ({d / EPS_ATOL:.0f} x the tolerance), b = {B_CONST}, s = {S_CONST}")
    assert bool(torch.isfinite(fu).all()) and d >= 100 * EPS_ATOL, d


def test_the_oracle_with_unit_constants_is_the_plain_oracle():
    from freeu_restated import model_cfg, oracle, window
    x, t, kw = window("tiny")
    plain = oracle("tiny")
    net = FreeUNetRef(model_cfg("tiny"), plain.net.sd)
    tm = torch.tensor(plain.s.timestep_map, dtype=t.dtype)[t]
    assert torch.equal(net(x, tm, **kw), oracle_eps("tiny"))
