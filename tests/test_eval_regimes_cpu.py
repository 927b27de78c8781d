"""CPU: the inputs of the evaluation kernels' launch-regime tests (tests/eval_regime_cases.py) do what the GPU tests say they do.

The GPU tests enter branches only large inputs select: SSIM / PSNR strips on frames 240 pixels or wider, the chunk loop of
`vd_lpips_embed`, pixels whose feature vector is all zero, farthest-point selection over more than 256 candidates.  Whether an
input reaches its branch is a question about the launchers' host code and about the inputs, so it is answered here: the plan
queries `vd_frame_metrics_plan` and `vd_lpips_embed_chunk` (host only; the launchers take their numbers from the same functions)
against the stated properties and a restatement, and the constructions against the fp64 restatement of the feature stack."""
import ctypes

import pytest
import torch

import eval_regime_cases as rc
from video_diffusion_amd import _lib
from video_diffusion_amd import lpips as vlp
from video_diffusion_amd import metrics as vmt


@pytest.mark.parametrize("H,W", rc.WIDE_CASES)
def test_wide_case_plan(H, W):
    plan = vmt.launch_plan(H, W)
    rc.check_wide_plan(H, W, *plan)


def test_wide_cases_cover_the_regimes():
    """Over the set: the boundary pair, a short last strip, a plane that is no multiple of 4 floats (plane_floats rounds up), a strip whose
    own rows are no multiple of 4 floats (the scalar staging path at an aligned base), and more than one pass of the column loop."""
    plans = {hw: vmt.launch_plan(*hw) for hw in rc.WIDE_CASES}
    assert plans[(40, 239)][0] == 32 and plans[(40, 240)][0] < 32
    short_last = [hw for hw, (rt, ns, _) in plans.items() if ns > 1 and hw[0] - (ns - 1) * (rt - 6) < rt]
    assert (70, 300) in short_last
    assert any((rt * hw[1]) % 4 for hw, (rt, _, _) in plans.items())
    assert any(((rt - 6) * hw[1]) % 4 for hw, (rt, _, _) in plans.items())
    assert any(hw[1] - 6 > 2 * rc.THREADS for hw in plans) and any(rc.THREADS < hw[1] - 6 < 2 * rc.THREADS for hw in plans)
    # the narrow shapes of tests/test_gpu_metrics.py are all on the other side: a full tile, one pass of the column loop
    for hw in [(7, 7), (9, 33), (64, 64), (100, 70), (128, 128), (200, 160)]:
        rt, _, _ = vmt.launch_plan(*hw)
        assert rt == 32 and hw[1] - 6 <= rc.THREADS


def test_plan_refusals_are_the_launchers():
    L = _lib.lib()
    r, s, g = ctypes.c_int(-5), ctypes.c_int(-5), ctypes.c_int(-5)

    def plan(H, W):
        return L.vd_frame_metrics_plan(H, W, ctypes.byref(r), ctypes.byref(s), ctypes.byref(g))
    with pytest.raises(_lib.VdError, match="H >= 7"):
        _lib.check(plan(6, 20))
    with pytest.raises(_lib.VdError, match="H >= 7"):
        _lib.check(plan(20, 6))
    with pytest.raises(_lib.VdError, match="1024"):
        _lib.check(plan(7, 1025))
    assert (r.value, s.value, g.value) == (-5, -5, -5)                     # a refusal writes nothing
    with pytest.raises(_lib.VdError, match="null"):
        _lib.check(L.vd_frame_metrics_plan(7, 7, None, ctypes.byref(s), ctypes.byref(g)))
    assert vmt.launch_plan(7, 7) == (32, 1, 1)
    assert vmt.launch_plan(7, 1024)[1] == 1


@pytest.mark.parametrize("S", [31, 64, 128, 512])
def test_lpips_embed_chunk(S):
    want = rc.lpips_chunk_restated(S, S)
    assert _lib.lib().vd_lpips_embed_chunk(S, S) == want == vlp.embed_chunk(S, S)
    assert 1 <= want <= 65535
    if S == 512:
        assert want + 2 < 32                                                 # the chunk test's N: a few hundred MB, not more


def test_lpips_embed_chunk_non_square_and_too_small():
    assert _lib.lib().vd_lpips_embed_chunk(48, 40) == rc.lpips_chunk_restated(48, 40)
    for H, W in [(8, 64), (64, 12), (18, 18), (26, 40), (30, 64)]:          # where vd_lpips_dim gives -1
        assert _lib.lib().vd_lpips_dim(H, W) == -1 and _lib.lib().vd_lpips_embed_chunk(H, W) == -1
        with pytest.raises(ValueError, match="too small"):
            vlp.embed_chunk(H, W)


def test_zero_norm_construction():
    """Frame 0 has non-zero vectors at every tap and all-zero ones at the taps its case names -- between the two cases, at every tap; frame
    1 has only zero vectors; everything is finite."""
    covered = set()
    for W, flat, zero_taps in rc.ZERO_NORM_CASES:
        masks, finite = rc.zero_vector_masks(rc.zero_norm_frames(W, flat), rc.zero_norm_weights())
        assert finite and len(masks) == 5
        for k, m in enumerate(masks):
            assert not bool(m[0].all()), f"tap {k + 1} at W = {W}: only zero vectors"
            assert bool(m[0].any()) == (k + 1 in zero_taps), f"tap {k + 1} at W = {W}: {int(m[0].sum())} of {m.shape[1]} zero vectors"
            assert bool(m[1].all()), f"tap {k + 1} at W = {W}"
        covered |= set(zero_taps)
    assert covered == {1, 2, 3, 4, 5}


@pytest.mark.parametrize("ncand", [257, 512, 600, 1000])
def test_int_embeddings_are_exact_in_float32(ncand):
    e = rc.int_embeddings(ncand, seed=ncand)
    assert e.shape == (2, ncand, rc.INT_D) and bool((e == e.round()).all()) and float(e.abs().max()) <= rc.INT_MAX
    assert torch.equal(e[0].sort(dim=0).values, e[1].sort(dim=0).values) and not torch.equal(e[0], e[1])
    d = torch.cdist(e, e) ** 2
    assert float(d.max()) < 2 ** 24
    assert rc.INT_D * (2 * rc.INT_MAX) ** 2 < 2 ** 24                        # the bound no draw can pass
