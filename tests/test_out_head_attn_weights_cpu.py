"""CPU: the float64 references of tests/test_gpu_out_head.py and tests/test_gpu_attn_weights.py (tests/out_head_restated.py,
tests/attn_weights_restated.py) against torch.nn.functional and against the oracle's own attention (oracle/unet_ref.py, taps["attn_w"]);
then the mistakes those GPU tests exist to catch, each applied to the restatement as a deliberately wrong variant: every one of them
must leave the bound the GPU test uses (R.head_bound / R.maps_bound with the measured floors) on inputs of the GPU tests' kind.
Last, without a GPU: the library loads and vd_out_head_variant names the path every case of the GPU list was listed for."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import attn_temporal_restated as RT
import attn_weights_restated as RW
import out_head_restated as RH
from oracle.unet_ref import UNetRef
from video_diffusion_amd import _lib


# ---------------------------------------------------------------------------------------------------- the head
@pytest.mark.parametrize("c", [(2, 5, 7, 8, 3), (1, 4, 4, 32, 6), (3, 16, 12, 24, 3)], ids=RH.label)
def test_head_restatement_is_conv2d_of_silu_of_the_affine(c):
    h, A, B, w, b = RH.make_inputs(c)
    x = h.double().permute(0, 3, 1, 2)
    want = F.conv2d(F.silu(x * A.double()[:, :, None, None] + B.double()[:, :, None, None]), w.double(), b.double(), padding=1)
    got = RH.head_ref(h, A, B, w, b)
    assert got.dtype == torch.float64 and got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    r32 = RH.head_ref(h, A, B, w, b, dtype=torch.float32)
    assert r32.dtype == torch.float32 and 0 < RH.scaled_error(r32, want) < 1e-5


def head_leaves_bound(c, wrong):
    x = RH.make_inputs(c)
    ref, ref32 = RH.head_ref(*x), RH.head_ref(*x, dtype=torch.float32)
    bound, _ = RH.head_bound(ref, ref32, RH.FLOOR)
    assert bool(((ref32.double() - ref).abs() <= bound).all())               # (the float32 run of the right lines stays inside)
    return not bool(((wrong(*x) - ref).abs() <= bound).all())


HEAD_SHAPES = [(2, 32, 32, 32, 3), (2, 20, 20, 64, 6)]


@pytest.mark.parametrize("c", HEAD_SHAPES, ids=RH.label)
def test_head_bound_catches_a_transposed_tap(c):
    assert head_leaves_bound(c, lambda h, A, B, w, b: RH.head_ref(h, A, B, w.transpose(-1, -2), b))


@pytest.mark.parametrize("c", HEAD_SHAPES, ids=RH.label)
def test_head_bound_catches_clamping_in_place_of_zero_padding(c):
    assert head_leaves_bound(c, lambda h, A, B, w, b: RH.head_ref(h, A, B, w, b, pad_mode="replicate"))


@pytest.mark.parametrize("c", HEAD_SHAPES, ids=RH.label)
def test_head_bound_catches_a_neighbouring_frames_affine(c):
    assert head_leaves_bound(c, lambda h, A, B, w, b: RH.head_ref(h, A.roll(1, 0), B.roll(1, 0), w, b))


# ---------------------------------------------------------------------------------------------------- the maps
def oracle_attention(B, D, C, L, heads, allow, rpe, mask):
    """The oracle's attention on random weights: (qkv [B][D][L][3C], Rk, Rq [B][L][L][C] or None, the map it logged)."""
    g = torch.Generator().manual_seed(5)
    ora = UNetRef.__new__(UNetRef)
    ora.cfg = {"use_rpe_net": False, "rp_alpha": 2, "rp_beta": 4, "rp_gamma": 8, "allow_interactions_between_padding": bool(allow)}
    ora.heads, ora.taps = heads, {"attn_w": []}
    ora.sd = {"a.norm.weight": torch.rand(C, generator=g) + 0.5, "a.norm.bias": torch.randn(C, generator=g) * 0.1,
              "a.qkv.weight": torch.randn(3 * C, C, generator=g) * 0.3, "a.qkv.bias": torch.randn(3 * C, generator=g) * 0.1,
              "a.proj_out.weight": torch.randn(C, C, generator=g) * 0.1, "a.proj_out.bias": torch.zeros(C)}
    for r in ("k", "q", "v"):
        ora.sd[f"a.rpe_{r}.lookup_table_weight"] = torch.randn(9, heads, C // heads, generator=g)
    x = torch.randn(B, D, C, L, generator=g)
    fidx = torch.stack([torch.arange(L), torch.arange(L) * 3 + 1])[:B]
    ora.attention(x, "a", None, fidx, mask, rpe)
    xn = F.group_norm(x.reshape(B * D, C, L), 32, ora.sd["a.norm.weight"], ora.sd["a.norm.bias"], eps=1e-5).view(B, D, C, L).permute(0, 1, 3, 2)
    qkv = F.linear(xn, ora.sd["a.qkv.weight"], ora.sd["a.qkv.bias"])
    Rk = Rq = None
    if rpe:
        dist = fidx.unsqueeze(-1) - fidx.unsqueeze(-2)
        Rk, Rq = (ora.rpe_R(f"a.rpe_{r}", dist, None, C).reshape(B, L, L, C) for r in ("k", "q"))
    return qkv, Rk, Rq, ora.taps["attn_w"][0]


@pytest.mark.parametrize("allow", [0, 1])
def test_temporal_maps_restatement_matches_the_oracles_map(allow):
    B, HW, C, T, heads = 2, 3, 64, 6, 4
    mask = torch.tensor([[1.0, 1, 0, 1, 0, 0], [0, 1, 1, 1, 1, 0]])
    qkv, Rk, Rq, want = oracle_attention(B, HW, C, T, heads, allow, True, mask)
    got = RW.temporal_maps(qkv.permute(0, 2, 1, 3), Rk, Rq, mask, allow, B, T, HW, C, heads)
    assert got.shape == want.shape == (B * HW, T, T)
    assert float((got - want.double()).abs().max()) < 2e-6                        # (the oracle's softmax is float32)


def test_spatial_maps_restatement_matches_the_oracles_map():
    N, L, C, heads = 3, 10, 32, 2
    qkv, _, _, want = oracle_attention(1, N, C, L, heads, 1, False, None)
    got = RW.spatial_maps(qkv[0], N, L, C, heads)
    assert got.shape == want.shape == (N, L, L)
    assert float((got - want.double()).abs().max()) < 2e-6


def test_maps_are_the_head_mean_of_functional_softmax():
    N, L, C, heads = 2, 9, 24, 3
    qkv = torch.randn(N, L, 3 * C, generator=torch.Generator().manual_seed(1)).double()
    q, k, _ = qkv.view(N, L, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    want = F.softmax(q @ k.transpose(-1, -2) / (C // heads) ** 0.5, dim=-1).mean(1)
    assert float((RW.spatial_maps(qkv, N, L, C, heads) - want).abs().max()) < 1e-14
    got = RW.temporal_maps(qkv.permute(1, 0, 2).reshape(1, L, N, 3 * C), None, None, None, 1, 1, L, N, C, heads)    # frames as pixels
    assert float((got - want).abs().max()) < 1e-14


TEMPORAL_SHAPES = [(2, 7, 5, 96, 4, True, "half", 0, False), (2, 33, 5, 24, 2, True, "allpad", 0, False)]


def temporal_leaves_bound(c, wrong):
    B, T, HW, C, heads, rpe, mask, allow, hot = c
    x = RW.temporal_inputs(c)
    ref, ref32 = RW.temporal_maps(*x, allow, B, T, HW, C, heads), RW.temporal_maps(*x, allow, B, T, HW, C, heads, dtype=torch.float32)
    bound, _, _ = RW.maps_bound(ref, ref32, RW.FLOOR_TEMPORAL)
    assert bool(((ref32.double() - ref).abs() <= bound).all())
    return not bool(((wrong(*x, allow, B, T, HW, C, heads) - ref).abs() <= bound).all())           # (a NaN is outside too)


@pytest.mark.parametrize("c", TEMPORAL_SHAPES, ids=RW.label)
def test_maps_bound_catches_a_dropped_diagonal_rule(c):
    def no_diagonal(m, allow, B, T):
        m = m.double()
        return (m.view(B, 1, T) * m.view(B, T, 1)) != 0
    assert temporal_leaves_bound(c, lambda *a: RW.temporal_maps(*a, pairs=no_diagonal))


@pytest.mark.parametrize("c", TEMPORAL_SHAPES, ids=RW.label)
def test_maps_bound_catches_rq_indexed_t_s(c):
    assert temporal_leaves_bound(c, lambda qkv, Rk, Rq, *a: RW.temporal_maps(qkv, Rk, Rq.transpose(1, 2), *a))


@pytest.mark.parametrize("c", TEMPORAL_SHAPES, ids=RW.label)
def test_maps_bound_catches_a_head_mean_over_one_head_fewer(c):
    def short_mean(qkv, Rk, Rq, m, allow, B, T, HW, C, heads):
        a, _ = RT.attn_weights(qkv, Rk, Rq, m, allow, B, T, HW, C, heads)
        return (a.sum(2) / (heads - 1)).abs().reshape(B * HW, T, T)
    assert temporal_leaves_bound(c, short_mean)


def test_spatial_maps_bound_catches_a_head_mean_over_one_head_fewer():
    c = (3, 17, 16, 4, False)
    N, L, C, heads, _ = c
    qkv = RW.spatial_inputs(c)
    ref, ref32 = RW.spatial_maps(qkv, N, L, C, heads), RW.spatial_maps(qkv, N, L, C, heads, dtype=torch.float32)
    bound, _, _ = RW.maps_bound(ref, ref32, RW.FLOOR_SPATIAL)
    assert bool(((ref32.double() - ref).abs() <= bound).all())
    assert not bool(((ref * heads / (heads - 1) - ref).abs() <= bound).all())


def test_floors_are_inside_the_projects_bars():
    """A measured floor is a fraction of max |ref|; max ref of a map is at most 1, so the maps' floors are compared as they stand."""
    assert 0 < RW.FLOOR_TEMPORAL <= RW.ATOL and 0 < RW.FLOOR_SPATIAL <= RW.ATOL and 0 < RH.FLOOR <= RH.RTOL


# ---------------------------------------------------------------------------------------------------- the library, no GPU
def variant(c):
    name = ctypes.create_string_buffer(256)
    rc = _lib.lib().vd_out_head_variant(*c, name, 256)
    return rc, name.value.decode()


def test_out_head_variant_names_every_path_of_the_gpu_case_list():
    assert set(RH.CASES) == {"head_gemm/tpw2", "head_gemm/tpw8", "igemm/32", "igemm/64"}
    for path, c in RH.ALL_CASES:
        assert variant(c) == (1, path), (c, path)


def test_out_head_variant_boundaries_and_refusals():
    assert variant((127, 64, 64, 32, 3)) == (1, "head_gemm/tpw2") and variant((128, 64, 64, 32, 3)) == (1, "head_gemm/tpw8")
    assert variant((1, 32, 32, 128, 6)) == (1, "igemm/64") and variant((1, 32, 32, 160, 3)) == (1, "igemm/32")
    for c, why in [((1, 20, 20, 40, 3), "Cin must be a multiple of 32"), ((1, 32, 32, 64, 4), "3 or 6 output channels"),
                   ((1, 0, 32, 64, 3), "positive nfr, H, W and C")]:
        rc, name = variant(c)
        assert rc == 0 and name.startswith("refused: ") and why in name, (c, name)
    assert _lib.lib().vd_out_head_variant(1, 32, 32, 128, 3, ctypes.create_string_buffer(4), 4) < 0          # no room for the name
