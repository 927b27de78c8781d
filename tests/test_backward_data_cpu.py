"""CPU: the statements of tests/backward_data_restated.py against each other (the composed forms the engine runs = autograd of the plain
forward), the backward weight images of vd_pack_weight_bwd byte for byte against the forward packers over a torch-made rotated /
transposed weight, the zero padding of the stem image, and the case table of tests/backward_data_cases.py against the library's own
dispatch tables (host functions: no launch)."""
import numpy as np
import pytest
import torch

import backward_data_cases as C
import backward_data_restated as R
from video_diffusion_amd import _lib


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


# O != I, and O == I with weights that are neither symmetric in (o, i) nor under the rotation: a missing transposition or rotation shows
SHAPES = [(3, 5), (4, 4), (7, 2)]


@pytest.mark.parametrize("O,I", SHAPES)
def test_rotated_transposed_kernel_is_the_gradient_of_the_plain_conv(O, I):
    w, dy = rnd(O, I, 3, 3, seed=O), rnd(2, 6, 6, O, seed=I)
    want = R.conv_bwd(dy, w, 6)
    torch.testing.assert_close(R.conv_s1(dy, R.rotated(w)), want, rtol=1e-12, atol=1e-12)
    # each of the two halves alone is another operator
    for wrong in (w.transpose(0, 1).contiguous(), w.flip(2, 3) if O == I else None):
        if wrong is not None:
            assert float((R.conv_s1(dy, wrong) - want).abs().max()) > 1e-3


@pytest.mark.parametrize("O,I", SHAPES)
def test_downsample_backward_is_a_stride_1_conv_of_the_zero_stuffed_gradient(O, I):
    w, dy = rnd(O, I, 3, 3, seed=10 + O), rnd(2, 3, 3, O, seed=20 + I)
    torch.testing.assert_close(R.down_bwd_composed(dy, w), R.conv_bwd(dy, w, 6, stride=2), rtol=1e-12, atol=1e-12)
    z = R.zero_stuff2(dy)
    assert z.shape == (2, 6, 6, O) and torch.equal(z[:, ::2, ::2], dy) and int((z != 0).sum()) == int((dy != 0).sum())


@pytest.mark.parametrize("O,I", SHAPES)
def test_upsample_backward_is_the_conv_backward_then_2x2_sums(O, I):
    w, dy = rnd(O, I, 3, 3, seed=30 + O), rnd(2, 8, 8, O, seed=40 + I)
    torch.testing.assert_close(R.up_bwd_composed(dy, w), R.conv_bwd(dy, w, 4, ups=1), rtol=1e-12, atol=1e-12)
    x, y = rnd(1, 4, 6, 2, seed=1), rnd(1, 2, 3, 2, seed=2)
    want = x.reshape(1, 2, 2, 3, 2, 2).sum(dim=(2, 4)) + y
    torch.testing.assert_close(R.sumpool2(x, y), want, rtol=1e-14, atol=1e-14)


@pytest.mark.parametrize("O,I", SHAPES)
def test_linear_and_stem_backward_are_products_with_the_transposed_matrix(O, I):
    w, dy = rnd(O, I, seed=50 + O), rnd(9, O, seed=60 + I)
    torch.testing.assert_close(R.linear_bwd(dy, w), dy @ w, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(R.linear_bwd(dy, w), dy @ R.bwd_weight(w, "linear")[:, :, 0, 0].t(), rtol=1e-12, atol=1e-12)
    ws = rnd(O, I, 3, 3, seed=70)
    g = R.stem_bwd(dy, ws)
    assert g.shape == (9, R.STEM_KPAD) and not g[:, 9 * I:].any()
    for t in range(9):
        for i in range(I):
            torch.testing.assert_close(g[:, t * I + i], dy @ ws[:, i, t // 3, t % 3], rtol=1e-12, atol=1e-12)
    # the im2col product IS the conv: cols @ lin^T against F.conv2d
    x = rnd(1, I, 4, 4, seed=71)
    cols = torch.nn.functional.unfold(x, 3, padding=1).reshape(I, 9, 16).permute(2, 1, 0).reshape(16, 9 * I)       # k = tap * I + i
    y = torch.nn.functional.conv2d(x, ws, padding=1).reshape(O, 16).t()
    torch.testing.assert_close(cols @ R.stem_matrix(ws)[:, :9 * I].t(), y, rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------------------------------------------- the images
def _u16(n):
    return torch.zeros(n, dtype=torch.int16)


def _bytes(t):
    return t.contiguous().numpy().tobytes()


def packed(kind, w):
    return C.pack(kind, w)


@pytest.mark.parametrize("O,I", [(64, 128), (128, 128), (96, 64), (32, 192)])
def test_winograd_image_is_the_forward_packer_on_the_rotated_transposed_kernel(O, I):
    w = rnd(O, I, 3, 3, seed=O + I).float()
    L = _lib.lib()
    want = _u16(L.vd_split_image_u16(I, 16 * O))
    wb = w.flip(2, 3).transpose(0, 1).contiguous()
    _lib.check(L.vd_pack_conv3_wino_split(_lib.ptr(wb), _lib.ptr(want), I, O))
    got = packed("wino", w)
    assert got.numel() * 2 == want.numel() == L.vd_bwd_image_floats(C.KIND["wino"], O, I) * 2
    assert _bytes(got) == _bytes(want)
    if O == I:                                                      # neither half of the transformation alone gives these bytes
        for wrong in (w.flip(2, 3).contiguous(), w.transpose(0, 1).contiguous(), w):
            other = _u16(want.numel())
            _lib.check(L.vd_pack_conv3_wino_split(_lib.ptr(wrong), _lib.ptr(other), I, O))
            assert _bytes(other) != _bytes(want)


@pytest.mark.parametrize("O,I", [(64, 32), (128, 256), (5, 7), (64, 64)])
def test_generic_image_is_tap_cout_cin_of_the_rotated_transposed_kernel(O, I):
    w = rnd(O, I, 3, 3, seed=O * I).float()
    wb = w.flip(2, 3).transpose(0, 1)                               # [I][O][3][3]: Cout' = I, Cin' = O
    want = wb.permute(2, 3, 0, 1).reshape(-1).contiguous()         # [tap][Cout'][Cin'], as conv_gemm_cases.pack lays the forward's out
    got = packed("generic", w)
    assert got.numel() == want.numel() == _lib.lib().vd_bwd_image_floats(C.KIND["generic"], O, I) == 9 * O * I
    assert _bytes(got) == _bytes(want)
    if O == I:
        assert _bytes(got) != _bytes(w.permute(2, 3, 0, 1).reshape(-1).contiguous())
        assert _bytes(got) != _bytes(w.flip(2, 3).permute(2, 3, 0, 1).reshape(-1).contiguous())


@pytest.mark.parametrize("O,I", [(64, 32), (384, 128), (128, 128), (32, 96)])
def test_linear_image_is_the_forward_packer_on_the_transposed_matrix(O, I):
    w = rnd(O, I, seed=3 * O + I).float()
    L = _lib.lib()
    want = _u16(L.vd_split_image_u16(I, O))
    wt = w.t().contiguous()
    _lib.check(L.vd_pack_linear_split(_lib.ptr(wt), _lib.ptr(want), I, O))
    got = packed("linear", w)
    assert got.numel() * 2 == want.numel() == L.vd_bwd_image_floats(C.KIND["linear"], O, I) * 2
    assert _bytes(got) == _bytes(want)
    if O == I:
        other = _u16(want.numel())
        _lib.check(L.vd_pack_linear_split(_lib.ptr(w), _lib.ptr(other), I, O))
        assert _bytes(other) != _bytes(want)


def decode_linear_split(img_u16, n_out, K, mode):
    """The [n_out][K] matrix a vd_pack_linear_split image holds, float64, and the three raw pieces [3][n_out][K] (include/vd_amd.h:
    [k/16][n_out/32][piece 3][lane 64 = 32 h + r][8], then n_out scales and n_out reciprocals as floats)."""
    words = img_u16[:3 * n_out * K].numpy().view(np.uint16).reshape(K // 16, n_out // 32, 3, 2, 32, 8)       # [ks][cb][q][h][r][j]
    pieces = words.transpose(2, 1, 4, 0, 3, 5).reshape(3, n_out, K)                                          # [q][cb r][ks h j]
    scale = img_u16[3 * n_out * K:].numpy().view(np.float32)[:n_out].astype(np.float64)
    if mode == "bf16x6":
        val = (pieces.astype(np.uint32) << 16).view(np.float32).astype(np.float64).sum(0)
    else:
        val = pieces[:2].view(np.float16).astype(np.float64).sum(0)
    return val / scale[:, None], pieces


@pytest.mark.parametrize("O,I", [(64, 5), (32, 6), (128, 3)])
def test_stem_image_is_the_padded_im2col_matrix_and_its_padding_rows_decode_to_zero(O, I):
    w = rnd(O, I, 3, 3, seed=O + I).float()
    L, mode = _lib.lib(), C.process_mode()
    lt = R.stem_matrix(w).t().contiguous().float()                  # [STEM_KPAD][O]: row k = tap * I + i
    want = _u16(L.vd_split_image_u16(R.STEM_KPAD, O))
    _lib.check(L.vd_pack_linear_split(_lib.ptr(lt), _lib.ptr(want), R.STEM_KPAD, O))
    got = packed("stem", w)
    assert got.numel() * 2 == want.numel() == L.vd_bwd_image_floats(C.KIND["stem"], O, I) * 2
    assert _bytes(got) == _bytes(want)
    val, pieces = decode_linear_split(got.view(torch.int16), R.STEM_KPAD, O, "bf16x6" if mode == "fp32" else mode)
    np.testing.assert_allclose(val[:9 * I], lt[:9 * I].double().numpy(), rtol=2.0 ** -20, atol=0)             # the decoder reads the right rows
    assert not (pieces[:, 9 * I:] & 0x7fff).any() and not val[9 * I:].any()                                  # every piece +-0


def test_packer_refuses_what_it_cannot_lay_out():
    L = _lib.lib()
    out = torch.zeros(16)
    w = torch.zeros(64 * 64 * 9)
    assert L.vd_bwd_image_floats(4, 64, 64) == -1 and L.vd_bwd_image_floats(0, 0, 64) == -1
    assert L.vd_pack_weight_bwd(_lib.ptr(w), 2, 64, 32, _lib.ptr(out)) != 0          # Winograd: Cout' = I must be a multiple of 64
    assert L.vd_pack_weight_bwd(_lib.ptr(w), 1, 64, 8, _lib.ptr(out)) != 0           # 72 stem columns do not fit 64
    assert L.vd_pack_weight_bwd(_lib.ptr(w), 0, 48, 64, _lib.ptr(out)) != 0


# ---------------------------------------------------------------------------------------------------- the case table
def test_every_variant_the_backward_pass_resolves_to_has_a_case_and_every_case_names_its_own():
    """From the parameter lists of the configurations tests/test_gpu_backward.py runs (C.CONFIGS) at the frame counts of its windows:
    every backward call, its image kind and the instantiation the library's tables give it; the table must cover every name."""
    mode = C.process_mode()
    if mode == "fp32":
        pytest.skip("VD_MATH=fp32: the backward pass is refused")
    need = C.needed_variants()
    classes = {call[2] for calls in need.values() for call in calls}
    assert classes == {"conv1", "conv2", "skip", "down", "up", "qkv", "proj", "stem"}
    widths = {call[5] for calls in need.values() for call in calls}
    assert {96, 192, 384, 896} <= widths                            # concat widths of the decoders
    seen = {}
    for c in C.CASES:
        rc, name = C.variant_of(c.cls, c.N, c.H, c.O, c.I, c.res)
        assert rc == 1 and name == C.variant_name(c, mode), (C.label(c), name)
        seen.setdefault(name, []).append(c)
    assert not set(need) - set(seen), sorted(set(need) - set(seen))
    assert len({C.label(c) for c in C.CASES}) == len(C.CASES)
    # split-K with more than one slice and with exactly one; the generic kernel below 8 x 8; Cout' a multiple of 64 but not of 128
    slices = {C.L().vd_conv_wino_ksplit(c.N, c.H, c.O, c.I) for c in C.CASES if C.kind_of(c.cls, c.H, c.O, c.I, mode) == "wino"}
    assert 1 in slices and max(slices) > 1
    assert any(c.H < 8 and c.cls not in C.LINEAR and seen for c in C.CASES)
    assert any(C.kind_of(c.cls, c.H, c.O, c.I, mode) == "wino" and c.I % 128 == 64 for c in C.CASES)
    # every class, residual in place on the two classes the engine runs with one
    assert {c.cls for c in C.CASES} == classes and any(c.cls == "down" and c.res for c in C.CASES) and any(c.cls == "qkv" and c.res for c in C.CASES)
    for c in C.SMALL:
        assert c.N <= 3 and c.H in (2, 4, 8, 16, 32) and 32 <= c.O <= 512


def test_grad_rescale_statement():
    for m, s in ((1.0, 1.0), (1.999, 1.0), (2.0, 0.5), (3e-5, 2.0 ** 16), (0.0, 1.0), (3e38, 1.0), (2.0 ** -149, 2.0 ** 100), (float("inf"), 1.0)):
        assert R.grad_rescale(torch.tensor([0.0, -m, float("nan")]))[0] == s, m
    for m in (1e-8, 0.37, 5.0, 1e30):
        s, _ = R.grad_rescale(torch.tensor([m]))
        assert 1.0 <= m * s < 2.0


def test_clip_boundary_share_of_randn_inputs():
    """The elements the guided tests exclude (|x0r| within 1e-5 of 1): about 1e-5 of randn inputs, far under the 0.1 % the GPU test
    allows; and the float32 closed forms equal float64 autograd away from them."""
    import step_nll_restated as S
    from video_diffusion_amd.script_util import create_gaussian_diffusion
    diff = create_gaussian_diffusion(**dict(S.SCHEDULES)["linear_ddim250"])
    tab = S.tables(diff)
    tab["al"] = (1.0 - np.asarray(diff.betas, np.float64)).astype(np.float32)
    g = torch.Generator().manual_seed(0)
    B, per = 4, 200_000
    x, eps, z, xm = (torch.randn(B, per, generator=g) for _ in range(4))
    t = torch.tensor([0, 3, 120, tab["NT"] - 1])
    obs = torch.ones(B, per)
    r = R.guided_grad(tab, x, eps, z, xm, obs, t, 1)
    near = ((r["x0r"].abs() - 1).abs() < 1e-5)
    share = float(near.double().mean())
    print(f"clip boundary share {share:.2e}")
    assert share < 1e-4
    f = R.guided_grad_f32(tab, x, eps, z, xm, obs, t, 1)
    u = R.guided_grad_units(tab, x, eps, z, xm, obs, t)
    for k in ("deps", "dxd", "mean", "xstart"):
        e = ((f[k].double() - r[k]).abs() / u[k].clamp_min(1e-300))[~near]
        assert float(e.max()) < 2.0 ** -20, (k, float(e.max()))
