"""tests/conv_gemm_restated.py (the float64 references of tests/test_gpu_conv_gemm.py) against explicit Python loops on tiny shapes and
against F.conv2d in double; the Winograd statement equals the direct one to 1e-12 S.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

from conv_gemm_restated import conv_ref, gn_block_sums, linear_ref, operand, phase_kernels, silu, upsample2, wino_ref

F64 = torch.float64


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.rand(*shape, generator=g, dtype=F64) * 2 - 1


def loops_conv(a, w, bias, stride, ups, fbias, res):
    """out[n][y][x][o], element by element; the upsampled source is indexed as source[y >> 1][x >> 1]."""
    N, Hs, Ws, C = a.shape
    O, _, k, _ = w.shape
    pad = (k - 1) // 2
    H, W = Hs << ups, Ws << ups
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    out = torch.zeros(N, Ho, Wo, O, dtype=F64)
    for n in range(N):
        for y in range(Ho):
            for x in range(Wo):
                for o in range(O):
                    s = 0.0
                    for dy in range(k):
                        for dx in range(k):
                            iy, ix = y * stride + dy - pad, x * stride + dx - pad
                            if 0 <= iy < H and 0 <= ix < W:
                                for c in range(C):
                                    s += float(a[n, iy >> ups, ix >> ups, c]) * float(w[o, c, dy, dx])
                    s += float(bias[o]) if bias is not None else 0.0
                    s += float(fbias[n, o]) if fbias is not None else 0.0
                    s += float(res[n, y, x, o]) if res is not None else 0.0
                    out[n, y, x, o] = s
    return out


@pytest.mark.parametrize("k,stride,ups,H", [(3, 1, 0, 4), (3, 2, 0, 5), (3, 2, 0, 4), (3, 1, 1, 3), (1, 1, 0, 3)])
def test_conv_ref_against_loops_and_conv2d(k, stride, ups, H):
    N, C, O = 2, 3, 4
    a, w, b = rnd(N, H, H, C), rnd(O, C, k, k, seed=1), rnd(O, seed=2)
    Ho = ((H << ups) + 2 * (k // 2) - k) // stride + 1
    fb, res = rnd(N, O, seed=3), rnd(N, Ho, Ho, O, seed=4)
    got = conv_ref(a, w, b, stride=stride, ups=ups, fbias=fb, res=res)
    want = loops_conv(a, w, b, stride, ups, fb, res)
    assert got.shape == want.shape and (got - want).abs().max() < 1e-13
    x = a.permute(0, 3, 1, 2)
    if ups:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    t = F.conv2d(x, w, b, stride=stride, padding=k // 2).permute(0, 2, 3, 1) + fb[:, None, None, :] + res
    assert (got - t).abs().max() < 1e-13
    # the unit S: the same sum over absolute values
    S = conv_ref(a, w, b, stride=stride, ups=ups, fbias=fb, res=res, absolute=True)
    assert (S - loops_conv(a.abs(), w.abs(), b.abs(), stride, ups, fb.abs(), res.abs())).abs().max() < 1e-13
    assert (S >= got.abs() - 1e-13).all()


def test_operand_concat_affine_silu_and_linear():
    N, H, C0, C1 = 2, 3, 2, 3
    x0, x1, A, B = rnd(N, H, H, C0), rnd(N, H, H, C1, seed=1), rnd(N, C0 + C1, seed=2) + 1.5, rnd(N, C0 + C1, seed=3)
    a = operand(x0, x1, A, B, act=1)
    for n in range(N):
        for c in range(C0 + C1):
            src = x0[n, :, :, c] if c < C0 else x1[n, :, :, c - C0]
            v = src * A[n, c] + B[n, c]
            assert (a[n, :, :, c] - v * torch.sigmoid(v)).abs().max() < 1e-15
    assert torch.equal(operand(x0, None), x0) and (silu(x0) - F.silu(x0)).abs().max() < 1e-15
    assert torch.equal(upsample2(x0)[:, 3, 4], x0[:, 1, 2])
    m, w, b, r = rnd(5, 4), rnd(3, 4, seed=1), rnd(3, seed=2), rnd(5, 3, seed=3)
    want = torch.tensor([[sum(float(m[i, k]) * float(w[j, k]) for k in range(4)) + float(b[j]) + float(r[i, j]) for j in range(3)] for i in range(5)],
                        dtype=F64)
    assert (linear_ref(m, w, b, r) - want).abs().max() < 1e-14
    assert (linear_ref(m, w, b, r, absolute=True) - (m.abs() @ w.abs().t() + b.abs() + r.abs())).abs().max() < 1e-14


@pytest.mark.parametrize("N,H,C,O,ups", [(2, 8, 5, 3, 0), (1, 16, 3, 2, 0), (3, 4, 4, 4, 1)])
def test_wino_ref_is_the_direct_convolution(N, H, C, O, ups):
    a, w, b = rnd(N, H, H, C), rnd(O, C, 3, 3, seed=1), rnd(O, seed=2)
    fb, res = rnd(N, O, seed=3), rnd(N, H << ups, H << ups, O, seed=4)
    ref = conv_ref(a, w, b, ups=ups, fbias=fb, res=res)
    S = conv_ref(a, w, b, ups=ups, fbias=fb, res=res, absolute=True)
    assert ((wino_ref(a, w, b, ups=ups, fbias=fb, res=res) - ref).abs() <= 1e-12 * S).all()
    Sw = wino_ref(a, w, b, ups=ups, fbias=fb, res=res, absolute=True)
    assert (Sw >= ref.abs() - 1e-12).all()          # the Winograd unit bounds the result as well (|sum| <= sum of | |)
    # the float32 evaluation of the same algorithm: its own rounding only
    f32 = wino_ref(a, w, b, ups=ups, fbias=fb, res=res, dtype=torch.float32)
    assert f32.dtype == torch.float32 and ((f32.double() - ref).abs() <= 64 * 2.0 ** -24 * Sw).all()


@pytest.mark.parametrize("N,H,C,O", [(2, 4, 3, 2), (1, 8, 2, 3)])
def test_sub_pixel_form_is_upsample_then_conv(N, H, C, O):
    a, w, b = rnd(N, H, H, C), rnd(O, C, 3, 3, seed=1), rnd(O, seed=2)
    ref = conv_ref(a, w, b, ups=1)
    S = conv_ref(a, w, b, ups=1, absolute=True)
    assert ((wino_ref(a, w, b, subpixel=True) - ref).abs() <= 1e-12 * S).all()
    g = phase_kernels(w)
    # each phase as a direct convolution of the source map, by loops over the phases' output pixels
    for py in range(2):
        for px in range(2):
            d = conv_ref(a, g[py, px], b)
            assert ((d - ref[:, py::2, px::2]).abs() <= 1e-12 * S[:, py::2, px::2]).all()
    assert (g[0, 0][:, :, 2] == 0).all() and (g[0, 0][:, :, :, 2] == 0).all() and (g[1, 1][:, :, 0] == 0).all() and (g[1, 1][:, :, :, 0] == 0).all()


def test_gn_block_sums_geometries_against_loops():
    N, C = 2, 3
    o = rnd(N, 32, 32, C).float()
    t = gn_block_sums(o, "wino")                                       # 2 x 2 groups of 16 x 16
    assert t.shape == (N, 4, C, 2)
    for by in range(2):
        for bx in range(2):
            blk = o[:, 16 * by:16 * by + 16, 16 * bx:16 * bx + 16].double()
            assert (t[:, by * 2 + bx, :, 0] - blk.sum((1, 2))).abs().max() < 1e-10 and (t[:, by * 2 + bx, :, 1] - (blk * blk).sum((1, 2))).abs().max() < 1e-10
    o8 = rnd(N, 8, 8, C).float()
    t8 = gn_block_sums(o8, "wino")
    assert t8.shape == (N, 1, C, 2) and (t8[:, 0, :, 0] - o8.double().sum((1, 2))).abs().max() < 1e-12
    # sub-pixel form: output 64 x 64 of a 32 x 32 source: 2 x 2 source groups, four phases each
    ou = rnd(1, 64, 64, C, seed=5).float()
    tu = gn_block_sums(ou, "ups")
    assert tu.shape == (1, 16, C, 2)
    for by in range(2):
        for bx in range(2):
            for py in range(2):
                for px in range(2):
                    blk = ou[:, 32 * by + py:32 * by + 32:2, 32 * bx + px:32 * bx + 32:2].double()
                    e = (by * 2 + bx) * 4 + 2 * py + px
                    assert (tu[:, e, :, 0] - blk.sum((1, 2))).abs().max() < 1e-10 and (tu[:, e, :, 1] - (blk * blk).sum((1, 2))).abs().max() < 1e-10
    tu16 = gn_block_sums(ou[:, :16, :16], "ups")                       # source 8 x 8: one group
    assert tu16.shape == (1, 4, C, 2) and (tu16[:, 3, :, 0] - ou[:, 1:16:2, 1:16:2].double().sum((1, 2))).abs().max() < 1e-12
    # GEMM epilogue: blocks of 32 consecutive rows of a frame of 64
    orow = rnd(3, 64, 1, C, seed=6).float()
    tr = gn_block_sums(orow, "rows", rows=32)
    assert tr.shape == (3, 2, C, 2) and (tr[:, 1, :, 0] - orow[:, 32:, 0].double().sum(1)).abs().max() < 1e-12
    assert (tr[:, 0, :, 1] - (orow[:, :32, 0].double() ** 2).sum(1)).abs().max() < 1e-12


def test_case_table_names_every_instantiation_without_a_launch():
    """vd_igemm_variant() and vd_igemm_variant_list() are host functions: the table of tests/conv_gemm_cases.py against the library's own
    dispatch, in this process' arithmetic (conv_wino_z128.hip's grid-fill rule reads the CU count: 256 where no device answers)."""
    from conv_gemm_cases import CASES, L, cases_for, label, process_mode, variant_list, variant_name, variant_of
    mode = process_mode()
    names = variant_list()
    assert len(names) == len(set(names)) == {"f16x3": 36, "bf16x6": 34, "fp32": 14}[mode]
    seen = set()
    for c in cases_for(mode):
        rc, name = variant_of(c)
        assert rc == 1 and name == variant_name(c, mode), (label(c), name)
        seen.add(name.split("+")[0])
        if "+ksplit" in c.variant:
            assert L().vd_conv_wino_ksplit(c.N, c.H, c.Cin, c.Cout) == int(c.variant.rsplit("+ksplit", 1)[1]), label(c)
    assert seen == set(names)
    assert len({label(c) for c in CASES}) == len(CASES)
