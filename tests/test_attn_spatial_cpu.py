"""CPU: tests/attn_spatial_restated.py (the fp64 reference of the spatial-attention GPU tests) against explicit Python loops over
(frame, head, query, key), written line by line from the reference's unet.py -- no matmul, no reshape, no permute here:

    q *= scale                                                            :487
    attn[i][j] = sum_f q[i][f] k[j][f]                                    :489
    a = softmax_j;  out[i][f] = sum_j a[i][j] v[j][f]                     :525-534

and the layout read straight off the flat buffer: element (n, i, third, h, f) of qkv is at ((n L + i) 3C + third C + h F + f).
"""
import math

import pytest
import torch

from attn_spatial_restated import attn_ref, row_scale, scaled_error, scaled_errors


def loops(qkv, N, L, C, heads):
    """(out [N][L][C], S [N][heads]) in double precision from the flat buffer."""
    Fd = C // heads
    scale = Fd ** -0.5
    x = qkv.double().reshape(-1).tolist()
    at = lambda n, i, third, h, f: x[(n * L + i) * 3 * C + third * C + h * Fd + f]
    out = [[[0.0] * C for _ in range(L)] for _ in range(N)]
    S = [[0.0] * heads for _ in range(N)]
    for n in range(N):
        for h in range(heads):
            for j in range(L):
                for f in range(Fd):
                    S[n][h] = max(S[n][h], abs(at(n, j, 2, h, f)))
            for i in range(L):
                w = []
                for j in range(L):
                    acc = 0.0
                    for f in range(Fd):
                        acc += at(n, i, 0, h, f) * scale * at(n, j, 1, h, f)
                    w.append(acc)
                mx = max(w)
                e = [math.exp(u - mx) for u in w]
                den = sum(e)
                for f in range(Fd):
                    o = 0.0
                    for j in range(L):
                        o += e[j] / den * at(n, j, 2, h, f)
                    out[n][i][h * Fd + f] = o
    return torch.tensor(out, dtype=torch.float64), torch.tensor(S, dtype=torch.float64)


def inputs(N, L, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, L, 3 * C, generator=g) * 1.5


@pytest.mark.parametrize("L", [1, 3, 33])
@pytest.mark.parametrize("Fd", [8, 24])
@pytest.mark.parametrize("heads", [1, 3])
def test_restatement_matches_explicit_loops(L, Fd, heads):
    N, C = 2, Fd * heads
    qkv = inputs(N, L, C, seed=100 * L + C)
    want, S_want = loops(qkv, N, L, C, heads)
    got = attn_ref(qkv, N, L, C, heads)
    assert got.dtype == torch.float64 and got.shape == want.shape == (N, L, C)
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())
    S = row_scale(qkv, N, L, C, heads)
    assert torch.equal(S, S_want)
    # the output is a convex combination of the vectors S bounds
    assert bool((got.abs().reshape(N, L, heads, Fd) <= S.view(N, 1, heads, 1) * (1 + 1e-12)).all())
    assert scaled_error(got, want, S) <= 1e-13
    if L == 1:                                                           # one key: the output is its v
        assert torch.equal(got, qkv[..., 2 * C:].double())


def test_heads_and_thirds_are_told_apart():
    """Were the restatement (or the loops) to read head h's k or v from another head or third, changing that one slice would not move
    exactly the outputs of (frame 1, head 2)."""
    N, L, Fd, heads = 2, 5, 8, 3
    C = Fd * heads
    qkv = inputs(N, L, C, seed=5)
    base = attn_ref(qkv, N, L, C, heads)
    for third in (0, 1, 2):
        x = qkv.clone()
        x[1, :, third * C + 2 * Fd:third * C + 3 * Fd] += 1.0 + torch.arange(L).view(L, 1)      # (a constant added to q or k alone could cancel in the softmax)
        got = attn_ref(x, N, L, C, heads)
        want, _ = loops(x, N, L, C, heads)
        assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())
        moved = (got != base).reshape(N, L, heads, Fd)
        assert bool(moved[1, :, 2].any()) and not bool(moved[0].any()) and not bool(moved[1, :, :2].any())


def test_scaled_errors_carry_a_nan_to_its_own_element_only():
    N, L, C, heads = 1, 2, 16, 2
    qkv = inputs(N, L, C, seed=1)
    ref = attn_ref(qkv, N, L, C, heads)
    got = ref.clone()
    got[0, 1, 9] = float("nan")
    e = scaled_errors(got, ref, row_scale(qkv, N, L, C, heads))
    assert e.shape == (N, L, heads, 8)
    assert int(torch.isnan(e).sum()) == 1 and bool(torch.isnan(e[0, 1, 1, 1]))
    assert math.isnan(scaled_error(got, ref, row_scale(qkv, N, L, C, heads)))


def test_float32_evaluation_is_the_same_restatement():
    N, L, C, heads = 2, 33, 48, 2
    qkv = inputs(N, L, C, seed=11)
    ref = attn_ref(qkv, N, L, C, heads)
    f32 = attn_ref(qkv, N, L, C, heads, dtype=torch.float32)
    assert f32.dtype == torch.float32
    e = scaled_error(f32, ref, row_scale(qkv, N, L, C, heads))
    assert 0 < e < 1e-5
