"""CPU: tests/attn_temporal_restated.py (the fp64 reference of the temporal-attention GPU tests) against explicit Python loops over
(t, s), written line by line from the reference's unet.py -- no einsum and no transpose here, since the transposed rpe_q term
(unet.py:506-509) is the classic trap of this operator:

    q *= scale                                                            :487
    attn[t][s]  = sum_f q[t][f] k[s][f]                                   :489
    attn[t][s] += sum_f q[t][f] Rk[t][s][f]                               :502 with 'bdhtf,btshf->bdhts' (:362-366)
    pre[s][t]   = sum_f (k[s][f] * scale) Rq[s][t][f];  attn[t][s] += pre[s][t]      :506-509 (.transpose(-1, -2))
    allowed[t][s] = m[t] m[s] (+ (1 - m[t]) (1 - m[s]) | allowed[t][t] = 1);  attn[t][s] -= inf where allowed is 0      :511-524
    a = softmax_s;  out[t][f] = sum_s a[t][s] v[s][f] + sum_s a[t][s] Rv[t][s][f]    :525-534 with 'bdhts,btshf->bdhtf' (:374-378)
"""
import math

import pytest
import torch

from attn_temporal_restated import allowed_pairs, attn_ref, row_scale, scaled_error


def loops(qkv, Rk, Rq, Rv, m, allow, B, T, HW, C, heads):
    """(out [B][T][HW][C], S [B][T][HW][heads]) as nested lists of Python floats (double precision)."""
    Fd = C // heads
    scale = Fd ** -0.5
    x = qkv.double().tolist()
    rk, rq, rv = (None if r is None else r.double().tolist() for r in (Rk, Rq, Rv))
    mm = None if m is None else m.double().tolist()
    out = [[[[0.0] * C for _ in range(HW)] for _ in range(T)] for _ in range(B)]
    S = [[[[0.0] * heads for _ in range(HW)] for _ in range(T)] for _ in range(B)]
    for b in range(B):
        for p in range(HW):
            for h in range(heads):
                q = [[x[b][t][p][h * Fd + f] * scale for f in range(Fd)] for t in range(T)]
                k = [[x[b][t][p][C + h * Fd + f] for f in range(Fd)] for t in range(T)]
                v = [[x[b][t][p][2 * C + h * Fd + f] for f in range(Fd)] for t in range(T)]
                for t in range(T):
                    w, ok = [], []
                    for s in range(T):
                        acc = 0.0
                        for f in range(Fd):
                            acc += q[t][f] * k[s][f]
                            if rk is not None:
                                acc += q[t][f] * rk[b][t][s][h * Fd + f]
                                acc += (k[s][f] * scale) * rq[b][s][t][h * Fd + f]
                        allowed = 1.0
                        if mm is not None:
                            allowed = mm[b][t] * mm[b][s]
                            if allow:
                                allowed += (1 - mm[b][t]) * (1 - mm[b][s])
                            elif t == s:
                                allowed = 1.0
                        ok.append(allowed != 0)
                        w.append(acc if allowed != 0 else -math.inf)
                    mx = max(w)
                    e = [math.exp(u - mx) for u in w]
                    den = sum(e)
                    for f in range(Fd):
                        o = 0.0
                        for s in range(T):
                            vec = v[s][f] + (rv[b][t][s][h * Fd + f] if rv is not None else 0.0)
                            o += e[s] / den * vec
                            if ok[s]:
                                S[b][t][p][h] = max(S[b][t][p][h], abs(vec))
                        out[b][t][p][h * Fd + f] = o
    return torch.tensor(out, dtype=torch.float64), torch.tensor(S, dtype=torch.float64)


def inputs(B, T, HW, C, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, T, HW, 3 * C, generator=g) * 1.5
    Rk, Rq, Rv = (torch.randn(B, T, T, C, generator=g) for _ in range(3))
    return qkv, Rk, Rq, Rv


# (B, T, HW, C, heads, rpe, mask rows or None, allow)
CASES = [
    (1, 3, 2, 16, 2, True, None, 0),
    (2, 4, 1, 8, 1, True, [[1, 1, 0, 1], [0, 1, 1, 0]], 0),
    (2, 5, 3, 16, 2, True, [[1, 0, 1, 1, 0], [1, 1, 1, 1, 0]], 1),
    (2, 4, 2, 16, 2, False, [[0, 1, 1, 0], [1, 1, 1, 1]], 1),
    (1, 4, 2, 8, 1, False, [[1, 0, 0, 1]], 0),
]


@pytest.mark.parametrize("B,T,HW,C,heads,rpe,mask,allow", CASES)
def test_restatement_matches_explicit_loops(B, T, HW, C, heads, rpe, mask, allow):
    qkv, Rk, Rq, Rv = inputs(B, T, HW, C, seed=7 * T + C)
    if not rpe:
        Rk = Rq = Rv = None
    m = None if mask is None else torch.tensor(mask, dtype=torch.float32)
    want, S_want = loops(qkv, Rk, Rq, Rv, m, allow, B, T, HW, C, heads)
    got = attn_ref(qkv, Rk, Rq, Rv, m, allow, B, T, HW, C, heads)
    assert got.dtype == torch.float64 and got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())
    S = row_scale(qkv, Rv, m, allow, B, T, HW, C, heads)
    assert torch.equal(S, S_want)
    # the output is a convex combination of the vectors S bounds
    assert bool((got.abs().reshape(B, T, HW, heads, -1) <= S.unsqueeze(-1) * (1 + 1e-12)).all())
    assert scaled_error(got, want, S) <= 1e-13


def test_asymmetric_relative_positions_tell_a_transposed_rq_apart():
    """Rq[s,t] != Rq[t,s] in these inputs, and a large one-sided entry makes the difference gross: were the restatement (or the
    loops) to read Rq[t,s], this test and the one above could not both pass."""
    B, T, HW, C, heads = 1, 4, 2, 8, 1
    qkv, Rk, Rq, Rv = inputs(B, T, HW, C, seed=3)
    Rq0 = Rq.clone()
    Rq[0, 1, 3] += 5.0                                                   # (s = 1, t = 3) only
    want, _ = loops(qkv, Rk, Rq, Rv, None, 0, B, T, HW, C, heads)
    got = attn_ref(qkv, Rk, Rq, Rv, None, 0, B, T, HW, C, heads)
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())
    swapped = attn_ref(qkv, Rk, Rq.transpose(1, 2).contiguous(), Rv, None, 0, B, T, HW, C, heads)
    assert float((swapped - want).abs().max()) > 1e-2 * float(want.abs().max())
    # the entry moves row t = 3 and leaves rows 0..2 alone
    base = attn_ref(qkv, Rk, Rq0, Rv, None, 0, B, T, HW, C, heads)
    assert torch.equal(base[:, :3], got[:, :3]) and not torch.equal(base[:, 3], got[:, 3])


def test_mask_rule_both_allow_values():
    m = torch.tensor([[1.0, 0.0, 1.0, 0.0]])
    no = allowed_pairs(m, 0, 1, 4)[0].tolist()
    yes = allowed_pairs(m, 1, 1, 4)[0].tolist()
    assert no == [[True, False, True, False], [False, True, False, False], [True, False, True, False], [False, False, False, True]]
    assert yes == [[True, False, True, False], [False, True, False, True], [True, False, True, False], [False, True, False, True]]
    assert bool(allowed_pairs(None, 0, 2, 3).all())


def test_float32_evaluation_is_the_same_restatement():
    B, T, HW, C, heads = 2, 5, 3, 16, 2
    qkv, Rk, Rq, Rv = inputs(B, T, HW, C, seed=11)
    m = torch.tensor([[1, 0, 1, 1, 0], [1, 1, 1, 1, 0]], dtype=torch.float32)
    ref = attn_ref(qkv, Rk, Rq, Rv, m, 0, B, T, HW, C, heads)
    f32 = attn_ref(qkv, Rk, Rq, Rv, m, 0, B, T, HW, C, heads, dtype=torch.float32)
    assert f32.dtype == torch.float32
    e = scaled_error(f32, ref, row_scale(qkv, Rv, m, 0, B, T, HW, C, heads))
    assert 0 < e < 1e-5
