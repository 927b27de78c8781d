"""GPU: the spatial GroupNorm kernels of csrc/norm.hip one at a time -- gn_stats_partial (vd_op_gn_stats), gn_final_affine_kernel with
its mean / rstd output (vd_op_gn_affine_mr), affine_act_fold_kernel (vd_op_gn_act_fold) and affine_act_kernel (vd_op_affine_act) --
per element against the exact-sum reference of tests/gn_spatial_restated.py, under the bounds derived there by counting roundings
(nothing in them is measured; tests/test_gn_spatial_cpu.py holds a line-by-line emulation of the kernels to the same bounds).
Every output lies between sentinel pads and is prefilled with NaN; the case lists and what each case reaches are in the restated
module.  Each case prints `GN_SPATIAL_CASE | kernel | case | max err/bound ..` and asserts <= 1 per element."""
import functools

import numpy as np
import pytest
import torch

import gn_spatial_restated as R
from video_diffusion_amd import _lib

pytestmark = pytest.mark.gpu
PAD = 4096
PIPE_IDS = [R.label(c) for c in R.PIPE_CASES]
STATS_IDS = [R.label(c) for c in R.STATS_CASES]


def dev(t):
    if t is None:
        return None
    return (torch.from_numpy(t) if isinstance(t, np.ndarray) else t).to("cuda").contiguous()


class Guarded:
    """n elements prefilled with NaN between two pads of sentinels."""
    def __init__(self, *shape, dtype=torch.float32):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * PAD,), R.SENTINEL, dtype=dtype, device="cuda")
        self.t = self.buf[PAD:PAD + n].view(*shape)
        self.t.fill_(float("nan"))
        self.n = n

    def read(self):
        """The contents as numpy, after checking that the pads are intact and every element was written with a finite value."""
        torch.cuda.synchronize()
        assert bool((self.buf[:PAD] == R.SENTINEL).all()) and bool((self.buf[PAD + self.n:] == R.SENTINEL).all()), "a pad was written"
        assert bool(torch.isfinite(self.t).all()), "an element was not written (or is not finite)"
        return self.t.cpu().numpy()

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf[:PAD] == R.SENTINEL).all()) and bool((self.buf[PAD + self.n:] == R.SENTINEL).all()) \
            and bool(torch.isnan(self.t).all())


def run_stats(x0, x1, split):
    """vd_op_gn_stats over the virtual concat of x0 [N][HW][C0] and x1 (or None) -> [N][split][C][2] doubles."""
    N, HW, C0 = x0.shape
    C = C0 + (x1.shape[2] if x1 is not None else 0)
    d0, d1 = dev(x0), dev(x1)
    part = Guarded(N, split, C, 2, dtype=torch.float64)
    _lib.check(_lib.lib().vd_op_gn_stats(_lib.ptr(d0), _lib.ptr(d1), C0, C, N, HW, split, _lib.ptr(part.t), _lib.current_stream()))
    return part.read()


@functools.lru_cache(maxsize=None)
def gpu_tables(c):
    """The case's one or two tables: by the statistics pass on the GPU where the source is a multiple of 32 channels wide, else by hand."""
    return R.pipe_tables(c, lambda x, split: run_stats(x, None, split))


def pipe_args(c):
    d = c.data
    gamma, beta, film, film_ld = R.make_params(d, c.film)
    t0, t1 = gpu_tables(c)
    return d, dev(gamma), dev(beta), dev(film), film_ld, dev(t0), dev(t1)


# ---------------------------------------------------------------------------------------------------- gn_stats_partial
@pytest.mark.parametrize("c", R.STATS_CASES, ids=STATS_IDS)
def test_statistics_table_per_entry(c):
    """Every [sum, sum of squares] entry against the exact sum: (m - 1) u S|x| and (m - 1) u Sxx for a range of m rows, equality on the
    exact families, zeros for an empty range; split 0 must be the split vd_gn_stats_split reports."""
    d = c.data
    x0, x1 = R.make_data(d)
    split = c.split if c.split > 0 else _lib.lib().vd_gn_stats_split(d.N, d.HW, d.C)
    assert split >= 1
    part = run_stats(x0, x1, split)
    if c.split <= 0:
        auto = Guarded(d.N, split, d.C, 2, dtype=torch.float64)
        d0 = dev(x0)
        _lib.check(_lib.lib().vd_op_gn_stats(_lib.ptr(d0), None, d.C0, d.C, d.N, d.HW, 0, _lib.ptr(auto.t), _lib.current_stream()))
        assert np.array_equal(auto.read(), part)
    t = R.exact_table(d, split)
    (es, ess), (bs, bss) = R.table_errors(part, t), R.table_bounds(t, d.exact)
    ws, wss = R.worst(part[..., 0], t.s_hi.astype(R.LD) + t.s_lo, bs), R.worst(part[..., 1], t.ss_hi.astype(R.LD) + t.ss_lo, bss)
    print(f"GN_SPATIAL_CASE | gn_stats | {R.label(c)} split {split} | max err/bound sum {ws:.3f} squares {wss:.3f}")
    assert bool((es <= bs).all()) and bool((ess <= bss).all()), (ws, wss)
    if d.exact:
        assert np.array_equal(part, t.part())
    assert not part[:, t.rows == 0].any()


# ---------------------------------------------------------------------------------------------------- gn_final_affine_kernel
@pytest.mark.parametrize("c", R.PIPE_CASES, ids=PIPE_IDS)
def test_final_affine_and_mean_rstd_per_element(c):
    """(A, B) per (frame, channel) and mr_out per (frame, group) from one or two tables; vd_op_gn_affine (no mr_out) gives the same bits."""
    d, gamma, beta, film, film_ld, t0, t1 = pipe_args(c)
    ref = R.reference(d, c.film)
    L = _lib.lib()
    A, B, mr = Guarded(d.N, d.C), Guarded(d.N, d.C), Guarded(d.N, 32, 2)
    _lib.check(L.vd_op_gn_affine_mr(_lib.ptr(t0), c.split0, d.C0, _lib.ptr(t1), c.split1, d.C, d.N, d.HW, _lib.ptr(gamma), _lib.ptr(beta),
                                    _lib.ptr(film), film_ld, _lib.ptr(A.t), _lib.ptr(B.t), _lib.ptr(mr.t), _lib.current_stream()))
    A2, B2 = Guarded(d.N, d.C), Guarded(d.N, d.C)
    _lib.check(L.vd_op_gn_affine(_lib.ptr(t0), c.split0, d.C0, _lib.ptr(t1), c.split1, d.C, d.N, d.HW, _lib.ptr(gamma), _lib.ptr(beta),
                                 _lib.ptr(film), film_ld, _lib.ptr(A2.t), _lib.ptr(B2.t), _lib.current_stream()))
    a, b, m = A.read(), B.read(), mr.read()
    assert np.array_equal(a, A2.read()) and np.array_equal(b, B2.read())
    w = {"A": R.worst(a, ref.A, ref.dA), "B": R.worst(b, ref.B, ref.dB),
         "mean": R.worst(m[..., 0], ref.mean, ref.dmean + R.E * np.abs(ref.mean).astype(np.float64)),
         "rstd": R.worst(m[..., 1], ref.rstd, ref.rho * ref.rstd.astype(np.float64))}
    print(f"GN_SPATIAL_CASE | gn_final_affine | {R.label(c)} | max err/bound " + " ".join(f"{k} {v:.3f}" for k, v in w.items()))
    assert max(w.values()) <= 1.0, w


# ---------------------------------------------------------------------------------------------------- affine_act_fold_kernel
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("c", R.PIPE_CASES, ids=PIPE_IDS)
def test_folding_pass_per_element(c, act):
    """y = silu?(x A + B) with (A, B) folded by every block from the tables: |x| dA + dB + 2e (|x A| + |B|), through SiLU's bound at act 1."""
    d, gamma, beta, film, film_ld, t0, t1 = pipe_args(c)
    ref = R.reference(d, c.film)
    x0, x1 = R.make_data(d)
    d0, d1 = dev(x0), dev(x1)
    y = Guarded(d.N, d.HW, d.C)
    _lib.check(_lib.lib().vd_op_gn_act_fold(_lib.ptr(d0), _lib.ptr(d1), d.C0, d.C, _lib.ptr(t0), c.split0, _lib.ptr(t1), c.split1, d.N, d.HW,
                                            _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(film), film_ld, act, _lib.ptr(y.t),
                                            _lib.current_stream()))
    want, bound = R.y_reference(R.concat(d), ref.A, ref.B, ref.dA, ref.dB, act)
    w = R.worst(y.read(), want, bound)
    print(f"GN_SPATIAL_CASE | affine_act_fold | {R.label(c)} act {act} | max err/bound {w:.3f}")
    assert w <= 1.0, w


# ---------------------------------------------------------------------------------------------------- affine_act_kernel
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("c", R.PIPE_CASES, ids=PIPE_IDS)
def test_activation_pass_per_element(c, act):
    """The pass alone, handed the reference's (A, B) rounded to fp32: 2e (|x A| + |B|), through SiLU's bound at act 1."""
    d = c.data
    ref = R.reference(d, c.film)
    A32, B32 = ref.A.astype(np.float32), ref.B.astype(np.float32)
    x0, x1 = R.make_data(d)
    d0, d1, dA, dB = dev(x0), dev(x1), dev(A32), dev(B32)
    y = Guarded(d.N, d.HW, d.C)
    _lib.check(_lib.lib().vd_op_affine_act(_lib.ptr(d0), _lib.ptr(d1), d.C0, d.C, _lib.ptr(dA), _lib.ptr(dB), d.N, d.HW, act, _lib.ptr(y.t),
                                           _lib.current_stream()))
    zero = np.zeros_like(ref.dA)
    want, bound = R.y_reference(R.concat(d), A32.astype(R.LD), B32.astype(R.LD), zero, zero, act)
    w = R.worst(y.read(), want, bound)
    print(f"GN_SPATIAL_CASE | affine_act | {R.label(c)} act {act} | max err/bound {w:.3f}")
    assert w <= 1.0, w


# ---------------------------------------------------------------------------------------------------- refusals
# (C0, C, src1 given, part1 given, what the message must name).  C 48 is a legal width for affine_act_kernel (any multiple of 4).
REFUSALS = [(48, 48, True, True, "C % 32 == 0"), (6, 64, True, True, "C0 % 4 == 0"), (1056, 1056, True, True, "C <= 1024"),
            (32, 64, False, True, "src1 != nullptr"), (32, 64, True, False, "part1")]


@pytest.mark.parametrize("C0,C,src1,part1,text", REFUSALS, ids=["C48", "C0=6", "C1056", "null-src1", "null-part1"])
def test_shapes_outside_the_envelope_are_refused_without_a_launch(C0, C, src1, part1, text):
    """Each entry answers -1, names the constraint in vd_last_error and writes nothing."""
    L = _lib.lib()
    N, HW, st = 1, 4, _lib.current_stream()
    big = torch.zeros(1 << 16, device="cuda")                       # every input: far larger than any of these shapes would read
    tab = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
    s1 = _lib.ptr(big) if src1 else None
    p1 = _lib.ptr(tab) if part1 else None
    outs = []

    def refused(rc, out):
        assert rc == -1 and text in L.vd_last_error().decode(), (rc, L.vd_last_error())
        outs.extend(out)

    if part1:                                                       # entries that read the tensor
        o = Guarded(N, 4, C, 2, dtype=torch.float64)
        refused(L.vd_op_gn_stats(_lib.ptr(big), s1, C0, C, N, HW, 1, _lib.ptr(o.t), st), [o])
        if C != 48:
            o = Guarded(N, HW, C)
            refused(L.vd_op_affine_act(_lib.ptr(big), s1, C0, C, _lib.ptr(big), _lib.ptr(big), N, HW, 1, _lib.ptr(o.t), st), [o])
    if src1:                                                        # entries that read the tables
        o = [Guarded(N, C), Guarded(N, C), Guarded(N, 32, 2)]
        refused(L.vd_op_gn_affine_mr(_lib.ptr(tab), 1, C0, p1, 1, C, N, HW, _lib.ptr(big), _lib.ptr(big), None, 0, _lib.ptr(o[0].t),
                                     _lib.ptr(o[1].t), _lib.ptr(o[2].t), st), o)
    o = Guarded(N, HW, C)
    refused(L.vd_op_gn_act_fold(_lib.ptr(big), s1, C0, C, _lib.ptr(tab), 1, p1, 1, N, HW, _lib.ptr(big), _lib.ptr(big), None, 0, 1,
                                _lib.ptr(o.t), st), [o])
    assert all(g.untouched() for g in outs)
