"""CPU: the yardstick of tests/test_gpu_gn_spatial.py (tests/gn_spatial_restated.py) checked on its own -- the exact-sum reference
against F.group_norm in fp64, a line-by-line emulation of the three kernels against the derived bounds on every GPU case, the
same emulation with five deliberate mistakes (which the bounds must reject), the launch geometry the case list rests on, and
the host-side choices the library exports (vd_gn_act_form, vd_gn_stats_split)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gn_spatial_restated as R
from video_diffusion_amd import _lib

PIPE_IDS = [R.label(c) for c in R.PIPE_CASES]
STATS_IDS = [R.label(c) for c in R.STATS_CASES]


def emu_stats(x, split):
    return R.emulate_stats(x.numpy(), split)


def pipe_worst(c, *, final_kw=None, fold_kw=None, stats=emu_stats):
    """max err/bound of the emulated gn_final_affine (A, B, mr), folding pass (A, B, y at act 0 and 1) and activation pass."""
    d = c.data
    gamma, beta, film, _ = R.make_params(d, c.film)
    ref = R.reference(d, c.film)
    t0, t1 = R.pipe_tables(c, stats)
    x = R.concat(d)
    out = {}
    A, B, mr = R.emulate_final_affine(t0, c.split0, d.C0, t1, c.split1, d.C, d.HW, gamma, beta, film, **(final_kw or {}))
    out["affine A"], out["affine B"] = R.worst(A, ref.A, ref.dA), R.worst(B, ref.B, ref.dB)
    out["mr mean"] = R.worst(mr[..., 0], ref.mean, ref.dmean + R.E * np.abs(ref.mean).astype(np.float64))
    out["mr rstd"] = R.worst(mr[..., 1], ref.rstd, ref.rho * ref.rstd.astype(np.float64))
    A, B = R.emulate_fold_ab(t0, c.split0, d.C0, t1, c.split1, d.C, d.HW, gamma, beta, film, **(fold_kw or {}))
    out["fold A"], out["fold B"] = R.worst(A, ref.A, ref.dA), R.worst(B, ref.B, ref.dB)
    for act in (0, 1):
        y, bound = R.y_reference(x, ref.A, ref.B, ref.dA, ref.dB, act)
        out[f"fold y act{act}"] = R.worst(R.emulate_apply(x, A, B, act), y, bound)
        A32, B32 = ref.A.astype(np.float32), ref.B.astype(np.float32)
        zero = np.zeros_like(ref.dA)
        y, bound = R.y_reference(x, A32.astype(R.LD), B32.astype(R.LD), zero, zero, act)
        out[f"act y act{act}"] = R.worst(R.emulate_apply(x, A32, B32, act), y, bound)
    return out


@pytest.mark.parametrize("c", R.PIPE_CASES, ids=PIPE_IDS)
def test_reference_agrees_with_group_norm_in_fp64(c):
    """y of the exact-sum reference against F.group_norm(x, 32, gamma, beta, 1e-5) in fp64 with FiLM and SiLU written out: 1e-12.
    F.group_norm is handed x minus the family's offset (30, 100, 3.25: an exact subtraction in fp64, and GroupNorm does not see a
    common offset): its own fp64 mean is off by u |mean|, which the normalisation multiplies by rstd |gamma (1 + scale)| -- 1.5e-12 at
    the dyadic family's mean of 100, the error of the comparison and not of the reference under test."""
    d = c.data
    gamma, beta, film, _ = R.make_params(d, c.film)
    ref = R.reference(d, c.film)
    x = R.concat(d)
    off = {"n01": 0.0, "m30": 30.0, "dyadic": 100.0, "const": 3.25}[d.family]
    want = F.group_norm((torch.from_numpy(x).double() - off).permute(0, 2, 1), 32, gamma.double(), beta.double(), eps=1e-5).permute(0, 2, 1)
    if film is not None:
        want = want * (1 + film[:, None, :d.C].double()) + film[:, None, d.C:2 * d.C].double()
    zero = np.zeros_like(ref.dA)
    for act in (0, 1):
        got, _ = R.y_reference(x, ref.A, ref.B, zero, zero, act)
        w = F.silu(want) if act else want
        assert float(np.abs(got.astype(np.float64) - w.numpy()).max()) <= 1e-12


def test_the_exact_families_have_exact_sums():
    """Dyadic and constant data: every exact sum is a double (lo = 0), so a table of fp64 running sums must equal it to the bit."""
    seen = 0
    for c in R.STATS_CASES:
        if c.data.exact:
            t = R.exact_table(c.data, c.split)
            assert not t.s_lo.any() and not t.ss_lo.any()
            assert np.array_equal(R.emulate_stats(R.concat(c.data), c.split), t.part())
            seen += 1
    assert seen >= 5


@pytest.mark.parametrize("c", R.STATS_CASES, ids=STATS_IDS)
def test_emulated_statistics_pass_stays_inside_the_table_bounds(c):
    d = c.data
    split = c.split if c.split > 0 else _lib.lib().vd_gn_stats_split(d.N, d.HW, d.C)
    t = R.exact_table(d, split)
    part = R.emulate_stats(R.concat(d), split)
    (es, ess), (bs, bss) = R.table_errors(part, t), R.table_bounds(t, d.exact)
    assert bool((es <= bs).all()) and bool((ess <= bss).all())
    empty = t.rows == 0
    assert not part[:, empty].any()


@pytest.mark.parametrize("c", R.PIPE_CASES, ids=PIPE_IDS)
def test_emulated_kernels_stay_inside_the_bounds(c):
    w = pipe_worst(c)
    print(f"GN_SPATIAL_EMULATED | {R.label(c)} | " + " ".join(f"{k} {v:.3f}" for k, v in w.items()))
    assert max(w.values()) <= 1.0, w


def test_deliberate_mistakes_leave_the_bounds():
    """Five value-only mistakes, each of which must push at least one case past err/bound 1 (the bounds are tight enough to see them)."""
    # (a) the square in fp32, (b) the tail loop's last row missing from the sum of squares: both visible in the table itself
    for kw in (dict(sq32=True), dict(tail_drop_ss=True)):
        bad = 0
        for c in R.STATS_CASES[:8]:
            d = c.data
            split = c.split if c.split > 0 else 4
            t = R.exact_table(d, split)
            (es, ess), (bs, bss) = R.table_errors(R.emulate_stats(R.concat(d), split, **kw), t), R.table_bounds(t, d.exact)
            bad += bool((ess > bss).any())
        assert bad, kw
    two = [c for c in R.PIPE_CASES if c.data.C1]
    film = [c for c in R.PIPE_CASES if c.film]
    # (c) the folding pass walks the second table from pl + 1, (d) gn_final_affine takes split0 for the second table, (e) B from the scaled A
    assert any(max(v for k, v in pipe_worst(c, fold_kw=dict(skip_first=True)).items() if k.startswith("fold")) > 1.0 for c in two)
    up = [c for c in two if c.split0 < c.split1]             # (where the mistaken walk stays inside the second table)
    assert up and all(max(v for k, v in pipe_worst(c, final_kw=dict(swap_split=True)).items() if k.startswith("affine")) > 1.0 for c in up)
    assert all(max(v for k, v in pipe_worst(c, fold_kw=dict(b_after_sc=True)).items() if k.startswith("fold")) > 1.0 for c in film[:3])


def test_the_case_list_reaches_the_launch_shapes_it_names():
    fold = {R.label(c): R.fold_launch(c.data.N, c.data.HW, c.data.C) for c in R.PIPE_CASES}
    act = {R.label(c): R.act_launch(c.data.N, c.data.HW, c.data.C) for c in R.PIPE_CASES}
    assert {t for t, _, _ in fold.values()} >= {256, 240, 192, 168, 224}
    assert fold["C32-HW1024-n01-split1"] == (256, 2, 512) and fold["C1024-HW64-n01-split1-film"] == (256, 4, 16)
    assert act["C32-HW1024-n01-split1"] == (256, 8, 128) and act["C1024-HW64-n01-split1-film"] == (256, 16, 4)
    heads = set()
    for c in R.PIPE_CASES:                      # (head, tail) of pixel lane 0 in the folding pass
        _, _, per = fold[R.label(c)]
        rows = len(range(0, min(per, c.data.HW), R.ppi_of(c.data.C)))
        heads.add((rows >= 4, rows % 4 != 0))
    assert heads >= {(False, True), (True, True), (True, False)}
    items = {(c.data.C // 32) * max(c.split0, c.split1) for c in R.PIPE_CASES}
    assert items >= {1, 8, 32, 33} and max(items) >= 128
    assert any(c.split0 > R.ppi_of(c.data.C) for c in R.PIPE_CASES) and any(c.split0 < R.ppi_of(c.data.C) for c in R.PIPE_CASES)
    assert {(c.split0, c.split1) for c in R.PIPE_CASES if c.data.C1} >= {(16, 1), (1, 4)}
    assert any(0 in R.exact_table(c.data, c.split).rows for c in R.STATS_CASES if c.split)


def test_the_engines_choice_of_form_switches_at_64_mb():
    """vd_gn_act_form: the folding pass below 64 MB of fp32 tensor for the whole layer call, two launches from 64 MB on."""
    L = _lib.lib()
    assert L.vd_gn_act_form(524288, 1, 32) == 1 and L.vd_gn_act_form(524287, 1, 32) == 0        # 2^26 bytes, and 128 bytes less
    assert L.vd_gn_act_form(32, 4096, 128) == 1 and L.vd_gn_act_form(31, 4096, 128) == 0
    assert L.vd_gn_act_form(16, 4096, 224) == 0 and L.vd_gn_act_form(16, 4096, 256) == 1
    assert L.vd_gn_act_form(1, 16, 32) == 0
    assert L.vd_gn_act_form(128, 4096, 1024) == 1                                            # 2^31 bytes: no 32-bit product


def test_the_statistics_split_the_library_reports():
    L = _lib.lib()
    for nfr, HW, C in [(2, 1024, 32), (2, 64, 1024), (128, 4096, 128), (8, 256, 512), (4096, 4096, 32), (1, 5, 96)]:
        ppi, split = R.ppi_of(C), 1
        while nfr * split < 2048 and HW // (split * 2) >= ppi * 8:
            split *= 2
        assert L.vd_gn_stats_split(nfr, HW, C) == split
    assert L.vd_gn_stats_split(2, 64, 48) == -1 and L.vd_gn_stats_split(2, 64, 1056) == -1 and L.vd_gn_stats_split(0, 64, 32) == -1
