"""GPU: what lies between the kernels of the backward-data pass (csrc/engine.hip: backward()), element by element against float64 --
the two matrix-product calls bwd_conv3 / bwd_linear over the backward weight images (with the engine's own argument setup:
vd_op_conv3_bwd_data, vd_op_linear_bwd_data), zero_stuff2 / sumpool2 / add, launch_grad_rescale, and the two guidance passes.  The
references are the gradients of the plain forward by torch autograd (tests/backward_data_restated.py, held to the composed forms in
tests/test_backward_data_cpu.py); the cases are tests/backward_data_cases.py.  The process' own split mode here, the other one through
tools/backward_data_check.py as a child process."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import backward_data_cases as C
import backward_data_restated as R
import step_nll_restated as SN
import video_diffusion_amd as vda
from conv_gemm_cases import FACTOR, Guarded, guarded_in, same_bits
from helpers import load_npz, synth_sd
from video_diffusion_amd import _lib
from video_diffusion_amd.script_util import create_gaussian_diffusion

pytestmark = pytest.mark.gpu
p, L = _lib.ptr, _lib.lib


def stream():
    return _lib.current_stream()


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------------- convs and linears
@pytest.mark.parametrize("c", [pytest.param(c, id=C.label(c)) for c in C.CASES])
def test_backward_data_matrix_products_per_element(c):
    """e = max |out - ref64| / S <= max(4 e_f32, FLOOR[mode]) (tests/conv_gemm_cases.py: the factor and the floors; derivation in
    tests/test_gpu_conv_gemm.py).  ref64: torch.autograd.grad of F.conv2d(x, w, stride, padding=1) / x @ w.T / the stem's im2col product
    with respect to the input, in float64, + the residual -- a Downsample case differentiates the stride-2 conv and hands the call the
    zero-stuffed gradient.  S: the absolute sum of the element's own terms over the backward operator (conv_ref / wino_ref with
    absolute=True, residual included), e_f32 the float32 CPU evaluation of the same algorithm (wino_ref in float32 for the Winograd
    image; conv_ref(sequential=True), the sum starting at the residual where gemm_split.hip's accumulators do, on evenly spaced frames
    for the big shapes).  Nothing is taken from the kernel under test.

    Every case also: the library names the instantiation the case states (and the slices of its split-K); inputs are read between NaN
    margins, the output is written between sentinel margins that stay untouched; a second launch gives the same bits; a residual in
    place (res == out, `out` preloaded: the non-fresh Downsample branch) gives the bits of the residual out of place.  Cases marked
    mags, in every split mode: dy 2^-20 and 2^-40 through vd_op_grad_rescale -> the call -> * gs[1] meet the plain bound (required);
    the same without the rescale is measured and printed, not asserted (docs/LAB_NOTES.md: what launch_grad_rescale is for)."""
    mode = C.process_mode()
    if mode == "fp32":
        x = torch.zeros(16, device="cuda")                          # (refused before anything is read)
        for rc in (L().vd_op_conv3_bwd_data(p(x), 1, 4, 32, p(x), 3, 32, None, p(x), stream()),
                   L().vd_op_linear_bwd_data(p(x), 4, 32, p(x), None, p(x), 32, stream())):
            assert rc != 0 and C.REFUSAL in L().vd_last_error().decode()
        pytest.skip("VD_MATH=fp32: the backward pass is refused by name")
    r = C.run_case(c)
    print(C.case_line(r))
    assert not C.failures(r), (r["label"], C.failures(r), r)


CHILD_DIED = []          # a child that ended by signal or timeout: nothing more is started on the GPU
CHILD_TIMEOUT = 120      # measured: 4 s with library load and device start (docs/LAB_NOTES.md); some 25 x that for a loaded machine


def test_every_case_in_the_other_split_mode():
    """VD_MATH is read once per process: tools/backward_data_check.py runs the same table through the same run_case() in a fresh child
    process, and every line is held to the assertions above."""
    mode = C.process_mode()
    if mode == "fp32":
        pytest.skip("VD_MATH=fp32: the backward pass is refused by name")
    other = "bf16x6" if mode == "f16x3" else "f16x3"
    assert not CHILD_DIED, f"the {CHILD_DIED[0]} child ended by signal or timeout: no further child is started"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "backward_data_check.py")], env={**os.environ, "VD_MATH": other},
                           capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        CHILD_DIED.append(other)
        raise
    print(f"backward data, {other}: child ran {time.time() - t0:.0f} s of {CHILD_TIMEOUT}")
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        CHILD_DIED.append(other)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    lines = [json.loads(s) for s in r.stdout.splitlines() if s.startswith("{")]
    summary, rows = lines[-1], lines[:-1]
    assert summary.get("summary") is True and summary["mode"] == other and summary["cases"] == len(rows) == len(C.CASES)
    for c, row in zip(C.CASES, rows):
        print(C.case_line(row))
        assert row["label"] == C.label(c) and row["mode"] == other and row["expected_variant"] == C.variant_name(c, other)
        assert not C.failures(row), (row["label"], C.failures(row), row)
    assert summary["failed"] == []


# ---------------------------------------------------------------------------------------------------- zero_stuff2, sumpool2, add
# (nfr, Ho, Wo, C): one pixel; non-square; C = 4 and C = 1024; the last: more than 8192 * 256 quads of output, so the grid-stride loop wraps
SMALL_MAPS = [(3, 1, 1, 4), (2, 3, 5, 1024), (1, 1, 1, 1024), (5, 7, 2, 36)]
RESAMPLE = SMALL_MAPS + [(3, 32, 33, 704)]              # zero_stuff2 writes 4 Ho Wo pixels per frame
POOLED = SMALL_MAPS + [(3, 64, 43, 1024)]               # sumpool2 writes Ho Wo


@pytest.mark.parametrize("nfr,Ho,Wo,C", RESAMPLE)
def test_zero_stuff2_bits(nfr, Ho, Wo, C):
    x = rnd(nfr, Ho, Wo, C, seed=C + Ho)
    out, xd = Guarded((nfr, 2 * Ho, 2 * Wo, C)), guarded_in(x)     # out: preloaded with NaN between sentinel margins
    _lib.check(L().vd_op_zero_stuff2(p(xd), nfr, Ho, Wo, C, p(out.t), stream()))
    torch.cuda.synchronize()
    got = out.t.cpu()
    assert out.untouched() and same_bits(got, R.zero_stuff2(x))    # exact +0 at the odd positions, the source's bits at the even ones
    if (nfr, Ho) == RESAMPLE[-1][:2]:
        assert got.numel() // 4 > 8192 * 256


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("nfr,Ho,Wo,C", POOLED)
def test_sumpool2_bits(nfr, Ho, Wo, C, acc):
    """((b00 + b01) + b10) + b11, then + y: float32 torch in the kernel's written order, to the bit."""
    x, y = rnd(nfr, 2 * Ho, 2 * Wo, C, seed=C + Wo), rnd(nfr, Ho, Wo, C, seed=7)
    out, xd = Guarded((nfr, Ho, Wo, C)), guarded_in(x)
    if acc:
        out.t.copy_(y)
    _lib.check(L().vd_op_sumpool2(p(xd), nfr, Ho, Wo, C, acc, p(out.t), stream()))
    torch.cuda.synchronize()
    assert out.untouched() and same_bits(out.t.cpu(), R.sumpool2(x, y if acc else None))
    if (nfr, Ho) == POOLED[-1][:2]:
        assert out.t.numel() // 4 > 8192 * 256


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("n", [4, 4 * 1024, 1001 * 4, 4 * (8192 * 256 + 3)])
def test_add_bits(n, acc):
    x, y = rnd(n, seed=n % 1000), rnd(n, seed=3)
    out, xd = Guarded((n,)), guarded_in(x)
    if acc:
        out.t.copy_(y)
    _lib.check(L().vd_op_add(p(xd), n, acc, p(out.t), stream()))
    torch.cuda.synchronize()
    assert out.untouched() and same_bits(out.t.cpu(), x + y if acc else x)
    assert L().vd_op_add(p(out.t), 6, 0, p(out.t), stream()) != 0   # whole 16-byte quads only: refused, not rounded down


# ---------------------------------------------------------------------------------------------------- grad_rescale
def rescale(g):
    out = Guarded(tuple(g.shape))
    out.t.copy_(g)
    gs = torch.full((4,), float("nan"), device="cuda")
    _lib.check(L().vd_op_grad_rescale(p(out.t), g.numel(), p(gs), stream()))
    torch.cuda.synchronize()
    assert out.untouched()
    return out.t.cpu(), gs.cpu()


DENORM = float(np.float32(2.0 ** -126) - np.float32(2.0 ** -149))       # the largest denormal


@pytest.mark.parametrize("n", [1, 1000, 1024 * 256 + 3])
@pytest.mark.parametrize("mag", [1.0, 3e-9, 1e-30, 6e4, 2.9e38, DENORM, 0.0])
def test_grad_rescale_is_an_exact_power_of_two(n, mag):
    """g * s to the bit, gs[0] gs[1] == 1, max |g s| in [1, 2); all zero: s = 1; the largest denormal: the clamp 2^100; a maximum just
    under 3e38: the clamp 2^-100, nothing overflows."""
    g = rnd(n, seed=n)
    g = g / g.abs().max() * mag
    g[n // 2] = mag                                                 # the maximum is exactly mag
    got, gs = rescale(g)
    s, m = R.grad_rescale(g)
    assert float(gs[0]) == s and float(gs[0]) * float(gs[1]) == 1.0 and float(gs[3]) == 0.0
    assert gs.view(torch.int32)[2] == torch.tensor(m, dtype=torch.float32).view(torch.int32)
    assert same_bits(got, g * torch.tensor(s, dtype=torch.float32))
    assert torch.isfinite(got).all()
    if mag == 0.0:
        assert s == 1.0
    elif mag == DENORM:
        assert s == 2.0 ** 100
    elif mag == 2.9e38:
        assert s == 2.0 ** -100
    else:
        assert 1.0 <= float(got.abs().max()) < 2.0


def test_grad_rescale_edges():
    """A NaN among finite values: s from the finite maximum, the NaN stays; an inf: s = 1; 3e38 and above: s = 1."""
    g = rnd(5000, seed=1) * 1e-6
    g[17] = float("nan")
    got, gs = rescale(g)
    s, m = R.grad_rescale(g)
    assert float(gs[0]) == s > 1.0 and torch.isnan(got[17]) and int(torch.isnan(got).sum()) == 1
    keep = ~torch.isnan(g)
    assert same_bits(got[keep], (g * s)[keep]) and 1.0 <= float(got[keep].abs().max()) < 2.0
    for big in (float("inf"), 3.0e38, 3.4e38):
        g = rnd(300, seed=2)
        g[5] = -big
        got, gs = rescale(g)
        assert float(gs[0]) == 1.0 == float(gs[1]) and same_bits(got, g)


# ---------------------------------------------------------------------------------------------------- guided_grad / guided_final
_state = {}
SCHEDULE = "linear_ddim250"


def engine():
    """The tiny engine with a schedule bound -> (model, float32 rows)."""
    if not _state:
        cfg = json.loads(str(load_npz("unet_tiny.npz")["cfg_json"]))
        model, _ = vda.create_video_model_and_diffusion(**{k: cfg[k] for k in vda.video_model_and_diffusion_defaults()})
        model.load_state_dict(synth_sd(model.param_specs()))
        model.to("cuda")
        model.eval()
        diff = create_gaussian_diffusion(**dict(SN.SCHEDULES)[SCHEDULE])
        diff._bind(model)
        tab = SN.tables(diff)
        tab["al"] = (1.0 - np.asarray(diff.betas, np.float64)).astype(np.float32)
        _state.update(model=model, diff=diff, tab=tab)
    _state["diff"]._bind(_state["model"])
    return _state["model"], _state["tab"]


T_FR, PER_FR = 3, 1001                       # frames per item, elements per frame (unaligned to 4 and to 256)


def guided_inputs(tab, t, seed):
    """x, eps, noise, x_t_minus_1 [B][per], obs [B][T] of 0 and 1 per frame, and planted elements whose unclamped x_0 lies 1e-3 .. 1e-2
    inside and outside both clip bounds."""
    B, per = len(t), T_FR * PER_FR
    g = torch.Generator().manual_seed(seed)
    x, eps, z, xm = (torch.randn(B, per, generator=g) for _ in range(4))
    obs = torch.tensor([[1.0, 0.0, 1.0], [1.0, 1.0, 1.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]])[torch.arange(B) % 4]
    c = {k: torch.as_tensor(tab[k]).double()[t][:, None] for k in ("sr", "srm1")}
    targets = torch.tensor([1 + 1e-3, 1 - 1e-3, -1 + 1e-3, -1 - 1e-3, 1 + 1e-2, -1 - 1e-2, 1 - 1e-2, -1 + 1e-2], dtype=torch.float64)
    for f in range(T_FR):
        cols = f * PER_FR + 11 * torch.arange(len(targets))
        eps[:, cols] = ((c["sr"] * x[:, cols].double() - targets[None, :]) / c["srm1"]).float()
    return x, eps, z, xm, obs


def run_guided_grad(model, x, eps, z, xm, obs, t, clip, want=("mean", "xstart")):
    B, per = x.shape
    out = {k: Guarded((B, per)) for k in ("deps", "dxd") + tuple(want)}
    xd, ed, zd, md, od, td = [guarded_in(v) for v in (x, eps, z, xm, obs)] + [t.cuda()]
    _lib.check(L().vd_op_guided_grad(model._handle, B, T_FR, per, p(xd), p(ed), p(zd), p(md), p(od), p(td), clip, p(out["deps"].t), p(out["dxd"].t),
                                     p(out["mean"].t) if "mean" in out else None, p(out["xstart"].t) if "xstart" in out else None, stream()))
    torch.cuda.synchronize()
    assert all(o.untouched() for o in out.values())
    return {k: o.t.cpu() for k, o in out.items()}


def held(got, ref64, f32, unit, keep, what):
    """Every output on its own: e_got <= 4 e_f32 over the element's absolute sum."""
    for k in ref64:
        u = unit[k].clamp_min(1e-300)
        e_got = float(((got[k].double() - ref64[k]).abs() / u)[keep].max())
        e_f32 = float(((f32[k].double() - ref64[k]).abs() / u)[keep].max())
        print(f"GUIDED | {what} | {k} | e_got {e_got:.2e} | e_f32 {e_f32:.2e}")
        assert torch.isfinite(got[k][keep]).all() and e_got <= FACTOR * e_f32, (what, k, e_got, e_f32)


@pytest.mark.parametrize("clip", [1, 0])
def test_guided_grad_per_element(clip):
    """deps, dxd, mean, xstart against float64 autograd of the loss as oracle/sampler_ref.py states it (gaussian_diffusion.py:319-364),
    each at most 4 x the float32 torch evaluation of the same expressions over the element's absolute sum.  t = 0 (no noise term), 3, the
    middle and NT - 1; obs masks of 0 and 1 per frame.  The clip indicator is discontinuous: elements with ||x0r_64| - 1| < 1e-5 are
    excluded -- under 0.1 % (test_backward_data_cpu.py: about 1e-5 of randn inputs) -- and elements planted 1e-3 and 1e-2 inside and
    outside both bounds exercise both branches."""
    model, tab = engine()
    t = torch.tensor([0, 3, tab["NT"] // 2, tab["NT"] - 1])
    x, eps, z, xm, obs = guided_inputs(tab, t, seed=5 + clip)
    obs_e = obs.repeat_interleave(PER_FR, 1)
    ref = R.guided_grad(tab, x, eps, z, xm, obs_e, t, clip)
    x0r = ref.pop("x0r")
    near = ((x0r.abs() - 1).abs() < 1e-5) if clip else torch.zeros_like(x0r, dtype=torch.bool)
    assert float(near.double().mean()) < 1e-3
    planted = x0r[:, 11 * torch.arange(8)]
    assert bool((planted.abs() > 1).any()) and bool((planted.abs() < 1).any()) and float((planted.abs() - 1).abs().min()) > 9e-4
    got = run_guided_grad(model, x, eps, z, xm, obs, t, clip)
    held(got, ref, R.guided_grad_f32(tab, x, eps, z, xm, obs_e, t, clip), R.guided_grad_units(tab, x, eps, z, xm, obs_e, t), ~near, f"grad clip={clip}")
    if clip:                                                        # outside the bounds nothing passes to eps; the frames with obs = 0 have no gradient
        out = (x0r.abs() > 1 + 1e-5)
        assert not got["deps"][out].any() and bool(got["deps"][~out & (obs_e > 0)].any())
    assert not got["deps"][obs_e == 0].any() and not got["dxd"][obs_e == 0].any()
    # optional outputs as null: the same bits in the two that remain
    bare = run_guided_grad(model, x, eps, z, xm, obs, t, clip, want=())
    assert same_bits(bare["deps"], got["deps"]) and same_bits(bare["dxd"], got["dxd"])
    model.check_device_errors()


def test_guided_grad_out_of_range_t_and_non_finite_eps():
    model, tab = engine()
    model.check_device_errors()
    NT = tab["NT"]
    t = torch.tensor([5, NT, 0, -1])
    x, eps, z, xm, obs = guided_inputs(tab, t.clamp(0, NT - 1), seed=9)
    got = run_guided_grad(model, x, eps, z, xm, obs, t, 1)
    good = torch.tensor([0, 2])
    ref = run_guided_grad(model, x[good], eps[good], z[good], xm[good], obs[good], t[good], 1)
    for k in ("deps", "dxd"):
        assert torch.isnan(got[k][[1, 3]]).all() and same_bits(got[k][good], ref[k]) and torch.isfinite(ref[k]).all()
    model.check_device_errors()
    # a non-finite eps: bit 1 is raised and the x_0 prediction is not clamped into range
    t = torch.tensor([5, 7])
    x, eps, z, xm, obs = guided_inputs(tab, t, seed=10)
    eps[1, 40] = float("inf")
    eps[0, 90] = float("nan")
    got = run_guided_grad(model, x, eps, z, xm, obs, t, 1)
    with pytest.raises(FloatingPointError):
        model.check_device_errors()
    model.check_device_errors()
    assert not torch.isfinite(got["xstart"][1, 40]) and torch.isnan(got["xstart"][0, 90])
    assert int((~torch.isfinite(got["xstart"])).sum()) == 2


@pytest.mark.parametrize("inv_s", [1.0, 2.0 ** -17])
def test_guided_final_per_element(inv_s):
    """grad = dxd + dx_net gs[1], mean' = mean - 10 alpha_t grad / 2, sample = mean' + [t != 0] sigma z2: each against float64, at most
    4 x the float32 torch evaluation over the element's absolute sum; t = 0, NT - 1; optional outputs as null; t outside the table."""
    model, tab = engine()
    NT = tab["NT"]
    t = torch.tensor([0, 3, NT // 2, NT - 1])
    B, per = 4, T_FR * PER_FR
    g = torch.Generator().manual_seed(21)
    dxd, mean, z2 = (torch.randn(B, per, generator=g) for _ in range(3))
    dx_net = torch.randn(B, per, generator=g) / inv_s
    gs = torch.tensor([1.0 / inv_s, inv_s, 0.0, 0.0], device="cuda")

    def run(t, want=("grad", "mean_out", "sample")):
        out = {k: Guarded((len(t), per)) for k in want}
        a = lambda k: p(out[k].t) if k in out else None         # noqa: E731
        n = len(t)
        td, dd, md, nd, zd = [t.cuda()] + [guarded_in(v[:n].contiguous()) for v in (dxd, mean, dx_net, z2)]
        _lib.check(L().vd_op_guided_final(model._handle, n, T_FR, per, p(td), p(dd), p(md), p(nd), p(gs), p(zd), a("grad"), a("mean_out"), a("sample"),
                                          stream()))
        torch.cuda.synchronize()
        assert all(o.untouched() for o in out.values())
        return {k: o.t.cpu() for k, o in out.items()}

    got = run(t)
    keep = torch.ones(B, per, dtype=torch.bool)
    held(got, R.guided_final(tab, dxd, mean, dx_net, inv_s, z2, t), R.guided_final(tab, dxd, mean, dx_net, inv_s, z2, t, dtype=torch.float32),
         R.guided_final_units(tab, dxd, mean, dx_net, inv_s, z2, t), keep, f"final 1/s={inv_s:g}")
    assert same_bits(got["sample"][0], got["mean_out"][0])           # t = 0: no noise
    assert same_bits(run(t, want=("sample",))["sample"], got["sample"]) and same_bits(run(t, want=("grad",))["grad"], got["grad"])
    bad = run(torch.tensor([NT, 3, -1, NT - 1]))
    for k in ("mean_out", "sample"):
        assert torch.isnan(bad[k][[0, 2]]).all() and same_bits(bad[k][[1, 3]], got[k][[1, 3]])
    model.check_device_errors()
