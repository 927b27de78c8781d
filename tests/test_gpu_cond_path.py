"""GPU: the kernels that build what the network is conditioned on (csrc/misc.hip), each through its vd_op_* entry -- the launcher the
forward pass calls, arguments in the forward pass' form -- against the references of tests/cond_path_restated.py (checked on the CPU by
tests/test_cond_path_cpu.py).

Per kernel: what it is held to, and the largest error measured on an MI355X (every test prints its figure before it asserts).

  kernel                     reference                                         bound                         measured
  rpe_table_kernel           UNetRef.rpe_R table branch, CPU float32           same row, torch.equal         0 rows differ (*)
  rpe_hidden_tab_kernel      float64 restatement                               1e-4 + 1e-4 |ref|             4.07e-6
  sinus_kernel               float64 cos | sin of the float32 product t f      4 * 2^-23 = 4.77e-7 absolute  6.59e-8
  frame_t_kernel             fi - fi.mean(1), CPU float32 (exact sums)         equality                      0
  assemble_kernel            UNetRef.with_grad's x5 / t_frames / anything      torch.equal                   0
                             + F.unfold reordered to k = tap * Cs + channel
  posenc_kernel              x + P + femb, CPU float32, in that order          equality                      0
  move_rows_kernel           the rows themselves                               bit for bit                   0
  scatter_stats_kernel       float64 sum over split, in order                  equality                      0
  engine, bucket table /     UNetRef eps, frame indices with d = +-4, +-8      1e-4 + 1e-4 |ref|             6.44e-6 / 6.41e-6
  RPENet, frame encoding       at (alpha, beta, gamma) = (2, 4, 8)

(*) The float32 form of the bucket (logf, fused multiply-add) agreed with the reference at every exact-integer distance of the table in
cond_path_restated.EXACT_INTEGER_DISTANCES except d = +-20 of (3, 7, 20): row 6 (and its mirror 9) instead of 7 (8).  rpe_table_kernel now
evaluates the value in fp64 and snaps it to an integer it is within 1e-6 of ("Bucket ids"); with that, 0 of the 112 560 compared
entries (per channel width) differ.
"""
import pytest
import torch

import cond_path_restated as R
import video_diffusion_amd as vda
from helpers import close, synth_sd
from oracle.unet_ref import UNetRef
from video_diffusion_amd import _lib

pytestmark = pytest.mark.gpu
SENT = -77.25                              # fill of every output buffer: what a kernel must not write stays this


def dev(t):
    return t.to("cuda").contiguous()


def op(name, *args):
    _lib.check(getattr(_lib.lib(), name)(*args, _lib.current_stream()))
    torch.cuda.synchronize()


def refused(name, *args):
    """The entry returns an error code and says why; nothing is launched."""
    rc = getattr(_lib.lib(), name)(*args, _lib.current_stream())
    torch.cuda.synchronize()
    return rc != 0 and len(_lib.lib().vd_last_error()) > 0


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + 7 * sum(shape) + len(shape))
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


# ================================================================================================ bucket table
BUCKET_SETS = list(R.EXACT_INTEGER_DISTANCES) + [R.DEGENERATE]


def rpe_table(table, fidx, al, be, ga):
    B, T = fidx.shape
    C = table.shape[1]
    out = torch.full((B, T, T, C), SENT, device="cuda")
    bufs = [dev(table), dev(fidx)]
    op("vd_op_rpe_table", _lib.ptr(bufs[0]), _lib.ptr(bufs[1]), B, T, C, float(al), float(be), float(ga), _lib.ptr(out))
    return out.cpu()


def _bucket_case(params):
    """fidx, distances, the entries the reference defines, and the reference's distances (0 where it defines nothing)."""
    al, be, ga = params
    fidx = R.covering_fidx(ga)
    dist = R.distances(fidx)
    present = set(dist.flatten().tolist())
    assert set(range(-(ga + 3), ga + 4)) <= present
    for d in R.EXACT_INTEGER_DISTANCES.get(params, {}):                 # a later edit must not drop the distances this test is about
        assert d in present and -d in present, (params, d)
    if al == be == ga:
        # alpha == beta == gamma: beyond alpha the reference computes log(|d| / alpha) / log(1) * 0 = inf * 0 = NaN and casts it to int,
        # which is undefined (on the CPU it comes out as INT_MIN and the table lookup raises).  Only |d| <= alpha is defined there.
        defined = dist.abs() <= al
    else:
        defined = torch.ones_like(dist, dtype=torch.bool)
    return fidx, dist, defined, torch.where(defined, dist, torch.zeros_like(dist))


@pytest.mark.parametrize("C", [32, 320])
@pytest.mark.parametrize("params", BUCKET_SETS, ids=lambda p: "a%d_b%d_g%d" % p)
def test_rpe_table_selects_the_reference_row_at_every_distance(params, C):
    al, be, ga = params
    nb = 2 * be + 1
    fidx, dist, defined, dist_ref = _bucket_case(params)
    want = R.bucket_rows_ref(dist_ref, al, be, ga)
    table = torch.arange(nb, dtype=torch.float32)[:, None].expand(nb, C).contiguous()      # row i holds i: the row can be read off
    got = rpe_table(table, fidx, al, be, ga)
    assert (got == got[..., :1]).all(), "a gathered row mixes table rows"
    rows = got[..., 0].long()
    assert ((rows >= 0) & (rows < nb)).all() and (got[..., 0] == rows).all()
    bad = (rows != want) & defined
    print(f"rpe_table {params} C={C}: {int(defined.sum())} entries compared, {int(bad.sum())} differ"
          + (f"; d = {sorted(set(dist[bad].tolist()))}: device {sorted(set(rows[bad].tolist()))}" if bad.any() else ""))
    assert not bad.any(), f"rows differ from the reference at distances {sorted(set(dist[bad].tolist()))}"
    for d, b in R.EXACT_INTEGER_DISTANCES.get(params, {}).items():
        assert (rows[dist == d] == b).all() and (rows[dist == -d] == nb - b).all(), (params, d)
    neg = dist < 0                                                           # negative ids wrap to id + 2 beta + 1
    assert (rows[neg & defined] == nb - rows.transpose(1, 2)[neg & defined]).all()
    if not defined.all():
        # where the reference defines nothing the kernel's fmin(beta, NaN) = beta: +-beta, wrapped -- whatever it is, a row of the table
        out = rows[~defined]
        assert ((out == be) | (out == nb - be)).all()


@pytest.mark.parametrize("C", [32, 320])
@pytest.mark.parametrize("params", BUCKET_SETS, ids=lambda p: "a%d_b%d_g%d" % p)
def test_rpe_table_gathers_random_rows(params, C):
    al, be, ga = params
    fidx, dist, defined, dist_ref = _bucket_case(params)
    table = rnd(2 * be + 1, C, seed=al + ga)
    want = R.bucket_gather_ref(table, dist_ref, al, be, ga)
    got = rpe_table(table, fidx, al, be, ga)
    assert torch.equal(got[defined], want[defined])


# ================================================================================================ RPENet hidden layer
def _fidx_patterns(B, T):
    """Frame-index tensors (B, T): ascending, descending, with repeats (d == 0 off the diagonal), gaps up to 10 000 with one row that
    starts at 50 000."""
    g = torch.Generator().manual_seed(B * 1000 + T)
    asc = torch.arange(T).view(1, T).repeat(B, 1) + 3 * torch.arange(B).view(B, 1)
    rep = torch.randint(0, max(2, T // 2), (B, T), generator=g)
    gaps = torch.cumsum(torch.randint(1, 10001, (B, T), generator=g), dim=1)
    gaps[-1] = gaps[-1] - gaps[-1, 0] + 50000
    if T > 1:
        gaps[:, -1] = gaps[:, -2] + 10000
        rep[:, -1] = rep[:, 0]
    return dict(ascending=asc, descending=asc.flip(1), repeats=rep, gaps=gaps)


@pytest.mark.parametrize("B,T,C,nz", [(2, 1, 32, 1), (1, 5, 96, 3), (2, 64, 128, 2), (1, 65, 64, 3), (1, 128, 32, 2), (1, 7, 512, 1),
                                      (1, 3, 288, 2)])
def test_rpe_hidden_vs_fp64(B, T, C, nz):
    """T = 65 and 128: the 64-key chunk loop; C = 288 and 512: the c += 256 channel loop."""
    rows = B * T * T
    te_ld = nz * (C + 16) + 24                                               # wider than nz * C; net z's columns start at te_off[z]
    te_off = [8 + z * (C + 16) for z in range(nz)]
    te = rnd(B * T, te_ld, seed=1, scale=2.0)
    W = [rnd(C, 3, seed=10 + z) for z in range(nz)]
    bias = [rnd(C, seed=20 + z, scale=0.5) for z in range(nz)]
    # one weight buffer, weights and biases at unrelated places: [pad | b_{nz-1} .. b_0 | pad | W_0 | pad | W_1 ...]
    wbase, w_off, b_off, pos = [rnd(13, seed=3)], [0] * nz, [0] * nz, 13
    for z in reversed(range(nz)):
        b_off[z] = pos
        wbase.append(bias[z]); pos += C
    for z in range(nz):
        wbase.append(rnd(5 + z, seed=4)); pos += 5 + z
        w_off[z] = pos
        wbase.append(W[z].reshape(-1)); pos += 3 * C
    tab = torch.tensor([[te_off[z], w_off[z], b_off[z]] for z in range(nz)], dtype=torch.int64)
    zs_e = rows * C + 24
    bufs = [dev(te), dev(torch.cat(wbase)), dev(tab)]
    worst = 0.0
    for name, fidx in _fidx_patterns(B, T).items():
        E = torch.full((nz, zs_e), SENT, device="cuda")
        fd = dev(fidx)
        op("vd_op_rpe_hidden", _lib.ptr(bufs[0]), te_ld, _lib.ptr(bufs[1]), _lib.ptr(bufs[2]), _lib.ptr(fd), B, T, C, _lib.ptr(E), nz, zs_e)
        E = E.cpu()
        assert (E[:, rows * C:] == SENT).all(), f"{name}: wrote between two nets' outputs or behind the last"
        for z in range(nz):
            want = R.rpe_hidden_ref(te[:, te_off[z]:te_off[z] + C].reshape(B, T, C), W[z], bias[z], fidx)
            worst = max(worst, close(E[z, :rows * C].view(B, T, T, C), want))
    print(f"rpe_hidden B={B} T={T} C={C} nz={nz}: max |err| = {worst:.3e}")


# ================================================================================================ embeddings
T_VALUES = [0.0, -1.0, 999.0, 998.75, 3996.0, 12345.0, -7.5]               # t = 0; the 't=0' conditioning mode; (rescaled) timesteps;
SINUS_BOUND = 4 * 2.0 ** -23                                                # centred frame positions.  Bound: twice the documented 2 ulp
                                                                            # of the device's cosf / sinf on values of magnitude <= 1


@pytest.mark.parametrize("max_period", [10000, 160])                        # timestep table; frame table of a T = 16 model (10 * T)
@pytest.mark.parametrize("n", [1, 7, 260])
@pytest.mark.parametrize("dim", [32, 128, 512, 33])
def test_sinus_embed_vs_fp64(dim, n, max_period):
    t = torch.tensor(T_VALUES)
    t = t[3:4] if n == 1 else torch.cat([t, torch.linspace(-10.0, 4000.0, n - 7)])
    freqs = R.freq_table(dim // 2, max_period)
    out = torch.full((n, dim), SENT, device="cuda")
    bufs = [dev(t), dev(freqs)]
    op("vd_op_sinus_embed", _lib.ptr(bufs[0]), n, dim, _lib.ptr(bufs[1]), _lib.ptr(out))
    out = out.cpu()
    err = (out.double() - R.sinus_ref(t, freqs, dim)).abs().max().item()
    print(f"sinus_embed dim={dim} n={n} max_period={max_period}: max |err| = {err:.3e} (bound {SINUS_BOUND:.3e})")
    assert err <= SINUS_BOUND
    if dim % 2:
        assert (out[:, -1] == 0).all()


@pytest.mark.parametrize("center", [0, 1])
@pytest.mark.parametrize("B,T", [(1, 1), (2, 5), (3, 64), (1, 128)])
def test_frame_t_is_exact(B, T, center):
    g = torch.Generator().manual_seed(B * 131 + T)
    fidx = torch.randint(0, 100001, (B, T), generator=g)
    fidx[0, 0] = 100000
    if T > 2:
        fidx[:, 2] = fidx[:, 0]                                             # repeats
    assert (fidx.sum(1) < 2 ** 24).all()                                    # float32 sums are exact, whatever their order
    tv = torch.full((B, T), SENT, device="cuda")
    fd = dev(fidx)
    op("vd_op_frame_t", _lib.ptr(fd), B, T, center, _lib.ptr(tv))
    assert torch.equal(tv.cpu(), R.frame_t_ref(fidx, center))


# ================================================================================================ stem assembly
def _masks(B, T, pattern):
    """obs, latent, kinda-marginalised masks (B, T, 1, 1, 1) of 0 / 1."""
    m = torch.zeros(3, B, T)
    if pattern == "latent":
        m[1] = 1
    elif pattern == "observed":
        m[0] = 1
    elif pattern == "mixed":                                                # frames cycle observed, latent, kinda-marg, in no mask
        for b in range(B):
            for t in range(T):
                k = (b + t) % 4
                if k < 3:
                    m[k, b, t] = 1
    elif pattern == "one_item_observed":                                    # 't=0': item 0 has an observed frame, the others none
        m[1] = 1
        m[0, 0, T // 2], m[1, 0, T // 2] = 1, 0
    return [v.view(B, T, 1, 1, 1).clone() for v in m]


def _window(B, T, S, seed):
    x, x0, xm = (rnd(B, T, 3, S, S, seed=seed + i) for i in range(3))
    return x, x0, xm, torch.tensor([37.0, 999.0, 250.5])[:B].contiguous()


def _assemble(x, x0, xm, masks, t_model, cond_mode, obs_t_mode, Kpad, frame_list=None, scalars_only=0, expect_refusal=False):
    B, T, _, S, _ = x.shape
    N = B * T
    obs_src = x0 if cond_mode == 1 else (x if cond_mode == 2 else (x0, x, xm)[obs_t_mode])     # as the model's _pack_kwargs picks it
    cols = torch.full((N, S * S, max(Kpad, 1)), SENT, device="cuda")
    tf, am = torch.full((N,), SENT, device="cuda"), torch.full((N,), SENT, device="cuda")
    bufs = [dev(x), dev(obs_src)] + [dev(m.reshape(N)) for m in masks] + [dev(t_model)]
    fl = None if frame_list is None else dev(torch.tensor(list(frame_list) or [0], dtype=torch.int32))   # (an empty list is still a list)
    args = [*(_lib.ptr(b) for b in bufs), obs_t_mode, B, T, S, S, Kpad, cond_mode, _lib.ptr(fl), 0 if frame_list is None else len(frame_list),
            scalars_only, _lib.ptr(cols), _lib.ptr(tf), _lib.ptr(am)]
    if expect_refusal:
        assert refused("vd_op_assemble", *args)
    else:
        op("vd_op_assemble", *args)
    return cols.cpu(), tf.cpu(), am.cpu()


@pytest.mark.parametrize("Kpad", [64, 128])
@pytest.mark.parametrize("cond_mode", [0, 1, 2])
@pytest.mark.parametrize("B,T,S", [(2, 3, 8), (1, 2, 64), (1, 2, 128), (1, 1, 80)])
def test_assemble_shapes(B, T, S, cond_mode, Kpad):
    """S = 128: two 64-pixel strips per image row; S = 80: a ragged second strip (the launcher takes any width)."""
    x, x0, xm, t = _window(B, T, S, seed=S + cond_mode)
    masks = _masks(B, T, "mixed")
    obs_t_mode = (cond_mode + B) % 3
    want = R.assemble_ref(x, x0, xm, *masks, t, cond_mode, obs_t_mode, Kpad)
    got = _assemble(x, x0, xm, masks, t, cond_mode, obs_t_mode, Kpad)
    for g, w, what in zip(got, want, ("im2col", "t_frames", "amask")):
        assert torch.equal(g, w), what


@pytest.mark.parametrize("obs_t_mode", [0, 1, 2])
@pytest.mark.parametrize("cond_mode", [0, 1, 2])
def test_assemble_modes_and_masks(cond_mode, obs_t_mode):
    B, T, S = 2, 3, 8
    x, x0, xm, t = _window(B, T, S, seed=11)
    for pattern in ("latent", "observed", "mixed", "one_item_observed"):
        masks = _masks(B, T, pattern)
        want = R.assemble_ref(x, x0, xm, *masks, t, cond_mode, obs_t_mode, 64)
        got = _assemble(x, x0, xm, masks, t, cond_mode, obs_t_mode, 64)
        for g, w, what in zip(got, want, ("im2col", "t_frames", "amask")):
            assert torch.equal(g, w), (pattern, what)
        if cond_mode == 2 and pattern == "one_item_observed":
            assert got[1].tolist() == [-1.0] * T + [999.0] * T


@pytest.mark.parametrize("cond_mode", [0, 1, 2])
@pytest.mark.parametrize("B,T,S", [(2, 3, 8), (1, 2, 128)])
def test_assemble_frame_list_and_scalars_only(B, T, S, cond_mode):
    x, x0, xm, t = _window(B, T, S, seed=5)
    masks = _masks(B, T, "mixed")
    want = R.assemble_ref(x, x0, xm, *masks, t, cond_mode, 0, 64)
    frames = [4, 0, 3] if B * T == 6 else [1]                               # a permuted strict subset
    cols, tf, am = _assemble(x, x0, xm, masks, t, cond_mode, 0, 64, frame_list=frames)
    assert torch.equal(cols[:len(frames)], want[0][frames])                  # rows go to the list position ...
    assert (cols[len(frames):] == SENT).all() and (tf == SENT).all() and (am == SENT).all()      # ... nothing else is written
    cols, tf, am = _assemble(x, x0, xm, masks, t, cond_mode, 0, 64, scalars_only=1)
    assert (cols == SENT).all() and torch.equal(tf, want[1]) and torch.equal(am, want[2])
    cols, tf, am = _assemble(x, x0, xm, masks, t, cond_mode, 0, 64, frame_list=[])          # an empty list: nothing to do
    assert (cols == SENT).all() and (tf == SENT).all()


def test_assemble_refusals():
    x, x0, xm, t = _window(2, 3, 8, seed=5)
    masks = _masks(2, 3, "mixed")
    for kw in (dict(Kpad=64, frame_list=[4, 0], scalars_only=1), dict(Kpad=32), dict(Kpad=96), dict(Kpad=512), dict(Kpad=0)):
        out = _assemble(x, x0, xm, masks, t, 0, 0, kw.pop("Kpad"), expect_refusal=True, **kw)
        assert all((o == SENT).all() for o in out)


# ================================================================================================ posenc_add
@pytest.mark.parametrize("use_P,use_femb", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("nfr,HW,C", [(3, 16, 32), (2, 9, 128), (5, 64, 64)])
def test_posenc_add_is_exact(nfr, HW, C, use_P, use_femb):
    x = rnd(nfr, HW, C, seed=1)
    P = (torch.arange(HW * C, dtype=torch.float32).view(HW, C) + 1) / 64 if use_P else None          # distinct per (pixel, channel)
    femb = -(torch.arange(nfr * C, dtype=torch.float32).view(nfr, C) + 1) * 8 if use_femb else None  # distinct per (frame, channel)
    y = torch.full((nfr, HW, C), SENT, device="cuda")
    bufs = [dev(x), None if P is None else dev(P), None if femb is None else dev(femb)]
    op("vd_op_posenc_add", *(_lib.ptr(b) for b in bufs), nfr, HW, C, _lib.ptr(y))
    assert torch.equal(y.cpu(), R.posenc_ref(x, P, femb))


# ================================================================================================ row moves
def _bits(*shape, seed):
    """Random bit patterns as float32 (NaNs and denormals among them): a move must keep every bit."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2 ** 31, 2 ** 31, shape, generator=g, dtype=torch.int64).to(torch.int32)


@pytest.mark.parametrize("row_floats", [4, 1028, 4100 * 4])                 # 4100 quads per row: past one pass of the 5 x 256 threads
def test_move_rows_gather_then_scatter(row_floats):
    nrows, rows = 7, [5, 0, 3]
    src = dev(_bits(nrows, row_floats, seed=row_floats))
    li = dev(torch.tensor(rows, dtype=torch.int32))
    sent = torch.iinfo(torch.int32).max - 12345

    def move(scatter, s, n, d):
        op("vd_op_move_rows", scatter, _lib.ptr(s), _lib.ptr(li), n, row_floats, _lib.ptr(d))

    compact = torch.full((len(rows) + 1, row_floats), sent, dtype=torch.int32, device="cuda")
    move(0, src, len(rows), compact)
    assert torch.equal(compact[:3], src[rows]) and (compact[3] == sent).all()
    back = torch.full((nrows, row_floats), sent, dtype=torch.int32, device="cuda")
    move(1, compact, len(rows), back)
    others = [r for r in range(nrows) if r not in rows]
    assert torch.equal(back[rows], src[rows]) and (back[others] == sent).all()
    for scatter in (0, 1):                                                   # n = 0: nothing moves
        move(scatter, src, 0, back)
        assert torch.equal(back[rows], src[rows]) and (back[others] == sent).all()


def test_move_rows_refuses_rows_that_are_not_whole_quads():
    src, dst = dev(torch.zeros(4, 6)), torch.full((4, 6), SENT, device="cuda")
    li = dev(torch.tensor([1, 2], dtype=torch.int32))
    for scatter in (0, 1):
        assert refused("vd_op_move_rows", scatter, _lib.ptr(src), _lib.ptr(li), 2, 6, _lib.ptr(dst))
    assert (dst == SENT).all()


@pytest.mark.parametrize("C", [32, 384])
@pytest.mark.parametrize("split", [1, 3, 8])
def test_scatter_stats_sums_in_order(split, C):
    nfr, rows = 6, [4, 1, 2]
    g = torch.Generator().manual_seed(split * 1000 + C)
    src = (torch.rand(len(rows), split, C, 2, generator=g, dtype=torch.float64) - 0.3) * 1e4
    dst0 = torch.full((nfr, C, 2), SENT, dtype=torch.float64)
    dst = dev(dst0)
    bufs = [dev(src), dev(torch.tensor(rows, dtype=torch.int32))]
    op("vd_op_scatter_stats", _lib.ptr(bufs[0]), split, C, _lib.ptr(bufs[1]), len(rows), _lib.ptr(dst))
    assert torch.equal(dst.cpu(), R.scatter_stats_ref(src, rows, dst0))      # the unlisted rows too: untouched
    op("vd_op_scatter_stats", _lib.ptr(bufs[0]), split, C, _lib.ptr(bufs[1]), 0, _lib.ptr(dst))
    assert torch.equal(dst.cpu(), R.scatter_stats_ref(src, rows, dst0))


# ================================================================================================ one engine-level case
@pytest.mark.parametrize("use_rpe_net", [False, True])
def test_engine_eps_at_exact_integer_bucket_distances(use_rpe_net):
    """The whole network with the bucket table left of its degenerate setting: frame indices whose differences include +-4 and +-8, the
    two exact-integer distances of (alpha, beta, gamma) = (2, 4, 8), centred frame encoding on."""
    cfg = {**vda.video_model_and_diffusion_defaults(),
           **dict(T=8, image_size=32, num_channels=32, num_res_blocks=1, use_rpe_net=use_rpe_net, rp_alpha=2, rp_beta=4, rp_gamma=8,
                  use_frame_encoding=True, enforce_position_invariance=True, timestep_respacing="ddim50")}
    model, diff = vda.create_video_model_and_diffusion(**{k: cfg[k] for k in vda.video_model_and_diffusion_defaults()})
    sd = synth_sd(model.param_specs())
    model.load_state_dict(sd)
    model.to("cuda").eval()
    B, T = 2, 8
    fidx = torch.tensor([[0, 1, 2, 4, 8, 9, 16, 17], [17, 16, 9, 8, 4, 2, 1, 0]])
    d = set(R.distances(fidx).flatten().tolist())
    assert {4, -4, 8, -8} <= d
    g = torch.Generator().manual_seed(8)
    x0 = torch.rand(B, T, 3, 32, 32, generator=g) * 2 - 1
    x = torch.randn(B, T, 3, 32, 32, generator=g)
    obs = torch.zeros(B, T, 1, 1, 1)
    obs[:, :3] = 1
    kw = dict(frame_indices=fidx, x0=x0, obs_mask=obs, latent_mask=1 - obs, kinda_marg_mask=torch.zeros(B, T, 1, 1, 1))
    t_model = torch.tensor([620.0, 40.0])
    want = UNetRef(cfg, sd)(x, t_model, **kw)
    got = model(x.cuda(), t_model.cuda(), **{k: v.cuda() for k, v in kw.items()}, x_t_minus_1=x0.cuda(), observed_frames="x_0")
    got = got[0] if isinstance(got, tuple) else got
    err = close(got.cpu(), want)
    print(f"engine eps, use_rpe_net={use_rpe_net}, (2, 4, 8), d = +-4, +-8: max |err| = {err:.3e}")
