"""CPU: the references of tests/test_gpu_cond_path.py (tests/cond_path_restated.py) checked on their own, so that a GPU failure
there points at a kernel and not at the yardstick."""
import torch

import cond_path_restated as R


def test_bucket_reference_reproduces_the_exact_integer_distances():
    """At the listed distances -- and at no other integer distance up to gamma + 3 -- the value RPE.get_bucket_ids truncates is an
    exact integer, in float32 and in float64; rpe_R's table branch selects that bucket, and its wrapped mirror for -d."""
    for (al, be, ga), want in R.EXACT_INTEGER_DISTANCES.items():
        found = {}
        for d in range(al + 1, ga + 4):
            v32, v64 = R.bucket_value(d, al, be, ga, torch.float32), R.bucket_value(d, al, be, ga, torch.float64)
            if v32 == round(v32) or v64 == round(v64):
                assert v32 == v64, (al, be, ga, d, v32, v64)
                found[d] = int(v32)
        assert found == want, ((al, be, ga), found)
        ds = torch.tensor(sorted(want)).view(1, 1, -1)
        assert R.bucket_rows_ref(ds, al, be, ga).flatten().tolist() == [want[d] for d in sorted(want)]
        assert R.bucket_rows_ref(-ds, al, be, ga).flatten().tolist() == [2 * be + 1 - want[d] for d in sorted(want)]


def test_bucket_reference_small_distances_and_clamp():
    al, be, ga = 2, 4, 8
    d = torch.tensor([[[0, 1, 2, -1, -2, 3, 9, 11, -9]]])
    # |d| <= alpha: the distance itself; 3 -> int(2 + log(1.5) / log(4) * 2) = 2; beyond gamma: beta; negatives wrap by 2 beta + 1 = 9
    assert R.bucket_rows_ref(d, al, be, ga).flatten().tolist() == [0, 1, 2, 8, 7, 2, 4, 4, 5]
    tab = torch.arange(9 * 5, dtype=torch.float32).view(9, 5)
    assert torch.equal(R.bucket_gather_ref(tab, d, al, be, ga)[0, 0], tab[[0, 1, 2, 8, 7, 2, 4, 4, 5]])


def test_covering_rows_contain_every_distance_within_a_window():
    for al, be, ga in list(R.EXACT_INTEGER_DISTANCES) + [R.DEGENERATE]:
        fidx = R.covering_fidx(ga)
        assert fidx.shape[1] <= R.WINDOW
        assert set(range(-(ga + 3), ga + 4)) <= set(R.distances(fidx).flatten().tolist())


def test_unfold_reordering_on_a_hand_built_example():
    """3 x 3 image, 2 channels, value 10 c + 3 y + x + 1: row (pixel) p, column k = tap * 2 + channel, taps row-major from (-1, -1)."""
    img = torch.tensor([[[1., 2, 3], [4, 5, 6], [7, 8, 9]], [[11., 12, 13], [14, 15, 16], [17, 18, 19]]])[None]
    cols = R.im2col_k_tap_major(img, 32)
    assert cols.shape == (1, 9, 32)
    centre = [1, 11, 2, 12, 3, 13, 4, 14, 5, 15, 6, 16, 7, 17, 8, 18, 9, 19]
    assert cols[0, 4].tolist() == centre + [0.0] * 14
    corner = [0, 0, 0, 0, 0, 0, 0, 0, 1, 11, 2, 12, 0, 0, 4, 14, 5, 15]       # pixel (0, 0): the top row and left column of taps are padding
    assert cols[0, 0].tolist() == corner + [0.0] * 14
    last = [5, 15, 6, 16, 0, 0, 8, 18, 9, 19, 0, 0, 0, 0, 0, 0, 0, 0]         # pixel (2, 2)
    assert cols[0, 8].tolist() == last + [0.0] * 14


def test_assemble_reference_by_hand():
    """One item, frames [observed, latent, kinda-marginalised, in no mask], 1 x 1 images: the centre tap carries the stem channels."""
    B, T = 1, 4
    x = torch.tensor([1., 2, 3, 4]).view(B, T, 1, 1, 1).expand(B, T, 3, 1, 1).contiguous()
    x0, xm = x + 10, x + 20
    m = lambda *v: torch.tensor(v, dtype=torch.float32).view(B, T, 1, 1, 1)  # noqa: E731
    obs, lat, km = m(1, 0, 0, 0), m(0, 1, 0, 0), m(0, 0, 1, 0)
    t = torch.tensor([50.])
    cols, tf, am = R.assemble_ref(x, x0, xm, obs, lat, km, t, 0, 0, 64)         # 'channel', observed_frames 'x_0'
    assert cols.shape == (4, 1, 64) and am.tolist() == [1, 1, 1, 0] and tf.tolist() == [0, 50, 50, 50]
    assert cols[:, 0, 4 * 5:4 * 5 + 5].tolist() == [[11, 11, 11, 1, 0], [2, 2, 2, 0, 0], [0, 0, 0, 0, 1], [4, 4, 4, 0, 0]]
    assert cols[:, 0, :20].abs().sum() == 0 and cols[:, 0, 25:].abs().sum() == 0
    cols, tf, _ = R.assemble_ref(x, x0, xm, obs, lat, km, t, 0, 2, 64)           # observed_frames 'x_t_minus_1'
    assert cols[0, 0, 20:25].tolist() == [21, 21, 21, 1, 0] and tf.tolist() == [49, 50, 50, 50]
    cols, tf, _ = R.assemble_ref(x, x0, xm, obs, lat, km, t, 1, 1, 64)           # 'duplicate': x0 * obs whatever the mode
    assert cols[:, 0, 4 * 6:4 * 6 + 6].tolist() == [[0, 0, 0, 11, 11, 11], [2, 2, 2, 0, 0, 0], [0, 0, 0, 0, 0, 0], [4, 4, 4, 0, 0, 0]]
    assert tf.tolist() == [50] * 4
    cols, tf, _ = R.assemble_ref(x, x0, xm, obs, lat, km, t, 2, 0, 64)           # 't=0': x itself; an observed frame puts the item at -1
    assert cols[:, 0, 4 * 3:4 * 3 + 3].tolist() == [[1] * 3, [2] * 3, [3] * 3, [4] * 3] and tf.tolist() == [-1] * 4
    _, tf, _ = R.assemble_ref(x, x0, xm, 0 * obs, lat, km, t, 2, 0, 64)
    assert tf.tolist() == [50] * 4


def test_rpe_hidden_reference_by_hand():
    te = torch.tensor([[[0.5, -1.0]]]).expand(1, 2, 2).contiguous()               # B = 1, T = 2, C = 2
    W = torch.tensor([[1., 0, 0], [0, 2., 3.]])
    b = torch.tensor([0.25, 0.])
    fidx = torch.tensor([[7, 4]])
    e = R.rpe_hidden_ref(te, W, b, fidx)
    silu = lambda v: v / (1 + torch.exp(torch.tensor(-v, dtype=torch.float64)))  # noqa: E731
    l4 = torch.log(torch.tensor(4., dtype=torch.float64)).item()
    want = torch.stack([torch.stack([torch.stack([silu(0.75), silu(2.0)]), torch.stack([silu(0.75 + l4), silu(-1.0)])]),
                        torch.stack([torch.stack([silu(0.75), silu(-1 + 2 * l4)]), torch.stack([silu(0.75), silu(2.0)])])])[None]
    assert e.dtype == torch.float64 and torch.allclose(e, want, rtol=0, atol=1e-15)


def test_embedding_references():
    f = R.freq_table(4, 10000)
    assert f[0] == 1 and abs(f[2].item() - 0.01) < 1e-9
    e = R.sinus_ref(torch.tensor([0., 2.]), f, 9)
    assert e.shape == (2, 9) and e[0].tolist() == [1] * 4 + [0] * 5 and e[1, 8] == 0
    assert abs(e[1, 0].item() - torch.cos(torch.tensor(2., dtype=torch.float64)).item()) == 0
    fi = torch.tensor([[3, 5, 10], [100000, 0, 50000]])
    assert R.frame_t_ref(fi, 0).tolist() == [[3, 5, 10], [100000, 0, 50000]]
    assert R.frame_t_ref(fi, 1).tolist() == [[-3, -1, 4], [50000, -50000, 0]]


def test_posenc_and_scatter_stats_references():
    x, P, fe = torch.ones(2, 3, 4), torch.arange(12.).view(3, 4), torch.tensor([[100.] * 4, [200.] * 4])
    assert torch.equal(R.posenc_ref(x, None, None), x)
    assert R.posenc_ref(x, P, fe)[1, 2].tolist() == [209, 210, 211, 212]
    src = torch.arange(2 * 3 * 2 * 2, dtype=torch.float64).view(2, 3, 2, 2)
    out = R.scatter_stats_ref(src, [2, 0], torch.full((3, 2, 2), -1., dtype=torch.float64))
    assert out[2].flatten().tolist() == [12, 15, 18, 21] and out[0].flatten().tolist() == [48, 51, 54, 57] and (out[1] == -1).all()
