"""tests/pool_ref.py (the float64 reference of seg_pool2d_* / seg_pad2d_*) pinned
by hand-derived answers and, on tie-free inputs, by torch's own pooling."""
import torch
import torch.nn.functional as F

from tests import pool_ref as R


def test_same_geometry_known_answers():
    # in 5, k 3, s 2 SAME: out = ceil(5 / 2) = 3, total pad = (3 - 1) * 2 + 3 - 5 = 2 -> 1 / 1
    assert R.geometry(5, 3, 2, "SAME") == (3, 1, 1)
    # in 4: out = 2, total = (2 - 1) * 2 + 3 - 4 = 1 -> 0 before, 1 after
    assert R.geometry(4, 3, 2, "SAME") == (2, 0, 1)
    assert R.geometry(9, 3, 2, "VALID") == (4, 0, 0)
    assert R.geometry(11, 3, 2, "VALID") == (5, 0, 0)
    assert R.geometry(7, 1, 2, "VALID") == (4, 0, 0) == R.geometry(7, 1, 2, "SAME")    # the subsample: ceil(7 / 2)
    assert R.geometry(7, 2, 3, "VALID") == (2, 0, 0)
    # the pyramid on the 5 x 18 encoder map
    assert [R.out_shape((1, 5, 18, 8), k, k, "VALID")[1:3] for k in ((5, 18), (3, 9), (2, 6), (1, 3))] == \
        [(1, 1), (1, 2), (2, 3), (5, 6)]


def test_max_pool_tie_one_input_wins_two_windows():
    """5 x 1 column, 3 x 1 window, stride 2 VALID: windows rows {0,1,2} and
    {2,3,4}.  x = [1, 0, 7, 7, 0]: window 0's maximum 7 is row 2 (position 2);
    window 1 holds 7 at rows 2 and 3 -- the first (position 0, row 2) wins.
    Row 2 therefore gets both gradients, row 3 none."""
    x = torch.tensor([1.0, 0.0, 7.0, 7.0, 0.0]).view(1, 5, 1, 1)
    y, idx = R.max_pool(x, (3, 1), (2, 1), "VALID")
    assert y.view(-1).tolist() == [7.0, 7.0]
    assert idx.view(-1).tolist() == [2, 0]
    dx = R.max_pool_grad(idx, torch.tensor([10.0, 100.0]).view(1, 2, 1, 1), x.shape, (3, 1), (2, 1), "VALID")
    assert dx.view(-1).tolist() == [0.0, 0.0, 110.0, 0.0, 0.0]


def test_max_pool_3x3_stride2_tie_in_two_dimensions():
    """5 x 5 of zeros with a single 1 at (2, 2), 3 x 3 / 2 VALID: the centre is
    in all four windows and is each one's only maximum -- positions 8, 6, 2, 0 --
    so it collects all four gradients.  An all-equal window picks position 0."""
    x = torch.zeros(1, 5, 5, 1)
    x[0, 2, 2, 0] = 1.0
    y, idx = R.max_pool(x, (3, 3), (2, 2), "VALID")
    assert y.view(-1).tolist() == [1.0] * 4
    assert idx.view(-1).tolist() == [8, 6, 2, 0]
    dx = R.max_pool_grad(idx, torch.tensor([1.0, 2.0, 4.0, 8.0]).view(1, 2, 2, 1), x.shape, (3, 3), (2, 2), "VALID")
    assert dx[0, 2, 2, 0].item() == 15.0 and dx.sum().item() == 15.0
    _, idx0 = R.max_pool(torch.zeros(1, 5, 5, 1), (3, 3), (2, 2), "VALID")
    assert idx0.view(-1).tolist() == [0] * 4


def test_same_padding_never_wins_and_positions_count_the_padding():
    """4 x 4 of -1, 3 x 3 / 2 SAME (pad 0 before, 1 after): the zero padding
    must not beat -1.  5 x 5 SAME pads 1 before: the corner window's first
    in-image element is window position 1 * 3 + 1 = 4."""
    y, _ = R.max_pool(-torch.ones(1, 4, 4, 1), (3, 3), (2, 2), "SAME")
    assert y.view(-1).tolist() == [-1.0] * 4
    _, idx = R.max_pool(-torch.ones(1, 5, 5, 1), (3, 3), (2, 2), "SAME")
    assert idx[0, 0, 0, 0].item() == 4 and idx[0, 1, 1, 0].item() == 0


def test_avg_pool_same_corner_divides_by_in_image_count():
    """5 x 5 of ones, 3 x 3 / 2 SAME (pads 1 / 1): the corner window holds 4
    in-image elements, an edge window 6, the centre 9 -- every average is 1,
    and the gradient of a corner output is dy / 4 (not / 9)."""
    x = torch.ones(1, 5, 5, 1)
    assert torch.equal(R.avg_pool(x, (3, 3), (2, 2), "SAME"), torch.ones(1, 3, 3, 1, dtype=torch.float64))
    x[0, 0, 0, 0] = 5.0
    assert R.avg_pool(x, (3, 3), (2, 2), "SAME")[0, 0, 0, 0].item() == (5.0 + 3.0) / 4.0
    dy = torch.zeros(1, 3, 3, 1)
    dy[0, 0, 0, 0] = 1.0
    dx = R.avg_pool_grad(dy, x.shape, (3, 3), (2, 2), "SAME")
    assert dx[0, :2, :2, 0].tolist() == [[0.25, 0.25], [0.25, 0.25]] and dx.sum().item() == 1.0
    dy = torch.zeros(1, 3, 3, 1)
    dy[0, 0, 1, 0] = 1.0                                        # an edge window: 2 rows x 3 columns
    assert R.avg_pool_grad(dy, x.shape, (3, 3), (2, 2), "SAME")[0, 0, 1, 0].item() == 1.0 / 6.0


def test_gaps_and_leftovers_get_no_gradient():
    dx = R.avg_pool_grad(torch.ones(1, 2, 2, 1), (1, 7, 7, 1), (2, 2), (3, 3), "VALID")
    want = torch.zeros(7, 7, dtype=torch.float64)
    for a in (0, 1, 3, 4):
        for b in (0, 1, 3, 4):
            want[a, b] = 0.25
    assert torch.equal(dx[0, :, :, 0], want)
    assert not R.overlap((1, 7, 7, 1), (2, 2), (3, 3), "VALID").any()
    ov = R.overlap((1, 9, 11, 1), (3, 3), (2, 2), "VALID")
    assert ov[2, 2] and ov[1, 2] and not ov[0, 0] and not ov[1, 1]
    # 3 / 2 VALID over 10 columns: windows end at column 8, column 9 is a leftover
    dx = R.avg_pool_grad(torch.ones(1, 4, 4, 1), (1, 9, 10, 1), (3, 3), (2, 2), "VALID")
    assert not dx[0, :, 9, 0].any() and dx[0, :, 8, 0].all()


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def test_against_torch_on_tie_free_inputs():
    g = torch.Generator().manual_seed(3)
    for (N, H, W, C, kh, kw, sh, sw, padding) in [(2, 9, 11, 3, 3, 3, 2, 2, "VALID"), (1, 8, 8, 2, 3, 3, 2, 2, "SAME"),
                                                   (1, 5, 18, 2, 2, 6, 2, 6, "VALID"), (2, 7, 9, 2, 1, 1, 2, 2, "VALID"),
                                                   (1, 7, 7, 2, 2, 2, 3, 3, "VALID"), (1, 5, 7, 2, 3, 2, 2, 1, "SAME")]:
        x = torch.randperm(N * H * W * C, generator=g).double().view(N, H, W, C)     # all distinct
        _, pt, pb = R.geometry(H, kh, sh, padding)
        _, pl, pr = R.geometry(W, kw, sw, padding)
        xt = x.clone().requires_grad_(True)
        ym = F.max_pool2d(F.pad(_nchw(xt), (pl, pr, pt, pb), value=float("-inf")), (kh, kw), (sh, sw))
        y, idx = R.max_pool(x, (kh, kw), (sh, sw), padding)
        assert torch.equal(_nchw(y), ym.detach())
        dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
        ym.backward(_nchw(dy))
        assert torch.allclose(R.max_pool_grad(idx, dy, x.shape, (kh, kw), (sh, sw), padding), xt.grad, rtol=0, atol=1e-12)
        # average: torch divides by the in-image count with count_include_pad=False
        # only for its own padding, which must be symmetric: pad the larger side
        # explicitly, pool the padded tensor with a mask-based count instead
        xa = x.clone().requires_grad_(True)
        ones = torch.ones_like(x)
        num = F.avg_pool2d(F.pad(_nchw(xa), (pl, pr, pt, pb)), (kh, kw), (sh, sw), divisor_override=1)
        cnt = F.avg_pool2d(F.pad(_nchw(ones), (pl, pr, pt, pb)), (kh, kw), (sh, sw), divisor_override=1)
        ya = num / cnt
        assert torch.allclose(_nchw(R.avg_pool(x, (kh, kw), (sh, sw), padding)), ya.detach(), rtol=1e-13, atol=0)
        ya.backward(_nchw(dy))
        assert torch.allclose(R.avg_pool_grad(dy, x.shape, (kh, kw), (sh, sw), padding), xa.grad, rtol=1e-13, atol=1e-13)
        if pt == pb and pl == pr:
            yc = F.avg_pool2d(_nchw(x), (kh, kw), (sh, sw), padding=(pt, pl), count_include_pad=False)
            assert torch.allclose(_nchw(R.avg_pool(x, (kh, kw), (sh, sw), padding)), yc, rtol=1e-13, atol=0)
        # the autograd wrappers route to the same gradients
        xw = x.clone().requires_grad_(True)
        (R.max_pool_ad(xw, (kh, kw), (sh, sw), padding) * dy).sum().backward()
        assert torch.allclose(xw.grad, xt.grad, rtol=0, atol=1e-12)


def test_pad_and_crop():
    x = torch.arange(2 * 2 * 3 * 1, dtype=torch.float64).view(2, 2, 3, 1) + 1
    y = R.pad(x, (0, 2, 1, 0))
    assert y.shape == (2, 4, 4, 1)
    assert y[0, :, :, 0].tolist() == [[0, 1, 2, 3], [0, 4, 5, 6], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert torch.equal(R.crop(y, (0, 2, 1, 0)), x)
    assert torch.equal(_nchw(R.pad(x, (3, 3, 3, 3))), F.pad(_nchw(x), (3, 3, 3, 3)))
    xg = x.clone().requires_grad_(True)
    (R.pad_ad(xg, (1, 1, 1, 1)) * 2.0).sum().backward()
    assert torch.equal(xg.grad, torch.full_like(x, 2.0))
