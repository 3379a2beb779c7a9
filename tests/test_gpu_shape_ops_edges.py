"""Edge-case parity of the shape-changing kernels in csrc/eltwise.hip -- the
four MaxPool kernels, the two AvgPool kernels, the four bilinear-resize
kernels, the four concat kernels and dropout_k / dropout_ch_k -- through the
wrappers of ops.py.  (The channel reductions -- bias_relu_bwd, BatchNorm --
are in test_gpu_reduce_ops_edges.py.)

Every reference is computed on the CPU in float64 from the inputs as the
device sees them (`rnd`), with oracle/tf1_ops.py where it has the op.  Results
whose arithmetic is one IEEE operation sequence are compared bit for bit; the
others element by element against a bound derived next to the check, with
U = 2^-24 (fp32 arithmetic) and U_DT (one rounding into the storage format,
which may be a double rounding).  Outputs are prefilled with NaN and views lie
in buffers filled with 50s: what must be written is, nothing else changes.

Grid-stride cases: seg_grid_1d(n, 256) launches min(16384, ceil(n / 256))
blocks, the lane-geometry kernels min(16384, ceil(P / rows)); each large shape
below is the smallest that sends the kernel's loop into a second pass, with
the derivation next to it.  Their inputs are a small block tiled on the
device and their expected outputs the small reference tiled the same way.
"""
import numpy as np
import pytest
import torch

from oracle import tf1_ops as tf
from semanticsegmentation_tensorflow_amd import ops
from tests.gpu_utils import (U, assert_bits_equal, assert_surroundings, assert_within, nan_like_view,
                             randn_normal, rnd, storage_bound, tile_rows, to_dev)
from tests.test_gpu_eltwise_edges import _slice_view
from tests.test_gpu_ops_r2 import _np_uniform_vec

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DT_IDS = ["f32", "bf16", "f16"]
EINVAL = r"invalid argument \(status 1\)"
NAN = float("nan")
INF = float("inf")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _int_view(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _dev_bits_equal(got, ref, what):
    """assert_bits_equal for large device tensors without NaNs (compared on the device)."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    assert not bool(torch.isnan(got).any()), f"{what}: NaN left"
    ne = _int_view(got.contiguous()) != _int_view(ref.contiguous())
    n = int(ne.sum())
    assert n == 0, f"{what}: {n} of {got.numel()} elements differ, first at {int(ne.reshape(-1).nonzero()[0])}"


# ---------------------------------------------------------------------------
# A. 2x2 pooling
# ---------------------------------------------------------------------------
# one window; one window + odd tails on both axes; a single row / column of
# windows with a tail; CK = C / EPC = 5 (16-bit) or 10 (fp32); CK = 9 / 18
POOL_SHAPES = [(1, 2, 2, 8), (2, 3, 3, 8), (1, 2, 7, 24), (1, 7, 2, 24), (3, 6, 10, 40), (2, 5, 9, 72)]
POOL_IDS = ["x".join(map(str, s)) for s in POOL_SHAPES]
VIEWS = ["dense", "x", "y", "dy", "dx", "all"]
_EXTRA = {"x": 16, "y": 24, "dy": 32, "dx": 40}       # each view its own pixel stride


def _place(t64, dtype, dev, name, view):
    if view in (name, "all"):
        return _slice_view(t64, dtype, dev, extra=_EXTRA[name])
    return to_dev(t64, dtype, dev)


def _out(shape, dtype, dev, name, view):
    return _place(torch.full(shape, NAN, dtype=torch.float64), dtype, dev, name, view)


def _around(*ts):
    for t in ts:
        if t._base is not None:
            assert_surroundings(t)


def _pool_specials(dtype):
    """Window contents (row-major q = 0..3) placed by hand; s is fp16's smallest
    subnormal (a normal number in bf16 / fp32)."""
    big, s = torch.finfo(dtype).max, 2.0 ** -24
    return [(0.0, -0.0, -1.0, -1.0),          # +0 before -0: the first wins, y = +0
            (-0.0, 0.0, -1.0, -2.0),          # the reverse: y = -0
            (1.0, INF, INF, 2.0),             # first of two +inf
            (-INF, -INF, -INF, -INF),         # four -inf: q = 0, y = -inf
            (1.0, big, big, -big),            # largest finite, tied
            (0.0, s, 3 * s, -s),              # fp16 subnormals: q = 2
            (2.5, 2.5, 2.5, 2.5),             # four-way tie
            (-1.0, -2.0, -0.5, -3.0),         # relu_mask: negative max
            (0.0, -1.0, -0.0, -2.0),          # relu_mask: max +0
            (-0.0, -1.0, -2.0, -3.0),         # relu_mask: max -0
            (-1.0, s, -2.0, 0.0),             # relu_mask: tiny positive max, kept
            (-INF, INF, 1.0, INF)]


def _pool_input(shape, dtype, seed, specials=True):
    N, H, W, C = shape
    OH, OW = H // 2, W // 2
    x = randn_normal(shape, _gen(seed), dtype)
    if specials:
        pats = _pool_specials(dtype)
        for i in range(min(len(pats), N * OH * OW * C)):
            c, t = i % C, i // C
            ow, t = t % OW, t // OW
            oh, n = t % OH, t // OH
            for q in range(4):
                x[n, 2 * oh + q // 2, 2 * ow + q % 2, c] = pats[i][q]
    return rnd(x, dtype)


def _maxpool_ref(x, dy, relu_mask):
    """(y, first-max position per pooled element, dx) from the oracle's MaxPool
    and its TF1 tie-routing gradient; relu_mask: ReluGrad of the post-ReLU pool
    input, i.e. the gradient flows only where the window max is > 0."""
    N, H, W, C = x.shape
    OH, OW = H // 2, W // 2
    xr = x.clone().requires_grad_(True)
    y = tf.max_pool2x2(xr)
    (one,) = torch.autograd.grad(y, xr, torch.ones_like(y), retain_graph=True)
    win = one[:, :2 * OH, :2 * OW].reshape(N, OH, 2, OW, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(N, OH, OW, C, 4)
    assert bool((win.sum(-1) == 1).all())
    arg = win.argmax(-1)
    yd = y.detach()
    dyr = dy * (yd > 0) if relu_mask else dy
    (dx,) = torch.autograd.grad(y, xr, dyr)
    # the oracle's dy * 0 is -0.0 for a negative dy; MaxPoolGrad's untouched
    # and masked elements are the +0.0 of a zero-filled buffer
    return yd, arg, dx + 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=POOL_IDS)
def test_maxpool_fwd_bwd_pairs(dev, dtype, shape, view):
    """maxpool_fwd_k / maxpool_fwd_idx_k and maxpool_bwd_k / maxpool_bwd_idx_k:
    y, the switch bytes and dx bit for bit against the oracle, the two kernels
    of each pair bit for bit against each other, with and without relu_mask."""
    N, H, W, C = shape
    OH, OW = H // 2, W // 2
    x = _pool_input(shape, dtype, 1000 + H * 16 + W)
    dy = randn_normal((N, OH, OW, C), _gen(7), dtype)
    xd, dyd = _place(x, dtype, dev, "x", view), _place(dy, dtype, dev, "dy", view)
    # the x-reading gradient reads x with dx's pixel stride (segkern.h: one ldx)
    xb = _place(x, dtype, dev, "dx", view)
    y1, y2 = _out(dy.shape, dtype, dev, "y", view), _out(dy.shape, dtype, dev, "y", view)
    idx = torch.full((N, OH, OW, C), 0xFF, dtype=torch.uint8, device=dev)   # dense, row stride C
    ops.maxpool2x2_fwd(xd, y1)
    ops.maxpool2x2_fwd_argmax(xd, y2, idx)
    for relu in (False, True):
        y_ref, arg, dx_ref = _maxpool_ref(x, dy, relu)
        dx1, dx2 = _out(shape, dtype, dev, "dx", view), _out(shape, dtype, dev, "dx", view)
        ops.maxpool2x2_bwd(xb, y1, dyd, dx1, relu_mask=relu)
        ops.maxpool2x2_bwd_argmax(idx, dyd, dx2, relu_mask=relu)
        torch.cuda.synchronize()
        assert_bits_equal(y1, y_ref.to(dtype), "maxpool y")
        assert_bits_equal(y2, y_ref.to(dtype), "maxpool (argmax form) y")
        # bits 0-1 the first max, bit 2 max > 0, upper bits 0
        want = (arg | ((y_ref > 0).long() << 2)).to(torch.uint8)
        assert torch.equal(idx.cpu(), want), f"switch bytes differ at {(idx.cpu() != want).nonzero()[:4].tolist()}"
        assert_bits_equal(dx1, dx_ref.to(dtype), f"maxpool_bwd dx relu={relu}")       # tails: +0
        assert_bits_equal(dx2, dx_ref.to(dtype), f"maxpool_bwd_argmax dx relu={relu}")
        assert_bits_equal(dx2, dx1, "argmax vs x-reading MaxPoolGrad")
        _around(xd, dyd, xb, y1, y2, dx1, dx2)
        assert_bits_equal(xd, x.to(dtype), "x untouched")
        assert_bits_equal(dyd, dy.to(dtype), "dy untouched")


def test_maxpool_second_grid_stride_pass(dev):
    """bf16, C = 8 (one chunk per pooled pixel): 2049 x 2048 = 4196352 pooled
    pixels > 16384 blocks x 256 threads = 4194304, so all four kernels loop a
    second time (H = 4098 is the first even H past 4096 at W = 4096; the
    gradient's block count (H+1)/2 x (W+1)/2 is the same).  The argmax pair
    indexes these 4.2M work items in 32-bit unsigned arithmetic."""
    dtype, (h0, w0, C) = torch.bfloat16, (6, 64, 8)
    H, W = 4098, 4096
    ry, rx = H // h0, W // w0
    assert ry * h0 == H and rx * w0 == W and (H // 2) * (W // 2) > 16384 * 256 >= (H // 2 - 1) * (W // 2)
    x0 = _pool_input((1, h0, w0, C), dtype, 31)
    dy0 = randn_normal((1, h0 // 2, w0 // 2, C), _gen(32), dtype)
    x = x0.to(dtype).to(dev).repeat(1, ry, rx, 1)
    dy = dy0.to(dtype).to(dev).repeat(1, ry, rx, 1)
    y1, y2 = torch.full_like(dy, NAN), torch.full_like(dy, NAN)
    idx = torch.full(dy.shape, 0xFF, dtype=torch.uint8, device=dev)
    dx1, dx2 = torch.full_like(x, NAN), torch.full_like(x, NAN)
    ops.maxpool2x2_fwd(x, y1)
    ops.maxpool2x2_fwd_argmax(x, y2, idx)
    ops.maxpool2x2_bwd(x, y1, dy, dx1, relu_mask=True)
    ops.maxpool2x2_bwd_argmax(idx, dy, dx2, relu_mask=True)
    torch.cuda.synchronize()
    y_ref, arg, dx_ref = _maxpool_ref(x0, dy0, True)
    want_y = y_ref.to(dtype).to(dev).repeat(1, ry, rx, 1)
    _dev_bits_equal(y1, want_y, "maxpool y, tiled")
    _dev_bits_equal(y2, want_y, "maxpool (argmax form) y, tiled")
    want_idx = (arg | ((y_ref > 0).long() << 2)).to(torch.uint8).to(dev).repeat(1, ry, rx, 1)
    assert torch.equal(idx, want_idx)
    want_dx = dx_ref.to(dtype).to(dev).repeat(1, ry, rx, 1)
    _dev_bits_equal(dx1, want_dx, "maxpool_bwd dx, tiled")
    _dev_bits_equal(dx2, want_dx, "maxpool_bwd_argmax dx, tiled")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=POOL_IDS)
def test_avgpool_fwd_bwd(dev, dtype, shape, view):
    N, H, W, C = shape
    OH, OW = H // 2, W // 2
    x = _pool_input(shape, dtype, 2000 + H * 16 + W, specials=False)
    xi = torch.randint(-8, 9, shape, generator=_gen(5)).double()        # exact: |sum| <= 32, quarter steps
    dy = randn_normal((N, OH, OW, C), _gen(8), dtype)
    for src, exact in ((x, False), (xi, True)):
        xd = _place(src, dtype, dev, "x", view)
        y = _out(dy.shape, dtype, dev, "y", view)
        ops.avgpool2x2_fwd(xd, y)
        torch.cuda.synchronize()
        ref = tf.avg_pool2x2(src)
        if exact:       # every step exact in fp32 and the mean representable in the dtype
            assert_bits_equal(y, ref.to(dtype), "avgpool of small integers")
        else:
            # ((a + b) + (c + d)) * 0.25: two levels of additions (each <= U relative to the
            # partial sums, bounded by sum |.|) and an exact scale: 3 U 0.25 (|a|+|b|+|c|+|d|)
            # = 3 U avg_pool(|x|); then the storage rounding
            assert not bool(torch.isnan(y).any())
            assert_within(y.double().cpu(), ref, storage_bound(ref, dtype, 3 * U * tf.avg_pool2x2(src.abs())),
                          "avgpool y")
        _around(xd, y)
    dyd = _place(dy, dtype, dev, "dy", view)
    dx = _out(shape, dtype, dev, "dx", view)
    ops.avgpool2x2_bwd(dyd, dx)
    torch.cuda.synchronize()
    # one exact fp32 scale by 0.25 (inputs >= 2^-6 in magnitude: no fp16 subnormal result)
    q = (dy.to(dtype).float() * 0.25).to(dtype)
    want = torch.zeros(shape, dtype=dtype)                              # zeros in the odd tails
    want[:, :2 * OH, :2 * OW] = q.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    assert_bits_equal(dx, want, "avgpool dx")
    _around(dyd, dx)


def test_avgpool_second_grid_stride_pass(dev):
    """bf16, C = 8: the same 4098 x 4096 input as the MaxPool case (2049 x 2048
    pooled pixels > 16384 x 256) for avgpool_fwd_k and avgpool_bwd_k."""
    dtype, (h0, w0, C) = torch.bfloat16, (6, 64, 8)
    H, W = 4098, 4096
    ry, rx = H // h0, W // w0
    x0 = torch.randint(-8, 9, (1, h0, w0, C), generator=_gen(41)).double()
    dy0 = randn_normal((1, h0 // 2, w0 // 2, C), _gen(42), dtype)
    x = x0.to(dtype).to(dev).repeat(1, ry, rx, 1)
    dy = dy0.to(dtype).to(dev).repeat(1, ry, rx, 1)
    y, dx = torch.full_like(dy, NAN), torch.full_like(x, NAN)
    ops.avgpool2x2_fwd(x, y)
    ops.avgpool2x2_bwd(dy, dx)
    torch.cuda.synchronize()
    _dev_bits_equal(y, tf.avg_pool2x2(x0).to(dtype).to(dev).repeat(1, ry, rx, 1), "avgpool y, tiled")
    q = (dy0.to(dtype).float() * 0.25).to(dtype).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    _dev_bits_equal(dx, q.to(dev).repeat(1, ry, rx, 1), "avgpool dx, tiled")


@pytest.mark.parametrize("case", ["H1", "W1", "C12", "stride"])
def test_pooling_rejections(dev, case):
    """H = 1, W = 1, C = 12 and a pixel stride that is no multiple of 8: every
    launcher returns SEG_EINVAL before any launch (buffers in bounds anyway)."""
    N, H, W, C = {"H1": (1, 1, 4, 8), "W1": (1, 4, 1, 8), "C12": (1, 4, 4, 12), "stride": (1, 4, 4, 8)}[case]
    dt = torch.float32
    full = torch.ones(N, H, W, 12 if case == "stride" else C, dtype=dt, device=dev)
    x = full[..., :C]
    small = torch.full((N, max(H // 2, 1), max(W // 2, 1), 12 if case == "stride" else C), NAN, dtype=dt, device=dev)
    y = small[..., :C]
    dx = torch.full_like(full, NAN)[..., :C]
    idx = torch.full((N, max(H // 2, 1), max(W // 2, 1), C), 0xFF, dtype=torch.uint8, device=dev)
    dy = torch.ones_like(small)[..., :C]
    calls = [lambda: ops.maxpool2x2_fwd(x, y), lambda: ops.maxpool2x2_fwd_argmax(x, y, idx),
             lambda: ops.maxpool2x2_bwd(x, y, dy, dx), lambda: ops.maxpool2x2_bwd_argmax(idx, dy, dx),
             lambda: ops.avgpool2x2_fwd(x, y), lambda: ops.avgpool2x2_bwd(dy, dx)]
    for f in calls:
        with pytest.raises(RuntimeError, match=EINVAL):
            f()
    torch.cuda.synchronize()
    assert bool(torch.isnan(small).all()) and bool(torch.isnan(dx._base if dx._base is not None else dx).all())
    assert bool((idx == 0xFF).all())


# ---------------------------------------------------------------------------
# D. resize_bilinear(align_corners=True)
# ---------------------------------------------------------------------------
def _lerp_f32(n_in, n_out):
    """TF's float32 position arithmetic (resize_bilinear's CPU kernel): scale =
    float32(n_in - 1) / float32(n_out - 1), src = float32(o) * scale, then
    floor and fraction in float32 (the subtraction is exact)."""
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    src = np.arange(n_out).astype(np.float32) * scale
    assert src.dtype == np.float32
    lo = np.floor(src)
    frac = (src - lo).astype(np.float64)
    lo = lo.astype(np.int64)
    hi = np.minimum(lo + 1, n_in - 1)
    return torch.from_numpy(lo), torch.from_numpy(hi), torch.from_numpy(frac)


def _resize_ref(x, OH, OW):
    """float64 interpolation at the float32 positions; also |tl|+|tr|+|bl|+|br|."""
    N, H, W, C = x.shape
    y0, y1, fy = _lerp_f32(H, OH)
    x0, x1, fx = _lerp_f32(W, OW)
    fy, fx = fy.view(1, OH, 1, 1), fx.view(1, 1, OW, 1)
    tl, tr = x[:, y0][:, :, x0], x[:, y0][:, :, x1]
    bl, br = x[:, y1][:, :, x0], x[:, y1][:, :, x1]
    top = tl + (tr - tl) * fx
    bot = bl + (br - bl) * fx
    return top + (bot - top) * fy, tl.abs() + tr.abs() + bl.abs() + br.abs()


def _resize_matrix(n_in, n_out):
    lo, hi, f = _lerp_f32(n_in, n_out)
    m = torch.zeros(n_in, n_out, dtype=torch.float64)
    o = torch.arange(n_out)
    m.index_put_((lo, o), 1.0 - f, accumulate=True)
    m.index_put_((hi, o), f, accumulate=True)
    return m


def _resize_grad_ref(dy, H, W):
    """The transposed interpolation with the same float32 weights: (dx, sum |w dy|,
    number of contributing output positions) per input element."""
    wy, wx = _resize_matrix(H, dy.shape[1]), _resize_matrix(W, dy.shape[2])
    dx = torch.einsum("hp,wq,npqc->nhwc", wy, wx, dy)
    mag = torch.einsum("hp,wq,npqc->nhwc", wy, wx, dy.abs())
    n = (wy != 0).sum(1).view(1, H, 1, 1) * (wx != 0).sum(1).view(1, 1, W, 1)
    return dx, mag, n.double().expand_as(dx)


def _misaligned(t):
    """The same values at a base address 8 bytes past a 16-byte boundary."""
    assert t.element_size() == 2
    flat = torch.full((t.numel() + 8,), 50.0, dtype=t.dtype, device=t.device)
    v = flat[4:4 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 8
    return v


# (H, W) -> (OH, OW)
RESIZE_GEOM = [((5, 7), (5, 7)),       # identity
               ((1, 6), (4, 9)),       # H = 1, OH > 1
               ((6, 1), (9, 4)),       # W = 1, OW > 1
               ((7, 5), (1, 1)),       # OH = OW = 1
               ((9, 6), (2, 11)),      # OH = 2 from H = 9
               ((5, 5), (9, 9)),       # exact half-step scale: positions land on integers
               ((48, 6), (384, 10)),   # inexact scale (47 / 383) down the rows
               ((6, 48), (10, 384)),   # and along a row
               ((15, 15), (4, 4))]     # downsample
RESIZE_IDS = [f"{a[0]}x{a[1]}to{b[0]}x{b[1]}" for a, b in RESIZE_GEOM]
# 8-wide kernels: C in {8, 16} at aligned bases (16-bit only); scalar kernels: C in
# {2, 3, 5}, fp32 at any C, and C = 8 at a misaligned base ("8m")
RESIZE_DT_C = [(dt, c) for dt in DTYPES for c in (8, 16, 2, 3, 5, "8m") if not (c == "8m" and dt == torch.float32)]
RESIZE_DT_C_IDS = [f"{DT_IDS[DTYPES.index(dt)]}-C{c}" for dt, c in RESIZE_DT_C]


def _check_resize(dev, dtype, hw, ohw, C, misalign=False, N=2, seed=0):
    (H, W), (OH, OW) = hw, ohw
    g = _gen(3000 + seed + H * 7 + OW)
    x = randn_normal((N, H, W, C), g, dtype)
    dy = randn_normal((N, OH, OW, C), g, dtype)
    xd, dyd = x.to(dtype).to(dev), dy.to(dtype).to(dev)
    y = torch.full((N, OH, OW, C), NAN, dtype=dtype, device=dev)
    dx = torch.full((N, H, W, C), NAN, dtype=torch.float32, device=dev)
    if misalign:
        xd, dyd, y = _misaligned(xd), _misaligned(dyd), _misaligned(y)
    ops.resize_bilinear_fwd(xd, y)
    ops.resize_bilinear_bwd(dyd, dx)
    torch.cuda.synchronize()
    ref, mag = _resize_ref(x, OH, OW)
    # lx, ly exact (float32 positions); tr - tl, the fma onto tl, the same for the bottom
    # row, bot - top and the last fma: 6 roundings, each <= U (|tl|+|tr|+|bl|+|br|) since
    # every intermediate is a convex combination of the corners or a difference of two;
    # 8 U mag leaves the slack of the rule
    worst = assert_within(y.double().cpu(), ref, storage_bound(ref, dtype, 8 * U * mag), "resize y")
    gref, gmag, n = _resize_grad_ref(dy, H, W)
    # fp32 output: 1 - l and the two fma chains (nx + ny <= n + 1 links) round each
    # product at most n + 3 times in all: (n + 3) U sum |w dy|, for any summation order
    worst_g = assert_within(dx.double().cpu(), gref, (n + 3) * U * gmag, "resize dx")
    print(f"resize {hw}->{ohw} C={C} {dtype}: worst error / bound {worst:.3f} fwd, {worst_g:.3f} bwd")
    if (H, W) == (OH, OW):
        assert_bits_equal(y, xd, "identity resize")
        assert_bits_equal(dx, dyd.float(), "identity resize gradient")


@pytest.mark.parametrize("dtype,C", RESIZE_DT_C, ids=RESIZE_DT_C_IDS)
@pytest.mark.parametrize("geom", RESIZE_GEOM, ids=RESIZE_IDS)
def test_resize_against_float32_positions(dev, dtype, geom, C):
    mis = C == "8m"
    _check_resize(dev, dtype, geom[0], geom[1], 8 if mis else C, misalign=mis)


# grid.y is capped at 64 blocks of 256 threads: a row of more than 16384 work items
# takes a second pass.  8-wide: 1040 pixels x 128 / 8 chunks = 16640; scalar: 5462
# pixels x 3 channels = 16386 (the first pixel counts past 16384 at these C).
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("C,wide", [(128, 1040), (3, 5462)], ids=["fwd8_bwd8", "scalar"])
def test_resize_rows_past_the_grid_y_cap(dev, dtype, C, wide):
    assert (wide * C // 8 if C % 8 == 0 else wide * C) > 64 * 256
    _check_resize(dev, dtype, (2, 4), (3, wide), C, N=1, seed=1)      # forward row of `wide` pixels
    _check_resize(dev, dtype, (1, wide), (2, 4), C, N=1, seed=2)      # gradient row of `wide` pixels, 2-row dy


# ---------------------------------------------------------------------------
# E. concat
# ---------------------------------------------------------------------------
def _quarters(shape, g):
    """Multiples of 0.25 in [-16, 16]: exact in bf16 / fp16 / fp32, and so are their pairwise sums."""
    return torch.randint(-64, 65, shape, generator=g).double() / 4


def _run_concat_fwd(dev, dtype, chans, nhw, ych_extra=0, views=True, P_tile=None):
    """concat_fwd of parts with `chans` valid channels; returns y (float64, CPU).
    views: parts and y are channel slices of wider buffers."""
    N, H, W = nhw
    g = _gen(4000 + len(chans) + chans[0])
    xs = [_quarters((N, H, W, c), g) for c in chans]
    total = sum(chans)
    ych = ops.round8(total) + ych_extra
    if views:
        parts = [(_slice_view(x, dtype, dev, extra=8 * (i % 3 + 1)), c) for i, (x, c) in enumerate(zip(xs, chans))]
        y = nan_like_view((N, H, W, ych), dtype, dev, lambda t: _slice_view(t, dtype, dev, extra=24))
    else:
        parts = [(to_dev(x, dtype, dev), c) for x, c in zip(xs, chans)]
        y = torch.full((N, H, W, ych), NAN, dtype=dtype, device=dev)
    ops.concat_fwd(parts, y, ych)
    torch.cuda.synchronize()
    ref = torch.zeros(N, H, W, ych, dtype=torch.float64)           # channels >= sum are written 0
    ref[..., :total] = tf.concat(xs)
    assert_bits_equal(y, ref.to(dtype), f"concat {chans[:4]}.. {dtype}")
    _around(y, *[p for p, _ in parts])
    for (p, c), x in zip(parts, xs):
        assert_bits_equal(p[..., :c], x.to(dtype), "part untouched")
    return y.double().cpu()


def _run_concat_bwd(dev, dtype, chans, acc, nhw, slack=16, views=True):
    """concat_bwd into parts prefilled with NaN (write) or old values (accumulate,
    padding channels included); returns the parts' float64 values."""
    N, H, W = nhw
    g = _gen(5000 + len(chans) + chans[0])
    total = sum(chans)
    dy = _quarters((N, H, W, total + slack), g)                      # ldy > sum: slack channels never read
    dyd = _slice_view(dy, dtype, dev, extra=32) if views else to_dev(dy, dtype, dev)
    olds, dsts = [], []
    for i, (c, a) in enumerate(zip(chans, acc)):
        cp = ops.round8(c)
        old = _quarters((N, H, W, cp), g) if a else torch.full((N, H, W, cp), NAN, dtype=torch.float64)
        olds.append(old)
        dsts.append(_slice_view(old, dtype, dev, extra=8 * (i % 3 + 1)) if views else old.to(dtype).to(dev))
    ops.concat_bwd(dyd, [(d, c, a) for d, c, a in zip(dsts, chans, acc)])
    torch.cuda.synchronize()
    off, out = 0, []
    for d, c, a, old in zip(dsts, chans, acc, olds):
        want = old.to(dtype).clone()
        piece = dy[..., off:off + c].to(dtype)
        if a:       # valid channels: one fp32 addition, rounded; padding channels keep their bits
            want[..., :c] = (want[..., :c].float() + piece.float()).to(dtype)
        else:       # valid channels the gradient, padding channels +0
            want[..., :c] = piece
            want[..., c:] = 0
        assert_bits_equal(d, want, f"concat_bwd part of {c} at {off} acc={a} {dtype}")
        out.append(d.double().cpu())
        off += c
    _around(dyd, *dsts)
    assert_bits_equal(dyd[..., :total + slack], dy.to(dtype), "dy untouched")
    return out


# aligned offsets (bf16: concat_*_fast_k, fp16 / fp32: the element kernels) and unaligned
# ones (element kernels in every dtype); a ragged last part; 64 parts
CONCAT_LAYOUTS = {"aligned": [16, 8, 24], "aligned_ragged_tail": [8, 16, 5], "unaligned": [5, 12, 3, 16],
                  "single": [13], "parts64_aligned": [8] * 64, "parts64_by5": [5] * 64,
                  # 2056 channels = 257 chunks: the fast kernels' lanes own two chunks
                  "wide2056": [1024, 1024, 8]}


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("ych_extra", [0, 16])
@pytest.mark.parametrize("layout", list(CONCAT_LAYOUTS))
def test_concat_fwd_views_and_padding(dev, dtype, layout, ych_extra):
    """Parts and y as slice views (part.ld > round8(channels), ldy > ychannels);
    ychannels up to two chunks wider than round8(sum): those chunks are zeros."""
    _run_concat_fwd(dev, dtype, CONCAT_LAYOUTS[layout], (2, 3, 5), ych_extra=ych_extra)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("layout", list(CONCAT_LAYOUTS))
def test_concat_bwd_views_padding_and_mixed_accumulate(dev, dtype, layout):
    chans = CONCAT_LAYOUTS[layout]
    for acc in ([False] * len(chans), [True] * len(chans), [i % 2 == 0 for i in range(len(chans))],
                [i % 3 == 1 for i in range(len(chans))]):
        _run_concat_bwd(dev, dtype, chans, acc, (2, 3, 5))


@pytest.mark.parametrize("layout", ["aligned", "aligned_ragged_tail", "parts64_aligned", "wide2056"])
def test_concat_fast_and_element_kernels_agree(dev, layout):
    """An aligned layout runs concat_*_fast_k in bf16 and the element kernels in
    fp16; on values exact in both formats they give the same numbers (each is
    also compared with the reference inside the helpers)."""
    chans = CONCAT_LAYOUTS[layout]
    a = _run_concat_fwd(dev, torch.bfloat16, chans, (2, 3, 5), ych_extra=8)
    b = _run_concat_fwd(dev, torch.float16, chans, (2, 3, 5), ych_extra=8)
    assert torch.equal(a, b)
    acc = [i % 2 == 1 for i in range(len(chans))]
    for pa, pb in zip(_run_concat_bwd(dev, torch.bfloat16, chans, acc, (2, 3, 5)),
                      _run_concat_bwd(dev, torch.float16, chans, acc, (2, 3, 5))):
        assert torch.equal(pa.nan_to_num(nan=-77.0), pb.nan_to_num(nan=-77.0))


def test_concat_rejects_65_parts(dev):
    dt = torch.bfloat16
    parts = [(torch.ones(1, 1, 2, 8, dtype=dt, device=dev), 8) for _ in range(65)]
    y = torch.full((1, 1, 2, 8 * 65), NAN, dtype=dt, device=dev)
    with pytest.raises(RuntimeError, match=EINVAL):
        ops.concat_fwd(parts, y, 8 * 65)
    dsts = [(torch.full((1, 1, 2, 8), NAN, dtype=dt, device=dev), 8, False) for _ in range(65)]
    with pytest.raises(RuntimeError, match=EINVAL):
        ops.concat_bwd(torch.ones_like(y), dsts)
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and all(bool(torch.isnan(d).all()) for d, _, _ in dsts)


def test_concat_fast_second_pass(dev):
    """bf16, ychannels = 2048 (256 chunks: one pixel per workgroup pass, rows = 1),
    P = 16384 + 37 pixels > the 16384-block cap: the last 37 pixels are a second
    pass of concat_fwd_fast_k and concat_bwd_fast_k."""
    dt, P, p0, chans = torch.bfloat16, 16384 + 37, 41, [1024, 1024]
    g = _gen(77)
    xs0 = [_quarters((p0, c), g) for c in chans]
    parts = [(tile_rows(x.to(dt).to(dev), P).view(1, 1, P, c), c) for x, c in zip(xs0, chans)]
    y = torch.full((1, 1, P, 2048), NAN, dtype=dt, device=dev)
    ops.concat_fwd(parts, y, 2048)
    dy0, old0 = _quarters((p0, 2048), g), _quarters((p0, 1024), g)
    dy = tile_rows(dy0.to(dt).to(dev), P).view(1, 1, P, 2048)
    d0 = torch.full((1, 1, P, 1024), NAN, dtype=dt, device=dev)
    d1 = tile_rows(old0.to(dt).to(dev), P).view(1, 1, P, 1024).clone()
    ops.concat_bwd(dy, [(d0, 1024, False), (d1, 1024, True)])
    torch.cuda.synchronize()
    _dev_bits_equal(y.view(P, 2048), tile_rows(tf.concat(xs0).to(dt).to(dev), P), "concat fast, tiled")
    _dev_bits_equal(d0.view(P, 1024), tile_rows(dy0[:, :1024].to(dt).to(dev), P), "concat_bwd fast write, tiled")
    want1 = (old0.to(dt).float() + dy0[:, 1024:].to(dt).float()).to(dt)
    _dev_bits_equal(d1.view(P, 1024), tile_rows(want1.to(dev), P), "concat_bwd fast accumulate, tiled")


# ---------------------------------------------------------------------------
# F. dropout_k and the loop-form dropout_ch_k
# ---------------------------------------------------------------------------
def _dropout_ref(x_dt, kp, seed, counters):
    """((x * float32(1 / kp)) * floor(float32(kp) + u)).to(dtype) in fp32 steps, u the counter hash."""
    u = torch.from_numpy(_np_uniform_vec(seed, counters))
    assert u.dtype == torch.float32
    inv = torch.tensor(np.float32(1.0) / np.float32(kp))
    keep = torch.floor(torch.tensor(np.float32(kp)) + u)
    return ((x_dt.float() * inv) * keep.view(x_dt.shape)).to(x_dt.dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kp", [0.5, 0.8, 1.0])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 4099])
def test_dropout_fwd_bwd_bits(dev, dtype, kp, n):
    seed = 20240 + n
    g = _gen(n)
    x, dy = randn_normal((n,), g, dtype).to(dtype), randn_normal((n,), g, dtype).to(dtype)
    y, dx = torch.full((n + 8,), NAN, dtype=dtype, device=dev), torch.full((n + 8,), NAN, dtype=dtype, device=dev)
    ops.dropout_fwd(x.to(dev), y[:n], kp, seed)
    ops.dropout_bwd(dy.to(dev), dx[:n], kp, seed)
    torch.cuda.synchronize()
    cnt = np.arange(n, dtype=np.uint64)
    assert_bits_equal(y[:n], _dropout_ref(x, kp, seed, cnt), "dropout y")
    assert_bits_equal(dx[:n], _dropout_ref(dy, kp, seed, cnt), "dropout dx")
    assert bool(torch.isnan(y[n:]).all()) and bool(torch.isnan(dx[n:]).all())


def test_dropout_second_grid_stride_pass(dev):
    """bf16, n = 16384 x 256 + 5: the last five elements are dropout_k's second pass."""
    dt, kp, seed, n0 = torch.bfloat16, 0.8, 99, 1021
    n = 16384 * 256 + 5
    x0 = randn_normal((n0,), _gen(9), dt).to(dt)
    x = tile_rows(x0.to(dev), n)
    y = torch.full((n,), NAN, dtype=dt, device=dev)
    ops.dropout_fwd(x, y, kp, seed)
    torch.cuda.synchronize()
    want = _dropout_ref(tile_rows(x0, n), kp, seed, np.arange(n, dtype=np.uint64))
    _dev_bits_equal(y, want.to(dev), "dropout y, second pass")


def test_dropout_ch_loop_form_second_pass(dev):
    """dropout_ch_k (option dropout_flat = 0) at C = 2048 (rows = 1), P = 16384 +
    37 > its 16384-block cap: bit-equal to the flat form everywhere, and to the
    counter hash (counter pixel * c_valid + c) on the first pixels and on every
    pixel of the second pass."""
    dt, C, cv, P, kp, seed, p0 = torch.bfloat16, 2048, 2045, 16384 + 37, 0.8, 4711, 41
    dy0 = randn_normal((p0, C), _gen(10), dt).to(dt)
    dy = tile_rows(dy0.to(dev), P).view(1, 1, P, C)

    def run():
        dz = torch.full((1, 1, P, C), NAN, dtype=dt, device=dev)
        ops.dropout_bwd_ch(dy, dz, cv, kp, seed)
        return dz
    flat = run()
    ops.set_option("dropout_flat", 0)
    try:
        loop = run()
    finally:
        ops.set_option("dropout_flat", 1)
    torch.cuda.synchronize()
    _dev_bits_equal(loop, flat, "loop form vs flat form")
    full = tile_rows(dy0, P)
    for lo, hi in ((0, 64), (16384 - 8, P)):
        pix = np.arange(lo, hi, dtype=np.uint64)
        cnt = (pix[:, None] * np.uint64(cv) + np.arange(cv, dtype=np.uint64)[None, :]).reshape(-1)
        want = torch.zeros(hi - lo, C, dtype=dt)                       # padding channels: zeros
        want[:, :cv] = _dropout_ref(full[lo:hi, :cv].contiguous(), kp, seed, cnt)
        assert_bits_equal(loop.view(P, C)[lo:hi], want, f"dropout_ch_k pixels {lo}..{hi}")
