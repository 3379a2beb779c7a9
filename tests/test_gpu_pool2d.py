"""seg_pool2d_fwd / seg_pool2d_bwd and seg_pad2d_fwd / seg_pad2d_bwd (csrc/pool.hip)
against tests/pool_ref.py on the rounded inputs: f32, bf16 and f16, max and
average, forward and gradient, dense and (the C = 8 cases) through a channel
slice of a wider tensor.  Every destination starts as NaN, so an element the
kernel skips shows.

Max-pool inputs are small integers, so ties occur: y and the switches are
exact, dx is exact where windows do not overlap and within the dtype tolerance
(tests/gpu_utils.py) of the float64 sum where they do.  Averages and their
gradients: the dtype tolerance.  The 2x2 stride-2 VALID case must equal the
seg_maxpool2x2_* / seg_avgpool2x2_* kernels bit for bit.  Refused calls leave
their destination untouched."""
import ctypes
import functools

import pytest
import torch

from semanticsegmentation_tensorflow_amd import _lib, ops
from tests import pool_ref as R
from tests.gpu_utils import assert_bits_equal, assert_close, assert_surroundings, rnd

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
# (N, H, W, C, kh, kw, sh, sw, padding)
CASES = [(2, 9, 11, 16, 3, 3, 2, 2, "VALID"),        # overlapping windows
         (1, 8, 8, 8, 3, 3, 2, 2, "SAME"),           # asymmetric pad (0 before, 1 after)
         (2, 5, 18, 24, 5, 18, 5, 18, "VALID"),      # 1 x 1 output
         (1, 5, 18, 8, 3, 9, 3, 9, "VALID"),
         (1, 5, 18, 8, 2, 6, 2, 6, "VALID"),         # leftover row
         (1, 5, 18, 8, 1, 3, 1, 3, "VALID"),
         (2, 7, 9, 8, 1, 1, 2, 2, "VALID"),          # the subsample of a strided 1x1 conv
         (1, 7, 7, 8, 2, 2, 3, 3, "VALID"),          # gaps between windows: their gradient is 0
         (1, 6, 6, 40, 2, 2, 2, 2, "VALID")]         # the geometry of the 2x2 kernels
JUNK = 50.0
EINVAL = 1


def _ks(case):
    return (case[4], case[5]), (case[6], case[7]), case[8]


@functools.lru_cache(maxsize=None)
def reference(case, kind, dt):
    """(x, y, idx, dy, dx) float64 / int64 on the inputs rounded through the dtype."""
    N, H, W, C = case[:4]
    k, s, pad = _ks(case)
    dtype = DTYPES[dt]
    g = torch.Generator().manual_seed(2 * CASES.index(case) + (kind == "max"))
    if kind == "max":
        x = torch.randint(-2, 3, (N, H, W, C), generator=g).double()      # five values: ties in every window
        y, idx = R.max_pool(x, k, s, pad)
        dy = rnd(torch.randn(y.shape, generator=g, dtype=torch.float64), dtype)
        dx = R.max_pool_grad(idx, dy, x.shape, k, s, pad)
    else:
        x = rnd(torch.randn((N, H, W, C), generator=g, dtype=torch.float64), dtype)
        y, idx = R.avg_pool(x, k, s, pad), None
        dy = rnd(torch.randn(y.shape, generator=g, dtype=torch.float64), dtype)
        dx = R.avg_pool_grad(dy, x.shape, k, s, pad)
    return x, y, idx, dy, dx


def dense(t64, dtype, dev):
    return t64.to(dtype).to(dev).contiguous()


def slice_view(t64, dtype, dev, wide=24, off=8):
    """t64 [.., C] as channels off .. off + C of a [.., wide] tensor of JUNK."""
    base = torch.full(tuple(t64.shape[:-1]) + (wide,), JUNK, dtype=dtype, device=dev)
    v = base[..., off:off + t64.shape[-1]]
    v.copy_(t64.to(dtype))
    return v


def nan_dest(shape, dtype, dev, sliced):
    nan = torch.full(shape, float("nan"), dtype=torch.float64)
    return slice_view(nan, dtype, dev) if sliced else dense(nan, dtype, dev)


def run_case(dev, case, kind, dt, sliced):
    N, H, W, C = case[:4]
    k, s, pad = _ks(case)
    dtype = DTYPES[dt]
    x, y_ref, idx_ref, dy, dx_ref = reference(case, kind, dt)
    desc = ops.pool_desc(N, H, W, C, k, s, pad, ops.POOL_MAX if kind == "max" else ops.POOL_AVG, ops.seg_dtype(
        torch.empty(0, dtype=dtype)))
    assert (desc.OH, desc.OW) == tuple(y_ref.shape[1:3])
    put = slice_view if sliced else dense
    xd = put(x, dtype, dev)
    yd = nan_dest(y_ref.shape, dtype, dev, sliced)
    idx = torch.full((y_ref.numel(),), 255, dtype=torch.uint8, device=dev) if kind == "max" else None
    ops.pool2d_fwd(desc, xd, yd, idx)
    dyd = put(dy, dtype, dev)
    dxd = nan_dest(x.shape, dtype, dev, sliced)
    ops.pool2d_bwd(desc, idx, dyd, dxd)
    torch.cuda.synchronize()
    what = f"{kind} {case} {dt}{' sliced' if sliced else ''}"
    if sliced:
        for v in (xd, yd, dyd, dxd):
            assert_surroundings(v, JUNK, what)
    if kind == "max":
        assert_bits_equal(yd.contiguous(), y_ref.to(dtype), what + " y")
        assert torch.equal(idx.cpu().view(y_ref.shape).long(), idx_ref), what + " switches"
        got = dxd.double().cpu()
        assert not torch.isnan(got).any(), what
        single = ~R.overlap(x.shape, k, s, pad)
        assert_bits_equal(dxd.contiguous().cpu()[:, single], dx_ref.to(dtype)[:, single], what + " dx, one window")
        assert_close(got, dx_ref, dtype, what + " dx")
    else:
        assert_close(yd.double().cpu(), y_ref, dtype, what + " y")
        assert_close(dxd.double().cpu(), dx_ref, dtype, what + " dx")
        assert not torch.isnan(dxd.double()).any()
        covered = R.avg_pool_grad(torch.ones_like(dy), x.shape, k, s, pad) != 0
        assert bool((dxd.double().cpu()[~covered] == 0).all()), what + ": uncovered pixels must get 0"
    return xd, yd, idx, dyd, dxd


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("kind", ["max", "avg"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_pool2d_fwd_bwd(dev, case, kind, dt):
    run_case(dev, case, kind, dt, sliced=False)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("kind", ["max", "avg"])
@pytest.mark.parametrize("case", [c for c in CASES if c[3] == 8], ids=lambda c: "x".join(str(v) for v in c))
def test_pool2d_channel_slice_views(dev, case, kind, dt):
    run_case(dev, case, kind, dt, sliced=True)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_2x2_stride2_valid_equals_the_2x2_kernels_bit_for_bit(dev, dt):
    case = CASES[-1]
    N, H, W, C = case[:4]
    dtype = DTYPES[dt]
    xd, yd, idx, dyd, dxd = run_case(dev, case, "max", dt, sliced=False)
    y2 = torch.full_like(yd, float("nan"))
    idx2 = torch.full_like(idx, 255)
    dx2 = torch.full_like(dxd, float("nan"))
    ops.maxpool2x2_fwd_argmax(xd, y2, idx2)
    ops.maxpool2x2_bwd_argmax(idx2, dyd, dx2)
    torch.cuda.synchronize()
    assert_bits_equal(yd, y2, "max y")
    assert torch.equal(idx, idx2 & 3), "switches: bits 0-1 of the 2x2 kernels' byte"
    assert_bits_equal(dxd, dx2, "max dx")
    xd, yd, _, dyd, dxd = run_case(dev, case, "avg", dt, sliced=False)
    y2 = torch.full_like(yd, float("nan"))
    dx2 = torch.full_like(dxd, float("nan"))
    ops.avgpool2x2_fwd(xd, y2)
    ops.avgpool2x2_bwd(dyd, dx2)
    torch.cuda.synchronize()
    assert_bits_equal(yd, y2, "avg y")
    assert_bits_equal(dxd, dx2, "avg dx")


def test_refused_calls_write_nothing(dev):
    lib = _lib.lib()
    dtype = torch.bfloat16
    N, H, W, C = 1, 20, 20, 8
    x = torch.ones(N, H, W, C, dtype=dtype, device=dev)
    good = ops.pool_desc(N, H, W, C, (3, 3), (2, 2), "SAME", ops.POOL_MAX, ops.BF16)
    y = torch.full((N, good.OH, good.OW, C), float("nan"), dtype=dtype, device=dev)
    idx = torch.full((y.numel(),), 255, dtype=torch.uint8, device=dev)
    dx = torch.full((N, H, W, C), float("nan"), dtype=dtype, device=dev)
    dy = torch.ones_like(y)
    s = ops.stream_ptr()

    def edited(**kw):
        d = _lib.SegPoolDesc.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    bad = [edited(kh=17, kw=16),            # 272 window elements: more than the switch byte holds
           edited(kh=1, kw=257), edited(kh=0), edited(sh=0), edited(sw=-1), edited(C=12, ldx=12, ldy=12),
           edited(N=0), edited(OH=0), edited(ldx=4), edited(kind=2), edited(dtype=9),
           edited(OH=40),                   # windows that start below the image
           edited(N=1 << 20, H=1 << 10, W=1 << 10)]
    for d in bad:
        assert lib.seg_pool2d_fwd(ctypes.byref(d), ops.ptr(x), ops.ptr(y), ops.ptr(idx), s) == EINVAL
        assert lib.seg_pool2d_bwd(ctypes.byref(d), ops.ptr(idx), ops.ptr(dy), ops.ptr(dx), s) == EINVAL
    # the max-pool gradient needs the switches; the average ignores them
    assert lib.seg_pool2d_bwd(ctypes.byref(good), None, ops.ptr(dy), ops.ptr(dx), s) == EINVAL
    assert lib.seg_pool2d_fwd(ctypes.byref(good), None, ops.ptr(y), None, s) == EINVAL
    # pad: negative pads, a channel count that is not whole chunks
    yp = torch.full((N, H + 2, W + 2, C), float("nan"), dtype=dtype, device=dev)
    assert lib.seg_pad2d_fwd(ops.ptr(x), C, ops.ptr(yp), C, N, H, W, C, -1, 3, 1, 1, ops.BF16, s) == EINVAL
    assert lib.seg_pad2d_fwd(ops.ptr(x), C, ops.ptr(yp), C, N, H, W, 12, 1, 1, 1, 1, ops.BF16, s) == EINVAL
    assert lib.seg_pad2d_bwd(ops.ptr(yp), C, ops.ptr(dx), C, N, H, W, C, 1, 1, -1, 3, ops.BF16, s) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(dx).all()) and bool(torch.isnan(yp).all())
    assert bool((idx == 255).all())
    # and the unedited descriptor runs, with idx NULL on the forward (an inference plan)
    ops.pool2d_fwd(good, x, y, None)
    avg = edited(kind=ops.POOL_AVG)
    ops.pool2d_bwd(avg, None, dy, dx)
    torch.cuda.synchronize()
    assert bool((y == 1).all()) and not bool(torch.isnan(dx).any())


PAD_SHAPE = (2, 5, 7, 16)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("pads,sliced", [((3, 3, 3, 3), False), ((1, 1, 1, 1), True), ((0, 2, 1, 0), False)])
def test_pad2d_forward_and_crop_exact(dev, pads, sliced, dt):
    dtype = DTYPES[dt]
    g = torch.Generator().manual_seed(11)
    x = rnd(torch.randn(PAD_SHAPE, generator=g, dtype=torch.float64), dtype)
    y_ref = R.pad(x, pads)
    dy = rnd(torch.randn(y_ref.shape, generator=g, dtype=torch.float64), dtype)
    put = (lambda t: slice_view(t, dtype, dev, wide=40, off=16)) if sliced else (lambda t: dense(t, dtype, dev))
    nan = lambda shape: put(torch.full(shape, float("nan"), dtype=torch.float64))     # noqa: E731
    xd, yd, dyd, dxd = put(x), nan(y_ref.shape), put(dy), nan(x.shape)
    ops.pad2d_fwd(xd, yd, pads)
    ops.pad2d_bwd(dyd, dxd, pads)
    torch.cuda.synchronize()
    assert_bits_equal(yd.contiguous(), y_ref.to(dtype), f"pad {pads}")
    assert_bits_equal(dxd.contiguous(), R.crop(dy, pads).to(dtype), f"crop {pads}")
    if sliced:
        for v in (xd, yd, dyd, dxd):
            assert_surroundings(v, JUNK, f"pad {pads}")
