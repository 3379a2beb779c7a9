"""seg_dwconv2d_fwd / _bwd_data / _bwd_filter (csrc/dwconv.hip) against
tests/dwconv_ref.py: f32, bf16 and f16, dense and (the C = 8 cases) through a
channel slice of a wider tensor of JUNK.  Every destination starts as NaN, so
an element a kernel skips shows.

The inputs are rounded through bf16 with magnitudes floored at 2^-6, so one
float64 reference serves the three dtypes (such values are exact in f16 and
f32 too); the filter is an fp32 master.  Bounds are derived, not fitted:

* y, dx: computed in fp32 over at most R S terms and stored once --
  storage_bound(ref, dtype, R S U sum|terms|);
* dw (fp32): n U sum|x dy| with n the number of summed terms, which holds for
  any summation order.

The filter gradient run twice is bit-identical; a refused call leaves its
destinations untouched."""
import ctypes
import functools

import pytest
import torch

from semanticsegmentation_tensorflow_amd import _lib, ops
from tests import dwconv_ref as D
from tests.gpu_utils import U, assert_bits_equal, assert_surroundings, assert_within, randn_normal, storage_bound

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CASES = D.CASES
JUNK = 50.0
EINVAL, ESHAPE, EALIGN, EWORKSPACE = 1, 2, 3, 4
_id = lambda c: "x".join(str(v) for v in c).replace(" ", "")     # noqa: E731


@functools.lru_cache(maxsize=None)
def reference(case, c_valid=None):
    """float64 (x, w, y, dy, dx, dw) and the bounds' fp32 terms (ty, tdx, tdw)."""
    N, H, W, C, R, S, stride, rate, padding = case
    cv = c_valid or C
    g = torch.Generator().manual_seed(100 + CASES.index(case))
    x = randn_normal((N, H, W, cv), g, torch.bfloat16)
    w = torch.randn(R, S, cv, generator=g, dtype=torch.float64).float().double()
    y = D.forward(x, w, stride, rate, padding)
    dy = randn_normal(tuple(y.shape), g, torch.bfloat16)
    dx = D.input_grad(dy, w, tuple(x.shape), stride, rate, padding)
    dw = D.filter_grad(x, dy, R, S, stride, rate, padding)
    ty = R * S * U * D.forward(x.abs(), w.abs(), stride, rate, padding)
    tdx = R * S * U * D.input_grad(dy.abs(), w.abs(), tuple(x.shape), stride, rate, padding)
    n = D.filter_grad(torch.ones_like(x), torch.ones_like(dy), R, S, stride, rate, padding)
    tdw = n * U * D.filter_grad(x.abs(), dy.abs(), R, S, stride, rate, padding)
    return x, w, y, dy, dx, dw, ty, tdx, tdw


def _pad_c(t64, C):
    """[.., cv] -> [.., C] with zeros in the padding channels."""
    out = torch.zeros(tuple(t64.shape[:-1]) + (C,), dtype=torch.float64)
    out[..., :t64.shape[-1]] = t64
    return out


def dense(t64, dtype, dev):
    return t64.to(dtype).to(dev).contiguous()


def slice_view(t64, dtype, dev, wide=24, off=8):
    """t64 [.., C] as channels off .. off + C of a [.., wide] tensor of JUNK."""
    base = torch.full(tuple(t64.shape[:-1]) + (wide,), JUNK, dtype=dtype, device=dev)
    v = base[..., off:off + t64.shape[-1]]
    v.copy_(t64.to(dtype))
    return v


def run_case(dev, case, dt, sliced=False, c_valid=None):
    N, H, W, C, R, S, stride, rate, padding = case
    cv = c_valid or C
    dtype = DTYPES[dt]
    x, w, y_ref, dy, dx_ref, dw_ref, ty, tdx, tdw = reference(case, c_valid)
    desc = ops.dwconv_desc(N, H, W, C, cv, R, S, stride, rate, padding, ops.seg_dtype(torch.empty(0, dtype=dtype)))
    assert (desc.OH, desc.OW) == tuple(y_ref.shape[1:3])
    assert (desc.pad_top, desc.pad_left) == (D.geometry(H, R, stride, rate[0], padding)[1],
                                             D.geometry(W, S, stride, rate[1], padding)[1])
    put = slice_view if sliced else dense
    nan = lambda shape: put(torch.full(shape, float("nan"), dtype=torch.float64), dtype, dev)     # noqa: E731
    xd, dyd = put(_pad_c(x, C), dtype, dev), put(_pad_c(dy, C), dtype, dev)
    wd = w.float().to(dev).contiguous()
    yd, dxd = nan(tuple(y_ref.shape[:3]) + (C,)), nan((N, H, W, C))
    dwd = torch.full((R, S, cv), float("nan"), dtype=torch.float32, device=dev)
    dwd2 = torch.full_like(dwd, float("nan"))
    need = ops.dwconv_bwd_filter_workspace(desc)
    assert need >= R * S * C * 4 and need % (R * S * C * 4) == 0
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)       # NaN partial rows until written
    ops.dwconv2d_fwd(desc, xd, wd, yd)
    ops.dwconv2d_bwd_data(desc, dyd, wd, dxd)
    ops.dwconv2d_bwd_filter(desc, xd, dyd, dwd, ws)
    ops.dwconv2d_bwd_filter(desc, xd, dyd, dwd2, ws)
    torch.cuda.synchronize()
    what = f"{case} {dt}{' sliced' if sliced else ''}{f' c_valid {cv}' if c_valid else ''}"
    if sliced:
        for v in (xd, yd, dyd, dxd):
            assert_surroundings(v, JUNK, what)
    got_y, got_dx = yd.double().cpu(), dxd.double().cpu()
    fy = assert_within(got_y[..., :cv], y_ref, storage_bound(y_ref, dtype, ty), what + " y")
    fdx = assert_within(got_dx[..., :cv], dx_ref, storage_bound(dx_ref, dtype, tdx), what + " dx")
    fdw = assert_within(dwd.double().cpu(), dw_ref, tdw, what + " dw")
    print(f"{what}: fraction of the bound used: y {fy:.3f} dx {fdx:.3f} dw {fdw:.3f}")
    # padding channels: exact zeros; pixels no tap reaches: exact zeros
    assert bool((got_y[..., cv:] == 0).all()) and bool((got_dx[..., cv:] == 0).all()), what + " padding channels"
    reached = D.input_grad(torch.ones_like(dy), torch.ones_like(w), tuple(x.shape), stride, rate, padding) != 0
    assert bool((got_dx[..., :cv][~reached] == 0).all()), what + ": unreached pixels must get 0"
    assert_bits_equal(dwd, dwd2, what + " dw twice")
    return need


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_dwconv_fwd_bwd(dev, case, dt):
    need = run_case(dev, case, dt)
    if case == CASES[-1]:
        # the second pass of the filter gradient sums more than one partial row
        N, H, W, C, R, S = case[:6]
        assert need > R * S * C * 4, need


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("case", [c for c in CASES if c[3] == 8], ids=_id)
def test_dwconv_channel_slice_views(dev, case, dt):
    run_case(dev, case, dt, sliced=True)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("case", [CASES[1], CASES[4]], ids=_id)
def test_dwconv_three_valid_channels_of_eight(dev, case, dt):
    assert case[3] == 8
    run_case(dev, case, dt, c_valid=3)
    run_case(dev, case, dt, sliced=True, c_valid=3)


def test_cases_reach_zero_gradient_pixels_and_padding_only_taps():
    """(host) The case list does what its comments say."""
    x_shape = CASES[-2][:4]
    N, H, W, C, R, S, stride, rate, padding = CASES[-2]
    reached = D.input_grad(torch.ones(D.out_shape(x_shape, R, S, stride, rate, padding), dtype=torch.float64),
                           torch.ones(R, S, C, dtype=torch.float64), x_shape, stride, rate, padding)[0, :, :, 0] != 0
    assert bool(reached[:9, :11].all()) and not bool(reached[9].any()) and not bool(reached[:, 11].any())
    N, H, W, C, R, S, stride, rate, padding = CASES[3]
    n = D.filter_grad(torch.ones(N, H, W, C, dtype=torch.float64), torch.ones(N, H, W, C, dtype=torch.float64), R, S,
                      stride, rate, padding)[:, :, 0]
    assert n[1, 1] == H * W and n[0, 0] == 0 and n[1, 0] > 0       # rows above / below are never in-image


def test_refused_calls_write_nothing(dev):
    lib = _lib.lib()
    dtype = torch.bfloat16
    N, H, W, C = 1, 12, 12, 8
    good = ops.dwconv_desc(N, H, W, C, C, 3, 3, 1, (2, 2), "SAME", ops.BF16)
    x = torch.ones(N, H, W, C, dtype=dtype, device=dev)
    w = torch.ones(3, 3, C, dtype=torch.float32, device=dev)
    y = torch.full((N, good.OH, good.OW, C), float("nan"), dtype=dtype, device=dev)
    dx = torch.full((N, H, W, C), float("nan"), dtype=dtype, device=dev)
    dw = torch.full((3, 3, C), float("nan"), dtype=torch.float32, device=dev)
    dy = torch.ones_like(y)
    need = ops.dwconv_bwd_filter_workspace(good)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    s = ops.stream_ptr()

    def edited(**kw):
        d = _lib.SegDwconvDesc.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    bad = [(edited(R=8), EINVAL), (edited(S=0), EINVAL), (edited(N=0), EINVAL), (edited(stride=0), EINVAL),
           (edited(dil_h=0), EINVAL), (edited(dtype=9), EINVAL), (edited(pad_top=-1), EINVAL),
           (edited(c_valid=0), EINVAL), (edited(ldx=4), EALIGN), (edited(ldy=12), EALIGN),
           (edited(C=12, ldx=12, ldy=12), EALIGN), (edited(c_valid=9), EALIGN), (edited(C=16), EINVAL),
           (edited(stride=2), ESHAPE),                  # rate 2 with stride 2: TF's rule
           (edited(OH=0), ESHAPE), (edited(N=1 << 20, H=1 << 10, W=1 << 10), EINVAL)]
    for d, code in bad:
        assert lib.seg_dwconv2d_fwd(ctypes.byref(d), ops.ptr(x), ops.ptr(w), ops.ptr(y), s) == code
        assert lib.seg_dwconv2d_bwd_data(ctypes.byref(d), ops.ptr(dy), ops.ptr(w), ops.ptr(dx), s) == code
        assert lib.seg_dwconv2d_bwd_filter(ctypes.byref(d), ops.ptr(x), ops.ptr(dy), ops.ptr(dw), ops.ptr(ws),
                                           ctypes.c_size_t(need), s) == code
        assert lib.seg_dwconv_bwd_filter_workspace(ctypes.byref(d)) == 0
    # null pointers, and a workspace one byte short
    assert lib.seg_dwconv2d_fwd(ctypes.byref(good), None, ops.ptr(w), ops.ptr(y), s) == EINVAL
    assert lib.seg_dwconv2d_bwd_data(ctypes.byref(good), ops.ptr(dy), None, ops.ptr(dx), s) == EINVAL
    assert lib.seg_dwconv2d_bwd_filter(ctypes.byref(good), ops.ptr(x), ops.ptr(dy), ops.ptr(dw), ops.ptr(ws),
                                       ctypes.c_size_t(need - 1), s) == EWORKSPACE
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(dx).all()) and bool(torch.isnan(dw).all())
    assert bool((ws == 0xFF).all())
    # and the unedited descriptor runs: ones through a 3x3 of ones count the in-image taps
    ops.dwconv2d_fwd(good, x, w, y)
    ops.dwconv2d_bwd_data(good, dy, w, dx)
    ops.dwconv2d_bwd_filter(good, x, dy, dw, ws)
    torch.cuda.synchronize()
    assert y[0, 6, 6, 0].item() == 9 and y[0, 0, 0, 0].item() == 4 and torch.equal(y, dx)
    assert dw[1, 1, 0].item() == H * W and dw[0, 0, 0].item() == (H - 2) * (W - 2)
