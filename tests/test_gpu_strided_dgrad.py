"""Conv2DBackpropInput of strided convs (seg_conv2d_bwd_data with stride > 1):
the dgrad_s2 halo kernel (4x4 / 2, 16-bit) and the phase-GEMM fallback, both
against the float64 oracle (autograd through oracle.tf1_ops.conv2d) at the
project's per-dtype tolerances.

dgrad_s2 tiles dx in 8 x 32 padded coordinates (rows ih + pad_top, columns
iw + pad_left), so the 13 x 41 SAME case below is 2 x 2 tiles with ragged last
tiles (14 = 8 + 6 rows, 42 = 32 + 10 columns)."""
import ctypes
import functools
import math

import pytest
import torch

from oracle import tf1_ops as T
from semanticsegmentation_tensorflow_amd import _lib, ops
from tests.gpu_utils import assert_close, from_dev, rnd, to_dev

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DT = {torch.float32: ops.F32, torch.bfloat16: ops.BF16, torch.float16: ops.F16}

# (N, H, W, C, K, R, stride, padding), whether dgrad_s2 must take the 16-bit form
CASES = [
    ((1, 11, 13, 16, 32, 4, 2, "SAME"), True),      # odd sizes: asymmetric pads (1, 2)
    ((2, 13, 10, 32, 64, 4, 2, "VALID"), True),     # input row 12 is covered by no window: dx row 12 = 0
    ((2, 20, 36, 32, 64, 4, 2, "SAME"), True),      # LidCamNet conv3's channels on an 8x-reduced map
    ((1, 10, 18, 64, 128, 4, 2, "SAME"), True),     # LidCamNet conv5's channels
    ((2, 13, 41, 32, 32, 4, 2, "SAME"), True),      # 2 x 2 tiles, ragged last tiles
    ((1, 9, 9, 12, 24, 4, 2, "SAME"), False),       # C = 12 -> 16, K = 24: padding channels, phase GEMMs
    ((1, 8, 12, 16, 16, 2, 2, "VALID"), False),     # 2x2 / 2
    ((1, 12, 12, 8, 16, 4, 4, "SAME"), False),      # 4x4 / 4
]
IDS = [f"{c[0][1]}x{c[0][2]}x{c[0][3]}-{c[0][4]}-k{c[0][5]}s{c[0][6]}-{c[0][7]}" for c in CASES]
HALO_CASE, FALLBACK_CASE = CASES[2][0], CASES[6][0]


@pytest.fixture
def knob(dev):
    def set_(v):
        ops.set_option("dgrad_s2", v)
    yield set_
    ops.set_option("dgrad_s2", 1)


@functools.lru_cache(maxsize=None)
def _problem(case, dtype):
    """float64 inputs as the device sees them (rounded through dtype) and the
    oracle's input gradient; computed once per (case, dtype) and never changed."""
    N, H, W, C, K, R, st, pad = case
    g = torch.Generator().manual_seed(11)
    w = rnd(torch.randn(R, R, C, K, generator=g, dtype=torch.float64) / math.sqrt(R * R * C), dtype)
    x = torch.zeros(N, H, W, C, dtype=torch.float64, requires_grad=True)
    y = T.conv2d(x, w, st, pad, 1)
    dy = rnd(torch.randn(y.shape, generator=g, dtype=torch.float64), dtype)
    (y * dy).sum().backward()
    return w, dy, x.grad.detach()


def _pack_hwio(w64, dtype, dev):
    R, S, A, B = w64.shape
    src = w64.float().to(dev).contiguous()
    dst = torch.empty(ops.packed_shape(R, S, A, B, ops.PACK_HWIO), dtype=dtype, device=dev)
    return ops.pack_filter(src, dst, ops.round8(A), ops.round8(B), ops.PACK_HWIO)


def _desc(case, dtype):
    N, H, W, C, K, R, st, pad = case
    return ops.conv_desc(N, H, W, C, K, R, R, st, 1, pad, DT[dtype])


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("case,halo", CASES, ids=IDS)
def test_strided_bwd_data_both_routes(dev, knob, case, halo, dtype):
    N, H, W, C, K, R, st, pad = case
    w, dy, want = _problem(case, dtype)
    d = _desc(case, dtype)
    h16 = dtype != torch.float32
    assert ops.conv2d_bwd_data_s2_ok(d) == (halo and h16), case
    assert ops.conv_workspace(d, ops.OP_BWD_DATA) == 0
    dyd, wh = to_dev(dy, dtype, dev), _pack_hwio(w, dtype, dev)
    if case[1] == 13 and pad == "VALID":
        assert want[:, 12].abs().max().item() == 0        # the oracle agrees: no window covers row 12
    outs = {}
    for on in (1, 0):
        knob(on)
        name = ops.conv_kernel_info(d, ops.OP_BWD_DATA)[0]
        if halo and h16 and on:
            assert name.startswith("dgrad_s2<"), name
        else:
            assert name.startswith(("igemm_nt<", "igemm_nt2<", "igemm_nt3<")), name
        dx = torch.full((N, H, W, d.C), float("nan"), dtype=dtype, device=dev)
        ops.conv2d_bwd_data(d, dyd, wh, dx)
        torch.cuda.synchronize()
        e = assert_close(from_dev(dx, C), want, dtype, f"strided bwd_data {case} {name}")
        print(f"{case} {name}: rel err {e:.3e}")
        if d.C > C:
            assert dx[..., C:].float().abs().max().item() == 0, f"padding channels, {name}"
        if case[1] == 13 and pad == "VALID":
            assert dx[:, 12].float().abs().max().item() == 0, f"uncovered row, {name}"
        outs[on] = dx
    # the fallback is the phase split of seg_tconv2d_fwd on the mirrored descriptor,
    # reading the same HWIO copy: bit-identical where conv2d_transpose itself
    # runs the phase GEMMs (its tap-dense form -- 8 output channels at stride
    # >= 4, the 4x4 / 4 case -- rounds an intermediate and is compared at tolerance)
    OH, OW = d.OH, d.OW
    td = ops.tconv_desc(N, OH, OW, K, H, W, C, R, R, st, pad, DT[dtype])
    yt = torch.full((N, H, W, td.K), float("nan"), dtype=dtype, device=dev)
    ops.tconv2d_fwd(td, dyd, wh, yt)
    torch.cuda.synchronize()
    if ops.conv_workspace(td, ops.OP_TFWD) == 0:
        assert torch.equal(_bits(outs[0]), _bits(yt)), f"fallback vs conv2d_transpose {case}"
    else:
        assert (case[3], st) == (8, 4)
        assert_close(from_dev(yt, C), want, dtype, "tap-dense conv2d_transpose")


def _run(d, dyd, wh, dx, epi=None):
    ops.conv2d_bwd_data(d, dyd, wh, dx, epi=epi)
    torch.cuda.synchronize()


@pytest.mark.parametrize("on", [1, 0], ids=["knob-on", "knob-off"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("case", [HALO_CASE, FALLBACK_CASE], ids=["halo", "fallback"])
def test_strided_bwd_data_epilogue_and_views(dev, knob, case, dtype, on):
    N, H, W, C, K, R, st, pad = case
    w, dy, want = _problem(case, dtype)
    d = _desc(case, dtype)
    knob(on)
    name = ops.conv_kernel_info(d, ops.OP_BWD_DATA)[0]
    assert name.startswith("dgrad_s2<") == (case is HALO_CASE and dtype != torch.float32 and on == 1), name
    dyd, wh = to_dev(dy, dtype, dev), _pack_hwio(w, dtype, dev)
    g = torch.Generator().manual_seed(5)
    # residual, in place
    base = rnd(torch.randn(N, H, W, C, generator=g, dtype=torch.float64), dtype)
    dx = to_dev(base, dtype, dev)
    _run(d, dyd, wh, dx, ops.epilogue(residual=dx))
    assert_close(from_dev(dx, C), want + base, dtype, f"residual in place, {name}")
    # ReluGrad mask x 1 / keep_prob
    prev = torch.relu(torch.randn(N, H, W, C, generator=g, dtype=torch.float64))
    prev_d = to_dev(prev, dtype, dev)
    dx = torch.full((N, H, W, d.C), float("nan"), dtype=dtype, device=dev)
    _run(d, dyd, wh, dx, ops.epilogue(relu_mask=prev_d, mask_scale=1 / 0.8))
    wantm = torch.where(prev > 0, want / 0.8, torch.zeros_like(want))
    assert (wantm == 0).float().mean().item() > 0.3
    assert_close(from_dev(dx, C), wantm, dtype, f"relu_mask, {name}")
    assert (from_dev(dx, C)[prev == 0] == 0).all()
    # dx a channel slice of a wider buffer: the other channels untouched bit for bit
    wide = torch.randn(N, H, W, d.C + 16, generator=g, dtype=torch.float64).to(dtype).to(dev)
    keep = wide.clone()
    _run(d, dyd, wh, wide[..., 8:8 + d.C])
    assert_close(from_dev(wide[..., 8:8 + C]), want, dtype, f"dx slice, {name}")
    assert torch.equal(_bits(wide[..., :8]), _bits(keep[..., :8]))
    assert torch.equal(_bits(wide[..., 8 + d.C:]), _bits(keep[..., 8 + d.C:]))
    # dy a channel slice (ldy > K)
    dyw = torch.randn(N, d.OH, d.OW, d.K + 16, generator=g, dtype=torch.float64).to(dtype).to(dev)
    dyw[..., 8:8 + d.K] = dyd
    dx = torch.full((N, H, W, d.C), float("nan"), dtype=dtype, device=dev)
    _run(d, dyw[..., 8:8 + d.K], wh, dx)
    assert_close(from_dev(dx, C), want, dtype, f"dy slice, {name}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
def test_strided_bwd_data_refusals(dev, knob, dtype):
    lib = _lib.lib()
    SEG_EINVAL = 1
    for R, st, dil in [(4, 2, 2), (3, 2, 1)]:        # stride with dilation; 3x3 / 2
        d = ops.conv_desc(1, 12, 12, 16, 32, R, R, st, dil, "SAME", DT[dtype])
        assert not ops.conv2d_bwd_data_s2_ok(d)
        dy = torch.ones(1, d.OH, d.OW, d.K, dtype=dtype, device=dev)
        wh = torch.ones(R, R, d.C, d.K, dtype=dtype, device=dev)
        dx = torch.full((1, 12, 12, d.C), float("nan"), dtype=dtype, device=dev)
        for on in (1, 0):
            knob(on)
            st_ = lib.seg_conv2d_bwd_data(ctypes.byref(d), ops.ptr(dy), ops.ptr(wh), None, ops.ptr(dx), None, 0,
                                          ops.stream_ptr())
            assert st_ == SEG_EINVAL, (R, st, dil, st_)
            with pytest.raises(RuntimeError, match="status 1"):
                ops.conv_kernel_info(d, ops.OP_BWD_DATA)
        torch.cuda.synchronize()
        assert torch.isnan(dx.float()).all(), "a refused call wrote dx"
    # stride 1 is untouched by the knob
    d1 = ops.conv_desc(2, 20, 36, 32, 64, 4, 4, 1, 1, "SAME", DT[dtype])
    names = []
    for on in (1, 0):
        knob(on)
        names.append(ops.conv_kernel_info(d1, ops.OP_BWD_DATA))
    assert names[0] == names[1] and not names[0][0].startswith("dgrad_s2")
    assert not ops.conv2d_bwd_data_s2_ok(d1)


def test_s2_ok_takes_the_lidcamnet_shapes(dev):
    for dt in (ops.BF16, ops.F16):
        for N in (1, 4):
            assert ops.conv2d_bwd_data_s2_ok(ops.conv_desc(N, 80, 288, 32, 64, 4, 4, 2, 1, "SAME", dt))    # conv3
            assert ops.conv2d_bwd_data_s2_ok(ops.conv_desc(N, 40, 144, 64, 128, 4, 4, 2, 1, "SAME", dt))   # conv5
    assert not ops.conv2d_bwd_data_s2_ok(ops.conv_desc(4, 80, 288, 32, 64, 4, 4, 2, 1, "SAME", ops.F32))
