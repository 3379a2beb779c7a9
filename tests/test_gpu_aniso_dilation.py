"""Per-axis dilation (tf.nn.conv2d dilations=[1, dh, dw, 1], LidCamNet's
context module): forward (+bias), input gradient and filter gradient of 3x3
stride-1 convs against the float64 per-axis reference tests/aniso_ref.py, at
the project's per-dtype tolerances.  Every kernel family indexes taps with
tsh / tsw separately; these cases reach them with tsh != tsw (the family that
ran is in each assertion message)."""
import functools
import math

import pytest
import torch

from oracle import tf1_ops as T
from semanticsegmentation_tensorflow_amd import ops
from tests import aniso_ref
from tests.gpu_utils import assert_close, from_dev, rnd, to_dev

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DT = {torch.float32: ops.F32, torch.bfloat16: ops.BF16, torch.float16: ops.F16}

# (N, H, W, C, K), (dh, dw), padding
CASES = [
    ((1, 9, 14, 16, 24), (2, 3), "SAME"),
    ((1, 9, 14, 16, 24), (3, 1), "SAME"),
    ((1, 9, 14, 16, 24), (2, 3), "VALID"),
    # the context-module map of LidCamNet at 160 x 576 (conv8 ... conv12)
    ((1, 20, 72, 128, 128), (1, 2), "SAME"),
    ((1, 20, 72, 128, 128), (2, 4), "SAME"),
    ((1, 20, 72, 128, 128), (4, 8), "SAME"),
    ((1, 20, 72, 128, 128), (8, 16), "SAME"),
    ((1, 20, 72, 128, 128), (16, 32), "SAME"),
    # beside test_gpu_ops' "atrous halo" row: a halo family with tsh != tsw
    ((2, 30, 41, 64, 128), (2, 1), "SAME"),
]
IDS = [f"{c[0][1]}x{c[0][2]}x{c[0][3]}-{c[0][4]}-d{c[1][0]}x{c[1][1]}-{c[2]}" for c in CASES]


@functools.lru_cache(maxsize=None)
def _problem(shape, dil, pad, dtype):
    N, H, W, C, K = shape
    g = torch.Generator().manual_seed(21)
    x = rnd(torch.randn(N, H, W, C, generator=g, dtype=torch.float64), dtype).requires_grad_(True)
    w = rnd(torch.randn(3, 3, C, K, generator=g, dtype=torch.float64) / math.sqrt(9 * C), dtype).requires_grad_(True)
    b = (torch.randn(K, generator=g, dtype=torch.float64) * 0.1).float().double()
    conv = aniso_ref.conv2d(x, w, 1, pad, dil)
    dy = rnd(torch.randn(conv.shape, generator=g, dtype=torch.float64), dtype)
    (conv * dy).sum().backward()
    return x.detach(), w.detach(), b, dy, (conv + b).detach(), x.grad.detach(), w.grad.detach()


def _pack(w64, mode, dtype, dev):
    R, S, A, B = w64.shape
    dst = torch.empty(ops.packed_shape(R, S, A, B, mode), dtype=dtype, device=dev)
    return ops.pack_filter(w64.float().to(dev).contiguous(), dst, ops.round8(A), ops.round8(B), mode)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("shape,dil,pad", CASES, ids=IDS)
def test_aniso_conv_fwd_dgrad_wgrad(dev, shape, dil, pad, dtype):
    N, H, W, C, K = shape
    x, w, b, dy, y_ref, dx_ref, dw_ref = _problem(shape, dil, pad, dtype)
    d = ops.conv_desc(N, H, W, C, K, 3, 3, 1, dil, pad, DT[dtype])
    assert (d.dil_h, d.dil_w) == dil and (d.OH, d.OW) == tuple(y_ref.shape[1:3])
    fam = {op: ops.conv_kernel_info(d, op)[0] for op in (ops.OP_FWD, ops.OP_BWD_DATA, ops.OP_BWD_FILTER)}
    if shape[1:3] == (20, 72) and dil[0] >= 8 and dtype != torch.float32:
        # a (3-1)*8 x (3-1)*16 halo does not fit LDS: the implicit GEMMs
        assert fam[ops.OP_FWD].startswith("igemm_") and fam[ops.OP_BWD_DATA].startswith("igemm_"), fam
    xd, dyd = to_dev(x, dtype, dev), to_dev(dy, dtype, dev)
    # forward + bias
    y = torch.full((N, d.OH, d.OW, d.K), float("nan"), dtype=dtype, device=dev)
    ops.conv2d_fwd(d, xd, _pack(w, ops.PACK_KRSC, dtype, dev), y, ops.epilogue(bias=b.float().to(dev)))
    # input gradient
    dx = torch.full((N, H, W, d.C), float("nan"), dtype=dtype, device=dev)
    ops.conv2d_bwd_data(d, dyd, _pack(w, ops.PACK_HWIO, dtype, dev), dx)
    # filter gradient
    dw = torch.zeros(3, 3, C, K, dtype=torch.float32, device=dev)
    ops.conv2d_bwd_filter(d, xd, dyd, dw)
    torch.cuda.synchronize()
    e = [assert_close(from_dev(y, K), y_ref, dtype, f"fwd {shape} {dil} {pad} on {fam[ops.OP_FWD]}"),
         assert_close(from_dev(dx, C), dx_ref, dtype, f"dgrad {shape} {dil} {pad} on {fam[ops.OP_BWD_DATA]}"),
         assert_close(dw.double().cpu(), dw_ref, dtype, f"wgrad {shape} {dil} {pad} on {fam[ops.OP_BWD_FILTER]}")]
    print(f"{shape} {dil} {pad}: {fam} rel err {e}")
    if dil == (16, 32):
        # rows 4..15 see only the centre tap row (rows -12.. and 20.. are
        # padding), and the output there is not zero
        assert y_ref[:, 4:16].abs().max().item() > 0.1
        x2 = x.clone()
        x2[:, 4:16] = 0          # the only rows those outputs read
        y2 = aniso_ref.conv2d(x2, w, 1, pad, dil) + b
        assert torch.equal(y2[:, 4:16], b.expand_as(y2[:, 4:16]))
    if shape[1:3] == (20, 72) and dil == (1, 2):
        # not silently (1, 1) or (2, 2): both differ from the per-axis result by
        # far more than the tolerance
        got = from_dev(y, K)
        for iso in (1, 2):
            other = T.conv2d(x, w, 1, pad, iso) + b
            diff = (got - other).abs().max().item() / other.abs().max().item()
            assert diff > 0.2, (iso, diff)
