"""conv_res64pp's epilogue bodies take their wave-uniform switches (ReLU,
dropout, mask, padded channels) as compile-time constants for the usual
launches and as run-time flags otherwise.  tests/test_gpu_res64pp.py and
tests/test_gpu_relu_bits.py cover the constant forms of bias + ReLU, the
pooled forward and the masked input gradient; here are the remaining constant
form (no ReLU, no mask) and the run-time forms: a pooled forward without ReLU,
and fewer than 64 output channels (the padded-channel selects), each bit for
bit against the single-pipeline conv_res64 (res64_pp = 0), whose epilogue is
untouched.  Shapes: one tile, ragged tiles, several tiles per block."""
import pytest
import torch

from semanticsegmentation_tensorflow_amd import ops

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 32), (1, 22, 70), (3, 196, 300)]


def _both(fn):
    ops.set_option("res64_pp", 2)
    try:
        a = fn()
        ops.set_option("res64_pp", 0)
        b = fn()
    finally:
        ops.set_option("res64_pp", 1)
    torch.cuda.synchronize()
    return a, b


def _operands(dev, N, H, W, K, dtype, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(N, H, W, 64, device=dev, generator=g).to(dtype)
    w32 = torch.randn(3, 3, 64, K, device=dev, generator=g) / 24.0
    bias = torch.randn(K, device=dev, generator=g) * 0.1
    return x, w32, bias


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("K", [64, 40, 32])
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_without_relu_and_narrow(dev, shape, K, dtype):
    N, H, W = shape
    dt = ops.BF16 if dtype == torch.bfloat16 else ops.F16
    d = ops.conv_desc(N, H, W, 64, K, 3, 3, dtype=dt)
    assert ops.conv_kernel_info(d, ops.OP_FWD)[0].startswith("conv_res64")
    x, w32, bias = _operands(dev, N, H, W, K, dtype, 21)
    wk = torch.zeros(ops.packed_shape(3, 3, 64, K, ops.PACK_KRSC, 64), dtype=dtype, device=dev)
    ops.pack_filter(w32, wk, 64, K, ops.PACK_KRSC)
    ws = ops.Workspace(dev)
    for epi in (ops.epilogue(bias=bias), ops.epilogue(bias=bias, relu=True), ops.epilogue()):
        def run():
            y = torch.full((N, H, W, d.K), float("nan"), dtype=dtype, device=dev)
            ops.conv2d_fwd(d, x, wk, y, epi, ws)
            return y
        a, b = _both(run)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert bool((a.float() < 0).any())          # the last form really ran without ReLU


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[1] % 2 == 0 and s[2] % 2 == 0])
def test_pooled_forward_run_time_relu(dev, shape, relu):
    N, H, W = shape
    d = ops.conv_desc(N, H, W, 64, 64, 3, 3, dtype=ops.BF16)
    assert ops.conv2d_fwd_pool_ok(d)
    x, w32, bias = _operands(dev, N, H, W, 64, torch.bfloat16, 23)
    wk = torch.zeros(ops.packed_shape(3, 3, 64, 64, ops.PACK_KRSC, 64), dtype=torch.bfloat16, device=dev)
    ops.pack_filter(w32, wk, 64, 64, ops.PACK_KRSC)
    ws = ops.Workspace(dev)
    epi = ops.epilogue(bias=bias, relu=relu)

    def run():
        out = torch.full((N, H // 2, W // 2, 64), float("nan"), dtype=torch.bfloat16, device=dev)
        idx = torch.full((N * (H // 2) * (W // 2) * 64,), 255, dtype=torch.uint8, device=dev)
        ops.conv2d_fwd_pool(d, x, wk, out, idx, epi, ws)
        return out, idx
    (a, ai), (b, bi) = _both(run)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert torch.equal(ai, bi)
    # and the pair the fusion replaces
    y = torch.empty(N, H, W, 64, dtype=torch.bfloat16, device=dev)
    ops.conv2d_fwd(d, x, wk, y, epi, ws)
    ref, ref_idx = torch.empty_like(a), torch.empty_like(ai)
    ops.maxpool2x2_fwd_argmax(y, ref, ref_idx)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int16), ref.view(torch.int16))
    assert torch.equal(ai, ref_idx)
    assert relu or bool((a.float() < 0).any())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_input_gradient_without_mask(dev, shape, dtype):
    N, H, W = shape
    dt = ops.BF16 if dtype == torch.bfloat16 else ops.F16
    d = ops.conv_desc(N, H, W, 64, 64, 3, 3, dtype=dt)
    assert ops.conv_kernel_info(d, ops.OP_BWD_DATA)[0].startswith("conv_res64")
    dy, w32, _ = _operands(dev, N, H, W, 64, dtype, 25)
    wh = torch.zeros(ops.packed_shape(3, 3, 64, 64, ops.PACK_HWIO, 64), dtype=dtype, device=dev)
    ops.pack_filter(w32, wh, 64, 64, ops.PACK_HWIO)
    ws = ops.Workspace(dev)

    def run():
        dx = torch.full((N, H, W, 64), float("nan"), dtype=dtype, device=dev)
        ops.conv2d_bwd_data(d, dy, wh, dx, ws, None, None)
        return dx
    a, b = _both(run)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
