"""Edge-case parity of the small kernels in csrc/eltwise.hip -- the loss
(xent_k / sum_k), the prediction (softmax_k, argmax_k, confusion_k), the
optimizer step (adam_k), the loss-scale overflow check (check_finite_k) and the
graph's glue ops (add / fill / cast / copy_channels / prepare_input from uint8 /
spatial reduce and broadcast) -- through the C-ABI wrappers of ops.py.

Every reference is computed on the CPU in float64 from the inputs as the device
sees them (`rnd`: rounded through the compute dtype), with oracle/tf1_ops.py
where it has the op and plain torch otherwise.  Tolerances are the project's:
TOL[dtype] of tests/gpu_utils.py in the max-relative norm, 1e-5 * max(1, |loss|)
on the mean loss (test_softmax_xent), 1e-5 absolute for the fp32 softmax
(test_gpu_eval.py), 1e-6 for Adam (test_adam_tf1), 1e-5 / 4e-3 for the fp32 /
bf16 spatial reduce (test_gpu_ops_r2.py).  The glue ops are bit-exact.

Grid-stride cases: seg_grid_1d(n, 256, cap) launches min(cap, ceil(n / 256))
blocks of 256 threads, so a kernel's loop takes a second pass once n exceeds
cap * 256 work items.  Each large shape below is the smallest that gets there;
the comment next to it derives the pass count from the launch's cap.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import tf1_ops as tf
from semanticsegmentation_tensorflow_amd import ops
from tests.gpu_utils import TOL, assert_close, from_dev, rnd, to_dev

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DT_IDS = ["f32", "bf16", "f16"]
_INT_OF = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _slice_view(x, dtype, dev, extra=16, lead=8, junk=50.0):
    """float64 NHWC -> a channel-slice view [.., round8(C)] of a device buffer
    whose pixel stride is round8(C) + extra; everything outside the view holds
    `junk`, the view's own padding channels hold zeros (as to_dev)."""
    N, H, W, C = x.shape
    cp = ops.round8(C)
    assert lead % 8 == 0 and lead <= extra
    buf = torch.full((N, H, W, cp + extra), junk, dtype=dtype, device=dev)
    view = buf[..., lead:lead + cp]
    view.zero_()
    view[..., :C] = x.to(dtype).to(dev)
    assert ops.pixel_stride(view) == cp + extra
    return view


def _assert_bits_equal(got, ref, what=""):
    """Bit-for-bit (so -0.0 != +0.0), NaN compared by position, not by payload."""
    got, ref = got.cpu().reshape(-1), ref.cpu().reshape(-1)
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    gn, rn = torch.isnan(got), torch.isnan(ref)
    assert torch.equal(gn, rn), f"{what}: NaN positions differ"
    it = _INT_OF[got.dtype]
    gb, rb = got.view(it)[~gn], ref.view(it)[~rn]
    bad = (gb != rb).nonzero().reshape(-1)
    assert bad.numel() == 0, (f"{what}: {bad.numel()} elements differ, first at {bad[0].item()}: "
                              f"{got[~gn][bad[0]].item()!r} vs {ref[~rn][bad[0]].item()!r}")


# ---------------------------------------------------------------------------
# 1. softmax cross-entropy: xent_k + sum_k
# ---------------------------------------------------------------------------
def _valid_mask(N, H, W, valid):
    mask = torch.zeros(N, H, W, dtype=torch.float64)
    mask[:, :valid[0], :valid[1]] = 1
    return mask


def _xent_reference(z, y, valid):
    """Masked mean loss and its gradient, float64.  z: rounded logits, y: the
    label distribution the device reads (fp32 values, widened)."""
    N, H, W, _ = z.shape
    zz = z.clone().requires_grad_(True)
    loss = tf.mean_softmax_xent(zz, y, _valid_mask(N, H, W, valid))
    loss.backward()
    return loss.item(), zz.grad


def _labels(kind, idx, C, soft=None):
    """(device-side label tensor on the CPU, float64 distribution of the reference)."""
    if kind == "index":
        return idx.to(torch.uint8), tf.one_hot(idx, C)
    y32 = (tf.one_hot(idx, C) if soft is None else soft).float().contiguous()
    return y32, y32.double()


def _check_xent(dev, z, lab_cpu, y_ref, C, dtype, valid, wide=False, nan_outside=False, split_at=None):
    """Run ops.softmax_xent on rounded logits z [N,H,W,C] (float64) and compare
    the loss, dlogits, the padding channels and the region outside `valid`."""
    N, H, W, _ = z.shape
    vh, vw = valid
    loss_ref, g_ref = _xent_reference(z, y_ref, valid)
    zdev = z.clone()
    if nan_outside:                       # the reference never sees these: the mask removes them
        zdev[:, vh:] = float("nan")
        zdev[:, :, vw:] = float("nan")
    zd = _slice_view(zdev, dtype, dev) if wide else to_dev(zdev, dtype, dev)
    dz = torch.full((N, H, W, ops.round8(C)), float("nan"), dtype=dtype, device=dev)
    if wide:
        assert ops.pixel_stride(zd) != ops.pixel_stride(dz)
    ls = torch.zeros(1, dtype=torch.float32, device=dev)
    cnt = N * vh * vw
    ops.softmax_xent(zd, lab_cpu.to(dev), dz, ls, C, valid, grad_scale=1.0 / cnt)
    torch.cuda.synchronize()
    got_loss = ls.item() / cnt
    got = from_dev(dz, C)
    print(f"xent C={C} {dtype}: loss {got_loss:.8g} vs {loss_ref:.8g}, "
          f"|dlogits| max {g_ref.abs().max().item():.3e}")
    assert np.isfinite(got_loss) and torch.isfinite(dz.float()).all()
    assert abs(got_loss - loss_ref) <= 1e-5 * max(1.0, abs(loss_ref))
    assert_close(got, g_ref, dtype, "dlogits")
    if split_at is not None:              # the pixels of the second grid-stride pass on their own
        assert_close(got.reshape(-1, C)[split_at:], g_ref.reshape(-1, C)[split_at:], dtype, "dlogits, second pass")
    if ops.round8(C) > C:
        assert dz[..., C:].abs().max().item() == 0
    if vh < H:
        assert dz[:, vh:].abs().max().item() == 0
    if vw < W:
        assert dz[:, :, vw:].abs().max().item() == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind", ["index", "onehot"])
@pytest.mark.parametrize("C", [1, 2, 3, 8, 9, 16])
def test_xent_class_count_sweep(dev, dtype, kind, C):
    """C = 1 .. XENT_MAXC: loss, gradient, zeros in [C, ld_d), and an exactly
    zero gradient outside the valid region even where the logits are NaN."""
    N, H, W = 2, 12, 16
    g = _gen(100 + C)
    z = rnd(torch.randn(N, H, W, C, generator=g, dtype=torch.float64) * 3, dtype)
    idx = torch.randint(0, C, (N, H, W), generator=g)
    lab, y = _labels(kind, idx, C)
    _check_xent(dev, z, lab, y, C, dtype, (10, 13), nan_outside=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind", ["index", "onehot"])
def test_xent_rejects_more_than_16_classes(dev, dtype, kind):
    N, H, W, C = 1, 4, 5, 17
    g = _gen(117)
    zd = to_dev(torch.randn(N, H, W, C, generator=g, dtype=torch.float64), dtype, dev)
    idx = torch.randint(0, C, (N, H, W), generator=g)
    lab, _ = _labels(kind, idx, C)
    dz = torch.full_like(zd, float("nan"))
    ls = torch.zeros(1, dtype=torch.float32, device=dev)
    with pytest.raises(RuntimeError, match=r"invalid argument \(status 1\)"):     # SEG_EINVAL
        ops.softmax_xent(zd, lab.to(dev), dz, ls, C)
    torch.cuda.synchronize()
    assert torch.isnan(dz).all()
    assert ls.item() == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind", ["index", "onehot"])
@pytest.mark.parametrize("C", [2, 9])
def test_xent_logits_slice_view(dev, dtype, kind, C):
    """ld = round8(C) + 16 (a channel slice of a wider buffer filled with 50s),
    dlogits dense: ld != ld_d."""
    N, H, W = 2, 12, 16
    g = _gen(200 + C)
    z = rnd(torch.randn(N, H, W, C, generator=g, dtype=torch.float64) * 3, dtype)
    idx = torch.randint(0, C, (N, H, W), generator=g)
    lab, y = _labels(kind, idx, C)
    _check_xent(dev, z, lab, y, C, dtype, (10, 13), wide=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("C", [2, 9])
def test_xent_soft_labels_on_the_simplex(dev, dtype, C):
    """Labels that are not one-hot but sum to 1: 0.9 / 0.1 smoothing for C = 2,
    a random simplex point per pixel for C = 9.  The kernel's gradient is
    softmax * sum(y) - y, TensorFlow's is softmax - y; they agree when
    sum(y) = 1.  Unnormalised labels differ, but the reference never feeds them
    (its labels are one-hot), so they are not tested."""
    N, H, W = 2, 12, 16
    g = _gen(300 + C)
    z = rnd(torch.randn(N, H, W, C, generator=g, dtype=torch.float64) * 3, dtype)
    idx = torch.randint(0, C, (N, H, W), generator=g)
    if C == 2:
        soft = tf.one_hot(idx, C) * 0.8 + 0.1
    else:
        e = -torch.log(torch.rand(N, H, W, C, generator=g, dtype=torch.float64))
        soft = e / e.sum(-1, keepdim=True)
    lab, y = _labels("soft", idx, C, soft)
    assert (y.sum(-1) - 1).abs().max().item() < 1e-6 and (y.max(-1).values < 0.95).all()
    _check_xent(dev, z, lab, y, C, dtype, (10, 13))


_EXTREME = {torch.float32: 1e4, torch.bfloat16: 3e4, torch.float16: 6e4}


def _extreme_logits(N, H, W, C, dtype, seed):
    """Scale-40 logits with single entries at +-big (the largest magnitudes the
    dtype's range comfortably holds), and labels that are confidently wrong on
    about half the pixels (the least likely class), so the loss is a sum of
    large terms rather than of zeros."""
    g = _gen(seed)
    z = torch.randn(N, H, W, C, generator=g, dtype=torch.float64) * 40
    big = _EXTREME[dtype]
    flat = z.view(-1, C)
    P = flat.shape[0]
    for i, p in enumerate(range(3, P, 7)):
        flat[p, (i // 2) % C] = big if i % 2 == 0 else -big
    z = rnd(z, dtype)
    assert torch.isfinite(z).all()
    wrong = torch.rand(N, H, W, generator=g) < 0.5
    idx = torch.where(wrong, z.argmin(-1), z.argmax(-1))
    return z, idx


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind", ["index", "onehot"])
@pytest.mark.parametrize("C", [2, 9])
def test_xent_extreme_logits(dev, dtype, kind, C):
    """The max-subtraction has to carry these: exp(z) alone overflows fp32."""
    N, H, W = 2, 12, 16
    z, idx = _extreme_logits(N, H, W, C, dtype, 400 + C)
    lab, y = _labels(kind, idx, C)
    _check_xent(dev, z, lab, y, C, dtype, (10, 13))


# xent_launch: seg_grid_1d(P, 256, 2048) -> at most 2048 blocks of 256 threads,
# one pixel per thread and pass, so pixels >= 2048 * 256 = 524,288 are reached
# only by the second pass of the loop.  P = 520 * 1010 = 525,200 > 524,288: 912
# pixels in the second pass, and sum_k reduces 2048 partials (> 256: eight per
# thread in its strided pre-sum).
XENT_BIG = (1, 520, 1010, 2)
XENT_PASS1 = 2048 * 256


@functools.lru_cache(maxsize=None)
def _xent_big_inputs(dtype):
    N, H, W, C = XENT_BIG
    assert N * H * W > XENT_PASS1
    g = _gen(500)
    z = torch.randn(N, H, W, C, generator=g, dtype=torch.float64) * 3
    z.view(-1, C)[XENT_PASS1:, 1] += 2.0        # the second pass has its own distribution
    idx = torch.randint(0, C, (N, H, W), generator=g)
    return rnd(z, dtype), idx


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["index", "onehot"])
@pytest.mark.parametrize("valid", [(517, 1003), (520, 1010)], ids=["valid517x1003", "all_valid"])
def test_xent_grid_stride_and_wide_reduction(dev, dtype, kind, valid):
    """The second-pass pixels (>= 524,288) all lie in image row 519.  With the
    valid region (517, 1003) that row is masked, so a dropped second pass shows
    in dlogits only (NaN left where exact zeros belong); with the whole image
    valid it shows in the loss and in the gradient values as well."""
    N, H, W, C = XENT_BIG
    z, idx = _xent_big_inputs(dtype)
    lab, y = _labels(kind, idx, C)
    _check_xent(dev, z, lab, y, C, dtype, valid, split_at=XENT_PASS1)


# ---------------------------------------------------------------------------
# 2. softmax, argmax, confusion
# ---------------------------------------------------------------------------
def _check_softmax(dev, z, C, dtype, view, split_at=None):
    N, H, W, _ = z.shape
    ref = torch.softmax(z, dim=-1)
    xd = _slice_view(z, dtype, dev) if view else to_dev(z, dtype, dev)
    y = torch.full((N, H, W, ops.round8(C)), float("nan"), dtype=dtype, device=dev)
    ops.softmax(xd, y, C)
    torch.cuda.synchronize()
    got = from_dev(y, C)
    err = (got - ref).abs().max().item()
    print(f"softmax C={C} {dtype}: max abs err {err:.3e}")
    assert torch.isfinite(y.float()).all()
    parts = [(got, ref, "softmax")]
    if split_at is not None:
        parts.append((got.reshape(-1, C)[split_at:], ref.reshape(-1, C)[split_at:], "softmax, second pass"))
    for a, b, what in parts:
        if dtype == torch.float32:
            assert (a - b).abs().max().item() < 1e-5, what
        else:
            assert_close(a, b, dtype, what)
    if ops.round8(C) > C:
        assert y[..., C:].abs().max().item() == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("view", [False, True], ids=["dense", "slice"])
@pytest.mark.parametrize("C", [2, 9, 16])
def test_softmax(dev, dtype, view, C):
    z = rnd(torch.randn(2, 9, 31, C, generator=_gen(600 + C), dtype=torch.float64) * 3, dtype)
    _check_softmax(dev, z, C, dtype, view)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_softmax_extreme_logits(dev, dtype):
    z, _ = _extreme_logits(2, 12, 16, 9, dtype, 409)
    _check_softmax(dev, z, 9, dtype, False)


# seg_softmax / seg_argmax: seg_grid_1d(P, 256) with the default cap of 2048 * 8
# = 16384 blocks of 256 threads, one pixel per thread and pass, so pixels >=
# 16384 * 256 = 4,194,304 belong to the second pass.  P = 2048 * 2049 =
# 4,196,352: the last 2,048 pixels.
PRED_BIG = (1, 2048, 2049, 2)
PRED_PASS1 = 16384 * 256


@functools.lru_cache(maxsize=None)
def _pred_big_logits():
    N, H, W, C = PRED_BIG
    assert N * H * W - PRED_PASS1 == 2048
    z = torch.randn(N, H, W, C, generator=_gen(700), dtype=torch.float64)
    z.view(-1, C)[PRED_PASS1:, 0] += 3.0        # the second pass: class 0 favoured, elsewhere even odds
    return rnd(z, torch.bfloat16)


def test_softmax_grid_stride(dev):
    _check_softmax(dev, _pred_big_logits(), 2, torch.bfloat16, False, split_at=PRED_PASS1)


def _check_argmax(dev, z, C, dtype, view):
    """z: rounded float64 logits; exact equality with tf.argmax of them."""
    N, H, W, _ = z.shape
    zd = _slice_view(z, dtype, dev) if view else to_dev(z, dtype, dev)
    pred = torch.full((N * H * W,), -1, dtype=torch.int64, device=dev)
    ops.argmax(zd, pred, C)
    torch.cuda.synchronize()
    got = pred.cpu().view(N, H, W)
    ref = tf.argmax(z)
    assert torch.equal(got, ref), f"{(got != ref).sum().item()} of {ref.numel()} pixels differ"
    return got


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("view", [False, True], ids=["dense", "slice"])
@pytest.mark.parametrize("C", [2, 9, 16])
def test_argmax_ties_take_the_lowest_index(dev, dtype, view, C):
    """Ties made by rounding: `hi` and `hi * (1 + eps / 8)` differ in float64 and
    are the same number in the compute dtype."""
    N, H, W = 2, 9, 31
    g = _gen(800 + C)
    z = torch.randn(N, H, W, C, generator=g, dtype=torch.float64)
    hi, hi2 = 5.0, 5.0 * (1 + torch.finfo(dtype).eps / 8)
    mid, last = C // 2, C - 1
    flat = z.view(-1, C)
    flat[0, 0], flat[0, last] = hi, hi2            # first and last channel tie -> 0
    flat[1, 0], flat[1, last] = hi2, hi            # the same, unrounded order swapped -> 0
    flat[2, mid], flat[2, last] = hi, hi2          # a middle channel and the last tie -> mid
    flat[3, :] = hi                                # every channel ties -> 0
    flat[4, :] = hi
    flat[4, last] = hi2                            # ... also when the last is larger before rounding -> 0
    flat[5, last] = hi                             # the last channel alone is the maximum -> last
    flat[6, 1:] = hi2                              # everything but the first ties -> 1
    z = rnd(z, dtype)
    assert z.view(-1, C)[0, 0] == z.view(-1, C)[0, last] and z.view(-1, C)[4, last] == hi
    got = _check_argmax(dev, z, C, dtype, view).view(-1)
    assert got[:7].tolist() == [0, 0, mid, 0, 0, last, 1]


def test_argmax_grid_stride(dev):
    got = _check_argmax(dev, _pred_big_logits(), 2, torch.bfloat16, False).view(-1)
    assert (got[PRED_PASS1:] >= 0).all() and got[PRED_PASS1:].float().mean().item() < 0.1


def _conf_reference(pred, lab, C, valid):
    """Host bincount over the valid region of (label, prediction) pairs with
    both members in [0, C)."""
    p = pred.view(lab.shape)[:, :valid[0], :valid[1]].reshape(-1)
    t = lab[:, :valid[0], :valid[1]].reshape(-1).long()
    keep = (t < C) & (p >= 0) & (p < C)
    return torch.bincount(t[keep] * C + p[keep], minlength=C * C)


@pytest.mark.parametrize("C", [2, 5])
def test_confusion_counts_accumulate(dev, C):
    N, H, W, valid = 2, 9, 31, (7, 29)
    g = _gen(900 + C)
    lab = torch.randint(0, C, (N, H, W), generator=g, dtype=torch.uint8)
    lab[torch.rand(N, H, W, generator=g) < 0.2] = 255          # ignored label
    conf = torch.zeros(C * C, dtype=torch.int64, device=dev)
    ref = torch.zeros(C * C, dtype=torch.int64)
    for call in range(2):
        pred = torch.randint(0, C + 2, (N * H * W,), generator=g)     # C, C + 1: no class, ignored
        ops.confusion(pred.to(dev), lab.to(dev), conf, C, valid)
        torch.cuda.synchronize()
        ref += _conf_reference(pred, lab, C, valid)
        assert torch.equal(conf.cpu(), ref), f"after call {call + 1}"
    assert ref.sum().item() > 0 and (ref > 0).all()


@pytest.mark.parametrize("C", [2, 5])
def test_confusion_ignores_predictions_that_are_no_class(dev, C):
    """int64 predictions that are negative, or >= 2^31 with a low word that
    reads as a class (or as a small negative), count nowhere.  They sit only at
    pixels whose label is >= 1, and their low words lie in [-C, C): a kernel
    that compares the truncated value and does not require q >= 0 miscounts
    them in cells of the matrix, never outside it."""
    N, H, W, valid = 2, 9, 31, (7, 29)
    g = _gen(950 + C)
    lab = torch.randint(0, C, (N, H, W), generator=g, dtype=torch.uint8)
    lab[torch.rand(N, H, W, generator=g) < 0.1] = 255
    pred = torch.randint(0, C, (N * H * W,), generator=g)
    bad = [-1, -C, 2 ** 32, 2 ** 32 + 1, 2 ** 33 + C - 1, -2 ** 32 + 1, 2 ** 63 - 1, 2 ** 40 - 1, C, 255]
    low = [((b + 2 ** 31) % 2 ** 32) - 2 ** 31 for b in bad]                # (int)b
    assert all(-C <= w < C or 0 <= b < 2 ** 31 for b, w in zip(bad, low))
    labf = lab.view(-1)
    spots = ((labf >= 1) & (labf < C)).nonzero().reshape(-1)
    vmask = _valid_mask(N, H, W, valid).view(-1) > 0
    spots = spots[vmask[spots]]                     # inside the valid region, where they would count
    assert spots.numel() >= 4 * len(bad)
    for i, s in enumerate(spots[:4 * len(bad)].tolist()):
        pred[s] = bad[i % len(bad)]
    conf = torch.zeros(C * C, dtype=torch.int64, device=dev)
    ops.confusion(pred.to(dev), lab.to(dev), conf, C, valid)
    torch.cuda.synchronize()
    assert torch.equal(conf.cpu(), _conf_reference(pred, lab, C, valid))


# ---------------------------------------------------------------------------
# 3. overflow check and Adam
# ---------------------------------------------------------------------------
# seg_check_finite: seg_grid_1d(n / 4 + 1, 256, 4096) -> at most 4096 blocks of
# 256 threads, one float4 per thread and pass: 4096 * 256 * 4 = 4,194,304 floats
# per pass.  n = 8,388,615 = 2 * 4,194,304 + 7: two full passes, one more float4
# for thread 0's third pass (elements 8,388,608 .. 8,388,611) and a scalar tail
# of 3.  Element 4,194,304 + 5 is read in the second pass.
FINITE_PASS = 4096 * 256 * 4
FINITE_SIZES = [1, 3, 4, 5, 1027, 2 * FINITE_PASS + 7]


def _flag_of(g, flag):
    ops.check_finite(g, flag)
    torch.cuda.synchronize()
    return flag.item()


@pytest.mark.parametrize("n", FINITE_SIZES)
def test_check_finite(dev, n):
    assert n == 8_388_615 or n <= 1027
    x = torch.randn(n, generator=_gen(1000)).to(dev)
    assert x.data_ptr() % 16 == 0
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    assert _flag_of(x, flag) == 0
    flag.fill_(1)                                   # a stale flag of a skipped step is reset
    assert _flag_of(x, flag) == 0
    n4 = n // 4
    spots = {0, n - 1}                              # n - 1: inside the scalar tail when n % 4 != 0
    if n4:
        spots |= {4 * n4 - 1, 4 * n4 - 4}           # the last float4, both ends
    if n > FINITE_PASS + 5:
        spots |= {FINITE_PASS + 5, 2 * FINITE_PASS - 1, 2 * FINITE_PASS}
    for i in sorted(spots):
        keep = x[i].clone()
        for bad in (float("inf"), float("-inf"), float("nan")):
            x[i] = bad
            assert _flag_of(x, flag) == 1, f"n = {n}: {bad} at {i} not seen"
        x[i] = keep
        assert _flag_of(x, flag) == 0, f"n = {n}: flag stuck after {i}"


@pytest.mark.parametrize("n", [1, 4, 7, 1027])
def test_check_finite_accepts_every_finite_value(dev, n):
    """The largest finite magnitudes, denormals and -0.0 are no overflow."""
    vals = torch.tensor([3.4e38, -3.4e38, 1e-45, -1e-40, -0.0, 1.1754942e-38, 0.0], dtype=torch.float32)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    for shift in range(len(vals)):
        x = vals.roll(shift).repeat(n // len(vals) + 1)[:n].contiguous().to(dev)
        assert torch.isfinite(x).all()
        assert _flag_of(x, flag) == 0, f"n = {n}, shift {shift}"


# Hyper-parameters as the kernel receives them (C floats); the reference runs
# on the same values in float64, as it runs on the rounded tensors.  (With the
# double 0.999 instead, 1 - beta2 alone differs by 1.3e-5 relative, which is a
# difference of the inputs, not of the arithmetic.)
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS = (float(np.float32(v)) for v in (1e-3, 0.9, 0.999, 1e-8))
ADAM_GS = 2.0


def _adam_run(dev, p0, grads):
    """Device trajectory and float64 tf.AdamTF1 trajectory over `grads` (fp32)."""
    opt = tf.AdamTF1(lr=ADAM_LR, beta1=ADAM_B1, beta2=ADAM_B2, eps=ADAM_EPS)
    params = {"p": p0.double()}
    pd = p0.to(dev)
    m = torch.zeros_like(pd)
    v = torch.zeros_like(pd)
    for t, gr in enumerate(grads, 1):
        params = opt.apply(params, {"p": gr.double() * ADAM_GS})
        ops.adam_tf1_step(pd, gr.to(dev), m, v, ADAM_LR, t, beta1=ADAM_B1, beta2=ADAM_B2, eps=ADAM_EPS,
                          grad_scale=ADAM_GS)
    torch.cuda.synchronize()
    return (pd.cpu(), m.cpu(), v.cpu()), (params["p"], opt.m["p"], opt.v["p"])


def _adam_grads(n, steps, shift, g):
    """Element i's gradient class is (i + shift) % 3: exactly zero in every
    step, of size 1e-12, of size 1e3."""
    cls = (torch.arange(n) + shift) % 3
    scale = torch.tensor([0.0, 1e-12, 1e3])[cls]
    return cls, [(torch.randn(n, generator=g) * scale).float() for _ in range(steps)]


@pytest.mark.parametrize("n", [1, 3, 4, 1024])
def test_adam_small_sizes_and_gradient_scales(dev, n):
    """n < 4 (scalar tail only), n % 4 == 0 (no tail); zero gradients with
    v = 0 leave p unchanged bit for bit (0 / (sqrt(0) + eps) = 0)."""
    g = _gen(1100 + n)
    for shift in range(3):                          # every class reaches every position (n = 1 included)
        p0 = torch.randn(n, generator=g)
        cls, grads = _adam_grads(n, 3, shift, g)
        (p, m, v), (pr, mr, vr) = _adam_run(dev, p0, grads)
        assert_close(p.double(), pr, torch.float32, "adam p", 1e-6)
        for c in range(3):                          # small classes must not hide under the 1e3 one
            sel = cls == c
            if sel.any():
                assert_close(p[sel].double(), pr[sel], torch.float32, f"adam p, class {c}", 1e-6)
                # m is a running mix of gradients of either sign: its rounding error scales with the
                # largest term (max |grad_scale * g| of the class), not with a sum that may have cancelled
                gmax = max(gr[sel].abs().max().item() for gr in grads) * ADAM_GS
                assert (m[sel].double() - mr[sel]).abs().max().item() <= 1e-6 * gmax, f"adam m, class {c}"
                assert_close(v[sel].double(), vr[sel], torch.float32, f"adam v, class {c}", 1e-6)
        zero = cls == 0
        assert torch.equal(p[zero], p0[zero]) and (m[zero] == 0).all() and (v[zero] == 0).all()


# seg_adam_tf1_step: seg_grid_1d(n / 4 + 1, 256) with the default cap of 16384
# blocks of 256 threads, one float4 per thread and pass: 16384 * 256 * 4 =
# 16,777,216 floats per pass.  n = 16,777,216 + 1027: 1024 floats (256 float4)
# in the second pass and a scalar tail of 3.
ADAM_PASS = 16384 * 256 * 4


def test_adam_grid_stride(dev):
    n = ADAM_PASS + 1027
    g = _gen(1200)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * 1e-3 for _ in range(2)]
    for gr in grads:
        gr[ADAM_PASS:] *= 7.0                       # the second pass and the tail on their own scale
    got, ref = _adam_run(dev, p0, grads)
    for a, b, what in zip(got, ref, "pmv"):
        assert_close(a.double(), b, torch.float32, f"adam {what}", 1e-6)
        assert_close(a[ADAM_PASS:].double(), b[ADAM_PASS:], torch.float32, f"adam {what}, second pass", 1e-6)
        assert_close(a[-3:].double(), b[-3:], torch.float32, f"adam {what}, scalar tail", 1e-6)


# ---------------------------------------------------------------------------
# 4. glue ops (bit-exact)
# ---------------------------------------------------------------------------
# seg_add / seg_fill / seg_cast: seg_grid_1d(n, 256), default cap 16384 blocks of
# 256 threads, one element per thread and pass: elements >= 16384 * 256 =
# 4,194,304 belong to the second pass.  n = 4,194,304 + 1001.
ELT_PASS = 16384 * 256
ELT_SIZES = [1, 255, ELT_PASS + 1001]

_SPECIALS = [
    0.0, -0.0, 1.0, -1.0, float("inf"), float("-inf"), float("nan"),
    # fp32 -> bf16 halfway cases (8 significand bits): ties to even, both directions
    1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -23, 1 + 2.0 ** -8 - 2.0 ** -24,
    # fp32 -> fp16 halfway cases (11 significand bits)
    1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 3 * 2.0 ** -11), 1 + 2.0 ** -11 + 2.0 ** -23,
    # fp16 overflow: 65504 is the largest half, 65520 the halfway point that rounds to inf
    65504.0, 65519.0, 65520.0, -65520.0, 65536.0, 1e5,
    # the largest bf16 (0x7f7f), the largest fp32 (rounds to bf16 inf), just below the bf16 overflow tie
    3.3895313892515355e38, -3.3895313892515355e38, 3.4028234663852886e38, 3.396e38,
    # denormals: fp32 (also bf16 denormals), fp16 (2^-24 the smallest; 2^-25 ties to zero, 3 * 2^-25 to even)
    1e-45, -1e-45, 1e-40, 1.1754942e-38, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, -(2.0 ** -25), 2.0 ** -26, 6.1e-5,
    2.0 ** -133, 2.0 ** -134, 3 * 2.0 ** -134,
]


def _cast_source(n, src_dtype):
    """fp32 values holding the specials at both ends (so also in the second pass
    of the large size), sign- and scale-mixed randoms between; then rounded to
    the source dtype on the host."""
    g = _gen(1300 + n % 1000)
    x = torch.randn(n, generator=g) * torch.pow(10.0, torch.randint(-8, 9, (n,), generator=g).float() / 2)
    s = torch.tensor(_SPECIALS, dtype=torch.float32)
    k = min(n, len(s))
    x[:k] = s[:k]
    if n > 2 * len(s):
        x[-len(s):] = s.flip(0)
    return x.to(src_dtype)


CAST_PAIRS = [(torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32), (torch.float32, torch.float32),
              (torch.bfloat16, torch.bfloat16), (torch.float32, torch.float16), (torch.float16, torch.float32),
              (torch.float16, torch.float16)]


@pytest.mark.parametrize("n", ELT_SIZES)
@pytest.mark.parametrize("pair", CAST_PAIRS, ids=lambda p: f"{p[0]}-{p[1]}".replace("torch.", ""))
def test_cast_matches_host_rounding(dev, pair, n):
    src, dst = pair
    if n == 1:                                      # every special value as its own one-element cast
        xs = [torch.tensor([v], dtype=torch.float32).to(src) for v in _SPECIALS]
    else:
        xs = [_cast_source(n, src)]
    for x in xs:
        y = torch.full((x.numel(),), 7.0, dtype=dst, device=dev)
        ops.cast(x.to(dev), y)
        torch.cuda.synchronize()
        _assert_bits_equal(y, x.to(dst), f"cast {src} -> {dst} of {x[0].item()!r} ..")


def _add_operands(n, dtype, seed):
    g = _gen(seed)
    big = {torch.float32: 3e38, torch.bfloat16: 3e38, torch.float16: 6e4}[dtype]
    a = torch.randn(n, generator=g) * 3
    b = torch.randn(n, generator=g) * 3
    k = min(n, 8)
    # overflow to +-inf, cancellation to +0, signed zeros, denormals, 1 + 2^-8 (a bf16 rounding tie)
    a[:k] = torch.tensor([big, -big, 1.0, 0.0, -0.0, 1e-40, 1.0, 2.0 ** -24])[:k]
    b[:k] = torch.tensor([big, -big, -1.0, -0.0, -0.0, 1e-40, 2.0 ** -8, 2.0 ** -24])[:k]
    if n > 16:
        a[-8:], b[-8:] = a[:8].clone(), b[:8].clone()
    return a.to(dtype), b.to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", ELT_SIZES)
def test_add(dev, dtype, n):
    a, b = _add_operands(n, dtype, 1400)
    ref = (a.float() + b.float()).to(dtype)
    y = torch.full((n,), 7.0, dtype=dtype, device=dev)
    ops.add(a.to(dev), b.to(dev), y)
    torch.cuda.synchronize()
    _assert_bits_equal(y, ref, "add")
    acc = a.to(dev)                                 # the in-place form of the session's gradient accumulation
    ops.add(acc, b.to(dev), acc)
    torch.cuda.synchronize()
    _assert_bits_equal(acc, ref, "add in place")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", ELT_SIZES)
def test_fill(dev, dtype, n):
    for value in (0.0, -1.5, 1e-3):                 # 1e-3 is not representable: the rounded value is expected
        y = torch.full((n + 8,), 7.0, dtype=dtype, device=dev)
        ops.fill(y[:n], value)
        torch.cuda.synchronize()
        ref = torch.full((n,), value, dtype=torch.float32).to(dtype)
        _assert_bits_equal(y[:n], ref, f"fill {value}")
        assert (y[n:] == 7.0).all(), "fill wrote past n"


def _check_copy_channels(dev, dtype, N, H, W, C, src_w, src_off, dst_w, dst_off):
    g = _gen(1500)
    src = torch.randn(N, H, W, src_w, generator=g).to(dtype)
    dst0 = torch.randn(N, H, W, dst_w, generator=g).to(dtype)           # sentinels: every value distinct
    sd, dd = src.to(dev), dst0.to(dev)
    ops.copy_channels(sd[..., src_off:src_off + C], dd[..., dst_off:dst_off + C])
    torch.cuda.synchronize()
    want = dst0.clone()
    want[..., dst_off:dst_off + C] = src[..., src_off:src_off + C]
    _assert_bits_equal(dd, want, "copy_channels")
    _assert_bits_equal(sd, src, "copy_channels source")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_copy_channels_between_slice_views(dev, dtype):
    """Source and destination both channel slices, of buffers of different
    widths, at non-zero offsets; 3 (16-bit) or 6 (fp32) chunks per pixel."""
    _check_copy_channels(dev, dtype, 2, 5, 7, 24, src_w=48, src_off=8, dst_w=64, dst_off=32)


def test_copy_channels_grid_stride(dev):
    # seg_copy_channels: seg_grid_1d(P * C / 8, 256) for bf16, default cap 16384
    # blocks of 256 threads, one 16-byte chunk per thread and pass: chunks >=
    # 4,194,304 belong to the second pass.  P = 70,000 pixels of C = 512: 64
    # chunks per pixel, 4,480,000 chunks.
    assert 250 * 280 * (512 // 8) > 16384 * 256
    _check_copy_channels(dev, torch.bfloat16, 1, 250, 280, 512, src_w=520, src_off=8, dst_w=528, dst_off=0)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", [(2, 5, 7, 3, 8, 8, 8), (1, 4, 4, 8, 4, 6, 8), (1, 3, 5, 11, 4, 5, 16)])
def test_prepare_input_from_uint8(dev, dtype, shape):
    """uint8 NHWC image -> zero-padded compute tensor: exactly the cast."""
    N, H, W, c, HP, WP, CP = shape
    img = torch.randint(0, 256, (N, H, W, c), generator=_gen(1600), dtype=torch.uint8)
    img.view(-1)[:2] = torch.tensor([0, 255], dtype=torch.uint8)
    ref = torch.zeros(N, HP, WP, CP)
    ref[:, :H, :W, :c] = img.float()
    x = torch.full((N, HP, WP, CP), float("nan"), device=dev, dtype=dtype)
    ops.prepare_input(img.to(dev), x)
    torch.cuda.synchronize()
    _assert_bits_equal(x, ref.to(dtype), "prepare_input")


SPATIAL_TOL = {torch.float32: 1e-5, torch.bfloat16: 4e-3, torch.float16: TOL[torch.float16]}


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("view", [False, True], ids=["dense", "slice"])
@pytest.mark.parametrize("shape", [(2, 7, 9, 8), (3, 1, 1, 24), (2, 33, 5, 24), (1, 40, 50, 24)])
def test_spatial_reduce(dev, dtype, view, shape):
    """Mean and sum over H x W against a float64 sum of the rounded input; C = 24
    gives 3 (16-bit) or 6 (fp32) chunks, neither of which divides the block's 256
    threads; 40 x 50 pixels spread over 8 blocks whose partial sums are added
    atomically; the slice view has ldx = C + 16."""
    N, H, W, C = shape
    x = rnd(torch.randn(N, H, W, C, generator=_gen(1700), dtype=torch.float64), dtype)
    xd = _slice_view(x, dtype, dev) if view else to_dev(x, dtype, dev)
    assert xd.shape[-1] == C
    y = torch.full((N, 1, 1, C), float("nan"), device=dev, dtype=dtype)
    ws = ops.Workspace(dev)
    for scale in (1.0 / (H * W), 1.0):
        ops.spatial_reduce(xd, y, scale, ws)
        torch.cuda.synchronize()
        ref = x.sum(dim=(1, 2), keepdim=True) * float(np.float32(scale))
        assert_close(from_dev(y), ref, dtype, f"spatial_reduce scale {scale}", SPATIAL_TOL[dtype])


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("C", [24, 256])
def test_spatial_broadcast(dev, dtype, C):
    N, H, W = 2, 17, 30
    x = rnd(torch.randn(N, 1, 1, C, generator=_gen(1800), dtype=torch.float64), dtype)
    xd = x.to(dtype).to(dev)
    full = torch.full((N, H, W, C + 16), 7.0, device=dev, dtype=dtype)
    y = full[..., :C]                               # strided destination (pixel stride C + 16)
    for scale in (0.25, 1.0 / 3.0):
        ops.spatial_broadcast(xd, y, scale)
        torch.cuda.synchronize()
        ref = (x * float(np.float32(scale))).expand(N, H, W, C)
        assert_close(from_dev(y), ref, dtype, f"spatial_broadcast scale {scale}", SPATIAL_TOL[dtype])
        assert (full[..., C:] == 7.0).all()
