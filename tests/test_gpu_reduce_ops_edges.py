"""Edge-case parity of the channel-reduction kernels in csrc/eltwise.hip --
seg_bias_relu_bwd (bias_relu_bwd_k, col_sum_k, reduce_rows_k) and the
frozen-stat BatchNorm (bn_relu_fwd_k, bn_relu_bwd_k with bn_finish_k, the
dropout variant) -- through the wrappers of ops.py.  Companion of
test_gpu_shape_ops_edges.py; the same ground rules: float64 CPU references
from the rounded inputs, bit equality where the arithmetic is one IEEE
operation sequence, per-element bounds (U = 2^-24, U_DT) elsewhere, NaN
prefill, junk around views.

Lane geometry (red_geom): CK = C / EPC 16-byte chunks per pixel (EPC = 8 for
16-bit, 4 for fp32), LPP = min(CK, 256) lanes per pixel, rows = 256 / LPP
pixels per pass (ragged when CK does not divide 256), iters = ceil(CK / 256)
chunks per lane.  red_blocks() launches min(cap, ceil(P / (2 rows))) blocks,
cap = max(64, min(1024, 2^20 / C)).
"""
import ctypes

import numpy as np
import pytest
import torch

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
GUARD = 777.0


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _epc(dtype):
    return 4 if dtype == torch.float32 else 8


def _rows(C, dtype):
    return 256 // min(C // _epc(dtype), 256)


def _red_blocks(P, C, dtype):
    """red_blocks() of csrc/eltwise.hip."""
    cap = max(64, min(1024, (1 << 20) // C))
    return max(1, min(cap, -(-P // (2 * _rows(C, dtype)))))


def _p_list(C, dtype):
    r = _rows(C, dtype)
    return sorted({1, 3, max(r - 1, 1), 2 * r + 1})


def _p_past_cap(C, dtype):
    """The first P (+ 2) at which red_blocks() hits its cap: every block then covers
    more than two passes of its `rows` pixels."""
    cap = max(64, min(1024, (1 << 20) // C))
    P = cap * 2 * _rows(C, dtype) + 3
    assert _red_blocks(P, C, dtype) == cap == _red_blocks(10 * P, C, dtype)
    return P


def _view(t64, dtype, dev, extra):
    return _slice_view(t64, dtype, dev, extra=extra)


def _around(*ts):
    for t in ts:
        if t is not None and t._base is not None:
            assert_surroundings(t)


# ---------------------------------------------------------------------------
# B. seg_bias_relu_bwd
# ---------------------------------------------------------------------------
# CK = 1, 3, 5, 9, then 63 / 64 / 65 (col_sum_k needs CK >= 64), 257 (a second chunk per
# lane) and 512 / 1024 (the widest the kernels take)
# fp32 (EPC = 4): K = 252 / 260 / 1028 would be CK = 63 / 65 / 257, but the launcher takes
# K % 8 == 0 only (the activation layout pads channels to 8), so an fp32 CK is always even:
# those three are asserted to be refused, and 248 / 264 / 1032 (CK = 62 / 66 / 258) stand
# next to them on either side of the same switches
BIAS_K = {torch.float32: [8, 24, 248, 252, 256, 260, 264, 1028, 1032, 4096],
          torch.bfloat16: [8, 24, 40, 72, 504, 512, 520, 2056, 4096],
          torch.float16: [8, 24, 40, 72, 504, 512, 520, 2056, 4096]}
BIAS_CASES = [(dt, k) for dt in DTYPES for k in BIAS_K[dt]]
BIAS_IDS = [f"{DT_IDS[DTYPES.index(dt)]}-K{k}" for dt, k in BIAS_CASES]


def _check_bias(dev, dtype, P, K, k_valid=None, relu=True, scale=1.0, views=(), alias=False, with_dbias=True,
                ws=None, seed=0):
    k_valid = K if k_valid is None else k_valid
    g = _gen(6000 + seed + K + P % 1000)
    dy = randn_normal((1, 1, P, K), g, dtype)
    y = randn_normal((1, 1, P, K), g, dtype)
    pick = torch.randint(0, 4, y.shape, generator=g)
    y = torch.where(pick == 0, torch.zeros_like(y), torch.where(pick == 1, -torch.zeros_like(y), y))   # +0, -0, +-
    dyd = _view(dy, dtype, dev, 16) if "dy" in views else to_dev(dy, dtype, dev)
    yd = None
    if relu:
        yd = _view(y, dtype, dev, 24) if "y" in views else to_dev(y, dtype, dev)
    if alias:
        dzd = dyd
    else:
        dzd = nan_like_view(dy.shape, dtype, dev, (lambda t: _view(t, dtype, dev, 32)) if "dz" in views else None)
    dbias = torch.full((k_valid + 4,), GUARD, dtype=torch.float32, device=dev) if with_dbias else None
    ops.bias_relu_bwd(dyd, yd, dzd, dbias, k_valid, relu=relu, scale=scale, ws=ws)
    torch.cuda.synchronize()
    # dz: one fp32 product rounded into the dtype (rule 2); masked elements are +0
    s32 = torch.tensor(np.float32(scale))
    want = (dy.to(dtype).float() * s32).to(dtype) if scale != 1.0 else dy.to(dtype)
    mask = (y > 0) if relu else torch.ones_like(y, dtype=torch.bool)
    if relu:
        want = torch.where(mask, (dy.to(dtype).float() * s32).to(dtype), torch.zeros_like(want))
    assert_bits_equal(dzd, want, f"dz P={P} K={K} relu={relu} scale={scale}")
    if not alias:
        assert_bits_equal(dyd, dy.to(dtype), "dy untouched")
    if relu:
        assert_bits_equal(yd, y.to(dtype), "y untouched")
    _around(dyd, yd, dzd)
    if with_dbias:
        # the kernel sums the unrounded fp32 products t = dy * scale * mask: any fp32
        # summation order over P terms is within (P - 1) U sum |t|, the product rounding and
        # the final store add less than 2 U sum |t|: (P + 8) U sum |t| per channel
        t = torch.where(mask, dy * float(np.float32(scale)), torch.zeros_like(dy))[0, 0, :, :k_valid]
        got = dbias.double().cpu()
        assert_within(got[:k_valid], t.sum(0), (P + 8) * U * t.abs().sum(0), f"dbias P={P} K={K}")
        assert bool((got[k_valid:] == GUARD).all()), "dbias written past k_valid"


@pytest.mark.parametrize("dtype,K", BIAS_CASES, ids=BIAS_IDS)
def test_bias_relu_bwd_lane_geometry(dev, dtype, K):
    """Every K around the geometry's switches at P = 1, 3, rows - 1, 2 rows + 1
    and one P past the block cap; k_valid = K - 3 with a guard after it; ReLU
    from y, and the plain BiasAddGrad (dz aliasing dy, no ReLU, scale 1: col_sum_k
    once CK >= 64, bias_relu_bwd_k without a dz store below)."""
    if K % 8:
        dy = torch.ones(1, 1, 3, K, dtype=dtype, device=dev)
        dz, db = torch.full_like(dy, NAN), torch.full((K,), GUARD, device=dev)
        for relu in (True, False):
            with pytest.raises(RuntimeError, match=EINVAL):
                ops.bias_relu_bwd(dy, dy, dz, db, K, relu=relu)
        torch.cuda.synchronize()
        assert bool(torch.isnan(dz).all()) and bool((db == GUARD).all())
        return
    for P in _p_list(K, dtype) + [_p_past_cap(K, dtype)]:
        _check_bias(dev, dtype, P, K, k_valid=K - 3, relu=True)
        _check_bias(dev, dtype, P, K, k_valid=K - 3, relu=False, alias=True)


WIDE = [(dt, k) for dt in DTYPES for k in BIAS_K[dt] if k // _epc(dt) >= 64 and k % 8 == 0]


@pytest.mark.parametrize("dtype,K", WIDE, ids=[f"{DT_IDS[DTYPES.index(dt)]}-K{k}" for dt, k in WIDE])
def test_col_sum_row_lanes_and_tails(dev, dtype, K):
    """col_sum_k: fewer rows than its four row lanes (P = 1, 3), the tail of the
    unrolled-by-16 loop (5, 17), ragged row ranges (P = 203: 4 ranges of 51, 51,
    51, 50 rows at gx = 1), dy dense and as a slice view."""
    for P in (1, 3, 5, 17, 203):
        _check_bias(dev, dtype, P, K, relu=False, alias=True, seed=1)
        _check_bias(dev, dtype, P, K, k_valid=K - 5, relu=False, alias=True, views=("dy",), seed=2)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_bias_relu_bwd_modes(dev, dtype):
    K = 24 if dtype == torch.float32 else 40
    P = 2 * _rows(K, dtype) + 1
    for v in (("dy",), ("y",), ("dz",), ("dy", "y", "dz")):
        _check_bias(dev, dtype, P, K, k_valid=K - 3, views=v)
    _check_bias(dev, dtype, P, K, alias=True)                                  # dz aliases dy, with ReLU
    _check_bias(dev, dtype, P, K, alias=True, views=("dy", "y"))
    _check_bias(dev, dtype, P, K, scale=1.25)                                  # ReLU + 1/keep_prob
    _check_bias(dev, dtype, P, K, scale=1.25, relu=False)
    _check_bias(dev, dtype, P, K, scale=1.25, relu=False, alias=True)
    _check_bias(dev, dtype, P, K, relu=False)                                  # plain copy + sums
    _check_bias(dev, dtype, P, K, with_dbias=False)                            # the executor's ReluGrad
    _check_bias(dev, dtype, P, K, with_dbias=False, views=("dy", "y", "dz"))
    _check_bias(dev, dtype, P, 512, scale=1.25, relu=False, alias=True)        # wide K, scale != 1: not col_sum_k


class _FixedWs:
    """A workspace that reports `nbytes` whatever is asked for (its buffer is the full size)."""

    def __init__(self, dev, nbytes, real):
        self.buf = torch.empty(real, dtype=torch.uint8, device=dev)
        self.nbytes = nbytes

    def ptr_size(self, need):
        return ctypes.c_void_p(self.buf.data_ptr()), ctypes.c_size_t(self.nbytes)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_bias_relu_bwd_rejections(dev, dtype):
    """K = 4104 and a workspace one byte short are refused on the host before any
    launch (status 1 / 4); the workspace is required without dbias as well."""
    from semanticsegmentation_tensorflow_amd import _lib
    dy = torch.ones(1, 1, 2, 4104, dtype=dtype, device=dev)
    dz = torch.full_like(dy, NAN)
    with pytest.raises(RuntimeError, match=EINVAL):
        ops.bias_relu_bwd(dy, dy, dz, None, 4104)
    K, P = 40 if dtype != torch.float32 else 24, 700
    full = int(_lib.lib().seg_bias_grad_workspace(P, K))
    need = _red_blocks(P, K, dtype) * K * 4
    assert need <= full
    dy = torch.ones(1, 1, P, K, dtype=dtype, device=dev)
    dz2 = torch.full_like(dy, NAN)
    db = torch.full((K,), GUARD, device=dev)
    for dbias in (db, None):
        with pytest.raises(RuntimeError, match=r"\(status 4\)"):
            ops.bias_relu_bwd(dy, dy, dz2, dbias, K, ws=_FixedWs(dev, need - 1, full))
    torch.cuda.synchronize()
    assert bool(torch.isnan(dz).all()) and bool(torch.isnan(dz2).all()) and bool((db == GUARD).all())
    _check_bias(dev, dtype, P, K, ws=_FixedWs(dev, need, full))                # exactly enough is enough
    _check_bias(dev, dtype, P, K, with_dbias=False, ws=_FixedWs(dev, need, full))


# ---------------------------------------------------------------------------
# C. frozen-stat BatchNorm (+ ReLU)
# ---------------------------------------------------------------------------
# fp32 C = 1028 (CK = 257) is refused like the bias K above: C % 8 == 0 only; 1032 is CK = 258
BN_C = {torch.float32: [8, 24, 1028, 1032], torch.bfloat16: [8, 24, 40, 72, 2056, 4096],
        torch.float16: [8, 24, 40, 72, 2056, 4096]}
BN_CASES = [(dt, c) for dt in DTYPES for c in BN_C[dt]]
BN_IDS = [f"{DT_IDS[DTYPES.index(dt)]}-C{c}" for dt, c in BN_CASES]


def _bn_params(C, g):
    gamma = (1 + 0.3 * torch.randn(C, generator=g, dtype=torch.float64)).float()
    beta = (0.3 * torch.randn(C, generator=g, dtype=torch.float64)).float()
    return gamma, beta


def _inv(eps):
    """1 / sqrt(1 + eps) in float64 from the eps the device receives (a float)."""
    return 1.0 / float(np.sqrt(1.0 + float(np.float32(eps))))


def _check_bn_fwd(dev, dtype, P, C, cv, relu, eps, views=(), seed=0):
    g = _gen(7000 + seed + C + P % 1000)
    x = randn_normal((1, 1, P, C), g, dtype)                    # padding channels hold finite junk
    gamma, beta = _bn_params(C, g)
    xd = _view(x, dtype, dev, 16) if "x" in views else to_dev(x, dtype, dev)
    y = nan_like_view(x.shape, dtype, dev, (lambda t: _view(t, dtype, dev, 24)) if "y" in views else None)
    ops.bn_relu_fwd(xd, y, gamma.to(dev), beta.to(dev), cv, relu=relu, eps=eps)
    torch.cuda.synchronize()
    lin = x * (gamma.double() * _inv(eps))
    ref = lin + beta.double()
    if relu:
        ref = torch.relu(ref)
    # inv = 1 / sqrt(1 + eps) (three roundings, the square root halving the first), gamma * inv
    # and one fma: 4 U (|x gamma inv| + |beta|); the ReLU clamp cannot increase the error
    bound = storage_bound(ref, dtype, 4 * U * (lin.abs() + beta.double().abs()))
    ref[..., cv:] = 0                                           # padding channels: zeros, with and without ReLU
    bound[..., cv:] = 0
    assert_within(y.double().cpu(), ref, bound, f"bn y P={P} C={C} cv={cv} relu={relu}")
    assert_bits_equal(xd, x.to(dtype), "x untouched")
    _around(xd, y)


@pytest.mark.parametrize("dtype,C", BN_CASES, ids=BN_IDS)
def test_bn_fwd_lane_geometry(dev, dtype, C):
    if C % 8:
        x = torch.ones(1, 1, 3, C, dtype=dtype, device=dev)
        y = torch.full_like(x, NAN)
        with pytest.raises(RuntimeError, match=EINVAL):
            ops.bn_relu_fwd(x, y, torch.ones(C, device=dev), torch.zeros(C, device=dev), C)
        torch.cuda.synchronize()
        assert bool(torch.isnan(y).all())
        return
    for P in _p_list(C, dtype):
        for cv in (C, C - 3):
            _check_bn_fwd(dev, dtype, P, C, cv, relu=True, eps=1e-3)
            _check_bn_fwd(dev, dtype, P, C, cv, relu=False, eps=0.05, seed=1)


def test_bn_fwd_second_pass(dev):
    """bf16, C = 2048 (256 chunks: rows = 1, one pixel per workgroup pass), P =
    16384 + 37 > the 16384-block cap: bn_relu_fwd_k's last 37 pixels are a second pass."""
    dt, C, cv, P, p0, eps = torch.bfloat16, 2048, 2045, 16384 + 37, 41, 1e-3
    g = _gen(71)
    x0 = randn_normal((p0, C), g, dt)
    gamma, beta = _bn_params(C, g)
    x = tile_rows(x0.to(dt).to(dev), P).view(1, 1, P, C)
    y = torch.full_like(x, NAN)
    ops.bn_relu_fwd(x, y, gamma.to(dev), beta.to(dev), cv, relu=True, eps=eps)
    torch.cuda.synchronize()
    lin = x0 * (gamma.double() * _inv(eps))
    ref = torch.relu(lin + beta.double())
    bound = storage_bound(ref, dt, 4 * U * (lin.abs() + beta.double().abs()))     # as _check_bn_fwd
    ref[:, cv:] = 0
    bound[:, cv:] = 0
    assert_within(y.view(P, C).double(), tile_rows(ref.to(dev), P), tile_rows(bound.to(dev), P), "bn y, tiled")


def _check_bn_bwd(dev, dtype, P, C, cv, mode, eps=1e-3, views=(), accumulate=False, dropout=None, seed=0):
    """mode "y": ReLU mask from the stored y; "x": re-derived from x (y = None, beta
    given); "none": no ReLU, y and beta both None.  dropout = (keep_prob, drop_c_valid)."""
    g = _gen(8000 + seed + C + P % 1000)
    x = randn_normal((1, 1, P, C), g, dtype)
    dy = randn_normal((1, 1, P, C), g, dtype)
    gamma, beta = _bn_params(C, g)
    inv = _inv(eps)
    if mode == "x":
        # rule 4: the reference alone decides the sign -- no element within 1e-3 relative
        # of a cancellation -- then the exact cases by hand
        beta[0], beta[1] = 0.0, 0.25
        sc = gamma.double() * inv
        for _ in range(50):
            bad = (x * sc + beta.double()).abs() < 1e-3 * ((x * sc).abs() + beta.double().abs())
            if not bool(bad.any()):
                break
            x = torch.where(bad, randn_normal(x.shape, g, dtype), x)
        assert not bool(bad.any()), "resampling cut short"
        x[0, 0, 0, 0] = 0.0                         # x = 0, beta = 0: pre-activation 0, not kept
        x[0, 0, 0, 1] = 0.0                         # x = 0, beta > 0: kept
    pre = x * (gamma.double() * inv) + beta.double()
    yq = rnd(torch.relu(pre), dtype)                # the stored y: an input of the kernel under test
    if mode == "y":
        mask = yq > 0
    elif mode == "x":
        mask = pre > 0
        assert not bool(mask[0, 0, 0, 0]) and bool(mask[0, 0, 0, 1])
    else:
        mask = torch.ones_like(pre, dtype=torch.bool)
    old = randn_normal(x.shape, g, dtype) if accumulate else torch.full(x.shape, NAN, dtype=torch.float64)
    xd = _view(x, dtype, dev, 16) if "x" in views else to_dev(x, dtype, dev)
    yd = None
    if mode == "y":
        yd = _view(yq, dtype, dev, 24) if "y" in views else to_dev(yq, dtype, dev)
    dyd = _view(dy, dtype, dev, 32) if "dy" in views else to_dev(dy, dtype, dev)
    dxd = _view(old, dtype, dev, 40) if "dx" in views else old.to(dtype).to(dev)
    dg = torch.full((cv + 3,), GUARD, dtype=torch.float32, device=dev)
    db = torch.full((cv + 3,), GUARD, dtype=torch.float32, device=dev)
    kp, dcv, dseed = (dropout[0], dropout[1], 424242) if dropout else (1.0, 0, 0)
    ops.bn_relu_bwd(xd, yd, dyd, dxd, gamma.to(dev), dg, db, cv, relu=mode != "none", eps=eps,
                    accumulate=accumulate, beta=beta.to(dev) if mode == "x" else None,
                    dropout=(kp, dseed, dcv) if dropout else None)
    torch.cuda.synchronize()
    dz = torch.where(mask, dy, torch.zeros_like(dy))
    dz[..., cv:] = 0
    term = dz * (gamma.double() * inv)
    if dropout:
        cnt = (np.arange(P, dtype=np.uint64)[:, None] * np.uint64(dcv) + np.arange(dcv, dtype=np.uint64)[None, :])
        u = _np_uniform_vec(dseed, cnt.reshape(-1)).reshape(P, dcv)
        keep = torch.zeros(1, 1, P, C, dtype=torch.float64)                 # c >= drop_c_valid: zero
        keep[0, 0, :, :dcv] = torch.from_numpy(np.floor(np.float32(kp) + u).astype(np.float64))
        term = term * float(np.float32(1.0) / np.float32(kp)) * keep
    ref = term + old if accumulate else term
    # sc = gamma * inv carries 4 U (see the forward), dz * sc one rounding, the accumulate add
    # one, the dropout's 1 / kp and its product two: within 8 U (|term| + |old|), then storage
    bound = storage_bound(ref, dtype, 8 * U * (term.abs() + (old.abs() if accumulate else 0)))
    what = f"P={P} C={C} cv={cv} mode={mode} acc={accumulate} drop={dropout}"
    assert_within(dxd.double().cpu(), ref, bound, "bn dx " + what)
    if accumulate:          # padding channels keep the old value, bit for bit
        assert_bits_equal(dxd[..., cv:], old[..., cv:].to(dtype), "bn dx padding, accumulate")
    else:
        assert bool((dxd[..., cv:] == 0).all()), "bn dx padding"
    if dropout:
        dropped = (keep == 0).expand_as(ref)
        assert bool((dxd.cpu()[dropped] == 0).all()), "dropped elements"
    # channel sums over P terms, any order: (P + 8) U sum |t| (rule 3); dgamma's terms are
    # dz x inv (the product roundings and the inv factor inside the + 8); no dropout in either
    tg = (dz * x * inv)[0, 0, :, :cv]
    tb = dz[0, 0, :, :cv]
    got_g, got_b = dg.double().cpu(), db.double().cpu()
    assert_within(got_g[:cv], tg.sum(0), (P + 8) * U * tg.abs().sum(0), "dgamma " + what)
    assert_within(got_b[:cv], tb.sum(0), (P + 8) * U * tb.abs().sum(0), "dbeta " + what)
    assert bool((got_g[cv:] == GUARD).all()) and bool((got_b[cv:] == GUARD).all()), "written past c_valid"
    assert_bits_equal(xd, x.to(dtype), "x untouched")
    assert_bits_equal(dyd, dy.to(dtype), "dy untouched")
    _around(xd, yd, dyd, dxd)


@pytest.mark.parametrize("dtype,C", BN_CASES, ids=BN_IDS)
def test_bn_bwd_lane_geometry(dev, dtype, C):
    if C % 8:
        x = torch.ones(1, 1, 3, C, dtype=dtype, device=dev)
        dx = torch.full_like(x, NAN)
        dg, db = torch.full((C,), GUARD, device=dev), torch.full((C,), GUARD, device=dev)
        with pytest.raises(RuntimeError, match=EINVAL):
            ops.bn_relu_bwd(x, x, x, dx, torch.ones(C, device=dev), dg, db, C)
        torch.cuda.synchronize()
        assert bool(torch.isnan(dx).all()) and bool((dg == GUARD).all()) and bool((db == GUARD).all())
        return
    for P in _p_list(C, dtype):
        for cv in (C, C - 3):
            _check_bn_bwd(dev, dtype, P, C, cv, "y")
            _check_bn_bwd(dev, dtype, P, C, cv, "x", eps=0.05, seed=1)
            _check_bn_bwd(dev, dtype, P, C, cv, "none", seed=2)
            _check_bn_bwd(dev, dtype, P, C, cv, "x", accumulate=True, seed=3)
    _check_bn_bwd(dev, dtype, _p_past_cap(C, dtype), C, C - 3, "x", seed=4)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_bn_views(dev, dtype):
    C = 24 if dtype == torch.float32 else 40
    P = 2 * _rows(C, dtype) + 1
    for v in (("x",), ("y",), ("x", "y")):
        _check_bn_fwd(dev, dtype, P, C, C - 3, True, 1e-3, views=v, seed=5)
    for v in (("x",), ("y",), ("dy",), ("dx",), ("x", "y", "dy", "dx")):
        _check_bn_bwd(dev, dtype, P, C, C - 3, "y", views=v, seed=6)
    _check_bn_bwd(dev, dtype, P, C, C - 3, "x", views=("dx",), accumulate=True, seed=7)
    _check_bn_bwd(dev, dtype, P, C, C - 3, "none", views=("x", "dx"), accumulate=True, seed=8)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_bn_bwd_relu_without_y_or_beta_is_rejected(dev, dtype):
    C = 8
    x = torch.ones(1, 1, 4, C, dtype=dtype, device=dev)
    dx = torch.full_like(x, NAN)
    gamma = torch.ones(C, device=dev)
    dg, db = torch.full((C,), GUARD, device=dev), torch.full((C,), GUARD, device=dev)
    with pytest.raises(RuntimeError, match=EINVAL):
        ops.bn_relu_bwd(x, None, x, dx, gamma, dg, db, C, relu=True)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx).all()) and bool((dg == GUARD).all()) and bool((db == GUARD).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kp", [0.5, 0.8])
@pytest.mark.parametrize("dcv", ["C", "C-3", "1"])
def test_bn_relu_dropout_bwd(dev, dtype, kp, dcv):
    """dx also carries the gradient of the dropout fused into the producing conv
    (counter pixel * drop_c_valid + c): zero where dropped or c >= drop_c_valid;
    dgamma / dbeta unaffected."""
    C = 24 if dtype == torch.float32 else 40
    d = {"C": C, "C-3": C - 3, "1": 1}[dcv]
    P = 2 * _rows(C, dtype) + 1
    _check_bn_bwd(dev, dtype, P, C, C - 3 if d < C else C, "y", dropout=(kp, d), seed=9)
    _check_bn_bwd(dev, dtype, P, C, C, "x", dropout=(kp, d), views=("x", "dx"), seed=10)
    _check_bn_bwd(dev, dtype, 3, C, C, "none", dropout=(kp, d), seed=11)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_bn_as_plain_relu(dev, dtype):
    """gamma 1, beta 0, eps 0 is the executor's plain ReLU: y == relu(x) exactly,
    as values (the sign of a zero result is not pinned)."""
    C, fi = 16, torch.finfo(dtype)
    x = randn_normal((1, 3, 5, C), _gen(12), dtype)
    sub = fi.smallest_normal / 4
    special = [0.0, -0.0, float("inf"), -float("inf"), sub, -sub, fi.tiny, -fi.tiny, fi.max, -fi.max,
               2.0 ** -24, -2.0 ** -24]
    x.view(-1)[:len(special)] = torch.tensor(special, dtype=torch.float64)
    x = rnd(x, dtype)
    assert float(x.view(-1)[4]) == sub                      # the subnormal survives the rounding on the CPU
    xd = to_dev(x, dtype, dev)
    y = torch.full_like(xd, NAN)
    ops.bn_relu_fwd(xd, y, torch.ones(C, device=dev), torch.zeros(C, device=dev), C, relu=True, eps=0.0)
    torch.cuda.synchronize()
    got, want = y.double().cpu(), torch.relu(x)
    assert torch.equal(got, want), f"differs at {(got != want).nonzero()[:4].tolist()}"
