"""seg_bn_act_fwd / _bwd, seg_se_squeeze, seg_se_excite_fwd / _bwd
(csrc/mbconv.hip) against tests/mbconv_ref.py in f32, bf16 and f16, dense and
through channel slices of a wider tensor of JUNK.  Destinations start as NaN
and the padding channels of every input hold PAD (not zero), so a skipped
element or a padding channel left to the arithmetic shows.

Inputs are rounded through bf16 with magnitudes floored at 2^-6 (exact in all
three dtypes), gamma / beta are fp32 values and eps / scale the fp32 numbers
the library receives, so one float64 reference serves the three dtypes.  The
bounds are derived from the operations the kernels use, with u = 2^-24 and
zmag = |x scale| + |beta| >= |z| (the magnitudes that enter z):

* z: scale = gamma * inv with inv = 1 / sqrtf(1 + eps) -- four roundings, 4u --
  then one fma: |dz| <= 4u |x scale| + u |z| <= 5u zmag.
* sigmoid: expf (1 ulp = 2u, which moves 1 / (1 + e) by at most 2u), the sum
  and the quotient: 4u relative, plus sigmoid' <= 1/4 on dz.  swish adds one
  product (u) and |swish'| <= 1.1 on dz.  Both within
      K_FWD u (|y| + zmag),  K_FWD = 6  (5u |y| + 5.5u zmag),
  plus the storage rounding U_T |ref| and half the format's subnormal spacing.
* the gradient factor g = s (1 + z (1 - s)) (or s (1 - s)): 1 - s, z t, 1 + z t
  and the product carry at most 12u (1 + |z|) absolute, |g'| <= 1/2 on dz adds
  2.5u zmag; dy g and the product with scale (4u + u) give
      |d dx| <= K_BWD u |dy scale| (1 + zmag),  K_BWD = 22;
  accumulation adds u (|dx| + |old|).
* sums of n terms: n u sum|terms| in any order, plus the terms' own error
  (16u |dy| (1 + zmag) each, times |x| for dgamma) and 3u |ref| for the final
  product with inv; the squeeze's terms are exact and its scale costs 2u |ref|;
  ds sums fmas of exact inputs.  Results stored in T add the storage rounding.

The fraction of each bound used is printed (DESIGN.md section 12 records it).
Reductions run twice are bit-identical; refused calls leave everything untouched."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from semanticsegmentation_tensorflow_amd import _lib, ops
from tests import mbconv_ref as R
from tests.gpu_utils import U, U_DT, assert_bits_equal, assert_surroundings, assert_within, randn_normal, rnd

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SUB = {torch.float32: 2.0 ** -150, torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}
K_FWD, K_BWD, K_TERM = 6.0, 22.0, 16.0
JUNK, PAD = 50.0, 3.0
EPS = float(np.float32(1e-3))
EINVAL, EALIGN, EWORKSPACE = 1, 3, 4

# (P, C, c_valid, affine, sliced)
BN_CASES = [
    (1, 8, 4, False, False),        # the squeeze-excite vector of batch 1 (se_reduce of the first block)
    (1, 8, 4, True, False),
    (3, 8, 5, True, True),          # padding channels must be zeros (sigmoid(0) = 0.5); ldx > C
    (37, 16, 16, False, True),
    (1100, 24, 21, True, False),    # four partial rows (8192 elements each), 1100 pixels over them unevenly
    (6, 1152, 1152, True, False),   # 288 fp32 chunks: more than one chunk group
]
# (N, H, W, C, c_valid, sliced)
SE_CASES = [
    (1, 1, 1, 8, 4, False),         # H W = 1
    (2, 5, 7, 16, 16, True),        # a different gate per image; ldx > C
    (1, 19, 23, 24, 21, False),     # 437 pixels: four slices, the last one short
    (2, 3, 2, 1152, 1152, False),   # the width seg_spatial_reduce refuses in fp32
]
_id = lambda c: "x".join(str(int(v)) for v in c)     # noqa: E731


def storage(ref, dtype, fp32_term):
    return U_DT[dtype] * ref.abs() + SUB[dtype] + fp32_term


def put(t64, C, dtype, dev, sliced, pad=PAD):
    """[.., cv] float64 -> device [.., C] (padding channels = pad), dense or as
    channels 8 .. 8 + C of a wider tensor of JUNK."""
    full = torch.full(tuple(t64.shape[:-1]) + (C,), pad, dtype=torch.float64)
    full[..., :t64.shape[-1]] = t64
    if not sliced:
        return full.to(dtype).to(dev).contiguous()
    base = torch.full(tuple(full.shape[:-1]) + (C + 16,), JUNK, dtype=dtype, device=dev)
    v = base[..., 8:8 + C]
    v.copy_(full.to(dtype))
    return v


def nan_out(shape, dtype, dev, sliced):
    return put(torch.full(shape, float("nan"), dtype=torch.float64), shape[-1], dtype, dev, sliced)


@functools.lru_cache(maxsize=None)
def bn_reference(case, act):
    P, C, cv, affine, _ = case
    g = torch.Generator().manual_seed(300 + BN_CASES.index(case))
    x = randn_normal((1, 1, P, cv), g, torch.bfloat16, scale=2.0)
    dy = randn_normal((1, 1, P, cv), g, torch.bfloat16)
    old = randn_normal((1, 1, P, cv), g, torch.bfloat16)
    gamma = beta = None
    if affine:
        gamma = (1.0 + 0.3 * torch.randn(cv, generator=g, dtype=torch.float64)).float().double()
        beta = (0.5 * torch.randn(cv, generator=g, dtype=torch.float64)).float().double()
    y = R.bn_act_fwd(x, gamma, beta, EPS, act)
    dx, dgamma, dbeta = R.bn_act_bwd(x, dy, gamma, beta, EPS, act)
    z, scale = R.affine(x, gamma, beta, EPS)
    zmag = (x * scale).abs() + (beta.abs() if affine else 0.0)
    b_y = K_FWD * U * (y.abs() + zmag)
    b_dx = K_BWD * U * (dy * scale).abs() * (1.0 + zmag)
    b_sum = None
    if affine:
        inv = 1.0 / np.sqrt(1.0 + EPS)
        dz = dy * R.act_grad(z, act)
        term = K_TERM * U * dy.abs() * (1.0 + zmag)
        red = (0, 1, 2)
        b_dbeta = P * U * dz.abs().sum(red) + term.sum(red)
        b_dgamma = inv * (P * U * (dz * x).abs().sum(red) + (term * x.abs()).sum(red)) + 3 * U * dgamma.abs()
        b_sum = (b_dgamma, b_dbeta)
    return x, dy, old, gamma, beta, y, dx, dgamma, dbeta, b_y, b_dx, b_sum


def run_bn(dev, case, dt, act):
    P, C, cv, affine, sliced = case
    dtype = DTYPES[dt]
    x, dy, old, gamma, beta, y_ref, dx_ref, dg_ref, db_ref, b_y, b_dx, b_sum = bn_reference(case, act)
    what = f"bn_act {case} {dt} {act}"
    xd, dyd = put(x, C, dtype, dev, sliced), put(dy, C, dtype, dev, sliced)
    yd, dxd = nan_out((1, 1, P, C), dtype, dev, sliced), nan_out((1, 1, P, C), dtype, dev, sliced)
    dxa = put(old, C, dtype, dev, sliced, pad=0.0)
    gd = bd = dgd = dbd = dgd2 = dbd2 = None
    ws = None
    if affine:
        gd, bd = gamma.float().to(dev), beta.float().to(dev)
        dgd, dbd, dgd2, dbd2 = (torch.full((cv,), float("nan"), dtype=torch.float32, device=dev) for _ in range(4))
        need = ops.bn_act_bwd_workspace(P, C)
        assert need == min(512, -(-P * C // 8192)) * 2 * C * 4
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    ops.bn_act_fwd(xd, yd, gd, bd, cv, act, EPS)
    ops.bn_act_bwd(xd, dyd, dxd, gd, bd, dgd, dbd, cv, act, EPS, ws)
    ops.bn_act_bwd(xd, dyd, dxa, gd, bd, dgd2, dbd2, cv, act, EPS, ws, accumulate=True)
    torch.cuda.synchronize()
    if sliced:
        for v in (xd, dyd, yd, dxd, dxa):
            assert_surroundings(v, JUNK, what)
    got_y, got_dx, got_dxa = yd.double().cpu(), dxd.double().cpu(), dxa.double().cpu()
    for t in (got_y, got_dx, got_dxa):
        assert bool((t[..., cv:] == 0).all()), what + ": padding channels must be exact zeros"
    fy = assert_within(got_y[..., :cv], y_ref, storage(y_ref, dtype, b_y), what + " y")
    fdx = assert_within(got_dx[..., :cv], dx_ref, storage(dx_ref, dtype, b_dx), what + " dx")
    acc_ref = dx_ref + old
    fda = assert_within(got_dxa[..., :cv], acc_ref,
                        storage(acc_ref, dtype, b_dx + U * (dx_ref.abs() + old.abs())), what + " dx accumulated")
    msg = f"{what}: fraction of the bound used: y {fy:.3f} dx {fdx:.3f} dx+= {fda:.3f}"
    if affine:
        fg = assert_within(dgd.double().cpu(), dg_ref, b_sum[0], what + " dgamma")
        fb = assert_within(dbd.double().cpu(), db_ref, b_sum[1], what + " dbeta")
        assert_bits_equal(dgd, dgd2, what + " dgamma twice")
        assert_bits_equal(dbd, dbd2, what + " dbeta twice")
        msg += f" dgamma {fg:.3f} dbeta {fb:.3f}"
    print(msg)


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("case", BN_CASES, ids=_id)
def test_bn_act_fwd_bwd(dev, case, dt, act):
    run_bn(dev, case, dt, act)


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("dt", list(DTYPES))
def test_large_arguments_are_finite_and_correct(dev, dt, act, affine):
    """z in {-100, -20, 0, 20, 100}: exp overflows to inf on the way, the
    results are 0 / 1 / z, never NaN -- forward and backward."""
    dtype = DTYPES[dt]
    zs = torch.tensor([-100.0, -20.0, 0.0, 20.0, 100.0, -100.0, 100.0, 0.0], dtype=torch.float64)
    x = zs.reshape(1, 1, 1, 8).repeat(1, 1, 3, 1)
    dy = torch.full_like(x, 1.5)
    gamma = beta = gd = bd = dgd = dbd = ws = None
    if affine:
        gamma, beta = torch.ones(8, dtype=torch.float64), torch.zeros(8, dtype=torch.float64)
        gd, bd = gamma.float().to(dev), beta.float().to(dev)
        dgd, dbd = (torch.full((8,), float("nan"), dtype=torch.float32, device=dev) for _ in range(2))
        ws = torch.zeros(ops.bn_act_bwd_workspace(3, 8), dtype=torch.uint8, device=dev)
    xd, dyd = x.to(dtype).to(dev), dy.to(dtype).to(dev)
    yd, dxd = torch.full_like(xd, float("nan")), torch.full_like(xd, float("nan"))
    ops.bn_act_fwd(xd, yd, gd, bd, 8, act, 0.0)
    ops.bn_act_bwd(xd, dyd, dxd, gd, bd, dgd, dbd, 8, act, 0.0, ws)
    torch.cuda.synchronize()
    y, dx = yd.double().cpu(), dxd.double().cpu()
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all())
    y_ref = R.bn_act_fwd(x, gamma, beta, 0.0, act)
    dx_ref, dg_ref, db_ref = R.bn_act_bwd(x, dy, gamma, beta, 0.0, act)
    zmag = x.abs()
    assert_within(y, y_ref, storage(y_ref, dtype, K_FWD * U * (y_ref.abs() + zmag)), f"{dt} {act} y")
    assert_within(dx, dx_ref, storage(dx_ref, dtype, K_BWD * U * dy.abs() * (1.0 + zmag)), f"{dt} {act} dx")
    # the saturated ends exactly: sigmoid 0 / 1, swish 0 / z, slopes 0 / (0 or 1)
    assert y[0, 0, 0, 0].item() == 0.0 and y[0, 0, 0, 4].item() == (100.0 if act == "swish" else 1.0)
    assert dx[0, 0, 0, 0].item() == 0.0 and dx[0, 0, 0, 4].item() == (1.5 if act == "swish" else 0.0)
    if affine:
        assert bool(torch.isfinite(dgd).all()) and bool(torch.isfinite(dbd).all())
        term = K_TERM * U * dy.abs() * (1.0 + zmag)
        dz = dy * R.act_grad(x, act)
        assert_within(dbd.double().cpu(), db_ref, 3 * U * dz.abs().sum((0, 1, 2)) + term.sum((0, 1, 2)), "dbeta")
        assert_within(dgd.double().cpu(), dg_ref, 3 * U * (dz * x).abs().sum((0, 1, 2))
                      + (term * x.abs()).sum((0, 1, 2)) + 3 * U * dg_ref.abs(), "dgamma")


@functools.lru_cache(maxsize=None)
def se_reference(case):
    N, H, W, C, cv, _ = case
    g = torch.Generator().manual_seed(400 + SE_CASES.index(case))
    x = randn_normal((N, H, W, cv), g, torch.bfloat16)
    dy = randn_normal((N, H, W, cv), g, torch.bfloat16)
    old = randn_normal((N, H, W, cv), g, torch.bfloat16)
    s = rnd(torch.rand(N, cv, generator=g, dtype=torch.float64).clamp_min(2.0 ** -6), torch.bfloat16)
    scale = float(np.float32(1.0 / (H * W)))
    n = H * W
    sq = R.se_squeeze(x, scale)
    y = R.se_excite_fwd(x, s)
    dx, ds = R.se_excite_bwd(x, s, dy)
    b_sq = n * U * x.abs().sum((1, 2)) * scale + 2 * U * sq.abs()
    b_ds = n * U * (dy * x).abs().sum((1, 2))
    return x, dy, old, s, scale, sq, y, dx, ds, b_sq, b_ds


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("case", SE_CASES, ids=_id)
def test_squeeze_and_excite(dev, case, dt):
    N, H, W, C, cv, sliced = case
    dtype = DTYPES[dt]
    x, dy, old, s, scale, sq_ref, y_ref, dx_ref, ds_ref, b_sq, b_ds = se_reference(case)
    what = f"se {case} {dt}"
    xd, dyd = put(x, C, dtype, dev, sliced), put(dy, C, dtype, dev, sliced)
    sd = put(s.reshape(N, 1, 1, cv), C, dtype, dev, False)
    yd, dxd = nan_out((N, H, W, C), dtype, dev, sliced), nan_out((N, H, W, C), dtype, dev, sliced)
    dxa = put(old, C, dtype, dev, sliced, pad=0.0)
    sq, sq2, dsd, dsd2 = (torch.full((N, 1, 1, C), float("nan"), dtype=dtype, device=dev) for _ in range(4))
    need = ops.se_squeeze_workspace(N, H, W, C)
    slices = min(128, -(-(H * W) // 128))
    assert need == N * slices * C * 4
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    if C == 1152 and dt == "f32":
        # the present global-average-pool kernel refuses this width, writing nothing
        acc = torch.zeros(N * C, dtype=torch.float32, device=dev)
        st = _lib.lib().seg_spatial_reduce(ops.ptr(xd), C, ops.ptr(sq), N, H, W, C, scale, ops.ptr(acc), ops.F32,
                                           ops.stream_ptr())
        torch.cuda.synchronize()
        assert st == EINVAL and bool(torch.isnan(sq).all())
        assert not ops.spatial_reduce_fits(C, ops.F32) and ops.spatial_reduce_fits(C, ops.BF16)
    ops.se_squeeze(xd, sq, cv, scale, ws)
    ops.se_squeeze(xd, sq2, cv, scale, ws)
    ops.se_excite_fwd(xd, sd, yd, cv)
    ops.se_excite_bwd(xd, sd, dyd, dxd, dsd, cv, ws)
    ops.se_excite_bwd(xd, sd, dyd, dxa, dsd2, cv, ws, accumulate=True)
    torch.cuda.synchronize()
    if sliced:
        for v in (xd, dyd, yd, dxd, dxa):
            assert_surroundings(v, JUNK, what)
    got = {k: v.double().cpu() for k, v in dict(sq=sq, y=yd, dx=dxd, dxa=dxa, ds=dsd).items()}
    for k, t in got.items():
        assert bool((t[..., cv:] == 0).all()), f"{what} {k}: padding channels must be exact zeros"
    f1 = assert_within(got["sq"][:, 0, 0, :cv], sq_ref, storage(sq_ref, dtype, b_sq), what + " squeeze")
    f2 = assert_within(got["y"][..., :cv], y_ref, storage(y_ref, dtype, U * y_ref.abs()), what + " y")
    f3 = assert_within(got["dx"][..., :cv], dx_ref, storage(dx_ref, dtype, U * dx_ref.abs()), what + " dx")
    acc_ref = dx_ref + old
    f4 = assert_within(got["dxa"][..., :cv], acc_ref,
                       storage(acc_ref, dtype, 2 * U * dx_ref.abs() + U * old.abs()), what + " dx accumulated")
    f5 = assert_within(got["ds"][:, 0, 0, :cv], ds_ref, storage(ds_ref, dtype, b_ds), what + " ds")
    assert_bits_equal(sq, sq2, what + " squeeze twice")
    assert_bits_equal(dsd, dsd2, what + " ds twice")
    print(f"{what}: fraction of the bound used: squeeze {f1:.3f} y {f2:.3f} dx {f3:.3f} dx+= {f4:.3f} ds {f5:.3f}")


def test_refused_calls_write_nothing(dev):
    lib = _lib.lib()
    dtype = torch.bfloat16
    N, H, W, C = 2, 3, 4, 16
    P = N * H * W
    nanf = lambda *shape, dt=dtype: torch.full(shape, float("nan"), dtype=dt, device=dev)     # noqa: E731
    x = torch.ones(N, H, W, C, dtype=dtype, device=dev)
    dy = torch.ones_like(x)
    s_ = torch.full((N, 1, 1, C), 0.5, dtype=dtype, device=dev)
    gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    y, dx, sq, ds = nanf(N, H, W, C), nanf(N, H, W, C), nanf(N, 1, 1, C), nanf(N, 1, 1, C)
    dg, db = nanf(C, dt=torch.float32), nanf(C, dt=torch.float32)
    need_bn, need_se = ops.bn_act_bwd_workspace(P, C), ops.se_squeeze_workspace(N, H, W, C)
    ws = torch.full((max(need_bn, need_se),), 0xFF, dtype=torch.uint8, device=dev)
    st = ops.stream_ptr()
    p = ops.ptr
    Z = ctypes.c_size_t

    def fwd(x_=x, ldx=C, y_=y, ldy=C, g=gamma, b=beta, eps=1e-3, P_=P, C_=C, cv=C, act=1, dt=ops.BF16):
        return lib.seg_bn_act_fwd(p(x_), ldx, p(y_), ldy, p(g), p(b), eps, P_, C_, cv, act, dt, st)

    def bwd(x_=x, ldx=C, lddy=C, lddx=C, g=gamma, b=beta, dg_=dg, db_=db, P_=P, C_=C, cv=C, act=1, flags=0,
            dt=ops.BF16, ws_=ws, nbytes=need_bn):
        return lib.seg_bn_act_bwd(p(x_), ldx, p(dy), lddy, p(dx), lddx, p(g), p(b), 1e-3, p(dg_), p(db_), P_, C_, cv,
                                  act, flags, dt, p(ws_), Z(nbytes), st)

    def squeeze(x_=x, ldx=C, N_=N, H_=H, C_=C, cv=C, dt=ops.BF16, nbytes=need_se, ws_=ws):
        return lib.seg_se_squeeze(p(x_), ldx, p(sq), N_, H_, W, C_, cv, 1.0, p(ws_), Z(nbytes), dt, st)

    def excite(ldx=C, ldy=C, s=s_, N_=N, C_=C, cv=C, dt=ops.BF16):
        return lib.seg_se_excite_fwd(p(x), ldx, p(s), p(y), ldy, N_, H, W, C_, cv, dt, st)

    def excite_bwd(ldx=C, lddy=C, lddx=C, s=s_, N_=N, C_=C, cv=C, flags=0, dt=ops.BF16, nbytes=need_se, ws_=ws):
        return lib.seg_se_excite_bwd(p(x), ldx, p(s), p(dy), lddy, p(dx), lddx, p(ds), N_, H, W, C_, cv, flags,
                                     p(ws_), Z(nbytes), dt, st)

    off = x.view(-1)[4:]                 # 8 bytes past a 16-byte boundary
    checks = [
        (fwd(x_=None), EINVAL), (fwd(y_=None), EINVAL), (fwd(x_=off), EINVAL), (fwd(dt=9), EINVAL),
        (fwd(act=0), EINVAL), (fwd(act=3), EINVAL), (fwd(b=None), EINVAL), (fwd(g=None), EINVAL),
        (fwd(P_=0), EINVAL), (fwd(cv=0), EINVAL), (fwd(ldx=8), EINVAL), (fwd(ldy=8), EINVAL),
        (fwd(C_=12, ldx=16, ldy=16), EALIGN), (fwd(cv=C + 1), EALIGN), (fwd(ldx=C + 4), EALIGN),
        (fwd(P_=1 << 28, ldx=16), EINVAL),                          # 2^32 elements
        (bwd(x_=None), EINVAL), (bwd(flags=1), EINVAL), (bwd(flags=4), EINVAL), (bwd(act=0), EINVAL),
        (bwd(dg_=None), EINVAL), (bwd(db_=None), EINVAL), (bwd(b=None), EINVAL), (bwd(ws_=None), EINVAL),
        (bwd(g=None, b=None), EINVAL),                              # dgamma / dbeta without an affine
        (bwd(nbytes=need_bn - 1), EWORKSPACE), (bwd(lddx=8), EINVAL), (bwd(lddy=C + 4), EALIGN),
        (bwd(C_=12), EALIGN), (bwd(P_=1 << 28), EINVAL), (bwd(dt=-1), EINVAL),
        (squeeze(x_=None), EINVAL), (squeeze(N_=0), EINVAL), (squeeze(H_=0), EINVAL), (squeeze(C_=12), EALIGN),
        (squeeze(cv=C + 1), EALIGN), (squeeze(ldx=8), EINVAL), (squeeze(nbytes=need_se - 1), EWORKSPACE),
        (squeeze(ws_=None), EINVAL), (squeeze(dt=7), EINVAL), (squeeze(N_=1 << 16), EINVAL),
        (squeeze(H_=1 << 26), EINVAL),
        (excite(s=None), EINVAL), (excite(ldy=8), EINVAL), (excite(C_=20), EALIGN), (excite(cv=0), EINVAL),
        (excite(dt=3), EINVAL), (excite(ldx=C + 4), EALIGN),
        (excite_bwd(s=None), EINVAL), (excite_bwd(flags=1), EINVAL), (excite_bwd(nbytes=need_se - 1), EWORKSPACE),
        (excite_bwd(lddx=8), EINVAL), (excite_bwd(ws_=None), EINVAL), (excite_bwd(cv=C + 8), EALIGN),
        (excite_bwd(N_=0), EINVAL),
    ]
    for i, (got, want) in enumerate(checks):
        assert got == want, (i, got, want)
    assert lib.seg_bn_act_bwd_workspace(0, C) == 0 and lib.seg_bn_act_bwd_workspace(P, 12) == 0
    assert lib.seg_se_squeeze_workspace(N, 0, W, C) == 0 and lib.seg_se_excite_bwd_workspace(N, H, W, 12) == 0
    torch.cuda.synchronize()
    for t in (y, dx, sq, ds, dg, db):
        assert bool(torch.isnan(t).all())
    assert bool((ws == 0xFF).all())
    # and the unedited calls run: ones through swish with the identity affine (eps 0), gates of 1/2
    assert lib.seg_bn_act_fwd(p(x), C, p(y), C, p(gamma), p(beta), 0.0, P, C, C, 1, ops.BF16, st) == 0
    assert excite_bwd() == 0 and squeeze() == 0
    torch.cuda.synchronize()
    assert abs(y[0, 0, 0, 0].item() - 0.731) < 4e-3 and bool((dx == 0.5).all())
    assert bool((ds == H * W).all()) and bool((sq == H * W).all())
