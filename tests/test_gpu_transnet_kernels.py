"""seg_film_fwd / _bwd and seg_axpy_relu_fwd / _bwd (csrc/transnet.hip) against
tests/transnet_ref.py in f32, bf16 and f16, dense and through channel slices
of a wider tensor of JUNK.  Destinations start as NaN and the padding channels
of every input (and of every accumulated-into output) hold PAD, not zero, so a
skipped element or a padding channel left to the arithmetic shows.

Inputs are bf16 values with magnitudes floored at 2^-6 (exact in the three
dtypes), alpha_bias / lam the fp32 numbers the library receives, so one float64
reference serves the three dtypes.  A fixed handful of elements has z == 0
exactly (the gradient there must be 0: the mask is y > 0) and every other one
|z| >= 2^-12 (tests/test_transnet_ref.py asserts both with these seeds), far
above the error of z, so no element can flip and none is excluded.

Bounds, from the operations the kernels use (u = 2^-24 = U):
* t = alpha + alpha_bias: one rounding, u |t|.  z = fma(t, f, beta): u |t f|
  from t, and one rounding u |z|.      film y:   u (|t f| + |y|)
* z = fma(lam, b, a): one rounding.     axpy y:   u |y|
* dz = dy or 0: exact.                  dbeta, da: 0
* dalpha = dz * f: one product.                   u |dalpha|
* df = dz * t: t's rounding and one product.      2u |df|
* db = lam * dz: one product.                     u |db|
* accumulation new + old: one more rounding,      u (|new| + |old|)
each plus storage_bound's rounding into T; an accumulated sum can cancel into
f16's subnormal range, so those add half a subnormal spacing (SUB).
The fraction of each bound used is printed (DESIGN.md section 13 records it).
Two runs are bit-identical; refused calls leave everything untouched."""
import functools

import pytest
import torch

from semanticsegmentation_tensorflow_amd import _lib, ops
from tests import transnet_ref as R
from tests.gpu_utils import U, assert_bits_equal, assert_surroundings, assert_within, storage_bound

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SUB = {torch.float32: 2.0 ** -150, torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}
JUNK, PAD = 50.0, 3.0
EINVAL, EALIGN = 1, 3
BIG = R.KERNEL_CASES[-1]
_id = lambda c: "x".join(str(int(v)) for v in c)     # noqa: E731


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


def nan_out(P, C, dtype, dev, sliced):
    return put(torch.full((1, 1, P, C), float("nan"), dtype=torch.float64), C, dtype, dev, sliced)


def zeros64(t):
    return torch.zeros_like(t)


def check(got_dev, ref, fp32_term, cv, dtype, what, sub=False):
    got = got_dev.double().cpu()
    assert bool((got[..., cv:] == 0).all()), what + ": padding channels must be exact zeros"
    bound = storage_bound(ref, dtype, fp32_term) + (SUB[dtype] if sub else 0.0)
    return assert_within(got[..., :cv], ref, bound, what)


@functools.lru_cache(maxsize=None)
def film_reference(case, alpha_bias, relu):
    P, C, cv = case
    d = R.film_inputs(P, cv, R.film_seed(case, alpha_bias), alpha_bias)
    y = R.film_fwd(d["alpha"], d["f"], d["beta"], alpha_bias, relu)
    da, df, db = R.film_bwd(d["dy"], y, d["alpha"], d["f"], alpha_bias, relu)
    tf_ = ((d["alpha"] + alpha_bias) * d["f"]).abs()
    flat = y.reshape(-1)
    if relu:                                  # the forced zeros pass no gradient
        assert all(flat[i].item() == 0 and db.reshape(-1)[i].item() == 0 for i in d["forced"])
    return d, y, da, df, db, U * (tf_ + y.abs())


def run_film(dev, case, dt, sliced, alpha_bias, relu, variants):
    P, C, cv = case
    dtype = DTYPES[dt]
    d, y_ref, da_ref, df_ref, db_ref, b_y = film_reference(case, alpha_bias, relu)
    what = f"film {case} {dt} sliced={sliced} bias={alpha_bias} relu={relu}"
    ad, fd, bd, dyd = (put(d[k], C, dtype, dev, sliced) for k in ("alpha", "f", "beta", "dy"))
    yd, yd2 = nan_out(P, C, dtype, dev, sliced), nan_out(P, C, dtype, dev, sliced)
    ops.film_fwd(ad, fd, bd, yd, cv, alpha_bias, relu)
    ops.film_fwd(ad, fd, bd, yd2, cv, alpha_bias, relu)
    torch.cuda.synchronize()
    assert_bits_equal(yd, yd2, what + " y twice")
    fr = {"y": check(yd, y_ref, b_y, cv, dtype, what + " y")}
    views = [ad, fd, bd, dyd, yd]
    refs = (da_ref, df_ref, db_ref)
    olds = (d["old_a"], d["old_f"], d["old_b"])
    terms = (U * da_ref.abs(), 2 * U * df_ref.abs(), zeros64(db_ref))
    first = None
    for acc, null in variants:
        outs = []
        for i in range(3):
            if i == null:
                outs.append(None)
            elif acc[i]:
                outs.append(put(olds[i], C, dtype, dev, sliced))       # PAD in the output's own padding
            else:
                outs.append(nan_out(P, C, dtype, dev, sliced))
        # the stored y the mask is read from is the device's own
        ops.film_bwd(dyd, yd, ad, fd, outs[0], outs[1], outs[2], cv, alpha_bias, relu, acc)
        torch.cuda.synchronize()
        for i, n in enumerate(("dalpha", "df", "dbeta")):
            if outs[i] is None:
                continue
            views.append(outs[i])
            ref, term = refs[i], terms[i]
            if acc[i]:
                term = term + U * (ref.abs() + olds[i].abs())
                ref = ref + olds[i]
            key = n + ("+=" if acc[i] else "")
            fr[key] = max(fr.get(key, 0.0), check(outs[i], ref, term, cv, dtype, f"{what} {key} acc={acc} null={null}",
                                                  sub=acc[i]))
        if acc == (False, False, False) and null is None:
            if first is None:
                first = outs
            else:
                for a, b in zip(first, outs):
                    assert_bits_equal(a, b, what + " gradient twice")
    if sliced:
        for v in views:
            assert_surroundings(v, JUNK, what)
    print(f"{what}: fraction of the bound used: " + " ".join(f"{k} {v:.3f}" for k, v in fr.items()))


NONE3 = (False, False, False)
FILM_VARIANTS = [(NONE3, None), (NONE3, None), ((True, True, True), None), ((True, False, False), None),
                 ((False, True, False), None), ((False, False, True), None), (NONE3, 0), (NONE3, 1), (NONE3, 2),
                 ((True, True, True), 1)]


@pytest.mark.parametrize("sliced", [False, True])
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("case", R.KERNEL_CASES[:-1], ids=_id)
def test_film_fwd_bwd(dev, case, dt, sliced):
    for alpha_bias in R.ALPHA_BIASES:
        for relu in (True, False):
            run_film(dev, case, dt, sliced, alpha_bias, relu, FILM_VARIANTS)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_film_more_pixels_than_one_sweep_of_the_grid(dev, dt):
    """524325 pixels of 8 channels: 37 past one sweep of the capped grid in the
    16-bit dtypes, two sweeps and 37 in f32."""
    run_film(dev, BIG, dt, False, 1.0, True, [(NONE3, None), ((True, True, True), None)])


@functools.lru_cache(maxsize=None)
def axpy_reference(case, lam, relu):
    P, C, cv = case
    d = R.axpy_inputs(P, cv, R.axpy_seed(case, lam), lam)
    y = R.axpy_relu_fwd(d["a"], d["b"], lam, relu)
    da, db = R.axpy_relu_bwd(d["dy"], y, lam, relu)
    if relu:
        assert all(y.reshape(-1)[i].item() == 0 and da.reshape(-1)[i].item() == 0 for i in d["forced"])
    return d, y, da, db


def run_axpy(dev, case, dt, sliced, lam, relu, variants):
    P, C, cv = case
    dtype = DTYPES[dt]
    d, y_ref, da_ref, db_ref = axpy_reference(case, lam, relu)
    what = f"axpy {case} {dt} sliced={sliced} lam={lam:.3g} relu={relu}"
    ad, bd, dyd = (put(d[k], C, dtype, dev, sliced) for k in ("a", "b", "dy"))
    yd, yd2 = nan_out(P, C, dtype, dev, sliced), nan_out(P, C, dtype, dev, sliced)
    ops.axpy_relu_fwd(ad, bd, yd, cv, lam, relu)
    ops.axpy_relu_fwd(ad, bd, yd2, cv, lam, relu)
    torch.cuda.synchronize()
    assert_bits_equal(yd, yd2, what + " y twice")
    fr = {"y": check(yd, y_ref, U * y_ref.abs(), cv, dtype, what + " y")}
    views = [ad, bd, dyd, yd]
    refs, olds = (da_ref, db_ref), (d["old_a"], d["old_b"])
    terms = (zeros64(da_ref), U * db_ref.abs())
    first = None
    for acc, null in variants:
        outs = []
        for i in range(2):
            if i == null:
                outs.append(None)
            elif acc[i]:
                outs.append(put(olds[i], C, dtype, dev, sliced))
            else:
                outs.append(nan_out(P, C, dtype, dev, sliced))
        ops.axpy_relu_bwd(dyd, yd, outs[0], outs[1], cv, lam, relu, acc)
        torch.cuda.synchronize()
        for i, n in enumerate(("da", "db")):
            if outs[i] is None:
                continue
            views.append(outs[i])
            ref, term = refs[i], terms[i]
            if acc[i]:
                term = term + U * (ref.abs() + olds[i].abs())
                ref = ref + olds[i]
            key = n + ("+=" if acc[i] else "")
            fr[key] = max(fr.get(key, 0.0), check(outs[i], ref, term, cv, dtype, f"{what} {key} acc={acc} null={null}",
                                                  sub=acc[i]))
        if acc == (False, False) and null is None:
            if first is None:
                first = outs
            else:
                for a, b in zip(first, outs):
                    assert_bits_equal(a, b, what + " gradient twice")
    if sliced:
        for v in views:
            assert_surroundings(v, JUNK, what)
    print(f"{what}: fraction of the bound used: " + " ".join(f"{k} {v:.3f}" for k, v in fr.items()))


NONE2 = (False, False)
AXPY_VARIANTS = [(NONE2, None), (NONE2, None), ((True, True), None), ((True, False), None), ((False, True), None),
                 (NONE2, 0), (NONE2, 1), ((True, True), 0)]


@pytest.mark.parametrize("sliced", [False, True])
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("case", R.KERNEL_CASES[:-1], ids=_id)
def test_axpy_relu_fwd_bwd(dev, case, dt, sliced):
    for lam in R.LAMS:
        for relu in (True, False):
            run_axpy(dev, case, dt, sliced, lam, relu, AXPY_VARIANTS)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_axpy_more_pixels_than_one_sweep_of_the_grid(dev, dt):
    run_axpy(dev, BIG, dt, False, R.LAM, True, [(NONE2, None), ((True, True), None)])


def test_operands_of_a_skipped_output_may_be_null(dev):
    """dalpha alone reads f but not alpha; df alone reads alpha but not f;
    without the ReLU y is not read."""
    P, C = 5, 8
    dtype = torch.float32
    dy = torch.full((1, 1, P, C), 2.0, dtype=dtype, device=dev)
    alpha = torch.full_like(dy, 0.5)
    f = torch.full_like(dy, 3.0)
    nan = lambda: torch.full_like(dy, float("nan"))     # noqa: E731
    da, df, db = nan(), nan(), nan()
    ops.film_bwd(dy, None, None, f, da, None, None, C, 1.0, relu=False)
    ops.film_bwd(dy, None, alpha, None, None, df, None, C, 1.0, relu=False)
    ops.film_bwd(dy, None, None, None, None, None, db, C, 1.0, relu=False)
    torch.cuda.synchronize()
    assert bool((da == 6.0).all()) and bool((df == 3.0).all()) and bool((db == 2.0).all())


def test_refused_calls_write_nothing(dev):
    lib = _lib.lib()
    dtype = torch.bfloat16
    P, C = 24, 16
    nanf = lambda: torch.full((1, 1, P, C), float("nan"), dtype=dtype, device=dev)     # noqa: E731
    x = torch.ones(1, 1, P, C, dtype=dtype, device=dev)
    y, da, df, db = nanf(), nanf(), nanf(), nanf()
    st = ops.stream_ptr()
    p = ops.ptr
    off = x.view(-1)[4:]                 # 8 bytes past a 16-byte boundary

    def ffwd(a=x, lda=C, f=x, ldf=C, b=x, ldb=C, y_=y, ldy=C, P_=P, C_=C, cv=C, relu=1, dt=ops.BF16):
        return lib.seg_film_fwd(p(a), lda, p(f), ldf, p(b), ldb, p(y_), ldy, 1.0, P_, C_, cv, relu, dt, st)

    def fbwd(dy=x, lddy=C, y_=x, ldy=C, a=x, lda=C, f=x, ldf=C, da_=da, ldda=C, df_=df, lddf=C, db_=db, lddb=C, P_=P,
             C_=C, cv=C, flags=1, dt=ops.BF16):
        return lib.seg_film_bwd(p(dy), lddy, p(y_), ldy, p(a), lda, p(f), ldf, p(da_), ldda, p(df_), lddf, p(db_),
                                lddb, 1.0, P_, C_, cv, flags, dt, st)

    def afwd(a=x, lda=C, b=x, ldb=C, y_=y, ldy=C, P_=P, C_=C, cv=C, relu=1, dt=ops.BF16):
        return lib.seg_axpy_relu_fwd(p(a), lda, p(b), ldb, p(y_), ldy, 0.5, P_, C_, cv, relu, dt, st)

    def abwd(dy=x, lddy=C, y_=x, ldy=C, da_=da, ldda=C, db_=db, lddb=C, P_=P, C_=C, cv=C, flags=1, dt=ops.BF16):
        return lib.seg_axpy_relu_bwd(p(dy), lddy, p(y_), ldy, p(da_), ldda, p(db_), lddb, 0.5, P_, C_, cv, flags, dt,
                                     st)

    checks = [
        (ffwd(a=None), EINVAL), (ffwd(f=None), EINVAL), (ffwd(b=None), EINVAL), (ffwd(y_=None), EINVAL),
        (ffwd(a=off), EINVAL), (ffwd(dt=9), EINVAL), (ffwd(relu=2), EINVAL), (ffwd(P_=0), EINVAL),
        (ffwd(cv=0), EINVAL), (ffwd(C_=0), EINVAL), (ffwd(lda=8), EINVAL), (ffwd(ldy=8), EINVAL),
        (ffwd(C_=12), EALIGN), (ffwd(cv=C + 1), EALIGN), (ffwd(ldf=C + 4), EALIGN), (ffwd(ldb=C + 4), EALIGN),
        (ffwd(P_=1 << 27), EINVAL),                                 # 2^31 elements
        (fbwd(dy=None), EINVAL), (fbwd(y_=None), EINVAL), (fbwd(a=None), EINVAL), (fbwd(f=None), EINVAL),
        (fbwd(da_=None, df_=None, db_=None), EINVAL), (fbwd(flags=16), EINVAL), (fbwd(flags=-1), EINVAL),
        (fbwd(da_=off), EINVAL), (fbwd(ldda=8), EINVAL), (fbwd(lddf=C + 4), EALIGN), (fbwd(lddb=8), EINVAL),
        (fbwd(C_=12), EALIGN), (fbwd(cv=C + 8), EALIGN), (fbwd(P_=1 << 27), EINVAL), (fbwd(dt=-1), EINVAL),
        (fbwd(P_=-3), EINVAL),
        (afwd(a=None), EINVAL), (afwd(b=off), EINVAL), (afwd(y_=None), EINVAL), (afwd(relu=-1), EINVAL),
        (afwd(C_=20), EALIGN), (afwd(ldb=8), EINVAL), (afwd(lda=C + 4), EALIGN), (afwd(dt=3), EINVAL),
        (afwd(P_=1 << 27), EINVAL), (afwd(cv=0), EINVAL),
        (abwd(dy=None), EINVAL), (abwd(y_=None), EINVAL), (abwd(da_=None, db_=None), EINVAL), (abwd(flags=8), EINVAL),
        (abwd(ldda=8), EINVAL), (abwd(lddb=C + 4), EALIGN), (abwd(C_=12), EALIGN), (abwd(cv=C + 1), EALIGN),
        (abwd(P_=0), EINVAL), (abwd(dt=5), EINVAL),
    ]
    for i, (got, want) in enumerate(checks):
        assert got == want, (i, got, want)
    torch.cuda.synchronize()
    for t in (y, da, df, db):
        assert bool(torch.isnan(t).all())
    # and the unedited calls run: (1 + 1) * 1 + 1 = 3, 1 + 0.5 = 1.5
    assert ffwd() == 0 and fbwd() == 0
    torch.cuda.synchronize()
    assert bool((y == 3.0).all()) and bool((da == 1.0).all()) and bool((df == 2.0).all()) and bool((db == 1.0).all())
    assert afwd() == 0 and abwd() == 0
    torch.cuda.synchronize()
    assert bool((y == 1.5).all()) and bool((da == 1.0).all()) and bool((db == 0.5).all())
