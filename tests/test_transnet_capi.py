"""The refusals of seg_film_* / seg_axpy_relu_* (csrc/transnet.hip) happen on the
host, before anything is launched: checked here with fake pointers that are
never touched, so it runs without a GPU.  (tests/test_gpu_transnet_kernels.py
repeats them on real NaN-filled buffers.)"""
import ctypes

from semanticsegmentation_tensorflow_amd import _lib

EINVAL, EALIGN = 1, 3
BF16, F32 = 1, 0
FAKE = 1 << 20
P, C = 24, 16


def _p(v):
    return None if v is None else ctypes.c_void_p(v)


def test_film_refusals():
    lib = _lib.load()

    def fwd(a=FAKE, lda=C, f=FAKE, ldf=C, b=FAKE, ldb=C, y=FAKE, ldy=C, P_=P, C_=C, cv=C, relu=1, dt=BF16):
        return lib.seg_film_fwd(_p(a), lda, _p(f), ldf, _p(b), ldb, _p(y), ldy, 1.0, P_, C_, cv, relu, dt, None)

    def bwd(dy=FAKE, lddy=C, y=FAKE, ldy=C, a=FAKE, lda=C, f=FAKE, ldf=C, da=FAKE, ldda=C, df=FAKE, lddf=C, db=FAKE,
            lddb=C, P_=P, C_=C, cv=C, flags=1, dt=BF16):
        return lib.seg_film_bwd(_p(dy), lddy, _p(y), ldy, _p(a), lda, _p(f), ldf, _p(da), ldda, _p(df), lddf, _p(db),
                                lddb, 1.0, P_, C_, cv, flags, dt, None)

    checks = [
        (fwd(a=None), EINVAL), (fwd(f=None), EINVAL), (fwd(b=None), EINVAL), (fwd(y=None), EINVAL),
        (fwd(a=FAKE + 8), EINVAL), (fwd(y=FAKE + 2), EINVAL), (fwd(dt=3), EINVAL), (fwd(dt=-1), EINVAL),
        (fwd(relu=2), EINVAL), (fwd(P_=0), EINVAL), (fwd(C_=0), EINVAL), (fwd(cv=0), EINVAL),
        (fwd(lda=8), EINVAL), (fwd(ldf=8), EINVAL), (fwd(ldb=8), EINVAL), (fwd(ldy=8), EINVAL),
        (fwd(P_=1 << 27), EINVAL),
        (fwd(C_=12), EALIGN), (fwd(cv=C + 1), EALIGN), (fwd(lda=C + 4), EALIGN),
        (fwd(dt=F32, lda=C + 2), EALIGN),                   # in fp32 four elements are a whole chunk
        (bwd(dy=None), EINVAL), (bwd(y=None), EINVAL), (bwd(a=None), EINVAL), (bwd(f=None), EINVAL),
        (bwd(da=None, df=None, db=None), EINVAL), (bwd(flags=16), EINVAL), (bwd(da=FAKE + 4), EINVAL),
        (bwd(ldda=8), EINVAL), (bwd(lddf=8), EINVAL), (bwd(lddb=8), EINVAL), (bwd(lddy=C + 4), EALIGN),
        (bwd(C_=12), EALIGN), (bwd(cv=C + 8), EALIGN), (bwd(P_=1 << 27), EINVAL), (bwd(dt=9), EINVAL),
    ]
    for i, (got, want) in enumerate(checks):
        assert got == want, (i, got, want)


def test_axpy_relu_refusals():
    lib = _lib.load()

    def fwd(a=FAKE, lda=C, b=FAKE, ldb=C, y=FAKE, ldy=C, P_=P, C_=C, cv=C, relu=1, dt=BF16):
        return lib.seg_axpy_relu_fwd(_p(a), lda, _p(b), ldb, _p(y), ldy, 0.1, P_, C_, cv, relu, dt, None)

    def bwd(dy=FAKE, lddy=C, y=FAKE, ldy=C, da=FAKE, ldda=C, db=FAKE, lddb=C, P_=P, C_=C, cv=C, flags=1, dt=BF16):
        return lib.seg_axpy_relu_bwd(_p(dy), lddy, _p(y), ldy, _p(da), ldda, _p(db), lddb, 0.1, P_, C_, cv, flags, dt,
                                     None)

    checks = [
        (fwd(a=None), EINVAL), (fwd(b=None), EINVAL), (fwd(y=None), EINVAL), (fwd(b=FAKE + 8), EINVAL),
        (fwd(dt=3), EINVAL), (fwd(relu=-1), EINVAL), (fwd(P_=-1), EINVAL), (fwd(cv=0), EINVAL),
        (fwd(lda=8), EINVAL), (fwd(ldy=8), EINVAL), (fwd(P_=1 << 27), EINVAL),
        (fwd(C_=20), EALIGN), (fwd(cv=C + 1), EALIGN), (fwd(ldb=C + 4), EALIGN),
        (bwd(dy=None), EINVAL), (bwd(y=None), EINVAL), (bwd(da=None, db=None), EINVAL), (bwd(flags=8), EINVAL),
        (bwd(ldda=8), EINVAL), (bwd(lddb=C + 4), EALIGN), (bwd(C_=12), EALIGN), (bwd(cv=C + 1), EALIGN),
        (bwd(P_=0), EINVAL), (bwd(dt=5), EINVAL), (bwd(P_=1 << 27), EINVAL),
    ]
    for i, (got, want) in enumerate(checks):
        assert got == want, (i, got, want)
