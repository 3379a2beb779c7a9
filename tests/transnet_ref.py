"""float64 restatements of the TransNet operations of csrc/transnet.hip
(Network/model/FCDenseNet_TransNet.py:70-86) and their gradients, written out
as formulae -- no autograd; tests/test_transnet_ref.py pins them to torch's.
The ReLU gradient at zero is TF's ReluGrad: dz = dy where y > 0, else 0.

Also the input generators shared by the CPU and the GPU tests: values rounded
through bf16 with magnitudes floored at 2^-6 (exact in f32 / bf16 / f16), a
fixed handful of elements forced to z == 0 exactly, every other element
resampled until |z| >= Z_MIN, so no rounding of z can move an element across
the ReLU mask."""
import numpy as np
import torch

from oracle import tf1_ops as T

Z_MIN = 2.0 ** -12
LAM = float(np.float32(0.1))        # lamda as the fp32 number the library receives


def film_fwd(alpha, f, beta, alpha_bias=1.0, relu=True):
    z = (alpha + alpha_bias) * f + beta
    return torch.where(z > 0, z, torch.zeros_like(z)) if relu else z


def film_bwd(dy, y, alpha, f, alpha_bias=1.0, relu=True):
    """(dalpha, df, dbeta); the mask is read from the stored y."""
    dz = torch.where(y > 0, dy, torch.zeros_like(dy)) if relu else dy
    return dz * f, dz * (alpha + alpha_bias), dz


def axpy_relu_fwd(a, b, lam, relu=True):
    z = a + lam * b
    return torch.where(z > 0, z, torch.zeros_like(z)) if relu else z


def axpy_relu_bwd(dy, y, lam, relu=True):
    """(da, db)."""
    dz = torch.where(y > 0, dy, torch.zeros_like(dy)) if relu else dy
    return dz, lam * dz


class Film(torch.autograd.Function):
    """film_fwd / film_bwd as one differentiable op (for model restatements)."""

    @staticmethod
    def forward(ctx, alpha, f, beta, alpha_bias, relu):
        y = film_fwd(alpha, f, beta, alpha_bias, relu)
        ctx.save_for_backward(y, alpha, f)
        ctx.args = (alpha_bias, relu)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, alpha, f = ctx.saved_tensors
        da, df, db = film_bwd(dy, y, alpha, f, *ctx.args)
        return da, df, db, None, None


class AxpyRelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, lam, relu):
        y = axpy_relu_fwd(a, b, lam, relu)
        ctx.save_for_backward(y)
        ctx.args = (lam, relu)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        da, db = axpy_relu_bwd(dy, y, *ctx.args)
        return da, db, None, None


def transnet(x_img, x_lid, p, name, lamda=0.1, rt=lambda t: t):
    """The TransNet block (bias-free convs): p maps "<name>_alpha/weights" etc.
    (HWIO float64) to tensors; rt rounds at the device's storage points
    (identity in float64).  Differentiable through torch autograd with the
    ReluGrad convention above."""
    cat = torch.cat([x_img, x_lid], dim=-1)

    def conv(x, which, k=1):
        return rt(T.conv2d(x, p[f"{name}_{which}/weights"], 1, "VALID" if k == 1 else "SAME"))

    alpha, beta, lid = conv(cat, "alpha"), conv(cat, "beta"), conv(x_lid, "lid_feat")
    mod = rt(Film.apply(alpha, lid, beta, 1.0, True))
    fuse = conv(mod, "fuse", 3)
    return rt(AxpyRelu.apply(x_img, fuse, float(np.float32(lamda)), True))


def _bf16(x):
    return x.to(torch.bfloat16).double()


def _randn(shape, g, floor=2.0 ** -6):
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    x = torch.where(x.abs() < floor, torch.where(x < 0, -floor, floor).to(torch.float64), x)
    return _bf16(x)


def forced_zero_index(n):
    """The fixed handful of flat indices whose z is forced to exactly 0."""
    return sorted({0, n // 3, n // 2, (2 * n) // 3, n - 1})


def film_inputs(P, cv, seed, alpha_bias):
    """dict of [1, 1, P, cv] float64 tensors: alpha, f, beta, dy, old_a, old_f,
    old_b; `forced` the flat indices with z == 0."""
    g = torch.Generator().manual_seed(seed)
    shape = (1, 1, P, cv)
    alpha, f, beta = _randn(shape, g), _randn(shape, g), _randn(shape, g)
    forced = forced_zero_index(P * cv)
    keep = torch.zeros(P * cv, dtype=torch.bool)
    keep[forced] = True
    keep = keep.reshape(shape)
    for _ in range(100):
        bad = (((alpha + alpha_bias) * f + beta).abs() < Z_MIN) & ~keep
        if not bool(bad.any()):
            break
        alpha = torch.where(bad, _randn(shape, g), alpha)
        f = torch.where(bad, _randn(shape, g), f)
        beta = torch.where(bad, _randn(shape, g), beta)
    else:
        raise AssertionError("resampling did not converge")
    alpha = torch.where(keep, torch.full_like(alpha, -alpha_bias), alpha)
    beta = torch.where(keep, torch.zeros_like(beta), beta)
    out = dict(alpha=alpha, f=f, beta=beta, forced=forced)
    for k in ("dy", "old_a", "old_f", "old_b"):
        out[k] = _randn(shape, g)
    return out


def axpy_inputs(P, cv, seed, lam):
    """a, b, dy, old_a, old_b; z == 0 forced with a = b = 0."""
    g = torch.Generator().manual_seed(seed)
    shape = (1, 1, P, cv)
    a, b = _randn(shape, g), _randn(shape, g)
    forced = forced_zero_index(P * cv)
    keep = torch.zeros(P * cv, dtype=torch.bool)
    keep[forced] = True
    keep = keep.reshape(shape)
    for _ in range(100):
        bad = ((a + lam * b).abs() < Z_MIN) & ~keep
        if not bool(bad.any()):
            break
        a = torch.where(bad, _randn(shape, g), a)
        b = torch.where(bad, _randn(shape, g), b)
    else:
        raise AssertionError("resampling did not converge")
    a = torch.where(keep, torch.zeros_like(a), a)
    b = torch.where(keep, torch.zeros_like(b), b)
    out = dict(a=a, b=b, forced=forced)
    for k in ("dy", "old_a", "old_b"):
        out[k] = _randn(shape, g)
    return out


# (P, C, c_valid) of the kernel tests.  The last one: csrc/transnet.hip walks
# C = 8 with 256 (16-bit) or 128 (f32) pixel rows per workgroup and at most
# 2048 workgroups, so one sweep of the grid is 524288 (262144) pixels; 524325
# is 37 more and no multiple of either row count.
KERNEL_CASES = [
    (1, 8, 1),
    (3, 8, 5),
    (37, 16, 16),
    (90, 144, 143),          # the 5x18 map at batch 1
    (1100, 80, 76),
    (6, 1152, 1152),         # more than one chunk group in f32
    (524325, 8, 5),
]
ALPHA_BIASES = (1.0, 0.0)
LAMS = (LAM, 1.0)


def film_seed(case, alpha_bias):
    return 500 + 2 * KERNEL_CASES.index(case) + ALPHA_BIASES.index(alpha_bias)


def axpy_seed(case, lam):
    return 600 + 2 * KERNEL_CASES.index(case) + LAMS.index(lam)
