"""tests/transnet_ref.py (the float64 restatement the GPU kernels of
csrc/transnet.hip are compared against) pinned to torch autograd at 1e-12, and
the shared input generators checked for what the GPU tests rely on: a few
elements with z == 0 exactly, every other one with |z| >= 2^-12."""
import pytest
import torch

from tests import transnet_ref as R

TOL = 1e-12


def _close(a, b, what):
    err = (a - b).abs().max().item()
    assert err <= TOL * max(1.0, b.abs().max().item()), f"{what}: {err:.3e}"


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("alpha_bias", R.ALPHA_BIASES)
def test_film_matches_autograd(alpha_bias, relu):
    g = torch.Generator().manual_seed(11)
    alpha, f, beta = (torch.randn(2, 3, 4, 6, generator=g, dtype=torch.float64).requires_grad_(True)
                      for _ in range(3))
    dy = torch.randn(2, 3, 4, 6, generator=g, dtype=torch.float64)
    z = (alpha + alpha_bias) * f + beta
    y = torch.relu(z) if relu else z
    y.backward(dy)
    y_ref = R.film_fwd(alpha.detach(), f.detach(), beta.detach(), alpha_bias, relu)
    _close(y_ref, y.detach(), "y")
    da, df, db = R.film_bwd(dy, y_ref, alpha.detach(), f.detach(), alpha_bias, relu)
    _close(da, alpha.grad, "dalpha")
    _close(df, f.grad, "df")
    _close(db, beta.grad, "dbeta")


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("lam", R.LAMS)
def test_axpy_relu_matches_autograd(lam, relu):
    g = torch.Generator().manual_seed(12)
    a, b = (torch.randn(2, 3, 4, 6, generator=g, dtype=torch.float64).requires_grad_(True) for _ in range(2))
    dy = torch.randn(2, 3, 4, 6, generator=g, dtype=torch.float64)
    z = a + lam * b
    y = torch.relu(z) if relu else z
    y.backward(dy)
    y_ref = R.axpy_relu_fwd(a.detach(), b.detach(), lam, relu)
    _close(y_ref, y.detach(), "y")
    da, db = R.axpy_relu_bwd(dy, y_ref, lam, relu)
    _close(da, a.grad, "da")
    _close(db, b.grad, "db")


def test_relu_gradient_at_zero_is_zero():
    """TF's ReluGrad: the mask is y > 0, so z == 0 passes no gradient."""
    alpha = torch.tensor([-1.0, 0.5], dtype=torch.float64)
    f = torch.tensor([3.0, 2.0], dtype=torch.float64)
    beta = torch.tensor([0.0, -3.0], dtype=torch.float64)
    y = R.film_fwd(alpha, f, beta)
    assert y.tolist() == [0.0, 0.0]
    da, df, db = R.film_bwd(torch.ones(2, dtype=torch.float64), y, alpha, f)
    assert da.tolist() == [0.0, 0.0] and df.tolist() == [0.0, 0.0] and db.tolist() == [0.0, 0.0]
    zero = torch.zeros(1, dtype=torch.float64)
    da, db = R.axpy_relu_bwd(torch.ones(1, dtype=torch.float64), R.axpy_relu_fwd(zero, zero, 0.1), 0.1)
    assert da.item() == 0.0 and db.item() == 0.0


def test_autograd_wrappers_use_the_formulae():
    g = torch.Generator().manual_seed(13)
    alpha, f, beta, a = (torch.randn(5, 7, generator=g, dtype=torch.float64).requires_grad_(True) for _ in range(4))
    dy = torch.randn(5, 7, generator=g, dtype=torch.float64)
    y = R.AxpyRelu.apply(a, R.Film.apply(alpha, f, beta, 1.0, True), 0.1, True)
    y.backward(dy)
    got = [t.grad.clone() for t in (alpha, f, beta, a)]
    for t in (alpha, f, beta, a):
        t.grad = None
    torch.relu(a + 0.1 * torch.relu((alpha + 1.0) * f + beta)).backward(dy)
    for gt, t, n in zip(got, (alpha, f, beta, a), ("alpha", "f", "beta", "a")):
        _close(gt, t.grad, n)


def _weights(g, cin, cout, k):
    return torch.randn(k, k, cin, cout, generator=g, dtype=torch.float64) * (2.0 / (k * k * cin)) ** 0.5


def test_transnet_block_matches_autograd():
    """The whole block against the same expression written with torch.relu."""
    from oracle import tf1_ops as T
    g = torch.Generator().manual_seed(14)
    N, H, W, C = 2, 4, 5, 6
    p = {}
    for which, cin, k in (("alpha", 2 * C, 1), ("beta", 2 * C, 1), ("lid_feat", C, 1), ("fuse", C, 3)):
        p[f"t_{which}/weights"] = _weights(g, cin, C, k).requires_grad_(True)
    x_img = torch.randn(N, H, W, C, generator=g, dtype=torch.float64).requires_grad_(True)
    x_lid = torch.randn(N, H, W, C, generator=g, dtype=torch.float64).requires_grad_(True)
    dy = torch.randn(N, H, W, C, generator=g, dtype=torch.float64)
    leaves = [x_img, x_lid] + list(p.values())
    y = R.transnet(x_img, x_lid, p, "t")
    y.backward(dy)
    got = [t.grad.clone() for t in leaves]
    for t in leaves:
        t.grad = None

    def conv(x, which, pad):
        return T.conv2d(x, p[f"t_{which}/weights"], 1, pad)

    cat = torch.cat([x_img, x_lid], dim=-1)
    alpha = conv(cat, "alpha", "VALID") + 1
    lid = torch.relu(alpha * conv(x_lid, "lid_feat", "VALID") + conv(cat, "beta", "VALID"))
    y2 = torch.relu(x_img + R.LAM * conv(lid, "fuse", "SAME"))      # lamda as the fp32 number
    _close(y.detach(), y2.detach(), "y")
    y2.backward(dy)
    for i, (gt, t) in enumerate(zip(got, leaves)):
        _close(gt, t.grad, f"leaf {i}")
    assert all(float(gt.abs().max()) > 0 for gt in got)


@pytest.mark.parametrize("alpha_bias", R.ALPHA_BIASES)
@pytest.mark.parametrize("case", R.KERNEL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_film_inputs_pin_the_mask(case, alpha_bias):
    P, _, cv = case
    d = R.film_inputs(P, cv, R.film_seed(case, alpha_bias), alpha_bias)
    z = ((d["alpha"] + alpha_bias) * d["f"] + d["beta"]).reshape(-1)
    forced = torch.zeros(z.numel(), dtype=torch.bool)
    forced[d["forced"]] = True
    assert 1 <= len(d["forced"]) <= 5
    assert bool((z[forced] == 0).all())
    assert bool((z[~forced].abs() >= R.Z_MIN).all())
    for k in ("alpha", "f", "beta", "dy", "old_a", "old_f", "old_b"):      # exact in bf16, hence in f16 / f32
        assert torch.equal(d[k].to(torch.bfloat16).double(), d[k]) and torch.equal(d[k].half().double(), d[k])


@pytest.mark.parametrize("lam", R.LAMS)
@pytest.mark.parametrize("case", R.KERNEL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_axpy_inputs_pin_the_mask(case, lam):
    P, _, cv = case
    d = R.axpy_inputs(P, cv, R.axpy_seed(case, lam), lam)
    z = (d["a"] + lam * d["b"]).reshape(-1)
    forced = torch.zeros(z.numel(), dtype=torch.bool)
    forced[d["forced"]] = True
    assert bool((z[forced] == 0).all())
    assert bool((z[~forced].abs() >= R.Z_MIN).all())
    for k in ("a", "b", "dy", "old_a", "old_b"):
        assert torch.equal(d[k].to(torch.bfloat16).double(), d[k]) and torch.equal(d[k].half().double(), d[k])
