"""Helpers shared by the GPU parity tests (device tensors <-> oracle tensors)."""
import torch

from semanticsegmentation_tensorflow_amd import ops

TOL = {torch.float32: 2e-5, torch.bfloat16: 1.2e-2, torch.float16: 2e-3}


def to_dev(x, dtype, dev, cpad=None):
    """float64 NHWC -> padded device tensor [N,H,W,round8(C)] (zeros in padding)."""
    N, H, W, C = x.shape
    cp = cpad or ops.round8(C)
    t = torch.zeros(N, H, W, cp, dtype=dtype, device=dev)
    t[..., :C] = x.to(dtype).to(dev)
    return t


def from_dev(t, C=None):
    C = t.shape[-1] if C is None else C
    return t[..., :C].double().cpu()


def rnd(x, dtype):
    """Round a float64 tensor through `dtype` (what the device sees)."""
    return x.to(dtype).double()


def rel_err(a, b):
    a = a.double()
    b = b.double()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


_INT_OF = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}


def assert_bits_equal(got, ref, what=""):
    """Bit for bit (so -0.0 != +0.0); NaNs compared by position, not by payload."""
    got, ref = got.detach().cpu().reshape(-1), ref.detach().cpu().reshape(-1)
    assert got.dtype == ref.dtype and got.shape == ref.shape, f"{what}: {got.dtype}{tuple(got.shape)} vs " \
                                                              f"{ref.dtype}{tuple(ref.shape)}"
    gn, rn = torch.isnan(got), torch.isnan(ref)
    assert torch.equal(gn, rn), f"{what}: NaN positions differ ({int(gn.sum())} vs {int(rn.sum())})"
    it = _INT_OF[got.dtype]
    bad = ((got.view(it) != ref.view(it)) & ~gn).nonzero().reshape(-1)
    assert bad.numel() == 0, (f"{what}: {bad.numel()} of {got.numel()} elements differ, first at {bad[0].item()}: "
                              f"{got[bad[0]].item()!r} vs {ref[bad[0]].item()!r}")


# unit roundoffs: fp32 arithmetic (U) and the storage formats (U_DT)
U = 2.0 ** -24
U_DT = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def assert_within(got, ref, bound, what=""):
    """|got - ref| <= bound element by element (float64 tensors of one shape, on
    any one device); a NaN / Inf in got where ref is finite fails."""
    got, ref, bound = got.double(), ref.double(), bound.double()
    assert got.shape == ref.shape == bound.shape, f"{what}: {tuple(got.shape)} vs {tuple(ref.shape)}"
    err = (got - ref).abs()
    bad = ~(err <= bound)                       # also true for NaN
    n = int(bad.sum())
    if n:
        i = int(bad.reshape(-1).nonzero()[0])
        g, r, b = got.reshape(-1)[i].item(), ref.reshape(-1)[i].item(), bound.reshape(-1)[i].item()
        raise AssertionError(f"{what}: {n} of {got.numel()} elements out of bound, first at {i}: "
                             f"{g!r} vs {r!r} (|diff| {abs(g - r):.3e} > {b:.3e})")
    big = err / bound.clamp_min(1e-300)
    return float(big[bound > 0].max()) if bool((bound > 0).any()) else 0.0


def storage_bound(ref, dtype, fp32_term):
    """Rule for a result computed in fp32 and stored in `dtype`: the fp32 error
    term plus one rounding of the (possibly double-rounded) stored value."""
    return U_DT[dtype] * ref.abs() + fp32_term


def assert_surroundings(view, junk=50.0, what=""):
    """A channel-slice view's buffer still holds `junk` everywhere outside the view."""
    base = view._base
    assert base is not None and base.shape[:-1] == view.shape[:-1]
    lead = view.storage_offset() - base.storage_offset()
    cp = view.shape[-1]
    outside = torch.cat([base[..., :lead], base[..., lead + cp:]], dim=-1)
    assert bool((outside == junk).all()), f"{what}: bytes around the view changed"


def randn_normal(shape, gen, dtype, scale=1.0, floor=2.0 ** -6):
    """scale * randn rounded through `dtype`, magnitudes floored at `floor`: the
    values and their small multiples (x 0.25, x 1.25) stay normal in fp16."""
    x = torch.randn(shape, generator=gen, dtype=torch.float64) * scale
    x = torch.where(x.abs() < floor, torch.where(x < 0, -floor, floor).to(torch.float64), x)
    return rnd(x, dtype)


def nan_like_view(shape, dtype, dev, make_view):
    """An output buffer prefilled with NaN: dense, or (make_view: a function
    float64 NHWC -> device view) a channel-slice view."""
    full = torch.full(shape, float("nan"), dtype=torch.float64)
    return make_view(full) if make_view is not None else full.to(dtype).to(dev)


def tile_rows(t, P):
    """The first P rows of t [p0, ...] repeated along dim 0."""
    reps = (P + t.shape[0] - 1) // t.shape[0]
    return t.repeat(reps, *([1] * (t.dim() - 1)))[:P]


def packed_ref(src, mode, dtype, a_pad=None, b_pad=None, fill=0.0):
    """Host reference of a packed compute copy of the float master src [R,S,A,B]
    (seg_pack_filter's layouts): modes 1 / 2 dst[r,s,a,b], modes 0 / 3
    dst[b,r,s,a]; values src.to(dtype); the padding entries a in [A, a_pad),
    b in [B, b_pad) hold `fill` (0.0 after a pack; whatever the copy held
    before where a kernel leaves padding untouched)."""
    src = src.detach().cpu()
    R, S, A, B = src.shape
    ap = ops.round8(A) if a_pad is None else a_pad
    bp = ops.round8(B) if b_pad is None else b_pad
    out = torch.full((R, S, ap, bp), fill, dtype=dtype)
    out[:, :, :A, :B] = src.to(dtype)
    if mode in (ops.PACK_KRSC, ops.PACK_TCONV_BWD):
        out = out.permute(3, 0, 1, 2)
    return out.contiguous()


def assert_close(got, ref, dtype, what="", tol=None):
    tol = TOL[dtype] if tol is None else tol
    e = rel_err(got, ref)
    assert e <= tol, f"{what}: rel err {e:.3e} > {tol:.1e}"
    return e
