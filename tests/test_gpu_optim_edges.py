"""The kernels between a gradient and the next forward pass, at their edges:
the multi-tensor Adam + pack launch (adam_pack_k, csrc/optim.hip) and its
pack-only form (seg_pack_segments), seg_pack_filter, the fused filter-gradient
+ Adam epilogue of igemm_tn3 with rows_to_tr_k in the forms backward.py calls
it, and the deferred BatchNorm finish (bn_fold_batch_k / bn_finish_batch_k).

One host reference for a packed compute copy is used throughout
(gpu_utils.packed_ref: a permutation of master.to(dtype), compared bit for bit).
Adam is compared with oracle/tf1_ops.AdamTF1 in float64 on the hyper-parameters
as the kernel receives them, under the bounds of
test_adam_small_sizes_and_gradient_scales (optim.hip: the arithmetic is
adam_k's): 1e-6 max-relative for p and v, 1e-6 * max|grad_scale * g| for m, per
variable as well as over the whole buffer."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import tf1_ops as tf_ref
from semanticsegmentation_tensorflow_amd import _lib, ops
from tests.gpu_utils import assert_bits_equal, assert_close, packed_ref, rnd, to_dev

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DT_IDS = ["f32", "bf16", "f16"]
DT = {torch.float32: ops.F32, torch.bfloat16: ops.BF16, torch.float16: ops.F16}
TCONV_MODES = (ops.PACK_TCONV_FWD, ops.PACK_TCONV_BWD)
ROWS_MODES = (ops.PACK_HWIO, ops.PACK_TCONV_FWD)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.fixture
def knob(dev):
    """set(name, value) for a kernel-selection knob; every knob set through it
    gets its earlier value back when the test ends."""
    saved = {}

    def set_(name, value):
        saved.setdefault(name, ops.get_option(name))
        ops.set_option(name, value)
    yield set_
    for name, value in saved.items():
        ops.set_option(name, value)


# ---------------------------------------------------------------------------
# 1. seg_pack_filter against the host permutation
# ---------------------------------------------------------------------------
# (shape [R,S,A,B], a_pad or None = round8(A), modes)
PACK_CASES = [((3, 3, 3, 64), None, (0, 1, 2, 3)),
              ((1, 1, 40, 2), None, (0, 1, 2, 3)),
              ((3, 3, 72, 136), None, (0, 1, 2, 3)),       # 2 x 3 transpose tiles of 64 x 64, ragged edges
              ((7, 7, 8, 8), None, (0, 1, 2, 3)),
              ((1, 1, 1, 1), None, (0, 1, 2, 3)),
              ((16, 16, 2, 256), 2, TCONV_MODES),          # tap-dense tconv copies: a_pad = the true channel count
              ((16, 16, 4, 16), 4, TCONV_MODES)]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", PACK_CASES, ids=lambda c: "x".join(map(str, c[0])))
def test_pack_filter_is_the_host_permutation(dev, case, dtype):
    """Every entry of dst is written (it starts as NaN), valid entries are
    src.to(dtype) at the mode's position, padding entries are +0.0."""
    shape, a_pad, modes = case
    R, S, A, B = shape
    src = torch.randn(shape, generator=_gen(sum(shape)))
    src.view(-1)[::5] *= 300.0                             # some magnitudes past the fp16 range of small values
    ap, bp = a_pad or ops.round8(A), ops.round8(B)
    srcd = src.to(dev)
    for mode in modes:
        dst = torch.full(ops.packed_shape(R, S, A, B, mode, ap), float("nan"), dtype=dtype, device=dev)
        ops.pack_filter(srcd, dst, ap, bp, mode)
        torch.cuda.synchronize()
        assert_bits_equal(dst, packed_ref(src, mode, dtype, ap, bp), f"pack_filter {shape} mode {mode}")
    assert torch.equal(srcd.cpu(), src)


# ---------------------------------------------------------------------------
# 2 / 3. seg_adam_tf1_pack against float64, seg_pack_segments
# ---------------------------------------------------------------------------
# adam_pack_k tiles a variable viewed as [rs][a][b] into 32 x 128 tiles [a][b];
# float4 updates need b % 4 == 0 and an offset that is a multiple of 4.
# (shape, packed copies, a_pad or None = round8(A), offset mod 4)
K_, H_ = ops.PACK_KRSC, ops.PACK_HWIO
TF_, TB_ = ops.PACK_TCONV_FWD, ops.PACK_TCONV_BWD
ADAM_PLANS = {
    "multi": [((3, 3, 3, 64), (K_,), None, 0),
              ((3, 3, 72, 136), (K_, H_), None, 0),        # 3 x 2 tiles per tap, ragged in a and b
              ((4, 4, 2, 64), (TF_, TB_), None, 0),        # general tconv: a_pad = 8
              ((64,), (), None, 0),
              ((2,), (), None, 2),
              ((1, 1, 40, 2), (K_, H_), None, 0),
              ((16, 16, 2, 256), (TF_, TB_), 2, 0),        # tap-dense tconv: a_pad = 2
              ((16, 16, 4, 16), (TF_, TB_), 4, 0),         # tap-dense tconv: a_pad = 4
              ((1,), (), None, 3),
              ((129,), (), None, 1),
              ((1, 1, 1, 1), (), None, 2),
              ((1, 1, 31, 127), (H_,), None, 0),
              ((1, 1, 32, 128), (K_,), None, 1),           # b % 4 == 0 at an offset of residue 1: scalar updates
              ((1, 1, 33, 129), (K_, H_), None, 3),
              ((1, 1, 33, 260), (H_,), None, 0),           # three b tiles
              ((1, 2, 31, 3), (K_,), None, 2),
              ((1, 1, 72, 1), (K_, H_), None, 1),
              ((1, 1, 1, 260), (), None, 0),
              ((1, 1, 32, 136), (H_,), None, 2),           # vector-sized rows, residue 2
              ((2, 2, 33, 128), (), None, 3),              # vector-sized rows, residue 3
              ((1, 1, 32, 128), (K_, H_), None, 0)],       # one exact tile on the float4 path
    "single": [((3, 3, 72, 136), (K_, H_), None, 0)],
}
LEAD, GUARD = 4, 64
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS = (float(np.float32(v)) for v in (1e-3, 0.9, 0.999, 1e-8))
ADAM_GS = 2.0
ADAM_STEPS = (1, 2, 10000)
# grid caps of seg_adam_tf1_pack (option adam_blocks) from the plan's tile count
ADAM_BLOCKS = {"per-tile": lambda n: 0, "1": lambda n: 1, "3": lambda n: 3, "tiles-1": lambda n: n - 1,
               "above": lambda n: n + 1000}


def _numel(shape):
    return int(np.prod(shape))


def _rs_a_b(shape):
    return (shape[0] * shape[1], shape[2], shape[3]) if len(shape) == 4 else (1, 1, shape[0])


@functools.lru_cache(maxsize=None)
def _layout(which):
    """Offsets of the plan's variables in the flat buffers (each at its
    residue mod 4, at least one gap element before and after it), the buffer
    length and the mask of variable elements."""
    spec = ADAM_PLANS[which]
    offs, off = [], LEAD
    for shape, _, _, res in spec:
        while off % 4 != res:
            off += 1
        offs.append(off)
        off += _numel(shape) + 1
    total = off + GUARD
    var = torch.zeros(total, dtype=torch.bool)
    for (shape, *_), o in zip(spec, offs):
        var[o:o + _numel(shape)] = True
    assert sorted({o % 4 for o in offs}) == ([0, 1, 2, 3] if which == "multi" else [0])
    return offs, total, var


def _with_gap_sentinels(t, var, base):
    """Distinct non-zero values (exact in fp32) in every element outside the variables."""
    idx = torch.arange(t.numel())[~var]
    t[~var] = (base + idx).float()
    return t


def _make_plan(which, dtype, dev):
    """ops.AdamPlan of the named plan with fresh packed copies full of 7.0."""
    spec = ADAM_PLANS[which]
    offs, _, _ = _layout(which)
    segs, copies, tiles = [], [], 0
    for (shape, modes, a_pad, _), o in zip(spec, offs):
        rows = tr = None
        rs, a, b = _rs_a_b(shape)
        ap = a_pad or ops.round8(a)
        for mode in modes:
            t = torch.full(ops.packed_shape(*shape, mode, ap), 7.0, dtype=dtype, device=dev)
            if mode in ROWS_MODES:
                rows = (t, ap, ops.round8(b))
            else:
                tr = (t, ap, ops.round8(b))
            copies.append((t, shape, o, mode, ap))
        segs.append((o, rs, a, b, rows, tr))
        tiles += rs * ((a + 31) // 32) * ((b + 127) // 128)
    plan = ops.AdamPlan(segs, dev)
    assert plan.total_tiles == tiles and plan.nsegs == len(spec)
    return plan, copies


def _check_copies(P, copies, dtype, what):
    """Every packed copy == the host reference of P's variable; padding still 7.0."""
    Pc = P.cpu()
    bad = []
    for t, shape, o, mode, ap in copies:
        src = Pc[o:o + _numel(shape)].view(shape)
        try:
            assert_bits_equal(t, packed_ref(src, mode, dtype, ap, ops.round8(shape[3]), fill=7.0),
                              f"copy mode {mode} of {shape} at offset {o}")
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, f"{what}: {len(bad)} of {len(copies)} copies differ:\n" + "\n".join(bad)


@functools.lru_cache(maxsize=None)
def _adam_problem(which):
    """Inputs (mid-trajectory m / v, one gradient per step, each variable's
    gradients on a scale of its own) and the float64 AdamTF1 states after the
    last step."""
    spec = ADAM_PLANS[which]
    offs, total, var = _layout(which)
    g = _gen(4100 + len(spec))
    scale = torch.ones(total)
    for i, ((shape, *_), o) in enumerate(zip(spec, offs)):
        scale[o:o + _numel(shape)] = (1e-3, 1e-1, 1e1, 1e-2, 1.0)[i % 5]
    P0 = torch.randn(total, generator=g)
    grads = [torch.randn(total, generator=g) * scale for _ in ADAM_STEPS]
    M0 = (ADAM_GS * grads[0] * (torch.rand(total, generator=g) - 0.5)).float()
    V0 = ((ADAM_GS * grads[0]) ** 2 * 0.5 * torch.rand(total, generator=g)).float()
    # a band on the float4 path (inside the 72 x 136 filter) and one on the scalar path
    # with g = 0 in every step and m = v = 0: those elements must not move
    zero = torch.zeros(total, dtype=torch.bool)
    zi = 1 if which == "multi" else 0
    zero[offs[zi] + 1000:offs[zi] + 1300] = True
    if which == "multi":
        zero[offs[13] + 200:offs[13] + 250] = True
    assert (zero & ~var).sum() == 0
    for t in grads + [M0, V0]:
        t[zero] = 0.0
    for k, t in enumerate([P0, M0, V0] + grads):
        _with_gap_sentinels(t, var, 1000.0 * (k + 1))
    opt = tf_ref.AdamTF1(lr=ADAM_LR, beta1=ADAM_B1, beta2=ADAM_B2, eps=ADAM_EPS)
    opt.m, opt.v = {"p": M0.double()}, {"p": V0.double()}
    params = {"p": P0.double()}
    for t, gr in zip(ADAM_STEPS, grads):
        opt.t = t - 1
        params = opt.apply(params, {"p": gr.double() * ADAM_GS})
    return SimpleNamespace(spec=spec, offs=offs, total=total, var=var, zero=zero, P0=P0, M0=M0, V0=V0, grads=grads,
                           ref=(params["p"], opt.m["p"], opt.v["p"]))


def _adam_bounds(got, ref, grads, sel, what):
    (p, m, v), (pr, mr, vr) = got, ref
    assert_close(p[sel].double(), pr[sel], torch.float32, f"{what}: p", 1e-6)
    gmax = max(gr[sel].abs().max().item() for gr in grads) * ADAM_GS
    em = (m[sel].double() - mr[sel]).abs().max().item()
    assert em <= 1e-6 * gmax, f"{what}: m off by {em:.3e} > 1e-6 * {gmax:.3e}"
    assert_close(v[sel].double(), vr[sel], torch.float32, f"{what}: v", 1e-6)


@pytest.mark.parametrize("blocks", list(ADAM_BLOCKS))
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("which", list(ADAM_PLANS))
def test_adam_tf1_pack_against_float64(dev, knob, which, dtype, blocks):
    pb = _adam_problem(which)
    plan, copies = _make_plan(which, dtype, dev)
    cap = ADAM_BLOCKS[blocks](plan.total_tiles)
    knob("adam_blocks", cap)
    P, M, V = pb.P0.to(dev), pb.M0.to(dev), pb.V0.to(dev)
    for t, gr in zip(ADAM_STEPS, pb.grads):
        G = gr.to(dev)
        ops.adam_tf1_pack(P, G, M, V, plan, ADAM_LR, t, beta1=ADAM_B1, beta2=ADAM_B2, eps=ADAM_EPS,
                          grad_scale=ADAM_GS, dtype=DT[dtype])
        torch.cuda.synchronize()
        assert_bits_equal(G, gr, f"t = {t}: the gradient buffer")
        _check_copies(P, copies, dtype, f"t = {t}, grid cap {cap}")
    got = (P.cpu(), M.cpu(), V.cpu())
    # gaps between the variables, the lead and the guard band: bit-unchanged
    for t, t0, nm in zip(got, (pb.P0, pb.M0, pb.V0), "PMV"):
        assert_bits_equal(t[~pb.var], t0[~pb.var], f"{nm} outside the variables")
    # g = 0 with m = v = 0: p - lr_t * 0 / (sqrt(0) + eps) = p, bit for bit
    assert_bits_equal(got[0][pb.zero], pb.P0[pb.zero], "p of the zero-gradient band")
    for t, nm in zip(got[1:], "mv"):
        assert_bits_equal(t[pb.zero], torch.zeros(int(pb.zero.sum())), f"{nm} of the zero-gradient band")
    _adam_bounds(got, pb.ref, pb.grads, pb.var, "whole buffer")
    for (shape, *_), o in zip(pb.spec, pb.offs):
        sel = torch.zeros(pb.total, dtype=torch.bool)
        sel[o:o + _numel(shape)] = True
        _adam_bounds(got, pb.ref, pb.grads, sel, f"{shape} at offset {o}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("which", list(ADAM_PLANS))
def test_pack_segments_rewrites_every_copy_from_p(dev, which, dtype):
    """The repack after a ZeRO-1 all-gather: no update, copies from P alone."""
    _, total, var = _layout(which)
    plan, copies = _make_plan(which, dtype, dev)
    P0 = _with_gap_sentinels(torch.randn(total, generator=_gen(4200)), var, 500.0)
    P0[var] *= torch.where(torch.arange(total) % 3 == 0, 200.0, 1.0)[var]
    P = P0.to(dev)
    ops.pack_segments(P, plan, dtype=DT[dtype])
    torch.cuda.synchronize()
    _check_copies(P0, copies, dtype, "pack_segments")
    assert_bits_equal(P, P0, "P after pack_segments")


# ---------------------------------------------------------------------------
# 4. fused filter gradient + Adam in the forms backward.py launches
# ---------------------------------------------------------------------------
from tests.test_gpu_ops import ADAM_FUSED_CASES  # noqa: E402

FUSED_CASES = [c for c in ADAM_FUSED_CASES
               if c in [(1, 5, 7, 40, 264, 7), (1, 5, 7, 36, 264, 7), (2, 6, 9, 512, 512, 1)]]
FUSED_LR, FUSED_GS = 1e-3, 0.5


def _fused_run(d, xd, dyd, p0, m0, v0, t, ws, rows=True, tr=True, dw=False, dbias=False):
    """One seg_conv2d_bwd_filter_adam launch on fresh copies of p0 / m0 / v0; the
    copies that are not passed exist all the same and must keep their 7.0."""
    dev = xd.device
    R, _, C, K = p0.shape
    cp, kp = ops.round8(C), ops.round8(K)
    o = SimpleNamespace(p=p0.to(dev), m=m0.to(dev), v=v0.to(dev))
    o.rows = torch.full(ops.packed_shape(R, R, C, K, ops.PACK_HWIO), 7.0, dtype=torch.bfloat16, device=dev)
    o.tr = torch.full(ops.packed_shape(R, R, C, K, ops.PACK_KRSC), 7.0, dtype=torch.bfloat16, device=dev)
    o.dw = torch.full((R, R, C, K), float("nan"), device=dev) if dw else None
    o.db = torch.full((K,), float("nan"), device=dev) if dbias else None
    ops.conv2d_bwd_filter_adam(d, xd, dyd, o.p, o.m, o.v, FUSED_LR, t, grad_scale=FUSED_GS,
                               rows=(o.rows, cp, kp) if rows else None, tr=(o.tr, cp, kp) if tr else None,
                               dw=o.dw, dbias=o.db, ws=ws)
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("case", FUSED_CASES, ids=lambda c: "x".join(map(str, c)))
def test_fused_wgrad_adam_production_forms(dev, knob, case):
    """backward.py passes dw = None, and for conv6 / conv7 the HWIO copy only:
    the same kernel (no split-K, no atomics) must give the bits of the
    all-outputs call whichever outputs it is given."""
    N, H, W, C, K, R = case
    assert len(FUSED_CASES) == 3
    d = ops.conv_desc(N, H, W, C, K, R, R, dtype=ops.BF16)
    assert ops.wgrad_adam_fusable(d)
    g = _gen(21)
    x = torch.randn(N, H, W, C, generator=g, dtype=torch.float64)
    dy = torch.randn(N, H, W, K, generator=g, dtype=torch.float64)
    p0 = torch.randn(R, R, C, K, generator=g) * 0.05
    m0 = torch.randn(R, R, C, K, generator=g) * 1e-3
    v0 = torch.rand(R, R, C, K, generator=g) * 1e-5
    xd, dyd = to_dev(x, torch.bfloat16, dev), to_dev(dy, torch.bfloat16, dev)
    ws = ops.Workspace(dev)
    ws.get(max(ops.conv_workspace(d, ops.OP_BWD_FILTER), int(_lib.lib().seg_bias_grad_workspace(N * H * W, d.K)),
               4 * 1024 * 2 * d.K))
    cp, kp = ops.round8(C), ops.round8(K)
    t = 3
    knob("adam_tr_fused", 0)
    base = _fused_run(d, xd, dyd, p0, m0, v0, t, ws, dw=True)
    assert not torch.isnan(base.dw).any()
    assert_bits_equal(base.rows, packed_ref(base.p, ops.PACK_HWIO, torch.bfloat16, cp, kp, fill=7.0), "baseline HWIO")
    assert_bits_equal(base.tr, packed_ref(base.p, ops.PACK_KRSC, torch.bfloat16, cp, kp, fill=7.0), "baseline KRSC")
    assert not torch.equal(base.p.cpu(), p0)

    def same(o, what, rows, tr):
        for nm in "pmv":
            assert_bits_equal(getattr(o, nm), getattr(base, nm), f"{what}: {nm}")
        assert_bits_equal(o.rows, base.rows if rows else torch.full_like(base.rows, 7.0), f"{what}: HWIO copy")
        assert_bits_equal(o.tr, base.tr if tr else torch.full_like(base.tr, 7.0), f"{what}: KRSC copy")

    same(_fused_run(d, xd, dyd, p0, m0, v0, t, ws), "dw = None", True, True)
    same(_fused_run(d, xd, dyd, p0, m0, v0, t, ws, tr=False), "HWIO copy only", True, False)
    same(_fused_run(d, xd, dyd, p0, m0, v0, t, ws, rows=False, tr=False), "no copy", False, False)
    for trf in (0, 1):
        knob("adam_tr_fused", trf)
        same(_fused_run(d, xd, dyd, p0, m0, v0, t, ws, rows=False), f"KRSC copy only, adam_tr_fused {trf}", False, True)
    same(_fused_run(d, xd, dyd, p0, m0, v0, t, ws), "both copies, adam_tr_fused 1", True, True)
    knob("adam_tr_fused", 0)
    o = _fused_run(d, xd, dyd, p0, m0, v0, t, ws, dbias=True)
    same(o, "with dbias", True, True)
    assert_close(o.db.double().cpu(), rnd(dy, torch.bfloat16).sum(dim=(0, 1, 2)), torch.bfloat16, "dbias", 2e-5)
    # the first step of a run: t = 1 from m = v = 0, against float64 on the plain path's gradient
    gref = torch.empty(R, R, C, K, device=dev)
    ops.conv2d_bwd_filter(d, xd, dyd, gref)
    z = torch.zeros_like(p0)
    o = _fused_run(d, xd, dyd, p0, z, z, 1, ws)
    gc = gref.cpu().double() * FUSED_GS
    me, ve = 0.1 * gc, 0.001 * gc * gc
    pe = p0.double() - FUSED_LR * math.sqrt(1 - 0.999) / (1 - 0.9) * me / (ve.sqrt() + 1e-8)
    for got, ref, nm, tol in ((o.p, pe, "p", 1e-5), (o.m, me, "m", 1e-5), (o.v, ve, "v", 1e-4)):
        err = (got.cpu().double() - ref).abs().max().item() / ref.abs().max().item()
        assert err < tol, ("t = 1", nm, err)
    assert_bits_equal(o.rows, packed_ref(o.p, ops.PACK_HWIO, torch.bfloat16, cp, kp, fill=7.0), "t = 1: HWIO")
    assert_bits_equal(o.tr, packed_ref(o.p, ops.PACK_KRSC, torch.bfloat16, cp, kp, fill=7.0), "t = 1: KRSC")


# ---------------------------------------------------------------------------
# 5. BnFinishBatch on synthetic partial rows
# ---------------------------------------------------------------------------
# bn_fold_batch_k folds more than 128 rows into 128 groups first, 256 columns of
# the 2 C per block; bn_finish_batch_k sums 32 row groups for 8 channels a block
BN_NROWS = [1, 31, 32, 33, 128, 129, 257, 1000]
BN_C = [8, 16, 136, 520]
BN_EPS = [1e-3, 1e-5, 0.1]
BN_GUARD, BN_SENTINEL = 8, -77.0


def _bn_spec():
    """Every (nrows, C, cv, eps); two unfolded segments, then a folded one, ...,
    folded ones next to each other, an unfolded one last."""
    combos = [(n, C, cv, BN_EPS[(i + j) % 3]) for i, C in enumerate(BN_C) for j, cv in enumerate((C, C - 3, 1))
              for n in BN_NROWS]
    plain = [c for c in combos if c[0] <= 128]
    fold = [c for c in combos if c[0] > 128]
    last, out = plain.pop(), []
    while plain or fold:
        out += plain[:2] + fold[:1]
        plain, fold = plain[2:], fold[1:]
    return out + [last]


BN_SPEC = _bn_spec()


@functools.lru_cache(maxsize=None)
def _bn_parts(form):
    g = _gen(5100)
    if form == "exact":      # integers in [-8, 8]: every partial sum is an integer below 2^24, exact in any order
        return [torch.randint(-8, 9, (n, 2 * C), generator=g).float() for n, C, _, _ in BN_SPEC]
    return [torch.randn(n, 2 * C, generator=g) for n, C, _, _ in BN_SPEC]


def _bn_inv(eps):
    return np.float32(1.0) / np.sqrt(np.float32(1.0) + np.float32(eps))


def _bn_check(form, part, spec, dg, db, what):
    n, C, cv, eps = spec
    dg, db = dg.cpu(), db.cpu()
    sent = torch.full((BN_GUARD,), BN_SENTINEL)
    for t, nm in ((dg, "dgamma"), (db, "dbeta")):
        assert_bits_equal(t[:BN_GUARD], sent, f"{what}: guard before {nm}")
        assert_bits_equal(t[BN_GUARD + cv:], torch.full((C - cv + BN_GUARD,), BN_SENTINEL),
                          f"{what}: {nm}[cv:] and the guard after it")
    got_g, got_b = dg[BN_GUARD:BN_GUARD + cv], db[BN_GUARD:BN_GUARD + cv]
    s = part.double().sum(0)
    inv = _bn_inv(eps)
    if form == "exact":
        assert part.abs().sum(0).max().item() < 2 ** 24
        assert_bits_equal(got_b, s[C:C + cv].float(), f"{what}: dbeta")
        assert_bits_equal(got_g, torch.from_numpy(s[:cv].numpy().astype(np.float32) * inv), f"{what}: dgamma")
    else:                    # recursive-summation bound, any order: (n - 1) roundings, one more for * inv
        bound = (n + 1) * 2.0 ** -24 * part.double().abs().sum(0)
        eb = (got_b.double() - s[C:C + cv]).abs()
        assert (eb <= bound[C:C + cv]).all(), f"{what}: dbeta off by {eb.max().item():.3e}"
        eg = (got_g.double() - s[:cv] * float(inv)).abs()
        assert (eg <= bound[:cv] * float(inv)).all(), f"{what}: dgamma off by {eg.max().item():.3e}"


def _bn_out(C, dev):
    return torch.full((C + 2 * BN_GUARD,), BN_SENTINEL, device=dev)


@pytest.mark.parametrize("form", ["exact", "float"])
def test_bn_finish_batch_on_synthetic_rows(dev, form):
    parts = _bn_parts(form)
    dparts = [p.to(dev) for p in parts]
    assert any(a[0] > 128 >= b[0] for a, b in zip(BN_SPEC, BN_SPEC[1:])) and BN_SPEC[0][0] <= 128
    bad = []

    def run(idx, what):
        outs = [(_bn_out(BN_SPEC[i][1], dev), _bn_out(BN_SPEC[i][1], dev)) for i in idx]
        segs = [(dparts[i], BN_SPEC[i][0], BN_SPEC[i][1], BN_SPEC[i][2], BN_SPEC[i][3],
                 dg[BN_GUARD:BN_GUARD + BN_SPEC[i][1]], db[BN_GUARD:BN_GUARD + BN_SPEC[i][1]])
                for i, (dg, db) in zip(idx, outs)]
        batch = ops.BnFinishBatch(segs, dev)
        assert (batch.a_blocks > 0) == any(BN_SPEC[i][0] > 128 for i in idx)
        batch.run()
        torch.cuda.synchronize()
        for i, (dg, db) in zip(idx, outs):
            try:
                _bn_check(form, parts[i], BN_SPEC[i], dg, db, f"segment {i} {BN_SPEC[i]}")
                assert_bits_equal(dparts[i], parts[i], f"partial rows of segment {i}")
            except AssertionError as e:
                bad.append(f"{what}: {e}")

    run(list(range(len(BN_SPEC))), "one batch")
    for i in range(len(BN_SPEC)):
        run([i], "alone")
    assert not bad, f"{len(bad)} segment results of {2 * len(BN_SPEC)} are wrong:\n" + "\n".join(bad)


# ---------------------------------------------------------------------------
# 6. deferred against immediate BatchNorm backward on real launches
# ---------------------------------------------------------------------------
from tests.test_gpu_ops_r2 import BNB3_CASES, BNB_CASES, PRO_DT, _pro_case  # noqa: E402


def _macs(c):
    return c[0] * c[1] * c[2] * c[3] * c[4]


BN_PART_1X1 = sorted(BNB_CASES, key=_macs)[:3]
BN_PART_3X3 = min(BNB3_CASES, key=_macs)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_bn_part_then_batch_finish_equals_the_immediate_finish(dev, dtype):
    """segkern.h: seg_bn_grad_finish_batch is "bit-identical to
    seg_conv2d_bwd_data_bn's own finish" -- dx, dgamma and dbeta of
    conv2d_bwd_data_bn against conv2d_bwd_data_bn_part + one BnFinishBatch over
    all the launches."""
    assert BN_PART_1X1 == [(1, 17, 19, 24, 8, 1), (2, 9, 11, 48, 64, 1), (1, 12, 10, 136, 64, 1)]
    assert BN_PART_3X3 == (2, 9, 11, 32, 16)
    launches = [(c, acc, None) for c in BN_PART_1X1 for acc in (False, True)]
    launches += [(BN_PART_3X3 + (3,), False, kp) for kp in (None, 0.6)]
    now, later, segs = [], [], []
    for case, acc, kp in launches:
        N, H, W, C, K, R = case
        x, w, gamma, beta, xr, wr, a = _pro_case(case, dtype, dev)
        g = _gen(9)
        dy = to_dev(rnd(torch.randn(N, H, W, K, generator=g, dtype=torch.float64), dtype), dtype, dev)
        d = ops.conv_desc(N, H, W, C, K, R, R, 1, 1, "SAME", PRO_DT[dtype])
        assert ops.conv_bwd_data_bn_workspace(d) > 0 and d.C == C
        wh = torch.zeros(ops.packed_shape(R, R, C, K, ops.PACK_HWIO), dtype=dtype, device=dev)
        ops.pack_filter(w.float().to(dev).contiguous(), wh, ops.round8(C), ops.round8(K), ops.PACK_HWIO)
        xd, gd, bd = to_dev(x, dtype, dev), gamma.to(dev), beta.to(dev)
        drop = (kp, 12345) if kp is not None else None
        if R == 1:    # the input gradient lands in a channel slice of a wider (concat gradient) buffer
            old = rnd(torch.randn(N, H, W, C + 16, generator=g, dtype=torch.float64), dtype)
            wide = to_dev(old, dtype, dev) if acc else torch.full((N, H, W, C + 16), float("nan"), dtype=dtype,
                                                                   device=dev)
        else:
            wide = torch.full((N, H, W, C), float("nan"), dtype=dtype, device=dev)
        res = []
        for deferred in (False, True):
            buf = wide.clone()
            dx = buf[..., 8:8 + C] if R == 1 else buf
            dg, db = torch.full((C,), float("nan"), device=dev), torch.full((C,), float("nan"), device=dev)
            if not deferred:
                ops.conv2d_bwd_data_bn(d, dy, wh, xd, gd, bd, dx, dg, db, accumulate=acc, dropout=drop)
            else:
                rows = ops.conv_bwd_data_bn_part_rows(d)
                kernel = ops.conv_kernel_info(d, ops.OP_BWD_DATA_BN)[0]
                print(f"bn part rows: {case} {'accumulate' if acc else 'write'} dropout {kp}: {rows} ({kernel})")
                assert rows > 0
                part = torch.full((rows * 2 * d.C,), float("nan"), device=dev)
                ops.conv2d_bwd_data_bn_part(d, dy, wh, xd, gd, bd, dx, part, accumulate=acc, dropout=drop)
                segs.append((part, rows, d.C, d.c_valid, 1e-3, dg, db))
            res.append((buf, dg, db))
        now.append(res[0])
        later.append(res[1])
    ops.BnFinishBatch(segs, dev).run()
    torch.cuda.synchronize()
    for (case, acc, kp), a_, b_ in zip(launches, now, later):
        for ta, tb, nm in zip(a_, b_, ("dx", "dgamma", "dbeta")):
            assert not torch.isnan(ta[..., 8:8 + case[3]] if nm == "dx" and case[5] == 1 else ta).any(), (case, nm)
            assert_bits_equal(tb, ta, f"{case} accumulate {acc} dropout {kp}: {nm}")


# ---------------------------------------------------------------------------
# 7. packed copies after real steps, and after a restore
# ---------------------------------------------------------------------------
def _assert_copies_coherent(sess, what):
    """Every packed copy of the store == the host reference of its master,
    padding entries zero.  Returns the masters that have copies, by name."""
    assert sess.store.packed
    torch.cuda.synchronize()
    masters = {}
    for (name, mode), (t, ap, bp) in sess.store.packed.items():
        if name not in masters:
            masters[name] = sess.variable_value(name)
        assert_bits_equal(t, packed_ref(torch.from_numpy(masters[name]), mode, t.dtype, ap, bp),
                          f"{what}: {name} mode {mode}")
    return masters


@pytest.fixture(scope="module")
def fcn_weights():
    """The FCN's 138.9 M He-scaled parameters, drawn once for the module."""
    from oracle import models as M
    from tests.model_inputs import he_weights
    return he_weights(M.fcn_param_shapes(3, 2), 61)


COHERENCE = ["fcn-bf16", "fcn-f32", "fcdensenet-bf16", "fcn-bf16-var_list"]
FROZEN = ("conv3_2/weights", "conv3_2/biases")


@pytest.mark.parametrize("case", COHERENCE)
def test_packed_copies_follow_their_masters(dev, tmp_path, request, case):
    from oracle import models as M
    from semanticsegmentation_tensorflow_amd import tf
    from tests.model_inputs import densenet_weights, synthetic_batch
    model, dtype = case.split("-")[:2]
    N, H, W = 1, 64, 96
    if model == "fcn":
        from tests.test_gpu_fcn import build_fcn
        image, labels, keep, pred, logits, loss, train_step = build_fcn(H, W)
        weights = request.getfixturevalue("fcn_weights")
        kp = 1.0
    else:
        from tests.test_gpu_fcdensenet import build
        image, labels, keep, pred, logits, loss, train_step = build(H, W)
        weights = densenet_weights(M.fcdensenet_param_shapes(3, 2), 62)
        kp = 0.8
    frozen = FROZEN if case.endswith("var_list") else ()
    if frozen:
        var_list = [v for v in tf.trainable_variables() if v.var_name not in frozen]
        train_step = tf.train.AdamOptimizer(1e-4).minimize(loss, var_list=var_list)
    img, lab = synthetic_batch(N, H, W, 63)
    feed = {image: img, labels: lab, keep: kp}
    sess = tf.Session(compute_dtype=dtype, seed=5)
    sess.run(tf.global_variables_initializer())
    for k, v in weights.items():
        sess.assign(k, v)
    saver = tf.train.Saver()
    path = saver.save(sess, str(tmp_path / "before.ckpt"))
    for _ in range(3):
        sess.run(train_step, feed_dict=feed)
    masters = _assert_copies_coherent(sess, "after 3 steps")
    modes = {mode for _, mode in sess.store.packed}
    assert modes == {0, 1, 2, 3}, modes                   # conv and tconv copies, both layouts
    assert {k for k, v in weights.items() if v.ndim == 4} == set(masters)
    for k in set(masters) - set(frozen):                  # the copies are those of updated filters
        assert not np.array_equal(masters[k], weights[k]), k
    for k in frozen:                                      # bit-equal to its initial value (its copies: above)
        assert np.array_equal(sess.variable_value(k), weights[k]), k
    # back to the checkpoint: the copies hold the stepped values until the next run repacks them
    saver.restore(sess, path)
    sess.run(loss, feed_dict=feed)
    masters = _assert_copies_coherent(sess, "after restore")
    for k in weights:
        got = masters[k] if k in masters else sess.variable_value(k)
        assert np.array_equal(got, weights[k]), k
