"""float64 CPU restatement, in plain loops, of TF's general pooling and of
tf.pad on H and W (Network/utils/utils.py:306-310, :325-327; PSPNet50's 3x3
stride-2 max pool and its pyramid's average pools, Network/model/PSPNet.py:34,
:147-166) -- the reference of seg_pool2d_* and seg_pad2d_*:

* max pool over the in-image elements of each window, with the switch (the
  row-major window position r * kw + s of the FIRST maximum: strict '>');
* average pool dividing by the number of in-image elements (TF under SAME);
* both gradients (a window's dy goes to the switch's pixel / dy over count to
  every in-image pixel of the window; uncovered pixels get 0);
* pad and crop.

NHWC torch tensors in and out.  Pinned on the CPU by tests/test_pool_ref.py."""
import torch


def geometry(in_size, k, s, padding):
    """(out, pad_before, pad_after) along one axis, TF's rule."""
    if padding == "SAME":
        out = -(-in_size // s)
        total = max((out - 1) * s + k - in_size, 0)
        return out, total // 2, total - total // 2
    if padding == "VALID":
        return (in_size - k) // s + 1, 0, 0
    raise ValueError(padding)


def _windows(H, W, ksize, strides, padding):
    (kh, kw), (sh, sw) = ksize, strides
    OH, pt, _ = geometry(H, kh, sh, padding)
    OW, pl, _ = geometry(W, kw, sw, padding)
    for oh in range(OH):
        for ow in range(OW):
            cells = []                                   # (window position, ih, iw) of the in-image elements
            for r in range(kh):
                for s in range(kw):
                    ih, iw = oh * sh - pt + r, ow * sw - pl + s
                    if 0 <= ih < H and 0 <= iw < W:
                        cells.append((r * kw + s, ih, iw))
            yield oh, ow, cells


def out_shape(x_shape, ksize, strides, padding):
    N, H, W, C = x_shape
    return N, geometry(H, ksize[0], strides[0], padding)[0], geometry(W, ksize[1], strides[1], padding)[0], C


def max_pool(x, ksize, strides, padding):
    """-> (y float64 [N,OH,OW,C], idx int64 [N,OH,OW,C])."""
    x = x.double()
    N, H, W, C = x.shape
    y = torch.zeros(out_shape(x.shape, ksize, strides, padding), dtype=torch.float64)
    idx = torch.zeros(y.shape, dtype=torch.int64)
    for oh, ow, cells in _windows(H, W, ksize, strides, padding):
        pos0, ih0, iw0 = cells[0]
        best = x[:, ih0, iw0, :].clone()
        arg = torch.full_like(best, pos0, dtype=torch.int64)
        for pos, ih, iw in cells[1:]:
            v = x[:, ih, iw, :]
            upd = v > best
            best = torch.where(upd, v, best)
            arg = torch.where(upd, torch.full_like(arg, pos), arg)
        y[:, oh, ow, :] = best
        idx[:, oh, ow, :] = arg
    return y, idx


def max_pool_grad(idx, dy, x_shape, ksize, strides, padding):
    N, H, W, C = x_shape
    dy = dy.double()
    dx = torch.zeros(x_shape, dtype=torch.float64)
    for oh, ow, cells in _windows(H, W, ksize, strides, padding):
        for pos, ih, iw in cells:
            dx[:, ih, iw, :] += torch.where(idx[:, oh, ow, :] == pos, dy[:, oh, ow, :], torch.zeros(()).double())
    return dx


def avg_pool(x, ksize, strides, padding):
    x = x.double()
    N, H, W, C = x.shape
    y = torch.zeros(out_shape(x.shape, ksize, strides, padding), dtype=torch.float64)
    for oh, ow, cells in _windows(H, W, ksize, strides, padding):
        acc = torch.zeros(N, C, dtype=torch.float64)
        for _, ih, iw in cells:
            acc = acc + x[:, ih, iw, :]
        y[:, oh, ow, :] = acc / len(cells)
    return y


def avg_pool_grad(dy, x_shape, ksize, strides, padding):
    N, H, W, C = x_shape
    dy = dy.double()
    dx = torch.zeros(x_shape, dtype=torch.float64)
    for oh, ow, cells in _windows(H, W, ksize, strides, padding):
        for _, ih, iw in cells:
            dx[:, ih, iw, :] += dy[:, oh, ow, :] / len(cells)
    return dx


def overlap(x_shape, ksize, strides, padding):
    """bool [H, W]: pixels that more than one window contains."""
    _, H, W, _ = x_shape
    cnt = torch.zeros(H, W, dtype=torch.int64)
    for _, _, cells in _windows(H, W, ksize, strides, padding):
        for _, ih, iw in cells:
            cnt[ih, iw] += 1
    return cnt > 1


def pad(x, pads):
    """pads = (top, bottom, left, right) zero rows / columns."""
    t, b, l, r = pads
    N, H, W, C = x.shape
    y = torch.zeros(N, H + t + b, W + l + r, C, dtype=x.dtype)
    for h in range(H):
        for w in range(W):
            y[:, h + t, w + l, :] = x[:, h, w, :]
    return y


def crop(dy, pads):
    """Gradient of pad: dy's interior."""
    t, b, l, r = pads
    N, PH, PW, C = dy.shape
    return dy[:, t:PH - b, l:PW - r, :].clone()


# ---------------------------------------------------------------------------
# the same functions under torch.autograd (the gradients above, not torch's)
# ---------------------------------------------------------------------------
class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ksize, strides, padding):
        y, idx = max_pool(x.detach(), ksize, strides, padding)
        ctx.args = (idx, tuple(x.shape), ksize, strides, padding)
        return y

    @staticmethod
    def backward(ctx, dy):
        idx, shape, ksize, strides, padding = ctx.args
        return max_pool_grad(idx, dy, shape, ksize, strides, padding), None, None, None


class _AvgPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ksize, strides, padding):
        ctx.args = (tuple(x.shape), ksize, strides, padding)
        return avg_pool(x.detach(), ksize, strides, padding)

    @staticmethod
    def backward(ctx, dy):
        return avg_pool_grad(dy, *ctx.args), None, None, None


class _Pad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pads):
        ctx.pads = pads
        return pad(x.detach(), pads)

    @staticmethod
    def backward(ctx, dy):
        return crop(dy, ctx.pads), None


def max_pool_ad(x, ksize, strides, padding):
    return _MaxPool.apply(x, tuple(ksize), tuple(strides), padding)


def avg_pool_ad(x, ksize, strides, padding):
    return _AvgPool.apply(x, tuple(ksize), tuple(strides), padding)


def pad_ad(x, pads):
    return _Pad.apply(x, tuple(pads))
