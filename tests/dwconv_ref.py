"""float64 CPU restatement, in plain loops, of tf.nn.depthwise_conv2d with
channel multiplier 1 (SepConv_BN, Network/model/EfficientNet.py:426-462) -- the
reference of seg_dwconv2d_fwd / _bwd_data / _bwd_filter:

* forward  y[n,oh,ow,c] = sum over the in-image taps of
  x[n, oh*s - pt + r*dh, ow*s - pl + q*dw, c] * w[r,q,c];
* the input gradient (every term of the forward sent back to its x);
* the filter gradient dw[r,q,c] = sum over n, oh, ow of x[..] * dy[n,oh,ow,c];
* TF's SAME / VALID geometry on the effective window (k - 1) * d + 1.

NHWC torch tensors, w [R, S, C].  Pinned on the CPU by tests/test_dwconv_ref.py."""
import torch

# (N, H, W, C, R, S, stride, (dh, dw), padding): the kernel cases of tests/test_gpu_dwconv.py
CASES = [(2, 7, 9, 16, 3, 3, 1, (1, 1), "SAME"),
         (1, 8, 8, 8, 3, 3, 2, (1, 1), "SAME"),          # asymmetric pad 0 / 1
         (2, 9, 11, 8, 3, 3, 2, (1, 1), "VALID"),        # the last windows end flush with the image
         (1, 6, 10, 24, 3, 3, 1, (6, 6), "SAME"),        # pad >= image height: part of the taps never in-image
         (1, 5, 7, 8, 3, 3, 1, (2, 3), "SAME"),          # per-axis rate
         (1, 7, 7, 8, 3, 3, 1, (2, 2), "VALID"),         # dilated VALID
         (1, 9, 9, 8, 5, 5, 2, (1, 1), "SAME"),
         (1, 9, 12, 8, 5, 5, 1, (1, 1), "SAME"),
         (1, 10, 9, 8, 3, 3, 3, (1, 1), "SAME"),         # stride 3: dx divisibility
         (1, 6, 6, 8, 2, 2, 2, (1, 1), "SAME"),          # even filter
         (2, 4, 5, 40, 1, 1, 1, (1, 1), "SAME"),         # five chunks, 1x1
         (1, 3, 70, 8, 3, 3, 1, (1, 1), "SAME"),         # a row longer than one strip and one block's worth
         (1, 10, 12, 8, 3, 3, 2, (1, 1), "VALID"),       # leftover row and column: dx has zeros there
         (2, 33, 65, 16, 3, 3, 1, (1, 1), "SAME")]       # more than one partial row of the filter gradient


def geometry(in_size, k, s, d, padding):
    """(out, pad_before, pad_after) along one axis, TF's rule on the effective window."""
    k_eff = (k - 1) * d + 1
    if padding == "SAME":
        out = -(-in_size // s)
        total = max((out - 1) * s + k_eff - in_size, 0)
        return out, total // 2, total - total // 2
    if padding == "VALID":
        return (in_size - k_eff) // s + 1, 0, 0
    raise ValueError(padding)


def _terms(H, W, R, S, stride, rate, padding):
    """(oh, ow, r, q, ih, iw) of every in-image term."""
    dh, dw = rate
    OH, pt, _ = geometry(H, R, stride, dh, padding)
    OW, pl, _ = geometry(W, S, stride, dw, padding)
    for oh in range(OH):
        for ow in range(OW):
            for r in range(R):
                for q in range(S):
                    ih, iw = oh * stride - pt + r * dh, ow * stride - pl + q * dw
                    if 0 <= ih < H and 0 <= iw < W:
                        yield oh, ow, r, q, ih, iw


def out_shape(x_shape, R, S, stride, rate, padding):
    N, H, W, C = x_shape
    return N, geometry(H, R, stride, rate[0], padding)[0], geometry(W, S, stride, rate[1], padding)[0], C


def forward(x, w, stride, rate, padding):
    x, w = x.double(), w.double()
    N, H, W, C = x.shape
    R, S, _ = w.shape
    y = torch.zeros(out_shape(x.shape, R, S, stride, rate, padding), dtype=torch.float64)
    for oh, ow, r, q, ih, iw in _terms(H, W, R, S, stride, rate, padding):
        y[:, oh, ow, :] += x[:, ih, iw, :] * w[r, q, :]
    return y


def input_grad(dy, w, x_shape, stride, rate, padding):
    dy, w = dy.double(), w.double()
    N, H, W, C = x_shape
    R, S, _ = w.shape
    dx = torch.zeros(x_shape, dtype=torch.float64)
    for oh, ow, r, q, ih, iw in _terms(H, W, R, S, stride, rate, padding):
        dx[:, ih, iw, :] += dy[:, oh, ow, :] * w[r, q, :]
    return dx


def filter_grad(x, dy, R, S, stride, rate, padding):
    x, dy = x.double(), dy.double()
    N, H, W, C = x.shape
    dw = torch.zeros(R, S, C, dtype=torch.float64)
    for oh, ow, r, q, ih, iw in _terms(H, W, R, S, stride, rate, padding):
        dw[r, q, :] += (x[:, ih, iw, :] * dy[:, oh, ow, :]).sum(0)
    return dw


# ---------------------------------------------------------------------------
# the same function under torch.autograd (the gradients above, not torch's)
# ---------------------------------------------------------------------------
class _Depthwise(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, stride, rate, padding):
        ctx.save_for_backward(x.detach(), w.detach())
        ctx.args = (stride, rate, padding)
        return forward(x.detach(), w.detach(), stride, rate, padding)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        R, S, _ = w.shape
        return (input_grad(dy, w, tuple(x.shape), *ctx.args), filter_grad(x, dy, R, S, *ctx.args), None, None, None)


def depthwise_ad(x, w, stride=1, rate=(1, 1), padding="SAME"):
    """x NHWC, w [R, S, C] (or TF's [R, S, C, 1]) -> y; differentiable in both."""
    if w.dim() == 4:
        w = w[..., 0]
    rate = (rate, rate) if isinstance(rate, int) else tuple(rate)
    return _Depthwise.apply(x, w, int(stride), rate, padding)
