"""Forward pass of a Session step (mixin): staging of the fed values and one
launch method per node kind of the plan (`_fwd_<kind>`; backward.py holds the
matching `_bwd_<kind>`, planner.py decides a node's form at compile time).
Split out of session.py; `Session` inherits these methods."""
from __future__ import annotations

import numpy as np
import torch

from . import graph as G
from . import ops


def _np(x):
    if isinstance(x, torch.Tensor):
        return x
    return torch.from_numpy(np.ascontiguousarray(x))


class ForwardMixin:
    def _feed(self, p, feed_dict):
        feeds = {id(k): v for k, v in feed_dict.items()}
        # scalars (keep_probability) are read at launch time, not staged
        scal = {id(k): float(v) for k, v in feed_dict.items() if np.ndim(v) == 0}
        for tid, (kind, stage) in p.feed_slots.items():
            v = feeds[tid]
            if kind == "scalar":
                scal[tid] = float(v)
                continue
            src = _np(v)
            if kind == "image" and src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous() \
                    and src.shape == stage.shape:
                ops.prepare_input(src, p.buf[tid])   # augmented uint8 batch resident in HBM
                continue
            if src.is_cuda and src.dtype == stage.dtype and src.is_contiguous() and src.shape == stage.shape:
                src_dev = src                      # resident in HBM: no copy
            else:
                stage.copy_(src.to(stage.dtype) if src.dtype != stage.dtype else src, non_blocking=True)
                src_dev = stage
            if kind == "image":
                ops.prepare_input(src_dev, p.buf[tid])
            else:
                p.buf[tid] = src_dev
        return scal

    def _kp(self, kp, scal):
        if kp is None:
            return 1.0
        if isinstance(kp, G.Tensor):
            return scal[id(kp)]
        return float(kp)

    def _relu_fwd(self, x, y):
        C = x.shape[-1]
        one = torch.ones(C, dtype=torch.float32, device=self.device)
        zero = torch.zeros(C, dtype=torch.float32, device=self.device)
        ops.bn_relu_fwd(x, y, one, zero, C, True, eps=0.0)

    def _prologue(self, b):
        st = self.store
        return ops.prologue(st.param(b.gamma.var_name), st.param(b.beta.var_name), b.eps, b.relu)

    def _forward(self, p, scal, step_seed):
        """Every node of the plan in order, through its `_fwd_<kind>` method
        (p, node, output buffer, fed scalars, the node's dropout seed)."""
        for i, n in enumerate(p.nodes):
            if n.kind == "input":
                continue
            fwd = getattr(self, "_fwd_" + n.kind, None)
            if fwd is None:
                raise NotImplementedError(n.kind)
            fwd(p, n, p.buf[id(n.output)], scal, (step_seed + i * 131) & 0xFFFFFFFF)

    def _fwd_conv(self, p, n, y, scal, seed):
        buf, store = p.buf, self.store
        x = buf[id(n.inputs[0])]
        kp = self._kp(n.kp, scal)
        n.kp_val = kp
        n.seed_val = seed
        epi = ops.epilogue(bias=store.param(n.bias.var_name) if n.bias is not None else None,
                           relu=n.relu, keep_prob=kp, seed=n.seed_val)
        b = n.pro
        if id(n) in p.bn_out2:
            b2 = p.bn_out2[id(n)]
            self._timed(n.desc, ops.OP_FWD_PRO if b is not None else ops.OP_FWD, ops.conv2d_fwd_bn2, n.desc,
                        x if b is None else buf[id(b.inputs[0])], None if b is None else self._prologue(b),
                        self._pack(n, ops.PACK_KRSC), y, buf[id(b2.output)],
                        store.param(b2.gamma.var_name), store.param(b2.beta.var_name), b2.relu, b2.eps,
                        epi, self.ws)
        elif b is not None:
            self._timed(n.desc, ops.OP_FWD_PRO, ops.conv2d_fwd_pro, n.desc, buf[id(b.inputs[0])],
                        self._prologue(b), self._pack(n, ops.PACK_KRSC), y, epi, self.ws)
        elif id(n) in p.pool_fuse:
            m = p.pool_fuse[id(n)]
            self._timed(n.desc, ops.OP_FWD, ops.conv2d_fwd_pool, n.desc, x, self._pack(n, ops.PACK_KRSC),
                        buf[id(m.output)], p.pool_idx.get(id(m)), epi, self.ws)
        elif n.fwd_hwio:
            self._timed(n.desc, ops.OP_FWD, ops.conv2d_fwd_hwio, n.desc, x, self._pack(n, ops.PACK_HWIO), y,
                        epi, self.ws)
        elif id(n) in p.mask_bits:
            self._timed(n.desc, ops.OP_FWD, ops.conv2d_fwd_relu_bits, n.desc, x, self._pack(n, ops.PACK_KRSC), y,
                        p.mask_bits[id(n)], epi)
        else:
            self._timed(n.desc, ops.OP_FWD, ops.conv2d_fwd, n.desc, x, self._pack(n, ops.PACK_KRSC), y, epi,
                        self.ws)

    def _fwd_tconv(self, p, n, y, scal, seed):
        x = p.buf[id(n.inputs[0])]
        res = p.buf[id(n.residual)] if n.residual is not None else None
        epi = ops.epilogue(bias=self.store.param(n.bias.var_name) if n.bias is not None else None,
                           residual=res)
        self._timed(n.desc, ops.OP_TFWD, ops.tconv2d_fwd, n.desc, x, self._pack(n, ops.PACK_TCONV_FWD), y, epi,
                    self.ws)

    def _fwd_dwconv(self, p, n, y, scal, seed):
        # tf.nn.depthwise_conv2d: reads the fp32 master filter itself
        ops.dwconv2d_fwd(n.desc, p.buf[id(n.inputs[0])], self.store.param(n.w.var_name), y)

    def _fwd_MaxPool(self, p, n, y, scal, seed):
        idx = p.pool_idx.get(id(n))
        if id(n) in p.pool_fused:
            return                     # written by the producing conv's pooled epilogue
        if idx is not None:
            ops.maxpool2x2_fwd_argmax(p.buf[id(n.inputs[0])], y, idx)
        else:
            ops.maxpool2x2_fwd(p.buf[id(n.inputs[0])], y)

    def _fwd_AvgPool(self, p, n, y, scal, seed):
        ops.avgpool2x2_fwd(p.buf[id(n.inputs[0])], y)

    def _fwd_Pool2D(self, p, n, y, scal, seed):
        # any window / stride / padding; a max pool of a train plan records its switches
        ops.pool2d_fwd(n.desc, p.buf[id(n.inputs[0])], y, p.pool_idx.get(id(n)))

    def _fwd_Subsample(self, p, n, y, scal, seed):
        # every s-th pixel into the compact buffer a strided 1x1 conv reads (planner._lower_strided_1x1)
        ops.pool2d_fwd(n.desc, p.buf[id(n.inputs[0])], y)

    def _fwd_Pad(self, p, n, y, scal, seed):
        ops.pad2d_fwd(p.buf[id(n.inputs[0])], y, n.ops[0].attrs["pads"])

    def _fwd_Add(self, p, n, y, scal, seed):
        ops.add(p.buf[id(n.inputs[0])], p.buf[id(n.inputs[1])], y)

    def _fwd_bn(self, p, n, y, scal, seed):
        if id(n) in p.folded or id(n) in p.bn_out2_done:
            return                          # applied by its conv's operand prologue / written by its conv
        C = p.shapes[id(n.inputs[0])][3]
        if n.act is not None:               # BatchNorm + swish (MBConvBlock)
            ops.bn_act_fwd(p.buf[id(n.inputs[0])], y, self.store.param(n.gamma.var_name),
                           self.store.param(n.beta.var_name), C, n.act, n.eps)
            return
        ops.bn_relu_fwd(p.buf[id(n.inputs[0])], y, self.store.param(n.gamma.var_name),
                        self.store.param(n.beta.var_name), C, n.relu, n.eps)

    def _fwd_act(self, p, n, y, scal, seed):
        # a standalone swish / sigmoid (the squeeze-excite vectors): no affine
        ops.bn_act_fwd(p.buf[id(n.inputs[0])], y, None, None, p.shapes[id(n.inputs[0])][3], n.act)

    def _fwd_se_excite(self, p, n, y, scal, seed):
        x, s = n.inputs
        ops.se_excite_fwd(p.buf[id(x)], p.buf[id(s)], y, p.shapes[id(x)][3])

    def _fwd_Relu(self, p, n, y, scal, seed):
        self._relu_fwd(p.buf[id(n.inputs[0])], y)

    def _fwd_Dropout(self, p, n, y, scal, seed):
        kp = self._kp(n.ops[0].attrs["keep_prob"], scal)
        n.kp_val = kp
        n.seed_val = seed
        if kp < 1.0:
            ops.dropout_fwd(p.buf[id(n.inputs[0])], y, kp, n.seed_val)
        else:
            ops.copy_channels(p.buf[id(n.inputs[0])], y)

    def _fwd_xent(self, p, n, y, scal, seed):
        if n.twin is not None:
            return                          # forward-only, on another head's logits and labels: that launch's sum
        lg = p.buf[id(n.inputs[0])]
        labels = p.buf[id(n.labels)]
        # a head of Mean(sum_i w_i xent_i): dlogits carry loss_scale * w_i / count
        ops.softmax_xent(lg, labels, n.dlogits, n.loss_sum, n.num_classes, n.valid_hw,
                         grad_scale=(self.loss_scale if p.train else 1.0) * n.weight / n.count, ws=self.ws)

    def _fwd_xent_sum(self, p, n, y, scal, seed):
        if not n.wanted:
            return                          # the weighted loss is minimised, not fetched
        ops.fill(n.total, 0.0)
        for h in n.heads:
            ops.axpy(n.total, h.loss_sum, h.weight)

    def _fwd_film(self, p, n, y, scal, seed):
        # relu?((alpha + alpha_bias) * f + beta) in one launch (TransNet, FCDenseNet_TransNet.py:73-79)
        a, f, b = (p.buf[id(t)] for t in n.inputs)
        ops.film_fwd(a, f, b, y, p.shapes[id(n.output)][3], n.alpha_bias, n.relu)

    def _fwd_axpy(self, p, n, y, scal, seed):
        # relu?(x + lam * c) in one launch (FCDenseNet_TransNet.py:83-84)
        a, b = (p.buf[id(t)] for t in n.inputs)
        ops.axpy_relu_fwd(a, b, y, p.shapes[id(n.output)][3], n.lam, n.relu)

    def _fwd_ConcatV2(self, p, n, y, scal, seed):
        if id(n) not in p.alias_nodes:      # aliased: the parts already sit in place
            ops.concat_fwd([(p.buf[id(t)], p.shapes[id(t)][3]) for t in n.inputs], y,
                           p.shapes[id(n.output)][3])

    def _fwd_ArgMax(self, p, n, y, scal, seed):
        x = p.buf[id(n.inputs[0])]
        C = p.shapes[id(n.inputs[0])][3]
        ops.argmax(x, y.view(-1), C)

    def _fwd_Softmax(self, p, n, y, scal, seed):
        ops.softmax(p.buf[id(n.inputs[0])], y, p.shapes[id(n.inputs[0])][3])

    def _fwd_ResizeBilinear(self, p, n, y, scal, seed):
        x = p.buf[id(n.inputs[0])]
        if x.shape[1] == 1 and x.shape[2] == 1:      # align_corners from 1x1: a broadcast
            ops.spatial_broadcast(x, y, 1.0)
        else:
            ops.resize_bilinear_fwd(x, y)

    def _fwd_GlobalAvgPool(self, p, n, y, scal, seed):
        x = p.buf[id(n.inputs[0])]
        if not ops.spatial_reduce_fits(x.shape[3], self.cdt):
            # wider than seg_spatial_reduce takes (EfficientNet's 1152-channel fp32 maps): the squeeze kernel
            ops.se_squeeze(x, y, p.shapes[id(n.inputs[0])][3], 1.0 / (x.shape[1] * x.shape[2]), self.ws)
            return
        ops.spatial_reduce(x, y, 1.0 / (x.shape[1] * x.shape[2]), self.ws)

    def _fwd_ExpandDims(self, p, n, y, scal, seed):
        pass                               # a view of its input (planner._allocate)
