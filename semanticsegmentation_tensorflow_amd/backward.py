"""Backward pass of a Session step (mixin): the nodes of the plan in reverse
order, one launch method per node kind (`_bwd_<kind>`, beside forward.py's
`_fwd_<kind>`), and the gradient buffers of the pass (`_Grads`).  Split out of
session.py; `Session` inherits these methods."""
from __future__ import annotations

import torch

from . import ops


def _drops(n):
    """Node n's dropout is active this step (keep_prob < 1 fed or given)."""
    return n.kp_val is not None and n.kp_val < 1.0


def _drop_scale(n):
    return 1.0 / n.kp_val if _drops(n) else 1.0


class _Grads:
    """The activation gradients of one backward pass and where each launch
    writes its contribution.  The buffers themselves persist in the plan
    (Plan.scratch); this object only knows which of them hold data yet."""

    def __init__(self, sess, p):
        self.s = sess
        self.p = p
        self.grad = {}        # tensor id -> its gradient (complete once its node is reached)
        self.ginit = set()    # aliased-concat roots whose gradient buffer holds data this step
        # deferred BN-backward finishes: (segment, variable names) per fused launch
        self.bn_defer = ([] if (sess.defer_bn_finish and sess._dpa is None and sess._adam_ctx is None
                                and sess.device.type == "cuda") else None)
        self.main_wg = set()  # convs whose filter gradient stays on the compute stream
        if sess._red is not None and sess.main_wgrad > 0:
            convs = [m for m in p.nodes if m.kind == "conv" and m.w.var_name in p.var_set
                     and m.pro is None and id(m) not in p.adam_fusable]
            self.main_wg = {id(m) for m in convs[:sess.main_wgrad]}

    def _zeros_for(self, t):
        # (a pool-fused conv's output has no buffer: only its shape)
        b = self.p.buf[id(t)]
        return torch.zeros_like(b) if b is not None else self.s._act(self.p.shapes[id(t)])

    def dest(self, t):
        """(buffer to write t's gradient into, accumulate-after flag)."""
        if id(t) not in self.grad:
            gbuf = self.p.scratch(("g", id(t)), self._zeros_for, t)
            self.grad[id(t)] = gbuf
            return gbuf, None
        return self.p.scratch(("acc", id(t)), self._zeros_for, t), self.grad[id(t)]

    @staticmethod
    def done(dst, acc):
        if acc is not None:
            ops.add(acc, dst, acc)

    def var_dest(self, name):
        """Where a variable's gradient is written: its slice of the flat
        buffer when it is in var_list; otherwise a scratch sink, so the
        slices the data-parallel buckets release up front (never_ready) are
        not written while their all-reduce may be reading them."""
        store = self.s.store
        if name in self.p.var_set:
            return store.grad(name)
        return self.p.scratch(("gscratch", name), torch.zeros_like, store.grad(name))

    def bn_part(self, n):
        """Persistent partial-row buffer of node n's fused BN backward."""
        return self.p.scratch(("bnpart", id(n)), self._new_bn_part, n)

    def _new_bn_part(self, n):
        return torch.empty(max(1, ops.conv_bwd_data_bn_part_rows(n.desc)) * 2 * n.desc.C,
                           dtype=torch.float32, device=self.s.device)

    def alias_dest(self, t):
        """Slice of the root's gradient buffer for aliased t, and whether the
        kernel must accumulate into it (False only for the first write
        when it covers the whole root)."""
        p = self.p
        r, off = p.alias[id(t)]
        dB = p.scratch(("ga", r), torch.zeros_like, p.buf[r])
        C = p.shapes[id(t)][3]
        view = dB[..., off:off + C]
        self.grad[id(t)] = view
        if r not in self.ginit:
            self.ginit.add(r)
            if off == 0 and C == p.shapes[r][3]:
                return view, False
            dB.zero_()
        return view, True

    def kernel_dest(self, t):
        """(buffer, accumulate-after buffer, accumulate-in-kernel flag) for a
        kernel that can add into an aliased root's slice itself."""
        if id(t) in self.p.alias:
            dst, accf = self.alias_dest(t)
            return dst, None, accf
        dst, acc = self.dest(t)
        return dst, acc, False

    def contribute(self, t, g):
        """g is (a contribution to) t's gradient as it stands, no kernel needed."""
        if id(t) not in self.p.needs_grad:
            return
        if id(t) not in self.grad:
            # share the buffer only when no later contribution will add into
            # it (side-stream filter gradients may still be reading g)
            self.grad[id(t)] = g if self.p.ncons[id(t)] <= 1 else g.clone()
        else:
            ops.add(self.grad[id(t)], g, self.grad[id(t)])

    def alias_parts(self, n):
        """Aliased concat n (a view): its parts' gradients are slices of the
        root's buffer, which the consumers accumulated into."""
        p = self.p
        r = p.alias[id(n.output)][0]
        if r in self.ginit:
            dB = p.tmp[("ga", r)]
            for t in n.inputs:
                if id(t) in p.needs_grad and id(t) not in self.grad:
                    off = p.alias[id(t)][1]
                    self.grad[id(t)] = dB[..., off:off + p.shapes[id(t)][3]]


class BackwardMixin:
    def _grad_ready(self, names):
        """The gradients of `names` are final once the kernels enqueued so far
        run: hand them to the all-reduce (DP) or straight to the overlapped
        optimizer."""
        if self._ready_filter is not None:
            names = [nm for nm in names if nm in self._ready_filter]
        if self._dpa is not None:
            self.dp.ready(names)
        elif self._adam_ctx is not None:
            self._adam_ctx.launch(names)

    def _mask_epi(self, p, x):
        """Epilogue fusing the ReluGrad (x 1/keep_prob) of x's producer into the
        input-gradient kernel of x's (only) consumer, or None."""
        prod = p.producer.get(id(x))
        if prod is None or id(prod) not in p.mask_fuse:
            return None
        return ops.epilogue(relu_mask=p.buf[id(x)], mask_scale=_drop_scale(prod))

    def _scratch_grad(self, p, var):
        """fp32 gradient sink for a filter outside var_list whose layer still
        needs its bias gradient (the filter-gradient launch sums it)."""
        return p.scratch(("wscratch", var.var_name), torch.zeros, tuple(var.shape), dtype=torch.float32,
                         device=self.device)

    def _bias_relu_bwd(self, dy, y, dz, dbias, k_valid, relu, scale):
        # with TF1 dropout fused after the relu: dz = dy * (y > 0) / keep_prob
        ops.bias_relu_bwd(dy, y, dz, dbias, k_valid, relu, self.ws, scale=scale)

    def _grads_finite(self):
        """All gradients finite (every rank's, under data parallelism)?  One
        device-to-host read per step on the loss-scaled path."""
        if self._finite_flag is None:
            self._finite_flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        ops.check_finite(self.store.grads, self._finite_flag)
        if self._dpa is not None:
            import torch.distributed as dist
            dist.all_reduce(self._finite_flag, op=dist.ReduceOp.MAX, group=self.dp.group)
        return int(self._finite_flag.item()) == 0

    def _snap(self, t):
        """tests (self.capture): a copy of t as it is now on the stream (an
        extra copy; the launch plan is unchanged), else None."""
        return t.clone() if (self.capture is not None and t is not None) else None

    # ------------------------------------------------------------- backward
    def _backward(self, p, scal):
        g = _Grads(self, p)
        for n in reversed(p.nodes):
            if n.kind == "input" or id(n.output) not in p.needs_grad:
                continue
            if id(n) in p.alias_nodes:
                g.alias_parts(n)
                continue
            if n.kind == "xent":
                # only the heads of the loss being minimised; any other loss of the plan is forward-only
                if n.in_loss:
                    g.contribute(n.inputs[0], n.dlogits)
                continue
            dy = g.grad.get(id(n.output))
            if dy is None:
                continue          # output does not reach the loss
            bwd = getattr(self, "_bwd_" + n.kind, None)
            if bwd is None:
                raise NotImplementedError(f"backward of {n.kind}")
            bwd(p, n, dy, g)
        if g.bn_defer:
            # every deferred dgamma / dbeta in two launches (the same sums as
            # each launch's own finish); the segment table is built once per plan
            segs = [s for s, _ in g.bn_defer]
            key = tuple((s[0].data_ptr(), int(s[1]), s[5].data_ptr()) for s in segs)
            if p.bn_batch is None or p.bn_batch.key != key:
                p.bn_batch = ops.BnFinishBatch(segs, self.device)
            p.bn_batch.run()
            self._grad_ready([nm for _, names in g.bn_defer for nm in names])

    # ----------------------------------------------------------------- conv
    def _bwd_conv(self, p, n, dy, g):
        dz, fused_db = self._conv_dz(p, n, dy, g)
        dgrad = self._conv_dgrad(p, n, dz, g)
        if self.capture is not None:
            self.capture.append(self._capture_record(p, n, dz, dgrad))
        self._conv_wgrad(p, n, dz, fused_db, g)
        self._grad_ready([n.w.var_name] + ([n.bias.var_name] if n.bias is not None else []))

    def _conv_dz(self, p, n, dy, g):
        """The gradient at the conv's own output, before its epilogue's
        dropout / ReLU / bias: (dz, fused_db) with fused_db the bias-gradient
        destination when the filter-gradient launch is to sum it."""
        dz = dy
        fused_db = None
        yb = p.buf[id(n.output)]
        if not n.relu and _drops(n) and id(n) not in p.drop_folded:
            # dropout applied in the forward epilogue, no ReLU: re-draw its mask
            dz = p.scratch(("dz", id(n.output)), torch.zeros_like, yb)
            ops.dropout_bwd_ch(dy, dz, n.desc.k_valid, n.kp_val, n.seed_val)
            if n.bias is not None:
                fused_db = g.var_dest(n.bias.var_name)
        elif id(n) in p.mask_fuse or (n.bias is not None and not n.relu):
            # gradient arrives masked (or there is no ReLU): BiasAddGrad is
            # summed by the filter-gradient launch below
            if n.bias is not None:
                fused_db = g.var_dest(n.bias.var_name)
        elif n.relu or n.bias is not None:
            dz = p.scratch(("dz", id(n.output)), torch.zeros_like, yb)
            db = g.var_dest(n.bias.var_name) if n.bias is not None else None
            self._bias_relu_bwd(dy, yb if n.relu else None, dz, db, n.desc.k_valid, n.relu, _drop_scale(n))
        return dz, fused_db

    def _conv_dgrad(self, p, n, dz, g):
        """The conv's input gradient, in one of five forms.  Returns what the
        capture record (tests) says about it: dx (None when it went straight
        through a BatchNorm or MaxPool backward), dx_base, unpool, bn_bwd."""
        x = n.inputs[0]
        ng = p.needs_grad
        ws = self.ws
        out = {"dx": None, "dx_base": None, "unpool": None, "bn_bwd": None}
        b = n.pro if n.pro is not None else p.bn_before.get(id(n))
        if (b is not None and id(x) in ng and self.fuse_bn_bwd and id(b.inputs[0]) in ng
                and (b is n.pro or (id(b.inputs[0]) not in p.alias and id(b.inputs[0]) not in g.grad))
                and ops.conv_bwd_data_bn_workspace(n.desc) > 0):
            out["bn_bwd"] = self._conv_dgrad_bn(p, n, dz, g, b)
        elif id(n) in p.unpool_fuse:
            # input gradient continued through the MaxPoolGrad of the pool
            # before this conv (and its input's ReluGrad): written at the
            # pool input's resolution; the pooled gradient of the pool's
            # other consumers (done earlier in backward) is the residual
            m = p.unpool_fuse[id(n)]
            xf = m.inputs[0]
            dxf, accf = g.dest(xf)
            prod = p.producer.get(id(xf))
            relu = prod is not None and id(prod) in p.mask_fuse
            res = g.grad.get(id(x))
            out["dx_base"] = self._snap(res)
            self._timed(n.desc, ops.OP_BWD_DATA, ops.conv2d_bwd_data_unpool, n.desc, dz,
                        self._pack(n, ops.PACK_HWIO), p.pool_idx[id(m)], dxf, relu, res, ws)
            if self.capture is not None:
                # (full-res gradient, switches, relu) of the fused MaxPoolGrad
                out["unpool"] = (dxf.clone(), p.pool_idx[id(m)], relu)
            g.done(dxf, accf)
        elif id(x) in ng and id(x) in p.alias:
            # the input is an aliased concat root (FC-DenseNet decoder
            # concat views): the input gradient lands in the shared
            # gradient buffer -- whole (first write) or accumulated
            # in the epilogue
            dx, accf = g.alias_dest(x)
            if accf:
                out["dx_base"] = self._snap(dx)
            self._timed(n.desc, ops.OP_BWD_DATA, ops.conv2d_bwd_data, n.desc, dz, self._pack(n, ops.PACK_HWIO),
                        dx, ws, None, ops.epilogue(residual=dx) if accf else None)
            out["dx"] = dx
        elif id(x) in ng:
            dx, acc = g.dest(x)
            mepi = self._mask_epi(p, x)
            if acc is not None and mepi is None and self.fuse_grad_sum:
                # a further consumer's contribution: accumulated in the
                # epilogue, in place (residual = the gradient so far)
                out["dx_base"] = self._snap(acc)      # tests: the sum before this launch
                self._timed(n.desc, ops.OP_BWD_DATA, ops.conv2d_bwd_data, n.desc, dz,
                            self._pack(n, ops.PACK_HWIO), acc, ws, None, ops.epilogue(residual=acc))
                dx = acc
            elif mepi is not None and acc is None and id(n) in p.bits_dgrad:
                # the ReluGrad mask from the producer's bits (planner._plan_relu_bits)
                self._timed(n.desc, ops.OP_BWD_DATA, ops.conv2d_bwd_data_bits, n.desc, dz,
                            self._pack(n, ops.PACK_HWIO), p.mask_bits[id(p.producer[id(x)])], dx,
                            mepi.mask_scale, ws)
                g.done(dx, acc)
            else:
                self._timed(n.desc, ops.OP_BWD_DATA, ops.conv2d_bwd_data, n.desc, dz,
                            self._pack(n, ops.PACK_HWIO), dx, ws, None, mepi)
                g.done(dx, acc)
            out["dx"] = dx
        return out

    def _conv_dgrad_bn(self, p, n, dz, g, b):
        """Conv n's input gradient carried through the backward of BatchNorm
        (+ReLU) node b in the same launch; b's own backward is skipped (its
        output gradient is never materialised).  b is folded into n's prologue
        (n.pro) or precedes a growth conv (p.bn_before: the launch also applies
        the dropout gradient before b).  Returns the capture's bn_bwd (tests)."""
        store = self.store
        folded = b is n.pro
        xb = b.inputs[0]
        dxb, acc, accf = g.kernel_dest(xb)
        c1 = None if folded else p.drop_fold.get(id(b))
        drop = (c1.kp_val, c1.seed_val) if (c1 is not None and _drops(c1)) else None
        gn, bn_ = b.gamma.var_name, b.beta.var_name
        base = self._snap(dxb) if accf else None
        if g.bn_defer is not None:
            part = g.bn_part(n)
            self._timed(n.desc, ops.OP_BWD_DATA_BN, ops.conv2d_bwd_data_bn_part, n.desc, dz,
                        self._pack(n, ops.PACK_HWIO), p.buf[id(xb)], store.param(gn), store.param(bn_), dxb, part,
                        b.eps, b.relu, accf, None, drop)
            g.bn_defer.append(((part, ops.conv_bwd_data_bn_part_rows(n.desc), n.desc.C, n.desc.c_valid,
                                b.eps, g.var_dest(gn), g.var_dest(bn_)), [gn, bn_]))
        else:
            self._timed(n.desc, ops.OP_BWD_DATA_BN, ops.conv2d_bwd_data_bn, n.desc, dz,
                        self._pack(n, ops.PACK_HWIO), p.buf[id(xb)], store.param(gn), store.param(bn_), dxb,
                        g.var_dest(gn), g.var_dest(bn_), b.eps, b.relu, accf, self.ws, None, drop)
        rec = None
        if self.capture is not None:
            rec = {"xb": p.buf[id(xb)], "gamma": gn, "beta": bn_, "eps": b.eps, "relu": b.relu,
                   "base": base, "drop": drop, "folded": folded, "dxb": dxb.clone(),
                   "kernel": ops.conv_kernel_info(n.desc, ops.OP_BWD_DATA_BN)[0]}
        g.done(dxb, acc)
        if g.bn_defer is None:
            self._grad_ready([gn, bn_])
        return rec

    def _capture_record(self, p, n, dz, dgrad):
        # tests: the buffers of this layer's three kernels (they persist
        # after the step; dx before any accumulation of later consumers,
        # or -- accumulated in the epilogue -- with dx_base, the sum it
        # was added to; None when it went straight through a folded BN
        # backward)
        buf = p.buf
        x, pro, dx = n.inputs[0], n.pro, dgrad["dx"]
        mask = self._mask_epi(p, x) if dx is not None else None
        return {"kind": "conv", "name": n.w.var_name, "bias": getattr(n.bias, "var_name", None),
                "x": buf[id(x)] if pro is None else buf[id(pro.inputs[0])],
                "pro": None if pro is None else (pro.gamma.var_name, pro.beta.var_name, pro.eps, pro.relu),
                "y": buf[id(n.output)], "dz": dz,
                # MaxPool fused into the forward: (pooled map, switches)
                "pool": ((buf[id(p.pool_fuse[id(n)].output)], p.pool_idx.get(id(p.pool_fuse[id(n)])))
                         if id(n) in p.pool_fuse else None),
                # a copy: later consumers may accumulate into the buffer
                "dx": None if dx is None else dx.clone(), "dx_base": dgrad["dx_base"],
                "unpool": dgrad["unpool"],
                "dx_masked": mask is not None,
                "mask_scale": (mask.mask_scale if mask is not None else 1.0),
                "relu": n.relu, "keep_prob": n.kp_val, "seed": n.seed_val,
                # input gradient through a BatchNorm(+ReLU) backward in
                # the dgrad epilogue (igemm_nt2_bn / conv_res16c_bn)
                "bn_bwd": dgrad["bn_bwd"],
                "fused_adam": False, "desc": n.desc,
                "stride": n.stride, "dilation": n.dilation, "dilation_hw": n.dilation_hw,
                "padding": n.padding}

    def _conv_wgrad(self, p, n, dz, fused_db, g):
        """The conv's filter (and, with fused_db, bias) gradient."""
        store, ws = self.store, self.ws
        x = p.buf[id(n.inputs[0])]
        want_w = n.w.var_name in p.var_set
        want_b = n.bias is not None and n.bias.var_name in p.var_set
        gw = store.grad(n.w.var_name) if want_w else self._scratch_grad(p, n.w)
        if not (want_w or want_b):
            pass          # frozen layer (outside var_list): no filter gradient
        elif n.pro is not None:
            # input relu(BN(x)) recomputed from x while staging (folded BatchNorm);
            # on the side stream beside the input-gradient chain, as below
            b = n.pro
            side = self._wgrad_side(p, n)
            with self._beside(side):
                self._timed(n.desc, ops.OP_BWD_FILTER_PRO, ops.conv2d_bwd_filter_pro, n.desc,
                            p.buf[id(b.inputs[0])], self._prologue(b), dz, gw,
                            self._node_ws(p, n) if side is not None else ws, None, fused_db)
        elif self._fused is not None and id(n) in p.adam_fusable and want_w:
            # Conv2DBackpropFilter + AdamOptimizer on the filter in one launch
            opt, gs, fdone = self._fused
            wn = n.w.var_name
            side = self._wgrad_side(p, n, level=2)

            def launch_fused():
                # on the side stream too: its input gradient (the only reader of the
                # packed copies it rewrites) is already enqueued on the compute stream
                with self._beside(side):
                    self._timed(n.desc, ops.OP_BWD_FILTER, ops.conv2d_bwd_filter_adam, n.desc, x,
                                dz, store.param(wn), store.adam_m(wn), store.adam_v(wn), opt.lr, store.step,
                                opt.beta1, opt.beta2, opt.epsilon, gs, store.packed.get((wn, ops.PACK_HWIO)),
                                store.packed.get((wn, ops.PACK_KRSC)),
                                store.grad(wn) if self.store_fused_grads else None, fused_db,
                                self._node_ws(p, n) if side is not None else ws)
            if side is not None and self.fused_delay > 0:
                # issued after the next `fused_delay` side-stream filter gradients, so
                # the HBM-bound update does not starve the input-gradient chain early on
                self._pending_fused.append([self.fused_delay, launch_fused])
            else:
                launch_fused()
            fdone.add(wn)
            if self.capture is not None:
                self.capture[-1]["fused_adam"] = True
        elif self._red is not None and self.side_wgrad >= 1 and id(n) not in g.main_wg:
            # the whole filter gradient (kernel + split-K reduction) on the
            # side stream, beside the input-gradient chain: every operand
            # (x, dz, the per-node workspace) stays untouched until the
            # join before Adam
            wsb = p.wg_ws[id(n)]
            with self._beside(self._red[0]):
                tok = self._timed(n.desc, ops.OP_BWD_FILTER, ops.conv2d_bwd_filter_begin, n.desc, x,
                                  dz, gw, wsb, fused_db)
                ops.conv2d_bwd_filter_end(tok, gw, wsb, fused_db)
            self._tick_fused()
        elif self._red is not None and id(n) not in g.main_wg:
            # kernel now, its split-K reduction on the side stream
            side, main = self._red
            wsb = p.wg_ws[id(n)]
            tok = self._timed(n.desc, ops.OP_BWD_FILTER, ops.conv2d_bwd_filter_begin, n.desc, x,
                              dz, gw, wsb, fused_db)
            if tok[1][0] > 1:
                ev = torch.cuda.Event()
                ev.record(main)
                side.wait_event(ev)
                ops.conv2d_bwd_filter_end(tok, gw, wsb, fused_db, stream=side)
        else:
            self._timed(n.desc, ops.OP_BWD_FILTER, ops.conv2d_bwd_filter, n.desc, x, dz,
                        gw, ws, None, fused_db)

    # ---------------------------------------------------------- other kinds
    def _bwd_tconv(self, p, n, dy, g):
        x = n.inputs[0]
        ng, ws = p.needs_grad, self.ws
        if n.residual is not None:
            g.contribute(n.residual, dy)
        if id(x) in ng and id(x) in p.alias:
            # the input is an aliased concat root (decoder concat views)
            dx, accf = g.alias_dest(x)
            self._timed(n.desc, ops.OP_TBWD_DATA, ops.tconv2d_bwd_data, n.desc, dy,
                        self._pack(n, ops.PACK_TCONV_BWD), dx, ws, None,
                        ops.epilogue(residual=dx) if accf else None)
        elif id(x) in ng:
            dx, acc = g.dest(x)
            self._timed(n.desc, ops.OP_TBWD_DATA, ops.tconv2d_bwd_data, n.desc, dy,
                        self._pack(n, ops.PACK_TCONV_BWD), dx, ws, None, self._mask_epi(p, x))
            g.done(dx, acc)
        want_w = n.w.var_name in p.var_set
        want_b = n.bias is not None and n.bias.var_name in p.var_set
        if want_w or want_b:
            # on the side stream beside the input-gradient chain (as the conv filter gradients)
            side = self._wgrad_side(p, n)
            with self._beside(side):
                self._timed(n.desc, ops.OP_TBWD_FILTER, ops.tconv2d_bwd_filter, n.desc, p.buf[id(x)], dy,
                            self.store.grad(n.w.var_name) if want_w else self._scratch_grad(p, n.w),
                            self._node_ws(p, n) if side is not None else ws, None,
                            g.var_dest(n.bias.var_name) if n.bias is not None else None)
        self._grad_ready([n.w.var_name] + ([n.bias.var_name] if n.bias is not None else []))

    def _bwd_dwconv(self, p, n, dy, g):
        x = n.inputs[0]
        wn = n.w.var_name
        if id(x) in p.needs_grad:
            dx, acc = g.dest(x)
            ops.dwconv2d_bwd_data(n.desc, dy, self.store.param(wn), dx)     # a gather: dx written whole
            g.done(dx, acc)
        if wn in p.var_set:
            # on the side stream beside the input-gradient chain (as the conv filter gradients)
            side = self._wgrad_side(p, n)
            with self._beside(side):
                ops.dwconv2d_bwd_filter(n.desc, p.buf[id(x)], dy, self.store.grad(wn),
                                        p.wg_ws[id(n)] if side is not None else self.ws)
        self._grad_ready([wn])

    def _bwd_MaxPool(self, p, n, dy, g):
        x = n.inputs[0]
        if id(n) in p.unpool_pools:
            return            # done in the consuming conv's input-gradient epilogue
        if id(x) in p.needs_grad:
            dx, acc = g.dest(x)
            prod = p.producer.get(id(x))
            relu = prod is not None and id(prod) in p.mask_fuse
            idx = p.pool_idx.get(id(n))
            if idx is not None:
                ops.maxpool2x2_bwd_argmax(idx, dy, dx, relu_mask=relu)
            else:
                ops.maxpool2x2_bwd(p.buf[id(x)], p.buf[id(n.output)], dy, dx, relu_mask=relu)
            g.done(dx, acc)

    def _bwd_AvgPool(self, p, n, dy, g):
        x = n.inputs[0]
        if id(x) in p.needs_grad:
            dx, acc = g.dest(x)
            ops.avgpool2x2_bwd(dy, dx)
            g.done(dx, acc)

    def _bwd_Pool2D(self, p, n, dy, g):
        x = n.inputs[0]
        if id(x) in p.needs_grad:
            dx, acc = g.dest(x)
            ops.pool2d_bwd(n.desc, p.pool_idx.get(id(n)), dy, dx)     # a gather: dx written whole
            g.done(dx, acc)

    def _bwd_Subsample(self, p, n, dy, g):
        # the compact gradient (the sum over the sibling convs) scattered into
        # the full map, zeros at the pixels the stride skips
        self._bwd_Pool2D(p, n, dy, g)

    def _bwd_Pad(self, p, n, dy, g):
        x = n.inputs[0]
        if id(x) in p.needs_grad:
            dx, acc = g.dest(x)
            ops.pad2d_bwd(dy, dx, n.ops[0].attrs["pads"])
            g.done(dx, acc)

    def _bwd_Add(self, p, n, dy, g):
        for t in n.inputs:
            g.contribute(t, dy)

    def _bwd_ConcatV2(self, p, n, dy, g):
        parts = []
        for t in n.inputs:
            C = p.shapes[id(t)][3]
            if id(t) not in p.needs_grad:
                # still consume its channel range: a zero-width part is not allowed,
                # so write into a scratch gradient that nobody reads
                parts.append((p.scratch(("cz", id(t)), torch.zeros_like, p.buf[id(t)]), C, False))
            elif id(t) in p.alias:
                v, accf = g.alias_dest(t)
                parts.append((v, C, accf))
            elif id(t) in g.grad:
                parts.append((g.grad[id(t)], C, True))
            else:
                g.grad[id(t)] = p.scratch(("g", id(t)), torch.zeros_like, p.buf[id(t)])
                parts.append((g.grad[id(t)], C, False))
        ops.concat_bwd(dy, parts)

    def _bwd_bn(self, p, n, dy, g):
        x = n.inputs[0]
        store = self.store
        dx, acc, accf = g.kernel_dest(x)
        if n.act is not None:               # BatchNorm + swish: z and sigmoid(z) recomputed from x
            ops.bn_act_bwd(p.buf[id(x)], dy, dx, store.param(n.gamma.var_name), store.param(n.beta.var_name),
                           g.var_dest(n.gamma.var_name), g.var_dest(n.beta.var_name), p.shapes[id(x)][3], n.act,
                           n.eps, self.ws, accumulate=accf)
            g.done(dx, acc)
            self._grad_ready([n.gamma.var_name, n.beta.var_name])
            return
        drop = None
        c = p.drop_fold.get(id(n))
        if c is not None and _drops(c):
            if accf or acc is not None:
                raise RuntimeError(f"{n.ops[0].name}: folded dropout gradient needs a sole reader")
            drop = (c.kp_val, c.seed_val, c.desc.k_valid)
        ops.bn_relu_bwd(p.buf[id(x)], p.buf[id(n.output)], dy, dx, store.param(n.gamma.var_name),
                        g.var_dest(n.gamma.var_name), g.var_dest(n.beta.var_name), p.shapes[id(x)][3], n.relu,
                        n.eps, self.ws, accumulate=accf, beta=store.param(n.beta.var_name), dropout=drop)
        g.done(dx, acc)
        self._grad_ready([n.gamma.var_name, n.beta.var_name])

    def _bwd_act(self, p, n, dy, g):
        x = n.inputs[0]
        if id(x) in p.needs_grad:
            dx, acc = g.dest(x)
            ops.bn_act_bwd(p.buf[id(x)], dy, dx, None, None, None, None, p.shapes[id(x)][3], n.act)
            g.done(dx, acc)

    def _bwd_se_excite(self, p, n, dy, g):
        # dx = dy * s and ds = sum_hw dy * x in one pass; x's other reader (the
        # squeeze) adds its share through dest / done like any second reader
        x, s = n.inputs
        xb = p.buf[id(x)]
        cv = p.shapes[id(x)][3]
        if id(x) in p.needs_grad:
            dx, acc = g.dest(x)
        else:
            dx, acc = p.scratch(("sx", id(x)), torch.zeros_like, xb), None
        if id(s) in p.needs_grad:
            ds, sacc = g.dest(s)
        else:
            ds, sacc = p.scratch(("ss", id(s)), torch.zeros_like, p.buf[id(s)]), None
        ops.se_excite_bwd(xb, p.buf[id(s)], dy, dx, ds, cv, self.ws)
        if id(x) in p.needs_grad:
            g.done(dx, acc)
        if id(s) in p.needs_grad:
            g.done(ds, sacc)

    def _ew_dest(self, p, t, g):
        """(buffer, accumulate-after buffer, accumulate-in-kernel flag) of an
        elementwise gradient output, or (None, None, False) when t needs none."""
        if id(t) not in p.needs_grad:
            return None, None, False
        return g.kernel_dest(t)

    def _bwd_film(self, p, n, dy, g):
        # dalpha, df and dbeta in one pass; the ReLU mask from the stored output
        a, f, b = n.inputs
        if len({id(a), id(f), id(b)}) != 3:
            raise NotImplementedError(f"{n.ops[0].name}: one tensor as two operands of the modulation")
        dsts = [self._ew_dest(p, t, g) for t in (a, f, b)]
        if all(d[0] is None for d in dsts):
            return
        ops.film_bwd(dy, p.buf[id(n.output)] if n.relu else None, p.buf[id(a)], p.buf[id(f)], dsts[0][0], dsts[1][0],
                     dsts[2][0], p.shapes[id(n.output)][3], n.alpha_bias, n.relu, tuple(d[2] for d in dsts))
        for dst, acc, _ in dsts:
            if dst is not None:
                g.done(dst, acc)

    def _bwd_axpy(self, p, n, dy, g):
        # x's other readers (the concat) add their share through dest / done or the accumulate flag
        a, b = n.inputs
        if a is b:
            raise NotImplementedError(f"{n.ops[0].name}: x + number * x")
        dsts = [self._ew_dest(p, t, g) for t in (a, b)]
        if all(d[0] is None for d in dsts):
            return
        ops.axpy_relu_bwd(dy, p.buf[id(n.output)] if n.relu else None, dsts[0][0], dsts[1][0],
                          p.shapes[id(n.output)][3], n.lam, n.relu, tuple(d[2] for d in dsts))
        for dst, acc, _ in dsts:
            if dst is not None:
                g.done(dst, acc)

    def _bwd_Relu(self, p, n, dy, g):
        x = n.inputs[0]
        dx, acc = g.dest(x)
        self._bias_relu_bwd(dy, p.buf[id(n.output)], dx, None, p.shapes[id(x)][3], True, 1.0)
        g.done(dx, acc)

    def _bwd_Dropout(self, p, n, dy, g):
        dx, acc = g.dest(n.inputs[0])
        if n.kp_val < 1.0:
            ops.dropout_fwd(dy, dx, n.kp_val, n.seed_val)
        else:
            ops.copy_channels(dy, dx)
        g.done(dx, acc)

    def _bwd_GlobalAvgPool(self, p, n, dy, g):
        x = n.inputs[0]
        if id(x) in p.needs_grad:
            dx, acc = g.dest(x)
            xs = p.buf[id(x)]
            ops.spatial_broadcast(dy, dx, 1.0 / (xs.shape[1] * xs.shape[2]))
            g.done(dx, acc)

    def _bwd_ExpandDims(self, p, n, dy, g):
        if len(p.shapes[id(n.output)]) == 4 and len(p.shapes[id(n.inputs[0])]) == 4:
            g.contribute(n.inputs[0], dy)          # global-average-pool chain: same buffer

    def _bwd_ResizeBilinear(self, p, n, dy, g):
        x = n.inputs[0]
        if id(x) not in p.needs_grad:
            return
        dx, acc = g.dest(x)
        xs = p.buf[id(x)]
        if xs.shape[1] == 1 and xs.shape[2] == 1:
            ops.spatial_reduce(dy, dx, 1.0, self.ws)   # 1x1 -> HxW broadcast: gradient = spatial sum
        else:
            # align_corners bilinear: fp32 scatter-add, then cast to the compute dtype
            g32 = p.scratch(("rb32", id(x)), torch.zeros, dx.shape, dtype=torch.float32, device=self.device)
            ops.resize_bilinear_bwd(dy, g32)
            ops.cast(g32, dx)
        g.done(dx, acc)

    def _bwd_Softmax(self, p, n, dy, g):
        raise NotImplementedError("gradient of tf.nn.softmax: the reference uses it for evaluation only "
                                  "(Network/utils/utils.py:54); train on softmax_cross_entropy_with_logits")

    def _bwd_ArgMax(self, p, n, dy, g):
        pass
