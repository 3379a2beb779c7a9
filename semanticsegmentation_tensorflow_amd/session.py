"""Session: compiles the symbolic graph into a static launch plan over the HIP
C-ABI and runs it -- the stand-in for the reference's
`sess.run(train_step, feed_dict)` (Network/model/FCN.py:395-398).

Compilation (per fetch set and fed shapes):
  * shape resolution with TF's rules (conv2d_transpose shape check included);
  * fusion of single-consumer chains into one kernel launch each:
      Conv2D [+BiasAdd] [+Relu] [+Dropout]      -> conv (fused epilogue)
      Conv2DTranspose [+BiasAdd] [+Add]         -> tconv (bias + skip fusion)
      FusedBatchNorm [+Relu | +Swish]           -> bn
      SoftmaxXent + Mean                        -> xent (loss and dlogits)
      Mean(sum_i w_i SoftmaxXent_i)             -> one xent per head + xent_sum
      AddScalar -> MulFull -> Add [+Relu]       -> film (TransNet's modulation)
      Add(x, ScalarMul(lam, c)) [+Relu]         -> axpy (TransNet's fusion)
    and the lowering of a strided 1x1 Conv2D to a shared Subsample node + the
    same conv at stride 1 (planner._lower_strided_1x1);
  * static device buffers (NHWC, channels padded to 8) for every activation,
    gradient and workspace -- nothing is allocated while a step runs;
  * backward in reverse order with gradients written straight into the flat
    fp32 gradient buffer of the VariableStore; data-parallel buckets are
    all-reduced (RCCL) as soon as their gradients are complete, overlapping the
    rest of backward;
  * TF1 Adam over the flat buffer, then re-packing of the bf16/fp32 filter
    copies the convolution kernels read.

Here: run, the train-step surfaces, compilation into nodes and the step's top
level (`_execute`).  `Session` inherits the rest as mixins: planner.py (plans),
forward.py / backward.py (the launches, per node kind), streams.py (side stream).
"""
from __future__ import annotations

import numpy as np
import torch

from . import graph as G
from . import ops
from .backward import BackwardMixin
from .forward import ForwardMixin
from .planner import PlanMixin
from .streams import StreamMixin, _AdamOverlap
from .variables import VariableStore

_SEED_MIX = 0x9E3779B1


class _Node:
    """One fused kernel in the forward plan."""

    def __init__(self, kind, ops_, inputs, output, **kw):
        self.kind = kind
        self.ops = ops_
        self.inputs = inputs
        self.output = output
        # filled by _compile (kw) or the planner for some kinds only
        self.pro = None          # conv: the BatchNorm(+ReLU) node folded into its operand prologue
        self.fwd_hwio = False    # conv: the forward reads the HWIO packed copy
        self.residual = None     # tconv: the skip tensor added in its epilogue
        self.labels = None       # xent
        self.weight = 1.0        # xent: w_i of Mean(sum_i w_i xent_i)
        self.in_loss = True      # xent: a head of the loss being minimised (else forward-only)
        self.twin = None         # xent, forward-only: the xent node on the same logits / labels whose launch it shares
        self.kp = None           # conv: keep_prob of the dropout in its epilogue (tensor or number)
        self.kp_val = None       # conv / Dropout: this step's keep_prob and seed (set by the forward)
        self.seed_val = None
        self.act = None          # bn / act: "swish" or "sigmoid" (seg_bn_act_*); a bn with one takes no ReLU-BN fusion
        self.__dict__.update(kw)


class Plan:
    """The static launch plan of one fetch set at one set of fed shapes: the sets
    and dicts the executor reads start empty, planner.py fills those that apply."""

    def __init__(self):
        self.folded = set()        # BN node ids applied by their consumer conv's operand prologue
        self.drop_fold = {}        # BN node id -> conv whose dropout gradient the BN backward applies
        self.drop_folded = set()   # those convs' ids
        self.bn_before = {}        # growth conv id -> the BN node producing its input
        self.alias = {}            # tensor id -> (root tensor id, channel offset)
        self.alias_nodes = set()   # ConcatV2 node ids that became views
        self.pool_idx = {}         # MaxPool node id -> recorded switches (train plans)
        self.pool_fuse = {}        # conv id -> MaxPool node run in its pooled epilogue
        self.pool_fused = set()    # those MaxPool nodes' ids
        self.bn_out2 = {}          # conv id -> BN node whose output the conv launch also writes
        self.bn_out2_done = set()  # those BN nodes' ids
        self.unpool_fuse = {}      # conv id -> MaxPool node whose gradient runs in its dgrad epilogue
        self.unpool_pools = set()  # those MaxPool nodes' ids
        self.mask_fuse = set()     # ReLU conv ids whose gradient arrives already masked
        self.mask_bits = {}        # producer conv id -> its ReLU mask as bits
        self.bits_dgrad = set()    # consumer conv ids whose input gradient reads those bits
        self.adam_fusable = set()  # conv ids that can take the fused filter-gradient + Adam launch
        self.wg_ws = {}            # conv / tconv id -> its filter-gradient workspace (pending split-K slabs)
        self.producer = {}         # tensor id -> node
        self.ncons = {}            # tensor id -> number of consuming nodes
        self.tmp = {}              # persistent scratch buffers of the backward, by key
        self.bn_batch = None       # ops.BnFinishBatch of the deferred BN-backward finishes

    def scratch(self, key, make, *args, **kw):
        """The persistent buffer `key`, allocated as make(*args, **kw) on first use."""
        t = self.tmp.get(key)
        if t is None:
            t = self.tmp[key] = make(*args, **kw)
        return t


def _is_op(f, type_):
    return isinstance(f, G.Op) and f.type == type_


def _accumulator_pairs(op):
    """apply_gradients whose gradient sources are all variables (accumulators)."""
    return all(isinstance(g, G.Variable) for g, _ in op.attrs["pairs"])


def _gradient_source(t):
    """(loss, var, scale) of a compute_gradients output, optionally wrapped in
    tf.scalar_mul."""
    scale = 1.0
    if isinstance(t, G.Tensor) and t.op.type == "ScalarMul":
        scale = G.const_value(t.op.attrs["scalar"])
        t = t.op.attrs["x"]
    if not (isinstance(t, G.Tensor) and t.op.type == "Gradient"):
        raise NotImplementedError("expected an optimizer.compute_gradients output")
    return t.op.attrs["loss"], t.op.attrs["var"], scale


class _TrainSpec:
    """What a run call's gradient-consuming fetches ask for: the loss, the
    variables whose gradients are needed, and what consumes them (Adam with
    `optimizer`, or `accum` = [(accumulator, variable, scale)])."""

    def __init__(self, loss, optimizer, var_list, grad_scale, global_step, accum, ops_):
        self.inputs = [loss]
        self.attrs = {"optimizer": optimizer, "var_list": list(var_list), "grad_scale": float(grad_scale),
                      "global_step": global_step}
        self.accum = accum
        self.ops = ops_


_SIDE_STREAMS = {}


def side_stream_for(device):
    """The process-wide side stream of a device (filter gradients, their
    split-K reductions, the fused conv6 / conv7 update, bucket collectives),
    shared by every Session on it.  HIP maps streams onto a fixed pool of
    hardware queues (GPU_MAX_HW_QUEUES, 4 on the box), and a stream created
    after an RCCL communicator took some of them can land on the compute
    stream's queue: every launch of the step then runs serialised on one queue
    (round 6: the world-1 data-parallel step at 7.6 ms instead of 6.8,
    tools/queue_probe.py).  Created before init_process_group -- bench.py
    calls this first; a data-parallel program should too -- it keeps a queue
    of its own."""
    device = torch.device(device)
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    s = _SIDE_STREAMS.get(key)
    if s is None:
        s = _SIDE_STREAMS[key] = torch.cuda.Stream(device=device)
        with torch.cuda.stream(s):      # a first launch binds the stream to its queue now
            torch.zeros(1, device=device)
    return s


class Session(PlanMixin, ForwardMixin, BackwardMixin, StreamMixin):
    def __init__(self, graph=None, compute_dtype="bf16", device=None, seed=0, data_parallel=None,
                 overlap_optimizer=False, fuse_adam=True, loss_scale=None):
        """compute_dtype: "bf16" (default), "f16" (IEEE half activations and
        filter copies, fp32 accumulation -- config C5) or "f32" (parity path).
        loss_scale (f16): "dynamic" (default for f16: TF's DynamicLossScale,
        2^15 initial, x2 after 2000 finite steps, /2 and skip the update on
        overflow), a fixed number, or None/1 (no scaling)."""
        self.graph = graph or G.get_default_graph()
        if not torch.cuda.is_available():
            raise RuntimeError("Session needs an MI355X (HIP device); there is no CPU fallback")
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.cdt = {"bf16": ops.BF16, "bfloat16": ops.BF16, "f16": ops.F16, "fp16": ops.F16,
                    "float16": ops.F16, "f32": ops.F32, "fp32": ops.F32, "float32": ops.F32}[compute_dtype]
        self.tdt = ops.torch_dtype(self.cdt)
        if loss_scale is None and self.cdt == ops.F16:
            loss_scale = "dynamic"
        self.dynamic_scale = loss_scale == "dynamic"
        self.loss_scale = 2.0 ** 15 if self.dynamic_scale else float(loss_scale or 1.0)
        self.scale_increment_period = 2000
        self.good_steps = 0
        self.skipped_steps = 0
        self._finite_flag = None
        self.seed = seed
        self.store = None
        self.plans = {}
        self.ws = ops.Workspace(self.device)
        self.dp = data_parallel
        self.run_count = 0
        self._packed_version = -1
        self._adam_key = None
        self._adam = None
        self._adam_groups = {}
        self.overlap_optimizer = overlap_optimizer
        # Adam fused into the filter-gradient epilogue where the library supports
        # it (single process: nothing sits between gradient and update)
        self.fuse_adam = fuse_adam
        self.store_fused_grads = False   # tests: also write the fused layers' gradients
        self._fused = None               # names updated inside backward this step
        # split-K reductions of filter gradients on a side stream, overlapping
        # the next layer's input gradient (with data parallelism each bucket's
        # all-reduce is issued from that side stream, after it has caught up
        # with the compute stream)
        self.defer_wgrad_reduce = True
        # Dropout right after a bias-free / ReLU-free conv (FC-DenseNet's
        # Conv2D_Block + dropout) applied in the conv epilogue
        self.fuse_dropout = True
        # DenseBlock concatenations as channel views of one block buffer
        self.alias_concat = True
        # BatchNorm(+ReLU) feeding a single 1x1 conv folded into its operand prologue
        self.fold_bn = True
        self.fold_dropout_grad = True   # Conv -> Dropout -> BN: the dropout gradient inside the BN backward
        # Schedule attributes (measured defaults; every value is exercised by
        # tests/test_gpu_dp_rccl.py against the default schedule -- bench.py
        # --schedule NAME=VALUE sets them for A/B runs):
        # a tensor's later input-gradient contributions accumulate in the epilogue
        self.fuse_grad_sum = True
        self.fuse_bn_bwd = True         # folded BN: its backward in the consuming 1x1 conv's dgrad epilogue
        # conv (+bias +ReLU) -> 2x2 MaxPool as one launch (pooled epilogue)
        self.fuse_pool = True
        # 2x2 MaxPool -> conv: the MaxPoolGrad in the conv's input-gradient
        # epilogue (the pooled gradient never written)
        self.fuse_unpool = True
        # filters of >= 8 M elements: one packed copy (HWIO), read by the
        # forward too (igemm_nt3's B-transposed form) -- set before the first run
        self.fwd_hwio = True
        # conv1_1's ReLU mask written as bits for conv1_2's input gradient
        # (planner._plan_relu_bits)
        self.relu_bits = True
        # conv -> BatchNorm(+ReLU): the BN output written by the conv epilogue
        self.fuse_bn_out = True
        # the dgamma / dbeta sums of the BN backwards fused into input-gradient
        # launches finished together at the end of backward (two launches per
        # step instead of one or two per BatchNorm; single-process steps)
        self.defer_bn_finish = True
        self._red = None                 # (side stream, compute stream) during a step
        # deferred filter gradients: the kernel too (not only its reduction) on
        # the side stream (1), and the fused filter-gradient + Adam launches (2)
        self.side_wgrad = 2
        # the fused conv6 / conv7 filter-gradient + Adam launches go to the side
        # stream after the next `fused_delay` filter gradients there (the
        # HBM-bound update then overlaps the smaller conv4_x / conv3_x layers
        # instead of starving conv5_x's input gradients: 547 -> 554 img/s at 5-7
        # in round 3; round 6, with conv_halo4 and the update on 256 x 256
        # tiles: 2 -- 592.1 / 590.8 vs 583.6 / 582.8 img/s at 6 on the same box)
        self.fused_delay = 2
        self._pending_fused = []
        # the filter gradients of the first `main_wgrad` convs (the last in the
        # backward: conv1_1 / conv1_2 / conv2_1 in FCN) stay on the compute
        # stream, which has no input gradient left to run then, beside the side
        # stream's remaining filter gradients instead of after them (round 5:
        # 3 over 2 by 0.3 % in five A/B pairs)
        self.main_wgrad = 3
        # data-parallel all-reduce steps: the Adam update of every variable of
        # >= overlap_big_mb MB (FCN conv6 / conv7) as soon as its buckets'
        # collectives complete, on the side stream beside the rest of backward
        # (0: all at the end).  Default since round 6: the world-1 RCCL probe
        # 558.0 vs 555.7 img/s with the side stream on a queue of its own
        self.overlap_big_mb = 64

        self._side = None
        self._adam_ctx = None
        self._ready_filter = None
        self.capture = None    # tests: list -> per-conv buffer records of the last backward
        self.timer = None      # list -> (desc, op, start_event, end_event) per conv launch
        self.timer_match = None   # (desc, op) -> bool: which launches self.timer records (None: all)

    # ------------------------------------------------------------------ vars
    def _ensure_store(self):
        if self.store is None or len(self.store.all_vars) != len(self.graph.variables):
            old = self.store
            self.store = VariableStore(list(self.graph.variables.values()), self.device, self.seed)
            self.store.initialize()
            if old is not None:
                for v in old.all_vars:
                    self.store.assign(v.var_name, old.read(v.var_name))
            self.plans = {}
        return self.store

    def variable_value(self, name):
        return self._ensure_store().read(name)

    def assign(self, name, value):
        self._ensure_store().assign(name, value)

    # ------------------------------------------------------------------- run
    def run(self, fetches, feed_dict=None, as_numpy=True):
        feed_dict = feed_dict or {}
        single = not isinstance(fetches, (list, tuple))
        flist = [fetches] if single else list(fetches)
        if any(_is_op(f, "InitAll") for f in flist):
            self._ensure_store().initialize()
        self._ensure_store()
        out = {}
        rest, post = [], []
        for f in flist:
            if _is_op(f, "InitAll"):
                out[id(f)] = None
            elif _is_op(f, "Assign"):              # zero_ops (Network/main.py:84-85)
                self._run_assign(f)
                out[id(f)] = None
            elif _is_op(f, "ApplyGradients") and _accumulator_pairs(f):
                post.append(f)                      # Adam on accumulated gradients, after the fetches
            else:
                rest.append(f)
        if rest:
            key = (tuple(id(f) for f in rest),
                   tuple(sorted((id(k), tuple(np.shape(v))) for k, v in feed_dict.items())))
            plan = self.plans.get(key)
            if plan is None:
                plan = self._compile(rest, feed_dict)
                self.plans[key] = plan
            out.update(self._execute(plan, feed_dict))
        for f in post:
            self._apply_accumulated(f)
            out[id(f)] = None
        res = []
        for f in flist:
            r = out.get(id(f))
            if as_numpy and isinstance(r, torch.Tensor):
                r = r.cpu().numpy()
            res.append(r)
        return res[0] if single else res

    # ------------------------------------------- accumulate-then-apply template
    def _run_assign(self, op):
        """`var.assign(tf.zeros_like(var))` / `var.assign(constant)` on device."""
        store = self.store
        var, val = op.attrs["var"], op.attrs["value"]
        if isinstance(val, G.Tensor) and val.op.type == "ZerosLike":
            value = 0.0
        else:
            value = G.const_value(val)
        if var.var_name in store.aux:
            t = store.aux[var.var_name]
            if t.dtype == torch.int64:
                t.fill_(int(round(value)))
            else:
                ops.fill(t, value)
            store.aux_version += 1
        else:
            ops.fill(store.param(var.var_name), value)
            store.version += 1

    def _apply_accumulated(self, op):
        """optimizer.apply_gradients([(accum_i, var_i)]) (Network/main.py:98-101):
        TF1 Adam on each var_i with the accumulated gradient accum_i; nothing
        else in the graph runs."""
        store = self.store
        opt = op.attrs["optimizer"]
        names = []
        for acc, var in op.attrs["pairs"]:
            g = store.grad(var.var_name)
            ops.fill(g, 0.0)
            ops.axpy(g.view(-1), store.aux[acc.var_name].view(-1), 1.0)
            names.append(var.var_name)
        self._repack(None)
        self.sync_optimizer_slots()      # after ZeRO-1 steps: whole m / v before a whole-variable Adam
        store.step += 1
        ops.adam_tf1_pack(store.params, store.grads, store.m, store.v, self._adam_plan(names), opt.lr,
                          store.step, opt.beta1, opt.beta2, opt.epsilon, grad_scale=1.0,
                          dtype=self._pack_dtype())
        store.version += 1
        self._packed_version = store.version     # adam_tf1_pack rewrote the packed copies it owns
        self._bump_global_step(op.attrs.get("global_step"))

    def _bump_global_step(self, gs):
        if gs is not None:
            t = self.store.aux.get(gs.var_name)
            if t is None:
                raise ValueError(f"global_step {gs.var_name} must be a non-trainable tf.Variable")
            t.add_(1)

    def _train_spec(self, fetches):
        """The gradient-consuming fetches of one run call as one spec:
        TrainStep (minimize), ApplyGradients over compute_gradients outputs, or
        AssignAdd(accum, [scalar_mul(c,] gradient[)]) accumulation ops."""
        trains = [f for f in fetches if _is_op(f, "TrainStep")]
        applies = [f for f in fetches if _is_op(f, "ApplyGradients")]
        accs = [f for f in fetches if _is_op(f, "AssignAdd")]
        if len(trains) + len(applies) + (1 if accs else 0) > 1:
            raise NotImplementedError("one train / apply_gradients / accumulate group per run call")
        if trains:
            a = trains[0].attrs
            return _TrainSpec(trains[0].inputs[0], a["optimizer"], a["var_list"], a["grad_scale"],
                              a.get("global_step"), [], [trains[0]])
        if applies:
            op = applies[0]
            loss, scales, vars_ = None, set(), []
            for g, v in op.attrs["pairs"]:
                lss, var, sc = _gradient_source(g)
                if var is not v:
                    raise NotImplementedError("apply_gradients: gradient paired with a different variable")
                if loss is not None and lss is not loss:
                    raise NotImplementedError("apply_gradients: gradients of different losses")
                loss = lss
                scales.add(sc)
                vars_.append(v)
            if len(scales) != 1:
                raise NotImplementedError("apply_gradients: one gradient scale for all variables")
            return _TrainSpec(loss, op.attrs["optimizer"], vars_, scales.pop(), op.attrs.get("global_step"),
                              [], [op])
        if accs:
            loss, vars_, acc = None, [], []
            for op in accs:
                lss, var, sc = _gradient_source(op.attrs["value"])
                if loss is not None and lss is not loss:
                    raise NotImplementedError("assign_add: gradients of different losses")
                loss = lss
                if op.attrs["var"].trainable:
                    raise NotImplementedError("assign_add target must be a non-trainable accumulator")
                if tuple(op.attrs["var"].shape) != tuple(var.shape):
                    raise ValueError(f"{op.attrs['var'].var_name}: accumulator shape != {var.var_name}")
                vars_.append(var)
                acc.append((op.attrs["var"].var_name, var.var_name, sc))
            return _TrainSpec(loss, None, vars_, 1.0, None, acc, accs)
        return None

    # --------------------------------------------------------------- compile
    def _compile(self, fetches, feed_dict):
        g = self.graph
        p = Plan()
        p.fetches = fetches
        p.train = self._train_spec(fetches)
        train_ops = {id(o) for o in p.train.ops} if p.train else set()
        stray = [f for f in fetches if isinstance(f, G.Op) and id(f) not in train_ops]
        if stray:
            raise NotImplementedError(f"cannot fetch {stray[0]!r} here")
        roots = [f for f in fetches if not isinstance(f, G.Op)]
        if p.train:
            roots.append(p.train.inputs[0])

        # ---- needed ops (ancestors of the fetches), topological = creation order
        needed = set()
        stack = [t.op for t in roots]
        while stack:
            op = stack.pop()
            if op.id in needed:
                continue
            needed.add(op.id)
            stack.extend(t.op for t in op.inputs)
        order = [op for op in g.ops if op.id in needed]
        consumers = {}
        for op in order:
            for t in op.inputs:
                consumers.setdefault(id(t), []).append(op)
        fetched = {id(t) for t in roots}

        # ---- concrete shapes
        shp = {}
        feeds = {id(k): v for k, v in feed_dict.items()}
        for op in order:
            y = op.outputs[0]
            if op.type == "Placeholder":
                if id(y) not in feeds:
                    raise ValueError(f"placeholder {op.name} must be fed")
                shp[id(y)] = tuple(np.shape(feeds[id(y)]))
            elif op.type == "VariableV2":
                shp[id(y)] = tuple(y.shape)
            else:
                shp[id(y)] = self._infer(op, shp)
        p.shapes = shp

        # ---- which tensors need gradients (depend on a trainable variable)
        needs_grad = set()
        if p.train:
            var_ids = {id(v) for v in p.train.attrs["var_list"]}
            for op in order:
                if op.type == "VariableV2" and id(op.outputs[0]) in var_ids:
                    needs_grad.add(id(op.outputs[0]))
                elif any(id(t) in needs_grad for t in op.inputs):
                    needs_grad.add(id(op.outputs[0]))
        p.needs_grad = needs_grad

        nodes = self._fuse_nodes(order, consumers, fetched, shp, p.train.inputs[0] if p.train else None)
        p.nodes = self._lower_strided_1x1(p, nodes, _Node)
        p.fetched = fetched
        self._fold_bn_prologues(p, fetched)
        self._fold_dropout_grads(p, fetched)
        self._allocate(p, consumers, feeds)
        return p

    _FILM = "only relu?((x + number) * f + beta) is on the hot path (TransNet's modulation): AddScalar -> " \
            "multiply of two same-shape maps -> Add [-> Relu], each link with one consumer"
    _AXPY = "number * tensor is on the hot path only as relu?(x + number * c) (TransNet's fusion), as a weight " \
            "of a loss term, or as tf.scalar_mul on a gradient"
    _LOSS = "reduce_mean is only supported on the xent loss: softmax_cross_entropy_with_logits, or a sum of " \
            "such terms each optionally times a Python number"

    def _loss_heads(self, order, consumers, fetched):
        """Every Mean of the plan as a loss: mean op id -> [(SoftmaxXent op,
        weight)], and the ids of the Add / ScalarMul ops between them
        (Mean(xent + 0.4 * xent + 1.6 * xent), FCDenseNet_TransNet.py:268-271;
        the sum may be nested Adds, the weights are Python numbers)."""
        heads, inner = {}, set()

        def walk(t, w, terms):
            if id(t) in fetched or len(consumers.get(id(t), [])) != 1:
                raise NotImplementedError(self._LOSS)
            op = t.op
            if op.type == "SoftmaxXent":
                terms.append((op, w))
            elif op.type == "Add":
                inner.add(op.id)
                walk(op.inputs[0], w, terms)
                walk(op.inputs[1], w, terms)
            elif op.type == "ScalarMul" and not isinstance(op.attrs["scalar"], G.Tensor):
                inner.add(op.id)
                walk(op.attrs["x"], w * float(op.attrs["scalar"]), terms)
            else:
                raise NotImplementedError(self._LOSS)

        for op in order:
            if op.type == "Mean":
                terms = []
                walk(op.inputs[0], 1.0, terms)
                heads[op.id] = terms
        return heads, inner

    def _fuse_nodes(self, order, consumers, fetched, shp, train_loss=None):
        """Fusion of single-consumer op chains into nodes (one launch each)."""
        def single_consumer(t, type_):
            cs = consumers.get(id(t), [])
            if len(cs) == 1 and cs[0].type == type_ and id(t) not in fetched:
                return cs[0]
            return None

        def absorb(chain, type_):
            """Append the chain output's only consumer when it is a `type_` op
            reading it as its first input; that op, or None."""
            cur = chain[-1].outputs[0]
            nxt = single_consumer(cur, type_)
            if nxt is None or nxt.inputs[0] is not cur:
                return None
            chain.append(nxt)
            absorbed.add(nxt.id)
            return nxt

        def sole_input(t, type_):
            """t's producing op when it is a `type_` op read by nothing else."""
            if t.op.type == type_ and len(consumers.get(id(t), [])) == 1 and id(t) not in fetched:
                return t.op
            return None

        def elementwise_chain(add):
            """Add as the tail of a film or an axpy chain: (kind, inputs, attrs,
            the ops before it) or None for a plain tf.add."""
            for i in (0, 1):
                m, other = sole_input(add.inputs[i], "MulFull"), add.inputs[1 - i]
                if m is not None:
                    for j in (0, 1):
                        a = sole_input(m.inputs[j], "AddScalar")
                        if a is not None:
                            return ("film", [a.inputs[0], m.inputs[1 - j], other],
                                    {"alpha_bias": a.attrs["scalar"]}, [a, m])
                sm = sole_input(add.inputs[i], "ScalarMul")
                if sm is not None and not isinstance(sm.attrs["scalar"], G.Tensor):
                    return ("axpy", [other, sm.attrs["x"]], {"lam": float(sm.attrs["scalar"])}, [sm])
            return None

        heads, absorbed = self._loss_heads(order, consumers, fetched)
        xent_of = {x.id: (order_mean, w) for order_mean, terms in heads.items() for x, w in terms}
        multi = {}           # mean op id -> its xent nodes (a loss that is not the bare SoftmaxXent -> Mean)
        chained = set()      # AddScalar / MulFull / ScalarMul ops that a film / axpy node took in
        nodes = []
        for op in order:
            if op.id in absorbed or op.type in ("VariableV2",):
                continue
            t = op.type
            y = op.outputs[0]
            if t == "Conv2D":
                x, w = op.inputs
                chain = [op]
                b = absorb(chain, "BiasAdd")
                relu = absorb(chain, "Relu") is not None
                # Conv [+BiasAdd] [+Relu] + Dropout: applied in the epilogue (without
                # a ReLU the gradient re-draws the mask: seg_dropout_bwd_ch)
                d = absorb(chain, "Dropout") if (relu or self.fuse_dropout) else None
                nodes.append(_Node("conv", chain, [x], chain[-1].outputs[0], w=w,
                                   bias=b.inputs[1] if b is not None else None, relu=relu,
                                   kp=d.attrs["keep_prob"] if d is not None else None,
                                   stride=op.attrs["stride"], dilation=op.attrs["dilation"],
                                   dilation_hw=op.attrs["dilation_hw"], padding=op.attrs["padding"]))
            elif t == "Conv2DTranspose":
                x, w = op.inputs
                chain = [op]
                b = absorb(chain, "BiasAdd")
                res = None
                cur = chain[-1].outputs[0]
                nxt = single_consumer(cur, "Add")
                if nxt is not None:
                    a0, a1 = nxt.inputs
                    other = a1 if a0 is cur else a0
                    if shp[id(other)] == shp[id(nxt.outputs[0])] and other is not cur:
                        res = other
                        chain.append(nxt)
                        absorbed.add(nxt.id)
                nodes.append(_Node("tconv", chain, [x], chain[-1].outputs[0], w=w,
                                   bias=b.inputs[1] if b is not None else None, residual=res,
                                   stride=op.attrs["stride"], padding=op.attrs["padding"],
                                   output_shape=op.attrs["output_shape"]))
            elif t == "DepthwiseConv2D":
                # a kind of its own: the BN / ReLU around it stay standalone nodes
                x, w = op.inputs
                nodes.append(_Node("dwconv", [op], [x], y, w=w, stride=op.attrs["stride"], rate=op.attrs["rate"],
                                   padding=op.attrs["padding"]))
            elif t == "FusedBatchNorm":
                x, gamma, beta = op.inputs
                chain = [op]
                relu = absorb(chain, "Relu") is not None
                # BatchNorm -> swish (MBConvBlock): one seg_bn_act launch, outside the ReLU BN's fusions
                act = "swish" if not relu and absorb(chain, "Swish") is not None else None
                nodes.append(_Node("bn", chain, [x], chain[-1].outputs[0], gamma=gamma, beta=beta, relu=relu,
                                   eps=op.attrs["epsilon"], act=act))
            elif t in ("Swish", "Sigmoid"):
                nodes.append(_Node("act", [op], [op.inputs[0]], y, act=t.lower()))
            elif t == "Mul":
                nodes.append(_Node("se_excite", [op], list(op.inputs), y))
            elif t == "SoftmaxXent":
                logits, labels = op.inputs
                if op.id not in xent_of:
                    raise NotImplementedError("softmax_cross_entropy_with_logits must feed reduce_mean")
                mid, w = xent_of[op.id]
                mean = next(o for o in order if o.id == mid)
                in_loss = train_loss is None or mean.outputs[0] is train_loss
                if len(heads[mid]) == 1 and mean.inputs[0] is y:
                    absorbed.add(mean.id)
                    nodes.append(_Node("xent", [op, mean], [logits], mean.outputs[0], labels=labels,
                                       valid_hw=op.attrs["valid_hw"], in_loss=in_loss))
                else:
                    # a head of a weighted sum: its own launch; the Mean becomes the xent_sum node
                    nodes.append(_Node("xent", [op], [logits], y, labels=labels, valid_hw=op.attrs["valid_hw"],
                                       weight=w, in_loss=in_loss))
                    multi.setdefault(mid, []).append(nodes[-1])
            elif t == "Mean":
                hs = multi[op.id]
                ref = hs[0]
                for h in hs[1:]:
                    if (tuple(shp[id(h.inputs[0])][:3]) != tuple(shp[id(ref.inputs[0])][:3])
                            or h.valid_hw != ref.valid_hw):
                        raise ValueError(f"{op.name}: the heads of a weighted loss must share N, H, W and valid_hw")
                nodes.append(_Node("xent_sum", [op], [], y, heads=hs))
            elif t in ("AddScalar", "MulFull"):
                # taken in by the Add at the end of their chain (below), or not supported
                nxt = single_consumer(y, "MulFull" if t == "AddScalar" else "Add")
                if nxt is None or (t == "MulFull" and (elementwise_chain(nxt) or ("",))[0] != "film"):
                    raise NotImplementedError(f"{op.name}: {self._FILM}")
                if t == "AddScalar" and single_consumer(nxt.outputs[0], "Add") is None:
                    raise NotImplementedError(f"{op.name}: {self._FILM}")
            elif t == "ScalarMul":
                nxt = single_consumer(y, "Add")
                if isinstance(op.attrs["scalar"], G.Tensor) or nxt is None:
                    raise NotImplementedError(f"{op.name}: {self._AXPY}")
            elif t == "Add" and elementwise_chain(op) is not None:
                kind, ins, attrs, before = elementwise_chain(op)
                for i in ins:
                    if i.op.type in ("AddScalar", "MulFull", "ScalarMul"):
                        raise NotImplementedError(f"{op.name}: {self._FILM if kind == 'film' else self._AXPY}")
                chain = before + [op]
                chained.update(o.id for o in before)
                relu = absorb(chain, "Relu") is not None
                nodes.append(_Node(kind, chain, ins, chain[-1].outputs[0], relu=relu, **attrs))
            elif t == "Placeholder":
                nodes.append(_Node("input", [op], [], y))
            elif t in ("MaxPool", "AvgPool", "Pool2D", "Pad", "Add", "Relu", "Dropout", "BiasAdd", "ConcatV2",
                       "ResizeBilinear", "ArgMax", "ExpandDims", "Softmax", "GlobalAvgPool"):
                nodes.append(_Node(t, [op], list(op.inputs), y))
            else:
                raise NotImplementedError(f"op {t} is not on the hot path")
        for op in order:
            if op.type in ("AddScalar", "MulFull", "ScalarMul") and op.id not in absorbed and op.id not in chained:
                raise NotImplementedError(f"{op.name}: {self._FILM if op.type != 'ScalarMul' else self._AXPY}")
        return nodes

    @property
    def _dpa(self):
        """The DataParallel whose collectives run (None: single process, or
        world 1 where every collective is the identity)."""
        return self.dp if (self.dp is not None and self.dp.active) else None

    def side_stream(self):
        """The side stream of this Session's device (side_stream_for)."""
        if self._side is None:
            self._side = side_stream_for(self.device)
        return self._side

    def sync_optimizer_slots(self):
        """After ZeRO-1 steps each rank's Adam m / v are current on its own
        slices only: gather them (checkpoints, tests)."""
        if self._dpa is not None and self.store is not None and self.dp.store is self.store:
            self.dp.gather_slots()

    def _zero_update(self, p, opt, gs):
        """ZeRO-1 (dp.py): TF1 Adam on this rank's reduce-scattered slices of
        the variables being trained, the updated fp32 slices all-gathered in
        place, then every packed compute copy rewritten from the full
        parameters in one launch (seg_pack_segments)."""
        store = self.store
        key = ("zero", tuple(p.adam_names), len(store.packed))
        ranges = self._adam_groups.get(key)
        if ranges is None:
            spans = sorted((store.offset[nm], store.offset[nm] + int(np.prod(store.by_name[nm].shape)))
                           for nm in p.adam_names)
            starts = sorted(store.offset.values())
            ranges = []
            for a, b in self.dp.owned_ranges():
                for s0, e0 in spans:
                    lo, hi = max(a, s0), min(b, e0)
                    if lo >= hi:
                        continue
                    # merge over a gap that is only 16-byte alignment padding
                    # (zeros, which Adam leaves zero) -- never over a variable
                    # outside var_list
                    if ranges and lo - ranges[-1][1] <= 3 and not any(ranges[-1][1] <= o < lo for o in starts):
                        ranges[-1] = (ranges[-1][0], hi)
                    else:
                        ranges.append((lo, hi))
            self._adam_groups[key] = ranges
        for a, b in ranges:
            ops.adam_tf1_step(store.params[a:b], store.grads[a:b], store.m[a:b], store.v[a:b], opt.lr, store.step,
                              opt.beta1, opt.beta2, opt.epsilon, grad_scale=gs)
        self.dp.gather_params()
        ops.pack_segments(store.params, self._adam_plan(p.adam_names), dtype=self._pack_dtype())

    # -------------------------------------------------------------- execute
    def _repack(self, p):
        store = self.store
        if self._packed_version == store.version:
            return
        for (name, mode), (t, ap, bp) in store.packed.items():
            ops.pack_filter(store.param(name), t, ap, bp, mode)
        self._packed_version = store.version

    def _adam_plan(self, names=None):
        """Segment table of the fused Adam + pack launch: every variable of the
        store (or the subset `names`), with the packed copies that exist
        (rebuilt when packs are added)."""
        store = self.store
        key = (len(store.packed), store.numel)
        if names is not None:
            gk = (key, tuple(names))
            plan = self._adam_groups.get(gk)
            if plan is None:
                plan = ops.AdamPlan(self._adam_segments(set(names)), self.device)
                self._adam_groups[gk] = plan
            return plan
        if self._adam_key == key:
            return self._adam
        self._adam = ops.AdamPlan(self._adam_segments(None), self.device)
        self._adam_key = key
        return self._adam

    def _adam_segments(self, subset):
        store = self.store
        segs = []
        for v in store.order:
            if subset is not None and v.var_name not in subset:
                continue
            shape = tuple(v.shape)
            n = int(np.prod(shape))
            if len(shape) == 4:
                rs, a, b = shape[0] * shape[1], shape[2], shape[3]
            else:
                rs, a, b = 1, 1, n
            rows = tr = None
            for mode in (ops.PACK_KRSC, ops.PACK_HWIO, ops.PACK_TCONV_FWD, ops.PACK_TCONV_BWD):
                e = store.packed.get((v.var_name, mode))
                if e is None:
                    continue
                if mode in (ops.PACK_HWIO, ops.PACK_TCONV_FWD):
                    rows = e
                else:
                    tr = e
            segs.append((store.offset[v.var_name], rs, a, b, rows, tr))
        return segs

    def _pack(self, n, mode):
        """The packed compute copy (layout `mode`) of conv / tconv node n's filter."""
        return self.store.packed[(n.w.var_name, mode)][0]

    def _execute(self, p, feed_dict):
        self.run_count += 1
        # packed filter copies are current from here on; every update below
        # (fused filter-gradient + Adam, adam_tf1_pack) rewrites the copies of
        # the variables it changes, so they stay current after the step
        self._repack(p)
        self._check_bn_stats(p)
        scal = self._feed(p, feed_dict)
        step_seed = (self.seed * 1000003 + self.run_count * 7919) & 0xFFFFFFFF
        if self.dp is not None:
            step_seed ^= (self.dp.rank + 1) * _SEED_MIX
        self._forward(p, scal, step_seed)
        if p.train:
            self._train_step(p, scal)
        return self._fetch(p)

    def _train_step(self, p, scal):
        """Backward and optimizer: set-up, backward, loss-scale outcome, update."""
        store = self.store
        ts = p.train.attrs
        opt = ts["optimizer"]
        dpa = self._dpa
        world = dpa.world if dpa is not None else 1
        S = self.loss_scale                     # the scale this step's loss gradient carries
        scaled = S != 1.0
        gs = ts["grad_scale"] / world / S
        if scaled and self.overlap_optimizer:
            raise NotImplementedError("loss scaling needs the whole gradient checked before any update")
        if opt is not None:
            store.step += 1
        self._fused = None
        if opt is not None and self.fuse_adam and dpa is None and not self.overlap_optimizer \
                and not scaled and p.adam_fusable:
            self._fused = (opt, gs, set())
        # ZeRO-1 exchange for an Adam step (dp.py); the accumulate template
        # and the overlapped per-layer optimizer read whole gradients
        zero = (dpa is not None and dpa.shard and opt is not None and not self.overlap_optimizer
                and not p.train.accum)
        if dpa is not None:
            dpa.mode = "zero" if zero else "allreduce"
            if opt is not None and not zero and dpa.slots_stale:
                # a whole-variable Adam after ZeRO-1 steps: gather the m / v
                # slices of the other ranks first, or the replicas diverge
                self.sync_optimizer_slots()
        self._red = None
        if self.defer_wgrad_reduce and self.device.type == "cuda":
            # (with the overlapped optimizer the reductions and each layer's
            # Adam share the side stream: a layer's reduction precedes its update)
            self._red = (self.side_stream(), torch.cuda.current_stream(self.device))
            if dpa is not None:
                dpa.launch_streams = self._red
        if opt is not None and self.overlap_optimizer and self.device.type == "cuda":
            # per-layer Adam on a side stream as soon as the layer's gradient is final
            self._adam_ctx = _AdamOverlap(self, opt, gs, p.var_set)
            if dpa is not None:
                dpa.on_launch = self._adam_ctx.after_work
        elif (opt is not None and dpa is not None and not zero and self.overlap_big_mb and not scaled
              and not p.train.accum and self.device.type == "cuda"):
            self._adam_ctx = _AdamOverlap(self, opt, gs, p.var_set, big_only=True)
            dpa.on_launch = self._adam_ctx.after_work
        if dpa is not None and p.never_ready:
            dpa.ready(p.never_ready)
        self._ready_filter = p.var_set
        ok = False
        try:
            self._backward(p, scal)
            self._tick_fused(flush=True)
            ok = True
        finally:
            # on an exception: no stale fused conv6 / conv7 update is left
            # for the next step, and the compute stream does not run ahead
            # of side-stream kernels still reading this step's buffers
            self._ready_filter = None
            if not ok:
                self._pending_fused = []
                self._fused = None
                self._adam_ctx = None
            if self._red is not None:        # pending filter-gradient reductions done before Adam
                self._red[1].wait_stream(self._red[0])
                self._red = None
            if dpa is not None:
                if ok:
                    dpa.finish()
                else:
                    dpa.abort_step()
                dpa.on_launch = None
                dpa.launch_streams = None
        if scaled and not self._grads_finite():
            # overflow in the scaled fp16 gradients: no update this step
            # (TF LossScaleOptimizer), halve the scale
            self.skipped_steps += 1
            if opt is not None:
                store.step -= 1
            self.loss_scale = max(self.loss_scale / 2.0, 1.0)
            self.good_steps = 0
            opt = None
            p_accum = []
        else:
            p_accum = p.train.accum
            if scaled and self.dynamic_scale:
                self.good_steps += 1
                if self.good_steps >= self.scale_increment_period:
                    self.loss_scale *= 2.0
                    self.good_steps = 0
        if opt is None:
            # accumulate template: accum += const * grad (Network/main.py:92-95)
            for acc, var, sc in p_accum:
                ops.axpy(store.aux[acc].view(-1), store.grad(var).view(-1), sc / world / S)
            store.aux_version += 1
        elif self._adam_ctx is not None:
            self._adam_ctx.finish()
            self._adam_ctx = None
        elif zero:
            self._zero_update(p, opt, gs)
        else:
            done = self._fused[2] if self._fused is not None else set()
            rest = [nm for nm in p.adam_names if nm not in done]
            if rest:
                ops.adam_tf1_pack(store.params, store.grads, store.m, store.v, self._adam_plan(rest), opt.lr,
                                  store.step, opt.beta1, opt.beta2, opt.epsilon, grad_scale=gs,
                                  dtype=self._pack_dtype())
        self._fused = None
        if opt is not None:
            store.version += 1
            self._packed_version = store.version
            self._bump_global_step(ts.get("global_step"))

    def _fetch(self, p):
        out = {}
        for f in p.fetches:
            if isinstance(f, G.Op):
                out[id(f)] = None
                continue
            t = p.buf.get(id(f))
            node = next((n for n in p.nodes if n.output is f), None)
            if node is not None and node.kind in ("xent", "xent_sum"):
                out[id(f)] = (t / node.count).reshape(())
            elif f.dtype == G.int64:
                out[id(f)] = t
            else:
                C = p.shapes[id(f)][3]
                out[id(f)] = t[..., :C].float()
        return out

    def _pack_dtype(self):
        return self.cdt

    def _check_bn_stats(self, p):
        """The kernels fold BatchNorm's frozen statistics as mean 0 / variance
        1 (tf.layers.batch_normalization with training=False and never-updated
        moving averages, Network/utils/utils.py:300-301).  Refuse to run if a
        restore or assign changed them."""
        store = self.store
        if not store.aux_vars or getattr(self, "_bn_checked", None) == store.aux_version:
            return
        for v in store.aux_vars:
            kind = getattr(v, "bn_stat", None)
            if kind is None:
                continue
            t = store.aux[v.var_name]
            want = 0.0 if kind == "mean" else 1.0
            if not bool((t == want).all()):
                raise NotImplementedError(f"{v.var_name}: BatchNormalization moving statistics other than "
                                          f"the frozen (0, 1) of the reference are not on the hot path")
        self._bn_checked = store.aux_version

    def close(self):
        self.plans = {}

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
