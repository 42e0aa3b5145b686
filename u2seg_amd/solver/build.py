"""Optimizer and LR schedule (detectron2/solver/build.py:29-323, solver/lr_scheduler.py:22-138).

All trainable tensors live in one flat fp32 arena (parameters, gradients and momentum are views), so that
 * data-parallel gradient exchange is a handful of large RCCL all-reduces over xGMI instead of 248 small ones,
 * per-parameter L2 clipping (CLIP_TYPE "norm", applied per tensor as in solver/build.py:36-37,63-73) + SGD with
   momentum and weight decay is two kernel launches (u2_sgd_clip_step).
The solver's other options - CLIP_TYPE value, NORM_TYPE 1 / inf, NESTEROV, BIAS_LR_FACTOR - go through u2_sgd_step_opts, the same
stream with the options as kernel arguments; the default configuration keeps the two launches of u2_sgd_clip_step."""
import bisect
import math

import torch
import torch.distributed as dist

from .. import _hip
from ..layers.modules import BatchNorm2d, GroupNorm

CHUNK = 1 << 16
CLIP_NONE, CLIP_VALUE, CLIP_L2, CLIP_L1, CLIP_INF = range(5)   # clip_mode of u2_sgd_step_opts (include/u2seg_hip.h)


def clip_mode_of(clip_type, norm_type, clip_value):
    """SOLVER.CLIP_GRADIENTS.{CLIP_TYPE, NORM_TYPE, CLIP_VALUE} -> clip_mode (solver/build.py:29-46).  A CLIP_VALUE of 0 is this
    package's "no clipping" (what build_optimizer hands over with CLIP_GRADIENTS.ENABLED False)."""
    if clip_type not in ("value", "norm"):
        raise ValueError("SOLVER.CLIP_GRADIENTS.CLIP_TYPE must be 'value' or 'norm', got %r" % (clip_type,))
    if float(clip_value) < 0:
        raise ValueError("SOLVER.CLIP_GRADIENTS.CLIP_VALUE must not be negative, got %r" % (clip_value,))
    if float(clip_value) == 0:
        return CLIP_NONE
    if clip_type == "value":
        return CLIP_VALUE
    try:
        nt = float(norm_type)   # yaml writes the infinity norm as .inf or as the string "inf": float() reads both
    except (TypeError, ValueError):
        nt = None
    mode = {1.0: CLIP_L1, 2.0: CLIP_L2, math.inf: CLIP_INF}.get(nt)
    if mode is None:
        raise ValueError("SOLVER.CLIP_GRADIENTS.NORM_TYPE must be 1, 2 or inf, got %r: a general p-norm needs powf per element and "
                         "has no derived error bound here" % (norm_type,))
    return mode


class FlatSGD:
    def __init__(self, model, lr, momentum=0.9, weight_decay=0.0, weight_decay_norm=0.0, weight_decay_bias=None,
                 clip_value=0.0, bucket_bytes=64 << 20, nesterov=False, clip_type="norm", norm_type=2.0, bias_lr_factor=1.0):
        if nesterov and momentum <= 0:
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")   # torch.optim.SGD's own words
        self.nesterov = bool(nesterov)
        self.clip_mode = clip_mode_of(clip_type, norm_type, clip_value)
        # the bias override carries the learning rate too (solver/build.py:187-199): BASE_LR * BIAS_LR_FACTOR, in doubles, for
        # every parameter literally named "bias" - a normalisation layer's included
        self.has_bias_lr = bias_lr_factor is not None and float(bias_lr_factor) != 1.0
        self.initial_lr_bias = lr * bias_lr_factor if self.has_bias_lr else lr
        self.lr_bias = self.initial_lr_bias
        # per-parameter hyper-parameters by the reference's rule (solver/build.py:218-236 get_default_optimizer_params): the
        # module tree is walked in named_modules order, a normalisation layer's parameters take WEIGHT_DECAY_NORM, and the
        # legacy bias override - applied after it, to every parameter literally named "bias" - WEIGHT_DECAY_BIAS
        # `key_of` is the reference's grouping key: its per-parameter dict starts as {"lr": base_lr} - build_optimizer never
        # hands weight_decay to get_default_optimizer_params (solver/build.py:123-129), torch fills it in from the SGD default -
        # and gains a "weight_decay" entry only where an override applied.  So a parameter without override (key None) and one
        # whose override EQUALS the default still sit in different groups, and all overridden parameters of one value share one.
        # With BIAS_LR_FACTOR != 1 the dict's "lr" differs too, so the key is (lr, weight-decay override or None).
        wd_of, key_of, bias_of, seen = {}, {}, {}, set()
        for mod in model.modules():
            for pname, p in mod.named_parameters(recurse=False):
                if not p.requires_grad or id(p) in seen:
                    continue
                seen.add(id(p))
                key = None
                if isinstance(mod, (BatchNorm2d, GroupNorm)) and weight_decay_norm is not None:
                    key = float(weight_decay_norm)
                if pname == "bias" and weight_decay_bias is not None:
                    key = float(weight_decay_bias)
                bias_of[id(p)] = int(self.has_bias_lr and pname == "bias")
                key_of[id(p)] = (self.initial_lr_bias if bias_of[id(p)] else lr, key)
                wd_of[id(p)] = float(weight_decay) if key is None else key
        self.params = [p for p in model.parameters() if p.requires_grad]
        assert len(self.params) == len(wd_of)
        # the reference merges parameters with equal hyper-parameter dicts into one torch param group, groups in order of first
        # appearance (reduce_param_groups, solver/build.py:255-279); torch numbers the parameters group after group.  That
        # numbering is the key of a reference checkpoint's optimizer state (state_dict / load_state_dict below).
        group_keys = list(dict.fromkeys(key_of[id(p)] for p in self.params))
        self.group_wd = [float(weight_decay) if k is None else k for _, k in group_keys]
        self.group_members = [[i for i, p in enumerate(self.params) if key_of[id(p)] == k] for k in group_keys]
        # 1: the group's rate is lr_bias.  (A group never mixes the two: its key holds the rate.  With a base rate of 0 both
        # rates are 0 and the reference merges them; the class of the first member then serves all.)
        self.group_lr_class = [bias_of[id(self.params[m[0]])] for m in self.group_members]
        dev = self.params[0].device
        total = sum(p.numel() for p in self.params)
        self.total = total
        self.flat_param = torch.empty(total, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_mom = torch.zeros(total, dtype=torch.float32, device=dev)
        chunk_tensor, chunk_begin, chunk_len, wds, first_chunk = [], [], [], [], []
        off = 0
        for t, (name_p) in enumerate(self.params):
            p = name_p
            n = p.numel()
            self.flat_param[off : off + n].copy_(p.data.reshape(-1))
            p.data = self.flat_param[off : off + n].view(p.shape)
            p.grad = self.flat_grad[off : off + n].view(p.shape)
            p._u2_grad = p.grad  # layers/weights.py:grad_slot - kernels accumulate into the arena directly
            wds.append(wd_of[id(p)])
            first_chunk.append(len(chunk_tensor))
            for s in range(0, n, CHUNK):
                chunk_tensor.append(t)
                chunk_begin.append(off + s)
                chunk_len.append(min(CHUNK, n - s))
            off += n
        self.chunk_tensor = torch.tensor(chunk_tensor, dtype=torch.int32, device=dev)
        self.chunk_begin = torch.tensor(chunk_begin, dtype=torch.int64, device=dev)
        self.chunk_len = torch.tensor(chunk_len, dtype=torch.int32, device=dev)
        self.wd = torch.tensor(wds, dtype=torch.float32, device=dev)
        self.lr_class = torch.tensor([bias_of[id(p)] for p in self.params], dtype=torch.int32, device=dev)
        first_chunk.append(len(chunk_tensor))
        self.first_chunk = torch.tensor(first_chunk, dtype=torch.int32, device=dev)
        self.partial = torch.zeros(len(chunk_tensor), dtype=torch.float32, device=dev)
        self.lr, self.momentum, self.clip_value = lr, momentum, clip_value
        self.base_lr = lr  # "initial_lr" of the param groups once a torch LR scheduler has touched them
        self.param_offset = []
        off = 0
        for p in self.params:
            self.param_offset.append(off)
            off += p.numel()
        self.bucket_elems = bucket_bytes // 4
        self._pending, self._tail_from = [], None
        self._exchange_stream, self._step_stream = None, None
        # bf16 kernel layouts cached on the parameters (layers/weights.py:_weight_layout): [stamp] is shared with every
        # parameter; step() bumps it and rewrites all registered layouts with one launch.
        self._stamp = [0]
        self._layout_entries = []  # (param, key, entry)
        self._layout_table = None
        self._layout_table_len = -1
        for p in self.params:
            p._u2_stamp = self._stamp
            p._u2_layout_register = self._register_layout
            p.__dict__.pop("_u2_layouts", None)
            p.__dict__.pop("_u2_bias_rounded", None)

    def offset_of(self, param):
        """Element offset of a parameter inside the flat arena."""
        return (param.data_ptr() - self.flat_param.data_ptr()) // 4

    def zero_grad(self):
        from ..layers.functional import reset_deferred_gradients

        reset_deferred_gradients()   # a backward pass that raised midway must not leave deferred gradients behind
        if self.flat_grad.is_cuda:
            self._step_stream = torch.cuda.current_stream(self.flat_grad.device)  # the stream the training step is issued on
        self.flat_grad.zero_()

    def _distributed(self):
        return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1

    def _launch_all_reduce(self, lo, hi):
        """Async all-reduce of flat_grad[lo:hi] in buckets.  On the GPU the collectives are issued from a stream of their own
        that first waits - explicitly, event by event - for every stream that produced gradients: the stream the step runs on,
        the weight-gradient side stream and the branch streams.  ProcessGroupNCCL orders a collective behind whatever stream is
        current when it is called; the tail exchange is called from an autograd hook, where "current" is whichever stream the
        engine selected for that node, so nothing here depends on it."""
        if not self.flat_grad.is_cuda:
            for s in range(lo, hi, self.bucket_elems):
                self._pending.append(dist.all_reduce(self.flat_grad[s : min(s + self.bucket_elems, hi)], async_op=True))
            return
        from ..layers.functional import producer_streams

        dev = self.flat_grad.device
        if self._exchange_stream is None:
            self._exchange_stream = torch.cuda.Stream(device=dev)
        ex = self._exchange_stream
        producers = producer_streams(dev) + [torch.cuda.current_stream(dev)]
        if self._step_stream is not None:
            producers.append(self._step_stream)
        for st in producers:
            ev = torch.cuda.Event()
            ev.record(st)
            ex.wait_event(ev)
        with torch.cuda.stream(ex):
            for s in range(lo, hi, self.bucket_elems):
                self._pending.append(dist.all_reduce(self.flat_grad[s : min(s + self.bucket_elems, hi)], async_op=True))

    def begin_all_reduce_tail(self, first_elem):
        """Start summing the gradients of the arena's tail [first_elem, total) while backward is still running: the tail
        holds the head parameters (RPN, ROI heads, semantic head), which are final once the gradients of the FPN outputs
        exist; RCCL works on them over xGMI while the backbone backward (~40 % of the step) keeps the CUs busy."""
        if not self._distributed() or self._tail_from is not None:
            return
        self._tail_from = int(first_elem)  # (_launch_all_reduce waits for the producing streams itself)
        self._launch_all_reduce(self._tail_from, self.total)

    def all_reduce_grads(self):
        """Sum gradients over ranks in a few large buckets (mean is folded into the step's grad_scale)."""
        if not self._distributed():
            return 1.0
        self._launch_all_reduce(0, self.total if self._tail_from is None else self._tail_from)
        for h in self._pending:
            h.wait()  # the current stream (the optimizer's) waits for the collective; the host does not block on NCCL
        self._pending, self._tail_from = [], None
        return 1.0 / dist.get_world_size()

    def step(self, grad_scale=1.0):
        from ..layers.functional import join_all_streams

        join_all_streams()
        if not self.nesterov and not self.has_bias_lr and self.clip_mode in (CLIP_NONE, CLIP_L2):
            # every option at its default (clip_value 0 = no clipping): the two launches the shipped configs have always run
            _hip.call("u2_sgd_clip_step", self.flat_param, self.flat_grad, self.flat_mom, self.chunk_tensor, self.chunk_begin,
                      self.chunk_len, self.chunk_tensor.numel(), self.partial, self.first_chunk, self.wd, float(self.lr),
                      float(self.momentum), float(self.clip_value), float(grad_scale))
        else:
            _hip.call("u2_sgd_step_opts", self.flat_param, self.flat_grad, self.flat_mom, self.chunk_tensor, self.chunk_begin,
                      self.chunk_len, self.chunk_tensor.numel(), self.partial, self.first_chunk, self.wd, self.lr_class,
                      float(self.lr), float(self.lr_bias), float(self.momentum), int(self.nesterov), self.clip_mode,
                      float(self.clip_value), float(grad_scale))
        self.refresh_layouts()

    def _register_layout(self, param, key, entry):
        self._layout_entries.append((param, key, entry))

    def refresh_layouts(self):
        """The parameters changed under the kernels' feet: new stamp, then rewrite every cached layout in one launch."""
        self._stamp[0] += 1
        ents = self._layout_entries
        if not ents:
            return
        if self._layout_table_len != len(ents):
            import numpy as np

            desc = np.zeros(len(ents), dtype=np.dtype([("src", "<i8"), ("dst", "<u8"), ("N", "<i4"), ("Cin", "<i4"), ("T", "<i4"),
                                                       ("Cp", "<i4"), ("Npad", "<i4"), ("mode", "<i4"), ("blk", "<i4"),
                                                       ("rsv", "<i4")], align=True))
            assert desc.dtype.itemsize == 48
            base = self.flat_param.data_ptr()
            blocks = 0
            for i, (p, key, ent) in enumerate(ents):
                off = p.data_ptr() - base
                assert 0 <= off < self.total * 4 and off % 4 == 0
                desc[i] = (off // 4, ent[0].data_ptr()) + tuple(key) + (blocks, 0)
                n_, cin_, t_, cp_, npad_, mode_ = key
                if mode_ == 3:
                    blocks += (n_ + 4095) // 4096             # a bias vector rounded through bf16, fp32 out
                elif mode_ == 0 and t_ == 1 and cp_ == cin_:
                    blocks += (n_ * cp_ + 4095) // 4096  # plain conversion (u2_weight_layout_batched: the same rule)
                elif mode_ == 0:
                    blocks += n_ * ((cp_ + 63) // 64)
                else:
                    blocks += ((npad_ + 63) // 64) * ((cin_ * t_ + 63) // 64)
            self._layout_table = torch.from_numpy(desc.view(np.uint8).copy()).to(self.flat_param.device)
            self._layout_table_len = len(ents)
            self._layout_blocks = blocks
        _hip.call("u2_weight_layout_batched", self.flat_param, self._layout_table, len(ents), self._layout_blocks)
        stamp = self._stamp[0]
        for p, _, ent in ents:
            ent[1], ent[2] = p._version, stamp

    def state_dict(self):
        """The state dict `torch.optim.SGD` - the reference's optimizer (solver/build.py:119-139) - would write for this
        model: `param_groups` in the reference's grouping with torch's parameter numbering, `state[i]["momentum_buffer"]` a
        copy of parameter i's slice of the momentum arena.  A reference trainer can resume from it, and `load_state_dict`
        reads what a reference trainer wrote.  (Before the first step torch has no state entries; here the buffers exist
        from the start and are written as zeros, which is what torch's first step computes from: buf = grad.)"""
        groups, state, n = [], {}, 0
        for wd, members, cls in zip(self.group_wd, self.group_members, self.group_lr_class):
            groups.append({"lr": float(self.lr_bias if cls else self.lr), "momentum": float(self.momentum), "dampening": 0,
                           "weight_decay": wd, "nesterov": self.nesterov, "maximize": False, "foreach": True,
                           "differentiable": False, "fused": None,
                           "initial_lr": float(self.initial_lr_bias if cls else self.base_lr),
                           "params": list(range(n, n + len(members)))})
            for i in members:
                off = self.param_offset[i]
                p = self.params[i]
                state[n] = {"momentum_buffer": self.flat_mom[off : off + p.numel()].view(p.shape).clone()}
                n += 1
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        if "param_groups" not in sd:  # this package's first on-disk form: the whole momentum arena + lr
            self.flat_mom.copy_(sd["momentum"])
            self.lr = sd["lr"]
            return
        groups = sd["param_groups"]
        if [len(g["params"]) for g in groups] != [len(m) for m in self.group_members]:
            raise ValueError("loaded state dict has a different number of parameter groups / parameters per group: %s vs %s"
                             % ([len(g["params"]) for g in groups], [len(m) for m in self.group_members]))
        # groups are matched by position; the kernel knows two rates, the base class's and the bias class's (BIAS_LR_FACTOR)
        def rate_of(key, cls):
            found = {}
            for gi, g in enumerate(groups):
                if self.group_lr_class[gi] == cls:
                    found.setdefault(float(g[key]), []).append(gi)
            if len(found) > 1:
                raise ValueError("param_groups %s hold different '%s' values %s within the %s class: this optimizer steps with two "
                                 "rates, SOLVER.BASE_LR and SOLVER.BASE_LR * SOLVER.BIAS_LR_FACTOR%s"
                                 % (sorted(found.values()), key, sorted(found), "bias" if cls else "base",
                                    "" if self.has_bias_lr else " (built with BIAS_LR_FACTOR 1: one rate)"))
            return next(iter(found), None)

        flags = {(bool(g.get("nesterov", False)), float(g.get("momentum", self.momentum))) for g in groups}
        if len(flags) > 1:
            raise ValueError("param_groups differ in 'nesterov' / 'momentum' %s: SOLVER.NESTEROV and SOLVER.MOMENTUM hold for all"
                             % sorted(flags))
        for gi, g in enumerate(groups):
            for key in ("dampening", "maximize"):
                if g.get(key, 0):
                    raise ValueError("param_groups[%d]['%s'] = %r: not implemented (the reference's build_optimizer never sets it)"
                                     % (gi, key, g[key]))
        nesterov, momentum = flags.pop()
        if nesterov and momentum <= 0:
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        lr, lr_bias = rate_of("lr", 0), rate_of("lr", 1)
        self.nesterov = nesterov
        self.lr = self.lr if lr is None else lr
        self.lr_bias = self.lr if not self.has_bias_lr else (self.lr_bias if lr_bias is None else lr_bias)
        if all("initial_lr" in g for g in groups):  # written once a torch LR scheduler has touched the optimizer
            base, base_bias = rate_of("initial_lr", 0), rate_of("initial_lr", 1)
            self.base_lr = self.base_lr if base is None else base
            self.initial_lr_bias = self.base_lr if not self.has_bias_lr else (self.initial_lr_bias if base_bias is None else base_bias)
        for gi, (g, members) in enumerate(zip(groups, self.group_members)):
            self.momentum = float(g.get("momentum", self.momentum))
            wd = float(g.get("weight_decay", self.group_wd[gi]))
            if wd != self.group_wd[gi]:
                # torch takes a group's hyper-parameters from the file, not from the constructor (Optimizer.load_state_dict);
                # groups are addressed by position: two groups may hold equal values
                self.group_wd[gi] = wd
                self.wd[torch.tensor(members, device=self.wd.device)] = wd
            for key, i in zip(g["params"], members):
                off, p = self.param_offset[i], self.params[i]
                buf = (sd["state"].get(key) or {}).get("momentum_buffer")
                dst = self.flat_mom[off : off + p.numel()]
                if buf is None:  # torch creates the buffer in the first step: no entry = no history
                    dst.zero_()
                    continue
                if tuple(buf.shape) != tuple(p.shape):
                    raise ValueError("momentum buffer %s of parameter %d does not fit %s" % (tuple(buf.shape), key, tuple(p.shape)))
                dst.copy_(buf.reshape(-1))


def build_optimizer(cfg, model):
    s = cfg.SOLVER
    clip = 0.0
    if s.CLIP_GRADIENTS.ENABLED:
        clip = float(s.CLIP_GRADIENTS.CLIP_VALUE)
        if clip <= 0:
            raise ValueError("SOLVER.CLIP_GRADIENTS.CLIP_VALUE must be positive with CLIP_GRADIENTS.ENABLED, got %r" % (clip,))
    return FlatSGD(model, lr=s.BASE_LR, momentum=s.MOMENTUM, weight_decay=s.WEIGHT_DECAY,
                   weight_decay_norm=s.WEIGHT_DECAY_NORM, weight_decay_bias=s.WEIGHT_DECAY_BIAS, clip_value=clip,
                   nesterov=s.NESTEROV, clip_type=s.CLIP_GRADIENTS.CLIP_TYPE, norm_type=s.CLIP_GRADIENTS.NORM_TYPE,
                   bias_lr_factor=s.BIAS_LR_FACTOR)


class WarmupMultiStepLR:
    """lr(iter) = base_lr * gamma^(#milestones passed) * warmup(iter) with linear warm-up from warmup_factor
    (solver/build.py:283-323 via fvcore's MultiStepParamScheduler + LinearParamScheduler composite)."""

    def __init__(self, optimizer, base_lr, milestones, gamma, warmup_factor, warmup_iters, warmup_method="linear"):
        assert warmup_method == "linear"
        self.optimizer, self.base_lr = optimizer, base_lr
        self.milestones, self.gamma = sorted(milestones), gamma
        self.warmup_factor, self.warmup_iters = warmup_factor, warmup_iters
        self.last_iter = 0
        self.optimizer.lr = self.get_lr(0)

    def get_lr(self, it):
        value = self.base_lr * self.gamma ** bisect.bisect_right(self.milestones, it)
        if it < self.warmup_iters:
            # fvcore composite: linear from warmup_factor*start to the multistep value at the end of warm-up
            end = self.base_lr * self.gamma ** bisect.bisect_right(self.milestones, self.warmup_iters)
            start = self.warmup_factor * self.base_lr
            alpha = it / self.warmup_iters
            value = start * (1 - alpha) + end * alpha
        return value

    def step(self):
        self.last_iter += 1
        self.optimizer.lr = self.get_lr(self.last_iter)

    def resume_at(self, iteration):
        """Continue the schedule at `iteration` (the next step to run): the reference restores its scheduler through the
        checkpointer (engine/defaults.py:410-421 resume_or_load -> start_iter); without this a resumed run would restart the
        warm-up and count the STEPS milestones from the resume point."""
        self.last_iter = int(iteration)
        self.optimizer.lr = self.get_lr(self.last_iter)

    def state_dict(self):
        # "last_epoch" / "base_lrs" are what the reference's scheduler objects read back (fvcore's LRMultiplier and the plain
        # WarmupMultiStepLR of solver/lr_scheduler.py are torch LRSchedulers: load_state_dict = __dict__.update)
        groups = len(getattr(self.optimizer, "group_members", [0]))
        return {"last_iter": self.last_iter, "last_epoch": self.last_iter, "base_lrs": [self.base_lr] * groups}

    def load_state_dict(self, state):
        self.resume_at(state["last_iter"] if "last_iter" in state else state["last_epoch"])


def multistep_schedule(milestones, gamma, max_iter):
    """where in [0, 1] -> gamma^(#milestones passed): fvcore's MultiStepParamScheduler with values [gamma^k]
    (solver/build.py:289-301), whose iteration is int((where + 1e-6) * max_iter)."""
    milestones = sorted(milestones)
    return lambda where: gamma ** bisect.bisect_right(milestones, int((where + 1e-6) * max_iter))


def cosine_schedule(end):
    """where -> end + (1 - end) (1 + cos(pi where)) / 2: fvcore's CosineParamScheduler(1, end) (solver/build.py:302-305)."""
    return lambda where: end + 0.5 * (1.0 - end) * (1.0 + math.cos(math.pi * where))


class WarmupLR:
    """The reference's LRMultiplier over a WarmupParamScheduler (solver/lr_scheduler.py:22-58,61-125): one multiplier per
    iteration, and every group's rate is its initial rate times it - optimizer.lr = base_lr * m, and optimizer.lr_bias =
    optimizer.initial_lr_bias * m where the optimizer has a bias class (BIAS_LR_FACTOR), both in Python doubles as torch's
    scheduler forms them.  `schedule` maps where = iteration / max_iter to the main schedule's value (multistep_schedule,
    cosine_schedule).  The warm-up, restated from lr_scheduler.py:46-58 and the composite it builds:
        start = warmup_factor * schedule(0)
        end   = schedule(0) if rescale_interval else schedule(warmup_length),  warmup_length = min(warmup_iters / max_iter, 1)
        iteration < warmup_iters:  "constant": start;  "linear": end a + start (1 - a),  a = where / warmup_length
        afterwards:                schedule(where), or schedule((where - warmup_length) / (1 - warmup_length)) when rescaled
    Which part serves an iteration is decided on the integers (iteration < warmup_iters) where fvcore's composite compares
    where + 1e-6 with warmup_length: the same below a million iterations.  fvcore is not available to pin these values against;
    tests/test_solver_options_host.py checks them against numbers worked out by hand from the lines above."""

    def __init__(self, optimizer, base_lr, max_iter, schedule, warmup_factor, warmup_iters, warmup_method="linear",
                 rescale_interval=False):
        if warmup_method not in ("linear", "constant"):
            raise ValueError("SOLVER.WARMUP_METHOD must be 'linear' or 'constant', got %r" % (warmup_method,))
        self.optimizer, self.base_lr, self.max_iter, self.schedule = optimizer, base_lr, int(max_iter), schedule
        self.warmup_factor, self.warmup_iters = warmup_factor, min(int(warmup_iters), int(max_iter))
        self.warmup_method, self.rescale_interval = warmup_method, bool(rescale_interval)
        self.last_iter = 0
        self._apply()

    def multiplier(self, it):
        where = it / self.max_iter
        length = min(self.warmup_iters / self.max_iter, 1.0)
        if it < self.warmup_iters:
            start = self.warmup_factor * self.schedule(0.0)
            if self.warmup_method == "constant":
                return start
            end = self.schedule(0.0) if self.rescale_interval else self.schedule(length)
            a = where / length
            return end * a + start * (1 - a)
        if self.rescale_interval and length < 1.0:
            where = (where - length) / (1 - length)
        return self.schedule(where)

    def get_lr(self, it):
        return self.base_lr * self.multiplier(it)

    def _apply(self):
        m = self.multiplier(self.last_iter)
        self.optimizer.lr = self.base_lr * m
        if getattr(self.optimizer, "has_bias_lr", False):
            self.optimizer.lr_bias = self.optimizer.initial_lr_bias * m

    def step(self):
        self.last_iter += 1
        self._apply()

    def resume_at(self, iteration):
        """Continue the schedule at `iteration` (the next step to run), as WarmupMultiStepLR.resume_at."""
        self.last_iter = int(iteration)
        self._apply()

    def state_dict(self):
        # what LRMultiplier.state_dict writes: the groups' initial rates and the position
        opt = self.optimizer
        classes = getattr(opt, "group_lr_class", [0])
        base_lrs = [opt.initial_lr_bias if c and getattr(opt, "has_bias_lr", False) else self.base_lr for c in classes]
        return {"last_iter": self.last_iter, "last_epoch": self.last_iter, "base_lrs": base_lrs}

    def load_state_dict(self, state):
        self.resume_at(state["last_iter"] if "last_iter" in state else state["last_epoch"])


def build_lr_scheduler(cfg, optimizer):
    s = cfg.SOLVER
    name = s.LR_SCHEDULER_NAME
    warmup_iters = min(s.WARMUP_ITERS, s.MAX_ITER)
    rescale = bool(s.RESCALE_INTERVAL)
    if name == "WarmupMultiStepLR":
        steps = [x for x in s.STEPS if x <= s.MAX_ITER]
        if s.WARMUP_METHOD == "linear" and not rescale and not getattr(optimizer, "has_bias_lr", False):
            # the shipped configs: the class they have always run, and its values to the bit
            return WarmupMultiStepLR(optimizer, s.BASE_LR, steps, s.GAMMA, s.WARMUP_FACTOR, warmup_iters, s.WARMUP_METHOD)
        schedule = multistep_schedule(steps, s.GAMMA, s.MAX_ITER)
    elif name == "WarmupCosineLR":
        end = s.BASE_LR_END / s.BASE_LR
        if not 0.0 <= end <= 1.0:
            raise ValueError("SOLVER.BASE_LR_END / SOLVER.BASE_LR must lie in [0, 1], got %r" % (end,))
        schedule = cosine_schedule(end)
    elif name == "WarmupStepWithFixedGammaLR":
        raise ValueError("SOLVER.LR_SCHEDULER_NAME 'WarmupStepWithFixedGammaLR' is not implemented: its step rule lives in fvcore "
                         "(StepWithFixedGammaParamScheduler), which is not available to pin a restatement against")
    else:
        raise ValueError("Unknown SOLVER.LR_SCHEDULER_NAME: %r" % (name,))
    return WarmupLR(optimizer, s.BASE_LR, s.MAX_ITER, schedule, s.WARMUP_FACTOR, warmup_iters, s.WARMUP_METHOD, rescale)
