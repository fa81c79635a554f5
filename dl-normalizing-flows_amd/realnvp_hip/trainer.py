"""Fused RealNVP NLL training step (train.py:176-200) on the MI355X.

One step = logit_transform of a uint8-valued pixel batch (device Philox
noise), RealNVP forward with per-sample log-det accumulation, N(0,1) prior,
loss = -mean(log_prob + logdet) + 5e-5 * weight_scale, explicit backward
through every coupling / permutation, and a fused Adam update (coupled L2
weight decay, train.py:134) over ONE flat fp32 parameter arena.

MI355X-specific structure:
  * parameters, gradients and both Adam moments are flat arenas; the
    drop-in modules' nn.Parameters are views into the parameter arena, so
    state_dict / load_state_dict / torch optimizers keep working;
  * every buffer is allocated once; the whole step is captured into a HIP
    graph and replayed (no per-kernel host cost);
  * data parallel: one process per GPU, batch slice per rank, gradient
    arena averaged over RCCL in ~25 MB buckets that are issued on a
    communication stream as soon as backward has finished them (the deep
    scales, 86 % of the parameters, finish first), overlapping the
    remaining backward; optionally reduced in bf16.  BatchNorm statistics
    stay per rank (= the reference's semantics for each 64-image shard).
  * optimizer state converts to / from torch.optim.Adam.state_dict() format
    (train.py:139-154, 249-250 checkpoints).
  * optional step control (max_grad_norm / lr_schedule): the learning rate,
    clip_grad_norm_'s scale and the refusal of a non-finite gradient are
    decided on the device every step (rnvp_step_control), from a block the
    host only writes with stream-ordered copies -- the captured graph follows
    a schedule, set_lr() or set_max_grad_norm() without re-capture.
  * optional gradient accumulation (accum_steps=K): every step() is a
    micro-step of the same captured graph; the block counts them, K - 1
    steps add their gradient into an fp32 accumulator (rnvp_grad_accumulate)
    and hold -- parameters, moments, weight images and the step counter keep
    their bits -- and the K-th leaves the average in the gradient arena,
    decides on it and applies.  The dequantisation noise then has a counter
    of its own, which moves every micro-step.
  * optional weight averaging (ema_decay=d): an fp32 arena laid out like the
    parameters holds their exponential moving average; one launch after the
    step's last Adam launch (rnvp_ema_update) moves it, inside the captured
    step, and follows the device's skip / hold decisions.  ema_weights()
    exchanges the two arenas in place for evaluation and sampling.
"""
import contextlib
import ctypes as C
import gc
import math

import numpy as np
import torch

from . import _lib
from .engine import _launch, stream_ptr
from .engine import weights_key, wn_forward, wn_table  # noqa: F401 (importable from this module too)
from .program import FACTOR_OUT, RESTORE, SQUEEZE, UNDO, FlowProgram


def arena_blocks(model):
    """(offset, numel) of each coupling's parameters in the flat arena
    (named_parameters() order), couplings in forward order."""
    offs = {}
    off = 0
    for n, p in model.named_parameters():
        offs[n] = off
        off += p.numel()
    names = {id(m): n for n, m in model.named_modules()}
    out = []
    for mod in model.couplings():
        pre = names[id(mod)] + "."
        first = next(n for n, _ in mod.named_parameters())
        out.append((offs[pre + first], sum(p.numel() for p in mod.parameters())))
    return out


def bucket_plan(model, bucket_elems, n_total):
    """The trainer's all-reduce buckets for this model (dist.bucket_schedule
    over the coupling blocks in backward order)."""
    from .dist import bucket_schedule
    return bucket_schedule(list(reversed(arena_blocks(model))), bucket_elems, n_total)


class FlowTrainer:
    def __init__(self, model, batch_size, lr=5e-4, weight_decay=5e-5, betas=(0.9, 0.999), eps=1e-8,
                 scale_reg=5e-5, dtype="bf16", seed=0, process_group=None, bucket_mb=25, overlap=False,
                 comm="overlap", reduce_dtype="fp32", param_pass=None, chain=True, max_grad_norm=None,
                 lr_schedule=None, accum_steps=1, ema_decay=None, ema_warmup=True):
        from .stepctl import StepSchedule, check_accum_steps, check_ema_decay, check_max_grad_norm
        if lr_schedule is not None and not isinstance(lr_schedule, StepSchedule):
            raise ValueError("lr_schedule must be a realnvp_hip.stepctl.StepSchedule or None")
        self.max_grad_norm = check_max_grad_norm(max_grad_norm)
        self.lr_schedule = lr_schedule
        self.accum_steps = check_accum_steps(accum_steps)
        self.ema_decay, self.ema_warmup = check_ema_decay(ema_decay), bool(ema_warmup)
        if self.accum_steps > 1 and process_group is not None:
            raise ValueError("accum_steps > 1 with a process_group is not supported: every micro-step would "
                             "all-reduce (deferring it to the last one is not built)")
        # gradient-norm clipping (and the non-finite skip) is part of the step's
        # launch schedule: fixed at construction.  Gradient accumulation takes
        # the same schedule (the gradients final in the arena before ONE
        # parameter pass), with the accumulate pass where the norm is;
        # max_grad_norm=None then means guard only
        self.clip = self.max_grad_norm is not None or self.accum_steps > 1
        self.model = model
        self.dev = next(model.parameters()).device
        if self.dev.type != "cuda":
            raise RuntimeError("FlowTrainer needs the model on a HIP device")
        self.B = batch_size
        self.lr, self.wd, self.betas, self.eps, self.reg = lr, weight_decay, betas, eps, scale_reg
        self.dtype = dtype
        self.seed = seed
        self.pg = process_group
        self.rank = 0
        if process_group is not None:
            import torch.distributed as dist
            self.rank = dist.get_rank(process_group)
        model.set_precision(dtype)
        model.train()
        self._build_arenas()
        self._build_step_control()
        self._build_ema()
        self._build_plan(chain)
        self.graph = None
        self.graph_opt = None
        self.graph_input = None
        self.external_input = False
        self.bucket_elems = max(1, int(bucket_mb * 2 ** 20 // 4))
        if comm not in ("overlap", "split"):
            raise ValueError("comm must be 'overlap' or 'split'")
        if reduce_dtype not in ("fp32", "bf16"):
            raise ValueError("reduce_dtype must be 'fp32' or 'bf16'")
        self.comm, self.reduce_dtype = comm, reduce_dtype
        self._reduce_pg = None
        self._comm_off = False
        self.comm_events = None
        self.comm_stream = None
        if self.pg is not None and comm == "overlap":
            self.comm_stream = torch.cuda.Stream(device=self.dev)
        # side stream: weight gradients, weight-norm of the late couplings and
        # (single process) the per-coupling optimizer update run beside the
        # critical path (the forward/data-gradient chain)
        self.overlap = overlap
        self.side = torch.cuda.Stream(device=self.dev) if overlap else None
        # the deep couplings' weight-gradient groups of the running step, handed
        # over by their backward for the model-wide launch (engine.WGRAD_MULTI),
        # and the cached plans: key -> ([(WgradMulti, uploaded tables)] or None, groups)
        self._wg_multi = []
        self._wg_multi_plans = {}
        if param_pass not in (None, "fused", "separate"):
            raise ValueError("param_pass must be None (fused when possible), 'fused' or 'separate'")
        self._build_param_pass("separate" if param_pass == "separate" else "fused")
        if param_pass == "fused" and not self.fused:
            raise ValueError("param_pass='fused' is not possible for this model: %s" % self.param_pass_reason)
        if self.ctl_buf is not None and not self.fused:
            self._opt_all = self._adam_args(0)
        self._build_adam_ranges()
        self._build_buckets()
        self._cap_pg = self._capture_group()

    # ----------------------------------------------------------------- arenas
    def _build_arenas(self):
        named = list(self.model.named_parameters())
        n = sum(p.numel() for _, p in named)
        n_pad = (n + 3) // 4 * 4
        dev = self.dev
        self.n = n_pad
        self.param = torch.zeros(n_pad, device=dev, dtype=torch.float32)
        self.grad = torch.zeros(n_pad, device=dev, dtype=torch.float32)
        self.exp_avg = torch.zeros(n_pad, device=dev, dtype=torch.float32)
        self.exp_avg_sq = torch.zeros(n_pad, device=dev, dtype=torch.float32)
        mask = np.zeros(n_pad, dtype=np.uint8)
        self.offsets = {}
        off = 0
        with torch.no_grad():
            for name, p in named:
                k = p.numel()
                self.param[off:off + k].copy_(p.detach().reshape(-1))
                p.data = self.param[off:off + k].view_as(p)
                if p.requires_grad:
                    mask[off:off + k] = 2 if name.split(".")[-1] in ("weight_g", "scale") else 1
                self.offsets[name] = off
                off += k
        self.mask = torch.from_numpy(mask).to(dev)
        self.step_t = torch.zeros(1, device=dev, dtype=torch.int64)
        self.n_trainable = int((mask > 0).sum())

    # ----------------------------------------------------------- step control
    def _build_step_control(self):
        """The device-resident rnvp_step_ctl block (include/realnvp_hip.h) of a
        trainer built with lr_schedule and / or max_grad_norm, and the norm
        reduction's partials.  The host writes its configuration fields with
        stream-ordered fills (set_lr, set_max_grad_norm); nothing of it is a
        captured launch argument but its address."""
        self.ctl_buf = self.gs_partials = None
        # accumulation: the fp32 accumulator of the gradient arena, and the
        # dequantisation noise's own counter (the step counter stands still on
        # a held micro-step; this one moves every micro-step, skipped or not)
        self.acc = self.noise_t = None
        if self.lr_schedule is None and not self.clip:
            return
        from ._lib import StepCtl
        from .engine import upload
        from .stepctl import StepSchedule, fill_ctl
        c = fill_ctl(StepCtl(), self.lr, self.lr_schedule, self.max_grad_norm, self.accum_steps)
        c.lr = self.lr * (self.lr_schedule or StepSchedule()).factor(0)
        c.grad_scale = 1.0
        self.ctl_buf = upload(bytes(c), self.dev)
        if self.clip:
            self.gs_parts = int(_lib.lib().grad_sumsq_parts(self.n))
            self.gs_partials = torch.zeros(self.gs_parts, device=self.dev, dtype=torch.float64)
        if self.accum_steps > 1:
            self.acc = torch.zeros(self.n, device=self.dev, dtype=torch.float32)
            self.noise_t = torch.zeros(1, device=self.dev, dtype=torch.int64)

    def _ctl_field(self, name):
        """a one-element tensor view of a field of the control block"""
        from ._lib import StepCtl
        f = getattr(StepCtl, name)
        ct = dict(StepCtl._fields_)[name]
        dt = {C.c_float: torch.float32, C.c_double: torch.float64, C.c_int: torch.int32, C.c_longlong: torch.int64}[ct]
        return self.ctl_buf[f.offset:f.offset + f.size].view(dt)

    def _write_ctl_config(self):
        from ._lib import StepCtl
        from .stepctl import fill_ctl
        c = fill_ctl(StepCtl(), self.lr, self.lr_schedule, self.max_grad_norm)
        for name in ("base_lr", "warmup_start", "warmup_steps", "decay", "decay_rate", "decay_steps", "max_norm"):
            self._ctl_field(name).fill_(getattr(c, name))

    def set_lr(self, lr):
        """The base learning rate from the next step on.  With a control block
        a stream-ordered write (no re-capture); without one the rate is a
        captured launch argument, so the graph is dropped."""
        self.lr = float(lr)
        if self.ctl_buf is not None:
            self._ctl_field("base_lr").fill_(self.lr)
            return
        self._refresh_adam_args()
        if self.graph is not None:
            self.drop_graph()

    def set_max_grad_norm(self, v):
        """The clipping threshold from the next step on (None: no clipping, the
        non-finite skip stays); a stream-ordered write, no re-capture.  Needs a
        trainer built with max_grad_norm (or accum_steps > 1, which takes the
        same schedule): the norm pass is part of its step."""
        from .stepctl import check_max_grad_norm
        if not self.clip:
            raise RuntimeError("set_max_grad_norm needs a FlowTrainer built with max_grad_norm or accum_steps > 1 "
                               "(the gradient-norm pass is part of the step's launch schedule)")
        self.max_grad_norm = check_max_grad_norm(v)
        self._ctl_field("max_norm").fill_(self.max_grad_norm if self.max_grad_norm is not None else 0.0)

    def step_control_state(self):
        """What rnvp_step_control decided in the last step: lr, grad_norm (the
        pre-clip norm), grad_scale, skip, and the counters n_clipped /
        n_skipped; hold (the last step was a held micro-step of an
        accumulating trainer: skip is then set too, grad_norm and the counters
        are the last optimizer step's) and micro (micro-steps accumulated in
        the open optimizer step).  Synchronises (a device-to-host copy): the
        one documented sync of the step control."""
        if self.ctl_buf is None:
            raise RuntimeError("this FlowTrainer has no step control (built without lr_schedule / max_grad_norm)")
        from ._lib import StepCtl
        c = StepCtl.from_buffer_copy(bytes(self.ctl_buf.cpu().numpy()))
        return {"lr": c.lr, "grad_norm": c.grad_norm, "grad_scale": c.grad_scale, "skip": int(c.skip),
                "n_clipped": int(c.n_clipped), "n_skipped": int(c.n_skipped), "hold": int(c.hold),
                "micro": int(c.micro)}

    def _open_step(self):
        """first launch of a step with a control block: this step's learning
        rate, no clip and no skip until the norm has been taken"""
        if self.ctl_buf is not None:
            _launch("param", 64, 0.0, _lib.lib().step_control, self.ctl_buf.data_ptr(), self.step_t.data_ptr(), None,
                    0, stream_ptr())

    def _grad_norm_control(self):
        """Between the last gradient (after the all-reduce) and the first Adam
        launch: the arena's sum of squares, then the clip scale / skip.
        Accumulating: the accumulate pass in the norm's place (it leaves the
        averaged gradient and its partials on the final micro-step), then the
        control's hold / apply decision."""
        if not self.clip:
            return
        L = _lib.lib()
        s = stream_ptr()
        if self.acc is not None:
            _launch("param", 12 * self.n, 0.0, L.grad_accumulate, C.byref(self._opt_all), self.acc.data_ptr(), self.n,
                    self.ctl_buf.data_ptr(), self.gs_partials.data_ptr(), self.gs_parts, s)
        else:
            _launch("param", 5 * self.n, 0.0, L.grad_sumsq, C.byref(self._opt_all), self.n,
                    self.gs_partials.data_ptr(), self.gs_parts, s)
        _launch("param", 8 * self.gs_parts + 64, 0.0, L.step_control, self.ctl_buf.data_ptr(),
                self.step_t.data_ptr(), self.gs_partials.data_ptr(), self.gs_parts, s)

    def _advance_step(self):
        if self.ctl_buf is not None:
            _lib.lib().step_advance(self.step_t.data_ptr(), self.ctl_buf.data_ptr(), stream_ptr())
        else:
            _lib.lib().step_increment(self.step_t.data_ptr(), stream_ptr())
        if self.noise_t is not None:
            _lib.lib().step_increment(self.noise_t.data_ptr(), stream_ptr())

    def _noise_counter(self):
        """the Philox counter of the dequantisation noise: the step counter,
        or the micro-step counter of an accumulating trainer"""
        return (self.noise_t if self.noise_t is not None else self.step_t).data_ptr()

    # -------------------------------------------------------- weight averaging
    def _build_ema(self):
        """The average's arena (laid out like self.param, a copy of it to
        begin with) and its device-resident rnvp_ema_ctl block (include/
        realnvp_hip.h, "weight averaging") of a trainer built with ema_decay;
        nothing otherwise.  BatchNorm running statistics are buffers, and
        averages already: they are not part of it."""
        self.ema = self.ema_buf = None
        self._ema_in = False        # inside ema_weights(): the two arenas are exchanged
        if self.ema_decay is None:
            return
        from ._lib import EmaCtl
        from .engine import upload
        self.ema = self.param.clone()
        self.ema_buf = upload(bytes(EmaCtl(self.ema_decay, int(self.ema_warmup), 0.0, 0, 0)), self.dev)

    def _ema_field(self, name):
        """a one-element tensor view of a field of the average's block"""
        from ._lib import EmaCtl
        f = getattr(EmaCtl, name)
        dt = {C.c_float: torch.float32, C.c_int: torch.int32, C.c_longlong: torch.int64}[dict(EmaCtl._fields_)[name]]
        return self.ema_buf[f.offset:f.offset + f.size].view(dt)

    def _need_ema(self, what):
        if self.ema is None:
            raise RuntimeError("%s needs a FlowTrainer built with ema_decay" % what)

    def _not_swapped(self, what):
        if self._ema_in:
            raise RuntimeError("%s inside ema_weights(): the parameters hold the average" % what)

    def set_ema_decay(self, d):
        """The average's decay from the next step on: a stream-ordered write
        into its block, no re-capture."""
        from .stepctl import check_ema_decay
        self._need_ema("set_ema_decay")
        if d is None:
            raise ValueError("ema_decay must be in [0, 1), got None (weight averaging is fixed at construction)")
        self.ema_decay = check_ema_decay(d)
        self._ema_field("decay").fill_(self.ema_decay)

    def ema_state(self):
        """decay and warmup as configured, applied (the decay the last applied
        update used) and n_updates (updates applied: skipped and held steps
        do not count).  Synchronises (a device-to-host copy)."""
        self._need_ema("ema_state")
        from ._lib import EmaCtl
        c = EmaCtl.from_buffer_copy(bytes(self.ema_buf.cpu().numpy()))
        return {"decay": c.decay, "warmup": bool(c.warmup), "applied": c.applied, "n_updates": int(c.n_updates)}

    def reset_ema(self):
        """The average becomes the current parameters and n_updates 0: after
        the caller has written the parameters itself (an initialisation, a
        model.load_state_dict)."""
        self._need_ema("reset_ema")
        self._not_swapped("reset_ema")
        with torch.no_grad():
            self.ema.copy_(self.param)
        self._ema_field("n_updates").fill_(0)

    def _ema_update(self, step_add):
        """the step's one averaging launch, after its last Adam launch;
        step_add: 1 while the step counter has not moved yet, 0 after"""
        if self.ema is None:
            return
        _launch("param", 12 * self.n, 0.0, _lib.lib().ema_update, self.ema.data_ptr(), self.param.data_ptr(), self.n,
                self.ema_buf.data_ptr(), self.step_t.data_ptr(), step_add,
                self.ctl_buf.data_ptr() if self.ctl_buf is not None else None, stream_ptr())

    def _ema_swap(self):
        _lib.lib().ema_swap(self.param.data_ptr(), self.ema.data_ptr(), self.n, stream_ptr())
        self.invalidate_packed()

    def ema_state_dict(self):
        """model.state_dict()'s keys and shapes, cloned: the parameters from
        the average, the buffers as they are.  Loads into another RealNVP (or
        the reference's)."""
        self._need_ema("ema_state_dict")
        avg = self.param if self._ema_in else self.ema
        shapes = dict(self.model.named_parameters())
        out = {}
        for k, v in self.model.state_dict().items():
            if k in shapes:
                off = self.offsets[k]
                out[k] = avg[off:off + v.numel()].view_as(v).clone()
            else:
                out[k] = v.detach().clone()
        return out

    def ema_weights(self):
        """with tr.ema_weights(): the model's parameters hold the average
        (rnvp_ema_swap exchanges the two arenas in place -- no pointer moves,
        no temporary), so FlowEvaluator, FlowSampler and the drop-in modules,
        which derive their packed weight images from the parameters on every
        pass, evaluate and sample from it.  Leaving the block (an exception
        included) exchanges them back, and the next step re-derives the
        training images.  step(), step_eager(), capture() and the checkpoint
        methods raise inside the block; it is not re-entrant."""
        self._need_ema("ema_weights")
        return self._ema_swapped()

    @contextlib.contextmanager
    def _ema_swapped(self):
        self._not_swapped("ema_weights")
        self._ema_swap()
        self._ema_in = True
        try:
            yield self
        finally:
            self._ema_swap()
            self._ema_in = False

    # ------------------------------------------------------------------- plan
    def _build_plan(self, chain=True):
        m = self.model
        B, C, S = self.B, m.channels, m.image_size
        dev = self.dev
        f32 = dict(device=dev, dtype=torch.float32)
        self.pix = torch.zeros(B, C, S, S, **f32)
        self.logdet = torch.zeros(B, **f32)
        self.ldj = torch.zeros(B, **f32)
        self.prior = torch.zeros(B, dtype=torch.float64, device=dev)
        self.lp = torch.empty(B, **f32)
        self.g_lp = torch.full((B,), -1.0 / B, **f32)
        self.ll_acc = torch.zeros(1, dtype=torch.float64, device=dev)
        # the flow program (program.py): its couplings carry their slice of the gradient arena
        self.program = FlowProgram(m, B, dev, self.dtype, True, alloc=self._alloc_coupling)
        self.stages, self.xl, self.z = self.program.stages, self.program.x, self.program.z
        # backward buffers: a gradient buffer per forward tensor
        self.gbuf = {}
        self._build_links(chain)
        self._build_wn_table()

    def _build_links(self, chain):
        """The flow program as coupling links (rnvp_coupling_link_fwd / _bwd,
        include/realnvp_hip.h): what sits between coupling k and the next one
        in the stage list -- nothing (the next coupling of the same combo),
        a squeeze, undo_squeeze + factor_out (the next scale), or the end of
        the flow (restores only).  The permutations then live in the links'
        addressing and the next coupling's in part in the previous coupling's
        link launch.  chain=False (or a model whose couplings do not link,
        e.g. without out_bn) keeps every coupling's in / out parts, the
        permutation kernels and the prior as separate launches."""
        from ._lib import LinkArgs, RNVP_LINK_FINAL, RNVP_LINK_SAME, RNVP_LINK_SQUEEZE, RNVP_LINK_UNFACTOR
        self.cidx = [i for i, st in enumerate(self.stages) if st.kind == "coupling"]
        self.links = None
        if not chain:
            return
        types = []
        for k, i in enumerate(self.cidx):
            j = self.cidx[k + 1] if k + 1 < len(self.cidx) else len(self.stages)
            between = [st.kind for st in self.stages[i + 1:j]]
            a = self.stages[i].eng
            if not a.hp.coupling_bn:
                return
            if k + 1 == len(self.cidx):
                if any(b != RESTORE for b in between):
                    return
                types.append(RNVP_LINK_FINAL)
                continue
            n = self.stages[j].eng
            if between == [] and a.chains_into(n):
                types.append(RNVP_LINK_SAME)
            elif between == [SQUEEZE] and a.kind == 0 and n.kind == 1:
                types.append(RNVP_LINK_SQUEEZE)
            elif between == [UNDO, FACTOR_OUT] and a.kind == 1 and n.kind == 0:
                types.append(RNVP_LINK_UNFACTOR)
            else:
                return
        self.links = types
        self.link_fwd, self.link_bwd = [], []
        for k, (i, lt) in enumerate(zip(self.cidx, types)):
            la = LinkArgs(lt, self.g_lp.data_ptr(), self.prior.data_ptr(), None, None)
            nc = int(_lib.lib().link_nclass(lt, self.stages[i].eng.kind))
            if lt == RNVP_LINK_FINAL:
                nf = nb = None
            else:
                n = self.stages[self.cidx[k + 1]]
                nf = (n.eng, n.saved, n.x)
                nb = (n.eng, n.saved, n.x, self._g(n.x), n.block)
            self.link_fwd.append(dict(nclass=nc, args=la, nxt=nf))
            self.link_bwd.append(dict(nclass=nc, args=la, nxt=nb))

    def _build_wn_table(self):
        """Weight-norm descriptor tables over the model's convs: the packed
        bf16/fp32 weight images are refreshed by two forward weight-norm calls
        per step (2 launches each) instead of one per coupling.  The first
        table covers the early couplings (few parameters, needed at once), the
        second the late, deep couplings (most of the parameters), which the
        side stream prepares while the early couplings run."""
        engines = [st.eng for st in self.program.couplings]
        self.wn_split = min(len(engines), max(1, len(engines) * 3 // 7))
        self.wn_tables = [t for t in (wn_table(engines[:self.wn_split], self.dtype, self.dev),
                                      wn_table(engines[self.wn_split:], self.dtype, self.dev)) if t is not None]

    def _wn_fwd(self, table):
        wn_forward(table, self.dtype)

    # ------------------------------------------------------- parameter pass
    def _build_param_pass(self, mode):
        """The fused row-local parameter pass (rnvp_weight_norm_bwd_adam).

        Single process: each coupling's weight-norm backward launch also runs
        Adam on its conv rows (v, g, bias) and writes the new norms and both
        packed weight images, so the step has no separate Adam pass over the
        convs and no weight-norm forward (the images the forward reads were
        written by the previous step).  Data parallel: the per-coupling
        weight-norm backward stays (the all-reduce comes between it and Adam)
        and ONE model-wide launch does Adam + norms + images after the
        all-reduce.  The arena elements outside the convs (BatchNorm affines,
        coupling scales: 0.3 % of config 1's parameters) get a gather-Adam.
        The images are re-derived eagerly (two weight-norm launches) when the
        parameters changed outside the trainer's own kernels (_packed_token).
        mode 'separate' keeps weight_norm_fwd + weight_norm_bwd + adam_step."""
        self.fused = False
        self._slab_table = None
        self._packed_token = None
        self.param_pass_mode, self.param_pass_reason = "separate", "requested"
        if mode != "fused":
            return
        from ._lib import Range, WNDesc
        import ctypes as C
        mask = self.mask.cpu().numpy()
        covered = np.zeros(self.n, dtype=bool)
        base = self.grad.data_ptr()
        model_descs, blk0 = [], 0
        slab_descs, ranges = [], []

        def rebased(d, off, b0):
            e = WNDesc()
            C.memmove(C.addressof(e), C.addressof(d), C.sizeof(WNDesc))
            e.dv_off += off
            e.dg_off = e.dg_off + off if e.dg_off >= 0 else -1
            e.db_off = e.db_off + off if e.db_off >= 0 else -1
            e.blk0 += b0
            return e
        for st in self.program.couplings:
            eng, sv, block = st.eng, st.saved, st.block
            off = (block.data_ptr() - base) // 4
            ws = eng.weights(self.dtype)
            if ws["blocks"] < 0:
                self.param_pass_reason = "a conv row of %s does not fit the fused pass's LDS" % self._module_name(
                    st.mod)
                return
            if self.pg is None and not self.clip:
                # single process: every coupling's pass is deferred to ONE launch
                # at the end of the backward over the couplings' (persistent)
                # weight-gradient slabs.  (With gradient-norm clipping the
                # gradients must be final before the pass that consumes them:
                # the data-parallel schedule, with the norm where the
                # all-reduce is.)
                sdescs, rg = eng.param_pass_info(sv, self.dtype)
                slab_descs += [rebased(d, off, blk0) for d in sdescs]
                ranges += rg
            for d in ws["descs"]:
                kr = d.cin * d.ks * d.ks
                a = off + d.dv_off
                if not (mask[a:a + d.cout * kr] == 1).all():
                    self.param_pass_reason = "a conv of %s has frozen or regularised weight_v" % self._module_name(
                        st.mod)
                    return
                covered[a:a + d.cout * kr] = True
                if d.g and d.dg_off >= 0:
                    covered[off + d.dg_off:off + d.dg_off + d.cout] = True
                if d.db_off >= 0:
                    covered[off + d.db_off:off + d.db_off + d.cout] = True
                model_descs.append(rebased(d, off, blk0))
            blk0 += ws["blocks"]
        from .engine import upload
        self._opt_table = (upload(bytes((WNDesc * len(model_descs))(*model_descs)), self.dev), len(model_descs),
                           blk0)
        # algorithmic bytes of the parameter pass (bench.py kernel families):
        # dW replicas + v twice + m + v^2 read, grad + v + m + v^2 + wf written
        esz = 2 if self.dtype == "bf16" else 4
        n_w = sum(d.cout * d.cin * d.ks * d.ks for d in model_descs)
        nrep = sum(d.cout * d.cin * d.ks * d.ks * max(d.nz, 1) for d in slab_descs) if slab_descs else 0
        # the transposes also write the fragment-major copies (engine.weights: bf16 3x3 convs)
        n_frag = sum(d.cout * d.cin * d.ks * d.ks * (int(bool(d.wf_frag)) + int(bool(d.wd_frag))) for d in model_descs)
        self._param_bytes = (4 * (nrep if slab_descs else n_w) + 32 * n_w + esz * n_w, 2 * esz * n_w + esz * n_frag)
        self._slab_table = None
        if slab_descs:
            self._slab_table = (upload(bytes((WNDesc * len(slab_descs))(*slab_descs)), self.dev), len(slab_descs),
                                blk0)
            rt = (Range * len(ranges))(*[Range(p, b) for p, b in ranges])
            self._zero_table = (upload(bytes(rt), self.dev), len(ranges), max(b for _, b in ranges))
        rest = np.nonzero((mask > 0) & ~covered)[0].astype(np.int64)
        self._opt_rest = torch.from_numpy(rest).to(self.dev)
        self._opt_all = self._adam_args(0)
        self._vparams = [p for _, p in self.model.named_parameters()]
        self.fused = True
        self.param_pass_mode, self.param_pass_reason = "fused", None

    def _adam_args(self, off):
        from ._lib import AdamArgs
        a = AdamArgs()
        a.param, a.grad = self.param.data_ptr() + 4 * off, self.grad.data_ptr() + 4 * off
        a.exp_avg, a.exp_avg_sq = self.exp_avg.data_ptr() + 4 * off, self.exp_avg_sq.data_ptr() + 4 * off
        a.mask, a.step, a.step_add = self.mask.data_ptr() + off, self.step_t.data_ptr(), 1
        a.lr, a.beta1, a.beta2, a.eps = self.lr, self.betas[0], self.betas[1], self.eps
        a.weight_decay, a.reg_coef = self.wd, self.reg
        a.ctl = self.ctl_buf.data_ptr() if self.ctl_buf is not None else None
        return a

    def _refresh_adam_args(self):
        """lr / betas / eps / weight decay changed (load_optimizer_state_dict)"""
        if not self.fused and self.ctl_buf is None:
            return
        for a in (self._opt_all,):
            a.lr, a.beta1, a.beta2, a.eps = self.lr, self.betas[0], self.betas[1], self.eps
            a.weight_decay, a.reg_coef = self.wd, self.reg

    def _token(self):
        return (self.param._version, sum(p._version for p in self._vparams))

    def invalidate_packed(self):
        """Declare the parameters changed outside the trainer: the next step
        re-derives the packed weight images (fused parameter pass).  Writes
        through the parameters themselves (p.mul_, load_state_dict, ...) are
        seen on their own; writes through `p.data` (e.g. nn.init on
        `.data`, the reference's utils.py:103-113 style) or through the
        arena tensor's storage by other means are NOT -- call this after them."""
        self._packed_token = None

    def _ensure_packed(self):
        """Fused pass: the packed weight images and norms are the previous
        step's output; re-derive them (eagerly) when the parameters were
        changed by anything else (first step, capture's restore,
        load_state_dict, a caller writing the parameters: their version
        counters move; writes through `.data` need invalidate_packed())."""
        if not self.fused:
            return
        tok = self._token()
        if tok != self._packed_token:
            for t in self.wn_tables:
                self._wn_fwd(t)
            self._packed_token = tok

    def _build_adam_ranges(self):
        """Per-coupling optimizer ranges [ru4(off_i), ru4(off_next)) of the flat
        arena (float4 granules).  A granule straddling two couplings belongs to
        the range of the coupling at the LOWER offset, whose update runs after
        the other's in backward order -- so every gradient in a range is final
        when its update runs.  Disabled (one update at the end) unless the
        backward visits couplings in descending arena offset."""
        self.adam_ranges = None
        if self.pg is not None or not self.overlap or self.fused or self.links is not None or self.clip:
            return
        blocks = [st.block for st in self.program.couplings]
        base = self.grad.data_ptr()
        offs = [(b.data_ptr() - base) // 4 for b in blocks]
        if offs != sorted(offs) or offs[0] != 0:
            return
        ru = lambda v: (v + 3) // 4 * 4  # noqa: E731
        ends = offs[1:] + [self.n]
        self.adam_ranges = [(ru(o), (ru(e) if e < self.n else self.n)) for o, e in zip(offs, ends)]

    def _build_buckets(self):
        """All-reduce buckets in backward order (dist.bucket_schedule over the
        couplings' gradient blocks); bucket k is issued right after coupling
        bucket_after[k]'s backward has been scheduled."""
        blocks = [st.block for st in self.program.couplings]
        base = self.grad.data_ptr()
        spans = [((b.data_ptr() - base) // 4, b.numel()) for b in blocks]
        if spans != arena_blocks(self.model):
            raise RuntimeError("coupling gradient blocks do not follow the parameter arena")
        self.buckets = bucket_plan(self.model, self.bucket_elems, self.n)
        self.bucket_after = {}
        for lo, hi, k in self.buckets:
            self.bucket_after.setdefault(k, []).append((lo, hi))
        self.reduce_buf = None
        if self.pg is not None and self.reduce_dtype == "bf16":
            self.reduce_buf = torch.empty(self.n, device=self.dev, dtype=torch.bfloat16)

    def _reduce_bucket(self, lo, hi):
        """Average grad[lo:hi) over the process group (on the current stream).
        No-op during capture()'s warm-up steps (see capture)."""
        if self._comm_off:
            return
        from .dist import average_slice
        pg = self._reduce_pg if self._reduce_pg is not None else self.pg
        average_slice(self.grad, lo, hi, pg, self.reduce_buf)

    def _capture_group(self):
        """The process group the captured step all-reduces over.

        RCCL's process group hands every eager collective to a watchdog
        thread that polls the collective's completion event on the group's
        communication stream until it retires it.  Inside a capture that
        stream joins the graph, and an event poll on a capturing stream is a
        fatal HIP error (it aborted the world-1 test twice in round 2, when a
        warm-up all-reduce was still on the watchdog's list).  So the capture
        uses a second group over the same ranks, created at construction
        (every rank of the trainer's group constructs its trainer; local
        synchronisation, so a process_group that is a subgroup of a larger
        world does not need the ranks outside it), connected eagerly (no
        collective) and used ONLY inside captures: its watchdog list is empty
        by construction, and the warm-up group's stream never captures.
        Collectives issued while capturing are not handed to any watchdog.
        gloo (CPU tests) needs no second group."""
        if self.pg is None or self.comm_stream is None:
            return None
        import torch.distributed as dist
        if dist.get_backend(self.pg) != "nccl":
            return self.pg
        ranks = dist.get_process_group_ranks(self.pg)
        g = dist.new_group(ranks=ranks, backend="nccl", use_local_synchronization=True)
        g._get_backend(self.dev).eager_connect_single_device(self.dev)
        return g

    def _alloc_coupling(self, mod, x):
        eng = mod.engine()
        B, C, H, W = x.shape
        sv = eng.alloc_saved(B, H, W, self.dtype, self.dev, True)
        first = next(n for n, _ in mod.named_parameters())
        name = self._module_name(mod) + "." + first
        return eng, sv, self.grad[self.offsets[name]:self.offsets[name] + eng.n_params]

    def _module_name(self, mod):
        if not hasattr(self, "_names"):
            self._names = {id(m): n for n, m in self.model.named_modules()}
        return self._names[id(mod)]

    def _g(self, t):
        """gradient buffer shaped like forward tensor t"""
        k = t.data_ptr()
        g = self.gbuf.get(k)
        if g is None:
            g = torch.empty_like(t)
            self.gbuf[k] = g
        return g

    # ------------------------------------------------------------------- step
    def _wn_prepare(self):
        """the packed weight images of this step (separate parameter pass:
        the weight-norm forward; fused: the previous step's, _ensure_packed)"""
        late_ready = None
        if self.fused:
            pass
        elif len(self.wn_tables) > 1 and self.side is not None:
            ev = torch.cuda.Event()
            ev.record()
            self.side.wait_event(ev)
            with torch.cuda.stream(self.side):
                self._wn_fwd(self.wn_tables[1])
                late_ready = torch.cuda.Event()
                late_ready.record()
            self._wn_fwd(self.wn_tables[0])
        else:
            for t in self.wn_tables:
                self._wn_fwd(t)
        return late_ready

    def _forward(self):
        if self.links is not None:
            return self._forward_links()
        L = _lib.lib()
        s = stream_ptr()
        B = self.B
        n = self.pix[0].numel()
        if not self.external_input:
            L.logit_fwd(self.pix.data_ptr(), None, self.seed, 0, self._noise_counter(), 0.9, self.xl.data_ptr(),
                        self.logdet.data_ptr(), B, n, s)
        self.ldj.zero_()
        late_ready = self._wn_prepare()

        def coupling(ci, st):
            if ci == self.wn_split and late_ready is not None:
                torch.cuda.current_stream().wait_event(late_ready)
            st.eng.forward(st.x, True, self.dtype, False, saved=st.saved, prepare=False, ldj_sample=self.ldj,
                           z_out=st.z, zero_sums=False)
        self.program.forward(coupling)
        L.prior_logprob(self.z.data_ptr(), self.ldj.data_ptr(), self.lp.data_ptr(), B, self.z[0].numel(), s)
        self.ll_acc += (self.lp + self.logdet).mean().double()

    def _forward_links(self):
        """The flow program over coupling links: the input pass (logit
        transform + the first coupling's in_bn sums), the first coupling's in
        part, then per coupling its net, u's class sums and the link, and the
        per-sample log-likelihood.  No permutation kernel, no prior pass:
        the prior of the factored-out halves and of the last scale is added
        by the links."""
        L = _lib.lib()
        s = stream_ptr()
        B = self.B
        first = self.program.couplings[0]
        x0 = first.x
        a0 = first.eng.link_args(first.saved, x0)
        n_el, esz = x0.numel(), 2 if self.dtype == "bf16" else 4
        cs_h0 = a0.cs_h0
        if not self.external_input:
            _launch("logit", 8 * n_el, 0.0, L.flow_in_fwd, self.pix.data_ptr(), self.seed, self._noise_counter(),
                    0.9, self.xl.data_ptr(), self.logdet.data_ptr(), C.byref(a0), B, *x0.shape[1:], s)
            _launch("coupling", 4 * n_el + esz * x0[:, 0].numel() * cs_h0, 0.0, L.coupling_in_apply, C.byref(a0), s)
        else:
            _launch("coupling", 8 * n_el + esz * x0[:, 0].numel() * cs_h0, 0.0, L.coupling_in_fwd, C.byref(a0), s)
        late_ready = self._wn_prepare()
        for k, st in enumerate(self.program.couplings):
            if k == self.wn_split and late_ready is not None:
                torch.cuda.current_stream().wait_event(late_ready)
            st.eng.forward_link(st.x, st.saved, self.ldj, self.link_fwd[k])
        L.flow_lp_finish(self.prior.data_ptr(), self.ldj.data_ptr(), self.logdet.data_ptr(),
                         0 if self.external_input else 1, self.lp.data_ptr(), self.ll_acc.data_ptr(), B, s)

    def _issue_buckets(self, ci, n_coupling):
        """the all-reduce buckets that coupling ci's gradients complete"""
        if self.comm_stream is None:
            return
        for lo, hi in self.bucket_after.get(n_coupling - 1 - ci, ()):
            # the bucket's weight gradients were written on the side
            # stream (overlap) or the current one
            ev = torch.cuda.Event()
            ev.record(self.side if self.side is not None else torch.cuda.current_stream())
            self.comm_stream.wait_event(ev)
            with torch.cuda.stream(self.comm_stream):
                if self.comm_events is not None:     # bench.py: per-bucket timing (eager)
                    e0 = torch.cuda.Event(enable_timing=True)
                    e0.record()
                self._reduce_bucket(lo, hi)
                if self.comm_events is not None:
                    e1 = torch.cuda.Event(enable_timing=True)
                    e1.record()
                    self.comm_events.append((hi - lo, e0, e1))

    def _backward(self):
        if self.links is not None:
            return self._backward_links()
        L = _lib.lib()
        s = stream_ptr()
        B = self.B
        gz = self._g(self.z)
        L.prior_logprob_bwd(self.z.data_ptr(), self.g_lp.data_ptr(), gz.data_ptr(), B, self.z[0].numel(), s)
        n_coupling = len(self.cidx)

        def coupling(ci, st):
            after = None
            if self.adam_ranges is not None:
                lo, hi = self.adam_ranges[ci]
                after = (lambda lo=lo, hi=hi: self._adam_range(lo, hi))
            opt = "defer" if self._slab_table is not None else None
            st.eng.backward(st.saved, self._g(st.z), None, self.g_lp, st.block, gx=self._g(st.x), side=self.side,
                            after=after, zero_at_end=True, opt=opt, multi=self._multi_list(opt))
            self._issue_buckets(ci, n_coupling)
        # the permutations' gradients: the inverse program over the gradient buffers
        self.program.inverse(coupling, buf=self._g)

    def _backward_links(self):
        """Backward over the coupling links, last coupling first: its link
        backward (dL/dz from the consumer or the prior, then its out part),
        its net's data gradients and its in part's reduction pass.  A
        coupling's weight gradients (and, outside the fused single-process
        pass, its weight-norm backward, which leaves its sums zero) run after
        the previous coupling's link backward has read those sums; its
        all-reduce buckets follow them."""
        n_coupling = len(self.cidx)
        opt = "defer" if self._slab_table is not None else None
        pending, pending_ci = [], None
        for k in reversed(range(n_coupling)):
            st = self.program.couplings[k]
            mine = []
            st.eng.backward_link(st.saved, self.link_bwd[k], st.block, self._g(st.x), self.g_lp, k == 0, mine,
                                 opt=opt, multi=self._multi_list(opt))
            self._run_pending(pending, pending_ci, n_coupling)
            pending, pending_ci = mine, k
        self._run_pending(pending, pending_ci, n_coupling)

    def _multi_list(self, opt):
        """The list that collects the couplings' weight-gradient groups for
        the model-wide launch: the single-process deferred parameter pass on
        the main stream only (data-parallel, clipping, accumulation and
        --overlap schedules keep every coupling's own launch)."""
        from . import engine
        return self._wg_multi if engine.WGRAD_MULTI and opt == "defer" and self.side is None else None

    def _wgrad_multi(self):
        """The weight gradients the couplings' backwards handed over
        (engine.WGRAD_MULTI): one launch per tile class over all of them,
        after the last coupling's backward and before the parameter pass that
        first reads their slabs (merging per run of same-shape couplings
        instead, while their operands are still in the last-level cache,
        measured 0.10 ms per step slower: profiles/wgrad_multi_ab.txt).  The
        plan is built once and rebuilt when a coupling's backward plan or
        scratch changes."""
        items = self._wg_multi
        if not items:
            return
        from . import engine
        L = _lib.lib()
        s = stream_ptr()
        key = tuple((it[3], it[4]) for it in items)
        if key not in self._wg_multi_plans:
            if len(self._wg_multi_plans) >= 16:     # (stale keys: a backward plan or a scratch was rebuilt)
                self._wg_multi_plans.clear()
            groups = [g for it in items for g in it[0]]
            self._wg_multi_plans[key] = (engine.plan_wgrad_multi(groups, self.dev), groups)
        plan, groups = self._wg_multi_plans[key]
        nb, fl = sum(it[1] for it in items), sum(it[2] for it in items)
        if plan is None:
            # the library declines the combined list: every group's own launch
            for g in groups:
                _launch("conv_wgrad", nb / len(groups), fl / len(groups), L.conv2d_wgrad_grouped, C.byref(g), s)
        else:
            for m, _ in plan:
                _launch("conv_wgrad", nb / len(plan), fl / len(plan), L.conv2d_wgrad_multi, C.byref(m), s)
        items.clear()

    def _run_pending(self, pending, ci, n_coupling):
        if not pending:
            return
        if self.side is not None:
            self._flush_side(pending)
        else:
            for f in pending:
                f()
            pending.clear()
        self._issue_buckets(ci, n_coupling)

    def _flush_side(self, pending):
        """fork the deferred weight-gradient closures onto the side stream"""
        ev = torch.cuda.Event()
        ev.record()
        self.side.wait_event(ev)
        with torch.cuda.stream(self.side):
            for f in pending:
                f()
        pending.clear()

    def _adam_range(self, lo, hi):
        b1, b2 = self.betas
        if hi <= lo:
            return
        if self.ctl_buf is not None:
            _lib.lib().adam_range(C.byref(self._adam_args(lo)), hi - lo, stream_ptr())
            return
        _lib.lib().adam_update(self.param.data_ptr() + 4 * lo, self.grad.data_ptr() + 4 * lo,
                               self.exp_avg.data_ptr() + 4 * lo, self.exp_avg_sq.data_ptr() + 4 * lo, hi - lo,
                               self.step_t.data_ptr(), 1, self.lr, b1, b2, self.eps, self.wd,
                               self.mask.data_ptr() + lo, self.reg, stream_ptr())

    def _optimizer(self):
        self._grad_norm_control()
        if self.fused:
            L = _lib.lib()
            s = stream_ptr()
            dt = 1 if self.dtype == "bf16" else 0
            pb, tb = self._param_bytes
            if self._slab_table is None:
                # data parallel (or gradient-norm clipping): the conv rows' Adam +
                # norms + images, after the all-reduce (the norm)
                t, n, nblk = self._opt_table
                _launch("param", pb, 0.0, L.weight_norm_bwd_adam, t.data_ptr(), n, nblk, 0, dt,
                        C.byref(self._opt_all), None, 0, None, 0, s)
            else:
                # single process: every coupling's slabs -> dv / dg / dbias, Adam,
                # norms and forward images in ONE launch (small couplings' rows fill
                # the big ones' gaps), then their batch sums left zero
                t, n, nblk = self._slab_table
                _launch("param", pb, 0.0, L.weight_norm_bwd_adam, t.data_ptr(), n, nblk, 1, dt,
                        C.byref(self._opt_all), None, 0, None, 0, s)
                zt, nz, zb = self._zero_table
                L.zero_ranges(zt.data_ptr(), nz, zb, s)
            # the data-gradient images from the forward images the row kernels wrote
            for t, n, _, tiles in self.wn_tables:
                _launch("param", tb / len(self.wn_tables), 0.0, L.weight_norm_transpose, t.data_ptr(), n, tiles, dt,
                        s)
            L.adam_gather(C.byref(self._opt_all), self._opt_rest.data_ptr(), self._opt_rest.numel(), s)
            self._ema_update(1)
            self._advance_step()
            return
        if self.adam_ranges is not None:
            # the per-coupling updates already ran (side stream, t = step + 1;
            # _fwd_bwd has made this stream wait for them)
            self._ema_update(1)
            self._advance_step()
            return
        if self.ctl_buf is not None:
            # rnvp_adam_step's update (t = step + 1) under the step control
            _lib.lib().adam_range(C.byref(self._opt_all), self.n, stream_ptr())
            self._ema_update(1)
            self._advance_step()
            return
        b1, b2 = self.betas
        _lib.lib().adam_step(self.param.data_ptr(), self.grad.data_ptr(), self.exp_avg.data_ptr(),
                             self.exp_avg_sq.data_ptr(), self.n, self.step_t.data_ptr(), self.lr, b1, b2, self.eps,
                             self.wd, self.mask.data_ptr(), self.reg, stream_ptr())
        self._ema_update(0)     # (rnvp_adam_step's first kernel has moved the counter)

    def _allreduce(self):
        """Whole-arena bucketed average ("split" mode: between the captured
        forward/backward graph and the optimizer graph)."""
        if self.pg is None or self.comm_stream is not None:
            return
        for lo, hi, _ in self.buckets:
            self._reduce_bucket(lo, hi)

    def _fwd_bwd(self):
        self._open_step()
        if self.fused:
            # every conv gradient (v, g, bias) is written, not accumulated, by
            # the row kernels and every BatchNorm affine gradient by its
            # backward apply: only the accumulated ones (coupling scale /
            # scale_shift, +=) need zeroing -- the 0.3 % outside the convs
            self.grad.index_fill_(0, self._opt_rest, 0.0)
        else:
            self.grad.zero_()
        self._forward()
        del self._wg_multi[:]
        self._backward()
        self._wgrad_multi()
        if self.side is not None:
            torch.cuda.current_stream().wait_stream(self.side)
        if self.comm_stream is not None:
            torch.cuda.current_stream().wait_stream(self.comm_stream)

    def step_eager(self):
        self._not_swapped("step_eager()")
        self._ensure_packed()
        self._fwd_bwd()
        self._allreduce()
        self._optimizer()

    # --------------------------------------------------------------- graphs
    def _snapshot(self):
        bufs = {n: b.detach().clone() for n, b in self.model.named_buffers()}
        ctl = self.ctl_buf.clone() if self.ctl_buf is not None else None
        accum = (self.acc.clone(), self.noise_t.clone()) if self.acc is not None else None
        ema = (self.ema.clone(), self.ema_buf.clone()) if self.ema is not None else None
        return (self.param.clone(), self.exp_avg.clone(), self.exp_avg_sq.clone(), self.step_t.clone(),
                self.ll_acc.clone(), bufs, ctl, accum, ema)

    def _restore(self, snap):
        p, m, v, t, ll, bufs, ctl, accum, ema = snap
        with torch.no_grad():
            if ema is not None:
                self.ema.copy_(ema[0])
                self.ema_buf.copy_(ema[1])  # the warm-up steps' n_updates
            if ctl is not None:
                self.ctl_buf.copy_(ctl)     # the warm-up steps' counters (and micro)
            if accum is not None:
                self.acc.copy_(accum[0])
                self.noise_t.copy_(accum[1])
            self.param.copy_(p)
            self.exp_avg.copy_(m)
            self.exp_avg_sq.copy_(v)
            self.step_t.copy_(t)
            self.ll_acc.copy_(ll)
            for n, b in self.model.named_buffers():
                b.copy_(bufs[n])

    def capture(self, warmup=2, restore=True, before_capture=None):
        """Warm up eagerly on a side stream, then capture the step into HIP
        graphs.  The warm-up steps move the parameters, Adam moments, step
        counter (and with it the dequantisation noise) and BN running stats;
        with restore=True (default) all of that is put back afterwards, so
        the first replay is the caller's first training step.  The input mode
        (set_pixels: logit transform inside the graph, or set_input: an
        already transformed batch) is fixed at capture.

        Single process, and data parallel with comm="overlap": ONE graph
        holds forward, backward, the bucketed all-reduces on the
        communication stream and Adam.  comm="split": forward/backward graph,
        eager all-reduce, optimizer graph.

        Nothing but the captured step's own work runs while a capture is
        open (the round-4 abort: SIGABRT from a thread without a Python
        frame in the middle of a capture):
          * the warm-up steps issue no collective (their state is restored,
            so with a process group restore must be True);
          * the captured all-reduces use a capture-only group (_capture_group);
          * unreachable objects are collected and their HIP teardown drained
            before the capture, and the garbage collector is off during it,
            so no graph / event / stream of another object is destroyed
            mid-capture.
        tools/probe/capture_watchdog.py showed that a c10d watchdog polling a
        finished eager all-reduce during a thread-local capture does NOT
        abort on this stack, so a pending watchdog entry alone is not the
        cause; the construction above removes every other thread-visible
        event of the window."""
        if self.pg is not None and not restore:
            raise ValueError("with a process group, capture() must restore the warm-up state: its warm-up "
                             "steps issue no all-reduce (see capture)")
        self._not_swapped("capture()")
        snap = self._snapshot() if restore else None
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        # The warm-up steps issue NO collective: their state is discarded
        # (restore) and a collective issued here would sit on its group's
        # watchdog list when the capture opens (see _wait_collectives_retired)
        self._comm_off = True
        try:
            with torch.cuda.stream(side):
                for _ in range(warmup):
                    self.step_eager()
        finally:
            self._comm_off = False
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        # Destroy unreachable objects (earlier trainers' graphs, events,
        # streams) NOW and let the HIP work their destruction queues drain,
        # and run no garbage collection while the capture is open: a cyclic
        # collection triggered by any allocation inside the capture would
        # otherwise destroy HIP graphs / events / streams of other objects in
        # the middle of it (see capture's note on the round-4 abort)
        gc.collect()
        torch.cuda.synchronize()
        # the captured all-reduces go through a group of their own (see
        # _capture_group); eager collectives stay on self.pg
        if before_capture is not None:
            before_capture()
        self.graph = torch.cuda.CUDAGraph()
        self.graph_opt = None
        self.graph_input = self.external_input
        # thread-local capture: other threads' HIP calls are not checked
        # against our capture (HIP still refuses an event query meanwhile,
        # hence the drain above)
        mode = "thread_local"
        gc_on = gc.isenabled()
        gc.disable()
        try:
            if self.pg is None or self.comm_stream is not None:
                try:
                    self._reduce_pg = self._cap_pg
                    with torch.cuda.graph(self.graph, capture_error_mode=mode):
                        self._fwd_bwd()
                        self._optimizer()
                finally:
                    self._reduce_pg = None
            else:
                with torch.cuda.graph(self.graph, capture_error_mode=mode):
                    self._fwd_bwd()
                self.graph_opt = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph_opt, capture_error_mode=mode):
                    self._optimizer()
        finally:
            if gc_on:
                gc.enable()
        torch.cuda.synchronize()
        if snap is not None:
            self._restore(snap)
            torch.cuda.synchronize()
        return warmup

    def drop_graph(self):
        self.graph = self.graph_opt = self.graph_input = None

    def step(self):
        self._not_swapped("step()")
        if self.graph is None:
            return self.step_eager()
        self._ensure_packed()
        self.graph.replay()
        if self.graph_opt is not None:
            self._allreduce()
            self.graph_opt.replay()

    def _check_mode(self, external):
        if self.graph is not None and self.graph_input != external:
            raise RuntimeError("the captured step reads %s; call drop_graph() (or capture again) before feeding "
                               "%s" % ("set_input() batches" if self.graph_input else "set_pixels() pixels",
                                       "set_input() batches" if external else "set_pixels() pixels"))

    def set_pixels(self, pix):
        """Raw pixels in [0, 1]; the step applies logit_transform on the device."""
        self._check_mode(False)
        if self.external_input:
            self.logdet.zero_()   # the input pass adds the log-det (rnvp_flow_in_fwd)
        self.external_input = False
        self.pix.copy_(pix)

    def set_input(self, x, logdet):
        """Feed an already logit-transformed batch (parity tests)."""
        self._check_mode(True)
        self.external_input = True
        self.xl.copy_(x)
        self.logdet.copy_(logdet)

    # ------------------------------------------------------- checkpointing
    def _param_list(self):
        return list(self.model.named_parameters())

    def optimizer_state_dict(self):
        """The fused Adam's state as torch.optim.Adam(model.parameters(),
        lr, betas, eps, weight_decay).state_dict() would hold it (the
        reference's realnvp_state_optim.pt, train.py:250): per trainable
        parameter index exp_avg / exp_avg_sq / step; frozen parameters (no
        gradient, skipped by torch's Adam) carry no state."""
        step = float(self.step_t.item())
        state = {}
        named = self._param_list()
        for i, (n, p) in enumerate(named):
            if not p.requires_grad or step == 0:
                continue
            off, k = self.offsets[n], p.numel()
            state[i] = {"step": torch.tensor(step),
                        "exp_avg": self.exp_avg[off:off + k].view_as(p).clone(),
                        "exp_avg_sq": self.exp_avg_sq[off:off + k].view_as(p).clone()}
        group = {"lr": self.lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": self.wd,
                 "amsgrad": False, "maximize": False, "foreach": None, "capturable": False,
                 "differentiable": False, "fused": None, "decoupled_weight_decay": False,
                 "params": list(range(len(named)))}
        return {"state": state, "param_groups": [group]}

    def load_optimizer_state_dict(self, sd):
        """Inverse of optimizer_state_dict (accepts what torch.optim.Adam
        saved for model.parameters(); train.py:149-154)."""
        named = self._param_list()
        groups = sd["param_groups"]
        idx = [i for g in groups for i in g["params"]]
        if len(idx) != len(named):
            raise ValueError("optimizer state has %d parameters, the model %d" % (len(idx), len(named)))
        g0 = groups[0]
        if g0.get("amsgrad") or g0.get("maximize") or g0.get("decoupled_weight_decay"):
            raise ValueError("only plain Adam with coupled weight decay is supported (train.py:134)")
        steps = set()
        with torch.no_grad():
            self.exp_avg.zero_()
            self.exp_avg_sq.zero_()
            for pos, (n, p) in zip(idx, named):
                st = sd["state"].get(pos)
                if st is None:
                    continue
                off, k = self.offsets[n], p.numel()
                self.exp_avg[off:off + k].copy_(st["exp_avg"].reshape(-1))
                self.exp_avg_sq[off:off + k].copy_(st["exp_avg_sq"].reshape(-1))
                steps.add(float(st["step"]))
        if len(steps) > 1:
            raise ValueError("per-parameter Adam step counts differ: %s" % sorted(steps))
        self.step_t.fill_(int(steps.pop()) if steps else 0)
        baked = (tuple(self.betas), self.eps, self.wd) != (tuple(g0["betas"]), g0["eps"], g0["weight_decay"])
        self.lr, self.betas, self.eps, self.wd = g0["lr"], tuple(g0["betas"]), g0["eps"], g0["weight_decay"]
        self._refresh_adam_args()
        if self.ctl_buf is not None:
            # the base rate lives in the control block: no re-capture for it
            self._ctl_field("base_lr").fill_(self.lr)
            if not baked:
                return
        if self.graph is not None:
            self.drop_graph()    # lr / betas are baked into the captured launches

    def rng_state(self):
        """The dequantisation noise stream: k_logit_fwd draws step t's noise
        from Philox(seed, counter = t), so (seed, t) is the whole RNG state
        (the reference saves none, train.py:249-250).  The
        saving rank is recorded: data-parallel ranks draw from seeds of their
        own.  An accumulating trainer draws micro-step j's noise from counter
        j, a counter of its own ('noise_step'): the step counter stands still
        while gradients accumulate."""
        st = {"seed": int(self.seed), "rank": int(self.rank), "step": int(self.step_t.item())}
        if self.noise_t is not None:
            st["noise_step"] = int(self.noise_t.item())
        return st

    def state_dict(self):
        """{'model': model.state_dict(), 'optimizer': torch-Adam-format state,
        'rng': rng_state()} (the two files train.py:249-250 writes, plus the
        noise stream so a resumed run draws the same noise as an unbroken one).
        A trainer with a step control adds 'step_control': the schedule's
        configuration, max_grad_norm and the two counters (the base rate
        stays in the optimizer's param_groups[0]['lr']), accum_steps and
        micro, and -- taken between the micro-steps of one optimizer step,
        micro > 0 -- the gradient accumulator, so that the resumed run
        completes that step bit for bit.  A trainer with weight averaging
        adds 'ema': decay, warmup, n_updates and 'shadow', a clone of the
        average's arena."""
        self._not_swapped("state_dict()")
        sd = {"model": self.model.state_dict(), "optimizer": self.optimizer_state_dict(),
              "rng": self.rng_state()}
        if self.ctl_buf is not None:
            st = self.step_control_state()
            sd["step_control"] = {"schedule": self.lr_schedule.config() if self.lr_schedule is not None else None,
                                  "max_grad_norm": self.max_grad_norm, "n_clipped": st["n_clipped"],
                                  "n_skipped": st["n_skipped"], "accum_steps": self.accum_steps,
                                  "micro": st["micro"]}
            if st["micro"] > 0:
                sd["step_control"]["accum"] = self.acc.clone()
        if self.ema is not None:
            sd["ema"] = {"decay": self.ema_decay, "warmup": self.ema_warmup,
                         "n_updates": self.ema_state()["n_updates"], "shadow": self.ema.clone()}
        return sd

    def _load_ema(self, e):
        """the checkpoint's average, or -- a checkpoint without one -- the
        parameters just loaded"""
        if e is None:
            self.reset_ema()
            return
        shadow = e["shadow"].reshape(-1)
        if shadow.numel() != self.n:
            raise ValueError("the checkpoint's average has %d elements, the parameter arena %d"
                             % (shadow.numel(), self.n))
        self.set_ema_decay(e["decay"])
        self.ema_warmup = bool(e["warmup"])
        self._ema_field("warmup").fill_(int(self.ema_warmup))
        self._ema_field("n_updates").fill_(int(e["n_updates"]))
        with torch.no_grad():
            self.ema.copy_(shadow)

    def _load_step_control(self, sc):
        from .stepctl import StepSchedule, check_max_grad_norm
        if self.ctl_buf is None:
            if sc["schedule"] is not None or sc["max_grad_norm"] is not None:
                raise ValueError("the checkpoint carries a step control (%r); build the FlowTrainer with "
                                 "lr_schedule / max_grad_norm to resume it" % (sc,))
            return
        mgn = check_max_grad_norm(sc["max_grad_norm"])
        if mgn is not None and not self.clip:
            raise ValueError("the checkpoint clips at max_grad_norm=%g; build the FlowTrainer with max_grad_norm "
                             "to resume it" % mgn)
        self.lr_schedule = StepSchedule.from_config(sc["schedule"]) if sc["schedule"] is not None else None
        self.max_grad_norm = mgn
        self._write_ctl_config()
        self._ctl_field("n_clipped").fill_(int(sc["n_clipped"]))
        self._ctl_field("n_skipped").fill_(int(sc["n_skipped"]))
        if self.acc is not None:
            micro = int(sc.get("micro", 0))
            if not (0 <= micro < self.accum_steps) or (micro > 0) != ("accum" in sc):
                raise ValueError("the checkpoint's accumulation state is inconsistent (micro=%d)" % micro)
            self._ctl_field("micro").fill_(micro)
            if micro > 0:
                self.acc.copy_(sc["accum"].reshape(-1))
            else:
                self.acc.zero_()

    def load_state_dict(self, sd):
        # the accumulator's scale and the meaning of micro are accum_steps':
        # refused before anything is loaded
        sc = sd.get("step_control")
        k = int(sc.get("accum_steps", 1)) if sc is not None else 1
        if k != self.accum_steps:
            raise ValueError("the checkpoint was taken with accum_steps=%d, this FlowTrainer was built with "
                             "accum_steps=%d" % (k, self.accum_steps))
        self._not_swapped("load_state_dict()")
        if sd.get("ema") is not None and self.ema is None:
            raise ValueError("the checkpoint carries averaged weights (ema_decay=%r); build the FlowTrainer with "
                             "ema_decay to resume it" % (sd["ema"]["decay"],))
        with torch.no_grad():
            self.model.load_state_dict(sd["model"])
        self.load_optimizer_state_dict(sd["optimizer"])
        if sc is not None:
            self._load_step_control(sc)
        if self.ema is not None:
            self._load_ema(sd.get("ema"))
        rng = sd.get("rng")
        if rng is not None:
            # a checkpoint of THIS rank resumes its noise stream exactly; one
            # saved by another rank (usually rank 0 for all) restores only the
            # step counter, so every replica keeps drawing its own noise
            own = int(rng.get("rank", 0)) == self.rank
            if own and int(rng["seed"]) != self.seed:
                self.seed = int(rng["seed"])
                self.drop_graph()    # the seed is a captured launch argument
            self.step_t.fill_(int(rng["step"]))
            if self.noise_t is not None:
                self.noise_t.fill_(int(rng.get("noise_step", 0)))

    def reset_optimizer(self):
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        self.step_t.zero_()

    def reset_metrics(self):
        self.ll_acc.zero_()

    def mean_logll(self, steps):
        return float(self.ll_acc.item()) / max(steps, 1)

    def bits_per_dim(self, mean_ll):
        """train.py:203-204."""
        D = self.model.image_size ** 2 * self.model.channels
        return (-mean_ll + math.log(256.0) * D) / (D * math.log(2.0))
