"""The RealNVP multi-scale flow (flow_realnvp.py:196-327) as ONE program.

flow_schedule(model) is the forward op list of the reference's f: per scale
the checkerboard couplings, squeeze, the channelwise couplings, undo-squeeze
and factor-out, then the last scale's couplings and the restores.  The
inverse (the reference's g, the sampler, the trainer's backward over the
gradient buffers) is never written out: it is the reversed list with every op
replaced through INVERSE.

The drop-in model interprets the schedule functionally (run_functional);
FlowProgram gives it persistent buffers for the trainer, the evaluator and
the sampler.  The permutations run here, couplings stay with the caller.
"""
from typing import Any, NamedTuple

import torch

from . import _lib
from . import functions as Fn
from .engine import stream_ptr, weights_key, wn_table

COUPLING, REVERSE = "coupling", "reverse"
SQUEEZE, UNDO, FACTOR_OUT, RESTORE = "squeeze", "undo", "factor_out", "restore"
INVERSE = {COUPLING: REVERSE, REVERSE: COUPLING, SQUEEZE: UNDO, UNDO: SQUEEZE,
           FACTOR_OUT: RESTORE, RESTORE: FACTOR_OUT}


def flow_schedule(model):
    """[(kind, coupling module or None)] in the order of the reference's f."""
    ops = []
    for s in range(1, model.n_scales):
        ckbd, chan = model._scale_mods(s)
        ops += [(COUPLING, m) for m in ckbd]
        ops.append((SQUEEZE, None))
        ops += [(COUPLING, m) for m in chan]
        ops += [(UNDO, None), (FACTOR_OUT, None)]
    ops += [(COUPLING, m) for m in model._scale_mods(model.n_scales)[0]]
    ops += [(RESTORE, None)] * (model.n_scales - 1)
    return ops


def inverse_schedule(ops):
    return [(INVERSE[kind], mod) for kind, mod in reversed(ops)]


def run_functional(ops, coupling, *ts):
    """Interpret a schedule (or its inverse) with the autograd functions on
    the tensors ts, which all take the same permutations (f: z and the
    elementwise log-det); coupling(mod, *ts) -> ts runs a coupling.  The
    factored-out halves wait on a stack: a restore takes the latest."""
    offs = []
    for kind, mod in ops:
        if mod is not None:
            ts = coupling(mod, *ts)
        elif kind == SQUEEZE:
            ts = [Fn.squeeze(t) for t in ts]
        elif kind == UNDO:
            ts = [Fn.undo_squeeze(t) for t in ts]
        elif kind == FACTOR_OUT:
            halves = [Fn.factor_out(t) for t in ts]
            ts = [on for on, _ in halves]
            offs.append([off for _, off in halves])
        else:
            ts = [Fn.restore(t, off) for t, off in zip(ts, offs.pop())]
    return ts


# Stage records: plain tuples with names, kind first.
class Coupling(NamedTuple):
    kind: str
    mod: Any
    eng: Any
    x: torch.Tensor
    z: torch.Tensor
    saved: Any
    block: Any      # the coupling's slice of the gradient arena (trainer), else None


class Reshape(NamedTuple):      # squeeze: a [B,C,H,W] -> b [B,4C,H/2,W/2]; undo: the other way
    kind: str
    a: torch.Tensor
    b: torch.Tensor


class FactorOut(NamedTuple):
    kind: str
    a: torch.Tensor
    on: torch.Tensor
    off: torch.Tensor


class Restore(NamedTuple):
    kind: str
    on: torch.Tensor
    off: torch.Tensor
    full: torch.Tensor


def inverse_perm(st, buf=lambda t: t):
    """The inverse of a permutation stage over buf(t) for each of its tensors."""
    kind = INVERSE[st.kind]
    if st.kind in (SQUEEZE, UNDO):
        return Reshape(kind, buf(st.b), buf(st.a))
    if st.kind == FACTOR_OUT:
        return Restore(kind, buf(st.on), buf(st.off), buf(st.a))
    return FactorOut(kind, buf(st.full), buf(st.on), buf(st.off))


def run_perm(st):
    """Launch a permutation stage (B, C, H, W are the unsqueezed / whole side's)."""
    L = _lib.lib()
    s = stream_ptr()
    if st.kind == SQUEEZE:
        L.squeeze(st.a.data_ptr(), st.b.data_ptr(), *st.a.shape, s)
    elif st.kind == UNDO:
        L.undo_squeeze(st.a.data_ptr(), st.b.data_ptr(), *st.b.shape, s)
    elif st.kind == FACTOR_OUT:
        L.factor_out(st.a.data_ptr(), st.on.data_ptr(), st.off.data_ptr(), *st.a.shape, s)
    else:
        L.restore(st.on.data_ptr(), st.off.data_ptr(), st.full.data_ptr(), *st.full.shape, s)


class FlowProgram:
    """The schedule with persistent fp32 buffers for one batch size: an output
    per coupling, sq / un / on / off per scale, a full per restore.  x is the
    flow's input, z its output, stages the records in forward order.
    alloc(mod, x) -> (engine, saved activations, gradient block) replaces the
    coupling allocation (the trainer adds its gradient block)."""

    def __init__(self, model, batch, device, dtype, training, alloc=None):
        self.dtype, self.dev, self.training = dtype, device, training
        alloc = alloc or self._alloc
        B, c, s = batch, model.channels, model.image_size
        f32 = dict(device=device, dtype=torch.float32)
        self.x = cur = torch.empty(B, c, s, s, **f32)
        self.stages = []
        offs = []
        for kind, mod in flow_schedule(model):
            # every record's tensors: what it reads, then what it writes
            if kind == COUPLING:
                eng, saved, block = alloc(mod, cur)
                st = Coupling(kind, mod, eng, cur, torch.empty_like(cur), saved, block)
                cur = st.z
            elif kind == SQUEEZE:
                st = Reshape(kind, cur, torch.empty(B, 4 * c, s // 2, s // 2, **f32))
                cur = st.b
            elif kind == UNDO:
                st = Reshape(kind, cur, torch.empty(B, c, s, s, **f32))
                cur = st.b
            elif kind == FACTOR_OUT:
                c, s = 2 * c, s // 2
                st = FactorOut(kind, cur, torch.empty(B, c, s, s, **f32), torch.empty(B, c, s, s, **f32))
                offs.append(st.off)
                cur = st.on
            else:
                c, s = c // 2, 2 * s
                st = Restore(kind, cur, offs.pop(), torch.empty(B, c, s, s, **f32))
                cur = st.full
            self.stages.append(st)
        self.z = cur
        self.couplings = [st for st in self.stages if st.kind == COUPLING]

    def _alloc(self, mod, x):
        eng = mod.engine()
        return eng, eng.alloc_saved(x.shape[0], x.shape[2], x.shape[3], self.dtype, self.dev, self.training), None

    def forward(self, coupling):
        """Walk the program; coupling(k, stage) runs the k-th coupling."""
        k = 0
        for st in self.stages:
            if st.kind == COUPLING:
                coupling(k, st)
                k += 1
            else:
                run_perm(st)

    def inverse(self, coupling, buf=lambda t: t):
        """Walk the inverse program, last stage first; the permutations'
        inverses run over buf(t) (the identity: the sampler; a gradient
        buffer per tensor: the trainer's backward)."""
        k = len(self.couplings)
        for st in reversed(self.stages):
            if st.kind == COUPLING:
                k -= 1
                coupling(k, st)
            else:
                run_perm(inverse_perm(st, buf))


# What FlowEvaluator and FlowSampler share around their programs.
def current_wn_table(engines, dtype, dev, key, table):
    """(table, key, moved): the weight-norm table over these couplings,
    rebuilt when their packed-weight arenas moved since `key` was taken (the
    table, and a graph captured with it, hold raw arena pointers)."""
    k = weights_key(engines, dtype)
    if k == key:
        return table, key, False
    return wn_table(engines, dtype, dev), k, True


def capture_graph(run):
    """run() once on a side stream, then captured into a HIP graph."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        run()
    torch.cuda.synchronize()
    return graph
