"""Validation loop of the training script (train.py:214-233) on the device.

Per batch the reference runs, in eval mode under no_grad:
    x, logdet = logit_transform(x); logll, weight_scale = model(x)
    logll = (logll + logdet).mean(); running_logll += logll.item()
and reports bits/dim = (-mean_logll + ln 256 * D) / (D ln 2) over the batches.

``FlowEvaluator`` holds persistent eval-mode buffers for one batch size (BN
running statistics, so every shape is fixed) and captures logit transform
(device Philox noise, a fresh counter per batch), the forward flow with
per-sample log-det accumulation, the N(0, 1) prior and the running sum into
one HIP graph; the host reads the sum once per pass instead of once per batch
(the reference's per-batch .item()).  The weight-norm refresh runs once per
pass (weights do not change inside a validation loop).
"""
import math

import torch

from . import _lib
from .engine import stream_ptr, weights_key, wn_forward, wn_table
from .program import FlowProgram, capture_graph, current_wn_table


class FlowEvaluator:
    def __init__(self, model, batch_size, dtype=None, constraint=0.9, seed=0, graph=True):
        self.model = model
        self.dev = next(model.parameters()).device
        if self.dev.type != "cuda":
            raise RuntimeError("FlowEvaluator needs the model on a HIP device")
        self.B = batch_size
        self.dtype = dtype or next(model.couplings()).compute_dtype
        self.constraint, self.seed = constraint, seed
        C, S = model.channels, model.image_size
        f32 = dict(device=self.dev, dtype=torch.float32)
        self.pix = torch.zeros(batch_size, C, S, S, **f32)
        self.logdet = torch.empty(batch_size, **f32)
        self.ldj = torch.zeros(batch_size, **f32)
        self.lp = torch.empty(batch_size, **f32)
        self.ll_sum = torch.zeros(1, dtype=torch.float64, device=self.dev)
        self.counter = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self.n_batches = 0
        # the forward flow program (program.py) in eval mode, per-sample log-det accumulation
        self.program = FlowProgram(model, batch_size, self.dev, self.dtype, False)
        self.xl, self.z = self.program.x, self.program.z
        self.engines = list(dict.fromkeys(st.eng for st in self.program.couplings))
        self.table = wn_table(self.engines, self.dtype, self.dev)
        self._wkey = weights_key(self.engines, self.dtype)
        self.graph = None
        self.use_graph = graph

    def _check_weights(self):
        """The weight-norm table follows parameters that moved since it was
        built; a graph captured with the old one is dropped."""
        self.table, self._wkey, moved = current_wn_table(self.engines, self.dtype, self.dev, self._wkey, self.table)
        if moved:
            self.graph = None

    def _batch(self):
        L = _lib.lib()
        s = stream_ptr()
        B = self.B
        n = self.pix[0].numel()
        L.logit_fwd(self.pix.data_ptr(), None, self.seed, 0, self.counter.data_ptr(), float(self.constraint),
                    self.xl.data_ptr(), self.logdet.data_ptr(), B, n, s)
        self.ldj.zero_()
        self.program.forward(lambda k, st: st.eng.forward(st.x, False, self.dtype, False, saved=st.saved,
                                                          prepare=False, ldj_sample=self.ldj, z_out=st.z))
        L.prior_logprob(self.z.data_ptr(), self.ldj.data_ptr(), self.lp.data_ptr(), B, self.z[0].numel(), s)
        self.ll_sum += (self.lp + self.logdet).mean().double()
        L.step_increment(self.counter.data_ptr(), s)

    def _capture(self):
        snap = (self.ll_sum.clone(), self.counter.clone())
        self.graph = capture_graph(self._batch)
        self.ll_sum.copy_(snap[0])
        self.counter.copy_(snap[1])

    def begin(self):
        """Start a validation pass: refresh the packed weights, zero the sum."""
        self._check_weights()
        if self.table is not None:
            wn_forward(self.table, self.dtype)
        self.ll_sum.zero_()
        self.n_batches = 0

    def add_batch(self, pix):
        """One validation batch of raw pixels in [0, 1] ([B, C, S, S])."""
        if tuple(pix.shape) != tuple(self.pix.shape):
            raise ValueError("FlowEvaluator batch is %s, got %s" % (tuple(self.pix.shape), tuple(pix.shape)))
        with torch.no_grad():
            self.pix.copy_(pix)
            if self.use_graph:
                if self.graph is None:
                    self._capture()
                self.graph.replay()
            else:
                self._batch()
        self.n_batches += 1

    def mean_logll(self):
        """running_logll / n_batches (one host read per pass)."""
        return float(self.ll_sum.item()) / max(self.n_batches, 1)

    def bits_per_dim(self, mean_ll=None):
        """train.py:230."""
        if mean_ll is None:
            mean_ll = self.mean_logll()
        D = self.model.image_size ** 2 * self.model.channels
        return (-mean_ll + math.log(256.0) * D) / (D * math.log(2.0))

    def evaluate(self, batches):
        """A full validation pass over an iterable of pixel batches (e.g.
        data.DeviceLoader(valid_set, B, dev, drop_last=True)); returns
        (mean log-likelihood, bits/dim)."""
        self.begin()
        for pix in batches:
            if isinstance(pix, (tuple, list)):
                pix = pix[0]
            self.add_batch(pix)
        ll = self.mean_logll()
        return ll, self.bits_per_dim(ll)
