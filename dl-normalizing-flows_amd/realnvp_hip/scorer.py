"""Per-image log-likelihoods on the device (include/realnvp_hip.h, "scoring").

The reference's validation loop (train.py:95-100, 214-233) scores every
image of a loader without drop_last and keeps only a mean.  ``FlowScorer``
keeps the values: one fp32 score per image (nats), for ranking, outlier
detection and per-class statistics, over batches of 1..B rows, optionally as
the K-draw bound log(1/K sum_k p(x + u_k)) over K draws of the uniform
dequantisation noise (n_draws = 1 is the reference's one-draw bound).

It is built like ``FlowEvaluator``: eval mode, one forward ``FlowProgram``,
the weight-norm refresh once per pass.  One captured graph is ONE draw of one
batch -- rnvp_score_in_fwd, the flow forward with per-sample log-det,
rnvp_score_finish -- and is replayed K times per batch.  Everything that
changes between replays (the destination, the running global index, the draw,
the number of valid rows) lives in a device-resident ``rnvp_score_ctl`` block
that the kernels advance themselves and the host only writes with
stream-ordered copies: no re-capture for a ragged last batch or another
capacity, and no host synchronisation until the results are read.

The noise of an image is keyed by its global index in the pass and the draw,
not by its batch slot: the scores do not depend on the batch size.
"""
import ctypes as C
import math

import torch

from . import _lib
from .engine import stream_ptr, upload, weights_key, wn_forward, wn_table
from .program import FlowProgram, capture_graph, current_wn_table


def check_n_draws(k):
    """noise draws per image: an int >= 1"""
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError("n_draws must be an int >= 1, got %r" % (k,))
    return k


def mean_of_batch_means(scores, batch_size):
    """The reference's statistic (train.py:214-233) from per-image scores in
    loader order: the mean over batches of per-batch means, the last batch
    over its own rows.  float64 on the scores' device; a Python float."""
    s = scores.detach().double().flatten()
    n, B = s.numel(), int(batch_size)
    if n == 0:
        raise ValueError("mean_of_batch_means of no scores")
    full = n // B
    means = [s[:full * B].view(full, B).mean(dim=1)]
    if n > full * B:
        means.append(s[full * B:].mean().reshape(1))
    return float(torch.cat(means).mean())


def bits_per_dim(ll, D):
    """train.py:230 on a mean (float) or on per-image scores (tensor)"""
    return (-ll + math.log(256.0) * D) / (D * math.log(2.0))


class FlowScorer:
    def __init__(self, model, batch_size, n_draws=1, dtype=None, constraint=0.9, seed=0, graph=True):
        self.K = check_n_draws(n_draws)
        if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
            raise ValueError("batch_size must be an int >= 1, got %r" % (batch_size,))
        self.dev = next(model.parameters()).device
        if self.dev.type != "cuda":
            raise RuntimeError("FlowScorer needs the model on a HIP device")
        if model.training:
            raise RuntimeError("FlowScorer scores in eval mode (train.py:214-233 runs after model.eval())")
        self.model = model
        self.B = batch_size
        self.dtype = dtype or next(model.couplings()).compute_dtype
        self.constraint, self.seed = constraint, seed
        Cc, S = model.channels, model.image_size
        self.D = Cc * S * S
        f32 = dict(device=self.dev, dtype=torch.float32)
        self.pix = torch.zeros(batch_size, Cc, S, S, **f32)
        self.noise = torch.zeros(batch_size, Cc, S, S, **f32)     # explicit noise of one draw (eager path)
        # rnvp_score_in_fwd adds into logdet, the couplings into ldj; rnvp_score_finish leaves both zero
        self.logdet = torch.zeros(batch_size, **f32)
        self.ldj = torch.zeros(batch_size, **f32)
        self.run = torch.zeros(batch_size, 2, **f32)
        self.lp = torch.empty(batch_size, **f32)                  # the last draw's log-likelihoods
        self.ctl_buf = upload(bytes(_lib.ScoreCtl()), self.dev)
        self._scores = None
        self._n_valid = None        # what the block's n_valid holds
        self.capacity = self.n_added = 0
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

    def _field(self, name):
        """a one-element tensor view of a field of the control block"""
        f = getattr(_lib.ScoreCtl, name)
        dt = {C.c_int: torch.int32, C.c_longlong: torch.int64}[dict(_lib.ScoreCtl._fields_)[name]]
        return self.ctl_buf[f.offset:f.offset + f.size].view(dt)

    def _draw(self, noise=None):
        """one noise draw of the batch in self.pix: the block's draw and first say which"""
        L = _lib.lib()
        s = stream_ptr()
        ctl = self.ctl_buf.data_ptr()
        L.score_in_fwd(self.pix.data_ptr(), noise.data_ptr() if noise is not None else None, self.seed, ctl,
                       float(self.constraint), self.xl.data_ptr(), self.logdet.data_ptr(), *self.pix.shape, s)
        self.program.forward(lambda k, st: st.eng.forward(st.x, False, self.dtype, False, saved=st.saved,
                                                          prepare=False, ldj_sample=self.ldj, z_out=st.z))
        L.score_finish(self.z.data_ptr(), self.ldj.data_ptr(), self.logdet.data_ptr(), self.run.data_ptr(),
                       self.lp.data_ptr(), ctl, self.B, self.D, s)

    def _capture(self):
        # capture_graph runs a draw for real before it records one: the block goes back afterwards (the
        # accumulators are zero again and run restarts in draw 0 by themselves)
        snap = self.ctl_buf.clone()
        self.graph = capture_graph(self._draw)
        self.ctl_buf.copy_(snap)

    def begin(self, capacity):
        """Start a pass of at most `capacity` images: refresh the packed
        weights, a fresh destination, the block back at image 0.  Stream-
        ordered; a captured graph is kept."""
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError("capacity must be >= 1, got %r" % (capacity,))
        self._check_weights()
        if self.table is not None:
            wn_forward(self.table, self.dtype)
        self._scores = torch.empty(capacity, device=self.dev, dtype=torch.float32)
        self.capacity, self.n_added, self._n_valid = capacity, 0, self.B
        blk = _lib.ScoreCtl(self._scores.data_ptr(), capacity, 0, 0, 0.0, self.B, self.K, 0, 0)
        self.ctl_buf.copy_(upload(bytes(blk), self.dev))

    def add_batch(self, pix, noise=None):
        """1..B images of raw pixels in [0, 1] ([rows, C, S, S]); the rest of
        the batch is zero-filled and scores nothing.  noise: explicit
        dequantisation noise [K, rows, C, S, S] in [0, 1) instead of the
        Philox draws (eager path)."""
        if self._scores is None:
            raise RuntimeError("FlowScorer.add_batch before begin(capacity)")
        rows = pix.shape[0] if pix.dim() == 4 else -1
        if not (1 <= rows <= self.B) or tuple(pix.shape[1:]) != tuple(self.pix.shape[1:]):
            raise ValueError("FlowScorer batch is 1..%d x %s, got %s"
                             % (self.B, tuple(self.pix.shape[1:]), tuple(pix.shape)))
        if noise is not None and tuple(noise.shape) != (self.K,) + tuple(pix.shape):
            raise ValueError("FlowScorer noise is %s, got %s" % ((self.K,) + tuple(pix.shape), tuple(noise.shape)))
        if self.n_added + rows > self.capacity:
            raise RuntimeError("FlowScorer: more than the %d images begin() made room for" % self.capacity)
        with torch.no_grad():
            self.pix[:rows].copy_(pix)
            if rows < self.B:
                self.pix[rows:].zero_()
            if rows != self._n_valid:
                self._field("n_valid").fill_(rows)
                self._n_valid = rows
            for k in range(self.K):
                if noise is not None:
                    self.noise[:rows].copy_(noise[k])
                    self._draw(self.noise)
                elif self.use_graph:
                    if self.graph is None:
                        self._capture()
                    self.graph.replay()
                else:
                    self._draw()
        self.n_added += rows

    def _state(self):
        """the block, read back (synchronises); raises when the pass overflowed"""
        if self._scores is None:
            raise RuntimeError("FlowScorer: no pass yet (begin / score)")
        c = _lib.ScoreCtl.from_buffer_copy(bytes(self.ctl_buf.cpu().numpy()))
        if c.overflow:
            raise RuntimeError("FlowScorer: the pass scored more than its capacity of %d images" % c.cap)
        return c

    def scores(self):
        """fp32 device tensor [N]: the log-likelihood (K-draw bound) of every
        image added so far, in order, nats per image.  Synchronises."""
        return self._scores[:int(self._state().n_scored)]

    def mean_logll(self, batch_mean=False):
        """The per-image mean ll_sum / n_scored, or with batch_mean the
        reference's mean over batches of per-batch means (the two differ when
        the last batch is ragged).  Synchronises."""
        c = self._state()
        if c.n_scored < 1:
            raise RuntimeError("FlowScorer: no image scored yet")
        if batch_mean:
            return mean_of_batch_means(self._scores[:int(c.n_scored)], self.B)
        return c.ll_sum / c.n_scored

    def bits_per_dim(self, per_image=False, batch_mean=False):
        """train.py:230 on the mean (a float), or per image (fp32 device tensor [N])"""
        if per_image:
            return bits_per_dim(self.scores(), self.D)
        return bits_per_dim(self.mean_logll(batch_mean=batch_mean), self.D)

    def score(self, batches, capacity=None):
        """A full pass over an iterable of pixel batches (or (pixels, target)
        pairs), the last one ragged, e.g. data.DeviceLoader(valid_set, B, dev,
        shuffle=False); returns scores().  capacity: an upper bound of the
        number of images; by default the loader's dataset size, or else a
        first pass over the batches' sizes."""
        def pixels(b):
            return b[0] if isinstance(b, (tuple, list)) else b
        if capacity is None:
            loader = getattr(batches, "loader", batches)
            if hasattr(loader, "dataset"):
                capacity = len(loader.dataset)
            else:
                batches = list(batches)
                capacity = sum(int(pixels(b).shape[0]) for b in batches)
        self.begin(capacity)
        for b in batches:
            self.add_batch(pixels(b))
        return self.scores()
