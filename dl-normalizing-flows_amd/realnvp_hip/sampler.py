"""Graph-replayed generation: RealNVP.sample(n) followed by
logit_transform(reverse=True), as train.py:253-259 draws its 100 samples
(flow_realnvp.py:342-352 -> g, 196-249; utils.py:34-42).

Eval mode (BatchNorm running statistics), so every buffer has a fixed
shape: z, the factor-out halves, each coupling's saved activations and the
output are allocated once, the N(0,1) draw, the weight-norm refresh (two
launches for the whole model) and every inverse kernel are captured into one
HIP graph and replayed per call.
"""
import torch

from . import _lib
from .engine import stream_ptr, weights_key, wn_forward, wn_table
from .program import FlowProgram, capture_graph, current_wn_table


class FlowSampler:
    def __init__(self, model, n, dtype=None, logit_reverse=True, constraint=0.9, graph=True):
        if model.training:
            raise RuntimeError("FlowSampler samples in eval mode (train.py:253-259 runs after model.eval())")
        self.model = model
        self.dev = next(model.parameters()).device
        if self.dev.type != "cuda":
            raise RuntimeError("FlowSampler needs the model on a HIP device")
        self.n = n
        self.dtype = dtype or next(model.couplings()).compute_dtype
        self.logit_reverse, self.constraint = logit_reverse, constraint
        C, S = model.channels, model.image_size
        self.out = torch.empty(n, C, S, S, device=self.dev, dtype=torch.float32)
        # the inverse view of the forward flow program (program.py): its output is
        # the latent to invert, its input the sample
        self.program = FlowProgram(model, n, self.dev, self.dtype, False)
        self.z, self.x = self.program.z, self.program.x
        self.engines = list(dict.fromkeys(st.eng for st in reversed(self.program.couplings)))
        self.table = wn_table(self.engines, self.dtype, self.dev)
        self._wkey = weights_key(self.engines, self.dtype)
        self.graph = None
        self.use_graph = graph
        if graph:
            self._capture()

    def _check_weights(self):
        """The weight-norm table (and the graph) follow parameters that moved
        since capture: the old arena has been freed (e.g. a FlowTrainer built
        after this sampler re-pointed the parameters into its flat arena)."""
        self.table, self._wkey, moved = current_wn_table(self.engines, self.dtype, self.dev, self._wkey, self.table)
        if moved:
            self.graph = None
            if self.use_graph:
                self._capture()

    def _run(self, draw=True):
        L = _lib.lib()
        s = stream_ptr()
        if draw:
            self.z.normal_()      # prior N(0, 1) (flow_realnvp.py:342-352)
        if self.table is not None:
            wn_forward(self.table, self.dtype)
        self.program.inverse(lambda k, st: st.eng.reverse(st.z, False, self.dtype, saved=st.saved, out=st.x,
                                                          want_ldj=False, prepare=False))
        if self.logit_reverse:
            L.logit_inv(self.x.data_ptr(), self.out.data_ptr(), float(self.constraint), self.x.numel(), s)
        else:
            self.out.copy_(self.x)

    def _capture(self):
        self.graph = capture_graph(self._run)

    def sample(self, z=None):
        """n images in [0, 1] (or the flow's x when logit_reverse=False).
        z: an optional [n, C, H, W] latent to invert instead of a fresh draw
        (eager path; used by the parity test)."""
        self._check_weights()
        if z is not None:
            with torch.no_grad():
                self.z.copy_(z)
                self._run(draw=False)
            return self.out
        if self.graph is not None:
            self.graph.replay()
        else:
            self._run()
        return self.out
