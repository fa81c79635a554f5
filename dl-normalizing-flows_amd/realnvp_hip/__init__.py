"""MI355X-native RealNVP coupling-layer engine (host side).

Layout:
  _lib.py        ctypes binding of include/realnvp_hip.h (librealnvp_hip.so)
  net.py         the s/t ResNet as a conv program (forward + derived backward)
  engine.py      per-coupling executor (workspaces, kernel sequencing)
  functions.py   autograd Functions for the drop-in modules
  program.py     the multi-scale flow as one schedule; its inverse is derived
  trainer.py     fused NLL training step (flat parameter arena, fused Adam,
                 HIP-graph capture, RCCL data parallelism)
  optim.py       FusedAdam: torch.optim.Adam drop-in for the reference loop
  scorer.py      FlowScorer: per-image log-likelihoods (ragged batches, K-draw bound)
  codec.py       FlowCodec: encode, decode, temperature sampling, interpolation
"""
from ._lib import LIB_PATH, lib  # noqa: F401
from .optim import FusedAdam  # noqa: F401
from .scorer import FlowScorer  # noqa: F401
from .codec import FlowCodec  # noqa: F401
