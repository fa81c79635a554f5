"""The callers of the flow program (realnvp_hip/program.py) on the device: the
coupling and permutation launches of the unchained trainer, the evaluator and
the sampler follow the schedule literals of test_flow_program_cpu.py, and the
evaluator and the sampler agree with the drop-in model."""
import numpy as np
import pytest
import torch

from formula_init import formula_state, pixels
from test_flow_program_cpu import f_literal, g_literal

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, CH, SIZE, N_SCALES = 4, 3, 32, 5
PERMS = ("squeeze", "undo_squeeze", "factor_out", "restore")
KEPT = ("coupling_in_fwd", "coupling_reverse", "coupling_out_bwd") + PERMS


def make_model():
    import flow_realnvp
    import utils
    prior = torch.distributions.Normal(torch.tensor(0.0, device=DEV), torch.tensor(1.0, device=DEV))
    m = flow_realnvp.RealNVP(CH, SIZE, prior, utils.Hyperparameters(8, 1, True, True, True, True))
    m.load_state_dict(formula_state(m))
    return m.to(DEV)


def record(monkeypatch):
    """wrap the kept entry points of the library object (every launch looks
    them up there when it runs); the permutations keep their B, C, H, W"""
    from realnvp_hip import _lib
    L = _lib.lib()
    trace = []
    for name in KEPT:
        def rec(*args, _fn=getattr(L, name), _name=name):
            trace.append((_name,) + tuple(args[-5:-1]) if _name in PERMS else _name)
            return _fn(*args)
        monkeypatch.setattr(L, name, rec)
    return trace


def launches(kinds, coupling, swap=False, size=SIZE):
    """A kind literal -> the launch literal: `coupling` per coupling, the
    permutations with the shape of their whole / unsqueezed side.  swap: every
    permutation's inverse entry point instead (the backward of that op)."""
    entry = {"squeeze": "squeeze", "undo": "undo_squeeze", "factor_out": "factor_out", "restore": "restore"}
    if swap:
        entry = {"squeeze": "undo_squeeze", "undo": "squeeze", "factor_out": "restore", "restore": "factor_out"}
    c, s = CH, size
    out = []
    for k in kinds:
        if k in ("coupling", "reverse"):
            out += coupling
            continue
        if k == "restore":
            c, s = c // 2, s * 2
        out.append((entry[k], B, c, s, s))
        if k == "factor_out":
            c, s = c * 2, s // 2
    return out


def test_launch_literal_at_two_scales():
    """the derivation above, spelled out once by hand (3 x 8 x 8, 2 scales)"""
    assert launches(f_literal(2), ["c"], size=8) == [
        "c", "c", "c", ("squeeze", 4, 3, 8, 8), "c", "c", "c", ("undo_squeeze", 4, 3, 8, 8),
        ("factor_out", 4, 3, 8, 8), "c", "c", "c", "c", ("restore", 4, 3, 8, 8)]


def test_unchained_trainer_launches_follow_the_schedule(monkeypatch):
    from realnvp_hip.trainer import FlowTrainer
    tr = FlowTrainer(make_model(), B, dtype="fp32", chain=False)
    assert tr.links is None
    tr.set_pixels(pixels(B, CH, SIZE, seed=2).to(DEV))
    trace = record(monkeypatch)
    tr.step_eager()
    torch.cuda.synchronize()
    fwd = launches(f_literal(N_SCALES), ["coupling_in_fwd"])
    bwd = launches(f_literal(N_SCALES), ["coupling_out_bwd"], swap=True)[::-1]
    assert trace == fwd + bwd


def test_chained_trainer_launches_no_permutation(monkeypatch):
    from realnvp_hip.trainer import FlowTrainer
    tr = FlowTrainer(make_model(), B, dtype="fp32", chain=True)
    assert tr.links is not None
    # an already transformed batch: the first coupling's in part is then a launch of its own
    tr.set_input(torch.randn(B, CH, SIZE, SIZE, generator=torch.Generator().manual_seed(2)).to(DEV),
                 torch.zeros(B, device=DEV))
    trace = record(monkeypatch)
    tr.step_eager()
    torch.cuda.synchronize()
    assert "coupling_in_fwd" in trace                   # the recorder sees this step
    assert not [t for t in trace if isinstance(t, tuple)]


def test_evaluator_launches_and_log_likelihood(monkeypatch):
    from realnvp_hip import _lib
    from realnvp_hip.engine import stream_ptr
    from realnvp_hip.evaluator import FlowEvaluator
    model = make_model()
    model.train()
    with torch.no_grad():   # move the running statistics off their defaults
        model(torch.rand(8, CH, SIZE, SIZE, device=DEV) * 2 - 1)
    model.eval()
    seed = 123
    pix = pixels(B, CH, SIZE, seed=3).to(DEV)
    ev = FlowEvaluator(model, B, seed=seed, graph=False)
    ev.begin()
    trace = record(monkeypatch)
    ev.add_batch(pix)
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert trace == launches(f_literal(N_SCALES), ["coupling_in_fwd"])
    # the batch's log-likelihood against model.log_prob on the same dequantised batch
    ll = ev.mean_logll()
    n = CH * SIZE * SIZE
    x, logdet = torch.empty_like(pix), torch.empty(B, device=DEV)
    _lib.lib().logit_fwd(pix.data_ptr(), None, seed, 0, None, 0.9, x.data_ptr(), logdet.data_ptr(), B, n,
                         stream_ptr())
    with torch.no_grad():
        ref = float((model.log_prob(x) + logdet).mean())
    print("evaluator ll %.9g  model.log_prob %.9g" % (ll, ref))
    assert abs(ll - ref) <= 1e-5 * abs(ref), (ll, ref)      # test_evaluator_matches_dropin_eval_loop's


def test_sampler_launches_and_sample(monkeypatch):
    from realnvp_hip.sampler import FlowSampler
    model = make_model().eval()
    z = torch.randn(B, CH, SIZE, SIZE, generator=torch.Generator().manual_seed(4)).to(DEV)
    s = FlowSampler(model, B, logit_reverse=False, graph=False)
    trace = record(monkeypatch)
    x = s.sample(z).clone()
    torch.cuda.synchronize()
    monkeypatch.undo()
    # a coupling's inverse: its in part, then the reverse kernel
    assert trace == launches(g_literal(N_SCALES), ["coupling_in_fwd", "coupling_reverse"])
    with torch.no_grad():
        ref = model.g(z)
    x, ref = x.cpu().numpy(), ref.cpu().numpy()
    rel = np.linalg.norm(x - ref) / np.linalg.norm(ref)
    print("sampler vs model.g: relative L2 %.3g" % rel)
    assert rel < 1e-4, rel                                   # test_sampler_matches_reference_g's
