"""In-graph weight averaging (include/realnvp_hip.h, "weight averaging":
rnvp_ema_update, rnvp_ema_swap) at the ABI level on raw tensors, then
FlowTrainer(ema_decay=d) on the m32_d8_r1 model at B = 4 (bf16: the step is
deterministic, so two trainers can be compared bit for bit)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from formula_init import formula_state, pixels, uniform_noise

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32_1 = 2e-7          # one fp32 rounding of a value computed in fp64 (2^-24 = 6e-8), with margin
FULL = 4 * 256 * 2048      # one sweep of the capped grid (2048 workgroups of 256 threads, a granule each)
# ... + 4: thread 0 alone has a second granule; 4 * FULL + 4: the loop over 4 granules per thread runs twice
SIZES = [4, 1028, FULL + 4, 1_000_004, 4 * FULL + 4]
US = [1, 9, 8990, 10 ** 6]


def L():
    from realnvp_hip import _lib
    return _lib.lib()


def sptr():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------ helpers
def make_ectl(decay, warmup, applied=-1.0, n_updates=0):
    """a device rnvp_ema_ctl block (uint8 tensor)"""
    from realnvp_hip._lib import EmaCtl
    c = EmaCtl(decay, int(warmup), applied, 0, n_updates)
    return torch.frombuffer(bytearray(bytes(c)), dtype=torch.uint8).to(DEV)


def read_ectl(t):
    from realnvp_hip._lib import EmaCtl
    return EmaCtl.from_buffer_copy(bytes(t.cpu().numpy()))


def make_ctl(skip, accum_steps=1):
    """a device rnvp_step_ctl block with the skip field set"""
    from realnvp_hip._lib import StepCtl
    from realnvp_hip.stepctl import fill_ctl
    c = fill_ctl(StepCtl(), 1e-3, None, None, accum_steps=accum_steps)
    c.skip = skip
    return torch.frombuffer(bytearray(bytes(c)), dtype=torch.uint8).to(DEV)


def arenas(n, seed):
    """parameters and average: randn times a per-1024-block scale from {1e-3,
    1, 1e3}; a tenth of the average's elements equal their parameter"""
    gen = torch.Generator().manual_seed(seed)
    nb = (n + 1023) // 1024

    def scaled():
        sc = torch.tensor([1e-3, 1.0, 1e3])[torch.randint(0, 3, (nb,), generator=gen)]
        return torch.randn(n, generator=gen) * sc.repeat_interleave(1024)[:n]
    p, e = scaled(), scaled()
    eq = torch.rand(n, generator=gen) < 0.1
    if n <= 8:
        eq[0] = True
    e[eq] = p[eq]
    return e, p, eq


def ema_update(e, p, ectl, step, step_add, ctl=None):
    st = torch.full((1,), step, device=DEV, dtype=torch.int64)
    L().ema_update(e.data_ptr(), p.data_ptr(), e.numel(), ectl.data_ptr(), st.data_ptr(), step_add,
                   ctl.data_ptr() if ctl is not None else None, sptr())
    torch.cuda.synchronize()
    assert int(st.item()) == step


def host_update(e, p, applied):
    """e + om * (p - e), three separately rounded fp32 operations on the host"""
    om = torch.tensor(np.float32(1.0) - np.float32(applied), dtype=torch.float32)
    diff = p - e
    inc = om * diff
    return e + inc


# ------------------------------------------------------------------- kernel
@pytest.mark.parametrize("warmup", [True, False], ids=["warmup", "nowarmup"])
@pytest.mark.parametrize("n", SIZES)
def test_applied_update(n, warmup):
    from realnvp_hip.stepctl import ema_decay_at
    assert L().grad_sumsq_parts(FULL) == 2048     # (the averaging kernels take the norm pass's grid)
    decay = 0.999
    e0, p0, eq = arenas(n, seed=n % 1000 + int(warmup))
    p = p0.to(DEV)
    for k, u in enumerate(US if n <= FULL + 4 else US[:2]):
        e = e0.to(DEV)
        ectl = make_ectl(decay, warmup, n_updates=7)
        # the counter before (step_add = 1) or after (step_add = 0) it has moved
        step, add = (u - 1, 1) if k % 2 == 0 else (u, 0)
        ema_update(e, p, ectl, step, add)
        c = read_ectl(ectl)
        want_d = ema_decay_at(decay, warmup, u)
        print("n=%d u=%d warmup=%d: applied %.9g, float64 %.17g" % (n, u, warmup, c.applied, want_d))
        np.testing.assert_allclose(c.applied, want_d, rtol=F32_1)
        assert c.n_updates == 8 and c.decay == np.float32(decay) and c.warmup == int(warmup) and c.pad == 0
        want = host_update(e0, p0, c.applied).to(DEV)
        assert same_bits(e, want), int((bits(e) != bits(want)).sum())
        assert same_bits(p, p0.to(DEV))
        assert same_bits(e[eq.to(DEV)], e0[eq].to(DEV)) and bool(eq.any())
        assert not same_bits(e, e0.to(DEV))
        # a second run from the same inputs
        e2, ectl2 = e0.to(DEV), make_ectl(decay, warmup, n_updates=7)
        ema_update(e2, p, ectl2, step, add)
        assert same_bits(e2, e) and bytes(read_ectl(ectl2)) == bytes(c)


@pytest.mark.parametrize("n", SIZES)
def test_decay_zero_copies_the_parameters(n):
    """d == 0 stores the parameter itself (e + (p - e) would be p only where
    the subtraction is exact: the arenas mix scales from 1e-3 to 1e3)"""
    e0, p0, _ = arenas(n, seed=3)
    e, p, ectl = e0.to(DEV), p0.to(DEV), make_ectl(0.0, False, applied=0.5)
    ema_update(e, p, ectl, 0, 1)
    c = read_ectl(ectl)
    assert c.applied == 0.0 and c.n_updates == 1
    assert same_bits(e, p) and same_bits(p, p0.to(DEV))
    if n >= 1028:
        assert not same_bits(host_update(e0, p0, 0.0), p0)
    # min(0, (1 + u) / (10 + u)) is 0 as well
    e, ectl = e0.to(DEV), make_ectl(0.0, True)
    ema_update(e, p, ectl, 0, 1)
    assert read_ectl(ectl).applied == 0.0 and same_bits(e, p)


@pytest.mark.parametrize("n", SIZES)
def test_skipped_step_touches_nothing(n):
    e0, p0, _ = arenas(n, seed=4)
    e, p, ectl = e0.to(DEV), p0.to(DEV), make_ectl(0.9, True, applied=0.25, n_updates=5)
    before = bytes(read_ectl(ectl))
    for ctl in (make_ctl(1), make_ctl(1, accum_steps=2)):
        ema_update(e, p, ectl, 3, 1, ctl)
        assert same_bits(e, e0.to(DEV)) and same_bits(p, p0.to(DEV))
        assert bytes(read_ectl(ectl)) == before


@pytest.mark.parametrize("n", [4, 1028, FULL + 4])
def test_applies_without_a_skip(n):
    """a control block with skip = 0, and no control block"""
    e0, p0, _ = arenas(n, seed=5)
    p = p0.to(DEV)
    out = []
    for ctl in (make_ctl(0), None):
        e, ectl = e0.to(DEV), make_ectl(0.9, False)
        ema_update(e, p, ectl, 3, 1, ctl)
        c = read_ectl(ectl)
        assert c.n_updates == 1 and c.applied == np.float32(0.9)
        assert same_bits(e, host_update(e0, p0, c.applied).to(DEV))
        out.append(e)
    assert same_bits(out[0], out[1])


@pytest.mark.parametrize("n", SIZES)
def test_swap(n):
    a0, b0, _ = arenas(n, seed=6)
    # one allocation, so that a write past either arena's end lands in a guard
    buf = torch.full((2 * n + 3 * 64,), 7.0, device=DEV)
    a, b = buf[64:64 + n], buf[128 + n:128 + 2 * n]
    a.copy_(a0)
    b.copy_(b0)
    L().ema_swap(a.data_ptr(), b.data_ptr(), n, sptr())
    torch.cuda.synchronize()
    assert same_bits(a, b0.to(DEV)) and same_bits(b, a0.to(DEV))
    L().ema_swap(a.data_ptr(), b.data_ptr(), n, sptr())
    torch.cuda.synchronize()
    assert same_bits(a, a0.to(DEV)) and same_bits(b, b0.to(DEV))
    guard = torch.cat([buf[:64], buf[64 + n:128 + n], buf[128 + 2 * n:]])
    assert bool((guard == 7.0).all())


def test_update_stays_inside_its_arena():
    n = 1028
    e0, p0, _ = arenas(n, seed=8)
    buf = torch.full((n + 128,), 7.0, device=DEV)
    e = buf[64:64 + n]
    e.copy_(e0)
    ema_update(e, p0.to(DEV), make_ectl(0.5, False), 0, 1)
    assert same_bits(e, host_update(e0, p0, 0.5).to(DEV))
    assert bool((buf[:64] == 7.0).all()) and bool((buf[64 + n:] == 7.0).all())


# ------------------------------------------------------------------ trainer
SIZE, BD, RB, B = 32, 8, 1, 4


def make_model():
    import flow_realnvp
    import utils
    prior = torch.distributions.Normal(torch.tensor(0.0, device=DEV), torch.tensor(1.0, device=DEV))
    m = flow_realnvp.RealNVP(3, SIZE, prior, utils.Hyperparameters(BD, RB, True, True, True, True))
    m.load_state_dict(formula_state(m))
    return m.to(DEV)


def make_trainer(dtype="bf16", **kw):
    from realnvp_hip.trainer import FlowTrainer
    return FlowTrainer(make_model(), B, dtype=dtype, **kw)


def batch(s):
    import utils
    return utils.logit_transform(pixels(B, 3, SIZE, seed=100 + s), noise=uniform_noise(B, 3, SIZE, seed=200 + s))


def packed_images(tr):
    out = []
    for st in tr.stages:
        if st[0] != "coupling":
            continue
        ws = st[2].weights(tr.dtype)
        dt = torch.bfloat16 if tr.dtype == "bf16" else torch.float32
        for name in ws["geo"]:
            for kind in ("wf:", "wd:"):
                out.append(ws["arena"].view(kind + name, dt).float().clone())
            out.append(ws["arena"].view("norm:" + name, torch.float32).clone())
    return out


def assert_same_bits(a, b, names=("param", "exp_avg", "exp_avg_sq", "grad"), what=""):
    for name in names:
        x, y = getattr(a, name), getattr(b, name)
        assert same_bits(x, y), (what, name, int((bits(x) != bits(y)).sum()))
    assert int(a.step_t.item()) == int(b.step_t.item())
    for x, y in zip(packed_images(a), packed_images(b)):
        assert torch.equal(x, y), (what, "packed images")


def start(tr, graph, s=0):
    tr.set_input(*batch(s))
    if graph:
        tr.capture(warmup=1)
    return tr


def steps(tr, n):
    for _ in range(n):
        tr.step()
    torch.cuda.synchronize()


GRAPH = pytest.mark.parametrize("graph", [False, True], ids=["eager", "hipgraph"])


def _variants():
    from realnvp_hip.stepctl import StepSchedule
    return {"fused": dict(), "separate": dict(param_pass="separate"), "unchained": dict(chain=False),
            "overlap": dict(overlap=True), "ranges": dict(overlap=True, param_pass="separate", chain=False),
            "scheduled": dict(lr_schedule=StepSchedule(warmup_steps=2, warmup_start=0.25, decay="exp", decay_rate=0.8)),
            "scheduled_separate": dict(param_pass="separate",
                                       lr_schedule=StepSchedule(warmup_steps=2, warmup_start=0.25)),
            "clipped": dict(max_grad_norm=100.0)}


@GRAPH
@pytest.mark.parametrize("name", list(_variants()))
def test_ema_does_not_perturb_training(name, graph):
    """four steps with and without ema_decay: everything the step leaves is
    equal bit for bit, in every optimizer path; the average moved four times,
    the last time with the fourth step's decay"""
    from realnvp_hip.stepctl import ema_decay_at
    kw = _variants()[name]
    a = start(make_trainer(ema_decay=0.9, **kw), graph)
    b = start(make_trainer(**kw), graph)
    assert b.ema is None and b.ema_buf is None
    assert (a.adam_ranges is not None) == (name == "ranges")
    assert a.fused == ("separate" not in name and name != "ranges")
    assert (a.ctl_buf is not None) == (name in ("scheduled", "scheduled_separate", "clipped"))
    assert a.ema.data_ptr() != a.param.data_ptr() and same_bits(a.ema, a.param)
    assert a.ema_state() == {"decay": float(np.float32(0.9)), "warmup": True, "applied": 0.0, "n_updates": 0}
    steps(a, 4)
    steps(b, 4)
    assert_same_bits(a, b, what=name)
    st = a.ema_state()
    assert st["n_updates"] == 4 and int(a.step_t.item()) == 4
    np.testing.assert_allclose(st["applied"], ema_decay_at(0.9, True, 4), rtol=F32_1)
    assert not same_bits(a.ema, a.param)


@GRAPH
@pytest.mark.parametrize("warmup", [True, False], ids=["warmup", "nowarmup"])
def test_trajectory(warmup, graph):
    """the average after 6 steps against the float64 recurrence over the
    recorded parameters: three roundings per update plus the decay's, each at
    most 2^-24 max|p|"""
    from realnvp_hip.stepctl import ema_decay_at
    T, decay = 6, 0.9
    tr = start(make_trainer(ema_decay=decay, ema_warmup=warmup), graph)
    ref = tr.param.double().cpu()
    shifted = ref.clone()
    pmax = float(ref.abs().max())
    for u in range(1, T + 1):
        steps(tr, 1)
        p = tr.param.double().cpu()
        pmax = max(pmax, float(p.abs().max()))
        ref = ref + (1.0 - ema_decay_at(decay, warmup, u)) * (p - ref)
        shifted = shifted + (1.0 - ema_decay_at(decay, warmup, u + 1)) * (p - shifted)
    st = tr.ema_state()
    assert st["n_updates"] == T and st["warmup"] == warmup
    np.testing.assert_allclose(st["applied"], ema_decay_at(decay, warmup, T), rtol=F32_1)
    err = float((tr.ema.double().cpu() - ref).abs().max())
    bound = 4 * T * 2.0 ** -24 * pmax
    print("max |ema - float64 recurrence| = %.3g, bound %.3g (max|p| %.3g); a recurrence one step ahead in u is "
          "off by %.3g" % (err, bound, pmax, float((shifted - ref).abs().max())))
    assert err <= bound


@GRAPH
def test_accumulation_moves_the_average_on_the_applying_micro_step(graph):
    tr = start(make_trainer(ema_decay=0.9, accum_steps=2), graph)
    e0 = tr.ema.clone()
    steps(tr, 1)
    assert tr.step_control_state()["hold"] == 1
    assert same_bits(tr.ema, e0) and tr.ema_state()["n_updates"] == 0 and tr.ema_state()["applied"] == 0.0
    steps(tr, 1)
    assert not same_bits(tr.ema, e0) and tr.ema_state()["n_updates"] == 1
    e1 = tr.ema.clone()
    steps(tr, 1)
    assert same_bits(tr.ema, e1) and tr.ema_state()["n_updates"] == 1
    steps(tr, 1)
    assert not same_bits(tr.ema, e1) and tr.ema_state()["n_updates"] == 2 and int(tr.step_t.item()) == 2


@GRAPH
def test_skipped_step_leaves_the_average(graph):
    tr = make_trainer(ema_decay=0.9, max_grad_norm=100.0)
    pix = pixels(B, 3, SIZE, seed=5).to(DEV)
    tr.set_pixels(pix)
    if graph:
        tr.capture(warmup=1)
    steps(tr, 1)
    e1, blk = tr.ema.clone(), tr.ema_buf.clone()
    assert tr.ema_state()["n_updates"] == 1
    bad = pix.clone()
    bad[1, 2, 3, 4] = float("nan")
    tr.set_pixels(bad)
    steps(tr, 1)
    assert tr.step_control_state()["n_skipped"] == 1 and tr.step_control_state()["skip"] == 1
    assert same_bits(tr.ema, e1) and torch.equal(tr.ema_buf, blk) and tr.ema_state()["n_updates"] == 1
    tr.set_pixels(pix)
    steps(tr, 1)
    assert tr.ema_state()["n_updates"] == 2 and not same_bits(tr.ema, e1) and bool(tr.ema.isfinite().all())


def test_set_ema_decay_on_a_captured_trainer():
    tr = start(make_trainer(ema_decay=0.9, ema_warmup=False), True)
    g = tr.graph
    steps(tr, 1)
    assert tr.ema_state()["applied"] == float(np.float32(0.9))
    tr.set_ema_decay(0.5)
    e = tr.ema.clone().cpu()
    steps(tr, 1)
    st = tr.ema_state()
    assert tr.graph is g and st["applied"] == 0.5 and st["decay"] == 0.5 and st["n_updates"] == 2
    assert same_bits(tr.ema, host_update(e, tr.param.cpu(), 0.5).to(DEV))
    for bad in (1.0, -0.1, "x", None):
        with pytest.raises(ValueError):
            tr.set_ema_decay(bad)
    assert tr.ema_state()["decay"] == 0.5


def test_capture_restores_the_average():
    tr = make_trainer(ema_decay=0.9)
    tr.set_input(*batch(0))
    steps(tr, 1)
    e, blk, p = tr.ema.clone(), tr.ema_buf.clone(), tr.param.clone()
    tr.capture(warmup=2)
    assert same_bits(tr.ema, e) and torch.equal(tr.ema_buf, blk) and same_bits(tr.param, p)
    assert tr.ema_state()["n_updates"] == 1


@GRAPH
def test_swap_in(graph):
    """Inside ema_weights() the model IS the averaged model: its parameters
    are ema_state_dict()'s bit for bit, and a FlowEvaluator pass gives the
    mean log-likelihood of a second model loaded from ema_state_dict(), to
    the larger of that second evaluator's own difference between two passes
    and one fp32 rounding.  A pass is not reproducible to the bit even from
    the same noise: the per-sample log-det is added up with float atomics
    (two passes of one model from counter 0 gave -381.056091 / -381.055969
    and -381.056152 / -381.056091, the pass inside the block -381.056091 and
    -381.05603; the raw weights -382.7777).  Two more steps after the block
    leave what a trainer that never swapped has."""
    from realnvp_hip.evaluator import FlowEvaluator
    a = start(make_trainer(ema_decay=0.9), graph)
    b = start(make_trainer(ema_decay=0.9), graph)
    steps(a, 2)
    steps(b, 4)
    raw, avg = a.param.clone(), a.ema.clone()
    esd = a.ema_state_dict()
    names = [n for n, _ in a.model.named_parameters()]
    assert list(esd) == list(a.model.state_dict())
    batches = [pixels(B, 3, SIZE, seed=300 + k).to(DEV) for k in range(2)]

    def logll(model):
        return FlowEvaluator(model, B, dtype="bf16", seed=11).evaluate(batches)[0]
    second = make_model()
    second.load_state_dict(esd)
    # two runs of the second model's evaluator: its first pass draws the noise
    # the pass inside the block draws (same seed, counter 0), its second pass
    # the next counters'
    ev2 = FlowEvaluator(second, B, dtype="bf16", seed=11)
    ll_second, ll_again = ev2.evaluate(batches)[0], ev2.evaluate(batches)[0]
    ll_raw = logll(a.model)
    with a.ema_weights() as inside:
        assert inside is a
        assert same_bits(a.param, avg) and same_bits(a.ema, raw)
        sd = a.model.state_dict()
        for k, v in a.ema_state_dict().items():
            assert v.data_ptr() != sd[k].data_ptr() and torch.equal(v, sd[k]) and torch.equal(v, esd[k]), k
            if k in names:
                assert same_bits(v, sd[k]), k
        ll_in = logll(a.model)
        for f in (a.step, a.step_eager, a.state_dict, a.capture, a.reset_ema, a.ema_weights().__enter__):
            with pytest.raises(RuntimeError, match="ema_weights"):
                f()
    tol = max(abs(ll_second - ll_again), F32_1 * abs(ll_second))
    print("mean log-likelihood: average in place %.9g, second model %.9g (again %.9g), raw weights %.9g"
          % (ll_in, ll_second, ll_again, ll_raw))
    assert abs(ll_in - ll_second) <= tol
    assert ll_raw != ll_in and abs(ll_raw - ll_in) > tol
    torch.cuda.synchronize()
    assert same_bits(a.param, raw) and same_bits(a.ema, avg)
    # an exception inside the block still swaps back
    with pytest.raises(KeyError):
        with a.ema_weights():
            raise KeyError("x")
    torch.cuda.synchronize()
    assert same_bits(a.param, raw) and same_bits(a.ema, avg)
    steps(a, 2)
    assert_same_bits(a, b, names=("param", "exp_avg", "exp_avg_sq", "grad", "ema"), what="after the swap")
    assert a.ema_state() == b.ema_state() and a.ema_state()["n_updates"] == 4


@GRAPH
def test_checkpoint(graph):
    a = start(make_trainer(ema_decay=0.9, seed=1), False)
    steps(a, 2)
    sd = copy.deepcopy(a.state_dict())
    assert sorted(sd["ema"]) == ["decay", "n_updates", "shadow", "warmup"]
    assert (sd["ema"]["decay"], sd["ema"]["warmup"], sd["ema"]["n_updates"]) == (0.9, True, 2)
    assert same_bits(sd["ema"]["shadow"], a.ema) and sd["ema"]["shadow"].data_ptr() != a.ema.data_ptr()
    steps(a, 2)
    b = make_trainer(ema_decay=0.5, ema_warmup=False, seed=2)
    b.load_state_dict(sd)
    start(b, graph)
    assert same_bits(b.ema, sd["ema"]["shadow"].to(DEV))
    assert b.ema_state() == {"decay": float(np.float32(0.9)), "warmup": True, "applied": 0.0, "n_updates": 2}
    steps(b, 2)
    assert_same_bits(b, a, names=("param", "exp_avg", "exp_avg_sq", "grad", "ema"), what="resumed")
    assert b.ema_state() == a.ema_state() and b.ema_state()["n_updates"] == 4
    # a trainer without the average refuses the checkpoint; one with it takes a checkpoint without
    plain = make_trainer()
    assert "ema" not in plain.state_dict()
    with pytest.raises(ValueError, match="ema_decay"):
        plain.load_state_dict(sd)
    start(plain, False)
    steps(plain, 1)
    c = make_trainer(ema_decay=0.9)
    start(c, False)
    steps(c, 1)
    c.load_state_dict(copy.deepcopy(plain.state_dict()))
    assert same_bits(c.ema, c.param) and same_bits(c.param, plain.param) and c.ema_state()["n_updates"] == 0


def test_refusals():
    from realnvp_hip.trainer import FlowTrainer
    m = make_model()
    for bad in (1.0, -0.1, "x"):
        with pytest.raises(ValueError, match="ema_decay"):
            FlowTrainer(m, B, ema_decay=bad)
    tr = FlowTrainer(m, B, ema_decay=None)
    assert tr.ema is None and tr.ema_buf is None
    for f in (tr.ema_weights, tr.ema_state, tr.ema_state_dict, tr.reset_ema, lambda: tr.set_ema_decay(0.5)):
        with pytest.raises(RuntimeError, match="ema_decay"):
            f()
    # reset_ema after the caller wrote the parameters
    tr = start(make_trainer(ema_decay=0.9), False)
    steps(tr, 1)
    with torch.no_grad():
        tr.param.mul_(0.5)
    tr.reset_ema()
    assert same_bits(tr.ema, tr.param) and tr.ema_state()["n_updates"] == 0
