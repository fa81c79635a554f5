"""In-graph gradient accumulation (include/realnvp_hip.h, "step control":
rnvp_grad_accumulate and rnvp_step_control's hold / apply decision) at the
ABI level on raw tensors, then FlowTrainer(accum_steps=K) on the m32_d8_r1
model at B = 4."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from formula_init import formula_state, pixels, uniform_noise

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32_1 = 2e-7          # one fp32 rounding of a value computed in fp64 (2^-24 = 6e-8), with margin
FULL = 4 * 256 * 2048      # one sweep of the capped grid
SIZES = [4, 1028, FULL + 4, 1_000_004]
REG = 0.5


def L():
    from realnvp_hip import _lib
    return _lib.lib()


def sptr():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------ helpers
def make_ctl(accum_steps, micro=0, max_norm=None, base_lr=1e-3):
    """a device rnvp_step_ctl block (uint8 tensor)"""
    from realnvp_hip._lib import StepCtl
    from realnvp_hip.stepctl import fill_ctl
    c = fill_ctl(StepCtl(), base_lr, None, max_norm, accum_steps=accum_steps)
    c.micro = micro
    return torch.frombuffer(bytearray(bytes(c)), dtype=torch.uint8).to(DEV)


def read_ctl(t):
    from realnvp_hip._lib import StepCtl
    return StepCtl.from_buffer_copy(bytes(t.cpu().numpy()))


def arena(n, seed):
    """parameters, gradients (randn times a per-1024-block scale from {1e-3, 1,
    1e3}), an accumulator of the same make and a mask drawn from {0, 1, 2} per
    element (granules mix all three)"""
    gen = torch.Generator().manual_seed(seed)
    nb = (n + 1023) // 1024

    def scaled():
        sc = torch.tensor([1e-3, 1.0, 1e3])[torch.randint(0, 3, (nb,), generator=gen)]
        return torch.randn(n, generator=gen) * sc.repeat_interleave(1024)[:n]
    p = torch.randn(n, generator=gen)
    g, acc = scaled(), scaled()
    mask = torch.randint(0, 3, (n,), generator=gen, dtype=torch.uint8)
    return p.to(DEV), g.to(DEV), acc.to(DEV), mask.to(DEV)


def adam_args(p, g, mask, reg=REG):
    from realnvp_hip._lib import AdamArgs
    z = torch.zeros(4, device=DEV)
    step = torch.zeros(1, device=DEV, dtype=torch.int64)
    a = AdamArgs()
    a.param, a.grad, a.exp_avg, a.exp_avg_sq = p.data_ptr(), g.data_ptr(), z.data_ptr(), z.data_ptr()
    a.mask = mask.data_ptr() if mask is not None else None
    a.step, a.step_add = step.data_ptr(), 1
    a.lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.reg_coef = 1e-3, 0.9, 0.999, 1e-8, 5e-5, reg
    return a, (z, step)


def accumulate(p, g, acc, mask, ctl):
    """rnvp_grad_accumulate in place on g / acc; the partials, prefilled with -1"""
    n = g.numel()
    parts = L().grad_sumsq_parts(n)
    out = torch.full((parts,), -1.0, device=DEV, dtype=torch.float64)
    a, keep = adam_args(p, g, mask)
    L().grad_accumulate(C.byref(a), acc.data_ptr(), n, ctl.data_ptr(), out.data_ptr(), parts, sptr())
    torch.cuda.synchronize()
    return out


def grad_sumsq(p, g, mask):
    n = g.numel()
    parts = L().grad_sumsq_parts(n)
    out = torch.full((parts,), -1.0, device=DEV, dtype=torch.float64)
    a, keep = adam_args(p, g, mask)
    L().grad_sumsq(C.byref(a), n, out.data_ptr(), parts, sptr())
    torch.cuda.synchronize()
    return out


def ref_sumsq(p, g, mask, reg=REG):
    x = g.double() + (mask == 2).double() * float(np.float32(2.0) * np.float32(reg)) * p.double()
    return float((x * x)[mask > 0].sum())


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------- kernel
@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_held_micro_step_adds_into_the_accumulator_only(n, K):
    """micro < K - 1: acc = acc + grad in fp32 (one IEEE addition per element,
    frozen elements and padding included), the gradient arena and the
    partials keep their bits"""
    p, g, acc, mask = arena(n, seed=n % 1000 + K)
    want = (acc.cpu() + g.cpu()).to(DEV)
    g0 = g.clone()
    ctl = make_ctl(K, micro=K - 2)
    before = read_ctl(ctl)
    parts = accumulate(p, g, acc, mask, ctl)
    assert same_bits(acc, want), int((acc != want).sum())
    assert same_bits(g, g0)
    assert bool((parts == -1.0).all())
    assert bytes(read_ctl(ctl)) == bytes(before)        # the pass only reads the block


@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_final_micro_step_leaves_the_average_and_its_partials(n, K):
    """micro == K - 1: grad = (acc + grad) / K as torch computes it in fp32 on
    the host (IEEE addition, then IEEE division), acc = 0, and the partials
    bitwise those of rnvp_grad_sumsq on that gradient; the pass reproduces."""
    assert L().grad_sumsq_parts(FULL) == 2048 and L().grad_sumsq_parts(FULL + 4) == 2048
    p, g, acc, mask = arena(n, seed=n % 1000 + 10 * K)
    want = ((acc.cpu() + g.cpu()) / K).to(DEV)
    g1, acc1, g2, acc2 = g.clone(), acc.clone(), g.clone(), acc.clone()
    ctl = make_ctl(K, micro=K - 1)
    parts = accumulate(p, g1, acc1, mask, ctl)
    again = accumulate(p, g2, acc2, mask, ctl)
    assert same_bits(g1, want), int((g1 != want).sum())
    assert not acc1.any() and same_bits(acc1, torch.zeros_like(acc1))
    assert parts.numel() == L().grad_sumsq_parts(n)
    norm_pass = grad_sumsq(p, g1, mask)
    assert same_bits(parts, norm_pass), int((parts != norm_pass).sum())
    ref = ref_sumsq(p, want, mask)
    np.testing.assert_allclose(math.sqrt(float(parts.sum())), math.sqrt(ref), rtol=1e-12)
    assert same_bits(g2, g1) and same_bits(acc2, acc1) and same_bits(again, parts), "not bitwise reproducible"
    # without a mask every element counts once, without the regulariser
    g3, acc3 = g.clone(), acc.clone()
    parts = accumulate(p, g3, acc3, None, ctl)
    assert same_bits(g3, want) and same_bits(parts, grad_sumsq(p, g3, None))


def test_accum_steps_of_one_or_zero_is_a_plain_norm_pass():
    """a block with accum_steps <= 1 (a zero-filled one included) always applies: K = 1"""
    n = 1028
    p, g, acc, mask = arena(n, seed=5)
    want = (acc.cpu() + g.cpu()).to(DEV)
    from realnvp_hip._lib import StepCtl
    for ctl in (make_ctl(1), torch.zeros(C.sizeof(StepCtl), dtype=torch.uint8, device=DEV)):
        gg, aa = g.clone(), acc.clone()
        parts = accumulate(p, gg, aa, mask, ctl)
        assert same_bits(gg, want) and not aa.any() and same_bits(parts, grad_sumsq(p, gg, mask))


def _micro_step(ctl, step, p, g, acc, mask):
    """one micro-step's control launches around the accumulate pass"""
    n = g.numel()
    parts = L().grad_sumsq_parts(n)
    part = torch.full((parts,), -1.0, device=DEV, dtype=torch.float64)
    a, keep = adam_args(p, g, mask)
    L().step_control(ctl.data_ptr(), step.data_ptr(), None, 0, sptr())
    L().grad_accumulate(C.byref(a), acc.data_ptr(), n, ctl.data_ptr(), part.data_ptr(), parts, sptr())
    L().step_control(ctl.data_ptr(), step.data_ptr(), part.data_ptr(), parts, sptr())
    L().step_advance(step.data_ptr(), ctl.data_ptr(), sptr())
    torch.cuda.synchronize()
    return read_ctl(ctl)


@pytest.mark.parametrize("K", [2, 3])
def test_control_holds_then_takes_the_clip_decision(K):
    n = 4 * 256 * 3 + 4
    p, _, _, mask = arena(n, seed=K)
    gs = [arena(n, seed=40 + j)[1] for j in range(K)]
    avg = gs[0].cpu()
    for g in gs[1:]:
        avg = avg + g.cpu()
    avg = (avg / K).to(DEV)
    norm = math.sqrt(ref_sumsq(p, avg, mask))
    max_norm = 0.5 * norm
    ctl = make_ctl(K, max_norm=max_norm)
    step = torch.full((1,), 7, device=DEV, dtype=torch.int64)
    acc = torch.zeros(n, device=DEV)
    for rounds in (1, 2):            # two optimizer steps on one block: micro goes back to 0
        for j in range(K):
            g = gs[j].clone()
            c = _micro_step(ctl, step, p, g, acc, mask)
            if j < K - 1:
                assert (c.skip, c.hold, c.micro) == (1, 1, j + 1)
                assert c.n_skipped == 0 and c.n_clipped == rounds - 1 and c.grad_scale == 1.0
                assert int(step.item()) == 7 + rounds - 1
                assert same_bits(g, gs[j])
            else:
                assert (c.skip, c.hold, c.micro) == (0, 0, 0)
                assert c.n_skipped == 0 and c.n_clipped == rounds
                np.testing.assert_allclose(c.grad_norm, norm, rtol=F32_1)
                np.testing.assert_allclose(c.grad_scale, float(np.float32(max_norm)) / (norm + 1e-6), rtol=F32_1)
                assert int(step.item()) == 7 + rounds
                assert same_bits(g, avg) and not acc.any()


def test_inf_in_an_early_micro_step_skips_the_optimizer_step_once():
    """an inf in micro-step 1 of 3 rides in the accumulator: nothing is counted
    while the step is held, micro-step 3 skips once, and the accumulator is
    clean for the next optimizer step"""
    K, n = 3, 1028
    p, _, _, mask = arena(n, seed=9)
    gs = [arena(n, seed=50 + j)[1] for j in range(K)]
    live = int((mask == 1).nonzero()[5])
    bad = gs[0].clone()
    bad[live] = float("inf")
    ctl = make_ctl(K, max_norm=1.0)
    step = torch.full((1,), 3, device=DEV, dtype=torch.int64)
    acc = torch.zeros(n, device=DEV)
    for j, g in enumerate([bad, gs[1].clone(), gs[2].clone()]):
        c = _micro_step(ctl, step, p, g, acc, mask)
        if j < K - 1:
            assert (c.skip, c.hold, c.micro, c.n_skipped, c.n_clipped) == (1, 1, j + 1, 0, 0)
        else:
            assert (c.skip, c.hold, c.micro, c.n_skipped, c.n_clipped) == (1, 0, 0, 1, 0)
            assert not math.isfinite(c.grad_norm) and c.grad_scale == 1.0
    assert int(step.item()) == 3
    assert not acc.any() and same_bits(acc, torch.zeros_like(acc))
    # the next optimizer step is clean
    for j in range(K):
        c = _micro_step(ctl, step, p, gs[j].clone(), acc, mask)
    assert (c.skip, c.hold, c.micro, c.n_skipped, c.n_clipped) == (0, 0, 0, 1, 1)
    assert int(step.item()) == 4 and math.isfinite(c.grad_norm)


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


def state_bits(tr):
    return [bits(t).clone() for t in (tr.param, tr.exp_avg, tr.exp_avg_sq, tr.step_t)] + packed_images(tr)


def assert_same_bits(a, b, names=("param", "exp_avg", "exp_avg_sq", "grad"), what=""):
    for name in names:
        x, y = getattr(a, name), getattr(b, name)
        assert same_bits(x, y), (what, name, int((x != y).sum()))
    assert int(a.step_t.item()) == int(b.step_t.item())
    for x, y in zip(packed_images(a), packed_images(b)):
        assert torch.equal(x, y), (what, "packed images")


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "hipgraph"])
def test_two_equal_micro_batches_equal_one_step(graph):
    """accum_steps = 2 fed the same batch twice against a clip-schedule trainer
    (max_grad_norm = 1e9 never binds) fed it once: (g + g) / 2 is exact, so
    everything the optimizer step leaves is equal bit for bit (bf16: the step
    is deterministic).  The held micro-step changes nothing but the
    accumulator."""
    x, ld = batch(0)
    a = make_trainer(accum_steps=2)
    b = make_trainer(max_grad_norm=1e9)
    assert a.fused and a._slab_table is None and a.max_grad_norm is None and a.acc is not None
    for t in (a, b):
        t.set_input(x, ld)
        if graph:
            t.capture(warmup=1)
    assert a.step_control_state()["micro"] == 0 and not a.acc.any()        # capture restored its warm-up
    a._ensure_packed()
    torch.cuda.synchronize()
    initial = state_bits(a)
    a.step()
    torch.cuda.synchronize()
    st = a.step_control_state()
    assert (st["hold"], st["skip"], st["micro"], st["n_skipped"]) == (1, 1, 1, 0)
    for u, v in zip(initial, state_bits(a)):
        assert torch.equal(u, v), "a held micro-step moved the optimizer's state"
    assert int(a.step_t.item()) == 0
    assert torch.equal(a.acc, a.grad)          # 0 + the micro-batch's gradient
    a.step()
    b.step()
    torch.cuda.synchronize()
    st = a.step_control_state()
    assert (st["hold"], st["skip"], st["micro"], st["n_skipped"], st["n_clipped"]) == (0, 0, 0, 0, 0)
    assert int(a.step_t.item()) == 1 and not a.acc.any()
    assert not same_bits(a.param, initial[0].view(torch.float32)), "the final micro-step did not apply"
    assert_same_bits(a, b, what="2 x same batch vs one step")
    assert st["grad_norm"] == b.step_control_state()["grad_norm"] and st["lr"] == b.step_control_state()["lr"]


def _variants():
    from realnvp_hip.stepctl import StepSchedule
    return {"separate": dict(param_pass="separate"), "unchained": dict(chain=False),
            "scheduled": dict(lr_schedule=StepSchedule(warmup_steps=2, warmup_start=0.25, decay="exp", decay_rate=0.8)),
            "clipped": dict(max_grad_norm=100.0)}


@pytest.mark.parametrize("name", ["separate", "unchained", "scheduled", "clipped"])
def test_accumulation_under_the_other_step_variants(name):
    """the separate parameter pass, the unchained flow program, a learning-rate
    schedule (u = optimizer steps, not micro-steps) and a binding clip: four
    replays of accum_steps = 2 on one batch against two replays of the K = 1
    trainer of the same make, bit for bit (bf16, captured)"""
    from realnvp_hip.stepctl import StepSchedule
    kw = _variants()[name]
    x, ld = batch(1)
    a = make_trainer(accum_steps=2, **kw)
    b = make_trainer(**dict(dict(max_grad_norm=1e9), **kw))
    assert a.fused == (name != "separate") and (a.links is None) == (name == "unchained")
    for t, n in ((a, 4), (b, 2)):
        t.set_input(x, ld)
        t.capture(warmup=1)
        for _ in range(n):
            t.step()
    torch.cuda.synchronize()
    assert_same_bits(a, b, what=name)
    sa, sb = a.step_control_state(), b.step_control_state()
    assert int(a.step_t.item()) == 2 and (sa["hold"], sa["micro"], sa["n_skipped"]) == (0, 0, 0)
    for k in ("lr", "grad_norm", "grad_scale", "n_clipped"):
        assert sa[k] == sb[k], (k, sa[k], sb[k])
    if name == "scheduled":
        sch = kw["lr_schedule"]
        assert isinstance(sch, StepSchedule)
        np.testing.assert_allclose(sa["lr"], float(np.float32(a.lr)) * sch.factor(1), rtol=F32_1)
    if name == "clipped":
        assert sa["n_clipped"] == 2 and sa["grad_scale"] < 1.0


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_accumulated_gradient_is_the_average(dtype):
    """K = 3, three different batches, eager: the arena after the third
    micro-step is torch's fp32 ((g1 + g2) + g3) / 3 of the three micro-batch
    gradients, bit for bit.

    bf16 (the step is deterministic): g1..g3 are what a K = 1 clip-schedule
    trainer computes at the same (unmoved: lr = 0, weight_decay = 0)
    parameters, and tr.grad after each held micro-step equals that trainer's.

    fp32: two fp32 steps on the same batch at the same parameters do not
    give the same bits -- the grouped weight gradient adds slab partials with
    atomics (test_gpu_trainer.py: _check_fused_vs_separate); a K = 1 trainer's
    gradients differed from the accumulating trainer's in 1190 .. 1381 of
    3,056,432 elements.  So the bitwise check uses the three gradients THIS
    trainer computed (tr.grad after each held micro-step; the third read
    between the backward and the accumulate pass, which is step_eager() taken
    apart), and the K = 1 trainer's average is compared in relative L2 at 8 x
    that trainer's own run-to-run difference on the same three batches
    (measured: 9.2e-9 against a run-to-run 9.8e-9), with a floor of 1e-6 (a
    few fp32 roundings of the vector's norm) should two runs ever agree: a
    dropped micro-batch or a missing division is off by 0.3 or more."""
    ref = make_trainer(dtype, max_grad_norm=1e9, lr=0.0, weight_decay=0.0)
    p0 = ref.param.clone()
    runs = []
    for _ in range(1 if dtype == "bf16" else 2):
        gs = []
        for s in range(3):
            ref.set_input(*batch(s))
            ref.step()
            torch.cuda.synchronize()
            gs.append(ref.grad.cpu().clone())
        runs.append(gs)
    assert same_bits(ref.param, p0)
    avg = [((gs[0] + gs[1]) + gs[2]) / 3 for gs in runs]
    tr = make_trainer(dtype, accum_steps=3)
    own = []
    for s in range(3):
        tr.set_input(*batch(s))
        if s < 2:
            tr.step()
        else:
            tr._ensure_packed()
            tr._fwd_bwd()
            torch.cuda.synchronize()
            own.append(tr.grad.cpu().clone())
            tr._optimizer()
        torch.cuda.synchronize()
        if s < 2:
            own.append(tr.grad.cpu().clone())
            assert tr.step_control_state()["hold"] == 1
        d = int((bits(own[s]) != bits(runs[0][s])).sum())
        print("%s micro-step %d: %d of %d gradient elements differ from the K = 1 trainer's" % (dtype, s + 1, d, tr.n))
        if dtype == "bf16":
            assert d == 0, "a held micro-step leaves its own gradient in tr.grad"
    want = (((own[0] + own[1]) + own[2]) / 3).to(DEV)
    d = int((bits(tr.grad) != bits(want)).sum())
    print("%s average: %d of %d elements differ from ((g1 + g2) + g3) / 3" % (dtype, d, tr.n))
    assert same_bits(tr.grad, want)
    if dtype == "bf16":
        assert same_bits(tr.grad, avg[0].to(DEV))
    else:
        noise, err = _rel(avg[1], avg[0]), _rel(tr.grad.cpu(), avg[0])
        print("fp32 average vs the K = 1 trainer's: rel %.3g (its own run-to-run %.3g)" % (err, noise))
        assert err <= max(1e-6, 8 * noise)
    st = tr.step_control_state()
    assert (st["hold"], st["skip"], st["micro"]) == (0, 0, 0)
    assert int(tr.step_t.item()) == 1 and not tr.acc.any()


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "hipgraph"])
def test_accumulated_clipped_trajectory_matches_reference(graph):
    """Two optimizer steps of the reference loop with (loss / 2).backward()
    twice, clip_grad_norm_(600) and Adam (tools/make_accum_golden.py).  The
    bounds are those of test_clipped_scheduled_trajectory_matches_reference
    (same model, no more steps): logll 1e-4, gradient norm and |exp_avg|_2
    5e-3, |exp_avg_sq|_1 1e-2, eval log-prob 5e-4.  A gradient summed instead
    of averaged is off by 2x in the norm, a missing clip by 2x in |exp_avg|."""
    from realnvp_hip.trainer import FlowTrainer
    import utils
    g = load_golden("accum_m32_d8_r1.npz")
    K, micro_steps = int(g["accum_steps"]), len(g["traj_logll"])
    steps = micro_steps // K
    assert K == 2 and steps == 2 and len(g["traj_grad_norm"]) == steps
    model = make_model()
    tr = FlowTrainer(model, int(g["batch"]), dtype="fp32", lr=float(g["base_lr"]),
                     weight_decay=float(g["weight_decay"]), max_grad_norm=float(g["max_norm"]), accum_steps=K)
    lls, norms, lrs, m1, m2 = [], [], [], [], []
    for s in range(micro_steps):
        x, ld = utils.logit_transform(pixels(B, 3, SIZE, seed=int(g["pixel_seeds"][s])),
                                      noise=uniform_noise(B, 3, SIZE, seed=int(g["noise_seeds"][s])))
        tr.set_input(x, ld)
        if graph and tr.graph is None:
            tr.capture(warmup=1)
        tr.reset_metrics()
        tr.step()
        st = tr.step_control_state()
        lls.append(tr.mean_logll(1))
        assert st["hold"] == int(s % K < K - 1) and st["micro"] == (s + 1) % K
        if not st["hold"]:
            norms.append(st["grad_norm"])
            lrs.append(st["lr"])
            m1.append(float(tr.exp_avg.double().norm()))
            m2.append(float(tr.exp_avg_sq.double().abs().sum()))
    print("logll", lls, g["traj_logll"], "\nnorm", norms, g["traj_grad_norm"], "\nlr", lrs, g["traj_lr"],
          "\n|m|2", m1, g["traj_exp_avg_l2"], "\n|v|1", m2, g["traj_exp_avg_sq_l1"])
    st = tr.step_control_state()
    assert st["n_clipped"] == steps and st["n_skipped"] == 0
    assert int(tr.step_t.item()) == steps == 2
    np.testing.assert_allclose(lrs, g["traj_lr"], rtol=F32_1)
    np.testing.assert_allclose(lls, g["traj_logll"], rtol=1e-4)
    np.testing.assert_allclose(norms, g["traj_grad_norm"], rtol=5e-3)
    np.testing.assert_allclose(m1, g["traj_exp_avg_l2"], rtol=5e-3)
    np.testing.assert_allclose(m2, g["traj_exp_avg_sq_l1"], rtol=1e-2)
    model.eval()
    with torch.no_grad():
        lp, _ = model(torch.from_numpy(load_golden("model_m32_d8_r1.npz")["x"]).to(DEV))
    np.testing.assert_allclose(lp.cpu().numpy(), g["traj_eval_logprob_after"], rtol=5e-4)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "hipgraph"])
def test_noise_advances_every_micro_step(graph):
    """set_pixels mode, the same pixels every step: micro-step j draws the
    noise of Philox counter j although the step counter stands still, i.e.
    what steps 1 and 2 of a K = 1 trainer with the same seed draw"""
    pix = pixels(B, 3, SIZE, seed=5).to(DEV)
    a = make_trainer(accum_steps=2, seed=3)
    b = make_trainer(seed=3)
    xa, xb = [], []
    for t, out in ((a, xa), (b, xb)):
        t.set_pixels(pix)
        if graph:
            t.capture(warmup=1)
        for _ in range(2):
            t.step()
            torch.cuda.synchronize()
            out.append(t.xl.clone())
    assert int(a.step_t.item()) == 1 and int(b.step_t.item()) == 2
    assert not torch.equal(xa[0], xa[1])
    assert same_bits(xa[0], xb[0]) and same_bits(xa[1], xb[1])
    assert a.rng_state()["noise_step"] == 2 and a.rng_state()["step"] == 1
    assert "noise_step" not in b.rng_state()


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "hipgraph"])
def test_checkpoint_between_micro_steps_resumes_bitwise(graph):
    """saved after 3 micro-steps of K = 2 (micro = 1: the accumulator travels),
    loaded into a fresh trainer (captured, when graph) and continued for 3
    more: the unbroken run, bit for bit (bf16), noise included"""
    pix = pixels(B, 3, SIZE, seed=5).to(DEV)
    kw = dict(accum_steps=2, max_grad_norm=100.0, seed=1)
    a = make_trainer(**kw)
    a.set_pixels(pix)
    for _ in range(3):
        a.step()
    sd = copy.deepcopy(a.state_dict())
    sc = sd["step_control"]
    assert sc["accum_steps"] == 2 and sc["micro"] == 1 and same_bits(sc["accum"], a.acc) and sc["accum"].any()
    assert sd["rng"]["noise_step"] == 3 and sd["rng"]["step"] == 1
    for _ in range(3):
        a.step()
    torch.cuda.synchronize()
    assert int(a.step_t.item()) == 3
    b = make_trainer(accum_steps=2, max_grad_norm=3.0, seed=1)
    b.load_state_dict(sd)
    b.set_pixels(pix)
    if graph:
        b.capture(warmup=1)
    st = b.step_control_state()
    assert st["micro"] == 1 and same_bits(b.acc, sc["accum"].to(DEV)) and int(b.noise_t.item()) == 3
    for _ in range(3):
        b.step()
    torch.cuda.synchronize()
    assert_same_bits(b, a, what="resumed between micro-steps")
    assert same_bits(b.xl, a.xl) and same_bits(b.acc, a.acc)
    assert b.step_control_state() == a.step_control_state() and b.rng_state() == a.rng_state()
    # a checkpoint on an optimizer-step boundary carries no accumulator
    assert a.step_control_state()["micro"] == 0 and "accum" not in a.state_dict()["step_control"]


def test_refusals():
    from realnvp_hip.trainer import FlowTrainer
    m = make_model()
    with pytest.raises(ValueError, match="process_group"):
        FlowTrainer(m, B, accum_steps=2, process_group=object())
    for bad in (0, -3, 65537, 2.5, "4", None):
        with pytest.raises(ValueError, match="accum_steps"):
            FlowTrainer(m, B, accum_steps=bad)
    a = make_trainer(accum_steps=2)
    a.set_input(*batch(0))
    a.step()
    sd = copy.deepcopy(a.state_dict())
    plain = make_trainer()
    plain.set_input(*batch(0))
    plain.step()
    psd = copy.deepcopy(plain.state_dict())
    for tr, ckpt in ((make_trainer(accum_steps=3), sd), (make_trainer(), sd), (make_trainer(max_grad_norm=1.0), sd),
                     (make_trainer(accum_steps=2), psd)):
        with pytest.raises(ValueError, match="accum_steps"):
            tr.load_state_dict(ckpt)
    make_trainer(accum_steps=2).load_state_dict(sd)
