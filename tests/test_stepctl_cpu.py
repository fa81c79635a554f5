"""Host side of the step control (realnvp_hip.stepctl) and the argument
checks of its entry points; no GPU needed."""
import ctypes

import numpy as np
import pytest
import torch

BASE, W, S, GAMMA, T, F = 5e-4, 5, 0.1, 0.97, 40, 0.05
US = range(61)


def _torch_lrs(make):
    """lr torch's scheduler applies at optimizer step u = 0, 1, ..."""
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=BASE)
    sched = make(opt)
    out = []
    for _ in US:
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    return np.array(out)


def _ours(sch, us=US):
    return np.array([BASE * sch.factor(u) for u in us])


def test_warmup_matches_linear_lr():
    from torch.optim.lr_scheduler import LinearLR
    from realnvp_hip.stepctl import StepSchedule
    ref = _torch_lrs(lambda o: LinearLR(o, start_factor=S, total_iters=W))
    np.testing.assert_allclose(_ours(StepSchedule(warmup_steps=W, warmup_start=S)), ref, rtol=1e-12)


def test_exp_matches_exponential_lr():
    from torch.optim.lr_scheduler import ExponentialLR
    from realnvp_hip.stepctl import StepSchedule
    ref = _torch_lrs(lambda o: ExponentialLR(o, gamma=GAMMA))
    np.testing.assert_allclose(_ours(StepSchedule(decay="exp", decay_rate=GAMMA)), ref, rtol=1e-12)


def test_cosine_matches_cosine_annealing_lr():
    from torch.optim.lr_scheduler import CosineAnnealingLR
    from realnvp_hip.stepctl import StepSchedule
    ref = _torch_lrs(lambda o: CosineAnnealingLR(o, T_max=T, eta_min=F * BASE))
    sch = StepSchedule(decay="cosine", decay_rate=F, decay_steps=T)
    np.testing.assert_allclose(_ours(sch)[:T + 1], ref[:T + 1], rtol=1e-12)
    # held at the floor after T (torch's recursion swings back up)
    np.testing.assert_allclose(_ours(sch)[T:], F * BASE, rtol=1e-12)


def test_warmup_times_exp_matches_chained_scheduler():
    from torch.optim.lr_scheduler import ChainedScheduler, ExponentialLR, LinearLR
    from realnvp_hip.stepctl import StepSchedule
    ref = _torch_lrs(lambda o: ChainedScheduler([LinearLR(o, start_factor=S, total_iters=W),
                                                 ExponentialLR(o, gamma=GAMMA)]))
    sch = StepSchedule(warmup_steps=W, warmup_start=S, decay="exp", decay_rate=GAMMA)
    np.testing.assert_allclose(_ours(sch), ref, rtol=1e-12)


def test_default_schedule_is_constant_and_config_roundtrips():
    from realnvp_hip.stepctl import StepSchedule
    assert all(StepSchedule().factor(u) == 1.0 for u in US)
    sch = StepSchedule(warmup_steps=W, warmup_start=S, decay="cosine", decay_rate=F, decay_steps=T)
    assert StepSchedule.from_config(sch.config()) == sch


@pytest.mark.parametrize("kw", [dict(warmup_steps=-1), dict(warmup_steps=2, warmup_start=0.0),
                                dict(warmup_steps=2, warmup_start=1.5), dict(warmup_steps=2, warmup_start=-0.1),
                                dict(decay="exp", decay_rate=0.0), dict(decay="exp", decay_rate=-0.5),
                                dict(decay="cosine", decay_rate=0.1, decay_steps=0),
                                dict(decay="cosine", decay_rate=0.1, decay_steps=-3),
                                dict(decay="cosine", decay_rate=0.1), dict(decay="linear")])
def test_bad_schedules_raise(kw):
    from realnvp_hip.stepctl import StepSchedule
    with pytest.raises(ValueError):
        StepSchedule(**kw)


@pytest.mark.parametrize("v", [0.0, -1.0, float("nan"), float("inf")])
def test_bad_max_grad_norm_raises(v):
    from realnvp_hip.stepctl import check_max_grad_norm
    from realnvp_hip.trainer import FlowTrainer
    with pytest.raises(ValueError):
        check_max_grad_norm(v)
    with pytest.raises(ValueError):      # checked before the device is looked at
        FlowTrainer(torch.nn.Linear(1, 1), 4, max_grad_norm=v)
    assert check_max_grad_norm(None) is None and check_max_grad_norm(2) == 2.0


def test_control_block_mirror_matches_the_library():
    from realnvp_hip import _lib
    dll = ctypes.CDLL(_lib.LIB_PATH)
    assert dll.rnvp_struct_size(12) == ctypes.sizeof(_lib.StepCtl)
    assert dll.rnvp_struct_size(7) == ctypes.sizeof(_lib.AdamArgs)
    assert dll.rnvp_struct_size(13) == -1
    assert _lib.AdamArgs.ctl.offset + 8 == ctypes.sizeof(_lib.AdamArgs)   # the trailing member
    assert dll.rnvp_version() >= 108


def test_step_control_entry_points_reject_bad_arguments_without_launch():
    """NULL pointers, a partial count other than rnvp_grad_sumsq_parts(n),
    misaligned or odd-sized arenas: RNVP_E_INVALID (-1) before any HIP call
    (the pointers below are host addresses: a launch would fault)."""
    from realnvp_hip import _lib
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("rnvp_grad_sumsq", "rnvp_step_control", "rnvp_adam_range", "rnvp_step_advance",
                 "rnvp_grad_sumsq_parts"):
        getattr(dll, name).restype = ctypes.c_int
    dll.rnvp_grad_sumsq_parts.argtypes = [ctypes.c_longlong]
    dll.rnvp_grad_sumsq.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_int,
                                    ctypes.c_void_p]
    dll.rnvp_step_control.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_void_p]
    dll.rnvp_adam_range.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]
    dll.rnvp_step_advance.argtypes = [ctypes.c_void_p] * 3

    parts = dll.rnvp_grad_sumsq_parts
    assert parts(-4) == -1
    assert parts(0) == 1 and parts(4) == 1 and parts(1024) == 1 and parts(1028) == 2
    assert parts(4 * 256 * 2048) == 2048 and parts(10 ** 9) == 2048       # bounded

    buf = (ctypes.c_double * 64)()          # 16-byte aligned host memory standing in for the arenas
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    ad = _lib.AdamArgs()
    ad.param = ad.grad = ad.exp_avg = ad.exp_avg_sq = base
    ad.step = base
    a = ctypes.addressof(ad)
    n = 1028
    assert dll.rnvp_grad_sumsq(None, n, base, parts(n), None) == -1
    assert dll.rnvp_grad_sumsq(a, n, None, parts(n), None) == -1
    assert dll.rnvp_grad_sumsq(a, n, base, parts(n) + 1, None) == -1
    assert dll.rnvp_grad_sumsq(a, n, base, parts(n) - 1, None) == -1
    assert dll.rnvp_grad_sumsq(a, n + 1, base, parts(n), None) == -1      # n % 4
    assert dll.rnvp_grad_sumsq(a, -4, base, 1, None) == -1
    bad = _lib.AdamArgs.from_buffer_copy(ad)
    bad.grad = None
    assert dll.rnvp_grad_sumsq(ctypes.addressof(bad), n, base, parts(n), None) == -1
    bad.grad = base + 4                                                    # not 16-byte aligned
    assert dll.rnvp_grad_sumsq(ctypes.addressof(bad), n, base, parts(n), None) == -1
    assert dll.rnvp_adam_range(ctypes.addressof(bad), 4, None) == -1

    assert dll.rnvp_step_control(None, base, None, 0, None) == -1
    assert dll.rnvp_step_control(base, None, None, 0, None) == -1
    assert dll.rnvp_step_control(base, base, base, 0, None) == -1
    assert dll.rnvp_step_control(base, base, base, 2049, None) == -1

    assert dll.rnvp_adam_range(None, 4, None) == -1
    assert dll.rnvp_adam_range(a, 6, None) == -1
    assert dll.rnvp_adam_range(a, -4, None) == -1
    bad = _lib.AdamArgs.from_buffer_copy(ad)
    bad.step = None
    assert dll.rnvp_adam_range(ctypes.addressof(bad), 4, None) == -1

    assert dll.rnvp_step_advance(None, base, None) == -1
    assert dll.rnvp_step_advance(base, None, None) == -1
