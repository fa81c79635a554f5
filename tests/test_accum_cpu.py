"""Host side of the in-graph gradient accumulation (FlowTrainer(accum_steps=K),
include/realnvp_hip.h "step control"): the control block's mirror, the
argument checks of rnvp_grad_accumulate and the trainer's argument validation;
no GPU needed."""
import ctypes

import pytest
import torch


def _dll():
    from realnvp_hip import _lib
    dll = ctypes.CDLL(_lib.LIB_PATH)
    dll.rnvp_grad_sumsq_parts.restype = ctypes.c_int
    dll.rnvp_grad_sumsq_parts.argtypes = [ctypes.c_longlong]
    dll.rnvp_grad_accumulate.restype = ctypes.c_int
    dll.rnvp_grad_accumulate.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    return dll


def test_control_block_mirror_has_the_accumulation_fields():
    from realnvp_hip import _lib
    dll = _dll()
    assert dll.rnvp_struct_size(12) == ctypes.sizeof(_lib.StepCtl)
    assert dll.rnvp_version() >= 110
    names = [f[0] for f in _lib.StepCtl._fields_]
    # trailing, in the header's order: nothing before them moved
    assert names[-3:] == ["accum_steps", "micro", "hold"] and names[-4] == "n_skipped"
    S = _lib.StepCtl
    assert S.accum_steps.offset == S.n_skipped.offset + 8
    assert S.micro.offset == S.accum_steps.offset + 4 and S.hold.offset == S.micro.offset + 4
    assert "rnvp_grad_accumulate" in _lib.EXPORTED


def test_fill_ctl_writes_accum_steps():
    from realnvp_hip._lib import StepCtl
    from realnvp_hip.stepctl import check_accum_steps, fill_ctl
    assert fill_ctl(StepCtl(), 1e-3, None, None).accum_steps == 1
    c = fill_ctl(StepCtl(), 1e-3, None, 2.0, accum_steps=8)
    assert c.accum_steps == 8 and c.micro == 0 and c.hold == 0 and c.max_norm == 2.0
    assert check_accum_steps(1) == 1 and check_accum_steps(65536) == 65536
    for bad in (0, -2, 65537, 2.0, "2", None, True):
        with pytest.raises(ValueError):
            check_accum_steps(bad)
        with pytest.raises(ValueError):
            fill_ctl(StepCtl(), 1e-3, None, None, accum_steps=bad)


def test_grad_accumulate_rejects_bad_arguments_without_launch():
    """NULL pointers, a partial count other than rnvp_grad_sumsq_parts(n),
    misaligned or odd-sized arenas, the accumulator aliasing the gradient:
    RNVP_E_INVALID (-1) before any HIP call (the pointers below are host
    addresses: a launch would fault)."""
    from realnvp_hip import _lib
    dll = _dll()
    parts = dll.rnvp_grad_sumsq_parts
    buf = (ctypes.c_double * 64)()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    acc, ctl, part = base + 64, base + 128, base + 256
    ad = _lib.AdamArgs()
    ad.param = ad.grad = ad.exp_avg = ad.exp_avg_sq = base
    ad.step = base
    a = ctypes.addressof(ad)
    n = 1028
    f = dll.rnvp_grad_accumulate
    assert f(None, acc, n, ctl, part, parts(n), None) == -1
    assert f(a, None, n, ctl, part, parts(n), None) == -1
    assert f(a, acc, n, None, part, parts(n), None) == -1
    assert f(a, acc, n, ctl, None, parts(n), None) == -1
    assert f(a, acc, n, ctl, part, parts(n) + 1, None) == -1
    assert f(a, acc, n, ctl, part, parts(n) - 1, None) == -1
    assert f(a, acc, n + 1, ctl, part, parts(n), None) == -1          # n % 4
    assert f(a, acc, n + 2, ctl, part, parts(n), None) == -1
    assert f(a, acc, -4, ctl, part, 1, None) == -1
    assert f(a, acc + 4, n, ctl, part, parts(n), None) == -1          # accumulator not 16-byte aligned
    assert f(a, acc + 8, n, ctl, part, parts(n), None) == -1
    assert f(a, acc, n, ctl, part + 4, parts(n), None) == -1          # partials not 8-byte aligned
    assert f(a, base, n, ctl, part, parts(n), None) == -1             # accumulator == gradient arena
    for field, value in (("grad", None), ("param", None), ("grad", base + 4), ("param", base + 8),
                         ("mask", base + 2)):
        bad = _lib.AdamArgs.from_buffer_copy(ad)
        setattr(bad, field, value)
        assert f(ctypes.addressof(bad), acc, n, ctl, part, parts(n), None) == -1, field


@pytest.mark.parametrize("k", [0, -1, 65537, 2.0, "2", None, True])
def test_bad_accum_steps_raises_before_the_device_check(k):
    from realnvp_hip.trainer import FlowTrainer
    with pytest.raises(ValueError):
        FlowTrainer(torch.nn.Linear(1, 1), 4, accum_steps=k)


def test_accumulation_with_a_process_group_is_refused_before_the_device_check():
    from realnvp_hip.trainer import FlowTrainer
    with pytest.raises(ValueError, match="process_group"):
        FlowTrainer(torch.nn.Linear(1, 1), 4, accum_steps=2, process_group=object())
    # a valid accum_steps gets as far as the device check (a CPU model)
    with pytest.raises(RuntimeError):
        FlowTrainer(torch.nn.Linear(1, 1), 4, accum_steps=2)
