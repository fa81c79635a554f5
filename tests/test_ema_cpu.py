"""Host side of the weight averaging (realnvp_hip.stepctl: check_ema_decay,
ema_decay_at) and the argument checks of rnvp_ema_update / rnvp_ema_swap; no
GPU needed."""
import ctypes

import pytest
import torch

vp, i64 = ctypes.c_void_p, ctypes.c_longlong


def _dll():
    from realnvp_hip import _lib
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("rnvp_version", "rnvp_ema_struct_size", "rnvp_ema_update", "rnvp_ema_swap"):
        getattr(dll, name).restype = ctypes.c_int
    dll.rnvp_ema_update.argtypes = [vp, vp, i64, vp, vp, i64, vp, vp]
    dll.rnvp_ema_swap.argtypes = [vp, vp, i64, vp]
    return dll


def test_block_mirror_matches_the_library():
    from realnvp_hip import _lib
    dll = _dll()
    assert dll.rnvp_version() >= 112
    assert dll.rnvp_ema_struct_size() == ctypes.sizeof(_lib.EmaCtl) == 24
    assert [n for n, _ in _lib.EmaCtl._fields_] == ["decay", "warmup", "applied", "pad", "n_updates"]
    assert (_lib.EmaCtl.applied.offset, _lib.EmaCtl.n_updates.offset) == (8, 16)
    for name in ("rnvp_ema_struct_size", "rnvp_ema_update", "rnvp_ema_swap"):
        assert name in _lib.EXPORTED
    assert callable(_lib.lib().ema_update) and callable(_lib.lib().ema_swap)


def test_a_library_with_another_block_is_refused(monkeypatch):
    from realnvp_hip import _lib

    class Grown(ctypes.Structure):
        _fields_ = list(_lib.EmaCtl._fields_) + [("extra", ctypes.c_longlong)]
    monkeypatch.setattr(_lib, "EmaCtl", Grown)
    with pytest.raises(RuntimeError, match="stale build"):
        _lib._Lib()
    monkeypatch.undo()
    _lib._Lib()


def test_entry_points_reject_bad_arguments_without_launch():
    """RNVP_E_INVALID (-1) before any HIP call: the pointers below are host
    addresses, a launch would fault."""
    dll = _dll()
    buf = (ctypes.c_double * 4096)()         # host memory standing in for two 1028-element arenas and the blocks
    a = (ctypes.addressof(buf) + 15) // 16 * 16
    b = a + 8192
    blk, step, ctl = b + 8192, b + 8192 + 64, b + 8192 + 128
    n = 1028
    up, sw = dll.rnvp_ema_update, dll.rnvp_ema_swap
    bad_update = [
        (None, b, n, blk, step, 1, None), (a, None, n, blk, step, 1, None), (a, b, n, None, step, 1, None),
        (a, b, n, blk, None, 1, None),                                       # null pointers
        (a, b, -4, blk, step, 1, None), (a, b, n + 1, blk, step, 1, None), (a, b, n + 2, blk, step, 1, None),
        (a + 4, b, n, blk, step, 1, None), (a, b + 8, n, blk, step, 1, None),   # arenas not 16-byte aligned
        (a, b, n, blk + 4, step, 1, None), (a, b, n, blk, step + 4, 1, None), (a, b, n, blk, step, 1, ctl + 4),
        (a, a, n, blk, step, 1, None), (a, a + 16, n, blk, step, 1, None),   # overlapping arenas
        (None, b, 0, blk, step, 1, None), (a + 4, b, 0, blk, step, 1, None),  # checked before n == 0 is accepted
    ]
    for args in bad_update:
        assert up(*args, None) == -1, args
    bad_swap = [(None, b, n), (a, None, n), (a, b, -4), (a, b, n + 1), (a, b, n + 3), (a + 4, b, n), (a, b + 12, n),
                (a, a, n), (a, a + 16, n), (a + 16, a, n), (a, a, 0), (None, b, 0)]
    for args in bad_swap:
        assert sw(*args, None) == -1, args
    # nothing to do is fine, and launches nothing
    assert up(a, b, 0, blk, step, 1, None, None) == 0
    assert up(a, b, 0, blk, step, 0, ctl, None) == 0
    assert sw(a, b, 0, None) == 0


@pytest.mark.parametrize("v", [1.0, 1.5, -0.1, -1e-9, float("nan"), float("inf"), "x", "0.9", True, [0.9]])
def test_bad_ema_decay_raises(v):
    from realnvp_hip.stepctl import check_ema_decay
    from realnvp_hip.trainer import FlowTrainer
    with pytest.raises(ValueError, match="ema_decay"):
        check_ema_decay(v)
    with pytest.raises(ValueError, match="ema_decay"):      # checked before the device is looked at
        FlowTrainer(torch.nn.Linear(1, 1), 4, ema_decay=v)


def test_good_ema_decay():
    from realnvp_hip.stepctl import check_ema_decay
    assert check_ema_decay(None) is None
    assert check_ema_decay(0) == 0.0 and isinstance(check_ema_decay(0), float)
    assert check_ema_decay(0.999) == 0.999 and check_ema_decay(1.0 - 2 ** -24) < 1.0


def test_ema_decay_at():
    from realnvp_hip.stepctl import ema_decay_at
    d = ema_decay_at(0.999, True, 1)
    assert isinstance(d, float) and d == 2 / 11
    assert ema_decay_at(0.999, True, 9) == 10 / 19
    # (1 + u) / (10 + u) reaches 0.999 at u = 8990: below it the warm-up binds, from there on the decay does
    assert ema_decay_at(0.999, True, 8989) == 8990 / 8999 < 0.999
    assert abs(ema_decay_at(0.999, True, 8990) - 0.999) <= 2e-16
    assert ema_decay_at(0.999, True, 8991) == 0.999 and ema_decay_at(0.999, True, 10 ** 6) == 0.999
    for u in (1, 9, 8990, 10 ** 6):
        assert ema_decay_at(0.999, False, u) == 0.999 and ema_decay_at(0.0, False, u) == 0.0
    assert ema_decay_at(0.5, True, 1) == 2 / 11 and ema_decay_at(0.5, True, 8) == 0.5 == ema_decay_at(0.5, True, 9)


@pytest.mark.parametrize("warmup", [True, False])
def test_recurrence_is_lerp(warmup):
    """e + (1 - d)(p - e) with ema_decay_at's d over 20 random updates against
    torch.lerp(e, p, 1 - d) in float64 (swa_utils.get_ema_multi_avg_fn's
    update), to 1e-15 relative"""
    from realnvp_hip.stepctl import ema_decay_at
    gen = torch.Generator().manual_seed(3)
    p = torch.randn(257, generator=gen, dtype=torch.float64)
    ours, ref = p.clone(), p.clone()
    for u in range(1, 21):
        p = p + 0.1 * torch.randn(257, generator=gen, dtype=torch.float64)
        d = ema_decay_at(0.9, warmup, u)
        ours = ours + (1.0 - d) * (p - ours)
        ref = torch.lerp(ref, p, 1.0 - d)
    assert not torch.equal(ref, p)
    assert float((ours - ref).abs().max() / ref.abs().max()) <= 1e-15
