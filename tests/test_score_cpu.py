"""Host side of the scoring (include/realnvp_hip.h, "scoring"): the control
block's mirror, the argument checks of rnvp_score_in_fwd / rnvp_score_finish
and FlowScorer's own, and its host arithmetic; no GPU needed."""
import ctypes

import pytest
import torch

vp, i32, u64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_float


def _dll():
    from realnvp_hip import _lib
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("rnvp_version", "rnvp_score_struct_size", "rnvp_score_in_fwd", "rnvp_score_finish"):
        getattr(dll, name).restype = ctypes.c_int
    dll.rnvp_score_in_fwd.argtypes = [vp, vp, u64, vp, f32, vp, vp, i32, i32, i32, i32, vp]
    dll.rnvp_score_finish.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, vp]
    return dll


def test_block_mirror_matches_the_library():
    from realnvp_hip import _lib
    dll = _dll()
    assert dll.rnvp_version() >= 113
    S = _lib.ScoreCtl
    assert dll.rnvp_score_struct_size() == ctypes.sizeof(S) == 56
    assert [n for n, _ in S._fields_] == ["scores", "cap", "first", "n_scored", "ll_sum", "n_valid", "n_draws",
                                          "draw", "overflow"]
    assert [getattr(S, n).offset for n, _ in S._fields_] == [0, 8, 16, 24, 32, 40, 44, 48, 52]
    for name in ("rnvp_score_struct_size", "rnvp_score_in_fwd", "rnvp_score_finish"):
        assert name in _lib.EXPORTED
    assert callable(_lib.lib().score_in_fwd) and callable(_lib.lib().score_finish)


def test_a_library_with_another_block_is_refused(monkeypatch):
    from realnvp_hip import _lib

    class Grown(ctypes.Structure):
        _fields_ = list(_lib.ScoreCtl._fields_) + [("extra", ctypes.c_longlong)]
    monkeypatch.setattr(_lib, "ScoreCtl", Grown)
    with pytest.raises(RuntimeError, match="stale build"):
        _lib._Lib()
    monkeypatch.undo()
    _lib._Lib()


def test_entry_points_reject_bad_arguments_without_launch():
    """RNVP_E_INVALID (-1) before any HIP call: the pointers below are host
    addresses, a launch would fault."""
    dll = _dll()
    buf = (ctypes.c_double * 1024)()
    a = (ctypes.addressof(buf) + 15) // 16 * 16
    x, noise, y, ld, ctl = a, a + 1024, a + 2048, a + 3072, a + 4096
    B, Cc, H, W = 2, 3, 4, 4
    inf = dll.rnvp_score_in_fwd
    good = dict(x=x, noise=noise, ctl=ctl, y=y, ld=ld, B=B, C=Cc, H=H, W=W)

    def call_in(**kw):
        g = dict(good, **kw)
        return inf(g["x"], g["noise"], 7, g["ctl"], 0.9, g["y"], g["ld"], g["B"], g["C"], g["H"], g["W"], None)
    bad_in = [dict(x=None), dict(y=None), dict(ld=None), dict(ctl=None),                      # null pointers
              dict(x=x + 2), dict(noise=noise + 1), dict(y=y + 2), dict(ld=ld + 3), dict(ctl=ctl + 4),   # misaligned
              dict(B=-1), dict(C=0), dict(H=0), dict(W=-3), dict(C=1 << 15, H=1 << 15, W=4),
              dict(B=0, x=None), dict(B=0, ctl=ctl + 4), dict(B=0, C=0)]     # checked before B == 0 is accepted
    for kw in bad_in:
        assert call_in(**kw) == -1, kw
    assert call_in(B=0) == 0 and call_in(B=0, noise=None) == 0

    fin = dll.rnvp_score_finish
    z, ldj, run, lp = x, noise, y, a + 5120
    goodf = dict(z=z, ldj=ldj, ld=ld, run=run, lp=lp, ctl=ctl, B=B, n=48)

    def call_fin(**kw):
        g = dict(goodf, **kw)
        return fin(g["z"], g["ldj"], g["ld"], g["run"], g["lp"], g["ctl"], g["B"], g["n"], None)
    bad_fin = [dict(z=None), dict(ldj=None), dict(ld=None), dict(run=None), dict(ctl=None),
               dict(z=z + 1), dict(ldj=ldj + 2), dict(ld=ld + 2), dict(run=run + 3), dict(lp=lp + 2), dict(ctl=ctl + 4),
               dict(B=-1), dict(n=0), dict(n=-48),
               dict(B=0, z=None), dict(B=0, ctl=ctl + 4), dict(B=0, n=0)]
    for kw in bad_fin:
        assert call_fin(**kw) == -1, kw
    assert call_fin(B=0) == 0 and call_fin(B=0, lp=None) == 0


@pytest.mark.parametrize("k", [0, -1, 1.0, 2.5, "3", None, True])
def test_bad_n_draws_raises_before_the_device_is_looked_at(k):
    from realnvp_hip import FlowScorer
    with pytest.raises(ValueError, match="n_draws"):
        FlowScorer(torch.nn.Linear(1, 1), 4, n_draws=k)


def test_cpu_model_is_refused():
    from realnvp_hip import FlowScorer
    with pytest.raises(RuntimeError, match="HIP device"):
        FlowScorer(torch.nn.Linear(1, 1).eval(), 4, n_draws=2)
    with pytest.raises(ValueError, match="batch_size"):
        FlowScorer(torch.nn.Linear(1, 1).eval(), 0)


def test_mean_of_batch_means():
    """N = 10 scores at B = 4: the reference loop's mean over batches of
    4, 4 and 2 rows, each batch's mean over its own rows"""
    from realnvp_hip.scorer import mean_of_batch_means
    s = torch.tensor([-3.0, 1.5, 2.25, -7.0, 11.0, 0.5, -2.0, 4.0, 100.0, -60.0], dtype=torch.float64) * 1e3
    want = (float(s[0:4].sum()) / 4 + float(s[4:8].sum()) / 4 + float(s[8:10].sum()) / 2) / 3
    got = mean_of_batch_means(s.float(), 4)
    assert abs(got - want) <= 1e-12 * abs(want)
    assert abs(got - float(s.mean())) > 1.0                  # not the per-image mean
    assert mean_of_batch_means(s[:8].float(), 4) == float(s[:8].mean())     # no ragged batch: the same thing
    assert mean_of_batch_means(s[:3].float(), 4) == float(s[:3].mean())     # one short batch
    with pytest.raises(ValueError):
        mean_of_batch_means(s[:0], 4)


def test_bits_per_dim_matches_the_oracle():
    import realnvp_oracle as O
    from realnvp_hip.scorer import bits_per_dim
    s = torch.tensor([-2100.5, -1999.25, -2500.0, -1800.125], dtype=torch.float32)
    D = 3 * 16 * 16
    per = bits_per_dim(s, D)
    assert per.dtype == torch.float32 and tuple(per.shape) == (4,)
    for v, p in zip(s.tolist(), per.tolist()):
        want = float(O.bits_per_dim(v, 16, 3))
        assert abs(p - want) <= 2e-7 * abs(want)
    m = float(s.double().mean())
    assert bits_per_dim(m, D) == pytest.approx(float(O.bits_per_dim(m, 16, 3)), rel=1e-15)
