"""Host side of the latents (include/realnvp_hip.h, "latents"): the control
block's mirror, the argument checks of rnvp_latent_draw / rnvp_latent_out /
rnvp_latent_mix and FlowCodec's own, and the float64 mirrors that the GPU
tests compare the kernels against; no GPU needed."""
import ctypes

import numpy as np
import pytest
import torch

vp, i32, i64, u64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_uint64, ctypes.c_float


def _dll():
    from realnvp_hip import _lib
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("rnvp_version", "rnvp_latent_struct_size", "rnvp_latent_draw", "rnvp_latent_out", "rnvp_latent_mix"):
        getattr(dll, name).restype = ctypes.c_int
    dll.rnvp_latent_draw.argtypes = [vp, u64, vp, i32, i64, vp]
    dll.rnvp_latent_out.argtypes = [vp, vp, f32, i32, i64, i32, vp]
    dll.rnvp_latent_mix.argtypes = [vp, vp, vp, vp, i32, i32, i64, i32, vp, vp]
    return dll


def test_block_mirror_matches_the_library():
    from realnvp_hip import _lib
    dll = _dll()
    assert dll.rnvp_version() >= 114
    S = _lib.LatentCtl
    assert dll.rnvp_latent_struct_size() == ctypes.sizeof(S) == 48
    assert [n for n, _ in S._fields_] == ["dst", "cap", "first", "n_done", "temperature", "n_valid", "overflow", "pad"]
    assert [getattr(S, n).offset for n, _ in S._fields_] == [0, 8, 16, 24, 32, 36, 40, 44]
    for name in ("rnvp_latent_struct_size", "rnvp_latent_draw", "rnvp_latent_out", "rnvp_latent_mix"):
        assert name in _lib.EXPORTED
    L = _lib.lib()
    assert callable(L.latent_draw) and callable(L.latent_out) and callable(L.latent_mix)
    assert (_lib.RNVP_OUT_F32, _lib.RNVP_OUT_U8_ROUND, _lib.RNVP_OUT_U8_FLOOR) == (0, 1, 2)
    assert (_lib.RNVP_MIX_LERP, _lib.RNVP_MIX_SLERP) == (0, 1)


def test_a_library_with_another_block_is_refused(monkeypatch):
    from realnvp_hip import _lib

    class Grown(ctypes.Structure):
        _fields_ = list(_lib.LatentCtl._fields_) + [("extra", ctypes.c_longlong)]
    monkeypatch.setattr(_lib, "LatentCtl", Grown)
    with pytest.raises(RuntimeError, match="stale build"):
        _lib._Lib()
    monkeypatch.undo()
    _lib._Lib()


def test_entry_points_reject_bad_arguments_without_launch():
    """RNVP_E_INVALID (-1) before any HIP call: the pointers below are host
    addresses, a launch would fault."""
    dll = _dll()
    buf = (ctypes.c_double * 1024)()
    a0 = (ctypes.addressof(buf) + 15) // 16 * 16
    z, ctl = a0, a0 + 4096
    B, n = 2, 48
    big = 1 << 62

    def draw(**kw):
        g = dict(dict(z=z, ctl=ctl, B=B, n=n), **kw)
        return dll.rnvp_latent_draw(g["z"], 7, g["ctl"], g["B"], g["n"], None)
    for kw in [dict(z=None), dict(ctl=None), dict(z=z + 2), dict(z=z + 1), dict(ctl=ctl + 4), dict(B=-1), dict(n=-1),
               dict(B=4, n=big), dict(B=0, z=None), dict(B=0, ctl=ctl + 4), dict(n=0, ctl=None), dict(B=0, n=-5)]:
        assert draw(**kw) == -1, kw
    assert draw(B=0) == 0 and draw(n=0) == 0

    def out(**kw):
        g = dict(dict(x=z, ctl=ctl, B=B, n=n, mode=0), **kw)
        return dll.rnvp_latent_out(g["x"], g["ctl"], 0.9, g["B"], g["n"], g["mode"], None)
    for kw in [dict(x=None), dict(ctl=None), dict(x=z + 2), dict(ctl=ctl + 4), dict(B=-1), dict(n=-48),
               dict(B=4, n=big), dict(mode=3), dict(mode=-1), dict(B=0, x=None), dict(B=0, ctl=ctl + 4),
               dict(B=0, mode=7), dict(n=0, mode=3)]:
        assert out(**kw) == -1, kw
    for mode in (0, 1, 2):
        assert out(B=0, mode=mode) == 0 and out(n=0, mode=mode) == 0

    a, b, t, o, ws = a0, a0 + 1024, a0 + 2048, a0 + 3072, a0 + 6144
    P, T = 2, 3

    def mix(**kw):
        g = dict(dict(a=a, b=b, t=t, o=o, P=P, T=T, n=n, mode=1, ws=ws), **kw)
        return dll.rnvp_latent_mix(g["a"], g["b"], g["t"], g["o"], g["P"], g["T"], g["n"], g["mode"], g["ws"], None)
    for kw in [dict(a=None), dict(b=None), dict(t=None), dict(o=None), dict(ws=None),
               dict(a=a + 2), dict(b=b + 1), dict(t=t + 2), dict(o=o + 3), dict(ws=ws + 4),
               dict(P=-1), dict(T=-1), dict(n=-1), dict(n=big), dict(P=1 << 16, T=1 << 16, n=0),
               dict(mode=2), dict(mode=-1), dict(P=0, a=None), dict(T=0, ws=ws + 4), dict(n=0, mode=5)]:
        assert mix(**kw) == -1, kw
    for mode in (0, 1):
        assert mix(P=0, mode=mode) == 0 and mix(T=0, mode=mode) == 0 and mix(n=0, mode=mode) == 0
    assert mix(P=0, mode=0, ws=None) == 0          # lerp needs no workspace


def _words(s):
    return [int(w, 16) for w in s.split()]


@pytest.mark.parametrize("counter, key, want", [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
], ids=["zeros", "ones", "pi"])
def test_philox4x32_known_answers(counter, key, want):
    from realnvp_hip.codec import philox4x32
    got = philox4x32(_words(counter), _words(key))
    assert got.dtype == np.uint32 and got.shape == (4,)
    assert [int(w) for w in got] == _words(want)


def test_philox4x32_is_vectorised():
    from realnvp_hip.codec import philox4x32
    ctr = np.array([_words("00000000 00000000 00000000 00000000"), _words("243f6a88 85a308d3 13198a2e 03707344")])
    one = philox4x32(ctr, _words("a4093822 299f31d0"))
    assert one.shape == (2, 4)
    assert [int(w) for w in one[1]] == _words("d16cfe09 94fdcceb 5001e420 24126ea1")
    assert [int(w) for w in one[0]] == [int(w) for w in philox4x32(ctr[0], _words("a4093822 299f31d0"))]


def test_prior_reference_moments_and_identity():
    """65,536 values of seed 5 from index 0: |mean| <= 5 / sqrt(N), |var - 1|
    <= 5 sqrt(2 / N) (five standard errors of either statistic of a standard
    normal sample); a value belongs to its global index."""
    from realnvp_hip.codec import prior_reference
    N = 65536
    g = prior_reference(5, 0, 64, 1024)
    assert g.dtype == np.float64 and g.shape == (64, 1024)
    mean, var, top = float(g.mean()), float(g.var()), float(np.abs(g).max())
    print("mean %.4f var %.4f max |g| %.2f" % (mean, var, top))
    assert abs(mean) <= 5.0 / np.sqrt(N) and abs(var - 1.0) <= 5.0 * np.sqrt(2.0 / N)
    assert top <= np.sqrt(2.0 * 24 * np.log(2.0)) + 1e-12            # u1 >= 2^-24
    # rows 3.. of a pass are rows 0.. of one that starts at 3; the temperature only scales; another seed differs
    assert np.array_equal(prior_reference(5, 3, 2, 1024), g[3:5])
    assert np.array_equal(prior_reference(5, 0, 1, 4096).reshape(4, 1024), g[:4])
    assert np.array_equal(prior_reference(5, 0, 2, 1024, 0.5), 0.5 * g[:2])
    assert not np.any(prior_reference(5, 0, 2, 1024, 0.0))
    assert np.abs(prior_reference(6, 0, 2, 1024) - g[:2]).max() > 1.0
    # beyond 2^32 elements the index carries into the second counter word
    far = prior_reference(5, 1 << 30, 1, 16)
    assert np.isfinite(far).all() and np.abs(far - g[0, :16]).max() > 0.1


def test_mix_reference():
    from realnvp_hip.codec import mix_reference
    rng = np.random.default_rng(3)
    a = rng.standard_normal((3, 2, 4, 4))
    b = rng.standard_normal((3, 2, 4, 4))
    b[1] = a[1]
    b[2] *= np.linalg.norm(a[2]) / np.linalg.norm(b[2])               # pair 2: equal norms
    t = [0.0, 0.25, 0.5, 0.75, 1.0]
    for mode in ("lerp", "slerp"):
        out = mix_reference(a, b, t, mode)
        assert out.dtype == np.float64 and out.shape == (3, 5, 2, 4, 4)
        assert np.array_equal(out[:, 0], a) and np.array_equal(out[:, 4], b)          # the ends, exactly
        assert np.abs(out[1] - a[1][None]).max() <= 1e-15                             # a = b gives a
    lerp, slerp = mix_reference(a, b, t, "lerp"), mix_reference(a, b, t, "slerp")
    assert np.allclose(lerp[:, 2], 0.5 * (a + b), rtol=0, atol=1e-15)
    r = np.linalg.norm(a[2])
    norms = np.linalg.norm(slerp[2].reshape(5, -1), axis=1)
    assert np.abs(norms / r - 1.0).max() <= 1e-12                                     # slerp keeps the norm
    assert np.linalg.norm(lerp[2, 2]) < 0.95 * r                                      # lerp does not
    # float32 endpoints are taken to float64 first
    assert np.array_equal(mix_reference(a.astype(np.float32), b.astype(np.float32), t, "slerp"),
                          mix_reference(a.astype(np.float32).astype(np.float64),
                                        b.astype(np.float32).astype(np.float64), t, "slerp"))
    # a zero endpoint has no direction: the lerp weights
    z = np.zeros_like(a[:1])
    assert np.array_equal(mix_reference(z, b[:1], t, "slerp"), mix_reference(z, b[:1], t, "lerp"))
    with pytest.raises(ValueError):
        mix_reference(a, b, t, "cubic")
    with pytest.raises(ValueError):
        mix_reference(a, b[:2], t)


@pytest.mark.parametrize("kw", [dict(batch_size=0), dict(batch_size=2.0), dict(batch_size=True),
                                dict(temperature=-0.1), dict(temperature=float("nan")), dict(temperature="1"),
                                dict(temperature=float("inf"))])
def test_bad_construction_raises_before_the_device_is_looked_at(kw):
    from realnvp_hip import FlowCodec
    kw = dict(dict(batch_size=4), **kw)
    with pytest.raises(ValueError, match="batch_size|temperature"):
        FlowCodec(torch.nn.Linear(1, 1).eval(), kw.pop("batch_size"), **kw)


def test_cpu_model_is_refused():
    from realnvp_hip import FlowCodec
    with pytest.raises(RuntimeError, match="HIP device"):
        FlowCodec(torch.nn.Linear(1, 1).eval(), 4)


def test_argument_checks_of_the_helpers():
    from realnvp_hip import codec
    assert [codec.check_u8(u) for u in (None, "round", "floor")] == [0, 1, 2]
    for bad in ("ceil", "", 8, True, b"round"):
        with pytest.raises(ValueError, match="u8"):
            codec.check_u8(bad)
    assert codec.check_temperature(0) == 0.0 and codec.check_temperature(0.7) == 0.7
