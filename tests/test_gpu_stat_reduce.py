"""The conv epilogues' batch-statistic tails (row_stats16, csrc/common.h): the
transposing 16-lane reduction leaves every sum in its own lane, and that lane
parks it -- where lane 0 used to hold and park all of them.

Exact-integer data through the C ABI, one aligned and one ragged shape per
kernel family, bf16 and fp32 where the family has both: activations in
[-2, 2], weight rows of 16 entries +-1 (so |y| <= 32, exact in bf16, and every
product and partial sum an integer far below 2^24: the reference asserts it),
the epilogue BatchNorm with mean 0, rstd 1, gamma 1, beta 0 and integer inputs
(so the ReLU mask is x > 0 and xhat = x).  The sums are then exact in fp64 in
ANY order, and out_sums (forward) and epi_sums (data gradient with the ReLU/BN
epilogue), added over their shards, must be bit-equal to the integer numpy
computation: zero differing elements, no tolerance.

Families (rnvp_conv2d_family tells deep / streaming 1x1 / band apart; halo,
tiled, stream and band1 all report RNVP_FAMILY_OTHER, so for those _other_kernel
walks the routing of csrc/conv.hip with the launchers themselves -- the band
predicate and the persistent band kernel's dry run, then the stream, halo and
tiled launchers in the dispatch's order on scratch outputs -- and the case
asserts which one takes the conv): the deep tiles by forced configuration (4:
8 waves, 0: 4 waves with the k-split, 2: 4 waves with a tile row each), the
halo kernel (3x3, 96 channels: no deep configuration, too wide for the stream
kernel), the tiled GEMM (variant 1, 96 outputs), the stream kernel (variant 1,
<= 64 channels), the band kernels at 32k pixels (bf16: the persistent one;
band1, one band per workgroup: fp32, and bf16 at 16 outputs, which the
persistent kernel declines), the streaming 1x1 at 16k pixels and its fan-out
group.

Coupling kernels (their seg_red sits on the same DPP moves): rnvp_coupling_out_u
on a checkerboard and a channelwise coupling and the final link's
rnvp_coupling_link_fwd, on the arenas of the smallest trainer the link tests use
(32x32, base 8, 1 block, batch 4; fp32), class sums against float64 numpy
from x, the net output and the scale parameters read back, at 1e-5 (the fp32
tolerance of the C-ABI tests, tests/test_gpu_bn_table.py).
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5
FAM_OTHER, FAM_DEEP, FAM_S1, FAM_BAND = 0, 1, 2, 3
DEEP0 = 16          # RNVP_VARIANT_DEEP0


def _stream():
    return torch.cuda.current_stream().cuda_stream


# name, dtypes, B, H, W, cin, cout, ks, variant, family, the RNVP_FAMILY_OTHER kernel
CASES = [
    ("deep8_aligned", ("bf16", "fp32"), 1, 8, 8, 256, 32, 1, DEEP0 + 4, FAM_DEEP, None),
    ("deep8_ragged", ("bf16", "fp32"), 1, 5, 5, 256, 40, 3, DEEP0 + 4, FAM_DEEP, None),
    ("deep4_aligned", ("bf16", "fp32"), 1, 8, 8, 128, 32, 1, DEEP0 + 0, FAM_DEEP, None),
    ("deep4_ragged", ("bf16", "fp32"), 1, 5, 5, 128, 40, 3, DEEP0 + 0, FAM_DEEP, None),
    ("deep4row_aligned", ("bf16", "fp32"), 4, 8, 8, 128, 64, 1, DEEP0 + 2, FAM_DEEP, None),
    ("deep4row_ragged", ("bf16", "fp32"), 1, 5, 5, 128, 40, 1, DEEP0 + 2, FAM_DEEP, None),
    ("halo_aligned", ("bf16", "fp32"), 1, 8, 8, 96, 96, 3, 0, FAM_OTHER, "halo"),
    ("halo_ragged", ("bf16", "fp32"), 1, 5, 5, 96, 88, 3, 0, FAM_OTHER, "halo"),
    ("tiled_aligned", ("bf16", "fp32"), 1, 8, 8, 96, 96, 3, 1, FAM_OTHER, "tiled"),
    ("tiled_ragged", ("bf16", "fp32"), 1, 5, 5, 96, 88, 1, 1, FAM_OTHER, "tiled"),
    ("stream_aligned", ("bf16", "fp32"), 1, 8, 8, 32, 32, 3, 1, FAM_OTHER, "stream"),
    ("stream_ragged", ("bf16", "fp32"), 1, 5, 5, 24, 40, 1, 1, FAM_OTHER, "stream"),
    ("band_aligned", ("bf16",), 8, 64, 64, 32, 32, 3, 0, FAM_BAND, None),
    ("band_ragged", ("bf16",), 9, 61, 60, 32, 40, 3, 0, FAM_BAND, None),
    ("band1_aligned", ("fp32",), 8, 64, 64, 32, 32, 3, 0, FAM_OTHER, "band1"),
    ("band1_ragged", ("fp32",), 9, 61, 60, 32, 40, 3, 0, FAM_OTHER, "band1"),
    ("band1n16_aligned", ("bf16",), 8, 64, 64, 32, 16, 3, 0, FAM_OTHER, "band1"),
    ("band1n16_ragged", ("bf16",), 9, 61, 60, 32, 16, 3, 0, FAM_OTHER, "band1"),
    ("s1_aligned", ("bf16",), 4, 64, 64, 32, 32, 1, 0, FAM_S1, None),
    ("s1_ragged", ("bf16",), 1, 129, 129, 24, 40, 1, 0, FAM_S1, None),
]
PARAMS = [(c, dt) for c in CASES for dt in c[1]]


def _ints(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float64)


def _weights(rng, cout, ks, cin):
    """[cout][ks][ks][cin]: 16 entries +-1 per output row"""
    K = ks * ks * cin
    w = np.zeros((cout, K))
    for o in range(cout):
        idx = rng.choice(K, size=16, replace=False)
        w[o, idx] = rng.choice([-1.0, 1.0], size=16)
    return w.reshape(cout, ks, ks, cin)


def _conv_ref(x, w, B, H, W):
    """y[m][co] = sum over taps of x[m + tap] . w[co][tap] (zero padding), in float64 on integers (exact)"""
    M, ci = x.shape
    ks = w.shape[1]
    x4 = x.reshape(B, H, W, ci)
    y = np.zeros((M, w.shape[0]))
    for ky in range(ks):
        for kx in range(ks):
            dy, dx = ky - ks // 2, kx - ks // 2
            sh = np.zeros_like(x4)
            ys, ye = max(0, -dy), min(H, H - dy)
            xs, xe = max(0, -dx), min(W, W - dx)
            sh[:, ys:ye, xs:xe] = x4[:, ys + dy:ye + dy, xs + dx:xe + dx]
            y += sh.reshape(M, ci) @ w[:, ky, kx, :].T
    return y


def _exact(*arrays):
    """the reference stays in the exact range: integers, every |value|, every
    square and every column's sum of magnitudes below 2^24 (so any partial sum
    is exact in fp32, let alone fp64)"""
    for a in arrays:
        assert np.array_equal(a, np.rint(a))
        assert np.abs(a).max() < 2 ** 12, np.abs(a).max()
        assert np.abs(a).sum(0).max() < 2 ** 24 and (a * a).sum(0).max() < 2 ** 24


def _bits_differ(got, ref):
    return int((got.view(np.int64) != np.ascontiguousarray(ref, dtype=np.float64).view(np.int64)).sum())


def _unit_bn(M, Cc):
    """a BatchNorm source with mean 0, rstd 1.0f exactly, gamma 1, beta 0"""
    from realnvp_hip._lib import BNSrc
    from realnvp_hip.engine import stat_shards
    sh = stat_shards(M)
    eps_d = np.float64(np.float32(EPS))
    var = (1.0 - eps_d) * M / M
    assert np.float32(1.0 / np.sqrt(var + eps_d)) == np.float32(1.0)
    sums = torch.zeros(sh, 2, Cc, dtype=torch.float64, device=DEV)
    sums[0, 1] = float((1.0 - eps_d) * M)
    gam, bet = torch.ones(Cc, device=DEV), torch.zeros(Cc, device=DEV)
    return BNSrc(sums.data_ptr(), float(M), None, None, gam.data_ptr(), bet.data_ptr(), EPS, sh), (sums, gam, bet), sh


def _problem(case, seed):
    _, _, B, H, W, cin, cout, ks = case[:8]
    rng = np.random.default_rng(seed)
    M = B * H * W
    x = _ints(rng, -2, 2, (M, cin))
    ex = _ints(rng, -3, 3, (M, cout))
    w = _weights(rng, cout, ks, cin)
    y = _conv_ref(x, w, B, H, W)
    out = y * (ex > 0)
    _exact(y, out, out * ex)
    return M, x, ex, w, y, out


# one reference per case, shared by the dtypes
_REF = {}


def _ref(case):
    if case[0] not in _REF:
        _REF[case[0]] = _problem(case, 11)
    return _REF[case[0]]


def _args(case, dtype, xd, wp, y, kp):
    from realnvp_hip._lib import ConvArgs
    _, _, B, H, W, cin, cout, ks, variant = case[:9]
    a = ConvArgs()
    a.dtype, a.B, a.H, a.W, a.ks = (0 if dtype == "fp32" else 1), B, H, W, ks
    a.x, a.cs_in, a.cin, a.w, a.kp = xd.data_ptr(), cin, cin, wp.data_ptr(), kp
    a.y, a.cs_out, a.n = y.data_ptr(), cout, cout
    a.variant = variant
    return a


_LAUNCHERS = {   # (csrc/conv_common.h; C++ linkage)
    "band_ok": "_Z17rnvp_conv_band_okPK14rnvp_conv_args",
    "band2": "_Z22rnvp_conv_band2_launchPK14rnvp_conv_argsP12ihipStream_tb",
    "stream": "_Z23rnvp_conv_stream_launchPK14rnvp_conv_argsP12ihipStream_t",
    "halo": "_Z21rnvp_conv_halo_launchPK14rnvp_conv_argsP12ihipStream_t",
    "tiled": "_Z22rnvp_conv_tiled_launchPK14rnvp_conv_argsP12ihipStream_t",
}


def _other_kernel(a):
    """Which RNVP_FAMILY_OTHER kernel dispatch_conv (csrc/conv.hip) reaches for
    a: its order, asked of the launchers themselves (a declining launcher
    launches nothing; a's outputs must be scratch)."""
    from realnvp_hip import _lib
    dll = _lib.lib().dll
    fn = {k: getattr(dll, v) for k, v in _LAUNCHERS.items()}
    fn["band_ok"].restype = C.c_bool
    fn["band_ok"].argtypes = [C.c_void_p]
    fn["band2"].restype = C.c_int
    fn["band2"].argtypes = [C.c_void_p, C.c_void_p, C.c_bool]
    for k in ("stream", "halo", "tiled"):
        fn[k].restype = C.c_int
        fn[k].argtypes = [C.c_void_p, C.c_void_p]
    tuned = a.variant != 1
    pa, s = C.addressof(a), _stream()
    if tuned and fn["band_ok"](pa):
        assert fn["band2"](pa, None, True) != 0, "the persistent band kernel takes it"
        return "band1"
    order = ("stream", "halo", "tiled") if tuned else ("stream", "tiled")
    for k in order:
        rc = fn[k](pa, s)
        torch.cuda.synchronize()
        if rc == 0:
            return k
        assert rc == -2, (k, rc)        # RNVP_E_UNSUPPORTED
    return None


@pytest.mark.parametrize("case,dtype", PARAMS, ids=["%s_%s" % (c[0], dt) for c, dt in PARAMS])
def test_conv_sums_bit_equal(case, dtype):
    from realnvp_hip import _lib
    from realnvp_hip.engine import stat_shards
    L = _lib.lib()
    _, _, B, H, W, cin, cout, ks, variant, fam, kernel = case
    assert cin % 8 == 0 and cout % 8 == 0      # (channel strides = channel counts)
    M, x, ex, w, y_ref, out_ref = _ref(case)
    tdt = torch.float32 if dtype == "fp32" else torch.bfloat16
    kp = (ks * ks * cin + 63) // 64 * 64
    wp = torch.zeros(cout, kp, dtype=tdt, device=DEV)
    wp[:, :ks * ks * cin] = torch.from_numpy(w.reshape(cout, -1)).to(DEV).to(tdt)
    xd = torch.from_numpy(x).to(DEV).to(tdt)
    exd = torch.from_numpy(ex).to(DEV).to(tdt)
    sh = stat_shards(M)

    # forward: out_sums
    y = torch.zeros(M, cout, dtype=tdt, device=DEV)
    osum = torch.zeros(sh, 2, cout, dtype=torch.float64, device=DEV)
    a = _args(case, dtype, xd, wp, y, kp)
    a.out_sums = osum.data_ptr()
    assert L.conv2d_family(C.byref(a)) == fam, (L.conv2d_family(C.byref(a)), fam)
    if kernel is not None:      # (on scratch outputs: the walk launches the kernel it finds)
        ys, oss = torch.zeros_like(y), torch.zeros_like(osum)
        b = _args(case, dtype, xd, wp, ys, kp)
        b.out_sums = oss.data_ptr()
        assert _other_kernel(b) == kernel
    L.conv2d(C.byref(a), _stream())
    torch.cuda.synchronize()
    got = osum.sum(0).cpu().numpy()
    d_y = int((y.double().cpu().numpy() != y_ref).sum())
    d_f = _bits_differ(got, np.stack([y_ref.sum(0), (y_ref * y_ref).sum(0)]))

    # data gradient with the ReLU/BN epilogue: epi_sums
    bn, keep, bsh = _unit_bn(M, cout)
    y2 = torch.zeros(M, cout, dtype=tdt, device=DEV)
    esum = torch.zeros(bsh, 2, cout, dtype=torch.float64, device=DEV)
    a = _args(case, dtype, xd, wp, y2, kp)
    a.epi_relu_bn_bwd, a.epi_x, a.epi, a.epi_sums = 1, exd.data_ptr(), bn, esum.data_ptr()
    assert L.conv2d_family(C.byref(a)) == fam, (L.conv2d_family(C.byref(a)), fam)
    if kernel is not None:
        ys, ess = torch.zeros_like(y2), torch.zeros_like(esum)
        b = _args(case, dtype, xd, wp, ys, kp)
        b.epi_relu_bn_bwd, b.epi_x, b.epi, b.epi_sums = 1, exd.data_ptr(), bn, ess.data_ptr()
        assert _other_kernel(b) == kernel
    L.conv2d(C.byref(a), _stream())
    torch.cuda.synchronize()
    got = esum.sum(0).cpu().numpy()
    d_y2 = int((y2.double().cpu().numpy() != out_ref).sum())
    d_e = _bits_differ(got, np.stack([out_ref.sum(0), (out_ref * ex).sum(0)]))
    print("differing elements: y %d, out_sums %d / %d, dgrad y %d, epi_sums %d / %d" %
          (d_y, d_f, 2 * cout, d_y2, d_e, 2 * cout))
    assert d_y == 0 and d_y2 == 0
    assert d_f == 0 and d_e == 0


FAN = [("fan_aligned", 8, 64, 64, 32, 32), ("fan_ragged", 1, 129, 129, 24, 40)]


@pytest.mark.parametrize("case", FAN, ids=[c[0] for c in FAN])
def test_fanout_sums_bit_equal(case):
    """two 1x1 convs sharing their input at a wide scale (k_s1_fanout, bf16), one of them with out_sums"""
    from realnvp_hip import _lib
    from realnvp_hip._lib import ConvArgs, NetStep
    from realnvp_hip.engine import stat_shards
    L = _lib.lib()
    name, B, H, W, cin, cout = case
    full = (name, ("bf16",), B, H, W, cin, cout, 1, 0, FAM_S1, None)
    M, x, _, w, y_ref, _ = _problem(full, 13)
    w2 = _weights(np.random.default_rng(17), cout, 1, cin)
    y2_ref = _conv_ref(x, w2, B, H, W)
    tdt = torch.bfloat16
    kp = (cin + 63) // 64 * 64
    xd = torch.from_numpy(x).to(DEV).to(tdt)
    sh = stat_shards(M)
    osum = torch.zeros(sh, 2, cout, dtype=torch.float64, device=DEV)
    ys, wps, args = [], [], []
    for i, wi in enumerate((w, w2)):
        wp = torch.zeros(cout, kp, dtype=tdt, device=DEV)
        wp[:, :cin] = torch.from_numpy(wi.reshape(cout, -1)).to(DEV).to(tdt)
        y = torch.zeros(M, cout, dtype=tdt, device=DEV)
        a = _args(full, "bf16", xd, wp, y, kp)
        if i == 0:
            a.out_sums = osum.data_ptr()
        ys.append(y)
        wps.append(wp)
        args.append(a)
    steps = (NetStep * 2)()
    for st, a in zip(steps, args):
        st.kind, st.conv, st.dgamma_off, st.dbeta_off = 0, a, -1, -1
    k, g, lb = C.c_int(), C.c_int(), C.c_int()
    assert L.net_group_prepare(steps, 2, C.byref(k), C.byref(g), C.byref(lb)) == 0
    assert k.value & (1 << 12), "the fan-out kernel"
    L.net_group(C.addressof(steps), 2, 1, k.value, g.value, lb.value, _stream())
    torch.cuda.synchronize()
    got = osum.sum(0).cpu().numpy()
    d_y = int((ys[0].double().cpu().numpy() != y_ref).sum()) + int((ys[1].double().cpu().numpy() != y2_ref).sum())
    d_f = _bits_differ(got, np.stack([y_ref.sum(0), (y_ref * y_ref).sum(0)]))
    print("differing elements: y %d, out_sums %d / %d" % (d_y, d_f, 2 * cout))
    assert d_y == 0 and d_f == 0


# ---------------------------------------------------------------------------
# coupling kernels: class sums against float64 numpy
# ---------------------------------------------------------------------------
COUPLING_SHARDS = 16      # RNVP_COUPLING_SHARDS


def _trainer():
    from formula_init import pixels
    from realnvp_hip.trainer import FlowTrainer
    from test_gpu_trainer import make_model
    tr = FlowTrainer(make_model(32, 8, 1), 4, dtype="fp32", seed=3)
    assert tr.links is not None
    tr.set_pixels(pixels(4, 3, 32, seed=3).to(DEV))
    tr.step_eager()           # fills every coupling's arena (x, the net output st)
    torch.cuda.synchronize()
    return tr


def _u_float64(st, nclass):
    """u [B][C][H][W] of one coupling in float64 from x, the net output and the
    scale parameters as they are on the device now, and each pixel's class"""
    import realnvp_oracle as O
    from realnvp_hip.net import chan_stride
    eng, sv, x = st.eng, st.saved, st.x
    B, Cc, H, W = x.shape
    Cb = Cc if eng.kind == 0 else Cc // 2
    T = eng._tensors()
    sc, ss = float(T["scale"].detach().double().cpu()), float(T["scale_shift"].detach().double().cpu())
    cs = chan_stride(eng.P.buf_ch["st"])
    net = sv["arena"].view("st", torch.float32)[:B * H * W * cs].view(B, H, W, cs).double().cpu().numpy()
    shift = np.transpose(net[..., :Cb], (0, 3, 1, 2))
    lr = sc * np.tanh(np.transpose(net[..., Cb:2 * Cb], (0, 3, 1, 2))) + ss
    xd = x.double().cpu().numpy()
    u = xd.copy()
    if eng.kind == 0:
        inv = 1.0 - O.checkerboard_mask(H, eng.cfg).double().numpy().reshape(1, 1, H, W)
        u = np.where(inv > 0, xd * np.exp(lr) + shift, xd)
    else:
        on = slice(0, Cb) if eng.cfg else slice(Cb, Cc)
        u[:, on] = xd[:, on] * np.exp(lr) + shift
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    q = np.zeros((H, W), dtype=np.int64) if nclass == 1 else ((i + j) & 1 if nclass == 2 else (i & 1) * 2 + (j & 1))
    return u, q


def _class_sums(v, w, q, nclass):
    """[nclass][2][C]: sums of v and w over the batch and the pixels of each class"""
    out = np.zeros((nclass, 2, v.shape[1]))
    for k in range(nclass):
        m = (q == k)
        out[k, 0] = v[:, :, m].sum((0, 2))
        out[k, 1] = w[:, :, m].sum((0, 2))
    return out


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _out_u(tr, k):
    """rnvp_coupling_out_u of coupling k into class sums of its own: (sums over shards, reference, u, q, args)"""
    from realnvp_hip import _lib
    st, link = tr.stages[tr.cidx[k]], tr.link_fwd[k]
    nc = link["nclass"]
    Cc = st.x.shape[1]
    a = st.eng.link_args(st.saved, st.x)
    cls = torch.zeros(COUPLING_SHARDS, nc, 2, Cc, dtype=torch.float64, device=DEV)
    ldj = torch.zeros(st.x.shape[0], device=DEV)
    a.nclass, a.cls_sums, a.ldj_sample, a.gl_sample = nc, cls.data_ptr(), ldj.data_ptr(), tr.g_lp.data_ptr()
    _lib.lib().coupling_out_u(C.byref(a), _stream())
    torch.cuda.synchronize()
    u, q = _u_float64(st, nc)
    return cls, _class_sums(u, u * u, q, nc), u, q, a


@pytest.mark.parametrize("kind", [0, 1], ids=["checkerboard", "channelwise"])
def test_out_u_class_sums(kind):
    tr = _trainer()
    k = next(i for i, ci in enumerate(tr.cidx) if tr.stages[ci].eng.kind == kind)
    cls, ref, _, _, _ = _out_u(tr, k)
    e = _rel(cls.sum(0).cpu().numpy(), ref)
    print("coupling %d (kind %d, %d classes, x %s): class sums of u, u^2 rel %.3g" %
          (k, kind, ref.shape[0], tuple(tr.stages[tr.cidx[k]].x.shape), e))
    assert e < 1e-5, e


def test_final_link_prior_sums():
    """rnvp_coupling_link_fwd of the last coupling (RNVP_LINK_FINAL: all of z goes
    to the prior): prior_sums = class sums of -z g_lp[b] and -z^2 g_lp[b], z =
    out_bn(u) where the coupling transforms and u elsewhere"""
    from realnvp_hip import _lib
    tr = _trainer()
    k = len(tr.cidx) - 1
    st, link = tr.stages[tr.cidx[k]], tr.link_fwd[k]
    assert link["nxt"] is None and link["args"].type == 3
    cls, _, u, q, a = _out_u(tr, k)
    nc, eng = link["nclass"], st.eng
    B, Cc, H, W = u.shape
    pri = torch.zeros(COUPLING_SHARDS, nc, 2, Cc, dtype=torch.float64, device=DEV)
    a.prior_sums = pri.data_ptr()
    _lib.lib().coupling_link_fwd(C.byref(a), None, C.byref(link["args"]), _stream())
    torch.cuda.synchronize()
    import realnvp_oracle as O
    z = u.copy()
    if eng.kind == 0:
        inv = 1.0 - O.checkerboard_mask(H, eng.cfg).double().numpy().reshape(1, 1, H, W)
        mean, var = u.mean((0, 2, 3), keepdims=True), u.var((0, 2, 3), keepdims=True)
        z = np.where(inv > 0, (u - mean) / np.sqrt(var + 1e-5), u)
    else:
        Cb = Cc // 2
        on = slice(0, Cb) if eng.cfg else slice(Cb, Cc)
        mean, var = u[:, on].mean((0, 2, 3), keepdims=True), u[:, on].var((0, 2, 3), keepdims=True)
        z[:, on] = (u[:, on] - mean) / np.sqrt(var + 1e-5)
    glp = tr.g_lp.double().cpu().numpy().reshape(B, 1, 1, 1)
    ref = _class_sums(-z * glp, -z * z * glp, q, nc)
    e = _rel(pri.sum(0).cpu().numpy(), ref)
    print("final link (kind %d, %d classes): prior sums rel %.3g" % (eng.kind, nc, e))
    assert e < 1e-5, e
