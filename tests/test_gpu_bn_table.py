"""Finalized BatchNorm tables (rnvp_bn_src.tab, engine.BN_TABLES): the s/t net's
BatchNorms keep mean | rstd per channel, written once per training forward by
the running-statistics update, and the backward consumers load their pair
instead of re-deriving it from the sharded fp64 sums in every workgroup.

(a) test_table_matches_float64: after a training forward of one coupling
    (1, 2 and 4 statistic shards; fp32 and bf16) EVERY float of every
    BatchNorm's table -- mean and rstd = 1/sqrt(var + eps), in both flavours
    (mean = sum * (1 / count) and mean = sum / count) -- against float64 numpy
    evaluated from the sums read back, to 1 float ulp.  (The table holds no
    scale / shift: a reader forms them in fp32 from its pair and the affine
    parameters as after its own reduction, which (b) checks bit for bit.)
(b) test_consumer_*: each consumer through the C ABI with tab = NULL and with
    the table rnvp_bn_running_update wrote from the same sums (sums spread
    over every shard): a data gradient with the ReLU/BN epilogue, one with
    the folded BatchNorm backward as well, the standalone apply with residual
    + accumulation, and a grouped weight gradient with the BN+ReLU prologue.
    BOTH results are held to the float64 restatement within the tolerance the
    suite uses for that kernel (test_gpu_conv / test_gpu_deep: 1e-5 fp32,
    4e-3 bf16; weight gradients 1e-4 bf16); the number of elements that
    differ between the two paths is printed (0 everywhere when measured).  The shapes are the smallest
    that reach each family, and the test asserts the family
    (rnvp_conv2d_family / rnvp_wgrad_class): deep tiles at M = 1,024 (1 shard)
    and 16,384 (2 shards), the streaming 1x1 and the band 3x3 at M = 32,768
    (4 shards; 32x32 C = 64 and 64x64 C = 32), weight-gradient classes 0 / 1
    at C = 128 and 2 / 3 at the wide shapes.
(c) test_trainer_step_tables_on_off: one captured step of the smallest model
    of the trainer tests (32x32, base 8, 1 block) at batch 32 (4 shards at
    scale 1) with BN_TABLES on and off: gradients, parameters and moments
    agree within test_gpu_train_equiv's floor for graph == eager, max(2 x the
    difference between two runs of the same configuration, 1e-6).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_group import _inputs, rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------
# (a) the table after a training forward
# ---------------------------------------------------------------------------
FWD_CASES = [
    # name, kind, in_out_dim, mid, size, batch, shards
    ("m1024_1shard", "ckbd", 12, 128, 8, 16, 1),
    ("m16384_2shards", "ckbd", 12, 128, 16, 64, 2),
    ("m32768_4shards", "ckbd", 6, 64, 32, 32, 4),
]


def _table_ref(sums, count, flavour):
    """float64 mean, rstd per channel from sums [shards][2][C] added in shard order."""
    s = np.zeros_like(sums[0])
    for h in range(sums.shape[0]):
        s = s + sums[h]
    mean = s[0] * (1.0 / count) if flavour == 0 else s[0] / count
    var = (s[1] * (1.0 / count) if flavour == 0 else s[1] / count) - mean * mean
    var = np.maximum(var, 0.0)
    rstd = 1.0 / np.sqrt(var + np.float64(np.float32(EPS)))
    return mean, rstd


def _check_table(tab, sums, count, what):
    """tab [C][4] fp32 = {mean, rstd} x 2 flavours against float64: the largest deviation in ulps."""
    worst = 0.0
    for fl in (0, 1):
        mean, rstd = _table_ref(sums, count, fl)
        for k, ref in ((0, mean), (1, rstd)):
            r32 = ref.astype(np.float32)
            got = tab[:, 2 * fl + k].astype(np.float64)
            ulps = np.abs(got - r32.astype(np.float64)) / np.spacing(np.abs(r32)).astype(np.float64)
            worst = max(worst, float(ulps.max()))
            assert ulps.max() <= 1.0, (what, fl, "rstd" if k else "mean", float(ulps.max()))
    return worst


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_table_matches_float64(case, dtype):
    from realnvp_hip import _lib
    _, kind, cio, mid, size, B, shards = case
    mod, x, _, _ = _inputs(kind, cio, mid, size, B)
    mod = mod.to(DEV).train()
    eng = mod.engine()
    _, _, sv = eng.forward(x.to(DEV), True, dtype, False)
    torch.cuda.synchronize()
    assert sv["shards"] == shards
    ar = sv["arena"]
    M = B * size * size
    worst = 0.0
    assert len(eng.P.bns) > 0
    for bn, spec in eng.P.bns.items():
        sums = ar.view("s:" + bn, torch.float64, (shards, 2, spec.c)).cpu().numpy()
        tab = ar.view("t:" + bn, torch.float32).view(spec.c, 4).cpu().numpy()
        assert tab.size == _lib.bn_tab_floats(spec.c)
        assert np.abs(sums[shards - 1]).max() > 0, "every shard carries a share"
        worst = max(worst, _check_table(tab, sums, float(M), bn))
    print("%d tables, largest deviation %.2f ulp" % (len(eng.P.bns), worst))


# ---------------------------------------------------------------------------
# (b) the consumers through the C ABI
# ---------------------------------------------------------------------------
def _rnd(t, dtype):
    return t.float().double() if dtype == "fp32" else t.to(torch.bfloat16).double()


class _BN:
    """A BatchNorm over t [M][C] (float64, already rounded to the net dtype):
    its sums spread over rnvp_stat_shards(M) shards, its affine, the table
    rnvp_bn_running_update writes from them, and the fp32 scale / shift /
    mean / rstd of the kernels' formula in float64."""

    def __init__(self, t, gen):
        from realnvp_hip import _lib
        from realnvp_hip._lib import BNRunning
        from realnvp_hip.engine import stat_shards, upload
        M, Cc = t.shape
        self.M, self.C, self.sh = M, Cc, stat_shards(M)
        sums = torch.zeros(self.sh, 2, Cc, dtype=torch.float64, device=DEV)
        for h, part in enumerate(torch.chunk(t, self.sh, 0)):
            sums[h, 0], sums[h, 1] = part.sum(0), (part * part).sum(0)
        self.sums = sums
        self.gam = (torch.rand(Cc, generator=gen, device=DEV) + 0.5)
        self.bet = (torch.randn(Cc, generator=gen, device=DEV) * 0.3)
        self.tab = torch.full((_lib.bn_tab_floats(Cc),), float("nan"), device=DEV)
        self.rm, self.rv = torch.zeros(Cc, device=DEV), torch.ones(Cc, device=DEV)
        self.nbt = torch.zeros(1, dtype=torch.int64, device=DEV)
        row = BNRunning(sums.data_ptr(), float(M), Cc, self.sh, self.rm.data_ptr(), self.rv.data_ptr(),
                        self.nbt.data_ptr(), EPS, self.tab.data_ptr())
        self.row = upload(bytes((BNRunning * 1)(row)), torch.device(DEV))
        _lib.lib().bn_running_update(self.row.data_ptr(), 1, Cc, 0.1, _stream())
        s = sums.sum(0)
        mean = s[0] / M
        var = (s[1] / M - mean * mean).clamp_min(0)
        self.rstd = (1.0 / torch.sqrt(var + EPS)).float().double()
        self.mean = mean.float().double()
        g, b = self.gam.double(), self.bet.double()
        self.scale = (g * self.rstd).float().double()
        self.shift = (b - self.mean * g * self.rstd).float().double()

    def src(self, with_tab):
        from realnvp_hip._lib import BNSrc
        return BNSrc(self.sums.data_ptr(), float(self.M), None, None, self.gam.data_ptr(), self.bet.data_ptr(), EPS,
                     self.sh, self.tab.data_ptr() if with_tab else None)

    def xhat(self, t):
        return (t - self.mean) * self.rstd


def _conv_ref(x, w, B, H, W):
    """float64 y[m][co] = sum over taps of x[m + tap] @ w[co][tap]^T (zero padding); w [co][ks][ks][ci]."""
    M, Ci = x.shape
    ks = w.shape[1]
    x4 = x.view(B, H, W, Ci)
    y = torch.zeros(M, w.shape[0], dtype=torch.float64, device=x.device)
    for ky in range(ks):
        for kx in range(ks):
            dy_, dx_ = ky - ks // 2, kx - ks // 2
            sh = torch.zeros_like(x4)
            ys, ye = max(0, -dy_), min(H, H - dy_)
            xs, xe = max(0, -dx_), min(W, W - dx_)
            sh[:, ys:ye, xs:xe] = x4[:, ys + dy_:ye + dy_, xs + dx_:xe + dx_]
            y += sh.reshape(M, Ci) @ w[:, ky, kx, :].T
    return y


def _pack(w, kp, tdt):
    co, ks, _, ci = w.shape
    wp = torch.zeros(co, kp, dtype=tdt, device=DEV)
    wp[:, :ks * ks * ci] = w.reshape(co, ks * ks * ci).to(tdt)
    return wp


# B, H, W, channels, family of the bf16 data gradient per kernel size (1: deep, 2: streaming 1x1, 3: band 3x3)
SHAPES = {
    "deep_m1024": (16, 8, 8, 128, {1: 1, 3: 1}),
    "deep_m16384": (64, 16, 16, 128, {1: 1, 3: 1}),
    "wide_32x32_c64": (32, 32, 32, 64, {1: 2, 3: 3}),
    "wide_64x64_c32": (8, 64, 64, 32, {1: 2, 3: 3}),
}
# the data gradient with the folded BatchNorm backward exists where rnvp_conv2d_check says so:
# deep tiles (1x1 up to 4,096 pixels, 3x3), and the bf16 streaming 1x1 / band 3x3
DGRAD = [(s, ks, dt, False) for s in SHAPES for ks in (1, 3) for dt in ("fp32", "bf16")]
DGRAD_BP = ([("deep_m1024", ks, dt, True) for ks in (1, 3) for dt in ("fp32", "bf16")] +
            [("deep_m16384", 3, dt, True) for dt in ("fp32", "bf16")] +
            [(s, ks, "bf16", True) for s in ("wide_32x32_c64", "wide_64x64_c32") for ks in (1, 3)])


def _differ(a, b):
    return int((a != b).sum()), a.numel()


@pytest.mark.parametrize("case", DGRAD + DGRAD_BP, ids=["%s_k%d_%s%s" % (c[0], c[1], c[2], "_bp" if c[3] else "")
                                                         for c in DGRAD + DGRAD_BP])
def test_consumer_dgrad(case):
    from realnvp_hip import _lib
    from realnvp_hip._lib import ConvArgs
    shape, ks, dtype, bp = case
    B, H, W, Cc, fam = SHAPES[shape]
    M = B * H * W
    L = _lib.lib()
    dt, tdt = (0, torch.float32) if dtype == "fp32" else (1, torch.bfloat16)
    gen = torch.Generator(device=DEV).manual_seed(3)
    g = _rnd(torch.randn(M, Cc, generator=gen, device=DEV), dtype)              # the conv's operand (a gradient)
    ex = _rnd(torch.randn(M, Cc, generator=gen, device=DEV) * 1.5 + 0.3, dtype)  # the epilogue BatchNorm's input
    w = _rnd(torch.randn(Cc, ks, ks, Cc, generator=gen, device=DEV) / (ks * ks * Cc) ** 0.5, dtype)
    kp = (ks * ks * Cc + 63) // 64 * 64
    wp = _pack(w, kp, tdt)
    ebn = _BN(ex, gen)
    dg, dex = g.to(tdt), ex.to(tdt)
    operand = g
    if bp:
        t = _rnd(torch.randn(M, Cc, generator=gen, device=DEV) * 1.5 + 0.3, dtype)  # the folded BatchNorm's input
        bbn = _BN(t, gen)
        xh = bbn.xhat(t)
        gsum = torch.zeros(bbn.sh, 2, Cc, dtype=torch.float64, device=DEV)
        for h, (pg, px) in enumerate(zip(torch.chunk(g, bbn.sh, 0), torch.chunk(xh, bbn.sh, 0))):
            gsum[h, 0], gsum[h, 1] = pg.sum(0), (pg * px).sum(0)
        k1, k2 = gsum[:, 0].sum(0) / M, gsum[:, 1].sum(0) / M
        dldt = bbn.gam.double() * bbn.rstd * (g - k1 - xh * k2)
        operand = _rnd(dldt, dtype)          # the kernel rounds the staged operand to the net dtype
        dt_ = t.to(tdt)
    ref = _conv_ref(operand, w, B, H, W) * ((ex * ebn.scale + ebn.shift) > 0)
    ref_s1, ref_s2 = ref.sum(0), (ref * ebn.xhat(ex)).sum(0)

    def run(with_tab):
        a = ConvArgs()
        a.dtype, a.B, a.H, a.W, a.ks = dt, B, H, W, ks
        a.x, a.cs_in, a.cin, a.w, a.kp = dg.data_ptr(), Cc, Cc, wp.data_ptr(), kp
        y = torch.zeros(M, Cc, dtype=tdt, device=DEV)
        es = torch.zeros(ebn.sh, 2, Cc, dtype=torch.float64, device=DEV)
        a.y, a.cs_out, a.n = y.data_ptr(), Cc, Cc
        a.epi_relu_bn_bwd, a.epi_x, a.epi, a.epi_sums = 1, dex.data_ptr(), ebn.src(with_tab), es.data_ptr()
        side = dgam = dbet = None
        if bp:
            side = torch.zeros(M, Cc, dtype=tdt, device=DEV)
            dgam, dbet = torch.zeros(Cc, device=DEV), torch.zeros(Cc, device=DEV)
            a.bp, a.bp_x, a.bp_bn, a.bp_sums, a.bp_shards = 1, dt_.data_ptr(), bbn.src(with_tab), gsum.data_ptr(), bbn.sh
            a.bp_out, a.bp_dgamma, a.bp_dbeta = side.data_ptr(), dgam.data_ptr(), dbet.data_ptr()
            assert L.conv2d_check(C.byref(a)) == 0
        want = fam[ks] if dtype == "bf16" or fam[ks] == 1 else 0
        assert L.conv2d_family(C.byref(a)) == want, (L.conv2d_family(C.byref(a)), want)
        L.conv2d(C.byref(a), _stream())
        torch.cuda.synchronize()
        return y, es.sum(0), side, dgam, dbet

    r0, r1 = run(False), run(True)
    tol = 1e-5 if dtype == "fp32" else 4e-3
    for name, (y, es, side, dgam, dbet) in (("sums", r0), ("table", r1)):
        e_y, e_1, e_2 = rel(y.double(), ref), rel(es[0], ref_s1), rel(es[1], ref_s2)
        print("%-5s y %.3g  epi sums %.3g %.3g" % (name, e_y, e_1, e_2))
        assert e_y < tol, (name, e_y)
        assert e_1 < 10 * tol and e_2 < 10 * tol, (name, e_1, e_2)      # (test_conv_vs_float64's allowance)
        if bp:
            e_s = rel(side.double(), dldt)
            print("      side %.3g" % e_s)
            assert e_s < tol, (name, e_s)
            assert rel(dbet.double(), gsum[:, 0].sum(0)) < 1e-6 and rel(dgam.double(), gsum[:, 1].sum(0)) < 1e-6
    print("elements differing between the two paths: y %d / %d" % _differ(r0[0], r1[0]) +
          (", side %d / %d" % _differ(r0[2], r1[2]) if bp else ""))


APPLY = [(s, dt) for s in SHAPES for dt in ("fp32", "bf16")]


@pytest.mark.parametrize("case", APPLY, ids=["%s_%s" % c for c in APPLY])
def test_consumer_apply(case):
    from realnvp_hip import _lib
    from realnvp_hip._lib import BNBwdArgs
    shape, dtype = case
    B, H, W, Cc, _ = SHAPES[shape]
    M = B * H * W
    L = _lib.lib()
    dt, tdt = (0, torch.float32) if dtype == "fp32" else (1, torch.bfloat16)
    gen = torch.Generator(device=DEV).manual_seed(5)
    g = _rnd(torch.randn(M, Cc, generator=gen, device=DEV), dtype)
    t = _rnd(torch.randn(M, Cc, generator=gen, device=DEV) * 1.5 + 0.3, dtype)
    res = _rnd(torch.randn(M, Cc, generator=gen, device=DEV), dtype)
    old = _rnd(torch.randn(M, Cc, generator=gen, device=DEV), dtype)
    bn = _BN(t, gen)
    xh = bn.xhat(t)
    gsum = torch.zeros(bn.sh, 2, Cc, dtype=torch.float64, device=DEV)
    for h, (pg, px) in enumerate(zip(torch.chunk(g, bn.sh, 0), torch.chunk(xh, bn.sh, 0))):
        gsum[h, 0], gsum[h, 1] = pg.sum(0), (pg * px).sum(0)
    k1, k2 = gsum[:, 0].sum(0) / M, gsum[:, 1].sum(0) / M
    ref = bn.gam.double() * bn.rstd * (g - k1 - xh * k2) + res + old
    dg, dt_, dres = g.to(tdt), t.to(tdt), res.to(tdt)

    def run(with_tab):
        dx = old.to(tdt).clone()
        dgam, dbet = torch.zeros(Cc, device=DEV), torch.zeros(Cc, device=DEV)
        b = BNBwdArgs()
        b.dtype, b.M, b.C, b.cs = dt, M, Cc, Cc
        b.g, b.x, b.bn, b.sums, b.sum_shards = dg.data_ptr(), dt_.data_ptr(), bn.src(with_tab), gsum.data_ptr(), bn.sh
        b.dx, b.residual, b.accumulate = dx.data_ptr(), dres.data_ptr(), 1
        b.dgamma, b.dbeta = dgam.data_ptr(), dbet.data_ptr()
        L.bn_bwd_apply(C.byref(b), _stream())
        torch.cuda.synchronize()
        return dx, dgam, dbet

    r0, r1 = run(False), run(True)
    tol = 1e-5 if dtype == "fp32" else 4e-3
    for name, (dx, dgam, dbet) in (("sums", r0), ("table", r1)):
        e = rel(dx.double(), ref)
        print("%-5s dx %.3g" % (name, e))
        assert e < tol, (name, e)
        assert rel(dbet.double(), gsum[:, 0].sum(0)) < 1e-6 and rel(dgam.double(), gsum[:, 1].sum(0)) < 1e-6
    print("elements differing between the two paths: %d / %d" % _differ(r0[0], r1[0]))


# shape, ks, the tap-shared bf16 kernel's class
WGRAD = [("deep_m1024", 3, 0), ("deep_m1024", 1, 1), ("wide_64x64_c32", 3, 2), ("wide_32x32_c64", 1, 3),
         ("wide_64x64_c32", 1, 3)]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", WGRAD, ids=["%s_k%d_cls%d" % c for c in WGRAD])
def test_consumer_wgrad(case, dtype):
    from realnvp_hip import _lib
    from realnvp_hip._lib import WgradGroup
    shape, ks, cls = case
    B, H, W, Cc, _ = SHAPES[shape]
    M = B * H * W
    L = _lib.lib()
    dt, tdt = (0, torch.float32) if dtype == "fp32" else (1, torch.bfloat16)
    gen = torch.Generator(device=DEV).manual_seed(7)
    x = _rnd(torch.randn(M, Cc, generator=gen, device=DEV) * 1.5 + 0.3, dtype)
    dy = _rnd(torch.randn(M, Cc, generator=gen, device=DEV), dtype)
    bn = _BN(x, gen)
    act = _rnd(torch.relu(x * bn.scale + bn.shift), dtype)
    kp = (ks * ks * Cc + 63) // 64 * 64
    # dW[co][tap][ci] = sum_m dy[m][co] act[m + tap][ci]: the conv reference with the roles exchanged
    a4 = act.view(B, H, W, Cc)
    ref = torch.zeros(Cc, kp, dtype=torch.float64, device=DEV)
    for ky in range(ks):
        for kx in range(ks):
            dy_, dx_ = ky - ks // 2, kx - ks // 2
            sh = torch.zeros_like(a4)
            ys, ye = max(0, -dy_), min(H, H - dy_)
            xs, xe = max(0, -dx_), min(W, W - dx_)
            sh[:, ys:ye, xs:xe] = a4[:, ys + dy_:ye + dy_, xs + dx_:xe + dx_]
            base = (ky * ks + kx) * Cc
            ref[:, base:base + Cc] = dy.T @ sh.reshape(M, Cc)
    dx_, ddy = x.to(tdt), dy.to(tdt)
    nz = int(L.wgrad_slabs(M))
    nrep = int(L.wgrad_replicas(nz))

    def run(with_tab):
        ws = torch.zeros(nrep, Cc, kp, device=DEV)
        wsb = torch.zeros(nrep, Cc, device=DEV)
        grp = WgradGroup()
        grp.dtype, grp.B, grp.H, grp.W, grp.n_conv = dt, B, H, W, 1
        c = grp.conv[0]
        c.x, c.cs_in, c.cin, c.ks = dx_.data_ptr(), Cc, Cc, ks
        c.pro_bn_relu, c.pro = 1, bn.src(with_tab)
        c.dy, c.cs_dy, c.n = ddy.data_ptr(), Cc, Cc
        c.ws, c.wsb, c.kp, c.nz, c.nrep = ws.data_ptr(), wsb.data_ptr(), kp, nz, nrep
        assert L.wgrad_class(C.byref(grp), 0) == (cls if dtype == "bf16" else -2)
        L.conv2d_wgrad_grouped(C.byref(grp), _stream())
        torch.cuda.synchronize()
        return ws.sum(0), wsb.sum(0)

    r0, r1 = run(False), run(True)
    tol = 1e-5 if dtype == "fp32" else 1e-4          # (test_grouped_wgrad_vs_torch's)
    for name, (dw, db) in (("sums", r0), ("table", r1)):
        e, eb = rel(dw.double(), ref), rel(db.double(), dy.sum(0))
        print("%-5s dW %.3g  dbias %.3g" % (name, e, eb))
        assert e < tol and eb < tol, (name, e, eb)
    print("elements differing between the two paths: %d / %d" % _differ(r0[0], r1[0]))


# ---------------------------------------------------------------------------
# (c) one captured trainer step, tables on and off
# ---------------------------------------------------------------------------
def _trainer_state(on):
    import flow_realnvp
    import utils
    from formula_init import formula_state, pixels
    from realnvp_hip import engine
    from realnvp_hip.trainer import FlowTrainer
    old = engine.BN_TABLES
    engine.BN_TABLES = on
    try:
        prior = torch.distributions.Normal(torch.tensor(0.0, device=DEV), torch.tensor(1.0, device=DEV))
        m = flow_realnvp.RealNVP(3, 32, prior, utils.Hyperparameters(8, 1, True, True, True, True))
        m.load_state_dict(formula_state(m))
        tr = FlowTrainer(m.to(DEV), 32, dtype="bf16", seed=5)
        tr.set_pixels(pixels(32, 3, 32, seed=5).to(DEV))
        tr.capture(warmup=1)                 # (restores the state it started from)
        tr.step()
        torch.cuda.synchronize()
        svs = [st[5] for st in tr.stages if st[0] == "coupling"]
        assert svs and all("bwd_plan" in sv for sv in svs)
        tabs = [bool(s.tab) for sv in svs for kind, c, *_ in sv["bwd_plan"][1][0]
                for s in ((c.epi,) if kind == "dgrad" else (c.bn,)) if kind != "dgrad" or c.epi_relu_bn_bwd]
        st = dict(grad=tr.grad.double().clone(), param=tr.param.double().clone(), m=tr.exp_avg.double().clone(),
                  v=tr.exp_avg_sq.double().clone(), lp=tr.lp.double().clone())
        del tr
        torch.cuda.empty_cache()
        return st, tabs
    finally:
        engine.BN_TABLES = old


def test_trainer_step_tables_on_off():
    off1, t_off = _trainer_state(False)
    off2, _ = _trainer_state(False)
    on, t_on = _trainer_state(True)
    assert not any(t_off)
    assert all(t_on)
    for k in off1:
        floor = rel(off2[k], off1[k])
        d = rel(on[k], off1[k])
        same = int((on[k] == off1[k]).sum()), on[k].numel()
        print("%-6s tables vs sums %.3g (bitwise equal %d / %d), sums vs sums %.3g" % (k, d, same[0], same[1], floor))
        assert d <= max(2 * floor, 1e-6), (k, d, floor)
