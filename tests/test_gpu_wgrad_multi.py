"""The model-wide weight-gradient launch (rnvp_conv2d_wgrad_multi,
engine.WGRAD_MULTI) on the MI355X.

(a) Through the C ABI: ONE multi launch per tile class over three groups of
    different shapes (B = 2: 4x4 -- one stage spans several images; 8x8;
    16x16 with nz = 4 -- a slab is one 128-pixel stage and ends mid-image, the
    halo case) holding 3x3 128->128, 3x3 with cin = 97 (channel stride 104, a
    partial second ci tile), 1x1 128->128, 1x1 160->96 (partial class-1
    tiles), convs with bias and convs with a BN+ReLU prologue.  Every ws / wsb
    float is bitwise what per-group rnvp_conv2d_wgrad_grouped launches write
    from the same inputs, each dW / bias gradient is within
    test_grouped_wgrad_vs_torch's bound (tests/test_gpu_deep.py: 1e-4 relative
    L2 for bf16) of torch's float64 weight gradient, and untouched padding
    (k >= ks^2 cs_in, the guard rows behind every buffer) stays zero.

(b) One captured step of a 32x32, R2, base-dim-8 bf16 trainer at B = 2,
    replayed three times, with WGRAD_MULTI on and off: gradients, parameters, both moments, log-prob and
    the packed weight images agree at the bound of the on/off step test in
    tests/test_gpu_bn_table.py (twice the off-vs-off difference, 1e-6 at
    least); the instrumented step's conv_wgrad launches drop from one per
    coupling to one per tile class (plus the couplings the planner declines:
    this model's 2x2 scale takes the generic kernel); a trainer with
    max_grad_norm issues exactly the launches it did before."""
import ctypes as C

import numpy as np
import pytest
import torch

from wgrad_multi_common import expected_convs, make_group, plan

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 256     # floats behind every ws / wsb buffer that must stay zero


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


# (B, H, W, nz or None, [(ks, cin, cout, bias, pro)])
GROUPS = [
    (2, 4, 4, None, [(3, 128, 128, False, False), (1, 160, 96, True, False), (3, 97, 128, False, True)]),
    (2, 8, 8, None, [(3, 97, 128, False, False), (1, 128, 128, True, False), (1, 160, 96, False, True)]),
    (2, 16, 16, 4, [(3, 128, 128, True, True), (3, 97, 128, False, False), (1, 128, 128, False, False),
                    (1, 160, 96, True, False)]),
]


def _build():
    from realnvp_hip import _lib
    from realnvp_hip.engine import stat_shards
    from realnvp_hip.net import chan_stride, round_up
    L = _lib.lib()
    gen = torch.Generator(device=DEV).manual_seed(11)
    groups, bufs, refs = [], [], []
    for B, H, W, nz, convs in GROUPS:
        M = B * H * W
        nzv = int(L.wgrad_slabs(M)) if nz is None else nz
        t = []
        for ks, cin, cout, bias, pro in convs:
            csi, cso = chan_stride(cin), chan_stride(cout)
            kp = round_up(ks * ks * csi, 64)
            d = {}
            d["x"] = torch.zeros(M, csi, device=DEV, dtype=torch.bfloat16)
            d["x"][:, :cin] = torch.randn(M, cin, device=DEV, generator=gen).to(torch.bfloat16)
            d["dy"] = torch.zeros(M, cso, device=DEV, dtype=torch.bfloat16)
            d["dy"][:, :cout] = torch.randn(M, cout, device=DEV, generator=gen).to(torch.bfloat16)
            d["ws"] = torch.zeros(nzv * cout * kp + GUARD, device=DEV)
            d["wsb"] = torch.zeros(nzv * cout + GUARD, device=DEV)
            act = d["x"][:, :cin].double()
            if pro:
                xf = act
                sh = stat_shards(M)
                d["sums"] = torch.zeros(sh, 2, cin, dtype=torch.float64, device=DEV)
                d["sums"][0, 0], d["sums"][0, 1] = xf.sum(0), (xf * xf).sum(0)
                d["gamma"] = torch.rand(cin, device=DEV, generator=gen) + 0.5
                d["beta"] = torch.randn(cin, device=DEV, generator=gen) * 0.3
                mean = d["sums"][0, 0] / M
                var = (d["sums"][0, 1] / M - mean * mean).clamp_min(0)
                rstd = (1.0 / torch.sqrt(var + 1e-5)).float().double()
                scale = (d["gamma"].double() * rstd).float().double()
                shift = (d["beta"].double() - mean.float().double() * d["gamma"].double() * rstd).float().double()
                act = torch.relu(xf * scale + shift).to(torch.bfloat16).double()
            a4 = act.reshape(B, H, W, cin).permute(0, 3, 1, 2)
            d4 = d["dy"][:, :cout].double().reshape(B, H, W, cout).permute(0, 3, 1, 2)
            ref = torch.nn.grad.conv2d_weight(a4, (cout, cin, ks, ks), d4, padding=ks // 2)
            refp = torch.zeros(cout, kp, dtype=torch.float64, device=DEV)
            for ky in range(ks):
                for kx in range(ks):
                    base = (ky * ks + kx) * csi
                    refp[:, base:base + cin] = ref[:, :, ky, kx]
            refs.append((refp.cpu(), d4.sum((0, 2, 3)).cpu(), nzv, cout, kp, ks * ks * csi, bias))
            t.append(d)
        groups.append(make_group(B, H, W, convs, lambda i, f, t=t: t[i][f].data_ptr(), nz=nzv, nrep=nzv))
        bufs += t
    return groups, bufs, refs


def _snapshot(bufs):
    return [(d["ws"].clone(), d["wsb"].clone()) for d in bufs]


@pytest.fixture(scope="module")
def multi_case():
    """(per-group results, multi results, references, classes launched): computed once"""
    from realnvp_hip import _lib
    from realnvp_hip.engine import plan_wgrad_multi
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    groups, bufs, refs = _build()
    for g in groups:
        L.conv2d_wgrad_grouped(C.byref(g), s)
    torch.cuda.synchronize()
    single = _snapshot(bufs)
    for d in bufs:
        d["ws"].zero_()
        d["wsb"].zero_()
    launches = plan_wgrad_multi(groups, DEV)
    assert launches is not None
    torch.cuda.synchronize()
    for m, _ in launches:
        L.conv2d_wgrad_multi(C.byref(m), s)
    torch.cuda.synchronize()
    multi = _snapshot(bufs)
    classes = sorted(m.cls for m, _ in launches)
    present = [cls for cls in range(4) if expected_convs(groups, cls)]
    # the planned launches cover every conv of the three groups
    assert classes == present and sum(m.n_conv for m, _ in launches) == len(bufs)
    assert sorted(present) == [0, 1]
    return single, multi, refs


def test_multi_bitwise_equals_per_group_launches(multi_case):
    single, multi, refs = multi_case
    for i, ((ws0, wb0), (ws1, wb1)) in enumerate(zip(single, multi)):
        assert ws0.abs().sum() > 0
        assert torch.equal(ws0, ws1), (i, int((ws0 != ws1).sum()))
        assert torch.equal(wb0, wb1), (i, int((wb0 != wb1).sum()))


def test_multi_vs_torch_float64(multi_case):
    _, multi, refs = multi_case
    for i, ((ws, wsb), (refp, refb, nz, cout, kp, kreal, bias)) in enumerate(zip(multi, refs)):
        got = ws[:nz * cout * kp].reshape(nz, cout, kp).sum(0).double().cpu()
        e = rel(got, refp)
        print("conv %d: dW rel %.3g" % (i, e))
        assert e < 1e-4, (i, e)
        if bias:
            eb = rel(wsb[:nz * cout].reshape(nz, cout).sum(0).double().cpu(), refb)
            print("conv %d: bias rel %.3g" % (i, eb))
            assert eb < 1e-4, (i, eb)


def test_multi_padding_stays_zero(multi_case):
    _, multi, refs = multi_case
    for i, ((ws, wsb), (refp, refb, nz, cout, kp, kreal, bias)) in enumerate(zip(multi, refs)):
        w = ws[:nz * cout * kp].reshape(nz, cout, kp)
        assert not w[:, :, kreal:].any(), i
        assert not ws[nz * cout * kp:].any(), i
        assert not wsb[nz * cout:].any(), i
        if not bias:
            assert not wsb.any(), i


# ---------------------------------------------------------------------------
# (b) the trainer
# ---------------------------------------------------------------------------
def _trainer(on, **kw):
    import flow_realnvp
    import utils
    from formula_init import formula_state, pixels
    from realnvp_hip import engine
    from realnvp_hip.trainer import FlowTrainer
    old = engine.WGRAD_MULTI
    engine.WGRAD_MULTI = on
    try:
        prior = torch.distributions.Normal(torch.tensor(0.0, device=DEV), torch.tensor(1.0, device=DEV))
        m = flow_realnvp.RealNVP(3, 32, prior, utils.Hyperparameters(8, 2, True, True, True, True))
        m.load_state_dict(formula_state(m))
        tr = FlowTrainer(m.to(DEV), 2, dtype="bf16", seed=5, **kw)
        tr.set_pixels(pixels(2, 3, 32, seed=5).to(DEV))
        tr.capture(warmup=1)                 # (restores the state it started from)
        for _ in range(3):                   # (the replays also carry the state the step leaves behind)
            tr.step()
        torch.cuda.synchronize()
        # the packed weight images (bf16: forward / data-gradient / fragment-major) and the fp32 norms
        images = []
        for st in tr.stages:
            if st[0] != "coupling":
                continue
            ar = st[2].weights("bf16")["arena"]
            for name, (off, nbytes) in ar.slots.items():
                dt = torch.float32 if name.startswith("norm:") else torch.bfloat16
                images.append(ar.buf[off:off + nbytes].view(dt).double())
        images = torch.cat(images)
        state = dict(grad=tr.grad.double().clone(), param=tr.param.double().clone(), m=tr.exp_avg.double().clone(),
                     v=tr.exp_avg_sq.double().clone(), lp=tr.lp.double().clone(), images=images)
        # the launches of one instrumented (eager) step
        engine.PROFILE = []
        try:
            tr.step_eager()
            torch.cuda.synchronize()
            fams = [p[0] for p in engine.PROFILE]
        finally:
            engine.PROFILE = None
        groups = [g for st in tr.stages if st[0] == "coupling" for g in st[5]["bwd_plan"][1][1]]
        # groups the planner declines keep their own launch (the 2x2 scale's
        # 3x3 staging does not fit the tap-shared kernel's LDS); the others'
        # tile classes are the model-wide launches
        L = engine._lib.lib()
        own = [g for g in groups if plan([g], 0)[0] != 0]
        classes = {int(L.wgrad_class(C.byref(g), c)) for g in groups if plan([g], 0)[0] == 0
                   for c in range(g.n_conv)}
        planned = [v[0] for v in tr._wg_multi_plans.values()]
        del tr
        torch.cuda.empty_cache()
        return state, fams, (len(groups), len(own)), classes, planned
    finally:
        engine.WGRAD_MULTI = old


def test_trainer_step_multi_on_off():
    off1, f_off, n_groups, classes, p_off = _trainer(False)
    off2 = _trainer(False)[0]
    on, f_on, n_groups_on, classes_on, p_on = _trainer(True)
    for k in off1:
        floor = rel(off2[k].cpu(), off1[k].cpu())
        d = rel(on[k].cpu(), off1[k].cpu())
        same = int((on[k] == off1[k]).sum()), on[k].numel()
        print("%-6s multi vs per-coupling %.3g (bitwise equal %d / %d), off vs off %.3g" % (k, d, same[0], same[1],
                                                                                           floor))
        assert d <= max(2 * floor, 1e-6), (k, d, floor)
    assert p_off == [] and len(p_on) == 1 and p_on[0] is not None
    assert n_groups == n_groups_on and classes == classes_on and min(classes) >= 0
    n_groups, own = n_groups
    print("conv_wgrad launches: %d (one per coupling) -> %d: classes %s + %d declined couplings" % (
        f_off.count("conv_wgrad"), f_on.count("conv_wgrad"), sorted(classes), own))
    assert f_off.count("conv_wgrad") == n_groups and 2 * own < n_groups and len(classes) < n_groups - own
    assert len(p_on[0]) == len(classes)
    assert f_on.count("conv_wgrad") == len(classes) + own
    # nothing else moved
    assert [f for f in f_on if f != "conv_wgrad"] == [f for f in f_off if f != "conv_wgrad"]


def test_trainer_with_clipping_keeps_its_launches():
    _, f_off, n_groups, _, p_off = _trainer(False, max_grad_norm=1.0)
    _, f_on, _, _, p_on = _trainer(True, max_grad_norm=1.0)
    assert p_off == [] and p_on == []
    assert f_on == f_off
    assert f_on.count("conv_wgrad") == n_groups[0]
