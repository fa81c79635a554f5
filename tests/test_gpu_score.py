"""Scoring (include/realnvp_hip.h, "scoring"): rnvp_score_finish and
rnvp_score_in_fwd at the ABI level on raw tensors, then FlowScorer on the
16x16 / base dim 4 / 1 block model against the float64 oracle, the drop-in's
own forward, itself at other batch sizes, and the averaged weights."""
import math

import numpy as np
import pytest
import torch

from formula_init import formula_state, pixels, uniform_noise

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZE, BD, RB = 16, 4, 1
D = 3 * SIZE * SIZE
N = 10                      # images: batches of 4, 4, 2 at B = 4
RTOL = 1e-5                 # the project's log-prob tolerance
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def L():
    from realnvp_hip import _lib
    return _lib.lib()


def sptr():
    return torch.cuda.current_stream().cuda_stream


def make_model():
    """tests/test_data_pipeline.py::_model after one training-mode forward
    (running statistics off their defaults), in eval mode"""
    import flow_realnvp
    import utils
    prior = torch.distributions.Normal(torch.tensor(0.0, device=DEV), torch.tensor(1.0, device=DEV))
    m = flow_realnvp.RealNVP(3, SIZE, prior, utils.Hyperparameters(BD, RB, True, True, True, True))
    m.load_state_dict(formula_state(m))
    m = m.to(DEV).train()
    with torch.no_grad():
        m(torch.from_numpy(np.random.default_rng(7).random((8, 3, SIZE, SIZE), dtype=np.float32)).to(DEV) * 2 - 1)
    return m.eval()


@pytest.fixture(scope="module")
def model():
    return make_model()


@pytest.fixture(scope="module")
def images():
    return pixels(N, 3, SIZE, seed=41)


@pytest.fixture(scope="module")
def noises():
    return torch.stack([uniform_noise(N, 3, SIZE, seed=50 + k) for k in range(3)])     # [3, N, C, S, S]


@pytest.fixture(scope="module")
def oracle_ll(model, images, noises):
    """[3, N] float64: the oracle's log-likelihood of every image under each
    of the three noise draws, with the model's own state in float64"""
    import realnvp_oracle as O
    spec = O.FlowSpec(3, SIZE, O.HP(BD, RB))
    S64 = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu())
           for k, v in model.state_dict().items()}
    out = []
    with torch.no_grad():
        for k in range(3):
            x, ld = O.logit_transform(images.double(), noises[k].double())
            out.append((O.log_prob(S64, spec, x, training=False) + ld).numpy())
    return np.stack(out)


def batches_of(t, B):
    return [t[i:i + B].to(DEV) for i in range(0, t.shape[0], B)]


def lse_bound(ll):
    """float64 log(1/K sum_k exp(ll[k])) along axis 0"""
    m = ll.max(axis=0)
    return m + np.log(np.exp(ll - m).sum(axis=0)) - math.log(ll.shape[0])


def make_ctl(scores, cap, first, n_valid, n_draws, draw=0):
    from realnvp_hip._lib import ScoreCtl
    c = ScoreCtl(scores.data_ptr() if scores is not None else None, cap, first, 0, 0.0, n_valid, n_draws, draw, 0)
    return torch.frombuffer(bytearray(bytes(c)), dtype=torch.uint8).to(DEV)


def read_ctl(t):
    from realnvp_hip._lib import ScoreCtl
    return ScoreCtl.from_buffer_copy(bytes(t.cpu().numpy()))


def assert_rel(got, want, rtol, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want) / np.abs(want)
    print("%s max rel err %.3g (bound %.1g)" % (what, float(err.max()), rtol))
    assert float(err.max()) <= rtol, (what, got, want)


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("cap", [8, 6])
@pytest.mark.parametrize("n", [105, 4099])
def test_finish_kernel(n, cap):
    """rnvp_score_finish alone: three draws of a 3-row batch with 2 valid
    rows at global index 5, into a destination of 8 floats of which `cap`
    may be written."""
    B, K, nv, first = 3, 3, 2, 5
    gen = torch.Generator().manual_seed(n)
    z = torch.randn(B, n, generator=gen)
    # [draw][row]: the draws' log-likelihoods differ by about 5 nats per row; row 0 has its largest in
    # draw 1, row 1 in draw 2, so the running maximum is both replaced and kept
    ldj = torch.tensor([[0.0, -4.5, -5.5], [5.0, 0.5, 0.25], [-5.0, 5.25, 4.75]])
    ldj = ldj + 0.1 * torch.randn(K, B, generator=gen)
    logdet = 100.0 + torch.rand(K, B, generator=gen)
    prior = (-0.5 * z.double() ** 2 - HALF_LOG_2PI).sum(dim=1)
    ll = (prior[None] + ldj.double() + logdet.double()).numpy()           # [K, B]
    want = lse_bound(ll)
    nan = float("nan")
    scores = torch.full((8,), nan, device=DEV)
    ctl = make_ctl(scores, cap, first, nv, K)
    zd = z.to(DEV)
    dl, dd = torch.empty(B, device=DEV), torch.empty(B, device=DEV)
    run = torch.full((B, 2), nan, device=DEV)
    for k in range(K):
        dl.copy_(ldj[k])
        dd.copy_(logdet[k])
        lp = torch.full((B,), nan, device=DEV)
        L().score_finish(zd.data_ptr(), dl.data_ptr(), dd.data_ptr(), run.data_ptr(), lp.data_ptr(), ctl.data_ptr(),
                         B, n, sptr())           # (raises on any status but 0)
        torch.cuda.synchronize()
        assert_rel(lp[:nv].cpu().numpy(), ll[k, :nv], 1e-6, "draw %d lp" % k)
        assert math.isnan(float(lp[2]))
        assert float(dl.abs().max()) == 0.0 and float(dd.abs().max()) == 0.0
        c = read_ctl(ctl)
        assert c.draw == (k + 1) % K and c.n_scored == (2 if k == K - 1 else 0) and c.first == (7 if k == K - 1 else 5)
        if k < K - 1:
            assert bool(torch.isnan(scores).all()) and c.ll_sum == 0.0 and c.overflow == 0
    s = scores.cpu().numpy()
    c = read_ctl(ctl)
    stored = 2 if cap >= 7 else 1
    assert_rel(s[5:5 + stored], want[:stored], 1e-6, "scores")
    assert np.isnan(s[:5]).all() and np.isnan(s[5 + stored:]).all()
    assert bool(torch.isnan(run[2]).all())          # a padding row keeps no running state either
    assert (c.n_scored, c.first, c.draw, c.overflow) == (2, 7, 0, int(cap < 7))
    assert (c.cap, c.n_valid, c.n_draws, c.scores) == (cap, nv, K, scores.data_ptr())
    # the finalised scores, added in row order in fp64 (row 1's from the kernel's own staging when it was not stored)
    row1 = np.float64(s[6]) if stored == 2 else np.float64(run[1, 0].item())
    assert c.ll_sum == float((np.float64(0.0) + np.float64(s[5])) + row1)
    if stored == 1:
        assert_rel(row1, want[1], 1e-6, "row 1 (not stored)")


@pytest.mark.parametrize("shape", [(3, 16, 16), (3, 17, 23)], ids=["16x16", "17x23"])
def test_noise_follows_the_image(shape):
    """rnvp_score_in_fwd row b in draw 1 of 2 at global index 3 + b is
    rnvp_logit_fwd of that one image at counter offset ((3 + b) 2 + 1) n; an
    explicit noise replaces the draw; the block is not written."""
    B, K, first, draw, seed = 4, 2, 3, 1, 1234
    n = shape[0] * shape[1] * shape[2]
    gen = torch.Generator().manual_seed(9)
    pix = torch.randint(0, 256, (B,) + shape, generator=gen).float().div(255).to(DEV)
    ctl = make_ctl(None, 0, first, B, K, draw)
    before = bytes(ctl.cpu().numpy())
    y, ld = torch.empty_like(pix), torch.zeros(B, device=DEV)
    L().score_in_fwd(pix.data_ptr(), None, seed, ctl.data_ptr(), 0.9, y.data_ptr(), ld.data_ptr(), B, *shape, sptr())
    y1, ld1 = torch.empty_like(pix[:1]), torch.empty(1, device=DEV)
    wrong = torch.empty_like(y1)
    for b in range(B):
        L().logit_fwd(pix[b:b + 1].data_ptr(), None, seed, ((first + b) * K + draw) * n, None, 0.9, y1.data_ptr(),
                      ld1.data_ptr(), 1, n, sptr())
        assert float((y[b] - y1[0]).abs().max()) <= 1e-5, b
        assert_rel(ld[b].item(), ld1.item(), 1e-6, "row %d logdet" % b)
        # the slot's counter (what rnvp_logit_fwd on the batch would use) is another stream altogether
        L().logit_fwd(pix[b:b + 1].data_ptr(), None, seed, b * n, None, 0.9, wrong.data_ptr(), ld1.data_ptr(), 1, n,
                      sptr())
        assert float((y[b] - wrong[0]).abs().max()) > 1e-2
    # logdet[b] +=: a second call doubles it
    first_ld = ld.clone()
    L().score_in_fwd(pix.data_ptr(), None, seed, ctl.data_ptr(), 0.9, y.data_ptr(), ld.data_ptr(), B, *shape, sptr())
    assert_rel(ld.cpu().numpy(), 2 * first_ld.cpu().numpy(), 1e-6, "accumulated logdet")
    # explicit noise
    noise = torch.rand((B,) + shape, generator=gen).to(DEV)
    yn, ldn = torch.empty_like(pix), torch.zeros(B, device=DEV)
    L().score_in_fwd(pix.data_ptr(), noise.data_ptr(), seed, ctl.data_ptr(), 0.9, yn.data_ptr(), ldn.data_ptr(), B,
                     *shape, sptr())
    yr, ldr = torch.empty_like(pix), torch.empty(B, device=DEV)
    L().logit_fwd(pix.data_ptr(), noise.data_ptr(), seed, 0, None, 0.9, yr.data_ptr(), ldr.data_ptr(), B, n, sptr())
    assert float((yn - yr).abs().max()) <= 1e-5
    assert_rel(ldn.cpu().numpy(), ldr.cpu().numpy(), 1e-6, "logdet with explicit noise")
    assert bytes(ctl.cpu().numpy()) == before


# ------------------------------------------------------------------- scorer
def scorer(model, B, **kw):
    from realnvp_hip import FlowScorer
    kw.setdefault("dtype", "fp32")
    return FlowScorer(model, B, **kw)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("K", [1, 3])
def test_scores_match_the_oracle(model, images, noises, oracle_ll, K, graph):
    """Batches of 4, 4, 2 with explicit noise (which takes the eager launches
    whatever `graph` says) against the float64 oracle: per-image scores, the
    reference loop's mean of batch means, the per-image mean, bits/dim."""
    import realnvp_oracle as O
    B = 4
    sc = scorer(model, B, n_draws=K, graph=graph)
    sc.begin(N)
    for i in range(0, N, B):
        sc.add_batch(images[i:i + B].to(DEV), noise=noises[:K, i:i + B].to(DEV))
    got = sc.scores()
    assert got.dtype == torch.float32 and tuple(got.shape) == (N,) and got.is_cuda
    want = lse_bound(oracle_ll[:K])
    if K == 1:
        assert np.array_equal(want, oracle_ll[0])
    assert_rel(got.cpu().numpy(), want, RTOL, "K=%d scores" % K)
    ref_loop = float(np.mean([want[i:i + B].mean() for i in range(0, N, B)]))     # train.py:214-233
    assert abs(sc.mean_logll(batch_mean=True) - ref_loop) <= RTOL * abs(ref_loop)
    assert abs(sc.mean_logll() - want.mean()) <= RTOL * abs(want.mean())
    seq = 0.0
    for v in got.cpu().tolist():        # ll_sum: one fp64 addition per image, in order
        seq += v
    assert sc.mean_logll() == seq / N
    assert abs(sc.bits_per_dim() - O.bits_per_dim(want.mean(), SIZE, 3)) <= 1e-5
    per = sc.bits_per_dim(per_image=True)
    assert_rel(per.cpu().numpy(), [O.bits_per_dim(v, SIZE, 3) for v in want], 1e-5, "bits/dim per image")
    assert sc.graph is None


def test_bf16_matches_the_dropin_forward(images, noises):
    """bf16: the same kernels as the drop-in's eval forward on the same
    (zero-padded) batches and noise, so only the tail differs."""
    B = 4
    m = make_model().set_precision("bf16")
    sc = scorer(m, B, dtype="bf16")
    sc.begin(N)
    ref = []
    with torch.no_grad():
        for i in range(0, N, B):
            pix, noise = images[i:i + B].to(DEV), noises[0, i:i + B].to(DEV)
            rows = pix.shape[0]
            sc.add_batch(pix, noise=noise[None])
            pad, npad = torch.zeros(B, 3, SIZE, SIZE, device=DEV), torch.zeros(B, 3, SIZE, SIZE, device=DEV)
            pad[:rows], npad[:rows] = pix, noise
            x, ld = torch.empty_like(pad), torch.empty(B, device=DEV)
            L().logit_fwd(pad.data_ptr(), npad.data_ptr(), 0, 0, None, 0.9, x.data_ptr(), ld.data_ptr(), B, D, sptr())
            lp, _ = m(x)
            ref.append((lp + ld)[:rows].double().cpu())
    assert_rel(sc.scores().cpu().numpy(), torch.cat(ref).numpy(), RTOL, "bf16 scores")


def test_scores_do_not_depend_on_the_batch_size(model, images):
    """Philox noise keyed by the image's global index: B = 4, 5 and 10 give
    the same scores; the images in reversed order do not."""
    got = {B: scorer(model, B, seed=77).score(batches_of(images, B)).cpu().numpy() for B in (4, 5, 10)}
    assert_rel(got[5], got[4], RTOL, "B=5 against B=4")
    assert_rel(got[10], got[4], RTOL, "B=10 against B=4")
    rev = scorer(model, 4, seed=77).score(batches_of(images.flip(0), 4)).cpu().numpy()[::-1]
    assert not np.allclose(rev, got[4], rtol=RTOL, atol=0.0)
    other = scorer(model, 4, seed=78).score(batches_of(images, 4)).cpu().numpy()
    assert not np.allclose(other, got[4], rtol=RTOL, atol=0.0)


def test_ragged_padding_is_inert(model, images):
    """The final batch of 2 rows scores the same whatever the other two rows
    of the pixel buffer held (zeros, a stale batch, or real images scored as
    part of a full batch), and exactly N scores are written."""
    B, cap = 4, 13
    nan = float("nan")

    def run(prepare, last):
        sc = scorer(model, B, seed=5)
        sc.begin(cap)
        sc._scores.fill_(nan)
        for b in batches_of(images[:8], B):
            sc.add_batch(b)
        prepare(sc)
        sc.add_batch(last)
        return sc
    tail = images[8:10].to(DEV)
    a = run(lambda sc: None, tail)                                       # the buffer holds batch 2
    b = run(lambda sc: sc.pix.zero_(), tail)
    c = run(lambda sc: sc.pix.fill_(0.75), tail)
    full = run(lambda sc: None, torch.cat([tail, images[:2].to(DEV)]))   # other images in rows 2 and 3
    sa = a.scores().cpu().numpy()
    assert sa.shape == (N,) and np.isfinite(sa).all()
    assert np.isnan(a._scores[N:].cpu().numpy()).all() and a._scores.numel() == cap
    assert float(a.pix[2:].abs().max()) == 0.0
    assert_rel(b.scores().cpu().numpy(), sa, RTOL, "zeros before")
    assert_rel(c.scores().cpu().numpy(), sa, RTOL, "garbage before")
    assert_rel(full.scores().cpu().numpy()[:N], sa, RTOL, "inside a full batch")
    assert full.scores().numel() == N + 2
    # argument checks of add_batch, and a pass that would overflow
    sc = scorer(model, B)
    with pytest.raises(RuntimeError, match="begin"):
        sc.add_batch(tail)
    sc.begin(5)
    for bad in (images[:0], images[:5], images[:2, :, :8], images[0]):
        with pytest.raises(ValueError):
            sc.add_batch(bad.to(DEV))
    sc.add_batch(images[:4].to(DEV))
    with pytest.raises(RuntimeError, match="room"):
        sc.add_batch(tail)
    assert sc.scores().numel() == 4


def test_graph_is_kept_and_follows_moved_weights(images):
    """One captured draw serves every pass: same seed, same scores, the same
    graph object at another capacity.  After a FlowTrainer step has moved the
    parameters into its arena the next pass re-captures and matches the eager
    launches on the current weights."""
    from realnvp_hip.trainer import FlowTrainer
    m = make_model()
    batches = batches_of(images, 4)
    sc = scorer(m, 4, seed=3, n_draws=2)
    s1 = sc.score(batches).clone()
    g = sc.graph
    assert g is not None
    s2 = sc.score(batches, capacity=16).clone()
    assert sc.graph is g and s2.numel() == N
    assert_rel(s2.cpu().numpy(), s1.cpu().numpy(), RTOL, "second pass")
    eager = scorer(m, 4, seed=3, n_draws=2, graph=False)
    assert_rel(eager.score(batches).cpu().numpy(), s1.cpu().numpy(), RTOL, "eager against graph")
    assert eager.graph is None
    m.train()
    tr = FlowTrainer(m, 4, dtype="fp32")
    tr.set_pixels(pixels(4, 3, SIZE, seed=2).to(DEV))
    tr.step()
    m.eval()
    s3 = sc.score(batches).clone()
    assert sc.graph is not g
    assert_rel(s3.cpu().numpy(), eager.score(batches).cpu().numpy(), RTOL, "after the step")
    assert not np.allclose(s3.cpu().numpy(), s1.cpu().numpy(), rtol=RTOL, atol=0.0)


def test_scores_of_the_averaged_weights(images):
    """Inside ema_weights() the scores are those of a second model loaded
    from ema_state_dict()."""
    from realnvp_hip.trainer import FlowTrainer
    m = make_model().train()
    tr = FlowTrainer(m, 4, dtype="fp32", ema_decay=0.5)
    for s in range(2):
        tr.set_pixels(pixels(4, 3, SIZE, seed=20 + s).to(DEV))
        tr.step()
    m.eval()
    batches = batches_of(images, 4)
    sc = scorer(m, 4, seed=9)
    raw = sc.score(batches).clone()
    with tr.ema_weights():
        inside = sc.score(batches).clone()
    second = make_model()
    second.load_state_dict(tr.ema_state_dict())
    want = scorer(second.eval(), 4, seed=9).score(batches)
    assert_rel(inside.cpu().numpy(), want.cpu().numpy(), RTOL, "average in place against a second model")
    assert not np.allclose(raw.cpu().numpy(), inside.cpu().numpy(), rtol=RTOL, atol=0.0)
    assert_rel(sc.score(batches).cpu().numpy(), raw.cpu().numpy(), RTOL, "after the block")
