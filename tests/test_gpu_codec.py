"""Latents (include/realnvp_hip.h, "latents"): rnvp_latent_draw, rnvp_latent_out
and rnvp_latent_mix at the ABI level on raw tensors against the float64
mirrors of realnvp_hip.codec, then FlowCodec on the 16x16 / base dim 4 /
1 block model of tests/test_gpu_score.py against the float64 oracle, the
sampler, the drop-in's own inverse, itself at other batch sizes, and the
averaged weights."""
import numpy as np
import pytest
import torch

from formula_init import formula_state, pixels, uniform_noise

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZE, BD, RB = 16, 4, 1
D = 3 * SIZE * SIZE
N = 10                      # images: batches of 4, 4, 2 at B = 4
FLOW_RTOL = 1e-4            # relative L2 of a flow pass against float64 (tests/test_gpu_sampler.py)
SAMPLER_ATOL = 1e-5         # max abs on images between two launch orders of the same kernels (same file)
NAN = float("nan")


def L():
    from realnvp_hip import _lib
    return _lib.lib()


def sptr():
    return torch.cuda.current_stream().cuda_stream


def make_model():
    """tests/test_gpu_score.py::make_model: the formula state after one
    training-mode forward (running statistics off their defaults), in eval mode"""
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
def noise():
    return uniform_noise(N, 3, SIZE, seed=50)


@pytest.fixture(scope="module")
def latents():
    return torch.randn(N, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(17))


@pytest.fixture(scope="module")
def oracle(model):
    """(state in float64, spec) of the model for realnvp_oracle"""
    import realnvp_oracle as O
    S64 = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu())
           for k, v in model.state_dict().items()}
    return S64, O.FlowSpec(3, SIZE, O.HP(BD, RB))


@pytest.fixture(scope="module")
def oracle_z(oracle, images, noise):
    """{"noise", "mid"}: float64 [N, C, S, S] latents of the images"""
    import realnvp_oracle as O
    S64, spec = oracle
    out = {}
    with torch.no_grad():
        for name, u in (("noise", noise.double()), ("mid", torch.full_like(images, 0.5).double())):
            x, _ = O.logit_transform(images.double(), u)
            out[name] = O.flow_f(S64, spec, x, training=False)[0].numpy()
    return out


@pytest.fixture(scope="module")
def oracle_x(oracle, latents):
    """float64 [N, C, S, S]: the oracle's images of the random latents"""
    import realnvp_oracle as O
    S64, spec = oracle
    with torch.no_grad():
        return O.logit_inverse(O.flow_g(S64, spec, latents.double(), training=False)).numpy()


def codec(model, B, **kw):
    from realnvp_hip import FlowCodec
    kw.setdefault("dtype", "fp32")
    return FlowCodec(model, B, **kw)


def make_ctl(dst, cap, first, n_valid, temperature=1.0):
    from realnvp_hip._lib import LatentCtl
    c = LatentCtl(dst.data_ptr() if dst is not None else None, cap, first, 0, temperature, n_valid, 0, 0)
    return torch.frombuffer(bytearray(bytes(c)), dtype=torch.uint8).to(DEV)


def read_ctl(t):
    from realnvp_hip._lib import LatentCtl
    return LatentCtl.from_buffer_copy(bytes(t.cpu().numpy()))


def rel_l2(got, want):
    """per row (axis 0) relative L2 error, float64"""
    got = np.asarray(got, dtype=np.float64).reshape(len(got), -1)
    want = np.asarray(want, dtype=np.float64).reshape(len(want), -1)
    return np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)


def assert_rel_l2(got, want, bound, what):
    err = rel_l2(got, want)
    print("%s: max relative L2 %.3g (bound %.1g)" % (what, float(err.max()), bound))
    assert float(err.max()) <= bound, (what, err)


def assert_abs(got, want, bound, what):
    err = float((got.double() - want.double()).abs().max())
    print("%s: max abs %.3g (bound %.1g)" % (what, err, bound))
    assert err <= bound, what


def torch_round_rule(v):
    """torchvision.utils.save_image (train.py:259)"""
    return v.mul(255).add(0.5).clamp(0, 255).to(torch.uint8)


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("n", [768, 1173])
def test_draw_matches_the_mirror(n):
    """B = 4 rows from global row 3, seed 1234, T = 0.7.  Bound 2e-5 T: |g| <=
    5.77, the fp32 rounding of 2 pi u2 and a few ulp of cosf / logf give about
    5.5e-6; four times that."""
    from realnvp_hip.codec import prior_reference
    B, first, seed, T = 4, 3, 1234, 0.7
    ctl = make_ctl(None, 0, first, B, T)
    before = bytes(ctl.cpu().numpy())
    z = torch.full((B, n), NAN, device=DEV)
    L().latent_draw(z.data_ptr(), seed, ctl.data_ptr(), B, n, sptr())
    want = prior_reference(seed, first, B, n, T)
    err = float(np.abs(z.cpu().numpy().astype(np.float64) - want).max())
    print("n=%d: max abs %.3g (bound %.3g)" % (n, err, 2e-5 * T))
    assert err <= 2e-5 * T
    # a row belongs to its global index: row b here is row 0 of a draw that starts at 3 + b, bit for bit
    one = torch.empty(1, n, device=DEV)
    for b in range(B):
        c1 = make_ctl(None, 0, first + b, 1, T)
        L().latent_draw(one.data_ptr(), seed, c1.data_ptr(), 1, n, sptr())
        assert torch.equal(one[0], z[b]), b
    assert bytes(ctl.cpu().numpy()) == before


def test_draw_moments():
    """65,536 device values of seed 5: the two five-standard-error bounds of
    tests/test_codec_cpu.py"""
    B, n = 64, 1024
    ctl = make_ctl(None, 0, 0, B, 1.0)
    z = torch.empty(B, n, device=DEV)
    L().latent_draw(z.data_ptr(), 5, ctl.data_ptr(), B, n, sptr())
    g = z.cpu().numpy().astype(np.float64)
    mean, var = float(g.mean()), float(g.var())
    print("mean %.4f var %.4f max |g| %.2f" % (mean, var, float(np.abs(g).max())))
    assert abs(mean) <= 5.0 / np.sqrt(B * n) and abs(var - 1.0) <= 5.0 * np.sqrt(2.0 / (B * n))


@pytest.mark.parametrize("cap", [8, 6])
@pytest.mark.parametrize("n", [105, 4099])
def test_out_kernel(n, cap):
    """rnvp_latent_out alone: a 3-row batch with 2 valid rows at global index
    5 into a destination of 8 rows of which `cap` may be written; odd n, so
    the byte rows start at every alignment."""
    from realnvp_hip import _lib
    B, nv, first = 3, 2, 5
    gen = torch.Generator().manual_seed(n)
    x = 3.0 * torch.randn(B, n, generator=gen)
    x[:, :8] = torch.tensor([-100.0, -25.0, -21.0, 21.0, 25.0, 100.0, 0.0, -0.0])     # both clamps fire
    x = x.to(DEV)
    v = torch.empty_like(x)
    L().logit_inv(x.data_ptr(), v.data_ptr(), 0.9, x.numel(), sptr())
    assert float(v.min()) < 0.0 and float(v.max()) > 1.0
    stored = min(nv, cap - first)
    want = {_lib.RNVP_OUT_F32: v,
            _lib.RNVP_OUT_U8_ROUND: torch_round_rule(v),
            _lib.RNVP_OUT_U8_FLOOR: torch.floor(v * 256).clamp(0, 255).to(torch.uint8)}
    for mode, w in want.items():
        if mode == _lib.RNVP_OUT_F32:
            dst = torch.full((8, n), NAN, device=DEV)
            fill = dst.clone()
        else:
            dst = torch.full((8, n), 0xAB, device=DEV, dtype=torch.uint8)
            fill = dst.clone()
        ctl = make_ctl(dst, cap, first, nv)
        L().latent_out(x.data_ptr(), ctl.data_ptr(), 0.9, B, n, mode, sptr())
        got = dst.view(torch.int32 if mode == _lib.RNVP_OUT_F32 else torch.uint8)
        exp = fill.clone()
        exp[first:first + stored] = w[:stored]
        exp = exp.view(got.dtype)
        assert torch.equal(got[first:first + stored], exp[first:first + stored]), ("stored rows", mode)
        assert torch.equal(got, exp), ("untouched rows", mode)
        c = read_ctl(ctl)
        assert (c.first, c.n_done, c.overflow) == (7, stored, int(cap < 7)), mode
        assert (c.dst, c.cap, c.n_valid, c.temperature) == (dst.data_ptr(), cap, nv, 1.0)
        # a second batch lands behind the first (or nowhere, once past cap)
        L().latent_out(x.data_ptr(), ctl.data_ptr(), 0.9, B, n, mode, sptr())
        c = read_ctl(ctl)
        more = max(0, min(nv, cap - 7))
        assert (c.first, c.n_done, c.overflow) == (9, stored + more, 1), mode
        exp = exp.view(fill.dtype)
        exp[7:7 + more] = w[:more]
        assert torch.equal(dst.view(got.dtype), exp.view(got.dtype)), ("second batch", mode)


@pytest.mark.parametrize("mode", ["lerp", "slerp"])
@pytest.mark.parametrize("n", [768, 4099, 40000])
def test_mix_kernel(n, mode):
    """A random pair, b = a and b = 1.001 a at t = 0 .. 1 against
    mix_reference.  Bound 1e-6 relative L2 per output row: three fp32
    roundings per element (6e-8 each) with weights formed in fp64 that are
    <= 1 for these inputs.  n = 40000 takes the path of several workgroups
    per pair."""
    from realnvp_hip import _lib
    from realnvp_hip.codec import mix_reference
    gen = torch.Generator().manual_seed(n)
    a = torch.randn(3, n, generator=gen)
    b = torch.randn(3, n, generator=gen)
    b[1] = a[1]
    b[2] = a[2] * 1.001
    t = torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0])
    want = mix_reference(a.numpy(), b.numpy(), t.numpy(), mode)
    ad, bd, td = a.to(DEV), b.to(DEV), t.to(DEV)
    out = torch.full((3, 5, n), NAN, device=DEV)
    ws = torch.full((9,), NAN, device=DEV, dtype=torch.float64)           # the call zeroes what it needs
    L().latent_mix(ad.data_ptr(), bd.data_ptr(), td.data_ptr(), out.data_ptr(), 3, 5, n,
                   {"lerp": _lib.RNVP_MIX_LERP, "slerp": _lib.RNVP_MIX_SLERP}[mode], ws.data_ptr(), sptr())
    got = out.cpu().numpy()
    assert_rel_l2(got.reshape(15, n), want.reshape(15, n), 1e-6, "%s n=%d" % (mode, n))
    assert np.array_equal(got[:, 0], a.numpy()) and np.array_equal(got[:, 4], b.numpy())     # the ends themselves
    if mode == "slerp":
        sums = ws.cpu().numpy().reshape(3, 3)
        ref = torch.stack([(a.double() * b.double()).sum(1), (a.double() ** 2).sum(1), (b.double() ** 2).sum(1)], 1)
        assert np.abs(sums / ref.numpy() - 1.0).max() <= 1e-12


# -------------------------------------------------------------------- codec
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_encode_matches_the_oracle(model, images, noise, oracle_z, graph):
    """Batches of 4, 4, 2 against flow_f in float64 on the oracle's logit
    transform, with an explicit noise tensor and with "mid"."""
    cd = codec(model, 4, graph=graph)
    z = cd.encode(images.to(DEV), noise=noise.to(DEV))
    assert z.dtype == torch.float32 and tuple(z.shape) == (N, 3, SIZE, SIZE) and z.is_cuda
    assert_rel_l2(z.cpu().numpy(), oracle_z["noise"], FLOW_RTOL, "explicit noise")
    zm = cd.encode([images[i:i + 4].to(DEV) for i in range(0, N, 4)], noise="mid")
    assert_rel_l2(zm.cpu().numpy(), oracle_z["mid"], FLOW_RTOL, "mid")
    assert (len(cd.graphs) == 1) == graph
    # the last batch of 2: the same rows whatever the pixel buffer held before
    cd.pix.fill_(0.75)
    again = cd.encode(images[8:].to(DEV), noise="mid")
    assert float(cd.pix[2:].abs().max()) == 0.0
    assert_rel_l2(again.cpu().numpy(), oracle_z["mid"][8:], FLOW_RTOL, "ragged batch alone")
    assert_abs(again, zm[8:], 1e-5, "ragged batch alone against inside the pass")


def test_philox_encode_follows_the_image(model, images):
    """noise="philox" is keyed by the image's index in the pass: B = 4 and 5
    agree, the latents differ from "mid" by no more than a dequantisation
    step allows and are not "mid"."""
    a = codec(model, 4, seed=7).encode(images.to(DEV), noise="philox")
    b = codec(model, 5, seed=7).encode(images.to(DEV), noise="philox")
    # each is within FLOW_RTOL of the exact latents of the same noise
    assert_rel_l2(a.cpu().numpy(), b.cpu().numpy(), 2 * FLOW_RTOL, "B=4 against B=5")
    mid = codec(model, 4, seed=7).encode(images.to(DEV))
    assert float((a - mid).abs().max()) > 1e-3
    other = codec(model, 4, seed=8).encode(images.to(DEV), noise="philox")
    assert float((a - other).abs().max()) > 1e-3


def test_decode_matches_the_oracle_and_the_sampler(model, latents, oracle_x):
    from realnvp_hip.sampler import FlowSampler
    zd = latents.to(DEV)
    sm = FlowSampler(model, 4, dtype="fp32", graph=False)
    for graph in (False, True):
        cd = codec(model, 4, graph=graph)
        img = cd.decode(zd)
        assert img.dtype == torch.float32 and tuple(img.shape) == (N, 3, SIZE, SIZE)
        assert_rel_l2(img.cpu().numpy(), oracle_x, FLOW_RTOL, "decode graph=%s" % graph)
        for i in (0, 4):
            assert_abs(img[i:i + 4], sm.sample(z=zd[i:i + 4]), SAMPLER_ATOL, "against FlowSampler, rows %d.." % i)
        # the byte formats are rules on the fp32 output
        assert torch.equal(cd.decode(zd, u8="round"), torch_round_rule(img))
        assert torch.equal(cd.decode(zd, u8="floor"), torch.floor(img * 256).clamp(0, 255).to(torch.uint8))
        assert len(cd.graphs) == (3 if graph else 0)


def test_bf16_decode_matches_the_dropin_inverse(latents):
    """bf16: the same kernels as the drop-in's g on the same zero-padded
    batches, then the same inverse logit transform."""
    import utils
    B = 4
    m = make_model().set_precision("bf16")
    cd = codec(m, B, dtype="bf16")
    zd = latents.to(DEV)
    img = cd.decode(zd)
    ref = []
    with torch.no_grad():
        for i in range(0, N, B):
            rows = min(B, N - i)
            pad = torch.zeros(B, 3, SIZE, SIZE, device=DEV)
            pad[:rows] = zd[i:i + rows]
            ref.append(utils.logit_transform(m.g(pad), reverse=True)[0][:rows])
    assert_abs(img, torch.cat(ref), 1e-5, "bf16 decode")


def test_exact_round_trip(model, images):
    """fp32: decode(encode(pix, "mid"), u8="floor") is round(255 pix) for all
    10 images, bit for bit.  (The oracle in float32 reconstructs within
    5.3e-5 of a quantisation step against a margin of 0.5.)"""
    cd = codec(model, 4)
    back = cd.decode(cd.encode(images.to(DEV), "mid"), u8="floor")
    want = torch.round(images * 255).to(torch.uint8)
    bad = int((back.cpu() != want).sum())
    print("round trip: %d of %d bytes differ" % (bad, want.numel()))
    assert back.dtype == torch.uint8 and bad == 0


def test_samples_belong_to_their_index(model):
    got = {B: codec(model, B, seed=11).sample(10) for B in (4, 5, 10)}
    assert got[4].dtype == torch.float32 and tuple(got[4].shape) == (N, 3, SIZE, SIZE)
    assert bool(torch.isfinite(got[4]).all())
    assert_abs(got[5], got[4], 1e-5, "B=5 against B=4")
    assert_abs(got[10], got[4], 1e-5, "B=10 against B=4")
    cd = codec(model, 4, seed=11)
    assert_abs(cd.sample(6, first=4), got[4][4:], 1e-5, "first=4")
    assert float((codec(model, 4, seed=12).sample(10) - got[4]).abs().max()) > 1e-2
    # a later call is the same images; the graph is kept
    g = cd.graphs[("sample", 0)]
    assert_abs(cd.sample(10), got[4], 1e-5, "a later call")
    z1 = cd.z.clone()                      # the latents of the last batch (samples 8..11) at T = 1
    assert cd.graphs[("sample", 0)] is g
    # temperature 0: every latent is zero, ten identical images
    cold = cd.sample(10, temperature=0.0)
    assert float(cd.z.abs().max()) == 0.0
    assert_abs(cold, cold[:1].expand_as(cold), 1e-5, "ten images of the zero latent")     # (slots of a batch: as B above)
    # the per-call temperature does not stick; set_temperature does, with no re-capture
    assert_abs(cd.sample(10), got[4], 1e-5, "after a per-call temperature")
    cd.set_temperature(0.5)
    half = cd.sample(10)
    assert cd.graphs[("sample", 0)] is g and len(cd.graphs) == 1
    assert torch.equal(cd.z, 0.5 * z1)
    assert float((half - got[4]).abs().max()) > 1e-3
    # bytes: the torch rule on the fp32 output
    assert torch.equal(cd.sample(10, u8="round"), torch_round_rule(half))
    # the latents are the mirror's
    from realnvp_hip.codec import prior_reference
    want = prior_reference(11, 8, 4, D, 0.5).reshape(4, 3, SIZE, SIZE)
    assert float(np.abs(cd.z.cpu().numpy() - want).max()) <= 2e-5 * 0.5


def test_interpolate(model, images):
    from realnvp_hip.codec import mix_reference
    cd = codec(model, 4)
    a, b = images[:2].to(DEV), images[2:4].to(DEV)
    mov = cd.interpolate(a, b, steps=5, mode="slerp", u8="floor")
    assert mov.dtype == torch.uint8 and tuple(mov.shape) == (2, 5, 3, SIZE, SIZE)
    want = torch.round(images * 255).to(torch.uint8).to(DEV)
    assert torch.equal(mov[:, 0], want[:2]) and torch.equal(mov[:, 4], want[2:4])
    for mode in ("slerp", "lerp"):
        f = cd.interpolate(a, b, steps=5, mode=mode)
        za, zb = cd.encode(a), cd.encode(b)
        mix = mix_reference(za.cpu().numpy(), zb.cpu().numpy(), np.linspace(0.0, 1.0, 5), mode)
        ref = cd.decode(torch.from_numpy(mix.reshape(10, 3, SIZE, SIZE)).float().to(DEV))
        assert_rel_l2(f.reshape(10, -1).cpu().numpy(), ref.reshape(10, -1).cpu().numpy(), 1e-4, mode)
    # the frames move: the middle one is neither end
    assert float((f[:, 2] - f[:, 0]).abs().max()) > 1e-2 and float((f[:, 2] - f[:, 4]).abs().max()) > 1e-2


def test_argument_checks(model, images):
    cd = codec(model, 4)
    x = images.to(DEV)
    bad_calls = [lambda: cd.decode(x, u8="ceil"), lambda: cd.decode(x[0]), lambda: cd.decode(x[:, :, :8]),
                 lambda: cd.encode(x[:, :2]), lambda: cd.encode(x, noise="none"), lambda: cd.encode(x, noise=x[:3]),
                 lambda: cd.encode([x[:5]]), lambda: cd.sample(0), lambda: cd.sample(4, first=-1),
                 lambda: cd.sample(4, temperature=-1.0), lambda: cd.sample(4, u8="u8"),
                 lambda: cd.interpolate(x[:2], x[2:4], steps=1), lambda: cd.interpolate(x[:2], x[2:5]),
                 lambda: cd.interpolate(x[:2], x[2:4], mode="cubic"), lambda: cd.set_temperature(-0.5)]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
        assert not cd.graphs, i          # nothing was launched or captured
    from realnvp_hip import FlowCodec
    with pytest.raises(RuntimeError, match="eval"):
        FlowCodec(make_model().train(), 4)


def test_graphs_follow_moved_weights(images):
    """After a FlowTrainer step has moved the parameters into its arena the
    next call re-captures and matches the eager codec on the current weights."""
    from realnvp_hip.trainer import FlowTrainer
    m = make_model()
    x = images.to(DEV)
    cd = codec(m, 4, seed=3)
    z1, s1 = cd.encode(x).clone(), cd.sample(10).clone()
    g = dict(cd.graphs)
    assert len(g) == 2
    assert_abs(cd.encode(x), z1, 1e-5, "second pass")
    assert cd.graphs[("encode", "noise")] is g[("encode", "noise")]
    eager = codec(m, 4, seed=3, graph=False)
    assert_abs(eager.encode(x), z1, 1e-5, "eager against graph, encode")
    assert_abs(eager.sample(10), s1, 1e-5, "eager against graph, sample")
    m.train()
    tr = FlowTrainer(m, 4, dtype="fp32")
    tr.set_pixels(pixels(4, 3, SIZE, seed=2).to(DEV))
    tr.step()
    m.eval()
    z2, s2 = cd.encode(x).clone(), cd.sample(10).clone()
    assert cd.graphs[("encode", "noise")] is not g[("encode", "noise")]
    assert cd.graphs[("sample", 0)] is not g[("sample", 0)]
    assert_abs(z2, eager.encode(x), 1e-5, "encode after the step")
    assert_abs(s2, eager.sample(10), 1e-5, "sample after the step")
    assert float((z2 - z1).abs().max()) > 1e-4


def test_codec_of_the_averaged_weights(images):
    """Inside ema_weights() the output is that of a second model loaded from
    ema_state_dict()."""
    from realnvp_hip.trainer import FlowTrainer
    m = make_model().train()
    tr = FlowTrainer(m, 4, dtype="fp32", ema_decay=0.5)
    for s in range(2):
        tr.set_pixels(pixels(4, 3, SIZE, seed=20 + s).to(DEV))
        tr.step()
    m.eval()
    x = images.to(DEV)
    cd = codec(m, 4, seed=9)
    raw_z, raw_s = cd.encode(x).clone(), cd.sample(10).clone()
    with tr.ema_weights():
        in_z, in_s = cd.encode(x).clone(), cd.sample(10).clone()
    second = make_model()
    second.load_state_dict(tr.ema_state_dict())
    c2 = codec(second.eval(), 4, seed=9)
    assert_abs(in_z, c2.encode(x), 1e-5, "encode: average in place against a second model")
    assert_abs(in_s, c2.sample(10), 1e-5, "sample: average in place against a second model")
    assert float((raw_z - in_z).abs().max()) > 1e-5
    assert_abs(cd.encode(x), raw_z, 1e-5, "encode after the block")
    assert_abs(cd.sample(10), raw_s, 1e-5, "sample after the block")
