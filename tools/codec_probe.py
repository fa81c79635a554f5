"""GPU probe: FlowCodec.sample against FlowSampler at config 1's shape
(64x64x3, R4, D32, B = 64, bf16), in images per second, and the byte round
trip decode(encode(x, "mid"), u8="floor") in fp32 and bf16.

Both classes are built on ONE eval-mode model in one process and timed
alternately (so drift of the card hits both alike): a round is --batches
batches between two device synchronisations (host clock) -- one
cd.sample(batches * B) call for the codec, batches FlowSampler.sample() calls
for the sampler -- after a warm-up round that captures the graphs.  The spread
between rounds of the same class is the noise floor of the comparison.

The round trip runs on config 1's random-init model (one batch of 64 images)
and on the 16x16 / base dim 4 / 1 block model of tests/test_gpu_codec.py (its
10 images): the number of bytes that differ from round(255 x).

    python tools/codec_probe.py [--rounds 5] [--batches 100] [--batch 64] [--out profiles/codec_probe.txt]

Needs a GPU: there is nothing to measure without one.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "dl-normalizing-flows_amd"), os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402


def round_trip(model, B, dtype, pix):
    """bytes of decode(encode(pix, "mid"), u8="floor") that differ from round(255 pix)"""
    from realnvp_hip import FlowCodec
    cd = FlowCodec(model, B, dtype=dtype)
    back = cd.decode(cd.encode(pix, "mid"), u8="floor")
    want = torch.round(pix * 255).to(torch.uint8)
    return dict(bytes=want.numel(), differ=int((back != want).sum()))


def small_model(dev):
    """tests/test_gpu_codec.py::make_model"""
    import numpy as np

    import flow_realnvp
    import utils
    from formula_init import formula_state
    prior = torch.distributions.Normal(torch.tensor(0.0, device=dev), torch.tensor(1.0, device=dev))
    m = flow_realnvp.RealNVP(3, 16, prior, utils.Hyperparameters(4, 1, True, True, True, True))
    m.load_state_dict(formula_state(m))
    m = m.to(dev).train()
    with torch.no_grad():
        m(torch.from_numpy(np.random.default_rng(7).random((8, 3, 16, 16), dtype=np.float32)).to(dev) * 2 - 1)
    return m.eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, default=100)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codec_probe.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/codec_probe.py needs a GPU")
    from bench import build_model, synthetic_pixels
    from formula_init import pixels
    from realnvp_hip import FlowCodec
    from realnvp_hip.sampler import FlowSampler
    dev = torch.device("cuda", 0)
    B, nb = args.batch, args.batches
    model = build_model(64, 4, 32, 5, dev, 0).eval()
    cd = FlowCodec(model, B, dtype="bf16", seed=1000)
    sm = FlowSampler(model, B, dtype="bf16")

    def codec_round():
        return cd.sample(nb * B)

    def sampler_round():
        for _ in range(nb):
            out = sm.sample()
        return out
    rounds = {"FlowCodec.sample": codec_round, "FlowSampler": sampler_round}
    for fn in rounds.values():        # warm-up: captures the graphs
        fn()
    torch.cuda.synchronize()
    ips = {name: [] for name in rounds}
    for _ in range(args.rounds):
        for name, fn in rounds.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ips[name].append(nb * B / (time.perf_counter() - t0))
    imgs = codec_round()
    out = {"batch": B, "batches_per_round": nb, "rounds": args.rounds, "dtype": "bf16",
           "images_per_s": {name: dict(mean=round(sum(v) / len(v), 1), min=round(min(v), 1), max=round(max(v), 1),
                                       rounds=[round(x, 1) for x in v]) for name, v in ips.items()},
           "samples_finite": bool(torch.isfinite(imgs).all())}
    m = out["images_per_s"]
    out["codec_over_sampler"] = round(m["FlowCodec.sample"]["mean"] / m["FlowSampler"]["mean"], 4)
    pix64 = synthetic_pixels(B, 3, 64, seed=3).to(dev)
    small, pix16 = small_model(dev), pixels(10, 3, 16, seed=41).to(dev)
    out["round_trip"] = {"config1_fp32": round_trip(model.set_precision("fp32"), B, "fp32", pix64),
                         "config1_bf16": round_trip(model.set_precision("bf16"), B, "bf16", pix64),
                         "test_model_fp32": round_trip(small, 4, "fp32", pix16),
                         "test_model_bf16": round_trip(small.set_precision("bf16"), 4, "bf16", pix16)}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
