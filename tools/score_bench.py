"""GPU benchmark: FlowScorer (K = 1, captured) against FlowEvaluator at config
1's shape (64x64x3, R4, D32, B = 64, bf16), in images per second.

Both are built on ONE eval-mode model in one process and timed alternately
(so drift of the card hits both alike): each round is --batches full batches
through add_batch between two device synchronisations (host clock), after a
warm-up pass that captures the graphs.  The scorer's round includes begin()
and ends with its own documented sync, scores(); the evaluator's with
mean_logll().  The spread between rounds of the same class is the noise floor
of the comparison.

    python tools/score_bench.py [--rounds 5] [--batches 32] [--batch 64] [--out profiles/score_bench.txt]

Needs a GPU: there is nothing to measure without one.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "dl-normalizing-flows_amd"), ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, default=32)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/score_bench.py needs a GPU")
    from bench import build_model, synthetic_pixels
    from realnvp_hip import FlowScorer
    from realnvp_hip.evaluator import FlowEvaluator
    dev = torch.device("cuda", 0)
    B, nb = args.batch, args.batches
    model = build_model(64, 4, 32, 5, dev, 0).eval()
    pix = [synthetic_pixels(B, 3, 64, seed=s).to(dev) for s in range(4)]
    sc = FlowScorer(model, B, dtype="bf16", seed=1000)
    ev = FlowEvaluator(model, B, dtype="bf16", seed=1000)

    def scorer_pass():
        sc.begin(nb * B)
        for i in range(nb):
            sc.add_batch(pix[i % len(pix)])
        return sc.scores()

    def evaluator_pass():
        ev.begin()
        for i in range(nb):
            ev.add_batch(pix[i % len(pix)])
        return ev.mean_logll()
    passes = {"FlowScorer": scorer_pass, "FlowEvaluator": evaluator_pass}
    for fn in passes.values():        # warm-up: captures the graphs
        fn()
    torch.cuda.synchronize()
    ips = {name: [] for name in passes}
    for _ in range(args.rounds):
        for name, fn in passes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ips[name].append(nb * B / (time.perf_counter() - t0))
    s = scorer_pass()
    out = {"batch": B, "batches_per_round": nb, "rounds": args.rounds, "dtype": "bf16", "n_draws": 1,
           "images_per_s": {name: dict(mean=round(sum(v) / len(v), 1), min=round(min(v), 1), max=round(max(v), 1),
                                       rounds=[round(x, 1) for x in v]) for name, v in ips.items()},
           "scores_finite": bool(torch.isfinite(s).all()), "mean_logll": {"scorer": sc.mean_logll(),
                                                                          "evaluator": evaluator_pass()}}
    m = out["images_per_s"]
    out["scorer_over_evaluator"] = round(m["FlowScorer"]["mean"] / m["FlowEvaluator"]["mean"], 4)
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
