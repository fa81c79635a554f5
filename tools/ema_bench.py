"""GPU benchmark: what FlowTrainer(ema_decay=d) costs at config 1 (64x64x3, R4,
D32, B=64, bf16, captured), and rnvp_ema_update alone against its bound.

Two trainers in ONE process, replayed alternately (so drift of the card hits
both alike):
  plain   the step bench.py measures
  ema     ema_decay=0.999: the same launches plus rnvp_ema_update after the
          last Adam launch
Each round times REPS replays per trainer with device events; the spread
between rounds of the same trainer is the noise floor of the comparison.
Then rnvp_ema_update alone over the ema trainer's arena (on a block of its
own: the trainer's average stays as it is), with its achieved bytes/s over
the algorithmic 12 B per element (parameter and average read, average
written) and the fraction of the 6.29 TB/s a float4 copy reaches on this
card; rnvp_ema_swap likewise (16 B per element).

    python tools/ema_bench.py [--rounds 5] [--reps 64] [--batch 64] [--out profiles/ema_step.txt]

Needs a GPU: there is nothing to measure without one.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "dl-normalizing-flows_amd"), ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402

HBM_TBS = 6.29      # achievable HBM bandwidth of the MI355X (float4 copy), TB/s


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def summary(v):
    return dict(mean=round(sum(v) / len(v), 4), min=round(min(v), 4), max=round(max(v), 4),
                rounds=[round(x, 4) for x in v])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=64)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_step.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/ema_bench.py needs a GPU")
    from bench import build_model, synthetic_pixels
    from realnvp_hip import _lib
    from realnvp_hip.trainer import FlowTrainer
    dev = torch.device("cuda", 0)
    kinds = {"plain": dict(), "ema": dict(ema_decay=0.999)}
    trainers = {}
    for name, kw in kinds.items():
        tr = FlowTrainer(build_model(64, 4, 32, 5, dev, 0), args.batch, dtype="bf16", seed=1000, **kw)
        tr.set_pixels(synthetic_pixels(args.batch, 3, 64, seed=0).to(dev))
        tr.capture(warmup=1)
        for _ in range(8):
            tr.step()
        trainers[name] = tr
    torch.cuda.synchronize()
    ms = {name: [] for name in kinds}
    for _ in range(args.rounds):
        for name, tr in trainers.items():
            ms[name].append(timed(tr.step, args.reps))
    out = {"batch": args.batch, "rounds": args.rounds, "reps": args.reps,
           "ms_per_step": {name: summary(v) for name, v in ms.items()}}
    e, p = out["ms_per_step"]["ema"], out["ms_per_step"]["plain"]
    e["delta_vs_plain"] = round(e["mean"] - p["mean"], 4)
    tr = trainers["ema"]
    out["ema_state"] = dict(tr.ema_state(), step=int(tr.step_t.item()))
    # the arena passes alone
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    n = tr.n
    avg, blk = tr.ema.clone(), tr.ema_buf.clone()

    def update():
        L.ema_update(avg.data_ptr(), tr.param.data_ptr(), n, blk.data_ptr(), tr.step_t.data_ptr(), 1, None, s)

    def swap():
        L.ema_swap(avg.data_ptr(), tr.grad.data_ptr(), n, s)       # (an even number of times: both stay as they are)
    for what, fn, per_elem in (("ema_update", update, 12), ("ema_swap", swap, 16)):
        nbytes = per_elem * n
        timed(fn, 10)
        t = [timed(fn, 50) for _ in range(3)]
        tbs = [nbytes / (x * 1e-3) / 1e12 for x in t]
        out[what] = dict(n=n, algorithmic_bytes=nbytes, bound_us=round(nbytes / HBM_TBS / 1e6, 2),
                         us=[round(x * 1e3, 2) for x in t], tb_per_s=[round(x, 3) for x in tbs],
                         fraction_of_bound=[round(x / HBM_TBS, 3) for x in tbs])
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
