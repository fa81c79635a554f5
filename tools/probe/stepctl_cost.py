"""GPU probe: what the step control costs per captured step at config 1
(64x64x3, R4, D32, B=64, bf16).

Three trainers in ONE process, replayed alternately (so drift of the card
hits all three alike): plain, schedule only (one single-workgroup launch more,
rnvp_step_advance instead of rnvp_step_increment), and schedule +
max_grad_norm=1e9 (the data-parallel launch schedule: per-coupling
rnvp_weight_norm_bwd, rnvp_grad_sumsq + rnvp_step_control, one
rnvp_weight_norm_bwd_adam(from_slabs=0)).  Each round times REPS replays per
trainer with device events; the spread between rounds of the same trainer is
the noise floor of the comparison.  Then rnvp_grad_sumsq alone on the
clipping trainer's arena, with its achieved bytes/s over the algorithmic
bytes (4 B gradient + 1 B mask per element).

    python tools/probe/stepctl_cost.py [--rounds 5] [--reps 20] [--batch 64]

--profile KIND (plain | schedule | schedule+clip) only captures that trainer
and replays it --reps times: the run to put under
`rocprofv3 --kernel-trace --stats -- python tools/probe/stepctl_cost.py --profile KIND`
for the per-kernel times of the parameter pass.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "dl-normalizing-flows_amd"), ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402

from bench import build_model, synthetic_pixels  # noqa: E402


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--profile", default=None, choices=["plain", "schedule", "schedule+clip"])
    args = ap.parse_args()
    from realnvp_hip import _lib
    from realnvp_hip.stepctl import StepSchedule
    from realnvp_hip.trainer import FlowTrainer
    dev = torch.device("cuda", 0)
    sch = StepSchedule(warmup_steps=100, warmup_start=0.1, decay="cosine", decay_rate=0.05, decay_steps=10000)
    kinds = {"plain": {}, "schedule": dict(lr_schedule=sch), "schedule+clip": dict(lr_schedule=sch, max_grad_norm=1e9)}
    if args.profile is not None:
        kinds = {args.profile: kinds[args.profile]}
    trainers = {}
    for name, kw in kinds.items():
        tr = FlowTrainer(build_model(64, 4, 32, 5, dev, 0), args.batch, dtype="bf16", seed=1000, **kw)
        tr.set_pixels(synthetic_pixels(args.batch, 3, 64, seed=0).to(dev))
        tr.capture(warmup=1)
        for _ in range(5):
            tr.step()
        trainers[name] = tr
    torch.cuda.synchronize()
    if args.profile is not None:
        print(json.dumps({"profile": args.profile, "ms_per_step": round(timed(trainers[args.profile].step, args.reps), 4)}))
        return
    ms = {name: [] for name in kinds}
    for _ in range(args.rounds):
        for name, tr in trainers.items():
            ms[name].append(timed(tr.step, args.reps))
    out = {"batch": args.batch, "rounds": args.rounds, "reps": args.reps, "ms_per_step": {}}
    for name, v in ms.items():
        out["ms_per_step"][name] = dict(mean=round(sum(v) / len(v), 4), min=round(min(v), 4), max=round(max(v), 4),
                                        rounds=[round(x, 4) for x in v])
    base = out["ms_per_step"]["plain"]["mean"]
    for name in ("schedule", "schedule+clip"):
        out["ms_per_step"][name]["delta_vs_plain"] = round(out["ms_per_step"][name]["mean"] - base, 4)
    st = trainers["schedule+clip"].step_control_state()
    out["clip_state"] = st
    # the arena pass alone
    tr = trainers["schedule+clip"]
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream

    def sumsq():
        L.grad_sumsq(C.byref(tr._opt_all), tr.n, tr.gs_partials.data_ptr(), tr.gs_parts, s)
    timed(sumsq, 10)
    t = [timed(sumsq, 50) for _ in range(3)]
    nbytes = 5 * tr.n
    out["grad_sumsq"] = dict(n=tr.n, parts=tr.gs_parts, algorithmic_bytes=nbytes, us=[round(x * 1e3, 2) for x in t],
                             tb_per_s=[round(nbytes / (x * 1e-3) / 1e12, 3) for x in t])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
