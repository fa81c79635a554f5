"""GPU probe: what a micro-step of FlowTrainer(accum_steps=8) costs at config 1
(64x64x3, R4, D32, B=64, bf16, captured) beside the clip-schedule step it is
built on.

Two trainers in ONE process, replayed alternately (so drift of the card hits
both alike):
  clip    max_grad_norm=1e9, accum_steps=1: per-coupling rnvp_weight_norm_bwd,
          rnvp_grad_sumsq + rnvp_step_control, one
          rnvp_weight_norm_bwd_adam(from_slabs=0)
  accum8  accum_steps=8: the same launches with rnvp_grad_accumulate in
          rnvp_grad_sumsq's place; 7 replays of 8 are held (the parameter pass
          sees ctl->skip and touches nothing), the 8th applies
Each round times REPS replays per trainer with device events (REPS a multiple
of 8; the default 64 replays are 1.2 s per leg and round); the spread between
rounds of the same trainer is the noise floor of the comparison.  A second
pass brackets every replay of accum8 with events of its own and reports held
and final micro-steps apart.  Then rnvp_grad_accumulate alone on accum8's
arena, held and final, with its achieved bytes/s over the algorithmic bytes
(held: gradient + accumulator read, accumulator written = 12 B per element;
final: + mask read and gradient written = 17 B).

    python tools/probe/accum_step.py [--rounds 5] [--reps 64] [--batch 64] [--legs clip,accum8]

--legs clip runs on a tree without accum_steps too: the same script on a build
of the parent commit gives the parent's time for the launches that leg shares
with this tree.
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

K = 8


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
    ap.add_argument("--legs", default="clip,accum8")
    args = ap.parse_args()
    if args.reps % K:
        ap.error("--reps must be a multiple of %d" % K)
    from realnvp_hip import _lib
    from realnvp_hip.trainer import FlowTrainer
    dev = torch.device("cuda", 0)
    kinds = {"clip": dict(max_grad_norm=1e9), "accum8": dict(accum_steps=K)}
    kinds = {name: kinds[name] for name in args.legs.split(",")}
    trainers = {}
    for name, kw in kinds.items():
        tr = FlowTrainer(build_model(64, 4, 32, 5, dev, 0), args.batch, dtype="bf16", seed=1000, **kw)
        tr.set_pixels(synthetic_pixels(args.batch, 3, 64, seed=0).to(dev))
        tr.capture(warmup=1)
        for _ in range(K):
            tr.step()
        trainers[name] = tr
    torch.cuda.synchronize()
    ms = {name: [] for name in kinds}
    for _ in range(args.rounds):
        for name, tr in trainers.items():
            ms[name].append(timed(tr.step, args.reps))
    out = {"batch": args.batch, "rounds": args.rounds, "reps": args.reps,
           "ms_per_step": {name: summary(v) for name, v in ms.items()}}
    if "accum8" in trainers:
        tr = trainers["accum8"]
        if "clip" in trainers:
            a, c = out["ms_per_step"]["accum8"], out["ms_per_step"]["clip"]
            a["delta_vs_clip"] = round(a["mean"] - c["mean"], 4)
        # every replay on its own: held and final micro-steps apart
        assert tr.step_control_state()["micro"] == 0
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        for e0, e1 in ev:
            e0.record()
            tr.step()
            e1.record()
        torch.cuda.synchronize()
        t = [e0.elapsed_time(e1) for e0, e1 in ev]
        held = [x for j, x in enumerate(t) if j % K < K - 1]
        final = [x for j, x in enumerate(t) if j % K == K - 1]
        out["accum8_per_replay"] = {what: dict(n=len(v), mean=round(sum(v) / len(v), 4), min=round(min(v), 4),
                                               max=round(max(v), 4)) for what, v in (("held", held), ("final", final))}
        st = tr.step_control_state()
        out["accum8_state"] = dict(st, step=int(tr.step_t.item()), noise_step=int(tr.noise_t.item()))
        # the arena pass alone (on a block of its own: the trainer's stays as it is)
        L = _lib.lib()
        s = torch.cuda.current_stream().cuda_stream
        out["grad_accumulate"] = {"n": tr.n, "parts": tr.gs_parts}
        for what, micro, nbytes in (("held", 0, 12 * tr.n), ("final", K - 1, 17 * tr.n)):
            ctl = tr.ctl_buf.clone()
            f = getattr(_lib.StepCtl, "micro")
            ctl[f.offset:f.offset + f.size].view(torch.int32).fill_(micro)

            def acc_pass():
                L.grad_accumulate(C.byref(tr._opt_all), tr.acc.data_ptr(), tr.n, ctl.data_ptr(),
                                  tr.gs_partials.data_ptr(), tr.gs_parts, s)
            timed(acc_pass, 10)
            t = [timed(acc_pass, 50) for _ in range(3)]
            out["grad_accumulate"][what] = dict(algorithmic_bytes=nbytes, us=[round(x * 1e3, 2) for x in t],
                                                tb_per_s=[round(nbytes / (x * 1e-3) / 1e12, 3) for x in t])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
