"""Golden trajectory of the reference loop WITH gradient-norm clipping and a
learning-rate schedule (build container only, like tools/make_goldens.py).

    python tools/make_stepctl_golden.py     # writes tests/golden/stepctl_m32_d8_r1.npz

Three steps of the train.py:176-200 loop on the m32_d8_r1 model (formula
weights, batch 4, pixel seeds 100+s / noise seeds 200+s -- the inputs of
make_goldens.model_goldens' trajectory) with, after loss.backward(),

    torch.nn.utils.clip_grad_norm_(model.parameters(), 600.0)

Adam(5e-4, weight_decay 5e-5) and ChainedScheduler([LinearLR(0.25,
total_iters=2), ExponentialLR(0.8)]).  The reference is imported through
make_goldens (same CPU shim); only arrays are stored.
"""
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_goldens as G  # noqa: E402  (imports the reference, CPU shim applied)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributions as D  # noqa: E402
from torch.optim.lr_scheduler import ChainedScheduler, ExponentialLR, LinearLR  # noqa: E402

NAME, SIZE, BD, RB, B, STEPS = "m32_d8_r1", 32, 8, 1, 4, 3
MAX_NORM, BASE_LR, WD = 600.0, 5e-4, 5e-5
WARM_START, WARM_STEPS, GAMMA = 0.25, 2, 0.8


def logit_inputs(pix, noise):
    x = (pix * 255.0 + noise) / 256.0
    x = ((x * 2.0 - 1.0) * 0.9 + 1.0) / 2.0
    xl = torch.log(x) - torch.log(1.0 - x)
    pre = torch.tensor(np.log(0.9) - np.log(0.1))
    ld = (torch.nn.functional.softplus(xl) + torch.nn.functional.softplus(-xl)
          - torch.nn.functional.softplus(-pre)).sum(dim=(1, 2, 3))
    return xl, ld


def main():
    prior = D.Normal(torch.tensor(0.0), torch.tensor(1.0), validate_args=False)
    model = G.flow_realnvp.RealNVP(3, SIZE, prior, G.hps(BD, RB))
    model.load_state_dict(G.formula_state(model))
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=BASE_LR, weight_decay=WD)
    sched = ChainedScheduler([LinearLR(opt, start_factor=WARM_START, total_iters=WARM_STEPS),
                              ExponentialLR(opt, gamma=GAMMA)])
    lls, norms, lrs, m1, m2 = [], [], [], [], []
    for s in range(STEPS):
        xl, ld = logit_inputs(G.pixels(B, 3, SIZE, seed=100 + s), G.uniform_noise(B, 3, SIZE, seed=200 + s))
        opt.zero_grad()
        lp, ws = model(xl)
        ll = (lp + ld).mean()
        (-ll + 5e-5 * ws).backward()
        norm = torch.nn.utils.clip_grad_norm_(model.parameters(), MAX_NORM)
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
        lls.append(float(ll))
        norms.append(float(norm))
        st = [opt.state[p] for p in model.parameters() if p in opt.state]
        m1.append(float(torch.sqrt(sum(t["exp_avg"].double().pow(2).sum() for t in st))))
        m2.append(float(sum(t["exp_avg_sq"].double().abs().sum() for t in st)))
        print("step %d logll %.4f pre-clip norm %.2f lr %.4g |m|2 %.4f |v|1 %.6g" % (s + 1, lls[-1], norms[-1],
                                                                                  lrs[-1], m1[-1], m2[-1]))
    _, _, x_in, _ = G.model_inputs(B, SIZE)
    model.eval()
    with torch.no_grad():
        lp_after, _ = model(x_in.clone())
    d = dict(pixel_seeds=np.array([100 + s for s in range(STEPS)]), noise_seeds=np.array([200 + s for s in range(STEPS)]),
             eval_pixel_seed=np.array(10), eval_noise_seed=np.array(11), batch=np.array(B),
             max_norm=np.array(MAX_NORM), base_lr=np.array(BASE_LR), weight_decay=np.array(WD),
             warmup_start=np.array(WARM_START), warmup_steps=np.array(WARM_STEPS), gamma=np.array(GAMMA),
             traj_logll=np.array(lls), traj_grad_norm=np.array(norms), traj_lr=np.array(lrs),
             traj_exp_avg_l2=np.array(m1), traj_exp_avg_sq_l1=np.array(m2),
             traj_eval_logprob_after=G.f32(lp_after))
    G.save("stepctl_%s.npz" % NAME, d)


if __name__ == "__main__":
    main()
