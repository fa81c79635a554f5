"""Golden trajectory of the reference loop WITH gradient accumulation and
gradient-norm clipping (build container only, like tools/make_goldens.py).

    python tools/make_accum_golden.py     # writes tests/golden/accum_m32_d8_r1.npz

Two optimizer steps of the train.py:176-200 loop on the m32_d8_r1 model
(formula weights) with K = 2 micro-batches of 4 per step: micro-batch s (0..3)
has pixel seed 100+s / noise seed 200+s (the inputs of
make_goldens.model_goldens' trajectory) and the loss

    (-ll + 5e-5 * ws) / K

is backpropagated K times before

    torch.nn.utils.clip_grad_norm_(model.parameters(), MAX_NORM)

and Adam(5e-4, weight_decay 5e-5).  MAX_NORM = 600 is about half the first
accumulated pre-clip norm the script prints (1205.6), so the clip binds in
both steps.  traj_logll holds one value per micro-batch, every other
trajectory one per optimizer step.  The reference is imported through
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
from make_stepctl_golden import logit_inputs  # noqa: E402

NAME, SIZE, BD, RB, B, K, STEPS = "m32_d8_r1", 32, 8, 1, 4, 2, 2
MAX_NORM, BASE_LR, WD = 600.0, 5e-4, 5e-5


def main():
    prior = D.Normal(torch.tensor(0.0), torch.tensor(1.0), validate_args=False)
    model = G.flow_realnvp.RealNVP(3, SIZE, prior, G.hps(BD, RB))
    model.load_state_dict(G.formula_state(model))
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=BASE_LR, weight_decay=WD)
    lls, norms, lrs, m1, m2 = [], [], [], [], []
    for s in range(STEPS):
        opt.zero_grad()
        for k in range(K):
            i = s * K + k
            xl, ld = logit_inputs(G.pixels(B, 3, SIZE, seed=100 + i), G.uniform_noise(B, 3, SIZE, seed=200 + i))
            lp, ws = model(xl)
            ll = (lp + ld).mean()
            ((-ll + 5e-5 * ws) / K).backward()
            lls.append(float(ll))
        norm = torch.nn.utils.clip_grad_norm_(model.parameters(), MAX_NORM)
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        norms.append(float(norm))
        st = [opt.state[p] for p in model.parameters() if p in opt.state]
        m1.append(float(torch.sqrt(sum(t["exp_avg"].double().pow(2).sum() for t in st))))
        m2.append(float(sum(t["exp_avg_sq"].double().abs().sum() for t in st)))
        print("step %d logll %s accumulated pre-clip norm %.2f lr %.4g |m|2 %.4f |v|1 %.6g"
              % (s + 1, ["%.4f" % v for v in lls[-K:]], norms[-1], lrs[-1], m1[-1], m2[-1]))
    _, _, x_in, _ = G.model_inputs(B, SIZE)
    model.eval()
    with torch.no_grad():
        lp_after, _ = model(x_in.clone())
    n = STEPS * K
    d = dict(pixel_seeds=np.array([100 + i for i in range(n)]), noise_seeds=np.array([200 + i for i in range(n)]),
             eval_pixel_seed=np.array(10), eval_noise_seed=np.array(11), batch=np.array(B),
             accum_steps=np.array(K),
             max_norm=np.array(MAX_NORM), base_lr=np.array(BASE_LR), weight_decay=np.array(WD),
             warmup_start=np.array(1.0), warmup_steps=np.array(0), gamma=np.array(1.0),
             traj_logll=np.array(lls), traj_grad_norm=np.array(norms), traj_lr=np.array(lrs),
             traj_exp_avg_l2=np.array(m1), traj_exp_avg_sq_l1=np.array(m2),
             traj_eval_logprob_after=G.f32(lp_after))
    G.save("accum_%s.npz" % NAME, d)


if __name__ == "__main__":
    main()
