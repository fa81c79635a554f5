"""Host side of the device step control (include/realnvp_hip.h, "step
control"): the learning-rate schedule's configuration and its float64 mirror.
Importable and usable without a GPU.

A FlowTrainer built with ``lr_schedule`` and / or ``max_grad_norm`` keeps a
device-resident ``rnvp_step_ctl`` block; ``rnvp_step_control`` evaluates the
schedule there from the optimizer's step counter, so a captured step follows
it without re-capture.  With ``accum_steps = K > 1`` the same block counts
the micro-steps of the open optimizer step (``micro``) and decides on the
device which replay holds and which applies.  A FlowTrainer built with
``ema_decay`` keeps the exponential moving average of its parameters with a
block of its own (``rnvp_ema_ctl``); ``ema_decay_at`` mirrors its decay.
"""
import math

DECAYS = {"none": 0, "exp": 1, "cosine": 2}


class StepSchedule:
    """lr(u) = base_lr * factor(u), u = optimizer steps already taken.

    factor(u) = warm(u) * decay(u) with
      warm(u)  = s + (1 - s) min(u, W) / W   (W = warmup_steps, s = warmup_start;
                 1 when W == 0): torch's LinearLR(start_factor=s, total_iters=W)
      decay(u) = 1                                             decay="none"
               = decay_rate ** u                               decay="exp"
                 (torch's ExponentialLR(gamma=decay_rate))
               = f + (1 - f) (1 + cos(pi min(u, T) / T)) / 2   decay="cosine"
                 (f = decay_rate, T = decay_steps: the closed form of
                 CosineAnnealingLR(T_max=T, eta_min=f * base_lr), held at the
                 floor after T)
    Linear warm-up times exponential decay is what ChainedScheduler([LinearLR,
    ExponentialLR]) gives.
    """

    def __init__(self, warmup_steps=0, warmup_start=1.0, decay="none", decay_rate=None, decay_steps=None):
        if int(warmup_steps) != warmup_steps or warmup_steps < 0:
            raise ValueError("warmup_steps must be a non-negative integer, got %r" % (warmup_steps,))
        if not (0.0 < float(warmup_start) <= 1.0):
            raise ValueError("warmup_start must be in (0, 1], got %r" % (warmup_start,))
        if decay not in DECAYS:
            raise ValueError("decay must be one of %s, got %r" % (sorted(DECAYS), decay))
        if decay_rate is None:
            decay_rate = 1.0 if decay != "cosine" else 0.0
        if decay_steps is None:
            decay_steps = 0
        if decay == "exp" and not (float(decay_rate) > 0.0):
            raise ValueError("decay='exp' needs decay_rate > 0, got %r" % (decay_rate,))
        if decay == "cosine":
            if int(decay_steps) != decay_steps or decay_steps <= 0:
                raise ValueError("decay='cosine' needs a positive integer decay_steps, got %r" % (decay_steps,))
            if not (0.0 <= float(decay_rate) <= 1.0):
                raise ValueError("decay='cosine' needs the floor decay_rate in [0, 1], got %r" % (decay_rate,))
        self.warmup_steps = int(warmup_steps)
        self.warmup_start = float(warmup_start)
        self.decay = decay
        self.decay_rate = float(decay_rate)
        self.decay_steps = int(decay_steps)

    def factor(self, u):
        """float64 mirror of rnvp_step_control's formula"""
        u = int(u)
        f = 1.0
        W, s = self.warmup_steps, self.warmup_start
        if W > 0:
            f = s + (1.0 - s) * min(u, W) / W
        if self.decay == "exp":
            f *= self.decay_rate ** u
        elif self.decay == "cosine":
            T, fl = self.decay_steps, self.decay_rate
            f *= fl + (1.0 - fl) * 0.5 * (1.0 + math.cos(math.pi * min(u, T) / T))
        return f

    def config(self):
        return {"warmup_steps": self.warmup_steps, "warmup_start": self.warmup_start, "decay": self.decay,
                "decay_rate": self.decay_rate, "decay_steps": self.decay_steps}

    @classmethod
    def from_config(cls, cfg):
        return cls(**cfg)

    def __eq__(self, other):
        return isinstance(other, StepSchedule) and self.config() == other.config()

    def __repr__(self):
        return "StepSchedule(%s)" % ", ".join("%s=%r" % kv for kv in self.config().items())


def check_max_grad_norm(v):
    """None (no clipping) or a positive finite float"""
    if v is None:
        return None
    v = float(v)
    if not (v > 0.0) or math.isinf(v):
        raise ValueError("max_grad_norm must be a positive finite number or None, got %r" % (v,))
    return v


def check_accum_steps(k):
    """micro-steps per optimizer step: an int in 1 .. 65536 (1 = no accumulation)"""
    if isinstance(k, bool) or not isinstance(k, int) or not (1 <= k <= 65536):
        raise ValueError("accum_steps must be an int in 1 .. 65536, got %r" % (k,))
    return k


def fill_ctl(ctl, base_lr, schedule, max_grad_norm, accum_steps=1):
    """the configuration fields of a _lib.StepCtl"""
    sch = schedule if schedule is not None else StepSchedule()
    ctl.base_lr = base_lr
    ctl.warmup_start, ctl.warmup_steps = sch.warmup_start, sch.warmup_steps
    ctl.decay, ctl.decay_rate, ctl.decay_steps = DECAYS[sch.decay], sch.decay_rate, sch.decay_steps
    ctl.max_norm = max_grad_norm if max_grad_norm is not None else 0.0
    ctl.accum_steps = check_accum_steps(accum_steps)
    return ctl


def check_ema_decay(v):
    """None (no weight averaging) or a decay 0 <= v < 1"""
    if v is None:
        return None
    try:
        if isinstance(v, (bool, str, bytes)):
            raise TypeError
        v = float(v)
    except (TypeError, ValueError):
        raise ValueError("ema_decay must be a number in [0, 1) or None, got %r" % (v,)) from None
    if not (0.0 <= v < 1.0):
        raise ValueError("ema_decay must be in [0, 1) or None, got %r" % (v,))
    return v


def ema_decay_at(decay, warmup, u):
    """float64 mirror of rnvp_ema_update's decay (include/realnvp_hip.h,
    "weight averaging") at the u-th optimizer step, u = 1, 2, ...: with
    warm-up min(decay, (1 + u) / (10 + u)), which reaches 0.999 at u = 8990;
    the average then is e + (1 - d) (p - e)."""
    decay, u = float(decay), int(u)
    return min(decay, (1.0 + u) / (10.0 + u)) if warmup else decay
